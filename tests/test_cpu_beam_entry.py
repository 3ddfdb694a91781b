"""The host side of the two beam-search entry points (w2l_ctc_beam_search, w2l_asg_beam_search; include/w2l_hip.h): what the
workspace queries answer, and that every argument error is refused before anything touches a device, with a message that
names the entry point.  No GPU: the descriptors and buffers are host memory that a refused call never reads through.  (On a
GPU machine the rejection matrix runs with device buffers in tests/test_gpu_lexicon.py and tests/test_gpu_hotwords.py, and is
skipped here, so that a check that regressed can never launch a kernel on host pointers.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from wav2letter_pytorch_amd import asg_beam
from wav2letter_pytorch_amd._lib import LexTables, LmTables, lib
from wav2letter_pytorch_amd.beam_search import _label_info
from wav2letter_pytorch_amd.data.label_sets import english_labels

LABELS = list(english_labels)
N, T, K = 2, 24, 4


def test_ctc_workspace_query():
    q = lib.w2l_ctc_beam_search_workspace_bytes
    plain = q(N, T, K, 0)
    assert plain > 0 and plain % N == 0
    # an LM adds a 64-byte state per trie node, whatever its order; a lexicon and hotwords add nothing (they are no argument)
    assert q(N, T, K, 1) == q(N, T, K, 6) >= plain + N * 64 * (K * T + 1)
    assert q(2 * N, T, K, 0) == 2 * plain and q(2 * N, T, K, 3) == 2 * q(N, T, K, 3)
    for bad in ((0, T, K, 0), (N, 0, K, 0), (N, T, 0, 0), (N, T, 0, 3), (N, T, K, 7), (N, T, K, -1), (N, 1 << 24, 32, 0)):
        assert q(*bad) == -1, bad


def test_asg_workspace_query():
    q = lib.w2l_asg_beam_search_workspace_bytes
    plain = q(N, T, 29, K, 0)
    assert plain > lib.w2l_ctc_beam_search_workspace_bytes(N, T, K, 0)          # 12 bytes per trie node, not 8
    assert q(N, T, 29, K, 1) == q(N, T, 29, K, 6) >= plain + N * 64 * (K * T + 1)
    assert q(1, 8, 64, 64, 0) > 0
    for bad in ((N, T, 65, K, 0), (N, T, 29, 65, 0), (N, T, 29, 0, 0), (N, T, 0, K, 0), (0, T, 29, K, 0), (N, 0, 29, K, 0),
                (N, T, 29, K, 7), (N, T, 29, K, -1), (N, 1 << 24, 29, 1, 0)):
        assert q(*bad) == -1, bad


class _Args:
    """host stand-ins for the buffers of a call, and descriptors that pass every check"""

    def __init__(self):
        self.buf = np.zeros(1 << 16, dtype=np.uint8)             # probs / workspace / out: never read by a refused call
        self.p = C.c_void_p(self.buf.ctypes.data)
        info, self.end = _label_info(LABELS, 0, '>')
        self.info = info | np.array([ch.isspace() << 11 for ch in LABELS], dtype=np.int32)
        self.space = LABELS.index(' ')
        tabbed = LABELS[:-3] + ['\t'] + LABELS[-2:]
        self.info_tab = _label_info(tabbed, 0, '>')[0] | np.array([ch.isspace() << 11 for ch in tabbed], dtype=np.int32)
        self.asg_info = asg_beam._label_info(LABELS, True)
        self.asg_info_tab = asg_beam._label_info(tabbed, True)
        a = self.buf.ctypes.data
        self.lm = LmTables(a, a, a, a, 16, a, a, 16, a, 3, 3, 4)
        self.trie = LexTables(a, a, 16, a, 4)

    def trie_variants(self):
        g = self.trie
        return dict(full=LexTables(g.trie_keys, g.trie_vals, g.trie_cap, g.trie_word, int(g.trie_cap // 2 + 2)),
                    odd_cap=LexTables(g.trie_keys, g.trie_vals, g.trie_cap - 1, g.trie_word, g.n_trie_nodes),
                    no_keys=LexTables(None, g.trie_vals, g.trie_cap, g.trie_word, g.n_trie_nodes),
                    no_word=LexTables(g.trie_keys, g.trie_vals, g.trie_cap, None, g.n_trie_nodes))

    def ctc(self, info=None, space=None, lm=None, order=2, lexicon=None, hotwords=None, weight=0.7, k=K, a=None, blank=0):
        info = self.info if info is None else info
        return lib.w2l_ctc_beam_search(self.p, None, N, T, len(LABELS) if a is None else a, info.ctypes.data_as(C.c_void_p),
                                       blank, self.end, self.space if space is None else space, k, 1.0, 5.0, 1e-3, 0, lm, order,
                                       lexicon, 1, hotwords, weight, self.p, 1 << 16, self.p, None)

    def asg(self, info=None, space=None, lm=None, order=2, k=K, a=None, repeat=0):
        info = self.asg_info if info is None else info
        return lib.w2l_asg_beam_search(self.p, self.p, None, N, T, len(LABELS) if a is None else a,
                                       info.ctypes.data_as(C.c_void_p), repeat, self.space if space is None else space, k, 1.0,
                                       5.0, 1e-3, lm, order, self.p, 1 << 16, self.p, None)


def _refused(rc, entry, *words):
    msg = (lib.w2l_last_error() or b'').decode()
    assert rc != 0 and msg.startswith(entry + ':'), (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason='host pointers: the GPU tests run this matrix on device buffers')


@needs_no_gpu
def test_ctc_entry_refuses_before_any_launch():
    s = _Args()
    name = 'ctc_beam_search'
    lm, good = C.byref(s.lm), C.byref(s.trie)
    for with_lm in (None, lm):
        for what, kw in (('lexicon', 'lexicon'), ('hotword', 'hotwords')):
            other = 'hotwords' if kw == 'lexicon' else 'lexicon'
            for with_other in (None, good):
                for kind, desc in s.trie_variants().items():
                    words = ('NULL',) if kind.startswith('no_') else ('capacity',)
                    _refused(s.ctc(lm=with_lm, **{kw: C.byref(desc), other: with_other}), name, what, *words)
        for tables in (dict(lexicon=good), dict(hotwords=good), dict(lexicon=good, hotwords=good)):
            _refused(s.ctc(info=s.info_tab, space=-1, lm=with_lm, **tables), name, 'whitespace')
            _refused(s.ctc(space=s.space - 1, lm=with_lm, **tables), name, "other than ' '")   # not the index of ' '
            _refused(s.ctc(space=len(LABELS), lm=with_lm, **tables), name, 'space index')
        for weight in (float('inf'), float('-inf'), float('nan')):
            for lexicon in (None, good):
                _refused(s.ctc(lm=with_lm, lexicon=lexicon, hotwords=good, weight=weight), name, 'finite')
    # the LM's own checks, and what an LM alone asks of the labels
    _refused(s.ctc(lm=lm, order=7), name, 'order')
    _refused(s.ctc(lm=lm, order=0), name, 'order')
    _refused(s.ctc(lm=lm, info=s.info_tab, space=-1), name, 'whitespace')
    _refused(s.ctc(lm=lm, space=s.space - 1), name, "other than ' '")
    a = s.buf.ctypes.data
    _refused(s.ctc(lm=C.byref(LmTables(a, None, a, a, 16, a, a, 16, a, 3, 3, 4))), name, 'NULL')
    _refused(s.ctc(lm=C.byref(LmTables(a, a, a, a, 24, a, a, 16, a, 3, 3, 4))), name, 'capacities')
    _refused(s.ctc(lm=C.byref(LmTables(a, a, a, a, 16, a, a, 16, a, 3, 2, 4))), name, 'words')
    # the checks of the search itself, with and without tables
    for tables in (dict(), dict(lm=lm, lexicon=good, hotwords=good)):
        _refused(s.ctc(k=0, **tables), name, 'beam width')
        _refused(s.ctc(k=65, **tables), name, 'beam width')
        _refused(s.ctc(a=129, **tables), name, 'labels')
        _refused(s.ctc(blank=len(LABELS), **tables), name, 'blank')
        bad_canon = s.info.copy()
        bad_canon[3] = (bad_canon[3] & ~0xff) | 5                # a canonical index above the label's own
        _refused(s.ctc(info=bad_canon, **tables), name, 'canonical')
        _refused(lib.w2l_ctc_beam_search(None, None, N, T, len(LABELS), s.info.ctypes.data_as(C.c_void_p), 0, s.end, s.space, K,
                                         1.0, 5.0, 1e-3, 0, tables.get('lm'), 2, tables.get('lexicon'), 1,
                                         tables.get('hotwords'), 0.7, s.p, 1 << 16, s.p, None), name, 'bad arguments')
    # a workspace below the query's answer: that of order 0 without an LM, of the order given with one
    small = lib.w2l_ctc_beam_search_workspace_bytes(N, T, K, 0)
    for tables, size in ((dict(), small - 1), (dict(lexicon=good, hotwords=good), small - 1), (dict(lm=lm), small)):
        _refused(lib.w2l_ctc_beam_search(s.p, None, N, T, len(LABELS), s.info.ctypes.data_as(C.c_void_p), 0, s.end, s.space, K,
                                         1.0, 5.0, 1e-3, 0, tables.get('lm'), 2, tables.get('lexicon'), 1,
                                         tables.get('hotwords'), 0.7, s.p, size, s.p, None), name, 'workspace')


@needs_no_gpu
def test_asg_entry_refuses_before_any_launch():
    s = _Args()
    name = 'asg_beam_search'
    lm = C.byref(s.lm)
    _refused(s.asg(lm=lm, order=7), name, 'order')
    _refused(s.asg(lm=lm, order=0), name, 'order')
    _refused(s.asg(lm=lm, info=s.asg_info_tab, space=-1), name, 'whitespace')
    _refused(s.asg(lm=lm, space=s.space - 1), name, "other than ' '")        # not the index of ' '
    _refused(s.asg(lm=lm, space=len(LABELS)), name, 'space index')
    a = s.buf.ctypes.data
    _refused(s.asg(lm=C.byref(LmTables(a, a, a, a, 16, None, a, 16, a, 3, 3, 4))), name, 'NULL')
    _refused(s.asg(lm=C.byref(LmTables(a, a, a, a, 16, a, a, 17, a, 3, 3, 4))), name, 'capacities')
    _refused(s.asg(lm=C.byref(LmTables(a, a, a, a, 16, a, a, 16, a, 3, 3, 10))), name, 'capacities')
    for with_lm in (None, lm):
        _refused(s.asg(lm=with_lm, k=0), name, 'beam width')
        _refused(s.asg(lm=with_lm, k=65), name, 'beam width')
        _refused(s.asg(lm=with_lm, a=65), name, 'labels')
        _refused(s.asg(lm=with_lm, repeat=len(LABELS)), name, 'repeat_index')
        bad_canon = s.asg_info.copy()
        bad_canon[3] = (bad_canon[3] & ~0xff) | 5
        _refused(s.asg(lm=with_lm, info=bad_canon), name, 'canonical')
        _refused(lib.w2l_asg_beam_search(s.p, None, None, N, T, len(LABELS), s.asg_info.ctypes.data_as(C.c_void_p), 0, s.space, K,
                                         1.0, 5.0, 1e-3, with_lm, 2, s.p, 1 << 16, s.p, None), name, 'bad arguments')
    small = lib.w2l_asg_beam_search_workspace_bytes(N, T, len(LABELS), K, 0)
    for with_lm, size in ((None, small - 1), (lm, small)):
        _refused(lib.w2l_asg_beam_search(s.p, s.p, None, N, T, len(LABELS), s.asg_info.ctypes.data_as(C.c_void_p), 0, s.space, K,
                                         1.0, 5.0, 1e-3, with_lm, 2, s.p, size, s.p, None), name, 'workspace')

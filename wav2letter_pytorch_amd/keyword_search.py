"""CTC keyword search: where in the posteriors is a phrase said, and how well?  Transcribing and searching the text loses
every occurrence the 1-best string gets wrong by one character and gives no score to threshold on; the posteriors hold both.
A keyword is a short CTC target, and the search is forced alignment (alignment.py) with a free start and a free end, for many
keywords at once, scored against the best unconstrained path.  No reference counterpart.

Definition (``keyword_scan_host`` is it in NumPy; csrc/ctc_kws.hip runs it on the MI355X).  For log-probabilities lp [T, A] and
a keyword c_1 .. c_S (no blank among them, 1 <= S <= 255) let b[t] = max_a lp[t, a] and e[t, s] = lp[t, lab(s)] - b[t] <= 0
(exactly 0 where the label is the frame's argmax).  The states are the extended CTC states from the first label to the last:
c_1, blank, c_2, ..., c_S -- 2 S - 1 of them, no leading or trailing blank, so an occurrence begins on the first frame of its
first character and ends on the last frame of its last one (the convention of ctc_forced_align's starts / ends).  Per frame

    D[t][s] = e[t, s] + max(D[t-1][s], D[t-1][s-1], D[t-1][s-2] if skip(s), 0 if s is the first state ("enter here"))

with CTC's skip (label states only, and only where the label differs from the previous label).  A candidate replaces the best
so far on a strict ``>`` only, in the order stay, s-1, s-2, enter, so equal scores give the earliest start.  Beside every D
travels B[t][s], the frame at which the winning path entered (t for "enter", else the winner's B): no back-pointers, no
back-trace.  A state whose best predecessor is -inf stays -inf with B = -1.  Per keyword that gives two curves over time:
``end_score[t] = D[t][last]`` -- the log-likelihood ratio of the best occurrence ending at t to the greedy path over the same
frames, <= 0 and 0 exactly where the greedy path spells the keyword -- and ``end_start[t] = B[t][last]``; from an utterance's
length on they are -inf and -1.

Hits (``pick_hits_host``): up to ``max_hits`` times, among the frames with end_score[t] >= thr whose segment [end_start[t], t]
overlaps no accepted segment of the same keyword, the best by (score descending, start ascending, end descending) is accepted;
the end-descending key makes a clean occurrence, which scores 0 on every frame of its last character, extend to the last of
them.  Hits are reported in start order; different keywords never suppress each other.

This module imports without a GPU: only ``ctc_keyword_search`` (and a KeywordTable's upload) touch the device."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

WIDTHS = (64, 128, 256, 512, 1024)     # block widths of the scan kernel (lanes = extended states)
MAX_LABELS = 255                       # labels per keyword: 509 states, inside a 512-lane block
MAX_KEYWORDS = 4096                    # keywords per w2l_ctc_kws call; a KeywordTable holds more as several chunks
MAX_HITS = 64
MAX_FRAMES = 32768
FIRST, LAST, SKIP, LABEL = 1, 2, 4, 8  # the flag bits of a table's meta words (include/w2l_hip.h, w2l_kws_table_t)
CURVE_BYTES = 1 << 30                  # the curves of one launch stay under this; a larger batch goes in several launches
HIT_DTYPE = np.dtype([('start', np.int32), ('end', np.int32), ('score', np.float32)])


# ---------------------------------------------------------------------------------------------------------------- host model
def _keyword_array(keyword, a: int, blank: int, what: str) -> np.ndarray:
    kw = np.asarray(keyword, dtype=np.int64).reshape(-1)
    if kw.size < 1:
        raise ValueError('%s: an empty keyword' % what)
    if kw.size > MAX_LABELS:
        raise ValueError('%s: a keyword of %d labels (at most %d)' % (what, kw.size, MAX_LABELS))
    if kw.min() < 0 or kw.max() >= a or (kw == blank).any():
        raise ValueError('%s: a keyword label lies outside [0, %d) or equals the blank (%d)' % (what, a, blank))
    return kw


def keyword_scan_host(lp, keyword, blank: int = 0, dtype=np.float64, length: Optional[int] = None):
    """The scan of one keyword over lp [T, A] (log-probabilities; -inf allowed, but every valid frame needs a finite maximum)
    -> (end_score [T] of ``dtype``, end_start int32 [T]); frames from ``length`` on give -inf / -1.  Vectorised over the
    2 S - 1 states, one Python iteration per frame.  With ``dtype=np.float32`` the arithmetic is the kernel's, subtract for
    subtract, add for add and compare for compare."""
    dtype = np.dtype(dtype).type
    lp = np.asarray(lp).astype(dtype, copy=False)
    if lp.ndim != 2 or lp.shape[0] < 1:
        raise ValueError('keyword_scan_host: expected [T >= 1, A] log-probabilities, got shape %s' % (lp.shape,))
    t_all, a = lp.shape
    if not 0 <= blank < a:
        raise ValueError('blank %d outside %d labels' % (blank, a))
    kw = _keyword_array(keyword, a, blank, 'keyword_scan_host')
    t_n = t_all if length is None else min(max(int(length), 0), t_all)
    n_st = 2 * kw.size - 1
    ext = np.full(n_st, blank, dtype=np.int64)
    ext[0::2] = kw
    skip = np.zeros(n_st, dtype=bool)
    skip[2::2] = kw[1:] != kw[:-1]
    ninf = dtype(-np.inf)
    d = np.full(n_st, ninf, dtype=dtype)
    b = np.full(n_st, -1, dtype=np.int64)
    end_score = np.full(t_all, ninf, dtype=dtype)
    end_start = np.full(t_all, -1, dtype=np.int32)
    for t in range(t_n):
        top = lp[t].max()
        if not np.isfinite(top):
            raise ValueError('keyword_scan_host: frame %d has no finite maximum' % t)
        e = lp[t, ext] - top
        best, bb = d.copy(), b.copy()
        a1 = np.concatenate(([ninf], d[:-1]))                  # ties: stay, then s-1, then s-2, then enter
        m = a1 > best
        best[m], bb[m] = a1[m], np.concatenate(([-1], b[:-1]))[m]
        a2 = np.concatenate(([ninf, ninf], d[:-2]))[:n_st]
        a2[~skip] = ninf
        m = a2 > best
        best[m], bb[m] = a2[m], np.concatenate(([-1, -1], b[:-2]))[:n_st][m]
        if 0 > best[0]:
            best[0], bb[0] = 0, t
        d = best + e
        dead = ~(d > ninf)
        d[dead], bb[dead] = ninf, -1
        b = bb
        end_score[t], end_start[t] = d[-1], b[-1]
    return end_score, end_start


def pick_hits_host(end_score, end_start, thr: float, max_hits: int = 8) -> List[tuple]:
    """the hits of one keyword's curves -> [(start, end, score)] in start order (the module docstring has the rule)"""
    if not 1 <= int(max_hits) <= MAX_HITS:
        raise ValueError('max_hits=%r outside 1..%d' % (max_hits, MAX_HITS))
    sc = np.asarray(end_score)
    st = np.asarray(end_start).astype(np.int64)
    ends = np.nonzero((sc >= thr) & (st >= 0))[0]
    free = np.ones(ends.size, dtype=bool)
    hits = []
    for _ in range(int(max_hits)):
        cand = ends[free]
        if not cand.size:
            break
        t = min(cand.tolist(), key=lambda t: (-float(sc[t]), int(st[t]), -t))
        hits.append((int(st[t]), int(t), sc[t].item()))
        free &= (st[ends] > t) | (ends < st[t])
    return sorted(hits)


# ---------------------------------------------------------------------------------------------------------------- the table
def plan_width(states: int) -> int:
    """the narrowest block that holds a keyword of ``states`` extended states"""
    for w in WIDTHS:
        if states <= w:
            return w
    raise ValueError('a keyword of %d states does not fit the widest block (%d)' % (states, WIDTHS[-1]))


def pack_keywords(keywords: Sequence[Sequence[int]], width: Optional[int] = None) -> dict:
    """the block layout of up to MAX_KEYWORDS keywords (label lists) as host arrays: ``width`` (default: the narrowest block
    that holds the longest keyword), ``n_blocks``, ``labels`` / ``meta`` int32 [n_blocks * width] and ``block_kw`` int32
    [n_blocks + 1].  The keywords fill the blocks in the given order; one that does not fit the rest of a block opens the
    next, so none is split."""
    if not 1 <= len(keywords) <= MAX_KEYWORDS:
        raise ValueError('%d keywords for one table chunk (1..%d)' % (len(keywords), MAX_KEYWORDS))
    states = [2 * len(kw) - 1 for kw in keywords]
    need = plan_width(max(states))
    if width is None:
        width = need
    if width not in WIDTHS or width < need:
        raise ValueError('width=%r: one of %s and at least %d for these keywords' % (width, WIDTHS, need))
    labels, meta, block_kw, fill = [], [], [0], 0
    for k, kw in enumerate(keywords):
        if fill + states[k] > width:
            labels += [0] * (width - fill)
            meta += [-1] * (width - fill)
            block_kw.append(k)
            fill = 0
        for s in range(states[k]):
            j = s >> 1
            flags = (FIRST if s == 0 else 0) | (LAST if s == states[k] - 1 else 0)
            if not s & 1:
                flags |= LABEL | (SKIP if j >= 1 and kw[j] != kw[j - 1] else 0)
            labels.append(int(kw[j]) if not s & 1 else 0)
            meta.append(k << 4 | flags)
        fill += states[k]
    labels += [0] * (width - fill)
    meta += [-1] * (width - fill)
    block_kw.append(len(keywords))
    return dict(width=width, n_blocks=len(block_kw) - 1, labels=np.asarray(labels, dtype=np.int32),
                meta=np.asarray(meta, dtype=np.int32), block_kw=np.asarray(block_kw, dtype=np.int32))


class KeywordTable(object):
    """Keywords packed for the scan kernel, built once and reusable across batches and devices.  ``keywords``: label sequences,
    or -- with ``labels`` -- strings (a character maps to its first index in ``labels``, as in ``Decoder.align``; a phrase
    contains the space label).  ValueError: an empty keyword, one longer than 255 labels, a character that is not in
    ``labels``, a blank or a negative label in a keyword.  ``chunks``: the block layouts (``pack_keywords``) of at most 4096
    keywords each, with ``k0`` / ``k1``, the range of keywords a chunk covers; one launch sequence per chunk."""

    def __init__(self, keywords, labels: Optional[Sequence[str]] = None, blank: int = 0, width: Optional[int] = None):
        if isinstance(keywords, str):
            keywords = [keywords]
        keywords = list(keywords)
        if keywords and isinstance(keywords[0], (int, np.integer)):      # one keyword's labels
            keywords = [keywords]
        if not keywords:
            raise ValueError('KeywordTable: no keywords')
        first = None
        if labels is not None:
            first = {}
            for i, ch in enumerate(labels):
                first.setdefault(ch, i)
        self.blank = int(blank)
        self.n_labels = None if labels is None else len(labels)
        self.texts, self.keywords = [], []
        for kw in keywords:
            if isinstance(kw, str):
                if first is None:
                    raise ValueError('KeywordTable: string keywords need ``labels``')
                try:
                    row = [first[ch] for ch in kw]
                except KeyError as e:
                    raise ValueError('KeywordTable: character %r of %r is not in the labels' % (e.args[0], kw)) from None
                self.texts.append(kw)
            else:
                row = [int(v) for v in (kw.tolist() if hasattr(kw, 'tolist') else kw)]
                self.texts.append(None)
            if not row:
                raise ValueError('KeywordTable: keyword %d is empty' % len(self.keywords))
            if len(row) > MAX_LABELS:
                raise ValueError('KeywordTable: keyword %d has %d labels (at most %d)' % (len(self.keywords), len(row), MAX_LABELS))
            if self.blank in row:
                raise ValueError('KeywordTable: keyword %d contains the blank (%d)' % (len(self.keywords), self.blank))
            if min(row) < 0 or self.n_labels is not None and max(row) >= self.n_labels:
                raise ValueError('KeywordTable: keyword %d has a label outside [0, %s)' % (len(self.keywords), self.n_labels))
            self.keywords.append(tuple(row))
        self.lengths = np.asarray([len(kw) for kw in self.keywords], dtype=np.int32)
        self.max_label = max(max(kw) for kw in self.keywords)
        self.chunks = []
        for k0 in range(0, len(self.keywords), MAX_KEYWORDS):
            chunk = pack_keywords(self.keywords[k0: k0 + MAX_KEYWORDS], width)
            chunk.update(k0=k0, k1=min(k0 + MAX_KEYWORDS, len(self.keywords)))
            self.chunks.append(chunk)
        self._device = {}

    def __len__(self):
        return len(self.keywords)

    def __repr__(self):
        return 'KeywordTable(%d keywords, %s)' % (len(self), ', '.join('%d x %d' % (c['n_blocks'], c['width']) for c in self.chunks))

    def on_device(self, index: int, device):
        """chunk ``index`` on ``device`` (uploaded once per device) -> (the tensor that owns the memory, _lib.KwsTable)"""
        import torch
        from ._lib import KwsTable
        key = (index, str(device))
        if key not in self._device:
            c = self.chunks[index]
            buf = torch.from_numpy(np.concatenate([c['labels'], c['meta'], c['block_kw']])).to(device)
            lanes = c['n_blocks'] * c['width']
            t = KwsTable(labels=buf.data_ptr(), meta=buf.data_ptr() + 4 * lanes, block_kw=buf.data_ptr() + 8 * lanes,
                         n_blocks=c['n_blocks'], width=c['width'], n_keywords=c['k1'] - c['k0'], reserved_=0)
            self._device[key] = (buf, t)
        return self._device[key]


# ---------------------------------------------------------------------------------------------------------------- the device
def kws_sections(n: int, k: int, max_hits: int):
    """byte offsets (status, hit_count, hits, total) of w2l_ctc_kws's small outputs inside one buffer"""
    o_count = 4 * n
    o_hits = o_count + 4 * n * k
    return 0, o_count, o_hits, o_hits + HIT_DTYPE.itemsize * n * k * max_hits


def launch_kws(x, sz, table, thr, max_hits: int, blank: int, log_probs: bool, small, score, start, phases: int = 7, ws=None):
    """one w2l_ctc_kws call on the current stream: x [N, T, A] float32 contiguous on the device, ``sz`` int32 [N] there or
    None, ``table`` a _lib.KwsTable, ``thr`` float32 [K] on the device, the small outputs into ``small`` (uint8, kws_sections'
    layout) and the curves into ``score`` / ``start`` [N, K, T].  -> the workspace tensor: keep it until the stream has passed."""
    import torch
    from . import _lib
    from ._lib import check, lib, ptr, stream_ptr
    n, t, a = x.shape
    k = table.n_keywords
    ws_bytes = int(lib.w2l_ctc_kws_workspace_bytes(n, t, k, int(max_hits)))
    if ws_bytes < 0:
        raise _lib.W2LError('ctc_keyword_search: N=%d (max 65535), T=%d (max %d), %d keywords (max %d) or max_hits=%d (1..%d) is '
                            'out of range' % (n, t, MAX_FRAMES, k, MAX_KEYWORDS, max_hits, MAX_HITS))
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    vp = C.c_void_p
    o = kws_sections(n, k, int(max_hits))
    base = small.data_ptr()
    check(lib.w2l_ctc_kws(ptr(x), ptr(sz), n, t, a, int(blank), int(bool(log_probs)), C.byref(table), ptr(thr), int(max_hits),
                          int(phases), ptr(ws), ws_bytes, ptr(score), ptr(start), vp(base + o[1]), vp(base + o[2]), vp(base + o[0]),
                          stream_ptr()), 'w2l_ctc_kws')
    return ws


def ctc_keyword_search(probs, keywords, input_lengths=None, blank: int = 0, log_probs: bool = False,
                       labels: Optional[Sequence[str]] = None, threshold: float = -1.0, max_hits: int = 8,
                       return_curves: bool = False):
    """Find keywords in the posteriors of a batch on the MI355X (three launches per 4096 keywords: frame maxima, scan, pick).

    probs: [N, T, A] or [T, A] (numpy or torch; probabilities, or log-probabilities with ``log_probs``); keywords: label
    sequences, strings with ``labels`` (a character maps to its first index, as in ``Decoder.align``; phrases contain the space
    label), or a ``KeywordTable`` (built once, reusable across batches); input_lengths[n]: the frames of utterance n in [0, T]
    (default: all T).  ``threshold`` is in nats per label: keyword k is reported where its score is at least ``threshold * S_k``.
    The default of -1.0 is a convention, not a tuned value.  ``max_hits`` (1..64): the most hits per keyword and utterance.

    Returns, per utterance, a list of ``(keyword index, start frame, end frame, score)`` on the host, ordered by start frame;
    with ``return_curves`` also ``end_score`` float32 and ``end_start`` int32, both [N, K, T].  ValueError before any launch: an
    empty keyword, one longer than 255 labels, a character not in ``labels``, a blank or a label outside [0, A) in a keyword,
    ``max_hits`` outside 1..64; and after the launches: a NaN, a negative probability or a frame without a finite maximum,
    naming the utterances."""
    import torch
    from .alignment import batch_of, on_device
    if not 1 <= int(max_hits) <= MAX_HITS:
        raise ValueError('ctc_keyword_search: max_hits=%r outside 1..%d' % (max_hits, MAX_HITS))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError('ctc_keyword_search: threshold is NaN')
    x, input_lengths, _ = batch_of(probs, input_lengths)
    if x.dim() != 3:
        raise ValueError('expected [N, T, labels] or [T, labels] posteriors, got shape %s' % (tuple(x.shape),))
    n, t, a = x.shape
    if n < 1 or t < 1 or a < 1:
        raise ValueError('ctc_keyword_search: empty posteriors, shape %s' % (tuple(x.shape),))
    if t > MAX_FRAMES:
        raise ValueError('ctc_keyword_search: T=%d (max %d) is out of range' % (t, MAX_FRAMES))
    if labels is not None and len(labels) != a:
        raise ValueError('ctc size:%d, labels: %d' % (a, len(labels)))
    if not 0 <= blank < a:
        raise ValueError('blank %d outside %d labels' % (blank, a))
    table = keywords if isinstance(keywords, KeywordTable) else KeywordTable(keywords, labels=labels, blank=blank)
    if table.blank != blank:
        raise ValueError('ctc_keyword_search: the KeywordTable was built for blank %d, not %d' % (table.blank, blank))
    if table.max_label >= a:
        raise ValueError('ctc_keyword_search: a keyword label lies outside [0, %d)' % a)
    il = None
    if input_lengths is not None:
        il = torch.as_tensor(input_lengths).detach().cpu().to(torch.int64).reshape(-1)
        if il.numel() != n:
            raise ValueError('input_lengths holds %d lengths for %d utterances' % (il.numel(), n))
        if bool((il < 0).any()) or bool((il > t).any()):
            raise ValueError('input_lengths must lie in [0, %d], got %s' % (t, il.tolist()))
        il = il.to(torch.int32)
    x = on_device(x, 'ctc_keyword_search', '; keyword_scan_host is the host model')
    k_all = len(table)
    found = [[] for _ in range(n)]
    if return_curves:
        all_score = np.empty((n, k_all, t), dtype=np.float32)
        all_start = np.empty((n, k_all, t), dtype=np.int32)
    with torch.cuda.device(x.device):
        sz_all = il.to(x.device) if il is not None else None
        for ci, chunk in enumerate(table.chunks):
            k0, k = chunk['k0'], chunk['k1'] - chunk['k0']
            _, dev_table = table.on_device(ci, x.device)
            thr = torch.from_numpy((np.float32(threshold) * table.lengths[k0: k0 + k].astype(np.float32))).to(x.device)
            rows = max(1, min(n, CURVE_BYTES // (8 * k * t)))
            for n0 in range(0, n, rows):
                n1 = min(n, n0 + rows)
                m = n1 - n0
                o = kws_sections(m, k, int(max_hits))
                small = torch.empty(o[3], dtype=torch.uint8, device=x.device)
                score = torch.empty(m, k, t, dtype=torch.float32, device=x.device)
                start = torch.empty(m, k, t, dtype=torch.int32, device=x.device)
                ws = launch_kws(x[n0:n1], None if sz_all is None else sz_all[n0:n1], dev_table, thr, max_hits, blank, log_probs,
                                small, score, start)
                host = small.cpu().numpy()
                del ws
                status = host[o[0]:o[1]].view(np.int32)
                if (status != 0).any():
                    raise ValueError('ctc_keyword_search: a NaN, a negative probability or a frame without a finite maximum (or a '
                                     'keyword label outside [0, %d) or equal to the blank, %d) in utterances %s'
                                     % (a, blank, (n0 + np.nonzero(status != 0)[0]).tolist()))
                count = host[o[1]:o[2]].view(np.int32).reshape(m, k)
                hits = host[o[2]:o[3]].view(HIT_DTYPE).reshape(m, k, int(max_hits))
                for i, j in zip(*np.nonzero(count)):
                    for h in hits[i, j, :count[i, j]]:
                        found[n0 + i].append((k0 + int(j), int(h['start']), int(h['end']), float(h['score'])))
                if return_curves:
                    all_score[n0:n1, k0: k0 + k] = score.cpu().numpy()
                    all_start[n0:n1, k0: k0 + k] = start.cpu().numpy()
    found = [sorted(f, key=lambda h: (h[1], h[2], h[0])) for f in found]
    return (found, all_score, all_start) if return_curves else found

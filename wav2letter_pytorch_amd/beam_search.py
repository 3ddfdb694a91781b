"""CTC prefix beam search with an optional language model (reference: decoder.py:147-267, itself after
Hannun et al. 2014 / corticph prefix-beam-search) -- an inference-side, host-only decoder.

Each hypothesis (prefix string) carries two masses per time step: ending in blank (``pb``) and ending in a
non-blank (``pnb``).  The reference's observable behaviour that callers rely on is kept: probabilities (not
logs) in, the first index of a label wins on duplicates, an ``end_char`` freezes a prefix, the LM is applied
when a word is closed (space or end char) with weight ``alpha``, ranking multiplies by (#words+1)**beta, only
strictly positive masses survive a step, ties keep first-seen order.

prefix_beam_search_gpu / GPUPrefixBeamSearchDecoder run the same recursion without a language model as one HIP launch per
batch (w2l_ctc_beam_search, csrc/beam_search.hip), in fp64 logs; with an ARPA n-gram model (ngram_lm.ArpaLM: ``lm=`` of
prefix_beam_search_gpu, GPUPrefixBeamSearchLMDecoder) the same launch scores words on the device (w2l_ctc_beam_search with lm)
as the host does with ``lm=lambda s: 10 ** arpa.score(s)``.  With ``return_offsets`` a second launch on the same stream
(w2l_ctc_align, alignment.py) aligns each best prefix to the posteriors where it lies in the search's device buffer, and the
character offsets come back in the same copy.  ``lexicon=`` confines the searches to a word list (lexicon.py); ``hotwords=`` /
``hotword_weight=`` make them prefer a list of words without forbidding anything else: the ranking weight of a string gains
``exp(hotword_weight * h)``, ``h`` = Lexicon.boost_chars (w2l_ctc_beam_search with hotwords; host and device state the same rule).
``mbr='word'|'char'`` returns, instead of the string of the greatest weight, the one of the least expected word / character
error under the n-best list's own posterior (mbr.py; w2l_nbest_mbr reads the list in the search's buffer, on the same stream)."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from collections import namedtuple
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .alignment import align_sections, launch_align, split_align
from .decoder import Decoder
from .mbr import check_mbr, check_mbr_status, launch_mbr, mbr_offset, mbr_rows, mbr_sections, split_mbr

_WORD_RE = re.compile(r'\w+[\s|>]')


def _n_words(prefix: str) -> int:
    return len(_WORD_RE.findall(prefix))


class _Step:
    """masses of one time step, remembering first-insertion order of prefixes (pb first, then pnb)"""

    def __init__(self):
        self.pb: Dict[str, float] = {}
        self.pnb: Dict[str, float] = {}

    def add_b(self, prefix, v):
        self.pb[prefix] = self.pb.get(prefix, 0.0) + v

    def add_nb(self, prefix, v):
        self.pnb[prefix] = self.pnb.get(prefix, 0.0) + v

    def total(self) -> Dict[str, float]:
        """pb + pnb keeping only positive sums (collections.Counter addition semantics)"""
        out: Dict[str, float] = {}
        for src in (self.pb, self.pnb):
            for k in src:
                if k not in out:
                    s = self.pb.get(k, 0.0) + self.pnb.get(k, 0.0)
                    if s > 0:
                        out[k] = s
        return out


def prefix_beam_search(ctc, labels: Sequence[str], blank_index: int = 0, lm: Optional[Callable[[str], float]] = None,
                       k: int = 5, alpha: float = 0.3, beta: float = 5, prune: float = 0.001, end_char: str = '>',
                       return_weights: bool = False, lexicon=None, complete_only: bool = True,
                       stats: Optional[dict] = None, hotwords=None, hotword_weight: float = 0.0):
    """ctc: [timesteps, alphabet] probabilities.  Returns the best prefix (and its ranking weight).

    ``lexicon`` (a lexicon.Lexicon; None: no constraint): an extension ``pre + ch`` that is not legal (Lexicon.allows) gets no
    mass -- not the ``p * (pb + pnb)`` term, not the two terms of an extension that fell off the beam; the repeat branch's
    contribution to ``pre`` itself stays.  With ``complete_only`` the result is the best beam member whose trailing partial word
    is empty or a whole word (Lexicon.complete); if the final beam holds none, the best member as it is.  Weights are the
    members' own, not renormalised.

    ``hotwords`` (a lexicon.Lexicon, a path to a word list or an iterable of single words; None: no boosting): the ranking
    weight of a string ``s``, in every frame and as returned, gets the factor ``exp(hotword_weight * h(s))``, ``h`` =
    Lexicon.boost_chars of the words the labels can spell.  Masses, the LM weight, the prune and ties are untouched.

    ``stats`` (a dict): ``frames`` and ``live`` (the candidates with a positive mass, summed over the frames) are added to it,
    and ``beam`` is set to the final beam, best first, ``weights`` to its members' ranking weights."""
    ctc = np.asarray(ctc)
    assert ctc.shape[1] == len(labels), "ctc size:%d, labels: %d" % (ctc.shape[1], len(labels))
    assert ctc.shape[0] > 1, "ctc length: %d was too short" % ctc.shape[0]
    assert (ctc >= 0).all(), 'ctc output contains negative numbers'
    score_lm = lm if lm is not None else (lambda _s: 1)
    labels = list(labels)
    first_index = {}
    for i, ch in enumerate(labels):
        first_index.setdefault(ch, i)
    blank = labels[blank_index]
    legal: Dict[str, bool] = {}
    if hotwords is None:
        def weight(s):
            return ranked.get(s, 0) * (_n_words(s) + 1) ** beta
    else:
        hot = _resolve_hotwords(hotwords).spellable(labels, blank_index)
        gamma = float(hotword_weight)
        if not math.isfinite(gamma):
            raise ValueError('hotword_weight must be finite, got %r' % (hotword_weight,))

        def weight(s):
            return ranked.get(s, 0) * (_n_words(s) + 1) ** beta * math.exp(gamma * hot.boost_chars(s, end_char))

    def allowed(ext):
        if ext not in legal:
            legal[ext] = lexicon.allows(ext, end_char)
        return legal[ext]

    prev = _Step()
    prev.pb[''] = 1.0
    prev.pnb[''] = 0.0
    beam: List[str] = ['']
    ranked: Dict[str, float] = {}
    for t in range(ctc.shape[0]):
        frame = ctc[t]
        cur = _Step()
        alphabet = [labels[i] for i in np.where(frame > prune)[0]]
        in_beam = set(beam)
        for pre in beam:
            pb_prev, pnb_prev = prev.pb.get(pre, 0.0), prev.pnb.get(pre, 0.0)
            if pre and pre[-1] == end_char:             # a closed hypothesis is carried unchanged
                cur.pb[pre] = pb_prev
                cur.pnb[pre] = pnb_prev
                continue
            for ch in alphabet:
                p = frame[first_index[ch]]
                if ch == blank:
                    cur.add_b(pre, frame[blank_index] * (pb_prev + pnb_prev))
                    continue
                ext = pre + ch
                if lexicon is not None and not allowed(ext):     # the extension leaves the word list: no mass for it
                    if pre and ch == pre[-1]:
                        cur.add_nb(pre, p * pnb_prev)
                    continue
                if pre and ch == pre[-1]:                # repeated character: only a blank separates two copies
                    cur.add_nb(ext, p * pb_prev)
                    cur.add_nb(pre, p * pnb_prev)
                elif pre.replace(' ', '') and ch in (' ', end_char):   # a word closes: language-model weight
                    w = score_lm(ext.strip(' ' + end_char)) ** alpha
                    cur.add_nb(ext, w * p * (pb_prev + pnb_prev))
                else:
                    cur.add_nb(ext, p * (pb_prev + pnb_prev))
                if ext not in in_beam:                   # mass of an extension that fell off the beam earlier
                    cur.add_b(ext, frame[blank_index] * (prev.pb.get(ext, 0.0) + prev.pnb.get(ext, 0.0)))
                    cur.add_nb(ext, p * prev.pnb.get(ext, 0.0))
        ranked = cur.total()
        if stats is not None:
            stats['frames'] = stats.get('frames', 0) + 1
            stats['live'] = stats.get('live', 0) + len(ranked)
        order = sorted(ranked, key=weight, reverse=True)   # stable
        beam = order[:k]
        prev = cur
    if not beam:
        beam = ['']
    if stats is not None:
        stats['beam'] = list(beam)                       # the final beam in rank order (before complete_only)
        stats['weights'] = [weight(s) for s in beam]     # and the members' ranking weights: the n-best list mbr.py reads
    if lexicon is not None and complete_only:
        beam = [s for s in beam if lexicon.complete(s, end_char)] or beam
    best = beam[0]
    if return_weights:
        return best, weight(best)
    return best


class PrefixBeamSearchLMDecoder(Decoder):
    """decoder.py:232-267: wraps prefix_beam_search; ``lm_path`` selects a kenlm model (optional dependency)."""

    def __init__(self, lm_path, labels, blank_index=0, k=5, alpha=0.3, beta=5, prune=1e-3):
        super(PrefixBeamSearchLMDecoder, self).__init__(labels, blank_index)
        if lm_path:
            import kenlm  # noqa: F401  (not shipped with this repo; raises ImportError if absent)
            self.lm = kenlm.Model(lm_path)
            self.lm_weigh = lambda f: 10 ** (self.lm.score(f))
        else:
            self.lm_weigh = lambda s: 1
        self.k, self.alpha, self.beta, self.prune = k, alpha, beta, prune

    def decode(self, probs, sizes=None, return_offsets=False):
        if return_offsets:
            raise NotImplementedError("Prefix beam search does not support offsets (yet).")
        if hasattr(probs, 'detach'):
            probs = probs.detach().cpu().numpy()
        if len(probs.shape) == 2:
            return prefix_beam_search(probs, self.labels, self.blank_index, self.lm_weigh, self.k, self.alpha, self.beta,
                                      self.prune)
        if len(probs.shape) == 3:
            return [self.decode(p) for p in probs]
        raise RuntimeError('Decoding with wrong shape: %s, expected either [Batch X Frames X Labels] or '
                           '[Frames X Labels]' % str(probs.shape))


# ---------------------------------------------------------------------------------------------------------------- device
_SEP_RE = re.compile(r'[\s|>]')
_WORDCH_RE = re.compile(r'\w')


def word_flags(ch: str) -> int:
    """the label-info bits both searches share: 9 = a word character (\\w), 10 = a word separator ([\\s|>])"""
    return bool(_WORDCH_RE.fullmatch(ch)) << 9 | bool(_SEP_RE.fullmatch(ch)) << 10


def _label_info(labels: Sequence[str], blank_index: int, end_char: str):
    """per-label flags of w2l_ctc_beam_search (include/w2l_hip.h) and the first index of ``end_char`` (-1: absent)"""
    labels = list(labels)
    if not all(isinstance(ch, str) and len(ch) == 1 for ch in labels):
        raise ValueError('prefix_beam_search_gpu: every label must be one character')
    first_index = {}
    for i, ch in enumerate(labels):
        first_index.setdefault(ch, i)
    blank = labels[blank_index]
    info = np.array([first_index[ch] | (ch == blank) << 8 | word_flags(ch) for ch in labels], dtype=np.int32)
    return info, first_index.get(end_char, -1)


def _align_best(x, sz, out, lay, t, blank_index, log_probs):
    """w2l_ctc_align right behind the search on the same stream: rank 0 of every utterance, read in ``out`` where the search
    wrote it (``lay``: search_out_layout; an empty slot's -1 aligns as the empty string), results behind the search's bytes"""
    return launch_align(x, sz, out.data_ptr() + lay.labels, lay.labels_stride, out.data_ptr() + lay.lengths, lay.lengths_stride,
                        t, blank_index, log_probs, out, lay.beam_bytes)


def _align_starts(host, n, t, beam_bytes):
    """starts [N, T] of _align_best from the host copy of the buffer"""
    _, status, _, starts, _ = split_align(host[beam_bytes:], n, t, t)
    if status.any():
        raise _lib.W2LError('w2l_ctc_align found no path for the decoded prefix of utterances %s (status %s)'
                            % (np.nonzero(status)[0].tolist(), status[status != 0].tolist()))
    return starts


def _resolve_lexicon(lexicon, lm):
    """a Lexicon from ``lexicon``: a Lexicon, a path, or 'lm' (the vocabulary of the ArpaLM ``lm``, cached on it)"""
    from .lexicon import Lexicon
    if isinstance(lexicon, Lexicon):
        return lexicon
    if isinstance(lexicon, str) and lexicon == 'lm':
        if lm is None:
            raise ValueError("lexicon='lm' needs a language model (lm=)")
        if getattr(lm, '_lexicon', None) is None:
            lm._lexicon = Lexicon.from_lm(lm)
        return lm._lexicon
    if isinstance(lexicon, (str, os.PathLike)):
        return Lexicon(lexicon)
    raise TypeError("lexicon must be a lexicon.Lexicon, a path or 'lm', got %s" % type(lexicon).__name__)


def _resolve_hotwords(hotwords):
    """a Lexicon holding the hotword list ``hotwords``: a Lexicon, a path to a word list, or an iterable of single words (an
    entry with whitespace is a ValueError)"""
    from .lexicon import Lexicon
    return hotwords if isinstance(hotwords, Lexicon) else Lexicon(hotwords)


SearchOutLayout = namedtuple('SearchOutLayout', 'beam_bytes labels labels_stride lengths lengths_stride')


def search_out_layout(n, k, t, with_lm):
    """a beam search's ``out`` buffer (include/w2l_hip.h): scores float64 [n, k] | lengths int32 [n, k] | status int32 [n] |
    labels int32 [n, k, t] | with an LM lm_log10 float32 [n, k].  -> its size, and for an alignment that reads rank 0 of every
    utterance in place the byte offset and the stride (elements, one utterance to the next) of its labels and of its length"""
    return SearchOutLayout(12 * n * k + 4 * n + 4 * n * k * t + (4 * n * k if with_lm else 0), 12 * n * k + 4 * n, k * t,
                           8 * n * k, k)


def split_search_out(host, n, k, t, with_lm):
    """the sections of a beam search's ``out`` buffer (include/w2l_hip.h; ``host``: its bytes on the host, anything after them
    ignored) -> scores float64 [n, k], lengths int32 [n, k], status int32 [n], labels int32 [n, k, t], lm_log10 float32 [n, k]
    (None unless ``with_lm``)"""
    scores = host[:8 * n * k].view(np.float64).reshape(n, k)
    rest = host[8 * n * k:search_out_layout(n, k, t, with_lm).beam_bytes].view(np.int32)
    lengths = rest[:n * k].reshape(n, k)
    status = rest[n * k:n * k + n]
    idx = rest[n * k + n:n * k + n + n * k * t].reshape(n, k, t)
    lm_log10 = rest[n * k + n + n * k * t:].view(np.float32).reshape(n, k) if with_lm else None
    return scores, lengths, status, idx, lm_log10


def _word_tables(labels, silent_index, lm, lexicon, hotwords, hotword_weight, dev, what):
    """the device tables of a search's LM, lexicon and hotword list, checked as both searches check them.  ``silent_index``: the
    label that spells nothing (the blank; under ASG the repeat label); ``what``: the caller's name in the messages.
    -> (LM tables, lexicon table, hotword table -- None where there is none --, the space's index or -1, the LM order or 0)"""
    if lm is None and lexicon is None and hotwords is None:
        return None, None, None, -1, 0
    from .ngram_lm import ArpaLM
    if lm is not None and not isinstance(lm, ArpaLM):
        raise TypeError('lm must be an ngram_lm.ArpaLM, got %s' % type(lm).__name__)
    odd = [ch for ch in labels if ch.isspace() and ch != ' ']
    if odd:
        raise ValueError('%s: whitespace labels other than a space (%r) cannot %s'
                         % (what, odd, 'be scored by a word LM' if lm is not None else
                            'separate the words of a lexicon or of a hotword list'))
    if hotwords is not None and not math.isfinite(float(hotword_weight)):
        raise ValueError('%s: hotword_weight must be finite, got %r' % (what, hotword_weight))
    tables = lm.to_device(labels, silent_index, dev) if lm is not None else None
    lex = _resolve_lexicon(lexicon, lm).to_device(labels, silent_index, dev) if lexicon is not None else None
    hot = _resolve_hotwords(hotwords).to_device(labels, silent_index, dev) if hotwords is not None else None
    return tables, lex, hot, labels.index(' ') if ' ' in labels else -1, lm.order if lm is not None else 0


def _desc(table):
    """a device table as the entry points take it (None: NULL)"""
    return table.desc_ref if table is not None else None


def _pick(found, nbest, return_weights, return_encoded=False):
    """n-best rows (text, weight[, encoded]), best first -> one utterance's result: the best text; (text, weight) with
    ``return_weights``; with ``nbest > 1`` a list of up to ``nbest`` such pairs.  ``return_encoded`` keeps the rows whole."""
    rows = [row if return_encoded else row[:2] for row in found]
    if nbest > 1:
        return rows[:nbest]
    if return_weights or return_encoded:
        return rows[0]
    return rows[0][0]


def _check_decode_shape(probs):
    if len(probs.shape) not in (2, 3):
        raise RuntimeError('Decoding with wrong shape: %s, expected either [Batch X Frames X Labels] or '
                           '[Frames X Labels]' % str(tuple(probs.shape)))


def _beam_search_device(probs, labels, blank_index, k, beta, prune, end_char, sizes, log_probs, lm=None, alpha=0.3,
                        offsets=False, lexicon=None, complete_only=True, hotwords=None, hotword_weight=0.0, mbr=None,
                        mbr_scale=1.0):
    """one launch of w2l_ctc_beam_search for probs [N, T, A] on the current stream; returns the host arrays
    (scores [N, k], lengths [N, k], labels [N, k, T]).  With ``lm`` (an ngram_lm.ArpaLM) a fourth array: lm_log10 [N, k]
    float32, the LM total of each result.  With ``offsets`` a launch of w2l_ctc_align follows and one more array: starts
    int32 [N, T], the first frame of each label of rank 0.  ``lexicon`` (a lexicon.Lexicon, or 'lm': the vocabulary of ``lm``)
    and ``hotwords`` (see _resolve_hotwords) are the entry point's other two tables; a table that is None is passed as NULL.
    With ``mbr`` ('word' or 'char') w2l_nbest_mbr follows the search, ``offsets`` aligns ITS pick (the section's pick_labels)
    instead of rank 0, and the last array is followed by one more element, the mbr.MbrResult."""
    if probs.dim() != 3:
        raise ValueError('expected [N, T, labels] or [T, labels] posteriors, got shape %s' % (tuple(probs.shape),))
    n, t, a = probs.shape
    if a != len(labels):
        raise ValueError('ctc size:%d, labels: %d' % (a, len(labels)))
    if not 0 <= blank_index < a:
        raise ValueError('blank_index %d outside %d labels' % (blank_index, a))
    if t < 2:
        raise ValueError('ctc length: %d was too short' % t)
    if offsets and t > 4095:
        raise ValueError('return_offsets: %d frames, w2l_ctc_align takes targets of at most 4095 labels' % t)
    info, end_index = _label_info(labels, blank_index, end_char)
    if not probs.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.W2LError('prefix_beam_search_gpu needs the MI355X device (there is no CPU fallback)')
        probs = probs.cuda()
    x = probs.detach().float().contiguous()
    dev = x.device
    sz = None
    if sizes is not None:
        host = torch.as_tensor(sizes).detach().cpu().to(torch.int64).reshape(-1)
        if host.numel() != n:
            raise ValueError('sizes holds %d lengths for %d utterances' % (host.numel(), n))
        if bool((host < 2).any()) or bool((host > t).any()):
            raise ValueError('sizes must lie in [2, %d], got %s' % (t, host.tolist()))
        sz = host.to(torch.int32).to(dev, non_blocking=True)
    tables, lex, hot, space_index, order = _word_tables(labels, blank_index, lm, lexicon, hotwords, hotword_weight, dev,
                                                        'prefix_beam_search_gpu')
    if lm is not None or lexicon is not None or hotwords is not None:
        info = info | np.array([ch.isspace() << 11 for ch in labels], dtype=np.int32)
    ws_bytes = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, order))
    if ws_bytes < 0:
        raise ValueError('prefix_beam_search_gpu: k=%d with T=%d%s is out of range'
                         % (k, t, '' if lm is None else ' (LM order %d)' % lm.order))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    lay = search_out_layout(n, k, t, lm is not None)
    mbr_at = mbr_offset(lay.beam_bytes)
    align_at = mbr_at + mbr_sections(n, k, t).total if mbr else lay.beam_bytes
    out = torch.empty(align_at + (align_sections(n, t, t)[5] if offsets else 0), dtype=torch.uint8, device=dev)
    check(lib.w2l_ctc_beam_search(ptr(x), ptr(sz), n, t, a, info.ctypes.data_as(C.c_void_p), int(blank_index), int(end_index),
                                  space_index, int(k), float(alpha), float(beta), float(prune), int(bool(log_probs)),
                                  _desc(tables), order, _desc(lex), int(bool(complete_only)), _desc(hot),
                                  float(hotword_weight), ptr(ws), ws_bytes, ptr(out), stream_ptr()), 'w2l_ctc_beam_search')
    mbr_ws = launch_mbr(out, mbr_at, n, k, t, labels, mbr, -1, mbr_scale) if mbr else None
    align_ws = None
    if offsets and mbr:                                # the pick, where w2l_nbest_mbr copied it: rows of stride T
        sec = mbr_sections(n, k, t)
        align_ws = launch_align(x, sz, out.data_ptr() + mbr_at + sec.pick_labels, t, out.data_ptr() + mbr_at + sec.pick_len, 1,
                                t, blank_index, log_probs, out, align_at)
    elif offsets:
        align_ws = _align_best(x, sz, out, lay, t, blank_index, log_probs)
    host = out.cpu().numpy()                           # the one copy to the host (ordered after the launches on this stream)
    del align_ws, mbr_ws
    scores, lengths, status, idx, lm_log10 = split_search_out(host, n, k, t, lm is not None)
    if status.any():
        raise ValueError('ctc output contains negative numbers (utterances %s)' % np.nonzero(status)[0].tolist())
    got = (scores, lengths, idx)
    if lm is not None:
        got += (lm_log10,)
    if offsets:
        got += (_align_starts(host, n, t, align_at),)
    if mbr:
        got += (split_mbr(host[mbr_at:], n, k, t),)
    return got


def prefix_beam_search_gpu(probs, labels: Sequence[str], blank_index: int = 0, k: int = 5, beta: float = 5,
                           prune: float = 0.001, end_char: str = '>', sizes=None, log_probs: bool = False, nbest: int = 1,
                           return_weights: bool = False, lm=None, alpha: float = 0.3, return_offsets: bool = False,
                           lexicon=None, complete_only: bool = True, hotwords=None, hotword_weight: float = 1.0, mbr=None,
                           mbr_scale: float = 1.0, return_risks: bool = False):
    """prefix_beam_search on the MI355X: one launch for a whole batch, masses as fp64 logs (no underflow on long
    utterances; the host function's float32 products do underflow), the host's candidate order and ties.  ``lm``: an
    ngram_lm.ArpaLM scored as the host's ``lm=lambda s: 10 ** lm.score(s)`` with weight ``alpha`` (None: no LM).

    probs: [T, labels] or [N, T, labels] (numpy or torch, any device; probabilities, or log-probabilities if ``log_probs``);
    ``sizes[n]``: decode only the first sizes[n] frames of utterance n (default: all T).  Per utterance the result is the best
    prefix, ``(best, log weight)`` if ``return_weights``, or if ``nbest > 1`` a list of up to ``nbest`` ``(prefix, log weight)``
    pairs, best first (log weight = log(mass * (words + 1) ** beta), the host's ranking weight).  A [T, labels] input gives one
    result, a batch a list of N.  ``return_offsets`` (only with ``nbest == 1``): ``(results, offsets)``, offsets an IntTensor
    per utterance holding the first frame of each character of its best prefix on that prefix's best frame path (one more
    launch, w2l_ctc_align, on the same stream; still one copy to the host).

    ``lexicon`` (a lexicon.Lexicon, a path to a word list, or 'lm': the vocabulary of ``lm``; None: no constraint): no mass
    goes to a string with a word outside the lexicon, as in prefix_beam_search(lexicon=...), with or without ``lm``.  With
    ``complete_only`` the results (best, n-best, offsets) are drawn from the members of the final beam whose trailing partial
    word is empty or a whole word, in rank order with their own weights; if there is none, from the whole beam.  Labels that
    are whitespace other than a space are an error with a lexicon, as with an LM.

    ``hotwords`` (a lexicon.Lexicon, a path to a word list, or an iterable of single words; None: no boosting) with
    ``hotword_weight`` (natural-log units per matched character, any finite real; the default of 1.0 is a convention, not a
    tuned value): the ranking weight gets the factor ``exp(hotword_weight * h)``, ``h`` = Lexicon.boost_chars of the string
    -- the characters of its closed words that are hotwords plus, provisionally, those of a partial word that is a prefix of a
    hotword -- as in prefix_beam_search(hotwords=...).  It goes with every other argument; the returned log weights include it.
    Weight 0 gives the results of no hotwords.  Single words only; one weight for the whole list.

    ``mbr`` ('word' or 'char'; None: today's result, no launch and no byte more): minimum-Bayes-risk selection over the k rows
    of the search (mbr.py: least expected word / character error under the posterior ``softmax(mbr_scale * log weights)``;
    ``mbr_scale`` = 1.0 is a convention, not a tuned value; any finite number >= 0).  The result is the pick instead of rank 0,
    with its own log weight under ``return_weights``; ``nbest > 1`` gives the rows in ascending risk, a tie by rank;
    ``return_risks`` appends each row's risk to it (``(text, risk)``, or ``(text, log weight, risk)`` with weights or
    ``nbest > 1``); ``return_offsets`` aligns the picked string.  One more entry point on the same stream, w2l_nbest_mbr; still
    one copy to the host.  A hypothesis of more than 4095 words / characters is a ValueError."""
    labels = list(labels)
    mbr, mbr_scale = check_mbr(mbr, mbr_scale, return_risks)
    if not 1 <= nbest <= k:
        raise ValueError('nbest=%d must lie in [1, k=%d]' % (nbest, k))
    if return_offsets and nbest != 1:
        raise ValueError('return_offsets aligns the best prefix only: nbest=%d must be 1' % nbest)
    x = probs if torch.is_tensor(probs) else torch.from_numpy(np.ascontiguousarray(probs))
    single = x.dim() == 2
    if single:
        x = x.unsqueeze(0)
        if sizes is not None:
            sizes = [int(np.asarray(sizes).reshape(-1)[0])]
    got = _beam_search_device(x, labels, blank_index, k, beta, prune, end_char, sizes, log_probs, lm=lm, alpha=alpha,
                              offsets=return_offsets, lexicon=lexicon, complete_only=complete_only, hotwords=hotwords,
                              hotword_weight=hotword_weight, mbr=mbr, mbr_scale=mbr_scale)
    scores, lengths, idx = got[:3]
    res = None
    if mbr:
        got, res = got[:-1], got[-1]
        check_mbr_status(res, 'prefix_beam_search_gpu')
    results = []
    for u in range(scores.shape[0]):
        ranks = [r for r in range(k) if lengths[u, r] >= 0]
        found = [(''.join(labels[j] for j in idx[u, r, :lengths[u, r]]), float(scores[u, r])) for r in ranks]
        if not found:                                  # the beam emptied: '' as on the host (weight 0)
            found = [('', float('-inf'))]
        results.append(mbr_rows(found, ranks, res, u, nbest, return_weights, return_risks) if mbr else
                       _pick(found, nbest, return_weights))
    if return_offsets:
        aligned_len = res.pick_len if mbr else lengths[:, 0]
        offs = [torch.IntTensor(got[-1][u, :max(int(aligned_len[u]), 0)].copy()) for u in range(scores.shape[0])]
        return (results[0], offs[0]) if single else (results, offs)
    return results[0] if single else results


def _nest_offsets(got, single):
    """prefix_beam_search_gpu's (results, offsets) in GreedyDecoder.decode's nesting: one single-element list per utterance"""
    results, offs = got
    return (results, [offs]) if single else (results, [[o] for o in offs])


def _decoder_hotwords(hotwords, hotword_weight, labels, blank_index):
    """the constructors' check of ``hotwords`` / ``hotword_weight``: (Lexicon or None, weight); ValueError for an entry with
    whitespace, for a list of which the labels can spell nothing, and for a weight that is not finite"""
    if hotwords is None:
        return None, float(hotword_weight)
    hot = _resolve_hotwords(hotwords)
    hot.spelling_trie(labels, blank_index)
    if not math.isfinite(float(hotword_weight)):
        raise ValueError('hotword_weight must be finite, got %r' % (hotword_weight,))
    return hot, float(hotword_weight)


class _GPUPrefixDecoder(Decoder):
    """what the two device prefix decoders share: ``decode`` over the attributes their constructors set (``lm``: None, or
    the ngram_lm.ArpaLM that ``alpha`` weighs)"""
    lm = None
    mbr, mbr_scale = None, 1.0

    def decode(self, probs, sizes=None, return_offsets=False):
        """[N, T, labels] -> N strings (utterance n over its first sizes[n] frames); [T, labels] -> one string.  With
        ``return_offsets``: ``(strings, offsets)`` nested as GreedyDecoder.decode's, ``offsets[n] = [IntTensor]`` (the first frame
        of each character of strings[n] on its best frame path), so get_time_per_word(strings[n], offsets[n][0]) applies"""
        _check_decode_shape(probs)
        got = prefix_beam_search_gpu(probs, self.labels, self.blank_index, self.k, self.beta, self.prune, sizes=sizes,
                                     log_probs=self.log_probs, return_offsets=return_offsets, lexicon=self.lexicon,
                                     hotwords=self.hotwords, hotword_weight=self.hotword_weight,
                                     **({'lm': self.lm, 'alpha': self.alpha} if self.lm is not None else {}),
                                     **({'mbr': self.mbr, 'mbr_scale': self.mbr_scale} if self.mbr is not None else {}))
        return _nest_offsets(got, len(probs.shape) == 2) if return_offsets else got


class GPUPrefixBeamSearchDecoder(_GPUPrefixDecoder):
    """PrefixBeamSearchLMDecoder on the MI355X (prefix_beam_search_gpu): the same constructor (plus ``log_probs``), no
    language model -- a scoring callable cannot run on the device.  ``lexicon``: a lexicon.Lexicon or a path to a word list
    that constrains the search (prefix_beam_search_gpu).  ``hotwords``: a lexicon.Lexicon, a path or an iterable of single
    words that the search prefers by ``hotword_weight`` per matched character (1.0 is a convention, not a tuned value).  ``mbr``
    ('word' or 'char') / ``mbr_scale``: ``decode`` returns the minimum-Bayes-risk pick of the k rows instead of rank 0 (mbr.py)."""

    def __init__(self, lm_path, labels, blank_index=0, k=5, alpha=0.3, beta=5, prune=1e-3, log_probs=False, lexicon=None,
                 hotwords=None, hotword_weight=1.0, mbr=None, mbr_scale=1.0):
        super(GPUPrefixBeamSearchDecoder, self).__init__(labels, blank_index)
        self.mbr, self.mbr_scale = check_mbr(mbr, mbr_scale)
        self.hotwords, self.hotword_weight = _decoder_hotwords(hotwords, hotword_weight, self.labels, blank_index)
        if isinstance(lexicon, str) and lexicon == 'lm':
            raise ValueError("GPUPrefixBeamSearchDecoder has no language model: lexicon='lm' needs GPUPrefixBeamSearchLMDecoder")
        self.lexicon = _resolve_lexicon(lexicon, None) if lexicon is not None else None
        if lm_path:
            raise ValueError('GPUPrefixBeamSearchDecoder has no language model (lm_path=%r, alpha=%r): use '
                             'PrefixBeamSearchLMDecoder, the host decoder, for LM scoring' % (lm_path, alpha))
        self.k, self.alpha, self.beta, self.prune, self.log_probs = k, alpha, beta, prune, log_probs


class GPUPrefixBeamSearchLMDecoder(_GPUPrefixDecoder):
    """PrefixBeamSearchLMDecoder on the MI355X with an ARPA n-gram model read without kenlm (ngram_lm.ArpaLM, plain or
    .gz): the reference decoder's constructor (plus ``log_probs``); a falsy ``lm_path`` decodes without an LM.  ``lexicon``: a
    lexicon.Lexicon, a path to a word list, or 'lm' (the model's vocabulary) that constrains the search.  ``hotwords`` /
    ``hotword_weight``, ``mbr`` / ``mbr_scale``: as in GPUPrefixBeamSearchDecoder."""

    def __init__(self, lm_path, labels, blank_index=0, k=5, alpha=0.3, beta=5, prune=1e-3, log_probs=False, lexicon=None,
                 hotwords=None, hotword_weight=1.0, mbr=None, mbr_scale=1.0):
        super(GPUPrefixBeamSearchLMDecoder, self).__init__(labels, blank_index)
        self.mbr, self.mbr_scale = check_mbr(mbr, mbr_scale)
        self.hotwords, self.hotword_weight = _decoder_hotwords(hotwords, hotword_weight, self.labels, blank_index)
        from .ngram_lm import ArpaLM
        self.lm = ArpaLM(lm_path) if lm_path else None
        self.lexicon = _resolve_lexicon(lexicon, self.lm) if lexicon is not None else None
        self.k, self.alpha, self.beta, self.prune, self.log_probs = k, alpha, beta, prune, log_probs


def get_time_per_word(predictions, offsets, ratio=1.0, end_offsets=None):
    """(word, start, end) triples from per-character offsets (decoder.py:270-302); the end time of a word is the
    first frame of its last character -- or, with ``end_offsets`` (the last frame of each character: Decoder.align's second
    result), the LAST frame of its last character."""
    assert len(predictions) == len(offsets)
    assert end_offsets is None or len(end_offsets) == len(offsets)
    words = []
    cur, start, end = '', -1, -1
    for i, (ch, off) in enumerate(zip(predictions, offsets)):
        if ch == ' ':
            if cur:
                words.append((cur, start, end))
                cur, start, end = '', -1, -1
            continue
        if cur:
            end = (off if end_offsets is None else end_offsets[i]) * ratio
            cur += ch
        else:
            start = off * ratio
            end = (off if end_offsets is None else end_offsets[i]) * ratio
            cur = ch
    if cur:
        words.append((cur, start, end))
    return words

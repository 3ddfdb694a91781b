"""Decoding an ASG model beyond Viterbi: a transition-aware prefix beam search with an optional word n-gram model, n-best lists,
and forced alignment -- what beam_search.py and alignment.py are to a CTC model.

The recursion.  ``x[t, c]`` are the model's scores, ``g[i, j]`` the criterion's transitions, ``r`` the repeat label; there is no
blank.  A hypothesis is an ENCODED label sequence ``e = (e_1 .. e_m)``, ``m >= 1``, no two neighbours equal (consecutive equal
frames merge); its text is ``decode_repeats(e)`` (each ``r`` becomes the decoded character before it, a leading ``r`` is
dropped; two hypotheses that differ only by a leading ``r`` stay distinct entries).  One mass per hypothesis, the log-sum over
the frame paths that read it, in float64 natural logs:

    M_0((c)) = x[0, c]                                             for every label c taking part in frame 0
    for t >= 1, members in beam order, l = last(e):
        stay     cur[e]   (+)= M_{t-1}(e) + g[l, l] + x[t, l]                        if l takes part in frame t
        extend   cur[e+c] (+)= M_{t-1}(e) + g[l, c] + x[t, c]  (+ the LM term)       each participating c != l, ascending
                 cur[e+c] (+)= M_{t-1}(e+c) + g[c, c] + x[t, c]                      if e+c is no member but was a candidate
                                                                                     of frame t-1 (it fell off the beam)

``(+)=`` is log-add in exactly this order.  Label c takes part in frame t if ``x[t, c] > log(prune)`` or c is the frame's first
argmax (``prune <= 0``: every label), so the beam never empties.  Rank key ``M_t(e) + beta * log(words(text) + 1)`` (words
counted as the CTC search counts them), ties in first-insertion order, the best k are the next beam.  No end character.  LM: the
extend contribution gets ``alpha * ln(lm(text of e))`` when c is the space, the member's last decoded character is not, and
its text has a non-space character (the rule of the CTC search, on decoded characters).

Word lists (``lexicon=``, ``hotwords=``; lexicon.py) act on the DECODED text, so a word with a doubled letter is reached through
the repeat label (``ALL`` is ``A L r``) and the only separator is the space.  Lexicon: a hypothesis whose text is not legal
(Lexicon.allows) gets no mass, from its parent or from its own previous mass; ``complete_only`` draws the results from the
final members whose last word is whole.  Hotwords: the rank key gains ``hotword_weight * Lexicon.boost_chars(text)``.  With no
blank a constrained beam could die -- every participating extension illegal while no member's last label takes part -- so
UNDER A LEXICON ONLY a label also takes part in frame t if ``t == 0`` (every label) or it is the last label of a member of
the current beam (every member can stay); it stays one ascending set per frame, for stays and extensions alike.

asg_prefix_beam_search / asg_viterbi_align_host restate the recursions on the host (the oracles of the device tests);
asg_beam_search_gpu / asg_forced_align launch csrc/asg_beam.hip (w2l_asg_beam_search_tables, w2l_asg_align)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .alignment import (Alignment, HostAlignment, _launch, align_buffers, align_sections, align_targets, aligned, batch_of,
                        host_lengths, on_device, split_align)
from .asg import MAX_LABELS, ASGDecoder, _check_labels, decode_repeats, encode_repeats
from .beam_search import (_check_decode_shape, _decoder_hotwords, _desc, _n_words, _pick, _resolve_hotwords, _resolve_lexicon,
                          _word_tables, search_out_layout, split_search_out, word_flags)
from .mbr import check_mbr, check_mbr_status, launch_mbr, mbr_offset, mbr_rows, mbr_sections, split_mbr

_NINF = float('-inf')


def _lae(a: float, b: float) -> float:
    """log(exp(a) + exp(b)) as the kernel forms it"""
    if a == _NINF:
        return b
    if b == _NINF:
        return a
    m, d = (a, b - a) if a > b else (b, a - b)
    return m + math.log1p(math.exp(d))


def _text(encoded, labels, repeat_index):
    return ''.join(labels[i] for i in decode_repeats(encoded, repeat_index))


def asg_prefix_beam_search(x, transitions, labels: Sequence[str], repeat_index: int = 0,
                           lm: Optional[Callable[[str], float]] = None, k: int = 5, alpha: float = 0.3, beta: float = 5,
                           prune: float = 1e-3, nbest: int = 1, return_weights: bool = False, return_encoded: bool = False,
                           lexicon=None, complete_only: bool = True, hotwords=None, hotword_weight: float = 1.0):
    """The recursion of the module docstring for one utterance, float64: x ``[T, A]`` scores, transitions ``[A, A]`` (None:
    zeros), ``lm`` a callable text -> probability.  Returns the best text; ``(text, weight)`` with ``return_weights`` (weight:
    the rank key, the log mass where beta = 0); with ``nbest > 1`` a list of up to ``nbest`` such pairs, best first.
    ``return_encoded`` appends the hypothesis' encoded label tuple to every result.

    ``lexicon`` (a lexicon.Lexicon; None: no constraint), stated on the DECODED text with ``str`` operations: a hypothesis gets
    mass -- in frame 0, as an extension, and from its own previous mass where it fell off the beam -- only if
    ``lexicon.allows(text, end_char='')`` (the words the labels can spell; the repeat label spells nothing of its own).  With
    ``complete_only`` the results are the members of the final beam with ``lexicon.complete(text, end_char='')``, in rank order
    with their own weights; all members if there is none.  Under a lexicon a label also takes part in a frame if the frame is
    the first or the label is the last label of a member of the current beam (the module docstring), so the beam never empties.

    ``hotwords`` (a lexicon.Lexicon, a path or an iterable of single words; None: no boosting): the rank key gains
    ``hotword_weight * hotwords.boost_chars(text, end_char='')``; masses are untouched, weight 0 gives the keys of no hotwords."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError('asg_prefix_beam_search: expected [T >= 1, A] scores, got shape %s' % (x.shape,))
    t_n, a = x.shape
    labels = list(labels)
    if a != len(labels):
        raise ValueError('asg size:%d, labels: %d' % (a, len(labels)))
    g = np.zeros((a, a)) if transitions is None else np.asarray(transitions, dtype=np.float64)
    if g.shape != (a, a):
        raise ValueError('transitions of shape %s for %d labels' % (g.shape, a))
    if not 1 <= nbest <= k:
        raise ValueError('nbest=%d must lie in [1, k=%d]' % (nbest, k))
    r = int(repeat_index)
    log_prune = math.log(prune) if prune > 0 else _NINF
    lex = lexicon.spellable(labels, r) if lexicon is not None else None
    hot, gamma = None, 0.0
    if hotwords is not None:
        hot = _resolve_hotwords(hotwords).spellable(labels, r)
        gamma = float(hotword_weight)
        if not math.isfinite(gamma):
            raise ValueError('hotword_weight must be finite, got %r' % (hotword_weight,))
    texts = {}
    legal = {}

    def text_of(e):
        s = texts.get(e)
        if s is None:
            s = texts[e] = _text(e, labels, r)
        return s

    lm_terms = {}

    def lm_term(e):
        s = text_of(e)
        if lm is None or not s or s[-1] == ' ' or not s.replace(' ', ''):
            return 0.0
        s = (s + ' ').strip(' ')
        if s not in lm_terms:
            v = lm(s)
            lm_terms[s] = alpha * math.log(v) if v > 0 else _NINF
        return lm_terms[s]

    def allowed(e):
        if lex is None:
            return True
        if e not in legal:
            legal[e] = lex.allows(text_of(e), end_char='')
        return legal[e]

    def takes_part(frame, members=None):
        """the frame's labels, ascending; under a lexicon every label of frame 0 (``members`` None) and the last label of
        every member of the beam take part as well"""
        first = int(np.argmax(frame))
        also = () if lex is None else (range(a) if members is None else {e[-1] for e in members})
        return [c for c in range(a) if prune <= 0 or frame[c] > log_prune or c == first or c in also]

    def rank(cur):
        live = [e for e in cur if cur[e] > _NINF]
        if hot is None:
            keys = {e: cur[e] + beta * math.log(_n_words(text_of(e)) + 1) for e in live}
        else:
            keys = {e: cur[e] + beta * math.log(_n_words(text_of(e)) + 1) + gamma * hot.boost_chars(text_of(e), end_char='')
                    for e in live}
        return sorted(live, key=lambda e: keys[e], reverse=True), keys       # stable: ties keep first insertion

    cur = {(c,): float(x[0, c]) for c in takes_part(x[0]) if allowed((c,))}
    order, keys = rank(cur)
    beam = order[:k]
    for t in range(1, t_n):
        frame = x[t]
        part = takes_part(frame, beam)
        part_set = set(part)
        prev, cur = cur, {}
        in_beam = set(beam)
        for e in beam:
            l = e[-1]
            if l in part_set:
                cur[e] = _lae(cur.get(e, _NINF), float(prev[e] + g[l, l] + frame[l]))
            closes = lm_term(e)
            for c in part:
                if c == l:
                    continue
                ext = e + (c,)
                if not allowed(ext):                     # the extension leaves the word list: no mass for it
                    continue
                v = float(prev[e] + g[l, c] + frame[c])
                if labels[c] == ' ':
                    v += closes
                cur[ext] = _lae(cur.get(ext, _NINF), v)
                if ext not in in_beam and ext in prev:
                    cur[ext] = _lae(cur[ext], float(prev[ext] + g[c, c] + frame[c]))
        order, keys = rank(cur)
        beam = order[:k]
    if lex is not None and complete_only:
        beam = [e for e in beam if lex.complete(text_of(e), end_char='')] or beam
    found = [(text_of(e), keys[e], e) for e in beam]
    if not found:
        found = [('', _NINF, ())]
    return _pick(found, nbest, return_weights, return_encoded)


def _encoded_target(target, a: int, repeat_index: int, encoded: bool, what: str):
    tg = [int(v) for v in np.asarray(target, dtype=np.int64).reshape(-1)]
    if any(v < 0 or v >= a for v in tg):
        raise ValueError('%s: a target lies outside [0, %d)' % (what, a))
    if not encoded:
        return np.asarray(encode_repeats(tg, repeat_index), dtype=np.int64)
    if any(u == v for u, v in zip(tg, tg[1:])):
        raise ValueError('%s: an encoded target has two equal neighbours' % what)
    return np.asarray(tg, dtype=np.int64)


def asg_viterbi_align_host(x, transitions, target, repeat_index: int = 0, encoded: bool = False,
                           dtype=np.float64) -> HostAlignment:
    """Best frame path of ``target`` under ASG, the Viterbi form of Z_tgt: over the encoded target y_0 .. y_{S-1} (``target`` is a
    raw transcript, encoded here, unless ``encoded``), ``score[0][0] = x[0, y_0]``, ``score[t][s] = max(score[t-1][s] + g[y_s,
    y_s], score[t-1][s-1] + g[y_{s-1}, y_s]) + x[t, y_s]``, a tie goes to staying, ending in state S-1 at the last frame;
    feasible iff 1 <= S <= T.  ``path`` holds the ENCODED label of each frame, ``starts`` / ``ends`` the first / last frame of
    each target position.  With ``dtype=np.float32`` the arithmetic is w2l_asg_align's, add for add."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype, copy=False)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError('asg_viterbi_align_host: expected [T >= 1, A] scores, got shape %s' % (x.shape,))
    t_n, a = x.shape
    g = (np.zeros((a, a)) if transitions is None else np.asarray(transitions)).astype(dtype, copy=False)
    y = _encoded_target(target, a, int(repeat_index), encoded, 'asg_viterbi_align_host')
    s_n = y.size
    none = np.full(s_n, -1, dtype=np.int32)
    infeasible = HostAlignment(dtype(-np.inf), np.full(t_n, -1, dtype=np.int32), none, none.copy(), False)
    if not 1 <= s_n <= t_n:
        return infeasible
    ninf = dtype(-np.inf)
    g_stay = g[y, y]
    g_move = g[y[:-1], y[1:]]
    score = np.full(s_n, ninf, dtype=dtype)
    score[0] = x[0, y[0]]
    moves = np.zeros((t_n, s_n), dtype=np.uint8)
    with np.errstate(invalid='ignore'):
        for t in range(1, t_n):
            best = score + g_stay
            a1 = np.full(s_n, ninf, dtype=dtype)
            a1[1:] = score[:-1] + g_move
            m = a1 > best                               # a tie goes to staying
            best[m] = a1[m]
            moves[t] = m
            score = best + x[t, y]
    best = score[s_n - 1]
    if not best > ninf:
        return infeasible
    states = np.empty(t_n, dtype=np.int64)
    s = s_n - 1
    for t in range(t_n - 1, 0, -1):
        states[t] = s
        s -= int(moves[t, s])
    states[0] = s
    change = states[1:] != states[:-1]
    first = np.concatenate(([True], change))
    last = np.concatenate((change, [True]))
    starts = np.full(s_n, -1, dtype=np.int32)
    ends = np.full(s_n, -1, dtype=np.int32)
    starts[states[first]] = np.nonzero(first)[0]
    ends[states[last]] = np.nonzero(last)[0]
    return HostAlignment(best, y[states].astype(np.int32), starts, ends, True)


# ---------------------------------------------------------------------------------------------------------------- device
def _label_info(labels, lm: bool = False):
    """per-label flags of w2l_asg_beam_search (include/w2l_hip.h): the first index of the character, \\w, [\\s|>], whitespace"""
    if not all(isinstance(ch, str) and len(ch) == 1 for ch in labels):
        raise ValueError('asg_beam_search_gpu: every label must be one character')
    first = {}
    for i, ch in enumerate(labels):
        first.setdefault(ch, i)
    return np.array([first[ch] | word_flags(ch) | (lm and ch.isspace()) << 11 for ch in labels], dtype=np.int32)


def _transitions_on(transitions, a: int, dev):
    if isinstance(transitions, nn.Module):            # a criterion: whatever Parameter it holds now
        transitions = transitions.transitions
    if transitions is None:
        return torch.zeros(a, a, dtype=torch.float32, device=dev)
    g = transitions if torch.is_tensor(transitions) else torch.from_numpy(np.ascontiguousarray(transitions))
    g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
    if tuple(g.shape) != (a, a):
        raise ValueError('transitions of shape %s for %d labels' % (tuple(g.shape), a))
    return g


def launch_asg_align(x, g, sz, tg_ptr: int, tg_stride: int, len_ptr: int, len_stride: int, smax: int, repeat_index: int,
                     encoded: bool, out, out_offset: int):
    """one w2l_asg_align launch on the current stream, addressed as alignment.launch_align: outputs into ``out`` (a uint8 device
    tensor) from byte ``out_offset`` in align_sections' layout.  -> the workspace tensor (or None): keep it alive until the
    stream has passed."""
    n, t, a = x.shape
    return _launch('w2l_asg_align', lib.w2l_asg_align_workspace_bytes(n, t, a, smax),
                   'asg_forced_align: T=%d (max 32768), target length %d (max 4095) or %d labels (max %d) out of range'
                   % (t, smax, a, MAX_LABELS), (ptr(x), ptr(g)), x, sz, tg_ptr, tg_stride, len_ptr, len_stride, smax,
                   (int(repeat_index), int(bool(encoded))), out, out_offset)


def _search_device(x, g, sz, labels, repeat_index, k, beta, prune, lm, alpha, offsets, lexicon=None, complete_only=True,
                   hotwords=None, hotword_weight=1.0, mbr=None, mbr_scale=1.0):
    """one launch of w2l_asg_beam_search_tables (a table that is None: passed as NULL) for x [N, T, A] on the current stream,
    with ``offsets`` followed by w2l_asg_align on rank 0 where the search wrote it; one copy to the host.  ``lexicon``: a
    lexicon.Lexicon, a path or 'lm' (the vocabulary of ``lm``); ``hotwords``: a Lexicon, a path or an iterable of single words.
    -> (scores [N, k], lengths [N, k], encoded labels [N, k, T], lm_log10 [N, k] or None, starts [N, T] or None).  With ``mbr``
    ('word' or 'char') w2l_nbest_mbr follows the search on the decoded text, ``offsets`` aligns ITS pick (the section's
    pick_labels) instead of rank 0, and the tuple has a sixth element, the mbr.MbrResult."""
    n, t, a = x.shape
    dev = x.device
    any_table = lm is not None or lexicon is not None or hotwords is not None
    info = _label_info(labels, any_table)
    if offsets and t > 4095:
        raise ValueError('return_offsets: %d frames, w2l_asg_align takes targets of at most 4095 labels' % t)
    # the repeat label takes the blank's place as the label that spells nothing
    tables, lex, hot, space_index, order = _word_tables(labels, repeat_index, lm, lexicon, hotwords, hotword_weight, dev,
                                                        'asg_beam_search_gpu')
    ws_bytes = int(lib.w2l_asg_beam_search_workspace_bytes(n, t, a, k, order))
    if ws_bytes < 0:
        raise ValueError('asg_beam_search_gpu: k=%d (1..64), %d labels (1..%d) or T=%d is out of range' % (k, a, MAX_LABELS, t))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    lay = search_out_layout(n, k, t, lm is not None)
    beam_bytes = lay.beam_bytes
    mbr_at = mbr_offset(beam_bytes)
    align_at = mbr_at + mbr_sections(n, k, t).total if mbr else beam_bytes
    out = torch.empty(align_at + (align_sections(n, t, t)[5] if offsets else 0), dtype=torch.uint8, device=dev)
    check(lib.w2l_asg_beam_search_tables(ptr(x), ptr(g), ptr(sz), n, t, a, info.ctypes.data_as(C.c_void_p), int(repeat_index),
                                         space_index, int(k), float(alpha), float(beta), float(prune),
                                         _desc(tables), order, _desc(lex), int(bool(complete_only)), _desc(hot),
                                         float(hotword_weight), ptr(ws), ws_bytes, ptr(out), stream_ptr()),
          'w2l_asg_beam_search_tables')
    mbr_ws = launch_mbr(out, mbr_at, n, k, t, labels, mbr, repeat_index, mbr_scale) if mbr else None
    align_ws = None
    if offsets and mbr:
        # the pick of every utterance, where w2l_nbest_mbr copied it: encoded rows of stride T
        sec = mbr_sections(n, k, t)
        align_ws = launch_asg_align(x, g, sz, out.data_ptr() + mbr_at + sec.pick_labels, t, out.data_ptr() + mbr_at + sec.pick_len,
                                    1, t, repeat_index, True, out, align_at)
    elif offsets:
        # rank 0 of every utterance, aligned where it lies
        align_ws = launch_asg_align(x, g, sz, out.data_ptr() + lay.labels, lay.labels_stride, out.data_ptr() + lay.lengths,
                                    lay.lengths_stride, t, repeat_index, True, out, beam_bytes)
    host = out.cpu().numpy()                           # the one copy to the host (ordered after the launches on this stream)
    del align_ws, mbr_ws
    scores, lengths, status, idx, lm_log10 = split_search_out(host, n, k, t, lm is not None)
    if status.any():
        raise ValueError('the scores or transitions contain NaN (utterances %s)' % np.nonzero(status)[0].tolist())
    res = split_mbr(host[mbr_at:], n, k, t) if mbr else None
    starts = None
    if offsets:
        _, a_status, _, starts, _ = split_align(host[align_at:], n, t, t)
        # (an emptied beam -- a frame without one finite score -- decodes to '' and has no characters to place: its empty
        # slot reads as S = 0, which the alignment calls infeasible; every other status is a real failure)
        a_status = np.where((res.pick_len if mbr else lengths[:, 0]) < 1, 0, a_status)
        if a_status.any():
            raise _lib.W2LError('w2l_asg_align found no path for the decoded hypothesis of utterances %s (status %s)'
                                % (np.nonzero(a_status)[0].tolist(), a_status[a_status != 0].tolist()))
    if mbr:
        return scores, lengths, idx, lm_log10, starts, res
    return scores, lengths, idx, lm_log10, starts


def asg_beam_search_gpu(x, transitions, labels: Sequence[str], repeat_index: int = 0, k: int = 5, beta: float = 5,
                        prune: float = 1e-3, sizes=None, nbest: int = 1, return_weights: bool = False, lm=None,
                        alpha: float = 0.3, return_offsets: bool = False, return_encoded: bool = False, lexicon=None,
                        complete_only: bool = True, hotwords=None, hotword_weight: float = 1.0, mbr=None,
                        mbr_scale: float = 1.0, return_risks: bool = False):
    """asg_prefix_beam_search on the MI355X: one launch for a whole batch, the host's candidate order and ties.  x: ``[T, A]`` or
    ``[N, T, A]`` scores (numpy or torch, any device), transitions ``[A, A]`` (a tensor, an array, an ASGLoss, or None: zeros),
    ``sizes[n]``: decode only the first sizes[n] frames of utterance n; ``lm``: an ngram_lm.ArpaLM, scored as the host's
    ``lm=lambda s: 10 ** lm.score(s)``.  Per utterance the result is asg_prefix_beam_search's; a ``[T, A]`` input gives one
    result, a batch a list of N.  ``return_offsets`` (only with ``nbest == 1``): ``(results, offsets)``, offsets an IntTensor per
    utterance holding the first frame of each character of its best text on that hypothesis' best frame path (one more launch,
    w2l_asg_align, on the same stream; still one copy to the host); the state of a leading repeat label emits none, an empty
    result has empty offsets.  ``return_offsets`` takes at most 4095 frames (w2l_asg_align's target limit: a hypothesis can be
    as long as the utterance).

    ``lexicon`` (a lexicon.Lexicon, a path to a word list, or 'lm': the vocabulary of ``lm``; None: no constraint), with
    ``complete_only``, and ``hotwords`` (a Lexicon, a path, or an iterable of single words; None: no boosting) with
    ``hotword_weight`` (natural-log units per matched character, any finite real; 1.0 is a convention, not a tuned value) are
    asg_prefix_beam_search's, with or without ``lm``: words are spelled by the decoded text, the results (best, n-best,
    offsets) come from the complete members of the final beam, the returned weights include the hotword term, and under a
    lexicon the participation rule of the module docstring keeps the beam alive.

    ``mbr`` ('word' or 'char'; None: today's result, no launch and no byte more), ``mbr_scale`` and ``return_risks`` are
    beam_search.prefix_beam_search_gpu's: minimum-Bayes-risk selection over the k rows (mbr.py), on their DECODED texts.  The
    result is the pick instead of rank 0; ``nbest > 1`` gives the rows in ascending risk; ``return_risks`` appends each row's
    risk (behind the encoded tuple with ``return_encoded``); ``return_offsets`` aligns the picked hypothesis."""
    labels = list(labels)
    mbr, mbr_scale = check_mbr(mbr, mbr_scale, return_risks)
    _check_labels(len(labels), 'asg_beam_search_gpu')
    if not 1 <= nbest <= k:
        raise ValueError('nbest=%d must lie in [1, k=%d]' % (nbest, k))
    if return_offsets and nbest != 1:
        raise ValueError('return_offsets aligns the best hypothesis only: nbest=%d must be 1' % nbest)
    x, sizes, single = batch_of(x, sizes)
    x = on_device(x, 'asg_beam_search_gpu')
    if x.dim() != 3:
        raise ValueError('expected [N, T, labels] or [T, labels] scores, got shape %s' % (tuple(x.shape),))
    n, t, a = x.shape
    if a != len(labels):
        raise ValueError('asg size:%d, labels: %d' % (a, len(labels)))
    if n < 1 or t < 1:
        raise ValueError('asg_beam_search_gpu: empty scores, shape %s' % (tuple(x.shape),))
    if not 0 <= int(repeat_index) < a:
        raise ValueError('repeat_index %d outside %d labels' % (repeat_index, a))
    g = _transitions_on(transitions, a, x.device)
    sz = host_lengths(sizes, n, t, 'sizes').to(x.device, non_blocking=True) if sizes is not None else None
    got = _search_device(x, g, sz, labels, int(repeat_index), int(k), beta, prune, lm, alpha, return_offsets, lexicon=lexicon,
                         complete_only=complete_only, hotwords=hotwords, hotword_weight=hotword_weight, mbr=mbr,
                         mbr_scale=mbr_scale)
    scores, lengths, idx, _, starts = got[:5]
    res = got[5] if mbr else None
    if mbr:
        check_mbr_status(res, 'asg_beam_search_gpu')
    results = []
    for u in range(n):
        found, ranks = [], []
        for rk in range(k):
            if lengths[u, rk] >= 0:
                e = tuple(int(v) for v in idx[u, rk, :lengths[u, rk]])
                found.append((_text(e, labels, repeat_index), float(scores[u, rk]), e))
                ranks.append(rk)
        if not found:
            found = [('', _NINF, ())]
        results.append(mbr_rows(found, ranks, res, u, nbest, return_weights, return_risks, return_encoded) if mbr else
                       _pick(found, nbest, return_weights, return_encoded))
    if return_offsets:
        offs = []
        for u in range(n):
            row, m = (res.pick_labels[u], int(res.pick_len[u])) if mbr else (idx[u, 0], int(lengths[u, 0]))
            m = max(m, 0)
            lead = 1 if m and row[0] == repeat_index else 0
            offs.append(torch.IntTensor(starts[u, lead:m].copy()))
        return (results[0], offs[0]) if single else (results, offs)
    return results[0] if single else results


def asg_forced_align(x, transitions, targets, input_lengths=None, target_lengths=None, labels: Optional[Sequence[str]] = None,
                     repeat_index: int = 0, encoded: bool = False) -> Alignment:
    """Align each utterance's target to its scores under ASG on the MI355X (w2l_asg_align): one launch, one copy to the host;
    the counterpart of alignment.ctc_forced_align, with its target formats.  Targets are RAW transcripts, repeat-encoded on the
    device (a label equal to ``repeat_index`` is a ValueError), unless ``encoded``: then the rows are encoded label sequences
    as the search returns them, the repeat label allowed, in front too.  ``paths`` holds the ENCODED label of each frame;
    ``starts`` / ``ends`` the first / last frame of each target position.  An utterance with an empty target or more labels than
    frames does not raise: ``feasible[n]`` is False."""
    x, input_lengths, _ = batch_of(on_device(x, 'asg_forced_align'), input_lengths)
    if x.dim() != 3:
        raise ValueError('expected [N, T, labels] or [T, labels] scores, got shape %s' % (tuple(x.shape),))
    n, t, a = x.shape
    if n < 1 or t < 1:
        raise ValueError('asg_forced_align: empty scores, shape %s' % (tuple(x.shape),))
    _check_labels(a, 'asg_forced_align')
    if labels is not None and len(labels) != a:
        raise ValueError('asg size:%d, labels: %d' % (a, len(labels)))
    if not 0 <= int(repeat_index) < a:
        raise ValueError('repeat_index %d outside %d labels' % (repeat_index, a))
    tg, tl, smax = align_targets(targets, target_lengths, labels, n, t, 'asg_forced_align')
    g = _transitions_on(transitions, a, x.device)
    il = host_lengths(input_lengths, n, t, 'input_lengths') if input_lengths is not None else None
    sz, tgt, out = align_buffers(x, il, tg, tl)
    ws = launch_asg_align(x, g, sz, tgt.data_ptr(), max(smax, 1), tgt.data_ptr() + 4 * n * smax, 1, smax, int(repeat_index),
                          encoded, out, 0)
    got = aligned(out, n, t, smax, tl, 'asg_forced_align: a target outside [0, %d), %s, in utterances %%s'
                  % (a, 'two equal neighbours in an encoded target' if encoded else
                     'or equal to the repeat label (%d)' % repeat_index))
    del ws
    return got


class ASGBeamSearchDecoder(ASGDecoder):
    """ASGDecoder with the prefix beam search in the place of the Viterbi path (asg_beam_search_gpu): the same constructor plus
    the search's ``k``, ``beta`` and ``prune``; ``decode`` has ASGDecoder.decode's arguments and return shapes, so it goes
    wherever the model's own decoder goes (``model.transcribe(decoder=...)``, ``evaluate(decoder=...)``).  ``lexicon`` (a
    lexicon.Lexicon or a path to a word list) with ``complete_only`` constrains the search, ``hotwords`` (a Lexicon, a path or
    an iterable of single words) with ``hotword_weight`` makes it prefer words (asg_beam_search_gpu).  ``mbr`` ('word' or
    'char') / ``mbr_scale``: ``decode`` returns the minimum-Bayes-risk pick of the k rows instead of rank 0 (mbr.py)."""
    lm = None
    alpha = 0.3

    def __init__(self, labels, repeat_index=0, transitions=None, k=5, beta=5, prune=1e-3, lexicon=None, complete_only=True,
                 hotwords=None, hotword_weight=1.0, mbr=None, mbr_scale=1.0):
        super().__init__(labels, repeat_index, transitions)
        self.k, self.beta, self.prune = int(k), beta, prune
        self.mbr, self.mbr_scale = check_mbr(mbr, mbr_scale)
        self._set_word_lists(lexicon, complete_only, hotwords, hotword_weight, None)

    def _set_word_lists(self, lexicon, complete_only, hotwords, hotword_weight, lm):
        self.hotwords, self.hotword_weight = _decoder_hotwords(hotwords, hotword_weight, list(self.labels), self.repeat_index)
        if lm is None and isinstance(lexicon, str) and lexicon == 'lm':
            raise ValueError("lexicon='lm' needs a language model: %s has none" % type(self).__name__)
        self.lexicon = _resolve_lexicon(lexicon, lm) if lexicon is not None else None
        self.complete_only = bool(complete_only)

    def decode(self, probs, sizes=None, transitions=None, return_offsets=False):
        """[N, T, labels] (or [T, labels]) scores -> one string per utterance; with ``return_offsets`` ``(strings, offsets)``,
        ``offsets[n] = [IntTensor]``: the first frame of each character of strings[n] on its hypothesis' best frame path (an
        empty string has empty offsets).  Limit: ``return_offsets`` takes at most 4095 frames -- a hypothesis can be as long
        as the utterance and w2l_asg_align takes targets of at most 4095 labels; without offsets the search has no such limit"""
        _check_decode_shape(probs)
        if len(probs.shape) == 2:
            probs = probs.unsqueeze(0) if torch.is_tensor(probs) else np.asarray(probs)[None]
        got = asg_beam_search_gpu(probs, self.transitions if transitions is None else transitions, list(self.labels),
                                  self.repeat_index, k=self.k, beta=self.beta, prune=self.prune, sizes=sizes, lm=self.lm,
                                  alpha=self.alpha, return_offsets=return_offsets, lexicon=self.lexicon,
                                  complete_only=self.complete_only, hotwords=self.hotwords,
                                  hotword_weight=self.hotword_weight,
                                  **({'mbr': self.mbr, 'mbr_scale': self.mbr_scale} if self.mbr is not None else {}))
        if return_offsets:
            return got[0], [[o] for o in got[1]]
        return got


class ASGBeamSearchLMDecoder(ASGBeamSearchDecoder):
    """ASGBeamSearchDecoder with an ARPA word n-gram model on the device (ngram_lm.ArpaLM, plain or .gz) at weight ``alpha``; a
    falsy ``lm_path`` decodes without an LM.  ``lexicon`` may also be 'lm', the model's vocabulary."""

    def __init__(self, lm_path, labels, repeat_index=0, transitions=None, k=5, alpha=0.3, beta=5, prune=1e-3, lexicon=None,
                 complete_only=True, hotwords=None, hotword_weight=1.0, mbr=None, mbr_scale=1.0):
        super().__init__(labels, repeat_index, transitions, k=k, beta=beta, prune=prune, mbr=mbr, mbr_scale=mbr_scale)
        from .ngram_lm import ArpaLM
        self.lm = ArpaLM(lm_path) if lm_path else None
        self.alpha = alpha
        self._set_word_lists(lexicon, complete_only, hotwords, hotword_weight, self.lm)

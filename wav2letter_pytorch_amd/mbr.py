"""Minimum-Bayes-risk (MBR) decoding over a beam search's n-best list, and the device edit distance it stands on.

A beam search returns the string of the greatest weight: the choice that minimises the chance of a wholly wrong sentence.  What
``test`` reports is WER.  MBR picks, from the same k rows, the one with the least EXPECTED error under the list's own posterior:

    m = max_j w_j,  e_j = exp(scale * (w_j - m)),  p_j = e_j / sum_j e_j          (w_j: the search's log weight as returned --
    risk_i = sum_j p_j * dist(i, j)                                                beta word bonus, LM, hotwords included)
    pick   = the row of least risk, a tie to the lower rank

in float64 with j = 0..k-1 in order over the rows that are present.  ``dist`` is the Levenshtein distance over words
(``str.split()``: what ``Decoder.wer`` compares) or over characters with ' ' removed (``Decoder.cer``).  ``scale`` = 1.0 takes
the weights as they are: a convention, not a tuned value.  It costs no model and no tuning, only k (k - 1) / 2 edit distances
per utterance, which is why they run on the device: w2l_nbest_mbr (csrc/edit_distance.hip) reads the search's ``out`` buffer in
place on the search's stream, and its section comes back in the search's one copy to the host.

The edit distance, here and on the device, is this recurrence over a reference a[0..na) and a hypothesis b[0..nb): D[0][0] = 0,
D[i][0] = i deletions, D[0][j] = j insertions; for i, j >= 1 the candidates in the order diagonal (D[i-1][j-1], plus one
substitution if a[i-1] != b[j-1]), deletion (D[i-1][j] + 1), insertion (D[i][j-1] + 1); the cell takes the FIRST candidate of the
smallest distance, with its counts.  edit_distance_gpu / edit_distance_pairs_gpu launch it for many pairs at once
(w2l_edit_distance); mbr_select_host is the host oracle of the selection."""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from typing import Sequence

import numpy as np

UNITS = ('word', 'char')
MAX_TOKENS = 4095              # per sequence: ED_MAX_LEN of csrc/edit_distance.hip (w2l_ctc_align's target limit)
MAX_K = 64

MbrSections = namedtuple('MbrSections', 'pick status risk dist pick_len pick_labels total')
MbrResult = namedtuple('MbrResult', 'pick status risk dist pick_len pick_labels')


def check_unit(unit, what: str = 'mbr') -> str:
    if unit not in UNITS:
        raise ValueError("%s=%r is not one of 'word', 'char'" % (what, unit))
    return unit


def check_mbr(mbr, mbr_scale, return_risks: bool = False):
    """the searches' and decoders' check of ``mbr`` / ``mbr_scale`` / ``return_risks``, before the device is touched"""
    if mbr is None:
        if return_risks:
            raise ValueError('return_risks needs mbr= (there are no risks without MBR selection)')
        return None, float(mbr_scale)
    check_unit(mbr)
    try:
        scale = float(mbr_scale)
    except (TypeError, ValueError):
        raise ValueError('mbr_scale=%r is not a number' % (mbr_scale,)) from None
    if not math.isfinite(scale) or scale < 0:
        raise ValueError('mbr_scale must be a finite number >= 0, got %r' % (mbr_scale,))
    return mbr, scale


def words_of(text: str):
    """the word unit's tokens: what Decoder.wer compares"""
    return text.split()


def chars_of(text: str):
    """the char unit's tokens: what Decoder.cer compares"""
    return list(text.replace(' ', ''))


def label_classes(labels: Sequence[str]) -> np.ndarray:
    """w2l_nbest_mbr's per-label class: the first index of the label's character | 0x100 for ' ' | 0x200 for whitespace"""
    labels = list(labels)
    if len(labels) > 128:
        raise ValueError('mbr: %d labels, w2l_nbest_mbr takes at most 128' % len(labels))
    if not all(isinstance(ch, str) and len(ch) == 1 for ch in labels):
        raise ValueError('mbr: every label must be one character')
    first = {}
    for i, ch in enumerate(labels):
        first.setdefault(ch, i)
    return np.array([first[ch] | (ch == ' ') << 8 | ch.isspace() << 9 for ch in labels], dtype=np.int32)


def mbr_sections(n: int, k: int, t: int) -> MbrSections:
    """byte offsets of w2l_nbest_mbr's outputs inside its section (include/w2l_hip.h), and the section's size"""
    o_status = 4 * n
    o_risk = o_status + 4 * n
    o_dist = o_risk + 8 * n * k
    o_len = o_dist + 4 * n * k * k
    o_labels = o_len + 4 * n
    return MbrSections(0, o_status, o_risk, o_dist, o_len, o_labels, o_labels + 4 * n * t)


def mbr_offset(beam_bytes: int) -> int:
    """where the section starts behind a search's ``beam_bytes``: the next multiple of 8 (it holds doubles)"""
    return (beam_bytes + 7) // 8 * 8


def launch_mbr(out, offset: int, n: int, k: int, t: int, labels, unit: str, repeat_index: int, scale: float):
    """one w2l_nbest_mbr call on the current stream over the search results at the head of ``out`` (a uint8 device tensor), the
    section written from byte ``offset``.  -> the workspace tensor: keep it alive until the stream has passed."""
    import torch
    from ._lib import check, lib, stream_ptr
    cls = label_classes(labels)
    ws_bytes = int(lib.w2l_nbest_mbr_workspace_bytes(n, k, t))
    if ws_bytes < 0:
        raise ValueError('mbr: N=%d (max 65535), k=%d (1..%d) or T=%d (max 32768) is out of range' % (n, k, MAX_K, t))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
    check(lib.w2l_nbest_mbr(C.c_void_p(out.data_ptr()), n, k, t, cls.ctypes.data_as(C.c_void_p), len(cls),
                            UNITS.index(unit), int(repeat_index), float(scale), C.c_void_p(ws.data_ptr()), ws_bytes,
                            C.c_void_p(out.data_ptr() + offset), stream_ptr()), 'w2l_nbest_mbr')
    return ws


def split_mbr(host: np.ndarray, n: int, k: int, t: int) -> MbrResult:
    """the host copy of the section's bytes -> MbrResult(pick [n], status [n], risk [n, k], dist [n, k, k], pick_len [n],
    pick_labels [n, t])"""
    o = mbr_sections(n, k, t)
    return MbrResult(host[o.pick:o.status].view(np.int32), host[o.status:o.risk].view(np.int32),
                     host[o.risk:o.dist].view(np.float64).reshape(n, k), host[o.dist:o.pick_len].view(np.int32).reshape(n, k, k),
                     host[o.pick_len:o.pick_labels].view(np.int32), host[o.pick_labels:o.total].view(np.int32).reshape(n, t))


def check_mbr_status(res: MbrResult, what: str):
    if res.status.any():
        raise ValueError('%s: mbr met a hypothesis of more than %d tokens, or a label outside the label set, in utterances %s'
                         % (what, MAX_TOKENS, np.nonzero(res.status)[0].tolist()))


def mbr_rows(found, ranks, res: MbrResult, u: int, nbest: int, return_weights: bool, return_risks: bool,
             return_encoded: bool = False):
    """one utterance's result under MBR.  ``found``: the present rows (text, weight, ...) in rank order, ``ranks`` their slots
    in the search's buffer.  The rows in ascending risk, a tie by rank -- the first is the device's pick --, each cut to
    ``(text, weight)`` (kept whole with ``return_encoded``) and given its risk with ``return_risks``: the first text alone; the
    first row with ``return_weights``, ``return_encoded`` or ``return_risks``; with ``nbest > 1`` a list of up to ``nbest``
    rows."""
    if ranks:
        order = sorted(range(len(ranks)), key=lambda i: (res.risk[u, ranks[i]], ranks[i]))
        assert ranks[order[0]] == int(res.pick[u]), (ranks, order, res.pick[u], res.risk[u])
        risks = [float(res.risk[u, ranks[i]]) for i in order]
    else:                                              # the beam emptied: the one row '' of the plain search
        order, risks = [0], [float('nan')]
    rows = []
    for i, risk in zip(order, risks):
        row = tuple(found[i]) if return_encoded else tuple(found[i][:2]) if (return_weights or nbest > 1) else (found[i][0],)
        rows.append(row + (risk,) if return_risks else row)
    if nbest > 1:
        return rows[:nbest]
    return rows[0] if len(rows[0]) > 1 else rows[0][0]


# --------------------------------------------------------------------------------------------------------------- host oracle
def mbr_select_host(rows, unit: str = 'word', scale: float = 1.0):
    """The selection of the module docstring on the host, for one utterance: ``rows`` = (text, log weight) pairs in rank order
    -> ``(pick, risks float64 [k], dist int32 [k, k])``, distances by Decoder.wer (``unit='word'``) / Decoder.cer (``'char'``),
    everything else float64 with j = 0..k-1 in order.  The oracle of the device tests."""
    from .decoder import Decoder
    check_unit(unit, 'unit')
    scale = np.float64(scale)
    dec = Decoder(['_'])
    measure = dec.wer if unit == 'word' else dec.cer
    k = len(rows)
    if k < 1:
        raise ValueError('mbr_select_host: no rows')
    dist = np.zeros((k, k), dtype=np.int32)
    for i in range(k):
        for j in range(i + 1, k):
            dist[i, j] = dist[j, i] = measure(rows[i][0], rows[j][0])
    w = [np.float64(r[1]) for r in rows]
    m = w[0]
    for v in w[1:]:
        m = max(m, v)
    with np.errstate(invalid='ignore'):
        e = [np.exp(scale * (v - m)) for v in w]
        total = np.float64(0.0)
        for v in e:
            total = total + v
        risks = np.zeros(k, dtype=np.float64)
        for i in range(k):
            r = np.float64(0.0)
            for j in range(k):
                r = r + e[j] / total * np.float64(dist[i, j])
            risks[i] = r
    pick = 0
    for i in range(1, k):
        if risks[i] < risks[pick]:                     # a tie stays with the lower rank
            pick = i
    return pick, risks, dist


# ------------------------------------------------------------------------------------------------------------------- device
def edit_distance_pairs_gpu(sequences, pairs, counts: bool = False):
    """Levenshtein distances on the MI355X, one launch (w2l_edit_distance): ``sequences``: int sequences; ``pairs``: (reference,
    hypothesis) indices into them, any sequence in any number of pairs.  -> ``dist`` int32 [P], and with ``counts``
    ``(dist, counts int32 [P, 3])``: substitutions, deletions, insertions of the module docstring's recurrence.  A sequence of
    more than 4095 tokens or an index outside the sequences is a ValueError before anything is launched."""
    import torch
    from . import _lib
    from ._lib import check, lib, ptr, stream_ptr
    seqs = [np.asarray(s, dtype=np.int32).reshape(-1) for s in sequences]
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    longest = max((len(s) for s in seqs), default=0)
    if longest > MAX_TOKENS:
        raise ValueError('edit distance: a sequence of %d tokens, the device takes at most %d' % (longest, MAX_TOKENS))
    if pr.size and (pr.min() < 0 or pr.max() >= len(seqs)):
        raise ValueError('edit distance: a pair names a sequence outside [0, %d)' % len(seqs))
    p_n = pr.shape[0]
    if p_n == 0:
        empty = np.zeros(0, dtype=np.int32)
        return (empty, np.zeros((0, 3), dtype=np.int32)) if counts else empty
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    total = int(offsets[-1])
    if int(lib.w2l_edit_distance_workspace_bytes(total, len(seqs), p_n, longest)) < 0:
        raise ValueError('edit distance: %d tokens in %d sequences, %d pairs: out of range' % (total, len(seqs), p_n))
    if not torch.cuda.is_available():
        raise _lib.W2LError('edit_distance_gpu needs the MI355X device (w2l_levenshtein_host is the host routine)')
    # one host buffer, one copy: offsets | pairs | tokens
    host = np.concatenate([offsets.astype(np.int32), pr.astype(np.int32).reshape(-1)] + seqs + [np.zeros(1, dtype=np.int32)])
    buf = torch.from_numpy(host).cuda()
    o_pairs, o_tok = len(seqs) + 1, len(seqs) + 1 + 2 * p_n
    out = torch.empty(p_n * (5 if counts else 2), dtype=torch.int32, device=buf.device)
    base = out.data_ptr()
    vp = C.c_void_p
    check(lib.w2l_edit_distance(vp(buf.data_ptr() + 4 * o_tok), total, ptr(buf), len(seqs), vp(buf.data_ptr() + 4 * o_pairs), p_n,
                                longest, None, 0, vp(base), vp(base + 8 * p_n) if counts else None, vp(base + 4 * p_n),
                                stream_ptr()), 'w2l_edit_distance')
    got = out.cpu().numpy()
    dist, status = got[:p_n], got[p_n:2 * p_n]
    if status.any():
        raise _lib.W2LError('w2l_edit_distance refused pairs %s (status %s)'
                            % (np.nonzero(status)[0].tolist()[:8], status[status != 0].tolist()[:8]))
    return (dist, got[2 * p_n:].reshape(p_n, 3)) if counts else dist


def edit_distance_gpu(refs, hyps, unit: str = 'word', counts: bool = False):
    """Edit distances of ``refs[i]`` against ``hyps[i]`` on the MI355X in one launch.  An item is a string -- tokenised as
    Decoder.wer (``unit='word'``: ``str.split()``, the words interned on the host) or Decoder.cer (``'char'``: ' ' removed)
    does -- or a sequence of ints, taken as it is.  -> ``dist`` int32 [P], or ``(dist, counts)`` with ``counts``: int32 [P, 3],
    (substitutions, deletions, insertions) of turning the reference into the hypothesis.  A sequence of more than 4095 tokens
    is a ValueError before anything is launched."""
    check_unit(unit, 'unit')
    if isinstance(refs, str) or isinstance(hyps, str):
        raise TypeError('edit_distance_gpu takes lists: refs[i] is scored against hyps[i]')
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError('edit_distance_gpu: %d references for %d hypotheses' % (len(refs), len(hyps)))
    vocab = {}

    def tokens(item):
        if not isinstance(item, str):
            return np.asarray(item, dtype=np.int32).reshape(-1)
        if unit == 'word':
            return np.array([vocab.setdefault(w, len(vocab)) for w in words_of(item)], dtype=np.int32)
        return np.array([ord(c) for c in chars_of(item)], dtype=np.int32)

    seqs = [tokens(r) for r in refs] + [tokens(h) for h in hyps]
    p_n = len(refs)
    return edit_distance_pairs_gpu(seqs, [(i, p_n + i) for i in range(p_n)], counts=counts)

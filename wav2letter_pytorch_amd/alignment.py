"""CTC forced alignment: the best frame path of a GIVEN label sequence (the Viterbi, max-instead-of-sum, form of the CTC
recursion).  It is what gives a beam-search result character offsets -- a beam result sums over many frame paths and has
none of its own (the reference stops at decoder.py:238, "Prefix beam search does not support offsets (yet)") -- and what
aligns a known transcript to the posteriors (segmenting a corpus, word start AND end times).

ctc_forced_align runs one HIP launch for a batch (w2l_ctc_align, csrc/ctc_align.hip); viterbi_align_host is the same recursion
in NumPy, the model the device tests compare with.  Both keep the same tie rules: among equal predecessors the state itself
(stay), then s-1, then s-2; at the end the last label's state before the trailing blank's; a state whose best predecessor is
-inf stays -inf."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

HostAlignment = namedtuple('HostAlignment', 'score path starts ends feasible')
HostAlignment.__doc__ = """viterbi_align_host's result: ``score`` (best-path log-probability, -inf if infeasible), ``path`` [T] (the label
emitted at each frame), ``starts`` / ends`` [S] (first / last frame of each target token), ``feasible``.  An infeasible target
has path, starts and ends filled with -1."""


class Alignment(object):
    """ctc_forced_align's result, host arrays: ``scores`` float32 [N], ``feasible`` bool [N], ``paths`` int32 [N, T] (label per
    frame, -1 past an utterance's frames), ``starts`` / ``ends`` int32 [N, Smax] (first / last frame of each target token, -1
    past a target's length).  An infeasible utterance has score -inf and -1 everywhere."""
    __slots__ = ('scores', 'feasible', 'paths', 'starts', 'ends', 'target_lengths')

    def __init__(self, scores, feasible, paths, starts, ends, target_lengths):
        self.scores, self.feasible, self.paths, self.starts, self.ends = scores, feasible, paths, starts, ends
        self.target_lengths = target_lengths

    def __repr__(self):
        return 'Alignment(N=%d, T=%d, feasible=%d)' % (self.paths.shape[0], self.paths.shape[1], int(self.feasible.sum()))


def viterbi_align_host(lp, target, blank: int = 0, dtype=np.float64) -> HostAlignment:
    """Best CTC path of ``target`` (a sequence of label indices, none equal to ``blank``) over the frames of ``lp`` [T, A]
    (log-probabilities; -inf allowed), vectorised over the 2 S + 1 extended states, one Python iteration per frame.  With
    ``dtype=np.float32`` the arithmetic is w2l_ctc_align's, add for add and compare for compare."""
    dtype = np.dtype(dtype).type
    lp = np.asarray(lp).astype(dtype, copy=False)
    if lp.ndim != 2 or lp.shape[0] < 1:
        raise ValueError('viterbi_align_host: expected [T >= 1, A] log-probabilities, got shape %s' % (lp.shape,))
    t_n, a = lp.shape
    tg = np.asarray(target, dtype=np.int64).reshape(-1)
    if not 0 <= blank < a:
        raise ValueError('blank %d outside %d labels' % (blank, a))
    if tg.size and (tg.min() < 0 or tg.max() >= a or (tg == blank).any()):
        raise ValueError('viterbi_align_host: a target lies outside [0, %d) or equals the blank (%d)' % (a, blank))
    s_n = tg.size
    n_st = 2 * s_n + 1
    ext = np.full(n_st, blank, dtype=np.int64)
    ext[1::2] = tg
    skip = np.zeros(n_st, dtype=bool)
    if s_n > 1:
        skip[3::2] = tg[1:] != tg[:-1]
    ninf = dtype(-np.inf)
    score = np.full(n_st, ninf, dtype=dtype)
    score[:2] = lp[0, ext[:2]]
    moves = np.zeros((t_n, n_st), dtype=np.uint8)
    a1 = np.full(n_st, ninf, dtype=dtype)
    a2 = np.full(n_st, ninf, dtype=dtype)
    with np.errstate(invalid='ignore'):
        for t in range(1, t_n):
            a1[1:] = score[:-1]
            if n_st > 2:
                a2[2:] = score[:-2]
                a2[~skip] = ninf
            best = score.copy()
            mv = moves[t]
            m = a1 > best                               # ties: stay, then s-1, then s-2
            best[m] = a1[m]
            mv[m] = 1
            m = a2 > best
            best[m] = a2[m]
            mv[m] = 2
            new = best + lp[t, ext]
            new[best == ninf] = ninf
            score = new
    end = n_st - 1
    if n_st > 1 and score[n_st - 2] >= score[n_st - 1]:  # the last label wins a tie with the trailing blank
        end = n_st - 2
    best = score[end]
    if not best > ninf:
        none = np.full(s_n, -1, dtype=np.int32)
        return HostAlignment(dtype(-np.inf), np.full(t_n, -1, dtype=np.int32), none, none.copy(), False)
    states = np.empty(t_n, dtype=np.int64)
    s = end
    for t in range(t_n - 1, 0, -1):
        states[t] = s
        s -= int(moves[t, s])
    states[0] = s
    path = ext[states].astype(np.int32)
    starts = np.full(s_n, -1, dtype=np.int32)
    ends = np.full(s_n, -1, dtype=np.int32)
    own = (states & 1) == 1
    first = own & np.concatenate(([True], states[1:] != states[:-1]))
    last = own & np.concatenate((states[1:] != states[:-1], [True]))
    starts[states[first] >> 1] = np.nonzero(first)[0]
    ends[states[last] >> 1] = np.nonzero(last)[0]
    return HostAlignment(best, path, starts, ends, True)


def _first_index(labels):
    first = {}
    for i, ch in enumerate(labels):
        first.setdefault(ch, i)
    return first


def _targets_to_array(targets, target_lengths, labels, n_expected: Optional[int]):
    """-> (int32 [N, Smax] padded with 0, int32 [N] lengths) on the host"""
    import torch
    if torch.is_tensor(targets):
        targets = targets.detach().cpu().numpy()
    if isinstance(targets, str):
        targets = [targets]
    if isinstance(targets, np.ndarray):
        if not np.issubdtype(targets.dtype, np.integer):
            raise ValueError('ctc_forced_align: targets must be integers, got %s' % targets.dtype)
        rows = targets.reshape(1, -1) if targets.ndim == 1 else targets
        if rows.ndim != 2:
            raise ValueError('ctc_forced_align: padded targets must be [N, Smax], got shape %s' % (targets.shape,))
        if target_lengths is None:
            lengths = np.full(rows.shape[0], rows.shape[1], dtype=np.int32)
        else:
            if torch.is_tensor(target_lengths):
                target_lengths = target_lengths.detach().cpu().numpy()
            lengths = np.asarray(target_lengths, dtype=np.int64).reshape(-1)
            if lengths.size != rows.shape[0]:
                raise ValueError('target_lengths holds %d lengths for %d targets' % (lengths.size, rows.shape[0]))
            if lengths.size and (lengths.min() < 0 or lengths.max() > rows.shape[1]):
                raise ValueError('target_lengths must lie in [0, %d], got %s' % (rows.shape[1], lengths.tolist()))
            lengths = lengths.astype(np.int32)
        return np.ascontiguousarray(rows, dtype=np.int32), lengths
    if target_lengths is not None:
        raise ValueError('ctc_forced_align: target_lengths goes with padded targets only (a list carries its own lengths)')
    targets = list(targets)
    if targets and isinstance(targets[0], (int, np.integer)):          # one utterance's labels
        targets = [targets]
    rows = []
    first = _first_index(labels) if labels is not None else None
    for row in targets:
        if isinstance(row, str):
            if first is None:
                raise ValueError('ctc_forced_align: string targets need ``labels``')
            try:
                rows.append([first[ch] for ch in row])
            except KeyError as e:
                raise ValueError('ctc_forced_align: character %r of %r is not in the labels' % (e.args[0], row)) from None
        else:
            rows.append([int(v) for v in row])
    lengths = np.array([len(r) for r in rows], dtype=np.int32)
    out = np.zeros((len(rows), int(lengths.max()) if len(rows) else 0), dtype=np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, lengths


def align_sections(n: int, t: int, smax: int):
    """byte offsets (score, status, path, starts, ends, total) of w2l_ctc_align's outputs inside one buffer"""
    o_status = 4 * n
    o_path = o_status + 4 * n
    o_starts = o_path + 4 * n * t
    o_ends = o_starts + 4 * n * smax
    return 0, o_status, o_path, o_starts, o_ends, o_ends + 4 * n * smax


def _launch(symbol: str, ws_bytes: int, out_of_range: str, head, x, sz, tg_ptr, tg_stride, len_ptr, len_stride, smax, flags, out,
            out_offset: int):
    """the launch behind launch_align and asg_beam.launch_asg_align.  ``ws_bytes``: the answer of the symbol's workspace query
    (negative: ``out_of_range`` is raised); ``head``: the symbol's leading pointer arguments; ``flags``: its two ints after Smax"""
    import torch
    from . import _lib
    from ._lib import check, lib, ptr, stream_ptr
    n, t, a = x.shape
    if ws_bytes < 0:
        raise _lib.W2LError(out_of_range)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    vp = C.c_void_p
    sections = [vp(out.data_ptr() + out_offset + o) for o in align_sections(n, t, smax)[:5]]
    check(getattr(lib, symbol)(*head, ptr(sz), vp(tg_ptr), int(tg_stride), vp(len_ptr), int(len_stride), n, t, a, int(smax),
                               *flags, ptr(ws), ws_bytes, *sections, stream_ptr()), symbol)
    return ws


def launch_align(x, sz, tg_ptr: int, tg_stride: int, len_ptr: int, len_stride: int, smax: int, blank: int, log_probs: bool,
                 out, out_offset: int):
    """one w2l_ctc_align launch on the current stream: x [N, T, A] float32 contiguous on the device, ``sz`` int32 [N] there or
    None, targets / lengths by device address and stride (elements), outputs into ``out`` (a uint8 device tensor) from byte
    ``out_offset`` in align_sections' layout.  -> the workspace tensor (or None): keep it alive until the stream has passed."""
    from ._lib import lib, ptr
    n, t, _ = x.shape
    return _launch('w2l_ctc_align', lib.w2l_ctc_align_workspace_bytes(n, t, smax),
                   'ctc_forced_align: T=%d (max 32768) or target length %d (max 4095) is out of range' % (t, smax), (ptr(x),),
                   x, sz, tg_ptr, tg_stride, len_ptr, len_stride, smax, (int(blank), int(bool(log_probs))), out, out_offset)


def split_align(host: np.ndarray, n: int, t: int, smax: int):
    """the host copy of align_sections' bytes -> (scores, status, paths, starts, ends)"""
    o = align_sections(n, t, smax)
    scores = host[o[0]:o[1]].view(np.float32)
    status = host[o[1]:o[2]].view(np.int32)
    paths = host[o[2]:o[3]].view(np.int32).reshape(n, t)
    starts = host[o[3]:o[4]].view(np.int32).reshape(n, smax)
    ends = host[o[4]:o[5]].view(np.int32).reshape(n, smax)
    return scores, status, paths, starts, ends


def batch_of(x, lengths):
    """``x`` as a tensor with a [T, A] input promoted to [1, T, A], its one length (if any) along with it -> (x, lengths,
    whether it was promoted)"""
    import torch
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    single = x.dim() == 2
    if single:
        x = x.unsqueeze(0)
        if lengths is not None:
            lengths = [int(np.asarray(torch.as_tensor(lengths).cpu()).reshape(-1)[0])]
    return x, lengths, single


def host_lengths(lengths, n: int, t: int, what: str):
    """``lengths`` as an int32 host tensor [N] with every entry in [1, T]"""
    import torch
    host = torch.as_tensor(lengths).detach().cpu().to(torch.int64).reshape(-1)
    if host.numel() != n:
        raise ValueError('%s holds %d lengths for %d utterances' % (what, host.numel(), n))
    if bool((host < 1).any()) or bool((host > t).any()):
        raise ValueError('%s must lie in [1, %d], got %s' % (what, t, host.tolist()))
    return host.to(torch.int32)


def on_device(x, what: str, hint: str = ''):
    """``x`` (numpy or torch) as a contiguous float32 tensor on the device"""
    import torch
    from . import _lib
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.W2LError('%s needs the MI355X device (there is no CPU fallback%s)' % (what, hint))
        x = x.cuda()
    return x.detach().float().contiguous()


def align_targets(targets, target_lengths, labels, n: int, t: int, what: str):
    """the targets of ``n`` utterances of ``t`` frames as arrays, within the kernels' limits -> (targets [N, Smax], lengths, Smax)"""
    tg, tl = _targets_to_array(targets, target_lengths, labels, n)
    if tg.shape[0] != n:
        raise ValueError('%d targets for %d utterances' % (tg.shape[0], n))
    smax = tg.shape[1]
    if smax > 4095 or t > 32768:
        raise ValueError('%s: T=%d (max 32768) or target length %d (max 4095) is out of range' % (what, t, smax))
    return tg, tl, smax


def align_buffers(x, il, tg, tl):
    """for x [N, T, A] on the device: the input lengths there (or None), the targets with their lengths in one buffer
    [N * Smax | N] int32, and the launch's ``out`` in align_sections' layout"""
    import torch
    sz = il.to(x.device, non_blocking=True) if il is not None else None
    tgt = torch.from_numpy(np.concatenate([tg.reshape(-1), tl])).to(x.device, non_blocking=True)
    return sz, tgt, torch.empty(align_sections(x.shape[0], x.shape[1], tg.shape[1])[5], dtype=torch.uint8, device=x.device)


def aligned(out, n: int, t: int, smax: int, tl, bad_input: str):
    """the one copy to the host of a launch's ``out`` (ordered after the launch on this stream) -> Alignment; a row of status 2
    raises ValueError(bad_input % rows)"""
    scores, status, paths, starts, ends = split_align(out.cpu().numpy(), n, t, smax)
    if (status == 2).any():
        raise ValueError(bad_input % (np.nonzero(status == 2)[0].tolist(),))
    return Alignment(scores, status == 0, paths, starts, ends, tl)


def ctc_forced_align(probs, targets, input_lengths=None, target_lengths=None, blank: int = 0, log_probs: bool = True,
                     labels: Optional[Sequence[str]] = None) -> Alignment:
    """Align each utterance's target to its posteriors on the MI355X: one launch, one copy to the host.

    probs: [N, T, A] or [T, A] (numpy or torch, any device; log-probabilities, or probabilities if not ``log_probs``);
    targets: padded int tensor / array [N, Smax] with ``target_lengths``, a list of int lists, or -- with ``labels`` -- a list
    of strings (a character maps to its first index in ``labels``, as in the decoders; an unknown one is a ValueError);
    input_lengths[n]: the frames of utterance n (default: all T).  An utterance whose target has no path of finite score
    (more labels, counting one blank between repeated ones, than frames; or a zero probability on every path) does not
    raise: ``feasible[n]`` is False and ``scores[n]`` -inf.  A negative probability, or a target outside [0, A) or equal to
    ``blank``, is a ValueError."""
    x, input_lengths, _ = batch_of(probs, input_lengths)
    if x.dim() != 3:
        raise ValueError('expected [N, T, labels] or [T, labels] posteriors, got shape %s' % (tuple(x.shape),))
    n, t, a = x.shape
    if n < 1 or t < 1 or a < 1:
        raise ValueError('ctc_forced_align: empty posteriors, shape %s' % (tuple(x.shape),))
    if labels is not None and len(labels) != a:
        raise ValueError('ctc size:%d, labels: %d' % (a, len(labels)))
    if not 0 <= blank < a:
        raise ValueError('blank %d outside %d labels' % (blank, a))
    tg, tl, smax = align_targets(targets, target_lengths, labels, n, t, 'ctc_forced_align')
    il = host_lengths(input_lengths, n, t, 'input_lengths') if input_lengths is not None else None
    x = on_device(x, 'ctc_forced_align', '; viterbi_align_host is the host model')
    sz, tgt, out = align_buffers(x, il, tg, tl)
    ws = launch_align(x, sz, tgt.data_ptr(), max(smax, 1), tgt.data_ptr() + 4 * n * smax, 1, smax, blank, log_probs, out, 0)
    got = aligned(out, n, t, smax, tl, 'ctc_forced_align: a negative probability, or a target outside [0, %d) or equal to the '
                  'blank (%d), in utterances %%s' % (a, blank))
    del ws
    return got


# ------------------------------------------------------------------------------------------ one long recording, whole transcript
LONG_MAX_T, LONG_MAX_S = 1 << 22, 1 << 20      # W2L_ALIGN_LONG_MAX_T / _MAX_S
LONG_MAX_TB, LONG_MAX_SB = 256, 2048           # W2L_ALIGN_LONG_MAX_TB / _MAX_SB
LONG_PLAN = (64, 128)                          # W2L_ALIGN_LONG_TB / _SB: what plan=None runs
# the (tb, sb) pairs tools/bench_align_long.py measures and the default is picked from (DESIGN 8s has the table)
LONG_CANDIDATES = [(32, 64), (32, 192), (64, 64), (64, 128), (64, 384), (64, 896), (96, 64), (128, 128), (128, 256), (128, 768),
                   (128, 1024), (256, 512), (256, 1536)]


def long_workspace_bytes(t: int, s: int, tb: int, sb: int) -> int:
    """w2l_ctc_align_long_workspace_bytes on the host (the formula of include/w2l_hip.h; tb, sb as launched, not 0)"""
    lp = -(-(2 * s + 1) // sb) * sb
    return 16 + 2 * lp * 4 + -(-t * 4 // 16) * 16 + -(-t // 16) * lp * 4


def _long_target(target, labels):
    """one int sequence, or a string with ``labels`` -> int32 [S]"""
    import torch
    if torch.is_tensor(target):
        target = target.detach().cpu().numpy()
    if isinstance(target, str):
        if labels is None:
            raise ValueError('ctc_forced_align_long: a string target needs ``labels``')
        first = _first_index(labels)
        try:
            return np.array([first[ch] for ch in target], dtype=np.int32)
        except KeyError as e:
            raise ValueError('ctc_forced_align_long: character %r is not in the labels' % (e.args[0],)) from None
    tg = np.asarray(target)
    if tg.size == 0:
        return np.zeros(0, dtype=np.int32)
    if tg.ndim != 1 or not np.issubdtype(tg.dtype, np.integer):
        raise ValueError('ctc_forced_align_long: the target is ONE sequence of integers (or a string with labels), got shape %s '
                         'of %s' % (tg.shape, tg.dtype))
    return np.ascontiguousarray(tg.clip(-1, 1 << 30), dtype=np.int32)      # (anything out of range stays out of range)


def launch_align_long(x, tgt, s: int, blank: int, log_probs: bool, plan, ws, out):
    """the launches of w2l_ctc_align_long on the current stream: x [T, A] float32 contiguous and ``tgt`` int32 [S] on the device,
    ``ws`` a uint8 device tensor of long_workspace_bytes, outputs into ``out`` in align_sections(1, T, S)'s layout"""
    from ._lib import check, lib, ptr, stream_ptr
    t, a = x.shape
    tb, sb = plan if plan is not None else (0, 0)
    vp = C.c_void_p
    sections = [vp(out.data_ptr() + o) for o in align_sections(1, t, s)[:5]]
    check(lib.w2l_ctc_align_long(ptr(x), t, a, ptr(tgt) if s else None, s, int(blank), int(bool(log_probs)), int(tb), int(sb),
                                 ptr(ws), int(ws.numel()), *sections, stream_ptr()), 'w2l_ctc_align_long')


def ctc_forced_align_long(probs, target, blank: int = 0, log_probs: bool = True, labels: Optional[Sequence[str]] = None,
                          plan=None, max_workspace_bytes: int = 8 << 30) -> Alignment:
    """ctc_forced_align for ONE recording of any length up to 2^22 frames against its whole transcript of up to 2^20 labels
    (w2l_ctc_align_long, csrc/ctc_align_long.hip: the trellis cut into time blocks and state tiles, many workgroups), bit-equal
    to ctc_forced_align wherever both take the shape.

    probs: [T, A]; target: one int sequence, or a string with ``labels``; ``plan=(tb, sb)`` forces the cut (tb a multiple of
    16 up to 256 frames, sb a multiple of 64 up to 2048 states; default: the measured one).  -> an Alignment with N = 1.
    Errors as ctc_forced_align's: bad input is a ValueError, no path is ``feasible[0] == False``.  The workspace holds two bits
    per trellis cell (about T * S / 4 bytes: 4.5 GB for an hour with 50 000 characters); above ``max_workspace_bytes`` (8 GiB by
    convention, not tuned) it is a ValueError that states the bytes.  Argument errors come before the device is looked for."""
    import torch
    x = probs if torch.is_tensor(probs) else torch.from_numpy(np.ascontiguousarray(probs))
    if x.dim() != 2:
        raise ValueError('ctc_forced_align_long: expected [T, labels] posteriors of one recording, got shape %s' % (tuple(x.shape),))
    t, a = x.shape
    if t < 1 or a < 1:
        raise ValueError('ctc_forced_align_long: empty posteriors, shape %s' % (tuple(x.shape),))
    if labels is not None and len(labels) != a:
        raise ValueError('ctc size:%d, labels: %d' % (a, len(labels)))
    if not 0 <= blank < a:
        raise ValueError('blank %d outside %d labels' % (blank, a))
    tg = _long_target(target, labels)
    s = int(tg.size)
    if t > LONG_MAX_T or s > LONG_MAX_S:
        raise ValueError('ctc_forced_align_long: T=%d (max %d) or target length %d (max %d) is out of range'
                         % (t, LONG_MAX_T, s, LONG_MAX_S))
    if plan is not None:
        try:
            tb, sb = (int(v) for v in plan)
        except (TypeError, ValueError):
            raise ValueError('ctc_forced_align_long: plan=%r is not a (tb, sb) pair' % (plan,)) from None
        if not (16 <= tb <= LONG_MAX_TB and tb % 16 == 0 and 64 <= sb <= LONG_MAX_SB and sb % 64 == 0):
            raise ValueError('ctc_forced_align_long: plan=(%d, %d): tb is a multiple of 16 in 16..%d, sb a multiple of 64 in 64..%d'
                             % (tb, sb, LONG_MAX_TB, LONG_MAX_SB))
        plan = (tb, sb)
    need = long_workspace_bytes(t, s, *(plan or LONG_PLAN))
    if need > max_workspace_bytes:
        raise ValueError('ctc_forced_align_long: T=%d frames x %d labels need a workspace of %d bytes, above max_workspace_bytes=%d'
                         % (t, s, need, max_workspace_bytes))
    x = on_device(x, 'ctc_forced_align_long', '; viterbi_align_host is the host model')
    from ._lib import lib
    with torch.cuda.device(x.device):
        if int(lib.w2l_ctc_align_long_workspace_bytes(t, s, *(plan or (0, 0)))) != need:
            raise RuntimeError('ctc_forced_align_long: the library plans %d workspace bytes, alignment.py %d'
                               % (lib.w2l_ctc_align_long_workspace_bytes(t, s, *(plan or (0, 0))), need))
        tgt = torch.from_numpy(tg).to(x.device, non_blocking=True)
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        out = torch.empty(align_sections(1, t, s)[5], dtype=torch.uint8, device=x.device)
        launch_align_long(x, tgt, s, blank, log_probs, plan, ws, out)
        got = aligned(out, 1, t, s, np.array([s], dtype=np.int32), 'ctc_forced_align_long: a negative probability, or a target '
                      'outside [0, %d) or equal to the blank (%d), in utterances %%s' % (a, blank))
    del ws
    return got

"""Auto Segmentation criterion (ASG) and its Viterbi decoder: the loss the Wav2Letter paper trains with, which the reference
replaces by CTC (its README, "Differences from article").  Selected by ``model.criterion: asg``; the default stays CTC.

ASG has no blank label.  It owns a learned ``[A, A]`` transition matrix ``g`` (``g[i, j]``: label j at frame t after label i at
frame t-1, no start or end scores) and is normalised over ALL label paths:

    loss_n = Z_full - Z_tgt
    Z_full = logsumexp over the A^T frame paths pi of  sum_t x[t, pi_t] + sum_{t>=1} g[pi_{t-1}, pi_t]
    Z_tgt  = the same sum over the paths that read the encoded target, every label held for at least one frame

Without a blank a doubled letter would read like a long one, so label index 0 -- this project's blank slot ``'_'`` -- is reused
as "the previous letter again": within a run of equal labels the 2nd, 4th, ... member becomes 0 (``hello -> hel_o``,
``lll -> l_l``).  The loss kernel encodes raw transcripts on the device; ``encode_repeats`` / ``decode_repeats`` are the host
reference of that rule and the core of the decoder.

Kernels: csrc/asg.hip (w2l_asg_loss, w2l_asg_viterbi).  There is no CPU path.  The prefix beam search (with an n-gram model),
n-best lists and forced alignment of an ASG model live in asg_beam.py (csrc/asg_beam.hip)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .decoder import Decoder

MAX_LABELS = 64
REDUCTIONS = {'mean': 0, 'sum': 1}


def encode_repeats(labels, repeat: int = 0):
    """within a run of equal labels the 2nd, 4th, ... member becomes ``repeat``; same length, no two neighbours equal.
    A transcript that already contains ``repeat`` is a ValueError."""
    out, prev, run = [], None, 0
    for v in labels:
        v = int(v)
        if v == repeat:
            raise ValueError(f'encode_repeats: the transcript contains the repeat label {repeat}')
        run = run + 1 if v == prev else 0
        out.append(repeat if run & 1 else v)
        prev = v
    return out


def decode_repeats(labels, repeat: int = 0):
    """inverse of ``encode_repeats`` on a collapsed label sequence: every ``repeat`` becomes the label before it; a leading
    ``repeat`` is dropped"""
    out = []
    for v in labels:
        v = int(v)
        if v != repeat:
            out.append(v)
        elif out:
            out.append(out[-1])
    return out


def collapse_frames(path):
    """frame path -> (labels with consecutive equal frames merged, the first frame of each)"""
    seq = np.asarray(path, dtype=np.int64)
    if len(seq) == 0:
        return [], []
    keep = np.ones(len(seq), dtype=bool)
    keep[1:] = seq[1:] != seq[:-1]
    return seq[keep].tolist(), np.nonzero(keep)[0].tolist()


def _check_labels(num_labels: int, what: str):
    if not 1 <= int(num_labels) <= MAX_LABELS:
        raise ValueError(f'{what}: {num_labels} labels; the ASG kernels hold one label per lane of a wave (1 to {MAX_LABELS})')


class _ASGFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, transitions, targets, input_lengths, target_lengths, repeat_index, reduction):
        # log_probs arrives as [T, N, C], as for CTCLoss; the kernels are batch-major
        _lib.require_device(log_probs, transitions)
        x = log_probs.detach().transpose(0, 1)
        if not x.is_contiguous() or x.dtype != torch.float32:
            x = x.contiguous().float()
        n, t, a = x.shape
        dev = x.device
        g = transitions.detach()
        if tuple(g.shape) != (a, a):
            raise ValueError(f'ASGLoss: transitions of shape {tuple(g.shape)} for {a} labels')
        if not g.is_contiguous() or g.dtype != torch.float32 or g.device != dev:
            g = g.to(device=dev, dtype=torch.float32).contiguous()
        if targets.dim() != 2:
            raise NotImplementedError('ASGLoss: targets must be 2-D [N, S_max] (padded), as the collator produces')
        tg = targets.to(device=dev, dtype=torch.int32).contiguous()
        il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int32).contiguous()
        tl = torch.as_tensor(target_lengths).to(device=dev, dtype=torch.int32).contiguous()
        smax = tg.shape[1]
        need = int(lib.w2l_asg_workspace_bytes(n, t, a, smax))
        if need < 0:
            raise ValueError(f'ASGLoss: N={n} T={t} labels={a} (max {MAX_LABELS}) S_max={smax} (max 4095) out of range')
        want_grad = any(ctx.needs_input_grad[:2])
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        nll = torch.empty(n, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        grad_x = torch.empty(n, t, a, dtype=torch.float32, device=dev) if want_grad else None
        grad_g = torch.empty(a, a, dtype=torch.float32, device=dev) if want_grad else None
        check(lib.w2l_asg_loss(ptr(x), ptr(g), ptr(tg), ptr(il), ptr(tl), n, t, a, smax, int(repeat_index),
                               REDUCTIONS[reduction], ptr(nll), ptr(loss), ptr(grad_x), ptr(grad_g), ptr(status), ptr(ws), need,
                               stream_ptr()), 'w2l_asg_loss')
        # the one host read of the call: a transcript the encoding cannot represent must not train silently
        bad = np.nonzero(status.cpu().numpy() == 2)[0]
        if len(bad):
            raise ValueError(f'ASGLoss: the transcripts of utterances {bad.tolist()} contain the repeat label {int(repeat_index)} '
                             f'or a label outside [0, {a})')
        ctx.grad_x, ctx.grad_g = grad_x, grad_g
        ctx.nll = nll
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        gx = (ctx.grad_x * gout).transpose(0, 1) if ctx.needs_input_grad[0] else None
        gg = ctx.grad_g * gout if ctx.needs_input_grad[1] else None
        return gx, gg, None, None, None, None, None


class ASGLoss(nn.Module):
    """ASG criterion with ``CTCLoss.forward``'s signature and layouts: log_probs ``[T, N, C]`` (any real scores), targets
    ``[N, S_max]`` padded RAW transcripts (the repetition encoding happens on the device), lengths ``[N]``.  Owns
    ``transitions`` (``[C, C]`` fp32, zeros at first).  ``'mean'`` is ``mean_n(loss_n / max(S_n, 1))`` -- CTCLoss's convention,
    so learning rates carry over --, ``'sum'`` is ``sum_n loss_n``.  An utterance with ``S = 0`` or ``S > T_n`` contributes loss
    and gradient 0, as ``zero_infinity=True`` does for CTC.  Each call reads one small status vector back (a host
    synchronisation): a transcript that contains ``repeat_index`` or a label outside ``[0, C)`` is a ValueError.

    Accuracy: alpha, beta and Z are kept in the log domain in fp32 as they grow (as the CTC kernels keep theirs), so the error
    of the gradients follows the magnitude ``|Z| ~ T * mean|x|``, not the label count: a posterior inherits a few fp32 ulp of
    ``|Z|`` as relative error.  Measured against float64: below 1e-4 of the gradients' scale up to ``|Z|`` of a few hundred
    (T = 40 log-probabilities), 2e-4 .. 4e-4 at ``|Z|`` ~ 4e2 .. 4e3 (T = 140, or emissions scaled by 30), and on the
    transition gradient 2.4e-3 at N = 32, T = 500 and 1.2e-3 at T = 1100 (``|Z|`` ~ 2e3 .. 3e3); the loss itself stays within
    1e-6 relative throughout."""
    is_asg = True

    def __init__(self, num_labels, repeat_index=0, reduction='mean'):
        super().__init__()
        _check_labels(num_labels, 'ASGLoss')
        if reduction not in REDUCTIONS:
            raise NotImplementedError(f"ASGLoss: reduction {reduction!r}; 'mean' and 'sum' are implemented")
        if not 0 <= int(repeat_index) < int(num_labels):
            raise ValueError(f'ASGLoss: repeat_index {repeat_index} outside [0, {num_labels})')
        self.num_labels = int(num_labels)
        self.repeat_index = int(repeat_index)
        self.reduction = reduction
        self.transitions = nn.Parameter(torch.zeros(self.num_labels, self.num_labels, dtype=torch.float32))

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return _ASGFn.apply(log_probs, self.transitions, targets, input_lengths, target_lengths, self.repeat_index,
                            self.reduction)


def viterbi_paths(x, transitions=None, sizes=None):
    """best frame paths on the device: x ``[N, T, A]`` scores -> (int32 ``[N, T]`` labels, -1 from ``sizes[n]`` on; fp32 ``[N]``
    path scores).  ``transitions=None`` means zeros (the per-frame argmax)."""
    _lib.require_device(x)
    x = x.detach()
    if not x.is_contiguous() or x.dtype != torch.float32:
        x = x.contiguous().float()
    n, t, a = x.shape
    dev = x.device
    need = int(lib.w2l_asg_viterbi_workspace_bytes(n, t, a))
    if need < 0:
        raise ValueError(f'ASG Viterbi: N={n} T={t} labels={a} (max {MAX_LABELS}) out of range')
    if transitions is None:
        g = torch.zeros(a, a, dtype=torch.float32, device=dev)
    else:
        g = transitions.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(g.shape) != (a, a):
            raise ValueError(f'ASG Viterbi: transitions of shape {tuple(g.shape)} for {a} labels')
    il = None if sizes is None else torch.as_tensor(sizes).to(device=dev, dtype=torch.int32).contiguous()
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    path = torch.empty(n, t, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib.w2l_asg_viterbi(ptr(x), ptr(g), ptr(il), n, t, a, ptr(ws), need, ptr(path), ptr(score), stream_ptr()),
          'w2l_asg_viterbi')
    return path, score


class ASGDecoder(Decoder):
    """Viterbi decoding with the learned transitions: the best frame path (w2l_asg_viterbi), consecutive equal frames merged,
    every repeat label replaced by the letter before it.  Return values as ``GreedyDecoder.decode``: one string per utterance,
    and with ``return_offsets`` the first frame of each emitted character as ``[[IntTensor]]``."""

    def __init__(self, labels, repeat_index=0, transitions=None):
        super().__init__(labels, blank_index=repeat_index)
        _check_labels(len(self.labels), 'ASGDecoder')
        self.repeat_index = int(repeat_index)
        self.transitions = transitions            # a tensor, or the ASGLoss module whose transitions are read at every call

    def process_path(self, path):
        """one frame path (valid frames only) -> (text, first frames)"""
        labs, firsts = collapse_frames(path)
        if labs and labs[0] == self.repeat_index:
            labs, firsts = labs[1:], firsts[1:]
        chars = [' ' if i == self.space_index else self.int_to_char[int(i)] for i in decode_repeats(labs, self.repeat_index)]
        return ''.join(chars), torch.IntTensor(np.asarray(firsts, dtype=np.int32))

    def decode(self, probs, sizes=None, transitions=None, return_offsets=False):
        if len(probs.shape) == 2:
            return self.decode(probs.unsqueeze(0), sizes, transitions, return_offsets)
        if not probs.is_cuda:
            if not torch.cuda.is_available():
                raise _lib.W2LError('ASGDecoder needs the MI355X device (no CPU fallback)')
            probs = probs.cuda()
        if transitions is None:
            transitions = self.transitions
        if isinstance(transitions, nn.Module):        # bound to a criterion: whatever Parameter it holds now
            transitions = transitions.transitions
        path, _ = viterbi_paths(probs, transitions, sizes)
        host = path.cpu().numpy()                 # the one D2H copy of the call
        if sizes is not None and torch.is_tensor(sizes):
            sizes = sizes.detach().cpu()
        decoded = [self.process_path(row[: len(row) if sizes is None else int(sizes[n])]) for n, row in enumerate(host)]
        strings = [text for text, _ in decoded]
        if return_offsets:
            return strings, [[frames] for _, frames in decoded]
        return strings

    def align(self, probs, texts, sizes=None, transitions=None):
        """forced alignment of ``texts`` (one string per utterance, or one string for a [T, labels] input) to the scores under
        ASG (asg_beam.asg_forced_align: the texts are repeat-encoded on the device) -> ``(offsets, end_offsets)`` in
        ``Decoder.align``'s format: ``offsets[n] = [IntTensor]``, the first frame of each character of texts[n], ``end_offsets``
        its last, so ``get_time_per_word(text, starts, ratio, end_offsets=ends)`` applies.  A text that no frame path spells (empty,
        or more characters than frames) is a ValueError."""
        from .asg_beam import asg_forced_align
        if isinstance(texts, str):
            texts = [texts]
        res = asg_forced_align(probs, self.transitions if transitions is None else transitions, list(texts),
                               input_lengths=sizes, labels=list(self.labels), repeat_index=self.repeat_index)
        if not res.feasible.all():
            raise ValueError('ASGDecoder.align: no frame path spells the texts of utterances %s'
                             % np.nonzero(~res.feasible)[0].tolist())
        offsets = [[torch.IntTensor(res.starts[n, :len(text)].copy())] for n, text in enumerate(texts)]
        end_offsets = [[torch.IntTensor(res.ends[n, :len(text)].copy())] for n, text in enumerate(texts)]
        return offsets, end_offsets

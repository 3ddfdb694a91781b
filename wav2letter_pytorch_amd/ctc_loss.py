"""nn.CTCLoss replacement backed by the alpha-beta HIP kernels (base_asr_models.py:23,81,90), and its wildcard form."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib, ptr, stream_ptr


def _operands(name, workspace_bytes, log_probs, targets, input_lengths, target_lengths):
    """what both loss entry points take: the batch-major operands (lp, tg, il, tl), the sizes (n, t, c, smax), the workspace
    (``workspace_bytes(n, t, smax)`` bytes, 4 at the least) and the nll [N], loss [1] and grad [N, T, C] buffers.
    ``name`` is the module's, for the message."""
    # log_probs arrives as [T, N, C] (the reference passes out.transpose(0,1)); kernels are batch-major
    _lib.require_device(log_probs)
    lp = log_probs.detach().transpose(0, 1)
    if not lp.is_contiguous() or lp.dtype != torch.float32:
        lp = lp.contiguous().float()
    n, t, c = lp.shape
    dev = lp.device
    if targets.dim() != 2:
        raise NotImplementedError(f'{name}: targets must be 2-D [N, S_max] (padded), as the collator produces')
    tg = targets.to(device=dev, dtype=torch.int32).contiguous()
    il = torch.as_tensor(input_lengths).to(device=dev, dtype=torch.int32).contiguous()
    tl = torch.as_tensor(target_lengths).to(device=dev, dtype=torch.int32).contiguous()
    smax = tg.shape[1]
    ws = torch.empty(max(int(workspace_bytes(n, t, smax)), 4), dtype=torch.uint8, device=dev)
    nll = torch.empty(n, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.empty(n, t, c, dtype=torch.float32, device=dev)
    return (lp, tg, il, tl), (n, t, c, smax), ws, nll, loss, grad


class _CTCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, blank, zero_infinity):
        (lp, tg, il, tl), (n, t, c, smax), ws, nll, loss, grad = _operands(
            'CTCLoss', lib.w2l_ctc_workspace_bytes, log_probs, targets, input_lengths, target_lengths)
        check(lib.w2l_ctc_loss(ptr(lp), ptr(tg), ptr(il), ptr(tl), n, t, c, smax, int(blank), int(zero_infinity),
                               ptr(nll), ptr(loss), ptr(grad), ptr(ws), stream_ptr()), 'w2l_ctc_loss')
        ctx.grad = grad
        ctx.nll = nll
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad * g
        return grad.transpose(0, 1), None, None, None, None, None


class CTCLoss(nn.Module):
    """CTCLoss(blank=0, reduction='mean', zero_infinity=True) -- the only configuration the
    reference instantiates.  Input layout and semantics follow torch.nn.CTCLoss:
    log_probs [T, N, C], targets [N, S_max] padded, lengths [N]."""

    def __init__(self, blank=0, reduction='mean', zero_infinity=False):
        super().__init__()
        if reduction != 'mean':
            raise NotImplementedError("only reduction='mean' is implemented (base_asr_models.py:23)")
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = zero_infinity

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return _CTCFn.apply(log_probs, targets, input_lengths, target_lengths, self.blank, self.zero_infinity)


class _WildcardCTCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, blank, zero_infinity, penalty, owner):
        (lp, tg, il, tl), (n, t, c, smax), ws, nll, loss, grad = _operands(
            'WildcardCTCLoss', lib.w2l_wctc_workspace_bytes, log_probs, targets, input_lengths, target_lengths)
        status = torch.empty(n, dtype=torch.int32, device=lp.device)
        # the wildcard id is the first index past the model's classes: no output unit, no decoder ever sees it
        check(lib.w2l_wctc_loss(ptr(lp), ptr(tg), ptr(il), ptr(tl), n, t, c, smax, int(blank), int(zero_infinity), c,
                                float(penalty), ptr(nll), ptr(loss), ptr(grad), ptr(status), ptr(ws), stream_ptr()),
              'w2l_wctc_loss')
        ctx.grad = grad
        ctx.nll = nll
        owner._status = status
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad * g
        return grad.transpose(0, 1), None, None, None, None, None, None, None


class WildcardCTCLoss(nn.Module):
    """CTC whose targets may hold a wildcard: "here is speech the transcript has no text for" (the common core of W-CTC and of
    Star Temporal Classification; the definition is in include/w2l_hip.h at w2l_wctc_loss).  Layout as CTCLoss: log_probs
    [T, N, C], targets [N, S_max] padded (host or device), lengths [N]; a target entry equal to C, the number of classes, is the
    wildcard.  Consecutive wildcards are one; a wildcard gap may take any number of frames, zero included between different
    labels, and each of its frames costs ``penalty`` (log domain, <= 0) in place of a blank's log-probability.  Target
    lengths count the raw entries, wildcards included; the mean divides each utterance's loss by its number of labels.

    The score is NOT a normalised probability: with a wildcard one frame labelling is reached through more than one state
    path, so the loss of an utterance may be negative (W-CTC and STC have the same property).  Without a wildcard in a row the
    value and the gradient are CTCLoss's.

    last_status() is the int32 [N] device tensor of the latest call: 0 ok, 1 no finite path, 2 an entry that is neither a
    label nor the wildcard (that utterance contributes loss and gradient 0).  Nothing reads it during a step."""

    def __init__(self, blank=0, reduction='mean', zero_infinity=False, penalty=0.0):
        super().__init__()
        if reduction != 'mean':
            raise NotImplementedError("only reduction='mean' is implemented (base_asr_models.py:23)")
        if not float(penalty) <= 0.0:
            raise ValueError(f'WildcardCTCLoss: penalty is a log-domain cost per frame and must be <= 0, got {penalty}')
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = zero_infinity
        self.penalty = float(penalty)
        self._status = None

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return _WildcardCTCFn.apply(log_probs, targets, input_lengths, target_lengths, self.blank, self.zero_infinity,
                                    self.penalty, self)

    def last_status(self):
        """status [N] (int32, on the device) of the latest forward, or None before the first"""
        return self._status

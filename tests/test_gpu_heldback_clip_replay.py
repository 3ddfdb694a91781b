"""Replayed steps with held-back weight gradients AND gradient clipping: the clip call computes the held-back gradients into
``p.grad`` (they belong in the norm), and the recorded optimizer phase names their addresses.  Those addresses must not depend on
which block the caching allocator hands out: here another tensor takes every block that ``zero_grad`` frees, the worst the
allocator can do, and the optimizer phase must still be replayed and every address it names must stay allocated."""
import numpy as np
import pytest
import torch

from gpu_helpers import build_w2l

pytestmark = pytest.mark.gpu

LAYERS = [(128, 11, 2, 1, 0.0), (192, 13, 1, 1, 0.0), (128, 29, 1, 2, 0.0)]


def _run(replay_on, steps, batches, sd):
    from wav2letter_pytorch_amd import _lib, replay
    from wav2letter_pytorch_amd.optim import FusedAdamW
    replay.ENABLED = replay_on
    _lib.AUDIT = replay_on
    for k in ('recorded', 'recorded_O', 'replayed_F', 'replayed_B', 'replayed_O', 'replayed_X'):
        replay.STATS[k] = 0
    replay.STATS['poisoned'] = []
    try:
        torch.manual_seed(11)
        model = build_w2l(LAYERS, sd, 'bf16').cuda().train()
        model.check_nan = False
        opt = FusedAdamW.from_adam(torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-2))
        opt.overlap = True
        opt.defer_wgrad(model, 2)
        losses, hogs = [], []
        for i in range(steps):
            x, il, tg, tl = batches[i % len(batches)]
            shapes = [tuple(p.grad.shape) for p in model.parameters() if p.grad is not None and p.dim() == 3]
            opt.zero_grad(set_to_none=True)
            # whatever zero_grad freed is taken at once: a gradient allocated in this step cannot land where the last one was
            hogs = [torch.empty(s, dtype=torch.float32, device='cuda') for s in shapes for _ in range(2)]
            out, ol = model(x, il)
            loss = model.criterion(out.transpose(0, 1), tg, ol, tl)
            loss.backward()
            opt.clip_grad_norm_(0.5)
            opt.step()
            losses.append(float(loss.detach()))
        opt.join()
        torch.cuda.synchronize()
        del hogs
        params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        bad = replay.audit(model.engine()) if replay_on else []
        return losses, params, dict(replay.STATS), bad
    finally:
        replay.ENABLED = True
        _lib.AUDIT = False


def test_clipped_held_back_gradients_keep_their_address(monkeypatch):
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd import engine as E
    monkeypatch.setattr(E, 'FOLD_BN_FWD', '0')
    monkeypatch.setattr(E, 'FAST_BN_BWD', False)
    monkeypatch.setattr(E, 'DETERMINISTIC_WGRAD', True)
    sd = O.init_wav2letter_state(LAYERS, seed=41)
    batches = []
    for b in range(3):
        x, il, tg, tl = O.synthetic_batch(4, 300, seed=50 + b, s_lo=8, s_hi=30)
        batches.append((x.cuda(), il, tg.cuda(), tl.cuda()))
    steps = 10
    le, pe, _, _ = _run(False, steps, batches, sd)
    lr_, pr, st, bad = _run(True, steps, batches, sd)
    print('replay statistics:', st)
    assert bad == [], bad[:8]
    assert st['poisoned'] == [] and st['recorded_O'] <= 2, st
    assert st['replayed_O'] >= 3, st                       # the recorded optimizer phase was found valid and replayed
    assert le == lr_, (le, lr_)
    for k in pe:
        assert np.array_equal(pe[k], pr[k]), k

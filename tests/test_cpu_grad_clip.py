"""Gradient clipping without a GPU: trainer.Trainer stores and validates gradient_clip_val / gradient_clip_algorithm
(Lightning's keys, reachable as trainer.* overrides of train.py), the model hook parses both Lightning signatures, and the new
entry points are declared in include/w2l_hip.h, bound in _lib and replayable, with the ABI version unchanged."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('w2l_grad_sqnorm_multi', 'w2l_grad_clip_value', 'w2l_sgd_pack_clip', 'w2l_sgd_small_multi_clip')


def test_trainer_stores_and_validates_clip_keys():
    from wav2letter_pytorch_amd.trainer import Trainer
    t = Trainer()
    assert t.gradient_clip_val is None and t.gradient_clip_algorithm == 'norm'
    t = Trainer(gradient_clip_val=400, gradient_clip_algorithm='value')
    assert t.gradient_clip_val == 400.0 and t.gradient_clip_algorithm == 'value'
    assert Trainer(gradient_clip_val=0).gradient_clip_val is None              # 0 = off, as in Lightning
    with pytest.raises(ValueError):
        Trainer(gradient_clip_val=-1.0)
    with pytest.raises(ValueError):
        Trainer(gradient_clip_val=1.0, gradient_clip_algorithm='l1')


def test_clip_gradients_rejects_unknown_algorithm():
    import torch
    from wav2letter_pytorch_amd.optim import clip_gradients
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.full((3,), 4.0)
    opt = torch.optim.SGD([p], lr=0.1)
    with pytest.raises(ValueError):
        clip_gradients(opt, 1.0, 'l1')
    n = clip_gradients(opt, 1.0, 'norm')                 # a CPU optimizer takes torch's own function
    assert abs(float(n) - 48 ** 0.5) < 1e-5 and abs(float(p.grad.norm()) - 1.0) < 1e-5
    clip_gradients(opt, 0.1, 'value')
    assert torch.equal(p.grad, torch.full((3,), 0.1))


def test_new_entry_points_declared_bound_and_replayable():
    from wav2letter_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'w2l_hip.h')).read()
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib.lib.w2l_replay_op(name.encode()) >= 0, name
    ops = _lib._replay_ops()
    assert all(name in ops for name in NEW)
    assert _lib.lib.w2l_abi_version() == 2
    assert '#define W2L_GNORM_CHUNK %d' % _lib.GNORM_CHUNK in hdr and '#define W2L_GNORM_BLOCKS %d' % _lib.GNORM_BLOCKS in hdr

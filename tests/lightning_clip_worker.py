"""Worker of test_gpu_grad_clip.py::test_lightning_hook_both_signatures: a MINIMAL stand-in for pytorch_lightning is put into
sys.modules BEFORE this package is imported (as in lightning_shim_worker.py), and its Trainer runs automatic optimisation with
gradient clipping in Lightning's closure order: zero_grad, training_step, backward, configure_gradient_clipping, step.  argv[1]
picks the hook signature the Trainer uses: '1' = Lightning 1.x (optimizer, optimizer_idx, gradient_clip_val,
gradient_clip_algorithm), '2' = Lightning 2.x (optimizer, gradient_clip_val=, gradient_clip_algorithm=).  Nothing here is
Lightning's code; the image has no Lightning to test against."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


class LightningModule(nn.Module):
    def __init__(self):
        super().__init__()
        self.trainer = None

    def log_dict(self, d, *args, **kwargs):
        pass

    def optimizers(self):
        return self.trainer.optimizers[0]

    def on_train_batch_end(self, outputs, batch, batch_idx):
        pass

    def on_train_epoch_end(self):
        pass


class Trainer:
    def __init__(self, max_steps=4, gradient_clip_val=None, gradient_clip_algorithm='norm', signature='2', **unused):
        self.max_steps = max_steps
        self.gradient_clip_val, self.gradient_clip_algorithm = gradient_clip_val, gradient_clip_algorithm
        self.signature = signature
        self.optimizers, self.schedulers = [], []
        self.hook_calls = 0

    def clip(self, model, opt, val, algorithm):
        self.hook_calls += 1
        if self.signature == '1':
            return model.configure_gradient_clipping(opt, 0, val, algorithm)
        return model.configure_gradient_clipping(opt, gradient_clip_val=val, gradient_clip_algorithm=algorithm)

    def fit(self, model, train_dataloader):
        model.trainer = self
        model = model.cuda()
        self.optimizers, self.schedulers = model.configure_optimizers()
        opt = self.optimizers[0]
        opt.overlap = True
        model.train()
        for i, batch in enumerate(train_dataloader):
            if i >= self.max_steps:
                break

            def closure():
                opt.zero_grad()
                loss = model.training_step(batch, i)
                loss.backward()
                if self.gradient_clip_val:
                    self.clip(model, opt, self.gradient_clip_val, self.gradient_clip_algorithm)
                return loss
            opt.step(closure)
            model.on_train_batch_end(None, batch, i)
        opt.join()
        return model


def main():
    sig = sys.argv[1]
    ptl = types.ModuleType('pytorch_lightning')
    ptl.LightningModule, ptl.Trainer = LightningModule, Trainer
    sys.modules['pytorch_lightning'] = ptl
    from gpu_helpers import build_w2l
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd import base_asr_models as B
    assert B._Base is LightningModule
    layers = [(128, 11, 2, 1, 0.0), (128, 11, 1, 1, 0.0), (128, 11, 1, 1, 0.0), (128, 11, 1, 1, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=21)
    x, il, tg, tl = O.synthetic_batch(4, 200, seed=22, s_lo=5, s_hi=12)
    texts = tuple(''.join(O.ENGLISH_LOWERCASE[int(i)] for i in tg[n, :int(tl[n])]) for n in range(4))
    batch = (x, il, tg, tl, ('a', 'b', 'c', 'd'), texts)
    model = build_w2l(layers, sd, 'bf16')
    model._cfg.optimizer.lr = 0.05
    import pytorch_lightning
    tr = pytorch_lightning.Trainer(max_steps=4, gradient_clip_val=1e-2, signature=sig)
    tr.fit(model, [batch] * 4)
    torch.cuda.synchronize()
    opt = tr.optimizers[0]
    bad = False
    try:
        tr.clip(model, opt, 1.0, 'l1')
    except ValueError:
        bad = True
    noop = tr.clip(model, opt, 0, 'l1') is None and '_w2l_clip_arm' not in opt.__dict__
    path = os.path.join(tempfile.mkdtemp(), 'params.npz')
    np.savez(path, **{k: v.detach().cpu().numpy() for k, v in model.named_parameters()})
    print(json.dumps({'bad_algorithm_raises': bad, 'hook_calls': tr.hook_calls - 2, 'zero_clip_noop': noop, 'params': path}))


if __name__ == '__main__':
    main()

"""Child process of tests/test_gpu_asg.py: a short training run of a small Wav2Letter with ``model.criterion=asg`` on one
repeated synthetic batch, bit-reproducible kernels selected; writes the final parameters (``criterion.transitions`` included)
to an .npz and prints the replay statistics.  ``W2L_REPLAY=0`` in the environment gives the eager run.

    python tests/asg_replay_worker.py OUT.npz STEPS
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAYERS = [(128, 11, 2, 1, 0.0), (128, 13, 1, 2, 0.0)]        # the smallest stack the smoke test drives


def build_model(criterion='asg', lr=0.01, seed=5):
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    cfg = wav2letter_model(mid_layers=len(LAYERS), dropout=False)
    cfg['layers'] = type(cfg['layers'])(type(cfg['layers'][0])(output_size=c, kernel_size=k, stride=s, dilation=d, dropout=p)
                                        for c, k, s, d, p in LAYERS)
    cfg['criterion'] = criterion
    cfg['optimizer']['lr'] = lr
    torch.manual_seed(seed)
    return Wav2Letter(cfg)


def synthetic_batch(labels, n=4, frames=120, seed=9):
    """_collator's 6-tuple: spectrograms [n, 64, frames], lengths, padded int32 targets, target lengths, paths, texts; the
    transcripts are two words of letters with one doubled letter each"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 64, frames, generator=g)
    lens = torch.full((n,), frames, dtype=torch.int32)
    index = {c: i for i, c in enumerate(labels)}
    texts = []
    for _ in range(n):
        ids = torch.randint(2, 28, (int(torch.randint(5, 12, (1,), generator=g)),), generator=g).tolist()
        word = ''.join(labels[i] for i in ids)
        texts.append(word[:3] + word[2] + ' ' + word[3:])          # a doubled letter, then a space
    tl = torch.tensor([len(t) for t in texts], dtype=torch.int32)
    tg = torch.zeros(n, int(tl.max()), dtype=torch.int32)
    for i, t in enumerate(texts):
        tg[i, :len(t)] = torch.tensor([index[c] for c in t], dtype=torch.int32)
    return x, lens, tg, tl, tuple(f'synthetic_{i}.wav' for i in range(n)), tuple(texts)


def main():
    out_path, steps = sys.argv[1], int(sys.argv[2])
    from wav2letter_pytorch_amd import engine as E, replay
    from wav2letter_pytorch_amd.optim import FusedSGD
    E.FOLD_BN_FWD = '0'
    E.FAST_BN_BWD = False
    E.DETERMINISTIC_WGRAD = True
    torch.cuda.set_device(0)
    model = build_model().cuda().train()
    x, il, tg, tl, _, _ = synthetic_batch(model.labels)
    x, tg, tl = x.cuda(), tg.cuda(), tl.cuda()
    opt = FusedSGD.from_sgd(torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4))
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        out, ol = model(x, il)
        loss = model.criterion(out.transpose(0, 1), tg, ol, tl)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    opt.join()
    torch.cuda.synchronize()
    np.savez(out_path, **{k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
    stats = {k: (v if k != 'poisoned' else list(v)) for k, v in replay.STATS.items()}
    print('ASG_WORKER ' + json.dumps({'losses': losses, 'stats': stats, 'replay': replay.ENABLED}), flush=True)


if __name__ == '__main__':
    main()

"""Worker of test_gpu_grad_clip.py::test_data_parallel_one_rank_clipped_steps_match_single_process: three clipped training
steps through the data-parallel path (a one-rank process group, the step engine handing every gradient to
distributed.GradReducer, forced active), then the same three steps in a plain single-process run; both final parameter sets
and last norms are written for the test to compare.  The norm is launched after the reducer's collectives (the averaged
gradient, as Lightning's DDP clips it)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(reducer):
    from gpu_helpers import build_w2l
    from oracle import w2l_oracle as O
    layers = [(128, 11, 2, 1, 0.0), (256, 13, 1, 1, 0.0), (128, 29, 1, 2, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=60)
    model = build_w2l(layers, sd, 'bf16').train()
    if reducer is not None:
        model.grad_reducer = reducer
    model._cfg.optimizer.lr = 0.05
    opt = model.configure_optimizers()[0][0]
    opt.overlap = True
    x, il, tg, tl = O.synthetic_batch(4, 240, seed=70, s_lo=5, s_hi=20)
    norm = None
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        out, ol = model(x.cuda(), il)
        model.criterion(out.transpose(0, 1), tg, ol, tl).backward()
        norm = opt.clip_grad_norm_(1e-3)
        opt.step()
    opt.join()
    torch.cuda.synchronize()
    return dict(norm=float(norm), **{'p/' + k: v.detach().cpu().numpy() for k, v in model.named_parameters()})


def main():
    import torch.distributed as dist
    from wav2letter_pytorch_amd import engine as E
    from wav2letter_pytorch_amd.distributed import GradReducer, init_process_group_from_env
    E.FOLD_BN_FWD, E.FAST_BN_BWD, E.DETERMINISTIC_WGRAD = '0', False, True
    torch.cuda.set_device(0)
    init_process_group_from_env(backend='gloo', force=True)
    red = GradReducer(force=True)
    assert red.active
    np.savez(sys.argv[1] + '.dp.npz', **run(red))
    dist.destroy_process_group()
    np.savez(sys.argv[1] + '.single.npz', **run(None))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""ASG kernel timing at the headline shape (N=32, T'=500, A=29, transcripts of 80..120 labels): w2l_asg_loss (loss + both
gradients), w2l_asg_viterbi, and w2l_ctc_loss at the same shape in the same process.  The three are timed in interleaved
rounds (device events around REPS back-to-back calls each), median and minimum over the rounds, plus the accuracy of the ASG
loss and gradients against a float64 reference of the same recursions (torch on the CPU, batched over the utterances).

    python tools/bench_asg.py [--rounds 15] [--reps 20] > profiles/asg_bench.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.asg import encode_repeats  # noqa: E402

N, T, A, S_LO, S_HI = 32, 500, 29, 80, 120
NEG = -1e30


def reference(x, g, targets, lens):
    """float64 loss ('mean') and gradients, the recursions batched over the utterances (all of full length T)"""
    x = x.double().requires_grad_(True)
    g = g.double().requires_grad_(True)
    smax = targets.shape[1]
    y = torch.zeros(N, smax, dtype=torch.long)
    for n in range(N):
        y[n, :int(lens[n])] = torch.tensor(encode_repeats(targets[n, :int(lens[n])].tolist()))
    valid = torch.arange(smax)[None, :] < lens[:, None].long()
    fa = x[:, 0]
    ta = torch.full((N, smax), NEG, dtype=torch.float64)
    ta = torch.cat([x[:, 0].gather(1, y[:, :1]), ta[:, 1:]], dim=1)
    stay = g[y, y]
    adv = g[y[:, :-1], y[:, 1:]]
    for t in range(1, T):
        fa = x[:, t] + torch.logsumexp(fa[:, :, None] + g[None], dim=1)
        moved = torch.cat([torch.full((N, 1), NEG, dtype=torch.float64), ta[:, :-1] + adv], dim=1)
        ta = x[:, t].gather(1, y) + torch.logsumexp(torch.stack([ta + stay, moved]), dim=0)
        ta = torch.where(valid, ta, torch.full_like(ta, NEG))
    zf = torch.logsumexp(fa, dim=1)
    zt = ta.gather(1, (lens.long() - 1)[:, None])[:, 0]
    loss = ((zf - zt) / lens.double()).mean()
    loss.backward()
    return float(loss.detach()), x.grad, g.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_asg.py measures on the GPU: no device found')
    gen = torch.Generator().manual_seed(0)
    x = torch.log_softmax(torch.randn(N, T, A, generator=gen) * 2, -1)
    g = torch.randn(A, A, generator=gen) * 0.5
    tl = torch.randint(S_LO, S_HI + 1, (N,), generator=gen, dtype=torch.int32)
    tg = torch.randint(1, A, (N, S_HI), generator=gen, dtype=torch.int32)
    il = torch.full((N,), T, dtype=torch.int32)
    xd, gd, tgd, tld, ild = x.cuda(), g.cuda(), tg.cuda(), tl.cuda(), il.cuda()

    ws_asg = torch.empty(int(lib.w2l_asg_workspace_bytes(N, T, A, S_HI)), dtype=torch.uint8, device='cuda')
    ws_vit = torch.empty(int(lib.w2l_asg_viterbi_workspace_bytes(N, T, A)), dtype=torch.uint8, device='cuda')
    ws_ctc = torch.empty(int(lib.w2l_ctc_workspace_bytes(N, T, S_HI)), dtype=torch.uint8, device='cuda')
    nll = torch.empty(N, device='cuda')
    loss = torch.empty(1, device='cuda')
    status = torch.empty(N, dtype=torch.int32, device='cuda')
    gx = torch.empty(N, T, A, device='cuda')
    gg = torch.empty(A, A, device='cuda')
    path = torch.empty(N, T, dtype=torch.int32, device='cuda')
    score = torch.empty(N, device='cuda')

    def asg():
        check(lib.w2l_asg_loss(ptr(xd), ptr(gd), ptr(tgd), ptr(ild), ptr(tld), N, T, A, S_HI, 0, 0, ptr(nll), ptr(loss), ptr(gx),
                               ptr(gg), ptr(status), ptr(ws_asg), ws_asg.numel(), stream_ptr()), 'w2l_asg_loss')

    def viterbi():
        check(lib.w2l_asg_viterbi(ptr(xd), ptr(gd), ptr(ild), N, T, A, ptr(ws_vit), ws_vit.numel(), ptr(path), ptr(score),
                                  stream_ptr()), 'w2l_asg_viterbi')

    def ctc():
        check(lib.w2l_ctc_loss(ptr(xd), ptr(tgd), ptr(ild), ptr(tld), N, T, A, S_HI, 0, 1, ptr(nll), ptr(loss), ptr(gx),
                               ptr(ws_ctc), stream_ptr()), 'w2l_ctc_loss')

    asg()
    torch.cuda.synchronize()
    ref_loss, ref_gx, ref_gg = reference(x, g, tg, tl)
    print(f'shape: N={N} T={T} A={A} transcripts {S_LO}..{S_HI} labels, reduction mean')
    print(f'asg loss {float(loss[0]):.6f} reference {ref_loss:.6f} rel err {abs(float(loss[0]) - ref_loss) / abs(ref_loss):.2e}')
    print(f'asg grad_x max abs err {float((gx.cpu().double() - ref_gx).abs().max()):.2e} (scale {float(ref_gx.abs().max()):.2e})')
    print(f'asg grad_trans max abs err {float((gg.cpu().double() - ref_gg).abs().max()):.2e} (scale {float(ref_gg.abs().max()):.2e})')

    runs = {'w2l_asg_loss': asg, 'w2l_asg_viterbi': viterbi, 'w2l_ctc_loss': ctc}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / args.reps * 1e3)
    for name, v in times.items():
        print(f'{name}: median {statistics.median(v):.1f} us, min {min(v):.1f} us per call ({args.rounds} interleaved rounds x '
              f'{args.reps} calls)')
    # what ASGLoss adds on the host: each call reads the status vector back (one synchronisation), CTCLoss's does not
    import time
    from wav2letter_pytorch_amd.asg import ASGLoss
    crit = ASGLoss(A).cuda()
    with torch.no_grad():
        crit.transitions.copy_(gd)
    lp = xd.transpose(0, 1).requires_grad_(True)
    wall = []
    for i in range(args.reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        crit(lp, tgd, ild, tld)
        if i >= 3:
            wall.append((time.perf_counter() - t0) * 1e6)
    print(f'ASGLoss.forward on an idle device, host wall time with its status read-back: median {statistics.median(wall):.1f} us '
          f'(the kernels above plus the launch, allocation and one device-to-host copy of {N} int32)')
    ratio = statistics.median(times['w2l_asg_loss']) / statistics.median(times['w2l_ctc_loss'])
    print(f'asg_loss / ctc_loss (median): {ratio:.2f}x')


if __name__ == '__main__':
    main()

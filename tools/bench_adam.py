#!/usr/bin/env python3
"""Fused Adam / AdamW, measured (profiles/adam_ab.txt is this tool's output):

  (a) w2l_adam_pack against w2l_sgd_pack per conv-weight shape of the Wav2Letter table, same process, interleaved rounds.
      Every launch takes the next of several buffer sets that together exceed the last-level cache several times over: the
      cold-operand rate a training step sees.  Both are HBM-bound passes; the byte model says 32 B against 24 B per
      parameter (34 / 26 with the e4m3 operands): a ratio of 1.33 (1.31).
  (b) the headline training step with optim.FusedAdamW (replay on, a warm-up schedule stepped per batch) against
      torch.optim.AdamW used as it was before FusedAdamW existed (torch foreach ops, the engine repacking every weight, an
      optimizer phase that cannot be recorded), two models in ONE process taking turns in blocks of steps (the
      tools/step_ab.py scheme): ms/step, host ms/step (the time the Python loop needs to enqueue a step), and how often the
      optimizer phase was recorded / replayed.

  python tools/bench_adam.py [--batch 32 --frames 1000 --block 10 --rounds 5] [--out profiles/adam_ab.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402


def table_shapes():
    cfg = B.w2l_cfg(20)
    cin, shapes = int(cfg.input_size), []
    for layer in cfg.layers:
        s = (int(layer['output_size']), cin, int(layer['kernel_size']))
        if s[0] % 64 == 0 and s[1] % 64 == 0 and s not in shapes:
            shapes.append(s)
        cin = s[0]
    return shapes


COLD_BYTES = 1 << 30


def kernel_ab(say, q, reps0=20, rounds=5):
    from wav2letter_pytorch_amd import _lib as L
    lib, ptr = L.lib, L.ptr
    state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device='cuda')
    state.view(torch.int64)[0] = 0
    dyn = torch.zeros(4, device='cuda')
    L.check(lib.w2l_adam_tick(ptr(state), ptr(dyn), 1e-3, 0.9, 0.999, L.stream_ptr()))
    say(f'(a) kernel time, e4m3 operands {"on" if q else "off"}: {rounds} interleaved rounds x >= {reps0} launches rotating among >= 1 GiB of buffer sets (cold operands), median us per launch')
    say(f'    {"Cout x Cin x Kw":>18s} {"sgd_pack":>10s} {"sgd spread":>11s} {"adam_pack":>10s} {"ratio":>6s} {"model":>6s} {"adam GB/s":>10s}')
    tot = [0.0, 0.0]
    for cout, cin, kw in table_shapes():
        # cold operands, as a training step finds them: the launches rotate among buffer sets that together exceed the 256 MB
        # last-level cache several times over, so no launch finds what an earlier one left there
        n = cout * cin * kw
        nsets = max(3, min(256, -(-COLD_BYTES // (n * (34 if q else 32)))))
        sets = []
        for _ in range(nsets):
            p, g, m, v = (torch.randn(kw, cout, cin, device='cuda') for _ in range(4))
            v.abs_()
            fh, dh = (torch.empty(kw, a, b, dtype=torch.bfloat16, device='cuda') for a, b in ((cout, cin), (cin, cout)))
            fq, dq = ((torch.empty(kw, a, b, dtype=torch.uint8, device='cuda') for a, b in ((cout, cin), (cin, cout))) if q else (None, None))
            sets.append((p, g, m, v, (ptr(fh), None, ptr(dh), None, ptr(fq), ptr(dq), 64.0 if q else 1.0), (fh, dh, fq, dq)))
        turn = [0]

        def sgd():
            p, g, m, v, ops, _ = sets[turn[0] % nsets]
            turn[0] += 1
            L.check(lib.w2l_sgd_pack(ptr(p), ptr(g), ptr(m), 0, 0.0, 0.9, 1e-4, 1, 0, cout, cin, kw, *ops, L.stream_ptr()))

        def adam():
            p, g, m, v, ops, _ = sets[turn[0] % nsets]
            turn[0] += 1
            L.check(lib.w2l_adam_pack(ptr(p), ptr(g), ptr(m), ptr(v), ptr(dyn), 0.9, 0.999, 1e-8, 1e-2, 1, 0, cout, cin, kw, *ops, None,
                                      L.stream_ptr()))

        reps = max(reps0, nsets)
        times = {sgd: [], adam: []}
        for fn in (sgd, adam):
            fn()
        del p, g, m, v
        for _ in range(rounds):
            for fn in (sgd, adam):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                b.synchronize()
                times[fn].append(a.elapsed_time(b) / reps * 1e3)
        ts, ta = statistics.median(times[sgd]), statistics.median(times[adam])
        spread = (max(times[sgd]) - min(times[sgd])) / ts
        tot[0] += ts
        tot[1] += ta
        say(f'    {cout:>6d} x {cin:>4d} x {kw:>2d} {ts:10.1f} {spread:10.1%} {ta:10.1f} {ta / ts:6.2f} {(34 / 26) if q else (32 / 24):6.2f} '
            f'{n * (34 if q else 32) / ta / 1e3:10.0f}')
    say(f'    {"sum over the shapes":>18s} {tot[0]:10.1f} {"":>11s} {tot[1]:10.1f} {tot[1] / tot[0]:6.2f}')


def warmup(s):
    return min(1.0, (s + 1) / 500.0)


def step_ab(say, args):
    from wav2letter_pytorch_amd import Wav2Letter, replay
    from wav2letter_pytorch_amd.defaults import synthetic_batch
    from wav2letter_pytorch_amd.optim import FusedAdamW
    dev = torch.device('cuda', 0)
    x, il, tg, tl = synthetic_batch(args.batch, args.frames, seed=1234)
    x, tg_d, tl_d = x.to(dev), tg.to(dev), tl.to(dev)
    runs = {}
    for name in ('fused', 'torch'):
        torch.manual_seed(0)
        model = Wav2Letter(B.w2l_cfg(20, precision='bf16')).to(dev).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
        if name == 'fused':
            opt = FusedAdamW.from_adam(opt)
            opt.overlap = True
            if args.defer:
                opt.defer_wgrad(model, args.defer)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, warmup)
        runs[name] = (model, opt, sch, model.compute_output_lengths(il).to(dev))

    def step(name):
        model, opt, sch, ol = runs[name]
        opt.zero_grad(set_to_none=True)
        out, _ = model(x, None)
        model.criterion(out.transpose(0, 1), tg_d, ol, tl_d).backward()
        opt.step()
        sch.step()

    def fence(name):
        getattr(runs[name][1], 'join', lambda: None)()
        torch.cuda.synchronize()

    for name in runs:
        for _ in range(8):
            step(name)
        fence(name)
    wall, host = {n: [] for n in runs}, {n: [] for n in runs}
    stats0 = dict(replay.STATS)
    for _ in range(args.rounds):
        for name in runs:
            for _ in range(3):
                step(name)
            fence(name)
            t0 = time.perf_counter()
            for _ in range(args.block):
                step(name)
            t1 = time.perf_counter()
            fence(name)
            wall[name].append((time.perf_counter() - t0) / args.block * 1e3)
            host[name].append((t1 - t0) / args.block * 1e3)
    say(f'(b) Wav2Letter (20 units) N={args.batch} T={args.frames} bf16, AdamW lr 1e-3 wd 1e-2, LambdaLR warm-up stepped every batch, '
        f'{args.rounds} rounds x {args.block} steps per variant, interleaved')
    say(f'    fused = optim.FusedAdamW (replay on, defer_wgrad {args.defer}); torch = torch.optim.AdamW as configure_optimizers used it before')
    for name in runs:
        w, h = wall[name], host[name]
        say(f'    {name:6s} {statistics.mean(w):8.3f} ms/step (min {min(w):.3f} max {max(w):.3f})   host {statistics.mean(h):7.3f} ms/step '
            f'(min {min(h):.3f} max {max(h):.3f})')
    say(f'    fused / torch = {statistics.mean(wall["fused"]) / statistics.mean(wall["torch"]):.3f} (ms/step), '
        f'{statistics.mean(host["fused"]) / statistics.mean(host["torch"]):.3f} (host)')
    say('    optimizer phases during the timed part (both variants share the counters; torch.optim.AdamW never reaches them): '
        + ', '.join(f'{k} +{replay.STATS[k] - stats0[k]}' for k in ('recorded_O', 'replayed_O', 'replayed_X', 'replayed_F')))
    say(f'    recordings dropped: {replay.STATS["poisoned"][-4:]}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--defer', type=int, default=0)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/bench_adam.py on {torch.cuda.get_device_name(0)}')
    kernel_ab(say, q=False)
    kernel_ab(say, q=True)
    if not args.skip_step:
        step_ab(say, args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""A/B of the inference forward: ``model.infer`` (one fused launch per convolution) against the evaluation-mode forward under
``no_grad`` (three launches per unit), same process, alternating legs, device events around at least a second of work per leg
after warming (and tuning) both.  Reports ms per forward, frames / s, library launches per forward, peak allocated memory of
each leg and the spread of the repeated legs.

    python tools/bench_infer.py [--legs 5] [--seconds 1.0] [--out profiles/infer_ab.txt]

``--precision fp8``: the two legs are the fused fp8 ``infer`` and the fp8 evaluation-mode forward of one ``precision='fp8'``
model, and a third leg is the bf16 ``infer`` of the same network."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from wav2letter_pytorch_amd import Jasper, Wav2Letter, _lib, defaults  # noqa: E402


def count_launches(fn):
    """library entry points that enqueue kernels, called by one run of fn"""
    names = list(_lib.TRACE_NAMES)
    saved = {n: getattr(_lib.lib, n) for n in names if hasattr(_lib.lib, n)}
    counts = {}

    def wrap(n, f):
        def inner(*a):
            counts[n] = counts.get(n, 0) + 1
            return f(*a)
        return inner
    for n, f in saved.items():
        setattr(_lib.lib, n, wrap(n, f))
    try:
        fn()
    finally:
        for n, f in saved.items():
            setattr(_lib.lib, n, f)
    return sum(counts.values()), counts


def leg(fn, seconds):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps, torch.cuda.max_memory_allocated() / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--out', default=None)
    ap.add_argument('--precision', choices=('bf16', 'fp8'), default='bf16')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    fp8 = args.precision == 'fp8'
    lines = [f'# tools/bench_infer.py --legs {args.legs} --seconds {args.seconds}' + (' --precision fp8' if fp8 else '') +
             ': infer (fused) vs eval() forward under no_grad, '
             f'{args.precision}' + (' (third leg: bf16 infer of the same network)' if fp8 else '') +
             f', alternating legs in one process; {torch.cuda.get_device_name(0)} '
             f'({getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")})']
    def build(which, precision):
        cfg = (defaults.wav2letter_model(mid_layers=20, dropout=False, precision=precision) if which == 'w2l'
               else defaults.jasper10x5_model(precision=precision))
        return (Wav2Letter if which == 'w2l' else Jasper)(cfg)
    shapes = [('wav2letter mid_layers=20', 'w2l', 32, 1000), ('jasper 10x5', 'jasper', 16, 1000)]
    for name, which, n, t in shapes:
        model = build(which, args.precision).cuda().eval()
        ref = None
        if fp8:                                          # the same network (same weights) with bf16 operands
            ref = build(which, 'bf16')
            ref.load_state_dict(model.state_dict())
            ref = ref.cuda().eval()
        x, il, _, _ = defaults.synthetic_batch(n, t)
        xd = x.cuda()
        frames = n * t // model.scaling_factor

        def fused():
            return model.infer(xd, il)

        def plain():
            with torch.no_grad():
                return model(xd, il)

        def bf16():
            return ref.infer(xd, il)
        fns = [('infer', fused), ('eval', plain)] + ([('bf16', bf16)] if fp8 else [])
        for _ in range(3):                           # warm all (the first call of each measures its block shapes)
            for _, fn in fns:
                fn()
        torch.cuda.synchronize()
        nl = {key: count_launches(fn)[0] for key, fn in fns}
        res = {key: [] for key, _ in fns}
        mem = {}
        for _ in range(args.legs):
            for key, fn in fns:
                ms, reps, peak = leg(fn, args.seconds)
                res[key].append(ms)
                mem[key] = peak
        lines.append(f'{name} N={n} T={t} ({frames} output frames per forward)')
        for key, _ in fns:
            v = sorted(res[key])
            med = v[len(v) // 2]
            lines.append(f'  {key:5s}: median {med:.3f} ms  min {v[0]:.3f}  max {v[-1]:.3f}  spread {(v[-1] - v[0]) / med * 100:.1f} %  '
                         f'{frames / med * 1e3:,.0f} frames/s  {nl[key]} launches/forward  peak {mem[key]:.0f} MiB  legs '
                         + ' '.join(f'{a:.3f}' for a in res[key]))
        mi, me = sorted(res['infer'])[len(res['infer']) // 2], sorted(res['eval'])[len(res['eval']) // 2]
        lines.append(f'  infer / eval = {mi / me:.3f} ({(1 - mi / me) * 100:+.1f} % time saved)')
        if fp8:
            mb = sorted(res['bf16'])[len(res['bf16']) // 2]
            lines.append(f'  fp8 infer / bf16 infer = {mi / mb:.3f}')
            lines.append(f'  fp8_saturated() after all legs: {model.engine().fp8_saturated()}')
        del model, ref
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

"""Measure the long-form path on the GPU (profiles/vad_bench.txt is this tool's output):

  power     w2l_vad_power on one hour of 16 kHz audio (230 MB), device events, warm, alternated in the same process with a
            device-to-device copy of the same buffer (which moves twice the bytes); GB/s of both against the 6.29 TB/s a
            float4 copy reaches on this chip;
  decide    w2l_vad_segments at F = 360 000 and F = 3 000 frames: one workgroup, a latency;
  e2e       a ten-minute synthetic recording through ConvCTCASR.transcribe_long against ConvCTCASR.transcribe of the same
            segments cut beforehand and passed in the same batches: the difference is what the segmentation costs, given
            with the spread of repeated runs.

    python tools/bench_vad.py [--reps 20] [--e2e-reps 5] [--batch-size 8] [--mid-layers 1]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_PEAK_TBS = 6.29


def recording(seconds, seed=0, rate=16000):
    """noise at -60 dBFS with bursts of louder noise of 1 to 12 s, separated by pauses of 0.4 to 2 s"""
    g = np.random.default_rng(seed)
    n = int(seconds * rate)
    x = (1e-3 * g.standard_normal(n)).astype(np.float32)
    t = 0.5
    while t < seconds - 1.0:
        d = float(g.uniform(1.0, 12.0))
        i, j = int(t * rate), min(n, int((t + d) * rate))
        x[i:j] += (0.3 * g.standard_normal(j - i)).astype(np.float32)
        t += d + float(g.uniform(0.4, 2.0))
    return x


def event_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def spread(ms):
    return f'median {statistics.median(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f} over {len(ms)} runs'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--e2e-reps', type=int, default=5)
    ap.add_argument('--batch-size', type=int, default=8)
    ap.add_argument('--mid-layers', type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_vad needs a GPU: a timing taken anywhere else says nothing')
    import ctypes as C
    from wav2letter_pytorch_amd._lib import lib, ptr, stream_ptr
    from wav2letter_pytorch_amd.segmentation import (VadConfig, batches_by_length, frame_power, segments_from_power, vad_params,
                                                     vad_segments)
    cfg = VadConfig()
    numbers = cfg.numbers(20.0)

    # ---- power pass, one hour
    hour = recording(600.0)
    x = torch.from_numpy(hour).cuda().repeat(6).view(1, -1).contiguous()
    n = x.shape[1]
    F = -(-n // cfg.hop)
    lens = torch.tensor([n], dtype=torch.int32).cuda()
    dst = torch.empty_like(x)
    for _ in range(3):                                   # warm both
        frame_power(x, lens, F, cfg.win, cfg.hop)
        dst.copy_(x)
    t_pow, t_copy = [], []
    for _ in range(args.reps):                           # alternated: both see the same machine
        t_pow += event_ms(lambda: frame_power(x, lens, F, cfg.win, cfg.hop), 1)
        t_copy += event_ms(lambda: dst.copy_(x), 1)
    gb = 4.0 * n / 1e9
    mp, mc = statistics.median(t_pow), statistics.median(t_copy)
    print(f'power pass, {n} samples ({gb * 1e3:.0f} MB read, {4 * F / 1e6:.1f} MB written), {F} frames: {spread(t_pow)}')
    print(f'  = {gb / mp * 1e3:.0f} GB/s read, {gb / mp / COPY_PEAK_TBS * 100:.0f} % of the {COPY_PEAK_TBS} TB/s a float4 copy reaches')
    print(f'device-to-device copy of the same buffer ({2 * gb * 1e3:.0f} MB moved): {spread(t_copy)}')
    print(f'  = {2 * gb / mc * 1e3:.0f} GB/s moved, {2 * gb / mc / COPY_PEAK_TBS * 100:.0f} % of {COPY_PEAK_TBS} TB/s;  power / copy = {mp / mc:.2f}')
    del dst

    # ---- decision pass: one workgroup
    power = frame_power(x, lens, F, cfg.win, cfg.hop)
    for frames in (F, 3000):
        pw = power[:, :frames].contiguous()
        nf = torch.tensor([frames], dtype=torch.int32).cuda()
        recs = segments_from_power(pw, nf, numbers, cap=4096)
        p = vad_params(numbers)
        ws_bytes = int(lib.w2l_vad_workspace_bytes(1, frames))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
        out = torch.empty(32 + 8 * 4096, dtype=torch.uint8, device='cuda')
        ms = event_ms(lambda: lib.w2l_vad_segments(ptr(pw), frames, ptr(nf), 1, C.byref(p), 4096, ptr(ws), ws_bytes, ptr(out), stream_ptr()),
                      args.reps)
        print(f'decision pass, F = {frames} ({recs[0]["count"]} segments): {spread(ms)}')
    del x, power

    # ---- end to end, ten minutes
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    from wav2letter_pytorch_amd.data.data_loader import SpectrogramExtractor
    SpectrogramExtractor.dithering = 0.0                 # (no random dither: the two paths must give the same text)
    torch.manual_seed(0)
    model = Wav2Letter(wav2letter_model(mid_layers=args.mid_layers, dropout=False)).cuda().eval()
    ten = recording(600.0, seed=1)
    segs = vad_segments([ten], cfg, 20.0)[0]
    lengths = (segs[:, 1] - segs[:, 0]).tolist()
    order = [i for b in batches_by_length(lengths, args.batch_size) for i in b]
    cut = [ten[int(segs[i, 0]): int(segs[i, 1])] for i in order]          # the same batches transcribe_long forms

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    long_fn = lambda: model.transcribe_long([ten], max_seconds=20.0, batch_size=args.batch_size)
    cut_fn = lambda: model.transcribe(cut, batch_size=args.batch_size)
    a, b = long_fn(), cut_fn()                           # warm: every batch shape is tuned once
    same = [s['text'] for s in sorted(a[0]['segments'], key=lambda s: s['start'])] == [b[order.index(i)] for i in range(len(order))]
    t_long, t_cut = [], []
    for _ in range(args.e2e_reps):
        t_long.append(wall(long_fn))
        t_cut.append(wall(cut_fn))
    print(f'end to end, 600 s recording, {len(segs)} segments (longest {max(lengths) / 16000:.1f} s), batch size {args.batch_size}, '
          f'Wav2Letter mid_layers={args.mid_layers}, dither off (the two paths give the same texts: {same})')
    print(f'  transcribe_long (upload, VAD, cut on the device, features, infer, decode): {spread(t_long)}')
    print(f'  transcribe of the segments cut beforehand, same batches:                  {spread(t_cut)}')
    diffs = [x - y for x, y in zip(t_long, t_cut)]
    print(f'  difference, run by run: median {statistics.median(diffs):+.2f} ms, min {min(diffs):+.2f}, max {max(diffs):+.2f}')


if __name__ == '__main__':
    main()

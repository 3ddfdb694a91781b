#!/usr/bin/env python3
"""Length-bucketed batches (data.bucket_rungs, data/bucketing.py) against manifest-order batches on a synthetic corpus with a
speech-like length distribution, through the real loader and the real training step:

    python tools/bench_buckets.py [--utts 256] [--batch 8] [--rungs 6] [--epochs 4] [--scale 0.25] [--mid-layers 1] [--out FILE]

The corpus: ``--utts`` lengths drawn as clip(exp(N(ln 1200, 0.5)), 100, 3500) frames (numpy seed 0), scaled by ``--scale`` so
that a run takes well under a minute; every row is a (offset, duration) window of one white-noise WAV, with a short transcript.
Two legs train their own small Wav2Letter in this process, epoch by epoch in turn (off, on, off, on, ...), so that clock drift
and a busy host fall on both:

    off   data.bucket_rungs=0: manifest order, every batch padded to its own longest utterance (the behaviour without the feature)
    on    data.bucket_rungs=K: batches cut from one rung at a time, padded to the rung, reshuffled every epoch

Per leg and epoch: valid feature frames per second and ms per step (wall clock around the epoch, loader included, one device
synchronisation at its end), padding as a share of the valid frames, distinct step shapes, kernel plans measured (growth of
engine._tuned_shapes) and the steps recorded / replayed (replay.STATS).  The off leg walks the same batches in the same order
every epoch, so on a corpus this small its shapes do come back after one epoch; on a real corpus an epoch has thousands of
shapes and nothing is kept that long (replay.MAX_GROUPS) -- epoch 0 is the off leg's steady state there."""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd import engine as E, replay, train as T  # noqa: E402
from wav2letter_pytorch_amd.data import label_sets  # noqa: E402

HOP, RATE = 160, 16000


def write_corpus(root, utts, scale):
    g = np.random.default_rng(0)
    frames = np.clip(np.exp(g.normal(np.log(1200), 0.5, utts)), 100, 3500)
    frames = np.maximum((frames * scale).astype(np.int64), 12)
    longest = int(frames.max()) * HOP
    noise = (0.2 * g.standard_normal(2 * longest)).clip(-1, 1)
    path = os.path.join(root, 'noise.wav')
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(RATE)
        w.writeframes((noise * 32767).astype('<i2').tobytes())
    letters = 'abcdefghijklmnopqrstuvwxyz'
    man = os.path.join(root, 'train.json')
    with open(man, 'w') as f:
        for i, t in enumerate(frames):
            n = (int(t) - 1) * HOP + int(g.integers(0, HOP))                   # 1 + n // HOP == t
            offset = int(g.integers(0, longest)) / RATE
            text = ''.join(letters[int(c)] for c in g.integers(0, 26, max(2, min(int(t) // 8, 20))))
            f.write(json.dumps(dict(audio_filepath=path, text=text, offset=offset, duration=(n + 0.5) / RATE)) + '\n')
    return man, frames


class Leg:
    def __init__(self, name, manifest, args, rungs):
        self.name = name
        cfg = T.build_config([f'data.train_manifest={manifest}', f'data.val_manifest={manifest}', f'data.batch_size={args.batch}',
                              f'model.mid_layers={args.mid_layers}', f'data.bucket_rungs={rungs}'])
        if type(cfg.model.labels) is str:
            cfg.model.labels = list(label_sets.labels_map[cfg.model.labels])
        cfg.model.decoder.labels = cfg.model.labels
        self.loader, _ = T.get_data_loaders(cfg.model.labels, cfg.data)
        torch.manual_seed(1)
        self.model = T.name_to_model[cfg.model.name](cfg.model).cuda().train()
        optimizers, _ = self.model.configure_optimizers()
        self.opt = self.model._optimizers = optimizers[0]
        if hasattr(self.opt, 'overlap'):
            self.opt.overlap = True
        self.rows = []

    def epoch(self, epoch):
        sampler = self.loader.batch_sampler
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)
        stats0 = {k: v for k, v in replay.STATS.items() if isinstance(v, int)}
        tuned0, shapes, cells, valid, steps = len(E._tuned_shapes), set(), 0, 0, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, batch in enumerate(self.loader):
            self.opt.zero_grad(set_to_none=True)
            loss = self.model.training_step(batch, i)
            loss.backward()
            self.opt.step()
            self.model.on_train_batch_end(loss, batch, i)
            shapes.add(tuple(batch[0].shape))
            cells += batch[0].shape[0] * batch[0].shape[2]
            valid += int(batch[1].sum())
            steps += 1
        getattr(self.opt, 'join', lambda: None)()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        self.model.resolve_metrics(wait_all=True)
        row = dict(leg=self.name, epoch=epoch, steps=steps, valid_frames_per_s=valid / dt, ms_per_step=1e3 * dt / steps,
                   padded_share=(cells - valid) / valid, shapes=len(shapes), plans_measured=len(E._tuned_shapes) - tuned0,
                   **{k: replay.STATS[k] - v for k, v in stats0.items() if k in ('recorded', 'replayed_F', 'replayed_B')},
                   loss=float(loss.detach()))
        self.rows.append(row)
        return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=256)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rungs', type=int, default=6)
    ap.add_argument('--epochs', type=int, default=4)
    ap.add_argument('--scale', type=float, default=0.25)
    ap.add_argument('--mid-layers', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as root:
        man, frames = write_corpus(root, args.utts, args.scale)
        say(f'# bench_buckets: {args.utts} utterances, {int(frames.min())}..{int(frames.max())} frames (median '
            f'{int(np.median(frames))}), batch {args.batch}, {args.rungs} rungs, Wav2Letter mid_layers={args.mid_layers}, '
            f'{torch.cuda.get_device_name(0)}')
        legs = [Leg('off', man, args, 0), Leg('on', man, args, args.rungs)]
        say(f'# ladder: {legs[1].loader.ladder}; replay {"on" if replay.ENABLED else "off"}, {replay.MAX_GROUPS} shapes kept, '
            f'{replay.WARM_STEPS} warm steps')
        say(f'{"leg":>4} {"epoch":>5} {"steps":>5} {"frames/s":>10} {"ms/step":>8} {"padding":>8} {"shapes":>6} {"plans":>6} '
            f'{"recorded":>8} {"replayed F/B":>12}')
        for epoch in range(args.epochs):
            for leg in legs:
                r = leg.epoch(epoch)
                say(f'{r["leg"]:>4} {r["epoch"]:>5} {r["steps"]:>5} {r["valid_frames_per_s"]:>10.0f} {r["ms_per_step"]:>8.2f} '
                    f'{100 * r["padded_share"]:>7.1f}% {r["shapes"]:>6} {r["plans_measured"]:>6} {r["recorded"]:>8} '
                    f'{r["replayed_F"]:>5}/{r["replayed_B"]:<6}')
        for leg in legs:
            rows = leg.rows
            total = sum(r['steps'] * r['ms_per_step'] for r in rows) / 1e3
            valid = sum(r['valid_frames_per_s'] * r['steps'] * r['ms_per_step'] / 1e3 for r in rows)
            say(f'# {leg.name:>3}: {args.epochs} epochs in {total:.2f} s, {valid / total:.0f} valid frames/s, '
                f'{1e3 * total / sum(r["steps"] for r in rows):.2f} ms/step, {sum(r["plans_measured"] for r in rows)} plans measured, '
                f'{sum(r["replayed_F"] for r in rows)} of {sum(r["steps"] for r in rows)} steps replayed; '
                f'poisoned: {replay.STATS["poisoned"]}')
        say('RESULT ' + json.dumps({leg.name: leg.rows for leg in legs}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

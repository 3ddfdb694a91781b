"""Length-bucketed batches (data/bucketing.py, data.bucket_rungs) on a real MI355X: the feature front end pads a batch to a
given width with exact zeros and leaves everything else bit for bit as it was; a bucketed loader built by train.get_data_loaders
yields batches whose widths are rungs of the ladder, whose rows still belong together and which are exactly the unbucketed
collate's batches plus zero columns; and a Trainer.fit over such a loader reaches the state the feature exists for -- every
step of a late epoch replayed from a recorded launch list, no kernel plan measured after the first epoch."""
import json
import math
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CONF = dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=16000)
N_UTTS, BATCH, RUNGS = 24, 4, 3


def _write_wav(path, samples, sr=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(samples, -1, 1) * 32767).astype('<i2').tobytes())


def test_pad_frames_appends_exact_zero_columns():
    from wav2letter_pytorch_amd.data.data_loader import SpectrogramExtractor
    ext = SpectrogramExtractor(CONF, mel_spec=64)
    g = np.random.default_rng(3)
    audio = [(0.2 * g.standard_normal(n)).astype(np.float32) for n in (4800, 9600, 7321)]           # 0.3 s, 0.6 s, 0.46 s
    plain, lens = ext.extract_batch(audio, noise=False)
    tmax = plain.shape[2]
    assert tmax == 1 + 9600 // 160
    for width in (tmax, tmax + 1, 64, 160, lambda t: t + 19):                # (64 and 160: other grid sizes of both kernels)
        padded, lens_p = ext.extract_batch(audio, noise=False, pad_frames=width)
        want = width(tmax) if callable(width) else width
        assert padded.shape == (3, 64, want) and padded.is_contiguous()
        assert torch.equal(padded[:, :, :tmax], plain)                       # bit for bit
        assert not padded[:, :, tmax:].any()                                 # exact zeros
        assert torch.equal(lens_p, lens) and lens_p.dtype == torch.int32
    for i, n in enumerate((4800, 9600, 7321)):
        assert int(lens[i]) == 1 + n // 160 and not plain[i, :, int(lens[i]):].any()
    with pytest.raises(ValueError):
        ext.extract_batch(audio, noise=False, pad_frames=tmax - 1)


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """24 WAV files of pairwise distinct lengths, 0.3 s .. 1.2 s in a fixed scrambled order, and their manifest"""
    root = tmp_path_factory.mktemp('buckets')
    g = np.random.default_rng(0)
    lengths = [4800 + 626 * i for i in g.permutation(N_UTTS)]                # 31 .. 120 frames, about 4 frames apart
    alphabet = 'abcdefghijklmnopqrstuvwxyz'
    rows = []
    for i, n in enumerate(lengths):
        path = root / f'u{i:02d}.wav'
        _write_wav(path, 0.2 * g.standard_normal(n))
        rows.append(dict(audio_filepath=str(path), text=alphabet[i] + alphabet[(i + 7) % 26] + ' ' + alphabet[(i + 13) % 26]))
    man = str(root / 'train.json')
    with open(man, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in rows) + '\n')
    return dict(manifest=man, rows=rows, frames=[1 + n // 160 for n in lengths])


def _loaders(corpus, *overrides):
    from wav2letter_pytorch_amd import train as T
    from wav2letter_pytorch_amd.data import label_sets
    cfg = T.build_config([f'data.train_manifest={corpus["manifest"]}', f'data.val_manifest={corpus["manifest"]}',
                          f'data.batch_size={BATCH}', 'model.mid_layers=1'] + list(overrides))
    if type(cfg.model.labels) is str:
        cfg.model.labels = list(label_sets.labels_map[cfg.model.labels])
    cfg.model.decoder.labels = cfg.model.labels
    train, val = T.get_data_loaders(cfg.model.labels, cfg.data)
    return cfg, train, val


def test_bucketed_loader_end_to_end(corpus):
    from wav2letter_pytorch_amd import train as T
    from wav2letter_pytorch_amd.data import bucketing as B
    from wav2letter_pytorch_amd.data.data_loader import BatchAudioDataLoader, _RawItems
    cfg, train, val = _loaders(corpus, f'data.bucket_rungs={RUNGS}')
    _, plain, _ = _loaders(corpus)
    assert len(set(corpus['frames'])) == N_UTTS
    assert B.nominal_frames(train._spect_ds).tolist() == corpus['frames']
    ladder = train.ladder
    assert ladder == B.choose_ladder(corpus['frames'], RUNGS, 16) and len(ladder) == RUNGS and val.ladder == ladder
    for ds in (train._spect_ds, plain._spect_ds):
        ds.extractor.dithering = 0.0                                         # (the dither is random; everything else is compared)
    text_of = {r['audio_filepath']: r['text'] for r in corpus['rows']}
    frames_of = {r['audio_filepath']: t for r, t in zip(corpus['rows'], corpus['frames'])}
    index_of = {r['audio_filepath']: i for i, r in enumerate(corpus['rows'])}
    model = T.name_to_model[cfg.model.name](cfg.model).cuda().eval()
    unbucketed = BatchAudioDataLoader(plain._spect_ds, batch_size=BATCH)
    raw = _RawItems(plain._spect_ds)
    widths, seen = [], []
    train.batch_sampler.set_epoch(2)
    for inputs, il, tg, tl, paths, texts in train:
        n, _, t = inputs.shape
        widths.append(t)
        assert n == BATCH and t in ladder                                    # every batch's T is a rung ...
        assert t == B.rung_for(ladder, int(il.max()))[0]                     # ... the smallest that holds it
        assert [text_of[p] for p in paths] == list(texts)                    # rows still belong together
        assert il.tolist() == [frames_of[p] for p in paths]
        assert [int(v) for v in tl] == [len(text_of[p].replace('_', '')) for p in paths]
        seen += list(paths)
        # the same rows through the unbucketed collate, zero-padded to the rung: the same tensor, the same model output
        want, wil, wtg, wtl, wpaths, _ = unbucketed._device_collate([raw[index_of[p]] for p in paths])
        assert want.shape[2] == int(il.max()) and tuple(wpaths) == tuple(paths)
        want = F.pad(want, (0, t - want.shape[2]))
        assert torch.equal(inputs, want) and torch.equal(il, wil) and torch.equal(tg, wtg) and torch.equal(tl, wtl)
        with torch.no_grad():
            got_out, got_lens = model(inputs, il)
            want_out, want_lens = model(want, wil)
        assert torch.equal(got_out, want_out) and torch.equal(got_lens, want_lens)
        assert torch.isfinite(got_out).all()
    assert sorted(seen) == sorted(text_of) and train.off_ladder == 0         # every row once
    assert len(set(widths)) <= RUNGS
    assert len({b[0].shape[2] for b in plain}) == N_UTTS // BATCH            # manifest order: 6 batches, 6 widths
    assert [b[0].shape[2] for b in val] == sorted(b[0].shape[2] for b in val) and len(list(val)) == N_UTTS // BATCH
    # a batch longer than the top rung (a ladder from another corpus) is padded to the next multiple, counted, and still usable
    low = BatchAudioDataLoader(train._spect_ds, batch_size=BATCH, ladder=[32, 48], align=16)
    shapes = [b[0].shape[2] for b in low]
    longest = [max(corpus['frames'][i:i + BATCH]) for i in range(0, N_UTTS, BATCH)]
    assert shapes == [B.rung_for([32, 48], t, 16)[0] for t in longest] and low.off_ladder == sum(t > 48 for t in longest) > 0


def test_trainer_replays_every_step_of_a_bucketed_epoch(corpus, tmp_path):
    """six epochs over the bucketed loader: a shape is recorded once it has come back (two eager steps, two recordings, then
    replays), so by the last epoch every step, forward and backward, is a replay, and no kernel plan was measured after the
    first epoch -- what manifest-order batches of six distinct widths never reach"""
    from wav2letter_pytorch_amd import engine as E, replay, train as T
    from wav2letter_pytorch_amd.data.bucketing import rung_for
    from wav2letter_pytorch_amd.trainer import Trainer
    cfg, train, _ = _loaders(corpus, f'data.bucket_rungs={RUNGS}')
    torch.manual_seed(3)
    model = T.name_to_model[cfg.model.name](cfg.model)
    replay.STATS['poisoned'] = []
    tr = Trainer(default_root_dir=str(tmp_path), max_epochs=6, enable_checkpointing=False, log_every_n_steps=1)
    tr.fit(model, train)
    epochs = tr.bucket_logged
    print('replay.STATS[poisoned] =', replay.STATS['poisoned'])
    for rec in epochs:
        print({k: v for k, v in rec.items() if k != 'ladder'})
    assert len(epochs) == 6 and all(rec['steps'] == N_UTTS // BATCH for rec in epochs)
    assert train.batch_sampler.epoch == 5                                    # Trainer.fit called set_epoch on the batch sampler
    assert all(rec['ladder'] == train.ladder and len(rec['shapes']) <= RUNGS and rec['off_ladder'] == 0 for rec in epochs)
    assert all(shape[0] == BATCH and shape[2] in train.ladder for rec in epochs for shape in rec['shapes'])
    last = epochs[-1]
    assert last['replayed_F'] == last['steps'] and last['replayed_B'] == last['steps'], (last, replay.STATS['poisoned'])
    assert [rec['tuned_shapes'] for rec in epochs[1:]] == [epochs[0]['tuned_shapes']] * 5, [rec['tuned_shapes'] for rec in epochs]
    assert len(E._tuned_shapes) == epochs[0]['tuned_shapes']
    valid = sum(corpus['frames'])
    padded = sum(rung_for(train.ladder, max(corpus['frames'][i] for i in b))[0] * len(b)
                 for b in train.batch_sampler.global_batches()) - valid
    assert last['padded_share'] == pytest.approx(padded / valid, rel=1e-12)
    losses = [logs['train_loss'] for _, logs in tr.logged]
    assert len(losses) == 6 * (N_UTTS // BATCH) and all(math.isfinite(v) for v in losses), losses

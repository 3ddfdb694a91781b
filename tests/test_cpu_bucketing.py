"""Length-bucketed batches (wav2letter_pytorch_amd/data/bucketing.py), host side: the ladder is the exact optimum (against a
brute force over all rung subsets), the padding it leaves on a LibriSpeech-like length distribution is a small fraction of what
manifest-order pad-to-longest batches leave, the batch sampler covers every row, keeps every rank on the same rung at the same
step, is reproducible from (seed, epoch) and leaves the global random generators alone, nominal_frames reads lengths from the
manifest or the file headers, the host collate pads to the rung, and data.bucket_rungs=0 leaves train.get_data_loaders as it
was."""
import itertools
import json
import random
import wave

import numpy as np
import pytest
import torch

from wav2letter_pytorch_amd.data import bucketing as B

CONF = dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=16000)


def _up(t, align):
    return -(-t // align) * align


def _brute(frames, rungs, align, headroom):
    """the least ladder cost over every subset of at most ``rungs`` candidate rungs that contains a sufficient top rung"""
    top = _up(max(int(np.ceil(max(frames) * headroom)), max(frames)), align)
    cand = sorted({_up(int(t), align) for t in frames} | {top})
    best = None
    for k in range(1, rungs + 1):
        for sub in itertools.combinations(cand, k):
            if sub[-1] < top:
                continue
            c = B.ladder_cost(frames, sub)
            best = c if best is None or c < best else best
    return best


def test_ladder_is_the_exact_optimum():
    g = np.random.default_rng(7)
    for case in range(200):
        pool = g.integers(1, 400, size=int(g.integers(1, 11)))               # at most 10 distinct lengths
        frames = g.choice(pool, size=int(g.integers(1, 40)))
        rungs, align = int(g.integers(1, 4)), int(g.choice([1, 4]))
        headroom = float(g.choice([1.0, 1.0, 1.0 / 0.9]))
        ladder = B.choose_ladder(frames, rungs, align, headroom)
        assert 1 <= len(ladder) <= rungs
        assert all(b > a for a, b in zip(ladder, ladder[1:])) and all(r % align == 0 for r in ladder), ladder
        assert ladder[-1] >= int(np.ceil(frames.max() * headroom)), (ladder, frames.max(), headroom)
        assert B.ladder_cost(frames, ladder) == _brute(frames.tolist(), rungs, align, headroom), (case, frames, ladder)
        assert ladder == B.choose_ladder(frames[::-1].copy(), rungs, align, headroom)          # deterministic, order-free


def test_ladder_ties_go_to_fewer_rungs_and_bad_arguments_raise():
    assert B.choose_ladder([32, 32, 32], 3, 16) == [32]
    assert B.choose_ladder([5, 17, 33], 3, 16) == [16, 32, 48]
    assert B.choose_ladder([5, 6, 7], 3, 16) == [16]
    assert B.choose_ladder([100], 2, 16, headroom=1 / 0.9) == [112]
    for bad in (dict(frames=[], rungs=2), dict(frames=[10], rungs=0), dict(frames=[10], rungs=1, align=0),
                dict(frames=[0, 5], rungs=1), dict(frames=[10], rungs=1, headroom=0.5)):
        with pytest.raises(ValueError):
            B.choose_ladder(**bad)
    assert B.rung_for([16, 48], 16) == (16, True) and B.rung_for([16, 48], 17) == (48, True)
    assert B.rung_for([16, 48], 50, 16) == (64, False)
    with pytest.raises(ValueError):
        B.ladder_cost([50], [16, 48])


def _lengths(seed, n=512):
    """the length distribution of the issue's simulation: log-normal around 12 s of 10 ms frames, clipped to 1 s .. 35 s"""
    return np.clip(np.exp(np.random.default_rng(seed).normal(np.log(1200), 0.5, n)), 100, 3500).astype(np.int64)


def _recount(sampler, frames, world):
    """(padded, valid) frames of the sampler's epoch, recounted from the batches every rank draws"""
    per_rank = [list(BS) for BS in (_rank(sampler, r, world) for r in range(world))]
    padded = valid = 0
    for step in zip(*per_rank):
        rows = [i for b in step for i in b]
        rung = B.rung_for(sampler.ladder, int(frames[rows].max()))[0]
        padded += rung * len(rows) - int(frames[rows].sum())
        valid += int(frames[rows].sum())
    return padded, valid


def _rank(s, rank, world):
    r = B.BucketBatchSampler(s.frames, s.batch_size, s.ladder, shuffle=s.shuffle, seed=s.seed, drop_last=s.drop_last,
                             num_replicas=world, rank=rank)
    r.set_epoch(s.epoch)
    return r


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_padding_on_a_speech_like_length_distribution(seed):
    frames = _lengths(seed)
    valid = int(frames.sum())
    ladder = B.choose_ladder(frames, 6, 16)
    assert len(ladder) == 6
    cost = B.ladder_cost(frames, ladder) - valid                             # the padding of a perfect packing
    print(f'seed {seed}: ladder {ladder}, ladder padding {cost / valid:.4f}')
    assert cost <= 0.16 * valid
    in_order = sum(int(frames[i:i + 16].max()) * len(frames[i:i + 16]) for i in range(0, len(frames), 16)) - valid
    assert in_order > 1.0 * valid
    for world in (1, 2, 4):
        G = 16 * world
        s = B.BucketBatchSampler(frames, 16, ladder, shuffle=True, seed=3, num_replicas=world)
        padded, counted = _recount(s, frames, world)
        print(f'  world {world}: padded share {s.padded_frames / s.valid_frames:.4f}, manifest order {in_order / valid:.4f}')
        assert (s.padded_frames, s.valid_frames) == (padded, counted)
        repeats = counted - valid                                            # frames of the rows repeated to fill the last step
        # every rung carries fewer than G rows upwards, none further than to the top rung
        assert s.padded_frames <= cost + (G - 1) * sum(ladder[-1] - r for r in ladder) + repeats
        if world == 1:
            assert repeats == 0 and s.padded_frames <= 0.25 * valid
        assert s.padded_frames / s.valid_frames < in_order / valid


@pytest.mark.parametrize('world', [1, 2, 4])
@pytest.mark.parametrize('shuffle', [False, True])
def test_sampler_covers_every_row_and_keeps_ranks_in_step(world, shuffle):
    frames = _lengths(5, 203)                                                # 203: no multiple of any global batch
    rungs, batch = 4, 6
    G = batch * world
    ladder = B.choose_ladder(frames, rungs, 16)
    ranks = [B.BucketBatchSampler(frames, batch, ladder, shuffle=shuffle, seed=9, num_replicas=world, rank=r) for r in range(world)]
    for s in ranks:
        s.set_epoch(1)
    drawn = [list(s) for s in ranks]
    assert len({len(d) for d in drawn}) == 1 and len(drawn[0]) == len(ranks[0])                # equal step counts
    seen = [i for d in drawn for b in d for i in b]
    assert set(seen) == set(range(len(frames)))
    assert len(seen) - len(frames) <= G - 1                                  # repeated rows: fewer than a global batch
    shapes = set()
    for step in zip(*drawn):
        rows = np.concatenate([np.asarray(b) for b in step])
        assert B.rung_for(ladder, int(frames[rows].max()))[1]                # every batch fits a rung
        per_rank = {(len(b), B.rung_for(ladder, int(frames[b].max()))[0]) for b in step}
        assert len(per_rank) == 1, per_rank                                  # the same (N, rung) on every rank at this step
        shapes |= per_rank
        valid = [int(frames[b].sum()) for b in step]
        assert max(valid) - min(valid) <= int(frames[rows].max() - frames[rows].min())         # near-equal valid frames
    assert len(shapes) <= rungs + 1, shapes
    # drop_last: only whole global batches, every row at most once
    d = B.BucketBatchSampler(frames, batch, ladder, shuffle=shuffle, seed=9, drop_last=True, num_replicas=world)
    rows = [i for b in d.global_batches() for i in b]
    assert len(rows) == len(set(rows)) == len(frames) // G * G and all(len(b) == G for b in d.global_batches())


def test_sampler_is_reproducible_and_leaves_global_generators_alone():
    frames = _lengths(6, 150)
    ladder = B.choose_ladder(frames, 3, 16)
    random.seed(123)
    torch.manual_seed(456)
    py0, t0 = random.getstate(), torch.get_rng_state()
    a = B.BucketBatchSampler(frames, 8, ladder, seed=4)
    b = B.BucketBatchSampler(frames, 8, ladder, seed=4)
    e0 = list(a)
    a.set_epoch(3)
    b.set_epoch(3)
    e3 = list(a)
    assert e3 == list(b) and e3 == list(a)                                   # (seed, epoch) fixes the epoch
    assert e3 != e0                                                          # another epoch, another order
    b.set_epoch(0)
    assert list(b) == e0
    assert B.BucketBatchSampler(frames, 8, ladder, seed=5).global_batches() != a.global_batches()
    plain = B.BucketBatchSampler(frames, 8, ladder, shuffle=False)
    first = plain.global_batches()
    plain.set_epoch(7)
    assert plain.global_batches() == first                                   # unshuffled: every epoch alike
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)


def _write_wav(path, n, sr=16000, channels=1):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.zeros(n * channels, dtype='<i2').tobytes())


class _Rows:
    """what nominal_frames reads of a SpectrogramDataset"""

    def __init__(self, rows, resample=False):
        self.rows, self.resample = rows, resample
        self.sample_rate, self.window_stride = 16000, 0.01

    def __len__(self):
        return len(self.rows)


def test_nominal_frames_from_durations_and_headers(tmp_path):
    from wav2letter_pytorch_amd.data.resample import output_length, resample_ratio
    _write_wav(tmp_path / 'a.wav', 8000)
    _write_wav(tmp_path / 'b.wav', 12345)
    _write_wav(tmp_path / 'c.wav', 22050, sr=22050, channels=2)
    a, b, c = (str(tmp_path / f) for f in ('a.wav', 'b.wav', 'c.wav'))
    rows = [dict(audio_filepath=a, offset=0, duration=-1), dict(audio_filepath=b, offset=0, duration=-1),
            dict(audio_filepath=b, offset=0.1, duration=-1), dict(audio_filepath=b, offset=0.1, duration=0.3),
            dict(audio_filepath='/nonexistent.wav', offset=0, duration=1.5)]            # a duration needs no file
    ds = _Rows(rows)
    got = B.nominal_frames(ds)
    assert got.dtype == np.int64
    assert got.tolist() == [1 + 8000 // 160, 1 + 12345 // 160, 1 + (12345 - 1600) // 160, 1 + 4800 // 160, 1 + 24000 // 160]
    assert B.nominal_frames(ds) is got                                       # cached on the dataset
    rs = _Rows([dict(audio_filepath=c, offset=0, duration=-1), dict(audio_filepath=c, offset=0, duration=0.5),
                dict(audio_filepath=a, offset=0, duration=-1)], resample=True)
    r = resample_ratio(22050, 16000)
    assert B.nominal_frames(rs).tolist() == [1 + output_length(22050, r) // 160, 1 + output_length(11025, r) // 160, 51]


def test_host_collate_pads_to_the_rung():
    from wav2letter_pytorch_amd.data import data_loader as DL
    g = torch.Generator().manual_seed(0)
    items = [(torch.randn(5, t, generator=g), [1, 2], f'f{t}', f't{t}') for t in (7, 19, 12)]
    plain = DL._collator(items)
    padded = DL._collator(items, ladder=[16, 32, 64])
    assert padded[0].shape == (3, 5, 32)
    assert torch.equal(padded[0][:, :, :19], plain[0]) and not padded[0][:, :, 19:].any()
    for a, b in zip(plain[1:4], padded[1:4]):
        assert torch.equal(a, b)
    assert padded[4:] == plain[4:]
    assert DL._collator(items, ladder=[8, 16], align=8)[0].shape == (3, 5, 24)           # above the top rung: the next multiple
    loader = DL.BatchAudioDataLoader(items, batch_size=3, ladder=[8, 16], align=8)
    assert next(iter(loader))[0].shape == (3, 5, 24) and loader.off_ladder == 1
    loader = DL.BatchAudioDataLoader(items, batch_size=2, ladder=[16, 32])
    assert [tuple(b[0].shape) for b in loader] == [(2, 5, 32), (1, 5, 16)] and loader.off_ladder == 0


class _NoExtractor:
    def __init__(self, *a, **k):
        pass


def _manifests(tmp_path, lengths):
    rows = []
    for i, n in enumerate(lengths):
        _write_wav(tmp_path / f'u{i}.wav', n)
        rows.append(dict(audio_filepath=str(tmp_path / f'u{i}.wav'), text='ab'))
    man = str(tmp_path / 'm.json')
    with open(man, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in rows) + '\n')
    return man


def test_config_keys_and_loaders(tmp_path, monkeypatch):
    """data.bucket_rungs=0 (the default) builds the loaders as before; K > 0 builds bucketed ones for both manifests"""
    from torch.utils.data import SequentialSampler
    from wav2letter_pytorch_amd import train as T
    from wav2letter_pytorch_amd.config import bucket_options
    from wav2letter_pytorch_amd.data import data_loader as DL
    monkeypatch.setattr(DL, 'SpectrogramExtractor', _NoExtractor)            # (the extractor needs a GPU; nothing here extracts)
    man = _manifests(tmp_path, [4000 + 700 * i for i in range(11)])
    cfg = T.build_config([f'data.train_manifest={man}', f'data.val_manifest={man}'])
    assert bucket_options(cfg.data) == dict(rungs=0, align=16, shuffle=True, seed=0, drop_last=False)
    labels = list('_ab')
    for loader in T.get_data_loaders(labels, cfg.data):
        assert type(loader) is DL.BatchAudioDataLoader and loader.ladder is None and loader.off_ladder == 0
        assert isinstance(loader.sampler, SequentialSampler) and loader.batch_size == cfg.data.batch_size
        assert type(loader.batch_sampler) is torch.utils.data.BatchSampler and not loader.drop_last
        assert loader.collate_fn == loader._device_collate
        assert [b for b in loader.batch_sampler] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    cfg = T.build_config([f'data.train_manifest={man}', f'data.val_manifest={man}', 'data.bucket_rungs=2', 'data.bucket_seed=5',
                          'data.speed_perturb=0.9,1.0,1.1'])
    train, val = T.get_data_loaders(labels, cfg.data, rank=1, world=2)
    frames = B.nominal_frames(train._spect_ds)
    assert train.ladder == B.choose_ladder(frames, 2, 16, headroom=1 / 0.9) and train.ladder[-1] >= int(np.ceil(frames.max() / 0.9))
    assert val.ladder == B.choose_ladder(frames, 2, 16)
    for loader, shuffle in ((train, True), (val, False)):
        s = loader.batch_sampler
        assert isinstance(s, B.BucketBatchSampler) and (s.shuffle, s.seed, s.num_replicas, s.rank) == (shuffle, 5, 2, 1)
        assert s.batch_size == cfg.data.batch_size and not s.drop_last and len(loader) == len(s) == 2
    for bad in ('data.bucket_rungs=-1', 'data.bucket_rungs=2.5', 'data.bucket_align=0'):
        with pytest.raises(ValueError):
            T.build_config([f'data.train_manifest={man}', f'data.val_manifest={man}', bad])

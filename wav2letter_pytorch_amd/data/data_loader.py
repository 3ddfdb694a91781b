"""Data side of the training step with the reference's interface (data/data_loader.py): ``load_audio``,
``SpectrogramExtractor``, ``SpectrogramDataset``, ``_collator``, ``BatchAudioDataLoader``.

MI355X-first difference: features are not computed one utterance at a time on the host.  The loader reads raw audio,
pads it into one [N, L_max] buffer, moves it to the GPU once and runs the whole batch through three HIP launches
(w2l_logmel, w2l_feature_normalize: csrc/features.hip), which write the batch directly in the right-zero-padded
[N, n_mels, T_max] layout ``_collator`` (data_loader.py:149-158) produces.  ``SpectrogramExtractor.extract`` and
``SpectrogramDataset.__getitem__`` keep the reference's per-utterance semantics (same kernels, N = 1).
"""
from __future__ import annotations

import json
import math
import os
import wave
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .._lib import check, lib, ptr, stream_ptr
from .bucketing import rung_for
from .mel import mel_filterbank
from .resample import BankCache, SpeedPerturb, plan_rows, resample_device

_TORCH_WINDOWS = {'hann': torch.hann_window, 'hamming': torch.hamming_window, 'blackman': torch.blackman_window,
                  'bartlett': torch.bartlett_window, 'none': None}


def load_audio(path, duration=-1, offset=0):
    """float32 samples in [-1, 1) (data_loader.py:20-31).  Uses soundfile when it is installed (any format it reads);
    otherwise PCM / float WAV files through the standard library."""
    try:
        import soundfile as sf
    except ImportError:
        sf = None
    if sf is not None:
        with sf.SoundFile(path, 'r') as f:
            sr = f.samplerate
            if offset > 0:
                f.seek(int(offset * sr))
            samples = f.read(int(duration * sr), dtype='float32') if duration > 0 else f.read(dtype='float32')
        return samples.transpose()
    samples, sr = _read_wav(path)
    start = int(offset * sr) if offset > 0 else 0
    stop = start + int(duration * sr) if duration > 0 else None
    return samples[start:stop].transpose()


def read_audio(path, duration=-1, offset=0):
    """(mono float32 samples, sample rate): ``load_audio`` that keeps the file's rate and averages the channels -- what
    the resampling paths read (soundfile when it is installed, otherwise the standard-library WAV reader)."""
    try:
        import soundfile as sf
    except ImportError:
        sf = None
    if sf is not None:
        with sf.SoundFile(path, 'r') as f:
            sr = f.samplerate
            if offset > 0:
                f.seek(int(offset * sr))
            samples = f.read(int(duration * sr), dtype='float32') if duration > 0 else f.read(dtype='float32')
    else:
        samples, sr = _read_wav(path)
        start = int(offset * sr) if offset > 0 else 0
        stop = start + int(duration * sr) if duration > 0 else None
        samples = samples[start:stop]
    if samples.ndim > 1:
        samples = samples.mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(samples, dtype=np.float32), int(sr)


def _read_wav(path):
    try:
        with wave.open(path, 'rb') as w:
            sr, nch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
            raw = w.readframes(n)
        if width == 2:
            data = np.frombuffer(raw, dtype='<i2').astype(np.float32) / 32768.0
        elif width == 4:
            data = np.frombuffer(raw, dtype='<i4').astype(np.float32) / 2147483648.0
        elif width == 1:
            data = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
        else:
            raise ValueError(f'{path}: unsupported sample width {width}')
    except wave.Error:
        from scipy.io import wavfile                      # IEEE-float WAV
        sr, data = wavfile.read(path)
        nch = 1 if data.ndim == 1 else data.shape[1]
        data = data.astype(np.float32).reshape(-1)
    if nch > 1:
        data = data.reshape(-1, nch)
    return data, sr


def _sample_rate(path) -> int:
    try:
        import soundfile as sf
        return sf.info(path).samplerate
    except ImportError:
        pass
    try:
        with wave.open(path, 'rb') as w:                  # the header only
            return w.getframerate()
    except wave.Error:
        return _read_wav(path)[1]


class SpectrogramExtractor(torch.nn.Module):
    """Log-mel features (data_loader.py:33-88): dither 1e-5, pre-emphasis 0.97, STFT (n_fft = next power of two of the
    window, hop = window_stride, centred, reflect), power, mel, log1p(. + 2^-24), per-feature mean / (unbiased std + 1e-5)
    over time.  Buffers ``fb`` [1, n_mels, n_fft/2+1] and ``window`` carry the reference's names."""
    dithering = 1e-5
    preemph = 0.97
    epsilon = 1e-5
    log_zero_guard_value = 2 ** -24

    def __init__(self, audio_conf, mel_spec=64, use_cuda=False, device=None):
        super().__init__()
        sr = audio_conf['sample_rate']
        self.sample_rate = int(sr)
        self._banks = BankCache()                         # resampling filter banks per (P, Q), uploaded once
        self.win_length = int(sr * audio_conf['window_size'])
        self.hop_length = int(sr * audio_conf['window_stride'])
        self.n_fft = 2 ** math.ceil(math.log2(self.win_length))
        if mel_spec is None:
            raise ValueError('mel_spec is required (the reference builds a mel filterbank unconditionally, data_loader.py:39-43)')
        self.n_mels = int(mel_spec)
        fb = torch.from_numpy(mel_filterbank(sr, self.n_fft, self.n_mels, 0.0, sr / 2)).unsqueeze(0)
        self.register_buffer('fb', fb)
        fn = _TORCH_WINDOWS.get(audio_conf['window'], None)
        window = fn(self.win_length, periodic=False).float() if fn else torch.ones(self.win_length)
        self.register_buffer('window', window)
        self.register_buffer('_fbT', fb[0].t().contiguous(), persistent=False)
        nz = fb[0] != 0                                   # run of non-zero bins per filter: [first, one past last)
        first = torch.where(nz.any(1), nz.float().argmax(1), torch.zeros(self.n_mels, dtype=torch.long))
        last = torch.where(nz.any(1), fb.shape[2] - nz.flip(1).float().argmax(1), torch.zeros(self.n_mels, dtype=torch.long))
        self.register_buffer('_fb_range', torch.stack([first, last], 1).to(torch.int32).contiguous(), persistent=False)
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('SpectrogramExtractor runs on MI355X only (HIP kernels, no CPU path)')
            device = torch.device('cuda', torch.cuda.current_device())
        self.to(device)

    def n_frames(self, n_samples: int) -> int:
        return 1 + n_samples // self.hop_length

    # ------------------------------------------------------------------ batched device path
    def _launch(self, audio: torch.Tensor, lens: torch.Tensor, noise: Optional[torch.Tensor], take_log: bool, tmax: int):
        """``tmax``: the frames per row of the output, at least n_frames(audio row width); frames past a row's own are zeros"""
        n, lmax = audio.shape
        out = torch.empty(n, tmax, self.n_mels, dtype=torch.float32, device=audio.device)
        check(lib.w2l_logmel(ptr(audio), ptr(lens), ptr(noise), self.dithering, self.preemph, n, lmax, ptr(self.window),
                             self.win_length, self.n_fft, self.hop_length, ptr(self._fbT), ptr(self._fb_range), self.n_mels,
                             int(take_log),
                             float(self.log_zero_guard_value), ptr(out), tmax, stream_ptr()), 'w2l_logmel')
        return out

    def _stage(self, signals: Sequence, noise, rates=None, speeds=None, augment=None):
        dev = self.fb.device
        if dev.type != 'cuda':
            raise RuntimeError('SpectrogramExtractor runs on MI355X only (HIP kernels, no CPU path)')
        arrs = [np.asarray(s.detach().cpu() if torch.is_tensor(s) else s, dtype=np.float32).reshape(-1) for s in signals]
        lens = np.array([a.shape[0] for a in arrs], dtype=np.int32)
        rows = None
        if rates is not None or speeds is not None:
            # per-row ratio speed * rate / model rate; a batch whose rows are all 1/1 takes the plain path (same launches)
            rows = plan_rows(lens, rates, self.sample_rate, speeds, self._banks)
            if (rows[:, 2] == rows[:, 3]).all():
                rows = None
            else:
                lens = rows[:, 1].copy()
        if lens.min() <= self.n_fft // 2:
            raise ValueError(f'an utterance of {int(lens.min())} samples is shorter than the STFT reflect padding '
                             f'({self.n_fft // 2}); torch.stft rejects it in the reference too')
        host = torch.zeros(len(arrs), max(a.shape[0] for a in arrs), dtype=torch.float32).pin_memory()
        for i, a in enumerate(arrs):
            host[i, :a.shape[0]] = torch.from_numpy(a)
        audio = host.to(dev, non_blocking=True)
        if rows is not None:
            audio = resample_device(audio, rows, self._banks)         # [N, max n_out], zero past each row's n_out
        if augment is not None:
            augmenter, plan = augment                                  # reverberation, then noise: lengths unchanged
            audio = augmenter.apply(audio, lens, plan)
        lens_d = torch.from_numpy(lens).to(dev, non_blocking=True)
        if noise is None:
            noise_d = torch.randn(audio.shape, dtype=torch.float32, device=dev) if self.dithering > 0 else None
        elif noise is False:
            noise_d = None
        else:
            noise_d = torch.zeros_like(audio)
            for i, z in enumerate(noise):
                z = torch.as_tensor(np.asarray(z, dtype=np.float32))
                noise_d[i, :z.shape[0]] = z.to(dev)
        return audio, lens_d, noise_d, lens

    def extract_batch(self, signals: Sequence, noise=None, rates=None, speeds=None, augment=None, pad_frames=None):
        """signals: N 1-D float arrays (any lengths).  noise: None = draw the dither on the device, False = no dither, or N
        arrays of N(0,1) draws (parity tests inject the reference's).  Returns (inputs fp32 [N, n_mels, T_max] on the
        device, zero beyond each utterance's frames; input_lengths IntTensor [N] on the host) -- _collator's layout.
        rates (the signals' sample rates) / speeds (speed factors), either one given: the staged batch goes through
        w2l_resample (data/resample.py) first; lengths, the dither and the returned input_lengths are those of the resampled
        rows (noise arrays, if given, are at the resampled lengths).  Both None, or every row at 1/1: the plain path's launches.
        augment: (a WaveformAugment, the plan its draw() returned for these N rows) -- reverberation and noise on the staged
        waveforms, after the resampler and before the dither (data/augment_wave.py); a plan that selects nothing adds no launch.
        pad_frames: the output is [N, n_mels, pad_frames] instead: its first T_max columns are what the call without it returns,
        the rest zeros, input_lengths unchanged (length-bucketed batches, data/bucketing.py).  An int, or a callable T_max -> int
        (T_max is known only after resampling and speed perturbation); a width below T_max is a ValueError."""
        audio, lens_d, noise_d, lens = self._stage(signals, noise, rates, speeds, augment)
        tmax = self.n_frames(int(audio.shape[1]))
        if pad_frames is not None:
            width = int(pad_frames(tmax) if callable(pad_frames) else pad_frames)
            if width < tmax:
                raise ValueError(f'pad_frames={width} is below the T_max of this batch ({tmax} frames)')
            tmax = width
        logmel = self._launch(audio, lens_d, noise_d, True, tmax)
        n = audio.shape[0]
        mean = torch.empty(n, self.n_mels, dtype=torch.float32, device=audio.device)
        std = torch.empty_like(mean)
        out = torch.empty(n, self.n_mels, tmax, dtype=torch.float32, device=audio.device)
        check(lib.w2l_feature_normalize(ptr(logmel), ptr(lens_d), self.hop_length, n, tmax, self.n_mels, float(self.epsilon),
                                        ptr(mean), ptr(std), ptr(out), stream_ptr()), 'w2l_feature_normalize')
        return out, torch.from_numpy(1 + lens // self.hop_length).to(torch.int32)

    def extract_rows(self, audio: torch.Tensor, lens, noise=None):
        """``extract_batch`` for waveforms that already lie on the device (segmentation.transcribe_long cuts them from a
        resident recording): audio fp32 [B, L] contiguous on the extractor's device, row b valid up to lens[b] samples (host
        ints) and zero beyond; noise: None = draw the dither on the device, False = none, or a [B, L] device tensor of N(0,1)
        draws.  Same launches and the same returns as ``extract_batch`` on the same samples with L = max(lens): with the dither
        off the features are bit-identical."""
        dev = self.fb.device
        if dev.type != 'cuda':
            raise RuntimeError('SpectrogramExtractor runs on MI355X only (HIP kernels, no CPU path)')
        if not (torch.is_tensor(audio) and audio.dim() == 2 and audio.device == dev and audio.dtype == torch.float32
                and audio.is_contiguous()):
            raise ValueError('extract_rows wants a contiguous fp32 [B, L] tensor on the extractor\'s device')
        lens = np.asarray(lens, dtype=np.int32).reshape(-1)
        if lens.shape[0] != audio.shape[0] or lens.max() > audio.shape[1]:
            raise ValueError(f'{audio.shape[0]} rows of {audio.shape[1]} samples, lengths {lens.tolist()}')
        if lens.min() <= self.n_fft // 2:
            raise ValueError(f'an utterance of {int(lens.min())} samples is shorter than the STFT reflect padding '
                             f'({self.n_fft // 2}); torch.stft rejects it in the reference too')
        lens_d = torch.from_numpy(lens).to(dev, non_blocking=True)
        if noise is None:
            noise = torch.randn(audio.shape, dtype=torch.float32, device=dev) if self.dithering > 0 else None
        elif noise is False:
            noise = None
        n, tmax = audio.shape[0], self.n_frames(int(audio.shape[1]))
        logmel = self._launch(audio, lens_d, noise, True, tmax)
        mean = torch.empty(n, self.n_mels, dtype=torch.float32, device=dev)
        std = torch.empty_like(mean)
        out = torch.empty(n, self.n_mels, tmax, dtype=torch.float32, device=dev)
        check(lib.w2l_feature_normalize(ptr(logmel), ptr(lens_d), self.hop_length, n, tmax, self.n_mels, float(self.epsilon),
                                        ptr(mean), ptr(std), ptr(out), stream_ptr()), 'w2l_feature_normalize')
        return out, torch.from_numpy(1 + lens // self.hop_length).to(torch.int32)

    # ------------------------------------------------------------------ the reference's per-utterance methods
    def _get_spect(self, audio, noise=None):
        """mel power spectrogram [1, n_mels, T] (data_loader.py:64-72)"""
        a, lens_d, noise_d, _ = self._stage([audio], None if noise is None else [noise])
        out = self._launch(a, lens_d, noise_d, False, self.n_frames(int(a.shape[1])))
        return out.transpose(1, 2).contiguous()

    def extract(self, signal, noise=None):
        """normalised log-mel features [n_mels, T] (data_loader.py:75-88), on the extractor's device"""
        out, _ = self.extract_batch([signal], None if noise is None else [noise])
        return out[0]


class SpectrogramDataset(Dataset):
    """Manifest dataset (data_loader.py:90-147): a .csv (first column = index; columns audio_filepath, text[, offset,
    duration]) or JSON lines.  ``dataset[i]`` -> (spect [n_mels, T], target ids, path, transcript) as in the reference;
    ``dataset.raw(i)`` -> the same with the raw samples instead of features (what BatchAudioDataLoader batches).
    ``resample=True`` (not in the reference): files of any rate and channel count; every row is read with ``read_audio`` and
    converted to ``audio_conf['sample_rate']`` on the GPU, instead of the assertion on the first row's rate.
    ``speed_perturb``: a ``SpeedPerturb`` (or its factors), applied per utterance by BatchAudioDataLoader's batches only.
    ``wave_augment``: a ``WaveformAugment`` (reverberation and noise on the waveform), likewise for the loader's batches only.
    ``wildcard``: the transcripts' mark for "speech without text here" (``model.wildcard``, one character outside ``labels``); it
    becomes the target id ``len(labels)``, which ctc_loss.WildcardCTCLoss reads as its wildcard.  ``wildcard_ends``
    (``data.wildcard_ends``, needs ``wildcard``): one wildcard before and one after every target -- the transcript covers only
    part of the audio (W-CTC's use)."""

    def __init__(self, manifest_filepath, audio_conf, labels, mel_spec=None, use_cuda=False, resample=False, speed_perturb=None,
                 wave_augment=None, wildcard=None, wildcard_ends=False):
        super().__init__()
        rows = self._read_manifest(manifest_filepath)
        self.rows = rows
        self.size = len(rows)
        self.window_stride = audio_conf['window_stride']
        self.window_size = audio_conf['window_size']
        self.sample_rate = audio_conf['sample_rate']
        self.use_cuda = use_cuda
        self.mel_spec = mel_spec
        self.labels_map = dict([(labels[i], i) for i in range(len(labels))])
        if wildcard is not None and (len(wildcard) != 1 or wildcard in self.labels_map):
            raise ValueError(f'wildcard={wildcard!r}: the mark is one character that is none of the labels')
        if wildcard_ends and wildcard is None:
            raise ValueError('wildcard_ends needs a wildcard mark (model.wildcard)')
        self.wildcard = wildcard
        self.wildcard_id = len(labels)
        self.wildcard_ends = bool(wildcard_ends)
        self.resample = bool(resample)
        if speed_perturb is not None and not isinstance(speed_perturb, SpeedPerturb):
            speed_perturb = SpeedPerturb(speed_perturb)
        self.speed_perturb = speed_perturb
        self.wave_augment = wave_augment
        self._rates = {}
        if not self.resample:
            self.validate_sample_rate()
        self.extractor = SpectrogramExtractor(audio_conf, mel_spec, use_cuda)

    @staticmethod
    def _read_manifest(path) -> List[dict]:
        if path.endswith('.csv'):
            import pandas as pd
            rows = pd.read_csv(path, index_col=0).to_dict('records')
        else:
            with open(path) as f:
                rows = [json.loads(line) for line in f if line.strip()]
        for r in rows:
            r.setdefault('offset', 0)
            r.setdefault('duration', -1)
        return rows

    def _target(self, transcript):
        # filter(None, ...) drops unknown characters AND label 0, the blank (data_loader.py:127)
        if self.wildcard is None:
            return list(filter(None, [self.labels_map.get(c) for c in list(transcript)]))
        ids = [self.wildcard_id if c == self.wildcard else self.labels_map.get(c) for c in list(transcript)]
        ids = list(filter(None, ids))
        return [self.wildcard_id] + ids + [self.wildcard_id] if self.wildcard_ends else ids

    def rate(self, index) -> int:
        """sample rate of row ``index``: the model's unless ``resample``, else the file's (read once per row)"""
        if not self.resample:
            return self.sample_rate
        sr = self._rates.get(index)
        if sr is None:
            sr = self._rates[index] = int(_sample_rate(self.rows[index]['audio_filepath']))
        return sr

    def raw(self, index):
        r = self.rows[index]
        if self.resample:
            audio, self._rates[index] = read_audio(r['audio_filepath'], r['duration'], r['offset'])
        else:
            audio = load_audio(r['audio_filepath'], r['duration'], r['offset'])
        return audio, self._target(r['text']), r['audio_filepath'], r['text']

    def __getitem__(self, index):
        audio, target, path, text = self.raw(index)
        if self.resample:
            return self.extractor.extract_batch([audio], rates=[self.rate(index)])[0][0], target, path, text
        return self.extractor.extract(audio), target, path, text

    def parse_audio(self, audio_path, duration, offset):
        if self.resample:
            audio, sr = read_audio(audio_path, duration, offset)
            return self.extractor.extract_batch([audio], rates=[sr])[0][0]
        return self.extractor.extract(load_audio(audio_path, duration, offset))

    def validate_sample_rate(self):
        path = self.rows[0]['audio_filepath']
        sr = _sample_rate(path)
        assert sr == self.sample_rate, 'Expected sample rate %d but found %d in first file' % (self.sample_rate, sr)

    def __len__(self):
        return self.size

    def data_channels(self):
        return self.mel_spec or int(1 + (int(self.sample_rate * self.window_size) / 2))


def _pad_targets(targets):
    target_lengths = torch.IntTensor([len(t) for t in targets])
    longest = int(target_lengths.max()) if len(targets) else 0
    tg = torch.zeros(len(targets), longest, dtype=torch.int32)
    for i, t in enumerate(targets):
        if len(t):
            tg[i, :len(t)] = torch.as_tensor(list(t), dtype=torch.int32)
    return tg, target_lengths


def _collator(batch, ladder=None, align=16):
    """(spect, target, path, text) items -> (inputs [N, F, T_max] right-zero-padded, input_lengths, targets [N, S_max]
    zero-padded int32, target_lengths, paths, texts) -- data_loader.py:149-158.  Spectrograms may live on the device.
    ``ladder`` (ascending rungs, or a callable T_max -> width): the inputs are zero-padded to the smallest rung at or above
    T_max instead, above the top rung to the next multiple of ``align`` (data/bucketing.py); input_lengths are unchanged."""
    inputs, targets, file_paths, texts = zip(*batch)
    inputs = [torch.as_tensor(x) for x in inputs]
    input_lengths = torch.IntTensor([x.shape[1] for x in inputs])
    longest = int(input_lengths.max())
    if ladder is not None:
        longest = int(ladder(longest)) if callable(ladder) else rung_for(ladder, longest, align)[0]
    out = torch.zeros(len(inputs), inputs[0].shape[0], longest, dtype=torch.float32, device=inputs[0].device)
    for i, x in enumerate(inputs):
        out[i, :, :x.shape[1]] = x
    tg, target_lengths = _pad_targets(targets)
    return out, input_lengths, tg, target_lengths, file_paths, texts


class _RawItems(Dataset):
    def __init__(self, ds: SpectrogramDataset):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        item = self.ds.raw(i)
        return item + (self.ds.rate(i),) if self.ds.resample else item


class BatchAudioDataLoader(DataLoader):
    """DataLoader yielding the reference's 6-tuple batches (data_loader.py:160-163).  For a SpectrogramDataset the
    features of the whole batch are computed on the GPU in one pass from the raw audio.
    ``ladder`` (ascending rungs, data/bucketing.choose_ladder; None = off): every batch is padded to the smallest rung at or
    above its T_max -- the value after resampling and speed perturbation -- instead of to T_max itself, so that the stream of
    step shapes is a small repeating set.  A batch above the top rung is padded to the next multiple of ``align``, counted in
    ``off_ladder``, and still trains.  Usually paired with ``batch_sampler=BucketBatchSampler(...)``."""

    def __init__(self, dataset, *args, ladder=None, align=16, **kwargs):
        self.ladder = None if ladder is None else [int(r) for r in ladder]
        self.align = int(align)
        self.off_ladder = 0
        self._spect_ds = dataset if isinstance(dataset, SpectrogramDataset) else None
        if self._spect_ds is not None:
            if kwargs.get('num_workers', 0):
                raise ValueError('GPU feature extraction runs in the loader process: num_workers must be 0')
            super().__init__(_RawItems(dataset), *args, **kwargs)
            self.collate_fn = self._device_collate
        else:
            super().__init__(dataset, *args, **kwargs)
            self.collate_fn = _collator if self.ladder is None else self._ladder_collate

    def _pad_width(self, tmax: int) -> int:
        width, on = rung_for(self.ladder, tmax, self.align)
        if not on:
            self.off_ladder += 1
        return width

    def _ladder_collate(self, batch):
        return _collator(batch, self._pad_width)

    def _device_collate(self, batch):
        ds = self._spect_ds
        rates = None
        if ds.resample:
            audio, targets, file_paths, texts, rates = zip(*batch)
        else:
            audio, targets, file_paths, texts = zip(*batch)
        speeds = ds.speed_perturb.draw(len(audio)) if ds.speed_perturb is not None else None
        augment = None
        if ds.wave_augment is not None and ds.wave_augment.active:
            augment = (ds.wave_augment, ds.wave_augment.draw(len(audio)))
        inputs, input_lengths = ds.extractor.extract_batch(audio, rates=rates, speeds=speeds, augment=augment,
                                                           pad_frames=None if self.ladder is None else self._pad_width)
        tg, target_lengths = _pad_targets(targets)
        return inputs, input_lengths, tg, target_lengths, file_paths, texts

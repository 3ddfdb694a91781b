"""Command-line entry of the training flow, the counterpart of the reference's ``train.py:28-41`` for a machine without
Hydra / Lightning:

    python -m wav2letter_pytorch_amd.train [--config-dir /path/to/configuration] data.train_manifest=train.csv \\
           data.val_manifest=val.csv [model=jasper] [model.mid_layers=20] [trainer.max_epochs=1] \\
           [data.resample=true] [data.speed_perturb=0.9,1.0,1.1] \\
           [data.rir_manifest=rirs.csv data.rir_prob=0.5 data.rir_max_seconds=0.5] \\
           [data.noise_manifest=noise.csv data.noise_prob=0.5 data.snr_db=5,20] \\
           [data.bucket_rungs=6 data.bucket_align=16 data.bucket_shuffle=true data.bucket_seed=0 data.drop_last=false] ...

Same override syntax and config keys as ``python train.py ...``; without ``--config-dir`` the built-in copy of the
hyper-parameters (defaults.py) is used.  Manifests, labels, feature extraction and batching are data/data_loader.py's;
the fit loop is trainer.Trainer.  ``trainer.gpus=N`` (the reference's Lightning flag, README.md:40) starts N ranks of this
command line (launch.py), one per GPU; ``python -m torch.distributed.run --nproc-per-node N`` works too.  Every rank trains
on its own shard of the manifest and gradients are averaged with RCCL (distributed.GradReducer).  ``data.resample=true``:
manifests may mix sample rates and channel counts (converted on the GPU, data/resample.py); ``data.speed_perturb=`` draws one
speed factor per training utterance.  ``data.rir_manifest=`` / ``data.noise_manifest=`` (manifests with an ``audio_filepath``
column; data/augment_wave.py) augment the training waveforms on the GPU: with probability ``data.rir_prob`` an utterance is
convolved with one of the room impulse responses (each cut ``data.rir_max_seconds`` after its peak), then with probability
``data.noise_prob`` a noise clip is added at an SNR drawn from ``data.snr_db=lo,hi``.  Validation is never augmented.
``model.scheduler_interval=step`` steps the learning-rate scheduler after every optimizer step instead of once per epoch
(warm-up schedules; ``model.optimizer._target_=torch.optim.AdamW`` then runs as optim.FusedAdamW without re-recording).
``data.bucket_rungs=K`` (0, the default: off) batches utterances of similar length together and pads every batch to one of K
widths chosen from the manifest (data/bucketing.py): the step then meets at most K + 1 shapes, which are tuned once and replayed,
instead of a new one per batch; ``data.bucket_shuffle`` / ``data.bucket_seed`` shuffle the rows inside each width and the batch
order per epoch, ``data.drop_last`` drops the one short batch.
``model.wildcard='*'`` names a mark character: where a transcript holds it, there is speech the text does not cover, and the
criterion becomes ctc_loss.WildcardCTCLoss (``model.wildcard_penalty``, <= 0, is the log-domain cost per frame spent there);
``data.wildcard_ends=true`` puts one wildcard before and after every training and validation target.  CER / WER score the
transcripts without the mark."""
from __future__ import annotations

import os
import sys

from .config import bucket_options, criterion_name, load_config, override_value, scheduler_interval, to_cfg, wildcard_options
from .launch import spawn_ranks, under_launcher

# Nothing above maps libw2l_hip.so (or imports torch): with trainer.gpus=N this process only starts the ranks, and a launch
# parent must not have touched the GPU (launch.py; bench.py follows the same rule).  The model / data / trainer modules are
# imported where a rank first needs them.


class _Models(dict):
    """``name_to_model`` of the reference's train.py:15-19.  The model classes pull in torch and the HIP library, which a
    launch parent must not map, so the table fills itself the first time ANY read touches it -- lookups, ``in``, ``get``,
    iteration, ``len`` -- and behaves like the reference's plain dict from then on."""

    def _fill(self):
        if not dict.__len__(self):
            from . import Jasper, Wav2Letter
            dict.update(self, jasper=Jasper, wav2letter=Wav2Letter)
        return self

    def __missing__(self, key):
        if dict.__contains__(self._fill(), key):
            return dict.__getitem__(self, key)
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self._fill(), key)

    def __iter__(self):
        return dict.__iter__(self._fill())

    def __len__(self):
        return dict.__len__(self._fill())

    def get(self, key, default=None):
        return dict.get(self._fill(), key, default)

    def keys(self):
        return dict.keys(self._fill())

    def values(self):
        return dict.values(self._fill())

    def items(self):
        return dict.items(self._fill())

    def __repr__(self):
        return dict.__repr__(self._fill())


name_to_model = _Models()


def get_data_loaders(labels, cfg, rank: int = 0, world: int = 1, wildcard=None):
    """train.py:21-26.  With more than one rank each loader walks its own shard of the manifest: a DistributedSampler
    over the raw items (indices rank, rank + world, ...; the tail padded so every rank takes the same number of steps --
    a rank that ran out of batches early would leave the others waiting in a collective), which is what Lightning's DDP
    injects into the reference's loaders.  ``data.bucket_rungs`` > 0: length-bucketed batches instead (data/bucketing.py) -- each
    loader gets a ladder chosen from its own manifest and a BucketBatchSampler sharded by rank, which takes the
    DistributedSampler's place (it too gives every rank the same number of steps); validation is bucketed unshuffled."""
    from torch.utils.data.distributed import DistributedSampler
    from .data.data_loader import BatchAudioDataLoader, SpectrogramDataset
    from .data.augment_wave import from_config
    from .data.resample import parse_speed_factors
    loaders = []
    resample = _truth(cfg.get('resample', False))
    factors = parse_speed_factors(cfg.get('speed_perturb'))         # the train loader only: validation is never perturbed
    wave = from_config(cfg, int(cfg.audio_conf['sample_rate']))     # None unless data.noise_manifest / data.rir_manifest is set
    ends = _truth(cfg.get('wildcard_ends', False))                  # one wildcard around every target, validation included
    if ends and wildcard is None:
        raise ValueError('data.wildcard_ends=true needs model.wildcard (the mark character, e.g. model.wildcard="*")')
    bucket = bucket_options(cfg)
    for train, (manifest, perturb, augment) in ((True, (cfg.train_manifest, factors, wave)), (False, (cfg.val_manifest, None, None))):
        ds = SpectrogramDataset(manifest, cfg.audio_conf, labels, mel_spec=cfg.mel_spec, resample=resample, speed_perturb=perturb,
                                wave_augment=augment, wildcard=wildcard, wildcard_ends=ends)
        if bucket['rungs']:
            from .data.bucketing import BucketBatchSampler, choose_ladder, nominal_frames
            frames, align = nominal_frames(ds), bucket['align']
            # a slowed-down utterance is longer than its manifest row says: the top rung covers the slowest factor
            ladder = choose_ladder(frames, bucket['rungs'], align, headroom=max(1.0, 1.0 / min(perturb)) if perturb else 1.0)
            sampler = BucketBatchSampler(frames, cfg.batch_size, ladder, shuffle=train and bucket['shuffle'], seed=bucket['seed'],
                                         drop_last=train and bucket['drop_last'], num_replicas=world, rank=rank)
            loaders.append(BatchAudioDataLoader(ds, batch_sampler=sampler, ladder=ladder, align=align))
            continue
        kw = {}
        if world > 1:
            kw['sampler'] = DistributedSampler(range(len(ds)), num_replicas=world, rank=rank, shuffle=False)
        loaders.append(BatchAudioDataLoader(ds, batch_size=cfg.batch_size, **kw))
    return loaders[0], loaders[1]


def _truth(v) -> bool:
    return v is True or (isinstance(v, str) and v.lower() in ('1', 'true', 'yes'))


def build_config(argv):
    config_dir = None
    rest = []
    it = iter(argv)
    for a in it:
        if a == '--config-dir':
            config_dir = next(it)
        elif a.startswith('--config-dir='):
            config_dir = a.split('=', 1)[1]
        else:
            rest.append(a)
    overrides = [a for a in rest if '=' in a]
    if config_dir is not None:
        cfg = load_config(config_dir, overrides)
        _check_augment(cfg)
        return cfg
    from .defaults import root_config
    group = 'wav2letter'
    plain = []
    for ov in overrides:
        k, v = ov.split('=', 1)
        if k == 'model':
            group = v
        else:
            plain.append((k, v))
    cfg = root_config(group)
    for k, v in plain:
        cur = cfg
        parts = k.split('.')
        for p in parts[:-1]:
            cur = cur.setdefault(p, to_cfg({}))
        cur[parts[-1]] = to_cfg(override_value(k, v))
    criterion_name(cfg.model)      # model.criterion: ctc | asg (absent: ctc), anything else is an error naming the two
    wildcard_options(cfg.model)    # model.wildcard: one character, none of the labels, not with asg
    scheduler_interval(cfg.model)  # model.scheduler_interval: epoch | step (absent: epoch)
    _check_augment(cfg)
    return cfg


def _check_augment(cfg):
    """data.snr_db is a range lo,hi with lo <= hi, data.noise_prob / data.rir_prob are probabilities: ValueError otherwise"""
    from .data.augment_wave import check_config
    if cfg.get('data') is not None:
        check_config(cfg.data)
        bucket_options(cfg.data)


def _requested_gpus(cfg) -> int:
    """trainer.gpus of the reference's config tree (configuration/config.yaml: passed to pytorch_lightning.Trainer):
    an int is a device count, a list names devices"""
    g = cfg.trainer.get('gpus', 0)
    if isinstance(g, (list, tuple)):
        return len(g)
    try:
        return int(g or 0)
    except (TypeError, ValueError):
        return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    cfg = build_config(argv)
    for key in ('train_manifest', 'val_manifest'):
        if cfg.data.get(key) in (None, '???'):
            raise SystemExit(f'data.{key} is required (e.g. data.{key}=/path/to/manifest.csv)')
    n_gpus = _requested_gpus(cfg)
    if criterion_name(cfg.model) == 'asg' and (n_gpus > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1):
        # distributed.GradReducer averages the gradients the step engine hands it, i.e. the engine's own weights;
        # criterion.transitions is not among them
        raise NotImplementedError('model.criterion=asg is not supported with data parallelism (trainer.gpus > 1 or a launcher '
                                  'with WORLD_SIZE > 1): the gradient reducer does not cover criterion.transitions')
    if n_gpus > 1 and not under_launcher():
        # Trainer(gpus=N) of the reference = N DDP processes.  This parent has not touched the GPU: it only starts the ranks.
        rc = spawn_ranks(n_gpus, [sys.executable, '-m', 'wav2letter_pytorch_amd.train'] + argv)
        if rc:
            raise SystemExit(rc)
        return None, None
    import torch
    from .data import label_sets
    from .trainer import Trainer
    if type(cfg.model.labels) is str:
        cfg.model.labels = list(label_sets.labels_map[cfg.model.labels])
    if isinstance(cfg.model.get('decoder'), dict):
        cfg.model.decoder.labels = cfg.model.labels
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = 0 if os.environ.get('W2L_DIST_BACKEND') == 'gloo' else int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    wildcard, _penalty = wildcard_options(cfg.model, cfg.model.labels)
    train_loader, val_loader = get_data_loaders(cfg.model.labels, cfg.data, rank, world, wildcard=wildcard)
    model = name_to_model[cfg.model.name](cfg.model)
    if world > 1:
        from .distributed import GradReducer, broadcast_parameters, init_process_group_from_env
        init_process_group_from_env()
        model = model.cuda()
        broadcast_parameters(model)
        model.grad_reducer = GradReducer()
    trainer = Trainer(**{k: v for k, v in cfg.trainer.items()})
    trainer.fit(model, train_loader, val_loader)
    return trainer, model


if __name__ == '__main__':
    main()

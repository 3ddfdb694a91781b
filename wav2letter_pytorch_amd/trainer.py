"""Minimal fit loop standing in for ``pytorch_lightning.Trainer(**cfg.trainer).fit(model, train, val)``
(reference train.py:34-37) when Lightning is not installed: epochs / max_steps, optimizer + scheduler from
``configure_optimizers`` (base_asr_models.py:73-76; a plain scheduler steps once per epoch, Lightning's dict form
``{'scheduler': s, 'interval': 'step' | 'epoch', 'frequency': k}`` after every k-th optimizer step / epoch), ``training_step`` /
``validation_step`` with their ``log_dict`` metrics, one checkpoint per epoch under ``default_root_dir``.

Data parallel (one process per GPU, launch.py / torchrun): every rank runs this loop on its own shard of the
manifest (train.py attaches a DistributedSampler, as Lightning's DDP does, or a rank-sharded BucketBatchSampler with
``data.bucket_rungs``; ``set_epoch`` is called on either), gradients are averaged by the
``distributed.GradReducer`` attached to the model; only rank 0 prints and writes checkpoints.

Checkpoints carry Lightning's keys: ``state_dict`` (reference parameter names), ``epoch``, ``global_step``,
``optimizer_states`` and ``lr_schedulers`` (lists, one entry per optimizer / scheduler), so an interrupted run
resumes with its momentum buffers and learning rate: ``Trainer(resume_from_checkpoint=path)`` or
``fit(..., ckpt_path=path)``."""
from __future__ import annotations

import os
import time
from typing import Optional

import torch
import torch.distributed as dist


def scheduler_plan(schedulers) -> list:
    """the second return value of ``configure_optimizers`` as a list of (scheduler, interval, frequency): a plain scheduler
    is ('epoch', 1); Lightning's dict form names its own (``interval`` 'step' or 'epoch', ``frequency`` a positive int)"""
    if schedulers is None:
        return []
    if not isinstance(schedulers, (list, tuple)):
        schedulers = [schedulers]
    plan = []
    for s in schedulers:
        if isinstance(s, dict):
            if 'scheduler' not in s:
                raise ValueError(f"a scheduler dict needs the key 'scheduler', got {sorted(s)}")
            interval, every = s.get('interval', 'epoch'), s.get('frequency', 1)
            if interval not in ('step', 'epoch'):
                raise ValueError(f"scheduler interval {interval!r} is not supported: use 'step' or 'epoch'")
            if isinstance(every, bool) or not isinstance(every, int) or every < 1:
                raise ValueError(f'scheduler frequency must be a positive integer, got {every!r}')
            plan.append((s['scheduler'], interval, every))
        else:
            plan.append((s, 'epoch', 1))
    return plan


class _EpochMean:
    """Batch-size-weighted mean of the logged scalars of one validation epoch (Lightning's on_epoch reduction)."""

    def __init__(self):
        self.sums, self.weight = {}, {}

    def add(self, logs: dict, n: int):
        for k, v in logs.items():
            self.sums[k] = self.sums.get(k, 0.0) + float(v) * n
            self.weight[k] = self.weight.get(k, 0) + n

    def result(self) -> dict:
        return {k: self.sums[k] / self.weight[k] for k in self.sums if self.weight[k]}


class Trainer:
    def __init__(self, default_root_dir: str = '.', max_epochs: int = 5, max_steps: Optional[int] = None, gpus=0,
                 log_every_n_steps: int = 50, enable_checkpointing: bool = True, resume_from_checkpoint: Optional[str] = None,
                 gradient_clip_val=None, gradient_clip_algorithm: Optional[str] = 'norm', **unused):
        self.default_root_dir = default_root_dir
        self.max_epochs = max_epochs
        self.max_steps = max_steps
        self.log_every_n_steps = log_every_n_steps
        self.enable_checkpointing = enable_checkpointing
        self.resume_from_checkpoint = resume_from_checkpoint
        # Lightning's gradient clipping: model.configure_gradient_clipping between loss.backward() and opt.step()
        if gradient_clip_val is not None and (isinstance(gradient_clip_val, bool) or float(gradient_clip_val) < 0):
            raise ValueError(f'gradient_clip_val must be a non-negative number or None, got {gradient_clip_val!r}')
        algorithm = getattr(gradient_clip_algorithm, 'value', gradient_clip_algorithm) or 'norm'
        if algorithm not in ('norm', 'value'):
            raise ValueError(f'gradient_clip_algorithm {gradient_clip_algorithm!r} is not supported: use "norm" or "value"')
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val else None
        self.gradient_clip_algorithm = algorithm
        self.global_step = 0
        self.current_epoch = 0
        self.logged = []
        self.val_logged = []                 # one dict of epoch-mean validation metrics per epoch
        self.bucket_logged = []              # one dict per epoch of a length-bucketed train loader (its ``ladder`` is set)

    @property
    def global_rank(self) -> int:
        return dist.get_rank() if dist.is_initialized() else 0

    @property
    def is_global_zero(self) -> bool:
        return self.global_rank == 0

    def _say(self, msg: str):
        if self.is_global_zero:
            print(msg, flush=True)

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path: str, model, optimizers, schedulers, epoch: int):
        state = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
        torch.save({'state_dict': state, 'epoch': epoch, 'global_step': self.global_step,
                    'optimizer_states': [o.state_dict() for o in optimizers],      # FusedSGD.state_dict joins its stream
                    'lr_schedulers': [s.state_dict() for s in schedulers]}, path)

    def _restore(self, path: str, model, optimizers, schedulers) -> int:
        ck = torch.load(path, map_location='cpu')
        model.load_state_dict(ck['state_dict'])
        from .engine import invalidate_packed
        invalidate_packed(model)
        for o, st in zip(optimizers, ck.get('optimizer_states', [])):
            o.load_state_dict(st)
        for s, st in zip(schedulers, ck.get('lr_schedulers', [])):
            s.load_state_dict(st)
        self.global_step = int(ck.get('global_step', 0))
        return int(ck.get('epoch', -1)) + 1          # the checkpoint is written at the END of its epoch

    def test(self, model, dataloader, ckpt_path: Optional[str] = None):
        """``Trainer.test`` of Lightning: load ``ckpt_path`` (its ``state_dict``), run ``model.infer`` over the loader and
        return (and print) ``test_loss`` (batch-size-weighted epoch mean, as validation forms it), corpus-level ``test_cer`` /
        ``test_wer`` (errors summed over the set / reference lengths summed over the set) and ``test_len_ratio``."""
        if not torch.cuda.is_available():
            raise RuntimeError('wav2letter_pytorch_amd runs on MI355X only (no CPU path)')
        from .evaluate import evaluate
        model = model.cuda()
        if ckpt_path:
            ck = torch.load(ckpt_path, map_location='cpu')
            model.load_state_dict(ck['state_dict'])
            from .engine import invalidate_packed
            invalidate_packed(model)
        metrics, records = evaluate(model, dataloader)
        self.test_records = records
        if hasattr(model, '_logged'):
            model._logged.update(metrics)
        self._say('test ' + ' '.join(f'{k}={v:.4g}' for k, v in metrics.items()))
        return metrics

    def _clip(self, model, opt):
        hook = getattr(model, 'configure_gradient_clipping', None)
        if hook is not None:
            hook(opt, gradient_clip_val=self.gradient_clip_val, gradient_clip_algorithm=self.gradient_clip_algorithm)
        else:
            from .optim import clip_gradients
            clip_gradients(opt, self.gradient_clip_val, self.gradient_clip_algorithm, model=model)

    # ------------------------------------------------------------------ loop
    def fit(self, model, train_dataloader, val_dataloader=None, ckpt_path: Optional[str] = None):
        if not torch.cuda.is_available():
            raise RuntimeError('wav2letter_pytorch_amd trains on MI355X only (no CPU path); trainer.gpus is implied')
        model = model.cuda()
        optimizers, schedulers = model.configure_optimizers()
        plan = scheduler_plan(schedulers)
        schedulers = [sch for sch, _, _ in plan]          # (what checkpoints save and restore: the inner schedulers)
        per_step = [(sch, every) for sch, interval, every in plan if interval == 'step']
        per_epoch = [(sch, every) for sch, interval, every in plan if interval == 'epoch']
        opt = optimizers[0]
        model._optimizers = opt
        join = getattr(opt, 'join', lambda: None)
        first_epoch = 0
        ckpt_path = ckpt_path or self.resume_from_checkpoint
        if ckpt_path:
            first_epoch = self._restore(ckpt_path, model, optimizers, schedulers)
            self._say(f'resumed from {ckpt_path}: epoch {first_epoch}, step {self.global_step}')
        if hasattr(opt, 'overlap'):          # optim.FusedSGD: weight updates stream under the next forward pass
            opt.overlap = True
            # ... and the top units' weight gradients run beside it (W2L_DEFER_WGRAD=k, 0 = off; default: 4 of a deep stack).
            # While a gradient is held back ``p.grad`` of that weight is None at step() ("Deferred weight
            # gradients"): set W2L_DEFER_WGRAD=0 for anything that reads gradients between backward() and step().
            # (after the restore: load_state_dict drops the step engine, which is what counts the units)
            # With gradient clipping on, the default is 0: the clip call computes every held-back gradient at once anyway.
            n_units = len(model.engine().units) if hasattr(model, 'engine') else 0
            k = int(os.environ.get('W2L_DEFER_WGRAD', 0 if self.gradient_clip_val else min(4, n_units // 4)))
            if k and hasattr(opt, 'defer_wgrad'):
                opt.defer_wgrad(model, k)
                if self.gradient_clip_val:
                    self._say(f'W2L_DEFER_WGRAD={k} with gradient clipping: every held-back weight gradient is computed at the '
                              'clip call (correct, but deferral buys nothing; W2L_DEFER_WGRAD=0 is the default while clipping)')
        from . import engine as _E, replay as _replay
        self._say('wav2letter_pytorch_amd: '
                  + ('bit-reproducible step (W2L_DETERMINISTIC=1)' if _E.DETERMINISTIC_WGRAD else
                     'default step: fp32 atomics in split reductions, not bit-reproducible from run to run (W2L_DETERMINISTIC=1: +0.6 %)')
                  + ('; warm step shapes are replayed from recorded launch lists (W2L_REPLAY=0: eager)' if _replay.ENABLED else
                     '; eager step (W2L_REPLAY=0)')
                  + ('; string metrics scored behind backward()' if getattr(model, 'async_metrics', False) else '')
                  + (f'; gradient clipping: {self.gradient_clip_algorithm} {self.gradient_clip_val:g}' if self.gradient_clip_val else ''))
        ladder = getattr(train_dataloader, 'ladder', None)          # length-bucketed batches (data/bucketing.py)
        if ladder is not None and _replay.ENABLED and len(ladder) + 1 > _replay.MAX_GROUPS:
            self._say(f'{len(ladder)} rungs and the short last batch are {len(ladder) + 1} step shapes, above the '
                      f'{_replay.MAX_GROUPS} kept recorded (W2L_REPLAY_MAX_SHAPES): the least recently used shape is re-recorded')
        done = self.max_steps is not None and self.global_step >= self.max_steps
        for epoch in range(first_epoch, self.max_epochs):
            if done:
                break
            self.current_epoch = epoch
            for sampler in (getattr(train_dataloader, 'sampler', None), getattr(train_dataloader, 'batch_sampler', None)):
                if hasattr(sampler, 'set_epoch'):
                    sampler.set_epoch(epoch)
            model.train()
            t0 = time.time()
            if ladder is not None:
                shapes, cells, valid, steps0 = set(), 0, 0, self.global_step
                stats0 = {k: v for k, v in _replay.STATS.items() if isinstance(v, int)}
            for i, batch in enumerate(train_dataloader):
                if ladder is not None:           # host values only: the shape and the (host) length vector
                    shapes.add(tuple(batch[0].shape))
                    cells += batch[0].shape[0] * batch[0].shape[-1]
                    valid += int(batch[1].sum())
                opt.zero_grad(set_to_none=True)
                loss = model.training_step(batch, i)
                loss.backward()
                if self.gradient_clip_val:           # Lightning's order: backward, clip, step
                    self._clip(model, opt)
                opt.step()
                # Lightning's hook order: the batch's string metrics (greedy decode, CER / WER) are scored HERE, with the
                # backward pass and the update already enqueued -- training_step itself never waits for the GPU
                model.on_train_batch_end(loss, batch, i)
                self.global_step += 1
                for sch, every in per_step:
                    if self.global_step % every == 0:
                        sch.step()
                if self.global_step % self.log_every_n_steps == 0 or self.global_step == 1:
                    if hasattr(model, 'resolve_metrics'):
                        model.resolve_metrics(wait_all=True)         # a logging point reports THIS step (one sync per log line)
                    logs = dict(getattr(model, '_logged', {}))
                    self.logged.append((self.global_step, logs))
                    self._say(f'epoch {epoch} step {self.global_step} ' + ' '.join(f'{k}={v:.4g}' for k, v in logs.items()))
                if self.max_steps is not None and self.global_step >= self.max_steps:
                    done = True
                    break
            model.on_train_epoch_end()
            if ladder is not None:
                rec = dict(epoch=epoch, steps=self.global_step - steps0, ladder=list(ladder), shapes=sorted(shapes),
                           padded_share=(cells - valid) / max(valid, 1), off_ladder=getattr(train_dataloader, 'off_ladder', 0),
                           tuned_shapes=len(_E._tuned_shapes), **{k: _replay.STATS[k] - v for k, v in stats0.items()})
                self.bucket_logged.append(rec)
                self._say(f'epoch {epoch} buckets: ladder {rec["ladder"]}, padding {100 * rec["padded_share"]:.1f} % of the valid '
                          f'frames, {len(shapes)} step shapes in {rec["steps"]} steps ({rec["off_ladder"]} batches off the ladder so '
                          'far); replay ' + ' '.join(f'{k}=+{rec[k]}' for k in stats0))
            for sch, every in per_epoch:
                if (epoch + 1) % every == 0:
                    sch.step()
            join()                               # parameters are read below (validation, checkpoint)
            if val_dataloader is not None:
                model.eval()
                mean = _EpochMean()
                with torch.no_grad():
                    for i, batch in enumerate(val_dataloader):
                        for k in [k for k in getattr(model, '_logged', {}) if k.startswith('val')]:
                            del model._logged[k]
                        model.validation_step(batch, i)
                        mean.add({k: v for k, v in getattr(model, '_logged', {}).items() if k.startswith('val')},
                                 len(batch[0]))
                logs = mean.result()
                if hasattr(model, '_logged'):
                    model._logged.update(logs)   # what a callback / the caller reads after the epoch: the epoch means
                self.val_logged.append(logs)
                self._say(f'epoch {epoch} validation ' + ' '.join(f'{k}={v:.4g}' for k, v in logs.items()))
            if self.enable_checkpointing and self.is_global_zero:
                os.makedirs(self.default_root_dir, exist_ok=True)
                path = os.path.join(self.default_root_dir, f'epoch={epoch}-step={self.global_step}.ckpt')
                self.save_checkpoint(path, model, optimizers, schedulers, epoch)
            eng = getattr(model, '_engine_cache', None)
            if eng is not None and getattr(eng[1], 'fp8', False):
                clipped = eng[1].fp8_saturated()          # one sync per epoch
                if clipped:
                    self._say(f'epoch {epoch}: {clipped} activation elements saturated the e4m3 range in fp8 mode (fixed '
                              'per-tensor activation scales, engine.FP8_ACT_SCALE): their forward operands were clipped')
            self._say(f'epoch {epoch} done in {time.time() - t0:.1f}s')
        join()
        return model

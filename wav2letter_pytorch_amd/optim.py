"""FusedSGD: torch.optim.SGD semantics (the reference's optimizer, configuration/optimizer/
exp_lr_optimizer.yaml:2-7) with the conv-weight update fused with the bf16 operand packing of the
next step (w2l_sgd_pack).  Non-conv parameters (biases, BatchNorm affine) use torch's own foreach
update.  State-dict layout is torch.optim.SGD's (``momentum_buffer`` per parameter).

The conv-weight updates are HBM-bound (24 B per parameter, 3.7 GB per step for the full Wav2Letter table) while the
forward convolutions that follow them are MFMA-bound, so ``step()`` enqueues them on a side HIP stream in forward order
and tags each weight's operand pack with an event; the step engine waits for a layer's event just before that layer's
first convolution (engine.pack_weights).  The next forward therefore starts as soon as layer 0 is updated, and the other
20 updates stream through HBM underneath it.  This is opt-in (``optimizer.overlap = True``; trainer.Trainer and bench.py
do): ``join()`` (also called by ``state_dict``) makes the caller's stream wait for the updates in flight, and anything
that reads the parameters outside the step engine must call it first.

``defer_wgrad(model, k)`` goes one step further: the weight gradients of the model's top ``k`` conv units are not computed
in backward at all but at the start of the NEXT forward pass, on the weight-gradient stream, each followed by this
optimizer's fused update of that weight (engine.StackEngine.flush_deferred).  The top layers are the first of the backward
pass and the last of the forward pass, so their gradients are the ones with slack; launched beside the forward they give
the matrix cores work while the forward's own BatchNorm / CTC kernels run.  One optimizer step per batch, as before: a
layer's forward convolution waits for the event behind its update.  ``p.grad`` of those weights stays ``None`` (the update
consumes the gradient directly); ``join()`` flushes whatever is pending.

``clip_grad_norm_(max_norm)`` / ``clip_grad_value_(v)`` between backward() and step(): torch.nn.utils.clip_grad_norm_ /
clip_grad_value_ with the coefficient computed on the device (w2l_grad_sqnorm_multi: every gradient read once, in one launch)
and applied by the NEXT step()'s update kernels as they read each gradient (w2l_sgd_pack_clip, w2l_sgd_small_multi_clip): no
host read, no pass that rewrites the gradients -- ``p.grad`` keeps the unclipped values.  Held-back weight gradients are
computed at the clip call (they belong in the norm).  Anything the fused path does not cover takes torch's own functions
(``clip_gradients``).

FusedAdamW: torch.optim.Adam / AdamW on the same machinery (FusedBase holds what does not depend on the update rule).  Its
step-dependent scalars -- the learning rate and the two bias corrections -- live in device memory (w2l_adam_tick), so a
recorded optimizer phase survives a per-step learning-rate schedule."""
from __future__ import annotations

import math
import os
import weakref

import torch

from . import _lib
from . import engine as E
from ._lib import check, lib, ptr, stream_ptr


def _dense(t: torch.Tensor) -> bool:
    """do the elements of ``t`` fill a dense block of memory (in any dimension order)?"""
    if t.is_contiguous():
        return True
    expect = 1
    for st, n in sorted((st, n) for st, n in zip(t.stride(), t.shape) if n > 1):
        if st != expect:
            return False
        expect *= n
    return True


def materialize_held_back(engines, opt=None):
    """compute now, on the current stream, the weight gradients that a backward pass held back (FusedSGD.defer_wgrad) and
    that no step() has consumed yet, into ``p.grad`` -- and drop their records, so that nothing applies them a second time"""
    for eng in engines:
        dopt = eng.deferred if opt is None else opt
        recs = [r for r in eng._deferred if not (dopt is not None and dopt.stepped(r.token))]
        if recs:
            eng._deferred = [r for r in eng._deferred if not any(r is q for q in recs)]
            eng._materialize(recs)


def clip_gradients(optimizer, clip_val, algorithm='norm', model=None, norm_type=2.0):
    """Lightning's gradient clipping (Trainer(gradient_clip_val=, gradient_clip_algorithm=)) for any optimizer: FusedSGD takes
    its fused path (clip_grad_norm_ / clip_grad_value_), every other optimizer torch.nn.utils.clip_grad_norm_ /
    clip_grad_value_ over its parameters' gradients, after the held-back weight gradients of ``model``'s step engine (if any)
    have been computed.  Returns the total norm (norm mode) or None."""
    opt = getattr(optimizer, '_optimizer', optimizer)           # (a Lightning optimizer wrapper)
    algorithm = getattr(algorithm, 'value', algorithm)           # (Lightning's GradClipAlgorithmType)
    if algorithm not in ('norm', 'value'):
        raise ValueError(f'gradient_clip_algorithm {algorithm!r} is not supported: use "norm" or "value"')
    if isinstance(opt, FusedBase):
        return opt.clip_grad_norm_(clip_val, norm_type) if algorithm == 'norm' else opt.clip_grad_value_(clip_val)
    hit = model.__dict__.get('_engine_cache') if model is not None else None
    if hit is not None:
        materialize_held_back([hit[1]])
    return _torch_clip([p for g in opt.param_groups for p in g['params'] if p.grad is not None], clip_val, algorithm, norm_type)


def _torch_clip(params, clip_val, algorithm, norm_type=2.0):
    if algorithm == 'norm':
        return torch.nn.utils.clip_grad_norm_(params, clip_val, norm_type=norm_type)
    torch.nn.utils.clip_grad_value_(params, clip_val)
    return None


def _is_tap_major(t: torch.Tensor) -> bool:
    """logical [Cout, Cin, Kw] view of a dense [Kw, Cout, Cin] storage"""
    if t.dim() != 3:
        return False
    co, ci, kw = t.shape
    return t.stride() == (ci, 1, co * ci)


def _conv_ok(p, g=None) -> bool:
    """a conv weight the fused update + operand pack takes (with its gradient ``g``, where there is one yet)"""
    return bool(p.is_cuda and p.dtype == torch.float32 and _is_tap_major(p) and (g is None or g.stride() == p.stride())
                and p.shape[0] % 64 == 0 and p.shape[1] % 64 == 0)


def _operands(p, recycle_grads=False, fp8=True):
    """the operand-pack buffers of the next step for conv weight ``p`` (kept from the last pack when they fit) ->
    (cache, precise, (fwd_hi, fwd_lo, dgr_hi, dgr_lo), recycle, f8); ``fp8`` False: an update that writes no e4m3 operands"""
    cout, cin, kw = p.shape
    dev = p.device
    cache = getattr(p, '_w2l_pack', None)
    if cache is None:
        cache = E._Volatile()
        p._w2l_pack = cache
    precise = any(k for k in cache)                              # keep hi/lo pairs alive only if fp32 mode is in use
    old = cache.get(precise)
    if old is not None and old.fwd_hi.device == dev and old.coutp == cout and old.cinp == cin:
        fwd_hi, fwd_lo, dgr_hi, dgr_lo = old.fwd_hi, old.fwd_lo, old.dgr_hi, old.dgr_lo
    else:
        _lib.poison('operand pack buffers created')
        fwd_hi = torch.empty(kw, cout, cin, dtype=torch.bfloat16, device=dev)
        dgr_hi = torch.empty(kw, cin, cout, dtype=torch.bfloat16, device=dev)
        fwd_lo = torch.empty_like(fwd_hi) if precise else None
        dgr_lo = torch.empty_like(dgr_hi) if precise else None
    # the gradient buffer is handed back to the step engine zero-filled (engine._wgrad_now takes it as the next dW when
    # zero_grad(set_to_none=True) has dropped p.grad): no fill launch for the split-K weight gradients of the next step
    recycle = recycle_grads and not precise
    # fp8 mode (engine._fp8_weights left its state on the parameter): emit the e4m3 operands of the next step here too,
    # with the scale in force -- its periodic re-derivation from amax stays with the engine (asynchronous: a new scale
    # is adopted at a forward pass, which then requantises both layouts itself for that one step).  Left alone (``fp8``
    # False), the state keeps the version of the last quantisation and the engine requantises.
    f8 = p.__dict__.get('_w2l_fp8') if fp8 else None
    if f8 is not None and (precise or f8['q'].shape != fwd_hi.shape or f8['q'].device != dev):
        f8 = None
    return cache, precise, (fwd_hi, fwd_lo, dgr_hi, dgr_lo), recycle, f8


def _packed(p, g, cache, precise, bufs, recycle, f8):
    """after the update kernel of conv weight ``p`` has been enqueued: the operand pack it wrote is the current one"""
    cout, cin, kw = p.shape
    if recycle:
        p._w2l_dw_zeroed = g.permute(2, 0, 1)                    # the dense [Kw, Cout, Cin] storage of g
    torch.autograd.graph.increment_version(p)                    # p changed through its raw pointer
    cache.clear()
    pk = E._PackedW(p._version, *bufs, cin, cout, p.data_ptr())
    cache[precise] = pk
    if f8 is not None:                      # both e4m3 layouts are current for this version
        f8['version'] = f8['version_d'] = pk.version
        f8['age'] += 1
    return pk


class FusedBase:
    """What the fused optimizers share, whatever their update rule: the side stream and ``overlap``, held-back weight gradients
    (``defer_wgrad`` / ``apply`` / ``join`` / ``token`` / ``stepped``), gradient clipping on read, the operand-pack buffers of a
    conv weight and the cached device tables of the one-launch small-parameter updates.  A mix-in in front of the torch
    optimizer whose semantics the subclass keeps; the subclass provides ``_group_fused_ok(group)``, ``_fused_conv(p, g, *hp,
    clip=None)`` and ``_step_eager()``."""
    # W2L_RECYCLE_GRADS=1: zero the consumed conv-weight gradients in the update kernel and hand them back as the next dW
    # (no fill launches for split-K weight gradients).  Off by default: measured NEUTRAL on the full Wav2Letter table
    # (13.54 vs 13.50 ms per step) -- the fills already ran hidden on the weight-gradient stream.
    recycle_grads = os.environ.get('W2L_RECYCLE_GRADS', '0') == '1'
    overlap = False           # opt-in (trainer.Trainer and bench.py set it): whoever enables it must join() before
                              # reading parameters outside the step engine (checkpoints, .cpu() copies, ...)

    def _side_state(self):
        st = self.__dict__.get('_w2l_side')
        if st is None:
            st = {'stream': None, 'held': [], 'pending': False, 'packs': []}
            self.__dict__['_w2l_side'] = st
        return st

    # ------------------------------------------------------------------ deferred weight gradients
    def _deferred_state(self):
        st = self.__dict__.get('_w2l_deferred')
        if st is None:
            st = {'seq': 0, 'hp': {}, 'engines': []}
            self.__dict__['_w2l_deferred'] = st
        return st

    def defer_wgrad(self, model, units):
        """hold back the weight gradients of some of ``model``'s conv units until its next forward pass: an int k = the top k
        units, an iterable of unit indices (negative: counted from the top) = exactly those; 0 / empty switches it off"""
        self.join()
        units = int(units) if isinstance(units, int) else frozenset(int(u) for u in units)
        model._defer_wgrad = units
        model._deferred_opt = self if units else None

    def _register_engine(self, eng):
        # weak references: a model that rebuilds its engine (module.to(), load_state_dict of replaced tensors) must not keep
        # every dead engine -- its streams and held tensors -- alive through the optimizer
        st = self._deferred_state()
        st['engines'] = [r for r in st['engines'] if r() is not None]
        if not any(r() is eng for r in st['engines']):
            st['engines'].append(weakref.ref(eng))

    def _engines(self):
        return [e for e in (r() for r in self._deferred_state()['engines']) if e is not None]

    def zero_grad(self, set_to_none: bool = True):
        """torch's zero_grad, plus: weight gradients held back by a backward pass that no step() followed are dropped with
        the rest (a skipped step -- non-finite loss guard, manual skip -- must not leak into the next one), and so is an armed
        gradient clip"""
        for eng in self._engines():
            eng.drop_unstepped()
        self.__dict__.pop('_w2l_clip_arm', None)          # (so is a clip call whose step was skipped)
        return super().zero_grad(set_to_none=set_to_none)

    def accepts(self, p) -> bool:
        """would step() take this parameter through the fused conv-weight update?"""
        hp = self._deferred_state()['hp'].get(id(p))
        if hp is None:
            for group in self.param_groups:
                ok = self._group_fused_ok(group)
                for q in group['params']:
                    self._deferred_state()['hp'][id(q)] = [ok, group, None]
            hp = self._deferred_state()['hp'].get(id(p))
        return bool(hp is not None and hp[0] and self.overlap and _conv_ok(p))

    def token(self) -> int:
        return self._deferred_state()['seq']

    def stepped(self, token: int) -> bool:
        """has step() run since ``token`` was drawn (i.e. since the backward pass that deferred a gradient)?"""
        return self._deferred_state()['seq'] > token

    @torch.no_grad()
    def apply(self, p, g):
        """the fused update of ONE conv weight with gradient ``g``, on the current stream (the stream that produced ``g``),
        with the hyper-parameters of the last step() call"""
        ok, group, hp = self._deferred_state()['hp'][id(p)]
        pk = self._fused_conv(p, g, *hp)
        pk.ready = E.weight_event(p)
        pk.ready.record()

    def join(self):
        """make the current stream wait for every update of the last step: deferred weight gradients are launched and
        applied first, then the weight-gradient stream and the optimizer's side stream are joined"""
        for eng in self._engines():
            eng.flush_deferred()
            eng.join_side()
        self._join_updates()

    def _join_updates(self):
        """make the current stream wait for the updates still running on the optimizer's side stream"""
        st = self._side_state()
        if st['pending'] and st['stream'] is not None:
            _lib.stream_wait_stream(_lib.raw_stream(), st['stream'])
        st['pending'] = False
        st['held'], st['packs'] = [], []
        if self._release_held in E.AFTER_FORWARD:
            E.AFTER_FORWARD.remove(self._release_held)

    def _release_held(self):
        """engine hook, end of a forward pass: once that forward has waited for every update event of the last step() the
        gradients those updates read (0.6 GB for the full Wav2Letter table) can go back to the allocator"""
        st = self._side_state()
        if all(pk.ready is None for pk in st['packs']):
            st['held'], st['packs'] = [], []
            if self._release_held in E.AFTER_FORWARD:
                E.AFTER_FORWARD.remove(self._release_held)

    def state_dict(self):
        self.join()
        return super().state_dict()

    # ------------------------------------------------------------------ gradient clipping
    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, norm_type=2.0):
        """torch.nn.utils.clip_grad_norm_ over this optimizer's gradients, between backward() and step(): returns the total
        norm (a 0-dim device tensor, no host sync) and arms the NEXT step() to apply min(1, max_norm / (norm + 1e-6)) as its
        update kernels read the gradients (``p.grad`` itself is left unclipped).  Held-back weight gradients are computed now.
        Norm types other than 2 and inf, and gradients the fused path does not take, go through torch's function."""
        norm_type = float(norm_type)
        grads = self._clip_prepare()
        if grads is None or norm_type not in (2.0, float('inf')):
            return _torch_clip(self._grad_params(), max_norm, 'norm', norm_type)
        st = self._clip_state(grads[0].device)
        table, nitems, nchunks = self._norm_table(st, grads)
        out = torch.empty((), dtype=torch.float32, device=grads[0].device)
        check(lib.w2l_grad_sqnorm_multi(ptr(table), nitems, nchunks, int(norm_type != 2.0), ptr(st['partials']), float(max_norm),
                                        ptr(st['buf']), ptr(out), stream_ptr()), 'w2l_grad_sqnorm_multi')
        self.__dict__['_w2l_clip_arm'] = 'norm'
        return out

    @torch.no_grad()
    def clip_grad_value_(self, clip_value):
        """torch.nn.utils.clip_grad_value_ on read: arms the NEXT step() to clamp every gradient to [-clip_value, clip_value]
        as its update kernels read it (``p.grad`` is left as it is)"""
        grads = self._clip_prepare()
        if grads is None:
            return _torch_clip(self._grad_params(), clip_value, 'value')
        st = self._clip_state(grads[0].device)
        check(lib.w2l_grad_clip_value(ptr(st['buf']), float(clip_value), stream_ptr()), 'w2l_grad_clip_value')
        self.__dict__['_w2l_clip_arm'] = 'value'
        return None

    def _grad_params(self):
        return [p for g in self.param_groups for p in g['params'] if p.grad is not None]

    def _clip_prepare(self):
        """the gradients of the next step, complete: held-back weight gradients computed, the updates of the last step that
        still read the clip buffer done.  -> their list, or None if the fused path cannot take them"""
        self.__dict__.pop('_w2l_clip_arm', None)
        materialize_held_back(self._engines(), self)
        side = self._side_state()
        if side['pending'] and side['stream'] is not None:
            _lib.stream_wait_stream(_lib.raw_stream(), side['stream'])
        grads = [p.grad for p in self._grad_params()]
        if (not grads or torch.cuda.is_current_stream_capturing()
                or not all(g.is_cuda and g.dtype == torch.float32 and g.device == grads[0].device and not g.is_sparse and _dense(g)
                           for g in grads)):
            return None
        return grads

    def _clip_state(self, dev):
        st = self.__dict__.get('_w2l_clip')
        if st is None or st['buf'].device != dev:
            st = self.__dict__['_w2l_clip'] = {
                'buf': torch.tensor([0.0, 1.0, float('inf'), 0.0], dtype=torch.float32, device=dev),
                'partials': torch.empty(_lib.GNORM_BLOCKS, dtype=torch.float64, device=dev), 'tables': {}}
        return st

    def _norm_table(self, st, grads):
        """the device table of w2l_grad_sqnorm_multi (g, n, first chunk), built once per set of gradient addresses (a
        replayed step's static gradient buffers: one table per record set)"""
        rows = tuple((g.data_ptr(), g.numel()) for g in grads if g.numel() > 0)
        hit = st['tables'].get(rows)
        if hit is None:
            if len(st['tables']) > 8:
                st['tables'].clear()
            flat, c0 = [], 0
            for gp, n in rows:
                flat += [gp, n, c0]
                c0 += -(-n // _lib.GNORM_CHUNK)
            table = torch.tensor(flat, dtype=torch.int64).to(grads[0].device) if rows else None
            hit = st['tables'][rows] = (table, len(rows), c0)
        return hit

    def _clip_signature(self):
        """what a recorded optimizer phase depends on besides the hyper-parameters: armed or not, in which mode, and which
        buffer it reads (max_norm / clip_value only reach the buffer: changing them needs no new record)"""
        mode = self.__dict__.get('_w2l_clip_arm')
        return None if mode is None else (mode, self.__dict__['_w2l_clip']['buf'].data_ptr())

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # the gradients of a recorded / replayed backward pass: the step is replayed as ONE w2l_replay call, or recorded now
        from . import replay
        try:
            if not self._before_step():
                replay._last_backward[0] = None                # (this step has work no recorded phase covers)
            if replay._last_backward[0] is not None and replay.optimizer_step(self, self._step_eager):
                return loss
            self._step_eager()
        finally:
            self.__dict__.pop('_w2l_clip_arm', None)          # clipping is armed for one step
        return loss

    def _before_step(self) -> bool:
        """what a step does on the host whether it then runs eagerly, is recorded or is replayed -> may it be replayed?"""
        return True

    # ------------------------------------------------------------------ the eager step, shared parts
    def _begin_eager(self):
        """the top of every eager step: order it after the last one, settle doubly-held gradients, count it -> the armed clip
        buffer or None"""
        clip = self.__dict__['_w2l_clip']['buf'] if self.__dict__.get('_w2l_clip_arm') else None
        rp_hit = None
        for eng in self._engines():
            rp_hit = eng.__dict__.get('_replayer') or rp_hit
        if rp_hit is not None:
            rp_hit.before_eager()
        self._join_updates()         # (normally a no-op: the forward pass has already waited for every event)
        for eng in self._engines():  # a weight with BOTH a held-back gradient and a .grad gets one update with their sum
            eng.settle_before_step()
        self._deferred_state()['seq'] += 1       # gradients deferred by the backward pass just run now count as "stepped"
        return clip

    def _set_hp(self, group, hp):
        """what a deferred update of this step is applied with (``apply``): the arguments of _fused_conv behind (p, g)"""
        table = self._deferred_state()['hp']
        for p in group['params']:
            ent = table.get(id(p))
            if ent is not None:
                ent[2] = hp

    def _run_fused(self, fused, hp, clip):
        """the fused conv-weight updates of one group: on the caller's stream, or (``overlap``) on the side stream in forward
        order, each tagging its operand pack with the weight's event"""
        if not fused:
            return
        if not self.overlap:
            for p, g in fused:
                self._fused_conv(p, g, *hp, clip=clip)
            return
        st = self._side_state()
        dev = fused[0][0].device
        if st['stream'] is None or st['stream'].device != dev:
            from .streams import concurrent_stream        # measured to run beside the main and weight-gradient streams
            _lib.poison('optimizer side stream created')
            st['stream'] = concurrent_stream(dev, 'sgd')
        side = st['stream']
        _lib.stream_wait_stream(side, _lib.raw_stream())     # gradients (wgrad join, all-reduce) are complete there
        with torch.cuda.stream(side):
            for p, g in fused:               # parameter order = forward order: layer 0's event fires first
                pk = self._fused_conv(p, g, *hp, clip=clip)
                pk.ready = E.weight_event(p)
                pk.ready.record(side)
                st['held'].append(g)         # zero_grad() must not hand this memory back while the kernel reads it
                st['packs'].append(pk)
        st['pending'] = True
        if self._release_held not in E.AFTER_FORWARD:
            E.AFTER_FORWARD.append(self._release_held)

    def _same_layout_buffer(self, p, state, key, what):
        """the state buffer ``key`` of ``p`` in the parameter's own strides (the kernels walk p, g and the state with one offset)"""
        buf = state.get(key)
        if buf is None:
            _lib.poison(what + ' created')
            buf = state[key] = torch.zeros_like(p)                   # preserves the tap-major strides
        elif buf.stride() != p.stride():
            _lib.poison(what + ' re-laid out')
            buf = state[key] = torch.empty_like(p).copy_(buf)
        return buf

    def _small_table(self, rows, device):
        """the device table of a one-launch small-parameter update (``rows``: tuples of addresses, the element count last),
        built once per set of addresses"""
        cache = self.__dict__.setdefault('_w2l_small_tables', {})
        table = cache.get(rows)
        if table is None:
            # (built while the optimizer phase of a step is being recorded, the table lives in that phase's own memory pool:
            # a live allocation nothing else of the record ever writes -- no reason to drop the recording)
            if len(cache) > 8:
                cache.clear()
            # (w2l_sgd_small_t / w2l_adam_small_t: the pointers, then {int32 n, int32 pad} = one int64 < 2^31)
            table = cache[rows] = torch.tensor([x for row in rows for x in row], dtype=torch.int64).to(device)
        rec = _lib.recording()
        if rec is not None:
            rec.keep.append(table)          # the recorded phase O owns its table: evicting it from the cache must not free it
        return table

    def _launch_small(self, entry, params, rows, *args):
        """ONE launch of entry point ``entry`` updating all of ``params`` (conv biases, BatchNorm gamma / beta, the
        classifier) instead of torch._foreach_* calls over ~60 tensors; an entry point, so a recorded launch list replays it"""
        table = self._small_table(tuple(rows), params[0].device)
        check(getattr(lib, entry)(ptr(table), len(rows), max(r[-1] for r in rows), *args, stream_ptr()), entry)
        for p in params:
            torch.autograd.graph.increment_version(p)

    def _load_in_place(self, state_dict, keys) -> bool:
        """torch's load_state_dict, except that a loaded state buffer (``keys``) is copied INTO the buffer it replaces when
        their layouts agree: recorded optimizer phases (replay.py, phases O and X) name the buffers by address.  -> did a
        buffer go or change layout (those phases are stale then)?"""
        self.join()
        old = {id(p): [self.state[p].get(k) for k in keys] for g in self.param_groups for p in g['params'] if p in self.state}
        super().load_state_dict(state_dict)
        stale = False
        for g in self.param_groups:
            for p in g['params']:
                for k, buf in zip(keys, old.get(id(p), ())):
                    new = self.state[p].get(k) if p in self.state else None
                    if buf is None or new is buf:
                        continue
                    if (new is not None and new.shape == buf.shape and new.stride() == buf.stride() and new.dtype == buf.dtype
                            and new.device == buf.device):
                        buf.copy_(new)
                        self.state[p][k] = buf
                    else:
                        stale = True
        return stale

    @staticmethod
    def _same_layout(a, b) -> bool:          # (the stride of a size-1 dimension means nothing)
        return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)

    def _elementwise_ok(self, p, buffers) -> bool:
        """may this parameter take the one-launch elementwise update?  fp32 on the device, dense, and gradient / state
        buffers in the parameter's own physical layout (contiguous, or -- a depthwise conv weight -- the tap-major permutation)"""
        g = p.grad
        if (not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or g.device != p.device
                or not self._same_layout(g, p)):
            return False
        if not (p.is_contiguous() or (p.dim() == 3 and p.permute(2, 0, 1).is_contiguous())):
            return False
        return all(b is not None and self._same_layout(b, p) and b.dtype == torch.float32 and b.device == p.device for b in buffers)


class FusedSGD(FusedBase, torch.optim.SGD):
    @classmethod
    def from_sgd(cls, opt: torch.optim.SGD) -> 'FusedSGD':
        new = cls.__new__(cls)
        new.__dict__.update(opt.__dict__)
        return new

    def _group_fused_ok(self, group) -> bool:
        return group['momentum'] != 0 and group['dampening'] == 0 and not group.get('maximize', False)

    def load_state_dict(self, state_dict):
        """torch's load_state_dict with the momentum buffers kept in place (_load_in_place)"""
        if self._load_in_place(state_dict, ('momentum_buffer',)):
            self.__dict__['_w2l_state_epoch'] = self.__dict__.get('_w2l_state_epoch', 0) + 1

    def _step_eager(self):
        clip = self._begin_eager()
        for group in self.param_groups:
            lr, mu, wd = group['lr'], group['momentum'], group['weight_decay']
            nesterov, dampening, maximize = group['nesterov'], group['dampening'], group.get('maximize', False)
            self._set_hp(group, (lr, mu, wd, nesterov))
            fused_ok = mu != 0 and dampening == 0 and not maximize
            rest, fused = [], []
            for p in group['params']:
                if p.grad is None:
                    continue
                g = p.grad
                if fused_ok and _conv_ok(p, g):
                    fused.append((p, g))
                else:
                    rest.append(p)
            if rest:
                self._plain(rest, lr, mu, wd, nesterov, dampening, maximize, clip)
            self._run_fused(fused, (lr, mu, wd, nesterov), clip)

    def _fused_conv(self, p, g, lr, mu, wd, nesterov, clip=None):
        state = self.state[p]
        first = state.get('momentum_buffer') is None                 # (the kernel is told, and does not read the fresh buffer)
        buf = self._same_layout_buffer(p, state, 'momentum_buffer', 'momentum buffer')
        cout, cin, kw = p.shape
        cache, precise, bufs, recycle, f8 = _operands(p, self.recycle_grads)
        args = (ptr(p), ptr(g), ptr(buf), int(first), float(lr), float(mu), float(wd), int(nesterov), int(recycle), cout, cin, kw,
                *(ptr(b) for b in bufs), ptr(f8['q']) if f8 else None, ptr(f8['qd']) if f8 else None, f8['scale'] if f8 else 1.0)
        if clip is None:
            check(lib.w2l_sgd_pack(*args, stream_ptr()), 'w2l_sgd_pack')
        else:                                                        # (gradient clipping armed: clip_grad_norm_ / _value_)
            check(lib.w2l_sgd_pack_clip(*args, ptr(clip), stream_ptr()), 'w2l_sgd_pack_clip')
        return _packed(p, g, cache, precise, bufs, recycle, f8)

    def _small_multi(self, params, lr, mu, wd, nesterov, clip=None) -> bool:
        """torch.optim.SGD's update of all the small parameters in one launch (w2l_sgd_small_multi): a device table of
        (p, g, m, n) built once per set of addresses (``params``: those _multi_ok admits)"""
        rows = []
        for p in params:
            m = self.state[p].get('momentum_buffer') if mu != 0 else None
            rows.append((p.data_ptr(), p.grad.data_ptr(), m.data_ptr() if m is not None else 0, p.numel()))
        hp = (float(lr), float(mu), float(wd), int(nesterov))
        if clip is None:
            self._launch_small('w2l_sgd_small_multi', params, rows, *hp)
        else:
            self._launch_small('w2l_sgd_small_multi_clip', params, rows, *hp, ptr(clip))
        return True

    def _multi_ok(self, p, mu) -> bool:
        """may this parameter take the one-launch elementwise update?  (with momentum: only once its buffer exists)"""
        return self._elementwise_ok(p, [self.state[p].get('momentum_buffer')] if mu != 0 else [])

    def _plain(self, params, lr, mu, wd, nesterov, dampening, maximize, clip=None):
        # (not under hipGraph capture: the gradient addresses -- and with them the table -- are the capture's own, and building
        # the table is a host-to-device copy from pageable memory, which a capturing stream refuses)
        if not maximize and dampening == 0 and params and not torch.cuda.is_current_stream_capturing():
            multi = [p for p in params if self._multi_ok(p, mu)]
            if multi and self._small_multi(multi, lr, mu, wd, nesterov, clip):
                if len(multi) == len(params):
                    return
                taken = set(id(p) for p in multi)
                params = [p for p in params if id(p) not in taken]
        _lib.poison('torch foreach update of the small parameters')
        grads = [p.grad for p in params]
        if clip is not None:            # the armed coefficient and bound, read on the device (no host sync)
            coef, bound = clip[_lib.CLIP_COEF], clip[_lib.CLIP_BOUND]
            grads = [torch.clamp(g, min=-bound, max=bound) for g in torch._foreach_mul(grads, coef)]
        if maximize:
            grads = torch._foreach_neg(grads)
        if wd != 0:
            grads = torch._foreach_add(grads, params, alpha=wd)
        if mu != 0:
            bufs = []
            fresh = []
            for p, g in zip(params, grads):
                st = self.state[p]
                if st.get('momentum_buffer') is None:
                    st['momentum_buffer'] = torch.clone(g).detach()
                    fresh.append(True)
                else:
                    fresh.append(False)
                bufs.append(st['momentum_buffer'])
            old = [b for b, f in zip(bufs, fresh) if not f]
            oldg = [g for g, f in zip(grads, fresh) if not f]
            if old:
                torch._foreach_mul_(old, mu)
                torch._foreach_add_(old, oldg, alpha=1 - dampening)
            if nesterov:
                grads = torch._foreach_add(grads, bufs, alpha=mu)
            else:
                grads = bufs
        torch._foreach_add_(params, grads, alpha=-lr)


class FusedAdamW(FusedBase, torch.optim.AdamW):
    """torch.optim.Adam / AdamW (``decoupled_weight_decay`` per group; amsgrad, maximize, capturable, differentiable off) with
    the conv-weight update fused with the operand pack of the next step (w2l_adam_pack) and every other device parameter in
    one launch (w2l_adam_small_multi).  State is torch's: per parameter ``step`` (a host count), ``exp_avg``, ``exp_avg_sq``.

    What changes from step to step -- the learning rate of a per-step schedule and the two bias corrections -- lives in
    device memory, per parameter group: ``state`` {step, beta1^step, beta2^step} and the float[4] ``dyn`` the kernels read,
    advanced by w2l_adam_tick at the top of every step().  A recorded optimizer phase names the buffers, not the values, so
    it stays valid while the learning rate moves (replay.opt_signature leaves it out).

    One bias correction per group: the fused path takes a parameter only while its own ``step`` equals the group's count.  A
    parameter that missed a gradient has its own bias correction from then on and is updated by torch ops, with its own
    count, for good; a step with such a parameter is not replayed."""

    @classmethod
    def from_adam(cls, opt) -> 'FusedAdamW':
        if type(opt) not in (torch.optim.Adam, torch.optim.AdamW):
            raise TypeError(f'from_adam takes a torch.optim.Adam or AdamW, got {type(opt).__name__}')
        for group in opt.param_groups:
            if not cls._group_supported(group):
                raise ValueError('FusedAdamW does not take amsgrad, maximize, capturable or differentiable')
        new = cls.__new__(cls)
        new.__dict__.update(opt.__dict__)
        for group in new.param_groups:
            group.setdefault('decoupled_weight_decay', type(opt) is torch.optim.AdamW)
        new._steps_to_host()
        new._rebuild_counters()
        return new

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        for group in self.param_groups:
            group.setdefault('decoupled_weight_decay', True)
            if not self._group_supported(group):
                raise ValueError('FusedAdamW does not take amsgrad, maximize, capturable or differentiable')

    def __setstate__(self, state):
        # (torch.optim.AdamW.__setstate__ forces decoupled_weight_decay on: the flag here is per group, Adam's or AdamW's)
        flags = [g.get('decoupled_weight_decay') for g in state.get('param_groups', [])]
        super().__setstate__(state)
        for g, flag in zip(self.param_groups, flags):
            if flag is not None:
                g['decoupled_weight_decay'] = flag

    @staticmethod
    def _group_supported(group) -> bool:
        return not (group.get('amsgrad') or group.get('maximize') or group.get('capturable') or group.get('differentiable'))

    def _group_fused_ok(self, group) -> bool:
        return self._group_supported(group)

    # ------------------------------------------------------------------ per-group step scalars
    def _scalars(self, gi):
        """group ``gi``'s host mirror {count, pow1, pow2} and, once a device parameter has stepped, its device ``state`` / ``dyn``"""
        table = self.__dict__.setdefault('_w2l_adam', {})
        gs = table.get(gi)
        if gs is None:
            gs = table[gi] = {'count': 0, 'pow1': 1.0, 'pow2': 1.0, 'betas': None, 'state': None, 'dyn': None}
        return gs

    def _device_scalars(self, gs, dev):
        if gs['state'] is None or gs['state'].device != dev:
            _lib.poison('Adam step scalars created')
            gs['state'] = torch.empty(3, dtype=torch.float64, device=dev)            # w2l_adam_state_t
            gs['dyn'] = torch.zeros(4, dtype=torch.float32, device=dev)
            self._upload(gs)
        return gs

    @staticmethod
    def _upload(gs):
        import numpy as np
        host = np.zeros(1, dtype=[('step', '<i8'), ('pow1', '<f8'), ('pow2', '<f8')])
        host['step'], host['pow1'], host['pow2'] = gs['count'], gs['pow1'], gs['pow2']
        gs['state'].copy_(torch.from_numpy(host.view(np.float64).copy()))            # (bits, not values: same dtype, no cast)

    def _in_sync(self, p, gs) -> bool:
        st = self.state.get(p)
        return (st['step'] if st is not None and 'step' in st else 0) == gs['count']

    def accepts(self, p) -> bool:
        if not super().accepts(p):
            return False
        group = self._deferred_state()['hp'][id(p)][1]
        index = self.__dict__.get('_w2l_group_index')
        if index is None or len(index) != len(self.param_groups) or id(group) not in index:
            index = self.__dict__['_w2l_group_index'] = {id(g): i for i, g in enumerate(self.param_groups)}
        return self._in_sync(p, self._scalars(index[id(group)]))     # (out of step with its group: torch ops, never held back)

    def _before_step(self) -> bool:
        """Count the step -- per parameter on the host, per group on the host and on the device (w2l_adam_tick) -- and sort
        the parameters into those that share the group's bias correction and those that have their own."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            # A captured step would bake this step's host counts into the graph: every parameter that takes torch ops (and,
            # with the table built from pageable memory ruled out under capture, that is every small parameter) would keep the
            # bias correction of the captured step on every replay, and the host counts that state_dict() stores would stand
            # still.  torch.optim.Adam refuses the same way (capturable=False); step replay (replay.py) is the supported way
            # to take the host out of the optimizer phase.
            raise RuntimeError('FusedAdamW.step() cannot run under hipGraph capture (graph.GraphedTrainStep, torch.cuda.graph): '
                               'its step counts live on the host, a captured step would replay the bias corrections of the '
                               'captured step for good.  Use the recorded-step replay (the default), or FusedSGD.')
        replayable = True
        held = set()
        for eng in self._engines():
            # held-back updates of the LAST step that no forward pass has launched (two steps with no forward pass between
            # them): they must read the ``dyn`` of their own step, so they are launched and joined now, before the tick
            old = [r for r in eng._deferred if self.stepped(r.token)]
            if old:
                new = [r for r in eng._deferred if not self.stepped(r.token)]
                eng._deferred = old
                eng.flush_deferred()
                eng.join_side()
                eng._deferred = new + eng._deferred
                replayable = False
            held.update(id(r.conv.weight) for r in eng._deferred if not self.stepped(r.token))
        # The tick overwrites ``dyn``, which the updates of the LAST step read.  Those on the side stream: the caller's stream
        # waits for it here (they are long done -- the forward pass between the two steps waited for each weight's event).
        # Those held back (phase X, or an eager apply(), on the weight-gradient stream) ran under that forward pass, each
        # followed by a record of its weight's event, and that layer's forward convolution waited for the event on the
        # caller's stream: every update of step s is ordered before the backward pass of step s+1, hence before this tick.
        # Held-back updates that no forward pass has launched yet were launched and joined just above.
        side = self._side_state()
        if side['pending'] and side['stream'] is not None:
            _lib.stream_wait_stream(_lib.raw_stream(), side['stream'])
        plan = []
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group['params'] if p.grad is not None or id(p) in held]
            if not live:
                plan.append(None)
                continue
            gs = self._scalars(gi)
            own = set()
            for p in live:
                st = self.state[p]
                if 'step' not in st:
                    st['step'] = 0
                if st['step'] != gs['count']:
                    own.add(id(p))
                st['step'] += 1
            if own:
                replayable = False
            beta1, beta2 = float(group['betas'][0]), float(group['betas'][1])
            dev = next((p.device for p in live if p.is_cuda), None)
            if dev is not None:
                self._device_scalars(gs, dev)
            if gs['betas'] != (beta1, beta2):
                # a scheduler that moves the betas (OneCycleLR's cycle_momentum): torch's corrections are 1 - beta**step with
                # the CURRENT beta, so the powers start over from it -- and the update launches carry the betas by value,
                # so such a step is recorded anew (replay.opt_signature)
                if gs['betas'] is not None:
                    gs['pow1'], gs['pow2'] = beta1 ** gs['count'], beta2 ** gs['count']
                    if gs['state'] is not None:
                        self._upload(gs)
                gs['betas'] = (beta1, beta2)
            gs['count'] += 1
            gs['pow1'] *= beta1
            gs['pow2'] *= beta2
            if dev is not None:
                # the ONLY call of a step whose arguments change from step to step: issued here, eagerly, outside any recorded
                # list, on the stream the optimizer phase starts from -- the side stream's first act is to wait for this stream
                check(lib.w2l_adam_tick(ptr(gs['state']), ptr(gs['dyn']), float(group['lr']), float(beta1), float(beta2),
                                        stream_ptr()), 'w2l_adam_tick')
            plan.append((gs, own))
        self.__dict__['_w2l_plan'] = plan
        return replayable

    def _step_eager(self):
        clip = self._begin_eager()
        plan = self.__dict__.pop('_w2l_plan')
        for group, ent in zip(self.param_groups, plan):
            if ent is None:
                continue
            gs, own = ent
            beta1, beta2 = group['betas']
            hp = (float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']),
                  int(bool(group['decoupled_weight_decay'])), gs['dyn'].data_ptr() if gs['dyn'] is not None else 0)
            self._set_hp(group, hp)
            fused, small, rest = [], [], []
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                if id(p) in own or gs['dyn'] is None or g.is_sparse:
                    rest.append(p)
                elif _conv_ok(p, g):
                    fused.append((p, g))
                elif self._small_ok(p):
                    small.append(p)
                else:
                    rest.append(p)
            if rest:
                self._torch_adam(rest, group, clip)
            if small:
                self._small_multi(small, hp, clip)
            self._run_fused(fused, hp, clip)

    def _moments(self, p):
        st = self.state[p]
        return (self._same_layout_buffer(p, st, 'exp_avg', 'Adam moment buffer'),
                self._same_layout_buffer(p, st, 'exp_avg_sq', 'Adam moment buffer'))

    def _fused_conv(self, p, g, beta1, beta2, eps, wd, decoupled, dyn_ptr, clip=None):
        m, v = self._moments(p)
        cout, cin, kw = p.shape
        cache, precise, bufs, recycle, f8 = _operands(p, self.recycle_grads)
        check(lib.w2l_adam_pack(ptr(p), ptr(g), ptr(m), ptr(v), dyn_ptr, beta1, beta2, eps, wd, decoupled, int(recycle), cout, cin,
                                kw, *(ptr(b) for b in bufs), ptr(f8['q']) if f8 else None, ptr(f8['qd']) if f8 else None,
                                f8['scale'] if f8 else 1.0, ptr(clip), stream_ptr()), 'w2l_adam_pack')
        return _packed(p, g, cache, precise, bufs, recycle, f8)

    def _small_ok(self, p) -> bool:
        st = self.state[p]
        if st.get('exp_avg') is None or st.get('exp_avg_sq') is None:
            _lib.poison('Adam moment buffer created')
            st['exp_avg'], st['exp_avg_sq'] = torch.zeros_like(p), torch.zeros_like(p)
        return self._elementwise_ok(p, [st['exp_avg'], st['exp_avg_sq']])

    def _small_multi(self, params, hp, clip=None):
        """every small parameter of a group in one launch (w2l_adam_small_multi): a device table of (p, g, m, v, n) built
        once per set of addresses"""
        beta1, beta2, eps, wd, decoupled, dyn_ptr = hp
        rows = [(p.data_ptr(), p.grad.data_ptr(), self.state[p]['exp_avg'].data_ptr(), self.state[p]['exp_avg_sq'].data_ptr(),
                 p.numel()) for p in params]
        self._launch_small('w2l_adam_small_multi', params, rows, dyn_ptr, beta1, beta2, eps, wd, decoupled, ptr(clip))

    def _torch_adam(self, params, group, clip=None):
        """torch's own rule (_single_tensor_adam) with each parameter's OWN step count: parameters out of step with their
        group, and whatever the kernels do not take (host tensors, other dtypes, gradients in another layout than the parameter's)"""
        _lib.poison('torch update of parameters outside the fused Adam path')
        lr, (beta1, beta2), eps, wd = group['lr'], group['betas'], group['eps'], group['weight_decay']
        for p in params:
            g, st = p.grad, self.state[p]
            if st.get('exp_avg') is None:
                st['exp_avg'], st['exp_avg_sq'] = torch.zeros_like(p), torch.zeros_like(p)
            m, v, t = st['exp_avg'], st['exp_avg_sq'], st['step']
            if clip is not None and g.is_cuda:     # the armed coefficient and bound, read on the device (no host sync)
                bound = clip[_lib.CLIP_BOUND]
                g = torch.clamp(g * clip[_lib.CLIP_COEF], min=-bound, max=bound)
            if group['decoupled_weight_decay']:
                p.mul_(1 - lr * wd)
            elif wd != 0:
                g = g.add(p, alpha=wd)
            m.lerp_(g, 1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            denom = (v.sqrt() / math.sqrt(1 - beta2 ** t)).add_(eps)
            p.addcdiv_(m, denom, value=-lr / (1 - beta1 ** t))

    # ------------------------------------------------------------------ state dict
    def _steps_to_host(self):
        for st in self.state.values():
            if 'step' in st and not isinstance(st['step'], int):
                st['step'] = int(round(float(st['step'])))

    def _rebuild_counters(self):
        """the group counts (host and device) from the parameters' ``step``: the largest of the group -- whoever is behind
        it missed a gradient once and keeps its own count"""
        for gi, group in enumerate(self.param_groups):
            gs = self._scalars(gi)
            steps = [self.state[p]['step'] for p in group['params'] if p in self.state and 'step' in self.state[p]]
            gs['count'], gs['pow1'], gs['pow2'] = max(steps, default=0), 1.0, 1.0
            beta1, beta2 = float(group['betas'][0]), float(group['betas'][1])
            gs['betas'] = (beta1, beta2)
            for _ in range(gs['count']):           # the running products of w2l_adam_tick, multiply for multiply
                gs['pow1'] *= beta1
                gs['pow2'] *= beta2
            if gs['state'] is not None:
                self._upload(gs)                   # (in place: recorded phases name the buffers)

    def state_dict(self):
        """torch.optim.AdamW's state dict: ``step`` as torch keeps it (a host tensor), the moments, no device scratch"""
        sd = super().state_dict()                  # (joins the streams first)
        dtype = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
        sd['state'] = {k: {n: (torch.tensor(float(x), dtype=dtype) if n == 'step' else x) for n, x in st.items()}
                       for k, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        """torch's load_state_dict with the moments kept in place (_load_in_place); the group counters are rebuilt from
        ``step``"""
        mine = [g['decoupled_weight_decay'] for g in self.param_groups]
        stale = self._load_in_place(state_dict, ('exp_avg', 'exp_avg_sq'))
        self._steps_to_host()
        for g, saved, flag in zip(self.param_groups, state_dict['param_groups'], mine):
            if 'decoupled_weight_decay' not in saved:          # (a state dict of a torch without the key: the rule stays ours)
                g['decoupled_weight_decay'] = flag
        self.__dict__.pop('_w2l_plan', None)
        self._rebuild_counters()
        # (always a new epoch: which parameters share their group's count may have changed, and with it what phase O launches)
        self.__dict__['_w2l_state_epoch'] = self.__dict__.get('_w2l_state_epoch', 0) + 1 + int(stale)

    def _replay_signature(self):
        """what a recorded optimizer phase depends on (replay.opt_signature): everything the launches carry by value, and the
        ``dyn`` buffers they read the learning rate and the bias corrections from -- NOT the learning rate"""
        table = self.__dict__.get('_w2l_adam', {})
        return tuple((tuple(float(b) for b in g['betas']), float(g['eps']), float(g['weight_decay']), bool(g['decoupled_weight_decay']),
                      table[gi]['dyn'].data_ptr() if gi in table and table[gi]['dyn'] is not None else 0)
                     for gi, g in enumerate(self.param_groups)) + (self.__dict__.get('_w2l_state_epoch', 0), self._clip_signature())

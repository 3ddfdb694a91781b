"""The inference path on a real MI355X: the fused convolution epilogue (w2l_conv1d_igemm_bnact) through the C ABI against
the three-launch chain it replaces and an fp64 evaluation of the same bf16 operands; ``model.infer`` against the
reference-generated fixtures; the folded-BatchNorm cache; the ``test`` command line end to end."""
import ast
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from gpu_helpers import build_jasper, build_w2l, scale_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')

def _conv_shapes():
    """every distinct convolution of the Wav2Letter table (defaults.W2L_LAYERS) and of Jasper 10x5
    (defaults.jasper10x5_model), derived from the tables themselves: (Cin, Cout, kernel, stride, dilation).  A Jasper block of
    ``repeat`` convolutions (jasper.py:166-174: every repeat with the block's kernel, stride and dilation, the first from the
    block's input width) plus, for a residual block, the 1x1 convolution inplanes -> planes (jasper.py:177-181)."""
    from wav2letter_pytorch_amd import defaults
    shapes = []

    def add(*sh):
        if sh not in shapes:
            shapes.append(sh)
    cin = 64
    for c, k, s, d, _ in defaults.W2L_LAYERS:
        add(cin, c, k, s, d)
        cin = c
    cin = 64
    for b in defaults.jasper10x5_model().jasper_blocks:
        c, k, s, d = b['layer_size'], b['kernel_size'], b['stride'], b.get('dilation', 1)
        k = k + 1 if k % 2 == 0 else k                           # even kernels are bumped to odd (jasper.py:53-58)
        for r in range(b.get('repeat', 1)):
            add(cin if r == 0 else c, c, k, s, d)
        if b['residual']:
            add(cin, c, 1, 1, 1)
        cin = c
    return shapes


CONV_SHAPES = _conv_shapes()
# the tables' own widths: thirteen Wav2Letter convolutions, Jasper's 1x1 residual convolutions of all nine width pairs
assert len(CONV_SHAPES) >= 22 and (64, 256, 11, 2, 1) in CONV_SHAPES and (896, 896, 29, 1, 2) in CONV_SHAPES
assert all((a, c, 1, 1, 1) in CONV_SHAPES for a, c in ((256, 256), (256, 384), (384, 384), (384, 512), (512, 512), (512, 640),
                                                        (640, 640), (640, 768), (768, 768)))


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _ref_rows(T, pl, pr, reflect):
    """padded row -> source frame (-1: a zero row)"""
    rows = []
    for r in range(pl + T + pr):
        t = r - pl
        if t < 0:
            t = -t if reflect else -1
        elif t >= T:
            t = 2 * (T - 1) - t if reflect else -1
        rows.append(t)
    return np.array(rows)


@pytest.mark.parametrize('N', [1, 3, 32])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fused_kernel_against_unfused_and_fp64(shape, N):
    """Both model families per shape: Wav2Letter (bias, reflect halo, clamp) and Jasper (zero halo, ReLU, ragged lens, with and
    without the residual operand).  Error = RMS difference from the fp64 evaluation over all stored elements (the maximum is
    printed too: both results end in one bf16 rounding, whose half ulp dominates a max norm)."""
    from wav2letter_pytorch_amd._lib import BnActDesc, BnActEpi, check, lib, ptr, stream_ptr
    cin, cout, k, s, d = shape
    g = torch.Generator().manual_seed(cin * 31 + cout * 7 + k + N)
    Tout = 150 if N < 32 else 70
    Tin = (Tout - 1) * s + (k - 1) * d + 1
    dev = torch.device('cuda')
    x = _bf16(torch.randn(N, Tin, cin, generator=g)).to(dev)
    w = _bf16(torch.randn(k, cout, cin, generator=g) / np.sqrt(cin * k)).to(dev)
    bias = (0.1 * torch.randn(cout, generator=g)).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(cout, generator=g)).to(dev), (0.3 * torch.randn(cout, generator=g)).to(dev)
    rmean, rvar = (0.2 * torch.randn(cout, generator=g)).to(dev), (0.5 + torch.rand(cout, generator=g)).to(dev)
    res = _bf16(torch.randn(N, Tout, cout, generator=g)).to(dev)
    lens = torch.randint(Tout // 2, Tout + 1, (N,), generator=g, dtype=torch.int32)
    lens[0] = Tout
    lens_d = lens.to(dev)
    scale, shift = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
    check(lib.w2l_bn_finalize(None, 0, cout, 1, ptr(gamma), ptr(beta), 1e-3, 0.1, ptr(rmean), ptr(rvar), None, None, ptr(scale),
                              ptr(shift), stream_ptr()), 'bn_finalize')
    ones, zeros = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    pad = (k - 1) * d
    # fp64 evaluation of the same bf16 operands
    xf, wf = _f64(x), _f64(w)
    acc = np.zeros((N, Tout, cout))
    for kk in range(k):
        acc += xf[:, kk * d: kk * d + (Tout - 1) * s + 1: s, :] @ wf[kk].T
    cases = [('w2l', True, 1, False, False, (4, 5) if s == 2 else (pad // 2, pad - pad // 2)),
             ('jasper', False, 2, True, False, (max(pad // 2, 1), max(pad // 2, 1))),
             ('jasper+res', False, 2, True, True, (28, 28))]
    if k == 1:        # as infer() launches a residual branch: affine only, dense output (no halo, no mask, exactly Tout rows)
        cases.append(('residual branch', False, 0, False, False, (0, 0)))
    for name, reflect, act, masked, with_res, (pl, pr) in cases:
        z = (acc + (_f64(bias) if reflect else 0.0)) * _f64(scale) + _f64(shift)
        if with_res:
            z = z + _f64(res)
        z = np.clip(z, 0, 20) if act == 1 else (np.maximum(z, 0) if act == 2 else z)
        if masked:
            z = z * (np.arange(Tout)[None, :, None] < lens.numpy()[:, None, None])
        rows = _ref_rows(Tout, pl, pr, reflect)
        ref = np.where(rows[None, :, None] >= 0, z[:, np.maximum(rows, 0), :], 0.0)
        # three rows beyond the padded extent, which must stay untouched (the dense case: exactly Tout rows, as infer() has it)
        R = pl + Tout + pr + (3 if name != 'residual branch' else 0)
        outs = {}
        for which in ('fused', 'unfused'):
            out = torch.full((N, R, cout), 7.0, dtype=torch.bfloat16, device=dev)
            b = ptr(bias) if reflect else None
            if which == 'fused':
                e = BnActEpi()
                e.scale, e.shift, e.res = ptr(scale), ptr(shift), (ptr(res) if with_res else None)
                e.act, e.lens, e.out_hi, e.out_rows = act, (ptr(lens_d) if masked else None), ptr(out), R
                e.pad_l, e.pad_r, e.pad_mode = pl, pr, int(reflect)
                check(lib.w2l_conv1d_igemm_bnact(ptr(x), Tin * cin, N * Tin, ptr(w), None, b, C.byref(e), N, cin, cout, Tout, k,
                                                 s, d, stream_ptr()), 'w2l_conv1d_igemm_bnact')
            else:
                y = torch.empty(N, Tout, cout, dtype=torch.bfloat16, device=dev)
                check(lib.w2l_conv1d_igemm(ptr(x), Tin * cin, N * Tin, ptr(w), ptr(y), 0, 0, b, None, N, cin, cout, Tout, k, s, d,
                                           stream_ptr()), 'w2l_conv1d_igemm')
                dsc = BnActDesc()
                dsc.N, dsc.T, dsc.C, dsc.y, dsc.y_f32 = N, Tout, cout, y.data_ptr(), 0
                dsc.scale, dsc.shift = scale.data_ptr(), shift.data_ptr()
                if with_res:
                    dsc.y2, dsc.scale2, dsc.shift2 = res.data_ptr(), ones.data_ptr(), zeros.data_ptr()
                dsc.act, dsc.drop_p = act, 0.0
                dsc.lens = lens_d.data_ptr() if masked else None
                check(lib.w2l_bn_act_fwd(C.byref(dsc), ptr(out), None, pl + Tout + pr, pl, pr, int(reflect), stream_ptr()),
                      'w2l_bn_act_fwd')
                # (the chain's output buffer has exactly pl + Tout + pr rows per utterance: lay it out in the R-row frame)
                flat = out.view(-1)[: N * (pl + Tout + pr) * cout].view(N, pl + Tout + pr, cout).clone()
                out = torch.full((N, R, cout), 7.0, dtype=torch.bfloat16, device=dev)
                out[:, : pl + Tout + pr] = flat
            torch.cuda.synchronize()
            outs[which] = out
        fused = outs['fused']
        assert bool((fused[:, pl + Tout + pr:] == 7.0).all()), (name, 'rows beyond the padded extent were written')
        got = {kname: _f64(v[:, : pl + Tout + pr]) for kname, v in outs.items()}
        rms = {kname: float(np.sqrt(np.mean((v - ref) ** 2))) for kname, v in got.items()}
        mx = {kname: float(np.abs(v - ref).max()) for kname, v in got.items()}
        print(f'[bnact] {shape} N={N} {name}: rms fused {rms["fused"]:.3e} unfused {rms["unfused"]:.3e}; '
              f'max fused {mx["fused"]:.3e} unfused {mx["unfused"]:.3e}')
        assert rms['fused'] <= rms['unfused'], (name, rms)
        # halo rows: bit-equal to the interior rows they mirror (reflect) or zero
        f16 = fused.view(torch.int16)
        for r, t in enumerate(rows):
            if r - pl == t:
                continue
            if t >= 0:
                assert torch.equal(f16[:, r], f16[:, pl + t]), (name, r, t)
            else:
                assert bool((f16[:, r] == 0).all()), (name, r)
        if masked:
            for n in range(N):
                assert bool((f16[n, pl + int(lens[n]): pl + Tout] == 0).all()), (name, n)


def _fixture_model(case, precision='fp32'):
    z = np.load(os.path.join(GOLD, case + '.npz'), allow_pickle=True)
    meta = ast.literal_eval(str(z['meta']))
    sd = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith('p0/')}
    sd.update({k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith('p1/')})     # state AFTER the training step
    if 'layers' in meta:
        layers = [(l['output_size'], l['kernel_size'], l['stride'], l['dilation'], 0.0) for l in meta['layers']]
        model = build_w2l(layers, sd, precision)
    else:
        model = build_jasper(meta['blocks'], sd, precision)
    return model.eval(), z


MARGIN = 1e-2


@pytest.mark.parametrize('case', ['w2l_ml1', 'w2l_ml3', 'w2l_mix5', 'jasper_dense', 'jasper_sep2', 'jasper_nomask'])
def test_infer_against_reference_fixtures(case):
    """fp32 mode: scale_err(infer, out_eval) < 2e-3 (the bound of the evaluation forward, test_gpu_model.py:135), equal
    lengths, the reference's argmax on every valid frame whose top-two margin (log domain) is at least 1e-2; at most 20 % of
    the valid frames may fall under that margin."""
    from wav2letter_pytorch_amd.decoder import GreedyDecoder, argmax_indices
    model, z = _fixture_model(case)
    x, il = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['in_lens'])
    out, out_lens = model.infer(x, il)
    err = scale_err(out.cpu().numpy(), z['out_eval'])
    print(f'[infer fixtures] {case}: scale_err {err:.3e}')
    again, _ = model.infer(x, il)
    # second call of a shape: every buffer (activations, depthwise outputs, residual tensors, the fp32 scratch) is reused
    assert model.engine().infer_buffers == 0 and torch.equal(again, out)
    assert err < 2e-3, err
    np.testing.assert_array_equal(np.asarray(out_lens), z['out_lens'])
    ref = z['out_eval'].astype(np.float64)
    logref = ref if ref.max() <= 0 else np.log(np.maximum(ref, 1e-300))          # Jasper's eval output is a softmax
    top = np.sort(logref, axis=-1)
    margin = top[..., -1] - top[..., -2]
    valid = np.arange(ref.shape[1])[None, :] < np.asarray(z['out_lens'])[:, None]
    use = valid & (margin >= MARGIN)
    left_out = int(valid.sum() - use.sum())
    print(f'[infer fixtures] {case}: {left_out}/{int(valid.sum())} valid frames under the {MARGIN} margin left out')
    assert left_out <= 0.2 * valid.sum()
    idx = argmax_indices(out).cpu().numpy()
    assert (idx[use] == ref.argmax(-1)[use]).all()
    dec = GreedyDecoder(list(model.labels))
    want = dec.decode(torch.from_numpy(z['out_eval']).cuda(), torch.from_numpy(np.asarray(z['out_lens'])))
    got = dec.decode(out, torch.from_numpy(np.asarray(z['out_lens'])))
    for n in range(ref.shape[0]):
        if not (valid[n] & ~use[n]).any():
            assert got[n] == want[n], n


def test_infer_cache_follows_the_weights(monkeypatch):
    """folded BatchNorm vectors: built once, reused, dropped by train(), load_state_dict, invalidate_packed and an optimizer
    step; infer after a training step uses the new weights; the eval-mode forward is bit-identical before and after infer"""
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd.engine import invalidate_packed
    layers = [(128, 11, 2, 1, 0.0), (128, 13, 1, 2, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=3)
    model = build_w2l(layers, sd, 'bf16').eval()
    x, il, tg, tl = O.synthetic_batch(3, 160, seed=4, s_lo=5, s_hi=15)
    xd = x.cuda()
    with torch.no_grad():
        before, _ = model(xd, il)
    a, _ = model.infer(xd, il)
    eng = model.engine()
    folds = eng.infer_folds
    b, _ = model.infer(xd, il)
    assert eng.infer_folds == folds and torch.equal(a, b)
    assert eng.infer_buffers == 0                     # second call: every activation buffer came from the free list
    with torch.no_grad():
        after, _ = model(xd, il)
    assert torch.equal(before, after)
    assert scale_err(a.cpu().numpy(), before.cpu().numpy()) < 3e-2
    for drop in ('train', 'load', 'invalidate'):
        eng0 = model.engine()
        n0 = eng0.infer_folds
        if drop == 'train':
            model.train().eval()
        elif drop == 'load':
            # a state with other running statistics and BatchNorm weights: infer must compute with THEM
            new_sd = {k_: v.clone() for k_, v in model.state_dict().items()}
            for k_, v in new_sd.items():
                if 'running_mean' in k_:
                    v += 0.3
                elif 'running_var' in k_:
                    v *= 2.5
                elif 'batch_norm.weight' in k_:
                    v *= 1.4
            model.load_state_dict(new_sd)
        else:
            invalidate_packed(model)
        got, _ = model.infer(xd, il)
        # (load_state_dict drops the whole engine, folds included: the new engine's counter starts again; what counts for
        # that leg is the output below)
        assert model.engine().infer_folds > (n0 if model.engine() is eng0 else 0), drop
        if drop == 'load':
            with torch.no_grad():
                want_l, _ = model(xd, il)
            assert scale_err(got.cpu().numpy(), want_l.cpu().numpy()) < 3e-2
            assert scale_err(got.cpu().numpy(), a.cpu().numpy()) > 3e-2          # (and the old state's result is far away)
    # one optimizer step: infer must see the new weights and running statistics (= the eval forward of the new state)
    model.train()
    opt = model.configure_optimizers()[0][0]
    for g_ in opt.param_groups:
        g_['lr'] = 0.05
    out, ol = model(xd, il)
    model.criterion(out.transpose(0, 1), tg, ol, tl).backward()
    opt.step()
    getattr(opt, 'join', lambda: None)()
    model.eval()
    c, _ = model.infer(xd, il)
    with torch.no_grad():
        want, _ = model(xd, il)
    assert not torch.equal(c, a)
    assert scale_err(c.cpu().numpy(), want.cpu().numpy()) < 3e-2
    monkeypatch.setattr('wav2letter_pytorch_amd.engine.FUSED_INFER', False)
    off, _ = model.infer(xd, il)
    assert torch.equal(off, want)                     # W2L_FUSED_INFER=0: the evaluation forward itself


def test_infer_between_replayed_training_steps():
    """the default training path replays recorded launch lists after a few warm steps: the running statistics and the small
    parameters then move through raw pointers, with no eager forward and no version bump.  infer() called between such steps,
    on a model left in training mode, must still compute with the current state."""
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd import replay
    from wav2letter_pytorch_amd.layers import run_stack
    layers = [(128, 11, 2, 1, 0.0), (128, 13, 1, 2, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=5)
    model = build_w2l(layers, sd, 'bf16').train()
    opt = model.configure_optimizers()[0][0]
    for g_ in opt.param_groups:
        g_['lr'] = 0.02
    x, il, tg, tl = O.synthetic_batch(3, 160, seed=6, s_lo=5, s_hi=15)
    probe = x.cuda()
    f0, o0 = replay.STATS['replayed_F'], replay.STATS['replayed_O']
    prev = None
    for step in range(8):
        xs = (x * (1.0 + 0.6 * step) + 0.2 * step).cuda()            # every step moves the running statistics visibly
        opt.zero_grad(set_to_none=True)
        out, ol = model(xs, il)
        model.criterion(out.transpose(0, 1), tg, ol, tl).backward()
        opt.step()
        folds = model.engine().infer_folds if hasattr(model.engine(), 'infer_folds') else 0
        got, _ = model.infer(probe, il)                              # no mode toggle, no eager forward in between
        assert model.training
        with torch.no_grad():                                        # the evaluation forward of the same state, mode untouched
            want, _ = run_stack(model.engine(), probe, None, False, softmax_mode=0)
        err = scale_err(got.cpu().numpy(), want.cpu().numpy())
        assert err < 3e-2, (step, err)
        assert model.engine().infer_folds > folds, step
        if prev is not None:
            assert scale_err(got.cpu().numpy(), prev.cpu().numpy()) > 3e-2, step     # (the state did move: a stale fold would show)
        prev = got
    getattr(opt, 'join', lambda: None)()
    if replay.ENABLED:                                               # (W2L_REPLAY=0: the same checks, on eager steps)
        assert replay.STATS['replayed_F'] - f0 >= 3 and replay.STATS['replayed_O'] - o0 >= 3, dict(replay.STATS)


def test_pad_channels_stay_zero():
    """a logical channel count that is not a multiple of 64 (48 of 64): the operand pack's pad rows are zero, the padded
    per-channel vectors are bias 0 / scale 1 / shift 0 -- the fused launch must store exact zeros into the pad channels of
    every row it writes, as the consumer assumes"""
    from wav2letter_pytorch_amd._lib import BnActEpi, check, lib, ptr, stream_ptr
    g = torch.Generator().manual_seed(9)
    N, cin, cp, c, k, Tout = 3, 64, 64, 48, 11, 150
    Tin = Tout + k - 1
    dev = torch.device('cuda')
    x = _bf16(torch.randn(N, Tin, cin, generator=g)).to(dev)
    w = torch.zeros(k, cp, cin)
    w[:, :c] = torch.randn(k, c, cin, generator=g) / np.sqrt(cin * k)
    w = _bf16(w).to(dev)
    bias, scale, shift = torch.zeros(cp), torch.ones(cp), torch.zeros(cp)
    bias[:c], scale[:c], shift[:c] = 0.1 * torch.randn(c, generator=g), 1 + 0.2 * torch.randn(c, generator=g), torch.randn(c, generator=g)
    bias, scale, shift = bias.to(dev), scale.to(dev), shift.to(dev)
    res = torch.zeros(N, Tout, cp)
    res[:, :, :c] = torch.randn(N, Tout, c, generator=g)
    res = _bf16(res).to(dev)
    for reflect, act, with_res, (pl, pr) in ((True, 1, False, (4, 5)), (False, 2, True, (14, 14)), (False, 0, False, (0, 0))):
        R = pl + Tout + pr
        out = torch.full((N, R, cp), 7.0, dtype=torch.bfloat16, device=dev)
        e = BnActEpi()
        e.scale, e.shift, e.res = ptr(scale), ptr(shift), (ptr(res) if with_res else None)
        e.act, e.out_hi, e.out_rows, e.pad_l, e.pad_r, e.pad_mode = act, ptr(out), R, pl, pr, int(reflect)
        check(lib.w2l_conv1d_igemm_bnact(ptr(x), Tin * cin, N * Tin, ptr(w), None, ptr(bias), C.byref(e), N, cin, cp, Tout, k, 1, 1,
                                         stream_ptr()), 'w2l_conv1d_igemm_bnact')
        torch.cuda.synchronize()
        assert bool((out.view(torch.int16)[:, :, c:] == 0).all()), (reflect, act)
        assert bool((out[:, :, :c] != 7.0).any(dim=-1).all()), (reflect, act)      # every row was written


def _write_wavs(tmp_path, n, sr=16000):
    import wave
    rng = np.random.default_rng(0)
    words = ['ab', 'cab', 'a', 'bca', 'ba c']
    rows = []
    for i in range(n):
        sig = (0.1 * rng.standard_normal(int(sr * (0.6 + 0.1 * (i % 3))))).astype(np.float32)
        p = str(tmp_path / f'u{i}.wav')
        with wave.open(p, 'wb') as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
            f.writeframes((sig * 32767).astype(np.int16).tobytes())
        rows.append({'audio_filepath': p, 'text': words[i % len(words)] + ' ' + words[(i + 2) % len(words)]})
    man = str(tmp_path / 'manifest.json')
    with open(man, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')
    return man, rows


def test_test_cli_end_to_end(tmp_path, monkeypatch):
    """train a few steps on a synthetic WAV manifest, then the ``test`` command line on the checkpoint: reported CER / WER equal
    the values recomputed from the output file's strings; beam decoders and word times run; transcribe returns the same text"""
    from wav2letter_pytorch_amd import test as T, train
    from wav2letter_pytorch_amd.decoder import GreedyDecoder
    # (no dither: the loader draws it on the device, and two passes over the files must see the same features)
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    man, rows = _write_wavs(tmp_path, 6)
    root = str(tmp_path / 'run')
    common = ['model.mid_layers=2', 'data.batch_size=3']
    trainer, model = train.main(common + [f'data.train_manifest={man}', f'data.val_manifest={man}', 'trainer.max_epochs=1',
                                          f'trainer.default_root_dir={root}', 'model.optimizer.lr=1e-3'])
    ckpt = [os.path.join(root, f) for f in os.listdir(root) if f.endswith('.ckpt')][0]
    out = str(tmp_path / 'hyp.jsonl')
    metrics, records = T.main(common + [f'model_path={ckpt}', f'data.test_manifest={man}', f'output={out}', 'word_times=true',
                                        'print_samples=2'])
    lines = [json.loads(l) for l in open(out)]
    assert len(lines) == len(rows) == len(records)
    dec = GreedyDecoder(list(model.labels))
    ce, cr = map(sum, zip(*(dec.cer_ratio(r['text'], r['hypothesis']) for r in lines)))
    we, wr = map(sum, zip(*(dec.wer_ratio(r['text'], r['hypothesis']) for r in lines)))
    assert abs(metrics['test_cer'] - ce / cr) < 1e-12 and abs(metrics['test_wer'] - we / wr) < 1e-12
    assert np.isfinite(metrics['test_loss'])
    for r in lines:
        assert len(r['words']) == len(r['hypothesis'].split())
        starts = [w['start'] for w in r['words']]
        assert starts == sorted(starts) and all(w['end'] >= w['start'] for w in r['words'])
    # W2L_FUSED_INFER=0: the hypotheses are GreedyDecoder.decode(model.eval()(x)) over the same batches
    monkeypatch.setattr('wav2letter_pytorch_amd.engine.FUSED_INFER', False)
    from wav2letter_pytorch_amd.data.data_loader import BatchAudioDataLoader, SpectrogramDataset
    cfg = T.build_config(common + [f'model_path={ckpt}', f'data.test_manifest={man}'])
    model.load_state_dict(torch.load(ckpt, map_location='cpu')['state_dict'])
    model.eval()
    _, rec0 = T.main(common + [f'model_path={ckpt}', f'data.test_manifest={man}'])
    ds = SpectrogramDataset(man, cfg.data.audio_conf, list(model.labels), mel_spec=cfg.data.mel_spec)
    want = []
    with torch.no_grad():
        for batch in BatchAudioDataLoader(ds, batch_size=3):
            o, ol = model(batch[0].cuda(), batch[1])
            want += dec.decode(o, ol)
    assert [r['hypothesis'] for r in rec0] == want
    monkeypatch.setattr('wav2letter_pytorch_amd.engine.FUSED_INFER', True)
    _, rec1 = T.main(common + [f'model_path={ckpt}', f'data.test_manifest={man}'])
    got = model.transcribe([r['audio_filepath'] for r in rows], batch_size=3)
    assert got == [r['hypothesis'] for r in rec1]
    # Trainer.test on the same checkpoint and loader: the command line's greedy metrics; test_step logs under the prefix 'test'
    from wav2letter_pytorch_amd.trainer import Trainer
    loader = BatchAudioDataLoader(ds, batch_size=3)
    m_tr = Trainer(enable_checkpointing=False).test(model, loader, ckpt_path=ckpt)
    m_cli, _ = T.main(common + [f'model_path={ckpt}', f'data.test_manifest={man}'])
    assert set(m_tr) == {'test_loss', 'test_cer', 'test_wer', 'test_len_ratio'}
    for key in ('test_cer', 'test_wer', 'test_len_ratio'):
        assert abs(m_tr[key] - m_cli[key]) < 1e-12, key
    assert abs(m_tr['test_loss'] - m_cli['test_loss']) < 1e-5 * abs(m_cli['test_loss'])
    batch = next(iter(loader))
    model.eval()
    loss = model.test_step(batch, 0)
    logged = getattr(model, '_logged', None)
    assert torch.isfinite(loss) and not loss.requires_grad
    if logged is not None:                      # (the package's own log_dict: Lightning's keeps its values elsewhere)
        assert {'test_loss', 'test_cer', 'test_wer', 'test_len_ratio'} <= set(logged)
        assert abs(logged['test_loss'] - float(loss)) < 1e-6 * max(1.0, abs(float(loss)))
    # beam search, and beam search with a tiny ARPA model
    arpa = str(tmp_path / 'lm.arpa')
    with open(arpa, 'w') as f:
        f.write('\\data\\\nngram 1=5\n\n\\1-grams:\n-1.0\t<unk>\n-99\t<s>\n-1.0\t</s>\n-0.7\tab\n-0.7\tcab\n\n\\end\\\n')
    for extra in (['decoder=beam', 'beam.k=4'], ['decoder=beam_lm', f'lm_path={arpa}', 'beam.k=4', 'beam.alpha=0.5']):
        m, rec = T.main(common + [f'model_path={ckpt}', f'data.test_manifest={man}'] + extra)
        assert len(rec) == len(rows) and all(isinstance(r['hypothesis'], str) for r in rec)


@pytest.mark.parametrize('net', ['wav2letter', 'jasper10x5'])
def test_infer_full_size_bf16_against_fp32_oracle(net):
    """bf16 mode at full size (Wav2Letter mid_layers=20, N=32 x T=1000; Jasper 10x5, N=16 x T=1000).  Yardstick: the fp32
    oracle's evaluation forward on the batch's first two utterances (what the CPU can afford; full-length utterances, so their
    outputs do not depend on the rest of the batch).  ``infer`` may exceed the existing evaluation forward's error by at most
    25 % -- the allowance is for clamp / ReLU gates and ties that fall the other way; the arithmetic rounds once less."""
    from oracle import w2l_oracle as O
    if net == 'wav2letter':
        layers = [l[:4] + (0.0,) for l in O.W2L_LAYERS]
        sd = O.init_wav2letter_state(layers, seed=0)
        model = build_w2l(layers, sd, 'bf16').eval()
        n = 32
    else:
        from wav2letter_pytorch_amd import Jasper
        from wav2letter_pytorch_amd.defaults import jasper10x5_model
        cfg = jasper10x5_model()
        blocks = [dict(b) for b in cfg.jasper_blocks]
        torch.manual_seed(7)
        sd = {k: v.detach().clone() for k, v in Jasper(cfg).state_dict().items()}
        model = build_jasper(blocks, sd, 'bf16').eval()
        n = 16
    x, il, _, _ = O.synthetic_batch(n, 1000, seed=1234)
    xd = x.cuda()
    with torch.no_grad():
        old, _ = model(xd, il)
    new, _ = model.infer(xd, il)
    with torch.no_grad():
        if net == 'wav2letter':
            ref = O.wav2letter_forward(x[:2], {k: v.clone() for k, v in sd.items()}, layers, training=False)
            ref = ref[0] if isinstance(ref, (tuple, list)) else ref
        else:
            ref, _ = O.jasper_forward(x[:2], il[:2], {k: v.clone() for k, v in sd.items()}, blocks, training=False)
    ref = ref.numpy()
    e_old = scale_err(old[:2].cpu().numpy(), ref)
    e_new = scale_err(new[:2].cpu().numpy(), ref)
    print(f'[infer full size] {net}: scale_err vs fp32 oracle: eval forward {e_old:.4e}, infer {e_new:.4e}')
    assert e_new <= 1.25 * e_old, (e_new, e_old)


def test_fused_kernel_split_k_form():
    """a split-K plan of the fused launch (two blocks per tile through fp32 slabs, the combining block runs the epilogue) gives
    the one-block-per-tile result up to the order of the fp32 sum"""
    from wav2letter_pytorch_amd._lib import BnActEpi, check, lib, ptr, stream_ptr
    g = torch.Generator().manual_seed(2)
    N, cin, cout, k, Tout, pl, pr = 3, 256, 256, 11, 150, 5, 5
    Tin = Tout + k - 1
    dev = torch.device('cuda')
    x = _bf16(torch.randn(N, Tin, cin, generator=g)).to(dev)
    w = _bf16(torch.randn(k, cout, cin, generator=g) / np.sqrt(cin * k)).to(dev)
    scale, shift = (1 + 0.2 * torch.randn(cout, generator=g)).to(dev), torch.randn(cout, generator=g).to(dev)
    ws = torch.zeros(int(lib.w2l_conv_splitk_workspace_bytes(N, cout, Tout)), dtype=torch.uint8, device=dev)
    outs = []
    for idx in (2, 2 + 52):                      # block shape 128 x 128, one block per tile / two blocks per tile
        out = torch.full((N, pl + Tout + pr, cout), 7.0, dtype=torch.bfloat16, device=dev)
        e = BnActEpi()
        e.scale, e.shift, e.act, e.out_hi, e.out_rows = ptr(scale), ptr(shift), 1, ptr(out), pl + Tout + pr
        e.pad_l, e.pad_r, e.pad_mode = pl, pr, 1
        lib.w2l_conv_force_tile_config(idx)
        try:
            check(lib.w2l_conv1d_igemm_bnact_ws(ptr(x), Tin * cin, N * Tin, ptr(w), None, None, C.byref(e), N, cin, cout, Tout, k,
                                                1, 1, ptr(ws), ws.numel(), stream_ptr()), 'w2l_conv1d_igemm_bnact_ws')
        finally:
            lib.w2l_conv_force_tile_config(-1)
        torch.cuda.synchronize()
        outs.append(out.float().cpu().numpy())
    assert not (outs[1] == 7.0).any()
    assert scale_err(outs[1], outs[0]) < 1e-2                    # one bf16 ulp at the top of the range
    assert float(np.mean(outs[1] == outs[0])) > 0.99
    assert bool((ws[: 64 * 1024] == 0).all())                    # tickets are back at zero for the next launch

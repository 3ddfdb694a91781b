"""ASG criterion and Viterbi decoder on a real MI355X against the float64 references of tests/asg_refs.py.

Bounds (the project's own for CTC in fp32): loss within 1e-4 relative, d loss / d x within 1e-3 absolute (a difference of two
posteriors), d loss / d transitions within 1e-3 of the largest magnitude in the reference tensor -- and, beside these flat
bounds, every element of both gradients, every nll and the loss within asg_refs.asg_ref's derived per-element bound (the flat
bound on d loss / d x cannot fail where 1 / (N S) is below it; tests/test_gpu_asg_direct.py calls the kernels on the full case
table under the derived bound alone).  Shapes are the smallest at
which each index and each code path of csrc/asg.hip can go wrong: label padding 5 -> 32, 29 -> 32 and 33 -> 64; T = S (one
path), T = 1, S > T (infeasible); two frame chunks of the gradient kernel (T = 70 > 64); the target-posterior buffer filled in
two passes with a 256-thread target block (S = 130); two target states per thread (S = 1030)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import asg_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGLISH = R.ENGLISH


_log_softmax, _pad, _make = R._log_softmax, R.old_pad, R.old_case


_CACHE = {}


def _case(name, reduction='mean', scale=(1.0, 1.0)):
    """the inputs of a case and its float64 reference, computed once per session and never changed"""
    key = (name, reduction, scale)
    if key not in _CACHE:
        x, g, targets, lens = _make(name)
        x, g = (x * np.float32(scale[0])), (g * np.float32(scale[1]))
        ref = R.asg_loss(x, g, targets, lens, reduction=reduction)
        ref['derived'] = R.old_case_ref(name, reduction, scale)              # the same values with per-element bounds
        _CACHE[key] = (x, g, targets, lens, ref)
    return _CACHE[key]


def _device_loss(x, g, targets, lens, reduction='mean', repeat=0, grads=True):
    """w2l_asg_loss called directly -> dict of host arrays (loss, nll, status, grad_x, grad_g)"""
    from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr
    tg, tl = _pad(targets)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    tgd, tld = torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda()
    ild = torch.tensor(lens, dtype=torch.int32).cuda()
    n, t, a = x.shape
    need = int(lib.w2l_asg_workspace_bytes(n, t, a, tg.shape[1]))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    nll = torch.full((n,), 7.0, device='cuda')
    loss = torch.full((1,), 7.0, device='cuda')
    status = torch.full((n,), 7, dtype=torch.int32, device='cuda')
    gx = torch.full((n, t, a), 7.0, device='cuda') if grads else None
    gg = torch.full((a, a), 7.0, device='cuda') if grads else None
    check(lib.w2l_asg_loss(ptr(xd), ptr(gd), ptr(tgd), ptr(ild), ptr(tld), n, t, a, tg.shape[1], repeat,
                           {'mean': 0, 'sum': 1}[reduction], ptr(nll), ptr(loss), ptr(gx), ptr(gg), ptr(status), ptr(ws), need,
                           stream_ptr()), 'w2l_asg_loss')
    torch.cuda.synchronize()
    return dict(loss=float(loss[0]), nll=nll.cpu().numpy(), status=status.cpu().numpy(),
                grad_x=gx.cpu().numpy() if grads else None, grad_g=gg.cpu().numpy() if grads else None,
                raw=(loss, gx, gg))


def _derived(got, der, what, factor=1.0):
    """every element within asg_ref's derived bound (asg_refs.py; ``factor``: the scale of an upstream gradient)"""
    from direct_helpers import ratio
    rs = {k: ratio(np.asarray(got[k], dtype=np.float64), factor * np.asarray(der[k]), factor * np.asarray(der[k + '_b']))
          for k in ('grad_x', 'grad_g')}
    print(f'ASG {what}: worst |error| / derived bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in rs.items()))
    assert max(rs.values()) <= 1.0, (what, rs)


def _compare(got, ref, lens, what, trans_tol=1e-3):
    der = ref['derived']
    assert abs(der['loss'] - ref['loss']) <= 1e-9 * abs(ref['loss']) and np.abs(der['grad_x'] - ref['grad_x']).max() < 1e-9
    assert abs(got['loss'] - der['loss']) <= der['loss_b'] and (np.abs(got['nll'] - der['nll']) <= der['nll_b']).all(), what
    _derived(got, der, what)
    loss_err = abs(got['loss'] - ref['loss']) / max(abs(ref['loss']), 1e-30)
    nll_err = float(np.max(np.abs(got['nll'] - ref['nll']) / np.maximum(np.abs(ref['nll']), 1.0)))
    gx_err = float(np.abs(got['grad_x'] - ref['grad_x']).max())
    gg_scale = max(float(np.abs(ref['grad_g']).max()), 1e-30)
    gg_err = float(np.abs(got['grad_g'] - ref['grad_g']).max()) / gg_scale
    print(f'ASG {what}: loss rel err {loss_err:.2e} (bound 1e-4), nll rel err {nll_err:.2e}, grad_x abs err {gx_err:.2e} '
          f'(bound 1e-3), grad_trans err / max|ref| {gg_err:.2e} (bound 1e-3)')
    assert np.isfinite(got['loss']) and np.isfinite(got['grad_x']).all() and np.isfinite(got['grad_g']).all()
    assert loss_err < 1e-4 and nll_err < 1e-4
    assert gx_err < 1e-3
    assert gg_err < trans_tol
    for n, tn in enumerate(lens):                      # frames past T_n: exactly zero
        assert not got['grad_x'][n, tn:].any(), n


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('name', ['main', 'a29', 'a33', 'chunks', 'long'])
def test_loss_and_gradients_match_the_float64_reference(name, reduction):
    x, g, targets, lens, ref = _case(name, reduction)
    got = _device_loss(x, g, targets, lens, reduction)
    _compare(got, ref, lens, f'{name}/{reduction}')
    if name == 'main':
        assert got['status'].tolist() == [0, 0, 0, 0, 1]
        assert got['nll'][4] == 0.0 and not got['grad_x'][4].any()          # S = 5 > 3 frames: infeasible
        assert ref['nll'][3] > 0 and got['nll'][3] > 0                      # T = S = 1
    else:
        assert not got['status'].any()
    # the loss alone (no gradient buffers) is the same number
    alone = _device_loss(x, g, targets, lens, reduction, grads=False)
    assert alone['loss'] == got['loss'] and np.array_equal(alone['nll'], got['nll'])


def test_two_target_states_per_thread():
    """S = 1030 > 1024: the 1024-thread target block with two states per thread, which needs T = 1100 frames.  The loss
    bound is the usual 1e-4 and the bound on d loss / d x the usual 1e-3 -- which is above every element's magnitude here
    (w_n = 1 / 1030), so what can fail is _compare's derived per-element bound (a zero gradient leaves it: test_cpu_asg.py).  The bound on d loss / d transitions is the number
    format's at this length, not 1e-3: the kernels keep alpha and
    beta in the log domain in fp32 (as the CTC kernels do), the values reach |Z_tgt| ~ nll ~ 3.3e3 where one fp32 ulp is
    2.4e-4, and every one of the 1100 recursion steps rounds once (0.5 ulp, accumulating as a random walk: sqrt(1100) / 2 ~ 17
    ulp).  A posterior exp(alpha + g + beta - Z) therefore carries a relative error of up to ~17 ulp(3.3e3) = 4e-3, which
    the relative bound on d loss / d transitions sees undiminished.  Measured on the MI355X: 1.2e-3 (d loss / d x, scaled by
    1 / S under 'mean': 8.7e-6)."""
    x, g, targets, lens, ref = _case('spt2', 'mean')
    tol = 0.5 * np.sqrt(x.shape[1]) * float(np.spacing(np.float32(ref['nll'][0])))
    assert 3e-3 < tol < 5e-3
    _compare(_device_loss(x, g, targets, lens, 'mean'), ref, lens, 'spt2/mean', trans_tol=tol)


@pytest.mark.parametrize('name', ['main', 'a33'])
def test_large_dynamic_range(name):
    """emissions x 30, transitions x 10: nothing overflows or underflows to NaN and the bounds still hold.  Both label
    paddings (32 and 64) at T <= 12: the property under test is the per-frame log-sum-exp (maximum subtraction, -inf in the
    padding), which does not depend on T, while at these T the log-domain magnitudes (<= ~4e3, one fp32 ulp 2.4e-4) still
    leave the 1e-3 bound meaningful."""
    for reduction in ('mean', 'sum'):
        x, g, targets, lens, ref = _case(name, reduction, scale=(30.0, 10.0))
        assert np.abs(x).max() > 100
        _compare(_device_loss(x, g, targets, lens, reduction), ref, lens, f'{name}/{reduction} x30/x10')


@pytest.mark.parametrize('name', ['a29', 'chunks'])
def test_two_calls_are_bit_identical(name):
    x, g, targets, lens, _ = _case(name)
    a = _device_loss(x, g, targets, lens)
    b = _device_loss(x, g, targets, lens)
    for u, v in zip(a['raw'], b['raw']):
        assert torch.equal(u, v)


def test_device_repeat_encoding_through_the_module():
    """ASGLoss on raw transcripts with doubled and tripled letters = the reference on encode_repeats of them (autograd path:
    [T, N, C] layout, gradients for log_probs and transitions); a transcript containing index 0 is a ValueError"""
    from wav2letter_pytorch_amd.asg import ASGLoss, encode_repeats
    rng = np.random.default_rng(40)
    N, T, A = 3, 14, 6
    x = _log_softmax(3.0 * rng.standard_normal((N, T, A))).astype(np.float32)
    g = rng.standard_normal((A, A)).astype(np.float32)
    targets = [[1, 1, 2, 2, 2, 3], [4, 4, 4, 4, 4], [5, 1, 1, 5]]
    lens = [14, 14, 9]
    enc = [encode_repeats(t) for t in targets]
    assert enc == [[1, 0, 2, 0, 2, 3], [4, 0, 4, 0, 4], [5, 1, 0, 5]]
    # the reference on the ENCODED targets, with a repeat label (-1) that never occurs: no second encoding
    ref = R.asg_loss(x, g, enc, lens, repeat=-1)
    crit = ASGLoss(A).cuda()
    with torch.no_grad():
        crit.transitions.copy_(torch.from_numpy(g))
    lp = torch.from_numpy(x).cuda().transpose(0, 1).contiguous().requires_grad_(True)       # [T, N, C]
    tg, tl = _pad(targets)
    loss = crit(lp, torch.from_numpy(tg).cuda(), torch.tensor(lens), torch.from_numpy(tl))
    (2.0 * loss).backward()
    assert abs(float(loss.detach()) - ref["loss"]) / abs(ref["loss"]) < 1e-4
    assert np.abs(lp.grad.transpose(0, 1).cpu().numpy() - 2.0 * ref['grad_x']).max() < 1e-3
    assert np.abs(crit.transitions.grad.cpu().numpy() - 2.0 * ref['grad_g']).max() < 1e-3 * 2.0 * np.abs(ref['grad_g']).max()
    tg0, tl0 = _pad(targets)
    der = R.asg_ref(x, g, tg0, lens, tl0, 0, 'mean', tg0.shape[1])           # raw transcripts: the encoding is the reference's own
    assert abs(der['loss'] - ref['loss']) < 1e-12 and abs(float(loss.detach()) - der['loss']) <= der['loss_b']
    _derived(dict(grad_x=lp.grad.transpose(0, 1).cpu().numpy(), grad_g=crit.transitions.grad.cpu().numpy()), der, 'module', 2.0)
    bad = tg.copy()
    bad[1, 2] = 0
    with pytest.raises(ValueError, match='repeat label'):
        crit(lp.detach(), torch.from_numpy(bad).cuda(), torch.tensor(lens), torch.from_numpy(tl))
    bad[1, 2] = A                                      # outside [0, A): never used as an index
    with pytest.raises(ValueError):
        crit(lp.detach(), torch.from_numpy(bad).cuda(), torch.tensor(lens), torch.from_numpy(tl))
    # a label past a transcript's length is padding, whatever it holds
    ok = tg.copy()
    ok[2, 5] = 99
    again = crit(lp.detach(), torch.from_numpy(ok).cuda(), torch.tensor(lens), torch.from_numpy(tl))
    assert float(again.detach()) == float(loss.detach())


@pytest.mark.parametrize('name', ['main', 'a29', 'a33', 'chunks'])
def test_viterbi_paths_and_scores(name):
    from wav2letter_pytorch_amd.asg import viterbi_paths
    x, g, _, lens, _ = _case(name)
    T = x.shape[1]
    refs = [R.viterbi(x[n, :tn].astype(np.float64), g.astype(np.float64)) for n, tn in enumerate(lens)]
    zero = [R.viterbi(x[n, :tn].astype(np.float64), np.zeros_like(g, dtype=np.float64)) for n, tn in enumerate(lens)]
    # the test cannot hide behind ties: every decision on the reference paths is clear of fp32 rounding
    for _, _, margin in refs + zero:
        assert margin > 1e-3, margin
    xd = torch.from_numpy(x).cuda()
    sizes = torch.tensor(lens, dtype=torch.int32)
    path, score = viterbi_paths(xd, torch.from_numpy(g).cuda(), sizes)
    path0, _ = viterbi_paths(xd, None, sizes)
    path, score, path0 = path.cpu().numpy(), score.cpu().numpy(), path0.cpu().numpy()
    assert path.dtype == np.int32 and path.shape == (len(lens), T)
    for n, tn in enumerate(lens):
        assert path[n, :tn].tolist() == refs[n][0], n
        assert abs(score[n] - refs[n][1]) <= 1e-5 * max(1.0, abs(refs[n][1])), n
        assert (path[n, tn:] == -1).all() and (path0[n, tn:] == -1).all()
        assert path0[n, :tn].tolist() == np.argmax(x[n, :tn], axis=1).tolist() == zero[n][0]
    assert torch.equal(torch.from_numpy(path0[:, :min(lens)]), torch.argmax(xd, dim=2)[:, :min(lens)].cpu().to(torch.int32))


def test_viterbi_long_utterance_walks_several_back_pointer_chunks():
    """T = 1100 > 2 x 512: the back-trace stages three chunks of back-pointers"""
    from wav2letter_pytorch_amd.asg import viterbi_paths
    x, g, _, lens, _ = _case('spt2')
    ref = R.viterbi(x[0].astype(np.float64), g.astype(np.float64))
    path, score = viterbi_paths(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda())
    got = path[0].cpu().numpy().tolist()
    if ref[2] > 1e-3:
        assert got == ref[0]
    # whatever rounding decides at a near-tie, the path's own float64 score is the optimum
    assert abs(R.path_score(x[0].astype(np.float64), g.astype(np.float64), got) - ref[1]) < 1e-2
    assert abs(float(score[0]) - ref[1]) < 1e-4 * abs(ref[1])


def test_decoder_spells_hello_through_a_repeat_label():
    from wav2letter_pytorch_amd.asg import ASGDecoder
    dec = ASGDecoder(list(ENGLISH))
    frames = 'hheelll__oo  wwoorrld'                   # "hel_o world" with labels held; '_' repeats the l
    post = np.full((2, len(frames) + 3, len(ENGLISH)), -8.0, dtype=np.float32)
    for t, c in enumerate(frames):
        post[0, t, ENGLISH.index(c)] = -0.01
    post[0, len(frames):, ENGLISH.index('q')] = 0.0    # frames past the utterance's size: ignored
    post[1, :, ENGLISH.index('a')] = -0.01             # "a" for every frame
    post[1, 0, ENGLISH.index('_')] = 0.0               # ... after a leading repeat label, which is dropped
    sizes = torch.tensor([len(frames), 5], dtype=torch.int32)
    out = torch.from_numpy(post).cuda()
    assert dec.decode(out, sizes) == ['hello world', 'a']
    strings, offsets = dec.decode(out, sizes, return_offsets=True)
    assert strings == ['hello world', 'a']
    assert offsets[0][0].tolist() == [0, 2, 4, 7, 9, 11, 13, 15, 17, 19, 20] and offsets[1][0].tolist() == [1]
    assert offsets[0][0].dtype == torch.int32
    assert dec.decode(out[0], sizes[:1]) == ['hello world']                       # 2-D input: one utterance
    # transitions that make entering any label but 'h' prohibitive keep the path there: the decoder really uses them
    g = torch.full((len(ENGLISH), len(ENGLISH)), -1000.0)
    g[:, ENGLISH.index('h')] = 0.0
    assert dec.decode(out[:1], sizes[:1], transitions=g.cuda()) == ['h']
    assert dec.cer('hello', 'hallo') == 1              # the helpers of decoder.Decoder are inherited


def _train(tmp_path, steps=30):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from asg_replay_worker import build_model, synthetic_batch
    from wav2letter_pytorch_amd.trainer import Trainer
    model = build_model()
    batch = synthetic_batch(model.labels)
    trainer = Trainer(default_root_dir=str(tmp_path), max_epochs=1, max_steps=steps, log_every_n_steps=1)
    trainer.fit(model, [batch] * steps)
    return model, trainer, batch


def test_end_to_end_training_checkpoint_transcribe_and_evaluation(tmp_path):
    from asg_replay_worker import build_model
    from wav2letter_pytorch_amd.asg import ASGLoss
    from wav2letter_pytorch_amd.evaluate import evaluate
    model, trainer, batch = _train(tmp_path)
    assert isinstance(model.criterion, ASGLoss)
    losses = [logs['train_loss'] for _, logs in trainer.logged]
    assert len(losses) == 30 and all(np.isfinite(losses))
    print(f'ASG end to end: loss step 1 {losses[0]:.4f}, step 30 {losses[-1]:.4f}')
    assert losses[-1] < losses[0]
    assert all(k in trainer.logged[-1][1] for k in ('train_cer', 'train_wer', 'train_len_ratio'))
    g = model.criterion.transitions.detach()
    assert g.is_cuda and bool(g.abs().max() > 0) and bool(torch.isfinite(g).all())
    # FusedSGD updates it through its one-launch small-parameter path
    opt = model.optimizers()
    tables = opt.__dict__.get('_w2l_small_tables', {})
    assert any(row[0] == g.data_ptr() for key in tables for row in key)
    # the checkpoint carries criterion.transitions and restores it
    ck = torch.load(os.path.join(str(tmp_path), 'epoch=0-step=30.ckpt'), map_location='cpu')
    assert torch.equal(ck['state_dict']['criterion.transitions'], g.cpu())
    fresh = build_model(seed=6).cuda()
    assert not fresh.criterion.transitions.detach().any()
    fresh.load_state_dict(ck['state_dict'])
    assert torch.equal(fresh.criterion.transitions.detach(), g)
    # transcribe and the evaluation loop of the test CLI, on the ASG decoder and infer()
    wave = (0.1 * np.random.default_rng(3).standard_normal(8000)).astype(np.float32)
    hyps = model.transcribe([wave, wave[:6000]])
    assert len(hyps) == 2 and all(isinstance(h, str) for h in hyps)
    metrics, records = evaluate(model, [batch])
    assert len(records) == 4 and all(np.isfinite(metrics[k]) for k in ('test_loss', 'test_cer', 'test_wer'))
    # what is out of scope fails loudly
    from wav2letter_pytorch_amd.decoder import GreedyDecoder
    with pytest.raises(NotImplementedError):
        model.transcribe([wave], word_times=True)
    with pytest.raises(NotImplementedError):
        model.transcribe([wave], decoder=GreedyDecoder(model.labels))
    with pytest.raises(NotImplementedError):
        evaluate(model, [batch], word_times=True)


def test_beam_search_decoder_and_too_many_labels_fail_loudly():
    from asg_replay_worker import build_model
    from wav2letter_pytorch_amd.asg import ASGLoss, viterbi_paths
    from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder
    from wav2letter_pytorch_amd.evaluate import decode_batch
    model = build_model().cuda().eval()
    out = torch.zeros(1, 6, 29, device='cuda')
    beam = GPUPrefixBeamSearchDecoder(labels=model.labels, lm_path=None, k=3, alpha=0.3, beta=5, prune=1e-3, log_probs=True)
    with pytest.raises(NotImplementedError, match='beam search'):
        decode_batch(model, beam, out, torch.tensor([6]))
    with pytest.raises(ValueError):
        ASGLoss(65)
    with pytest.raises(ValueError, match='out of range'):
        viterbi_paths(torch.zeros(1, 4, 65, device='cuda'))
    crit = ASGLoss(64)
    crit.num_labels = 65                               # a module whose label count outgrew the kernels
    crit.transitions = torch.nn.Parameter(torch.zeros(65, 65))
    with pytest.raises(ValueError, match='out of range'):
        crit.cuda()(torch.zeros(4, 1, 65, device='cuda'), torch.ones(1, 2, dtype=torch.int32), torch.tensor([4]),
                    torch.tensor([2]))


def _worker(tmp_path, tag, env_extra):
    out = str(tmp_path / f'{tag}.npz')
    env = dict(os.environ)
    env.pop('W2L_REPLAY', None)
    env.update(env_extra)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'asg_replay_worker.py'), out, '6'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith('ASG_WORKER ')][-1]
    return dict(np.load(out)), json.loads(line[len('ASG_WORKER '):])


def test_replayed_run_equals_the_eager_run_bit_for_bit(tmp_path):
    """six steps with recorded launch lists on (the default) and with W2L_REPLAY=0, each in a fresh process: the same
    parameters bit for bit, criterion.transitions included"""
    p_replay, info_replay = _worker(tmp_path, 'replay', {'W2L_REPLAY_WARM': '1'})
    p_eager, info_eager = _worker(tmp_path, 'eager', {'W2L_REPLAY': '0'})
    print('ASG replay run:', info_replay['stats'])
    assert info_replay['replay'] is True and info_eager['replay'] is False
    # the replayed run really was recorded and replayed (nothing poisoned, no silent fall back to eager)
    st = info_replay['stats']
    assert st['poisoned'] == [], st
    assert st['recorded'] > 0 and st['replayed_F'] > 0 and st['replayed_B'] > 0, st
    assert info_eager['stats']['recorded'] == 0 and info_eager['stats']['replayed_F'] == 0
    assert info_replay['losses'] == info_eager['losses']
    assert set(p_replay) == set(p_eager) and 'criterion.transitions' in p_replay
    assert p_replay['criterion.transitions'].any()
    for k in p_eager:
        assert np.array_equal(p_replay[k], p_eager[k]), k

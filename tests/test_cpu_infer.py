"""Host-side statements of the inference path (no GPU): the fused epilogue's row map against torch's padding, the BatchNorm
fold against the oracle, the ``test`` command line's configuration, corpus-level CER / WER, the public signatures."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from wav2letter_pytorch_amd import defaults
from wav2letter_pytorch_amd.engine import bnact_rows, bnact_zero_rows, fold_bn


def _model_pads():
    """every (pad_l, pad_r) the two model tables produce for a consumer"""
    from wav2letter_pytorch_amd.wav2letter import same_pad_amounts
    pads = set()
    cin = 64
    for c, k, s, d, _ in defaults.W2L_LAYERS:
        _, l, r = same_pad_amounts(cin, k, s, d)
        pads.add((l, r))
        cin = c
    for blocks in (defaults.JASPER_BLOCKS, [(b['layer_size'], b['kernel_size'], b['stride'], 0, 0, b.get('dilation', 1))
                                            for b in defaults.jasper10x5_model().jasper_blocks]):
        for b in blocks:
            k, d = b[1], (b[5] if len(b) > 5 else 1)
            k = k + 1 if k % 2 == 0 else k                       # even kernels are bumped to odd (jasper.py:53-58)
            p = d * (k - 1) // 2
            pads.add((p, p))
    return sorted(pads)


@pytest.mark.parametrize('reflect', [True, False])
def test_row_map_equals_torch_padding(reflect):
    pads = _model_pads()
    assert (4, 5) in pads and max(max(p) for p in pads) >= 28
    for pl, pr in pads:
        for T in list(range(max(pl, pr) + 1, 300, 7)) + [max(pl, pr) + 1, max(pl, pr) + 2, 299]:
            frames = torch.arange(1, T + 1, dtype=torch.float32).view(1, 1, T)
            want = F.pad(frames, (pl, pr), mode='reflect' if reflect else 'constant').view(-1)
            got = torch.full((pl + T + pr,), -1.0)
            written = np.zeros(pl + T + pr, dtype=int)
            for t in range(T):
                for r in bnact_rows(t, T, pl, pr, reflect):
                    got[r] = frames[0, 0, t]
                    written[r] += 1
            if not reflect:
                for r in bnact_zero_rows(T, pl, pr):
                    got[r] = 0.0
                    written[r] += 1
            assert (written == 1).all(), (pl, pr, T)             # every row written exactly once: no race, no gap
            assert torch.equal(got, want), (pl, pr, T)


def test_fold_equals_batch_norm_eval():
    from oracle import w2l_oracle as O                           # noqa: F401  (the oracle's BatchNorm is F.batch_norm)
    g = torch.Generator().manual_seed(0)
    y = torch.randn(3, 96, 50, generator=g) * 3
    gamma, beta = 1 + 0.3 * torch.randn(96, generator=g), torch.randn(96, generator=g)
    mean, var = torch.randn(96, generator=g), 0.2 + torch.rand(96, generator=g)
    want = F.batch_norm(y, mean, var, gamma, beta, training=False, eps=1e-3)
    scale, shift = fold_bn(gamma, beta, mean, var, 1e-3)
    got = y * scale[None, :, None] + shift[None, :, None]
    assert float((got - want).abs().max() / want.abs().max()) < 1e-6


def test_build_config_cases():
    from wav2letter_pytorch_amd import test as T
    with pytest.raises(SystemExit, match='model_path'):
        T.build_config(['data.test_manifest=m.csv'])
    with pytest.raises(SystemExit, match='data.test_manifest'):
        T.build_config(['model_path=a.ckpt'])
    base = ['model_path=a.ckpt', 'data.test_manifest=m.csv']
    cfg = T.build_config(base)
    assert cfg.decoder == 'greedy' and T.decoder_spec(cfg, True)[0] == 'GreedyDecoder'
    cfg = T.build_config(base + ['decoder=beam', 'beam.k=7', 'beam.beta=2', 'model=jasper', 'model.mid_layers=3'])
    name, kw = T.decoder_spec(cfg, False)
    assert name == 'GPUPrefixBeamSearchDecoder' and kw['k'] == 7 and kw['beta'] == 2.0 and kw['log_probs'] is False
    assert cfg.model.name == 'jasper' and cfg.model.mid_layers == 3
    cfg = T.build_config(base + ['decoder=beam_lm', 'lm_path=lm.arpa', 'beam.alpha=0.7', 'beam.prune=1e-4', 'print_all=true',
                                 'word_times=true', 'output=o.jsonl'])
    name, kw = T.decoder_spec(cfg, True)
    assert name == 'GPUPrefixBeamSearchLMDecoder' and kw['lm_path'] == 'lm.arpa' and kw['alpha'] == 0.7 and kw['prune'] == 1e-4
    assert cfg.print_all and cfg.word_times and cfg.output == 'o.jsonl'
    for bad in (['lm_path=lm.arpa'], ['lm_path=lm.arpa', 'decoder=beam'], ['decoder=beam_lm'], ['decoder=viterbi'],
                ['beam.width=3']):
        with pytest.raises(SystemExit):
            T.build_config(base + bad)


def test_corpus_level_metrics():
    from wav2letter_pytorch_amd.decoder import Decoder
    from wav2letter_pytorch_amd.evaluate import corpus_metrics
    dec = Decoder(['_', 'a', 'b', 'c', ' '])
    pairs = [('ab c', 'ab c'), ('abc abc abc', 'abc abd'), ('a', 'b b')]
    m = corpus_metrics(dec, pairs)
    # characters without spaces: 0 / 3, 4 / 9 (one substitution, three deletions), 2 / 1 -> 6 / 13; words: 0 / 2, 2 / 3, 2 / 1
    assert m['test_cer'] == 6 / 13 and m['test_wer'] == 4 / 6
    assert m['test_len_ratio'] == (4 + 7 + 3) / (4 + 11 + 1)
    per_utt_mean = np.mean([0 / 3, 4 / 9, 2 / 1])
    assert abs(m['test_cer'] - per_utt_mean) > 0.1               # corpus level, not a mean of ratios


def test_public_signatures():
    from wav2letter_pytorch_amd.base_asr_models import ConvCTCASR
    from wav2letter_pytorch_amd.trainer import Trainer
    assert list(inspect.signature(Trainer.test).parameters) == ['self', 'model', 'dataloader', 'ckpt_path']
    assert inspect.signature(Trainer.test).parameters['ckpt_path'].default is None
    assert list(inspect.signature(ConvCTCASR.test_step).parameters)[:3] == ['self', 'batch', 'batch_idx']
    tr = inspect.signature(ConvCTCASR.transcribe).parameters
    assert list(tr) == ['self', 'paths_or_waveforms', 'batch_size', 'decoder', 'word_times']
    assert tr['decoder'].default is None and tr['word_times'].default is False
    from wav2letter_pytorch_amd import Jasper, Wav2Letter
    assert callable(Wav2Letter.infer) and callable(Jasper.infer)

"""Command-line evaluation of a checkpoint, the ``test.py`` the reference's README promises (README.md:46-56) and never
shipped:

    python -m wav2letter_pytorch_amd.test [--config-dir /path/to/configuration] model_path=run/epoch=4-step=900.ckpt \\
           data.test_manifest=test.csv [model=jasper] [model.mid_layers=20] [decoder=greedy|beam|beam_lm|asg_beam|asg_beam_lm] [lm_path=lm.arpa] \\
           [beam.k=5] [beam.alpha=0.3] [beam.beta=5] [beam.prune=1e-3] [print_samples=K | print_all=true] \\
           [lexicon_path=words.txt | lexicon_from_lm=true] [hotwords_path=words.txt [hotword_weight=1.0]] \\
           [output=hyps.jsonl] [word_times=true] [data.resample=true] [mbr=word|char [mbr_scale=1.0]] [error_counts=true]

``train.py``'s override syntax and config tree.  The forward pass is ``model.infer`` (one fused launch per convolution);
``test_loss``, corpus-level ``test_cer`` / ``test_wer`` and ``test_len_ratio`` are printed and returned.  ``output=`` writes one
JSON line per utterance: path, text, hypothesis, character and word errors (and each word's start / end seconds with
``word_times=true``, by forced alignment of the hypothesis).  ``decoder=asg_beam|asg_beam_lm`` are the beam searches of a model
trained with ``model.criterion=asg`` (asg_beam.py), bound to the checkpoint's learned transitions.  ``lexicon_path=`` (a word
list, one word per line; ``decoder=beam|beam_lm``) or ``lexicon_from_lm=true`` (the model's vocabulary; ``decoder=beam_lm``)
constrains the beam search to strings of lexicon words (lexicon.py).  ``hotwords_path=`` (a word list, one single word per
line; ``decoder=beam|beam_lm``) makes the beam search prefer those words by ``hotword_weight=`` natural-log units per matched
character (default 1.0: a convention, not a tuned value) without forbidding anything else.  The ASG beam searches have both
(``lexicon=`` / ``hotwords=`` of asg_beam.ASGBeamSearchDecoder / ASGBeamSearchLMDecoder), but this command does not take the
keys with ``decoder=asg_beam|asg_beam_lm`` yet: it refuses them.  ``mbr=word|char`` (any of the four beam decoders) returns the
hypothesis of the least expected word / character error over the search's own n-best list instead of its best-weighted one
(mbr.py; ``mbr_scale=`` scales the log weights in the posterior, default 1.0: a convention, not a tuned value).
``error_counts=true`` splits the errors into substitutions, deletions and insertions, per record (``word_sub`` ... ``char_ins``)
and over the set (``test_word_sub`` ... ``test_char_ins``, each divided by the summed reference length)."""
from __future__ import annotations

import json
import math
import sys

from .train import build_config as _train_config

DECODERS = ('greedy', 'beam', 'beam_lm', 'asg_beam', 'asg_beam_lm')
LM_DECODERS = ('beam_lm', 'asg_beam_lm')
ASG_DECODERS = ('asg_beam', 'asg_beam_lm')
LEXICON_DECODERS = ('beam', 'beam_lm')
BEAM_DEFAULTS = dict(k=5, alpha=0.3, beta=5, prune=1e-3)
MBR_UNITS = ('word', 'char')


def _truth(v) -> bool:
    return v is True or (isinstance(v, str) and v.lower() in ('1', 'true', 'yes'))


def build_config(argv):
    """the config tree of ``train.build_config`` plus the evaluation keys, checked: ``model_path`` and
    ``data.test_manifest`` are required (SystemExit naming the key), ``decoder`` is one of greedy / beam / beam_lm /
    asg_beam / asg_beam_lm (the last two only with ``model.criterion=asg``), ``lm_path`` belongs to ``decoder=beam_lm`` and
    ``decoder=asg_beam_lm`` only (and those decoders need it), ``lexicon_path`` to ``decoder=beam|beam_lm`` and
    ``lexicon_from_lm`` to ``decoder=beam_lm`` (one of the two at most), ``hotwords_path`` to ``decoder=beam|beam_lm`` and
    ``hotword_weight`` (a finite number) to ``hotwords_path``."""
    cfg = _train_config(argv)
    if cfg.get('model_path') in (None, '???', ''):
        raise SystemExit('model_path is required (e.g. model_path=/path/to/epoch=0-step=100.ckpt)')
    if cfg.data.get('test_manifest') in (None, '???', ''):
        raise SystemExit('data.test_manifest is required (e.g. data.test_manifest=/path/to/manifest.csv)')
    cfg.setdefault('decoder', 'greedy')
    if cfg.decoder not in DECODERS:
        raise SystemExit(f'decoder={cfg.decoder!r} is not one of {", ".join(DECODERS)}')
    lm = cfg.get('lm_path')
    if lm and cfg.decoder not in LM_DECODERS:
        raise SystemExit(f'lm_path is given but decoder={cfg.decoder}: a language model needs decoder=beam_lm '
                         '(or asg_beam_lm under model.criterion=asg)')
    if cfg.decoder in LM_DECODERS and not lm:
        raise SystemExit(f'decoder={cfg.decoder} needs lm_path=/path/to/model.arpa')
    cfg['lexicon_from_lm'] = _truth(cfg.get('lexicon_from_lm', False))
    cfg.setdefault('lexicon_path', None)
    for key in ('lexicon_path', 'lexicon_from_lm'):
        if not cfg[key]:
            continue
        if cfg.decoder in ASG_DECODERS:
            raise SystemExit(f'{key} is given but decoder={cfg.decoder}: the lexicon constraint is not built for ASG beam '
                             'search in this command (ASGBeamSearchDecoder / ASGBeamSearchLMDecoder take lexicon=; '
                             'decoder=beam|beam_lm have the key)')
        if cfg.decoder not in LEXICON_DECODERS:
            raise SystemExit(f'{key} is given but decoder={cfg.decoder}: a lexicon constrains a beam search '
                             '(decoder=beam or decoder=beam_lm)')
    if cfg.lexicon_path and cfg.lexicon_from_lm:
        raise SystemExit('lexicon_path and lexicon_from_lm are both given: the search takes one lexicon')
    if cfg.lexicon_from_lm and cfg.decoder != 'beam_lm':
        raise SystemExit(f'lexicon_from_lm is given but decoder={cfg.decoder}: the vocabulary of a language model needs '
                         'decoder=beam_lm')
    cfg.setdefault('hotwords_path', None)
    cfg.setdefault('hotword_weight', None)
    for key in ('hotwords_path', 'hotword_weight'):
        if cfg[key] in (None, ''):
            continue
        if cfg.decoder in ASG_DECODERS:
            raise SystemExit(f'{key} is given but decoder={cfg.decoder}: hotword boosting is not built for ASG beam search '
                             'in this command (ASGBeamSearchDecoder / ASGBeamSearchLMDecoder take hotwords=; '
                             'decoder=beam|beam_lm have the key)')
        if cfg.decoder not in LEXICON_DECODERS:
            raise SystemExit(f'{key} is given but decoder={cfg.decoder}: hotwords bias a beam search '
                             '(decoder=beam or decoder=beam_lm)')
    if cfg.hotword_weight not in (None, ''):
        if not cfg.hotwords_path:
            raise SystemExit('hotword_weight is given without hotwords_path=/path/to/words.txt')
        try:
            cfg['hotword_weight'] = float(cfg.hotword_weight)
        except (TypeError, ValueError):
            raise SystemExit(f'hotword_weight={cfg.hotword_weight!r} is not a number')
        if not math.isfinite(cfg.hotword_weight):
            raise SystemExit(f'hotword_weight={cfg.hotword_weight!r} is not finite')
    if cfg.decoder in ASG_DECODERS and cfg.model.get('criterion', 'ctc') != 'asg':
        raise SystemExit(f'decoder={cfg.decoder} decodes with learned transitions: it needs model.criterion=asg')
    cfg.setdefault('mbr', None)
    cfg.setdefault('mbr_scale', None)
    if cfg.mbr == '':
        cfg['mbr'] = None
    if cfg.mbr is not None:
        if cfg.decoder == 'greedy':
            raise SystemExit('mbr is given but decoder=greedy: minimum-Bayes-risk selection needs the n-best list of a beam '
                             'search (decoder=beam, beam_lm, asg_beam or asg_beam_lm)')
        if cfg.mbr not in MBR_UNITS:
            raise SystemExit(f'mbr={cfg.mbr!r} is not one of {", ".join(MBR_UNITS)}')
    if cfg.mbr_scale not in (None, ''):
        if cfg.mbr is None:
            raise SystemExit('mbr_scale is given without mbr=word|char')
        try:
            cfg['mbr_scale'] = float(cfg.mbr_scale)
        except (TypeError, ValueError):
            raise SystemExit(f'mbr_scale={cfg.mbr_scale!r} is not a number')
        if not math.isfinite(cfg.mbr_scale) or cfg.mbr_scale < 0:
            raise SystemExit(f'mbr_scale={cfg.mbr_scale!r} is not a finite number >= 0')
    cfg['error_counts'] = _truth(cfg.get('error_counts', False))
    beam = dict(BEAM_DEFAULTS)
    beam.update(cfg.get('beam') or {})
    unknown = sorted(set(beam) - set(BEAM_DEFAULTS))
    if unknown:
        raise SystemExit(f'unknown beam option(s) {unknown}: beam.k, beam.alpha, beam.beta, beam.prune')
    cfg['beam'] = type(cfg)(beam)
    cfg['print_samples'] = int(cfg.get('print_samples') or 0)
    cfg['print_all'] = _truth(cfg.get('print_all', False))
    cfg['word_times'] = _truth(cfg.get('word_times', False))
    if cfg.model.get('criterion', 'ctc') == 'asg':
        # decoder=beam|beam_lm and the CLI's word times implement CTC's blank / collapse rules and know no transitions
        if cfg.decoder in ('beam', 'beam_lm'):
            raise NotImplementedError(f'decoder={cfg.decoder} under model.criterion=asg: the CTC beam search knows no '
                                      f'transitions; use decoder=asg_{cfg.decoder} (or decoder=greedy: Viterbi decoding)')
        if cfg.word_times:
            raise NotImplementedError('word_times=true under model.criterion=asg is not wired into the command line: forced '
                                      'alignment under ASG is ASGDecoder.align (asg_beam.asg_forced_align)')
    cfg.setdefault('output', None)
    return cfg


def decoder_spec(cfg, log_probs: bool):
    """(class name, constructor keywords) of the decoder the config selects -- no device needed to form it"""
    labels = cfg.model.labels
    if cfg.decoder == 'greedy':
        return 'GreedyDecoder', dict(labels=labels)
    mbr = {}
    if cfg.get('mbr'):                         # (the keys are absent without mbr=: the decoders' defaults)
        mbr['mbr'] = cfg.mbr
        if cfg.get('mbr_scale') not in (None, ''):
            mbr['mbr_scale'] = float(cfg.mbr_scale)
    if cfg.decoder in ASG_DECODERS:            # (``transitions`` is bound by main(), to the model's criterion)
        kw = dict(labels=labels, k=int(cfg.beam.k), beta=float(cfg.beam.beta), prune=float(cfg.beam.prune), **mbr)
        if cfg.decoder == 'asg_beam':
            return 'ASGBeamSearchDecoder', kw
        return 'ASGBeamSearchLMDecoder', dict(lm_path=cfg.lm_path, alpha=float(cfg.beam.alpha), **kw)
    kw = dict(labels=labels, k=int(cfg.beam.k), alpha=float(cfg.beam.alpha), beta=float(cfg.beam.beta),
              prune=float(cfg.beam.prune), log_probs=log_probs, **mbr)
    lexicon = 'lm' if cfg.get('lexicon_from_lm') else cfg.get('lexicon_path')
    if lexicon:                                # (the key is absent without a lexicon: the decoders' defaults)
        kw['lexicon'] = lexicon
    if cfg.get('hotwords_path'):               # (likewise absent without hotwords)
        kw['hotwords'] = cfg.hotwords_path
        kw['hotword_weight'] = 1.0 if cfg.get('hotword_weight') in (None, '') else float(cfg.hotword_weight)
    if cfg.decoder == 'beam':
        return 'GPUPrefixBeamSearchDecoder', dict(lm_path=None, **kw)
    return 'GPUPrefixBeamSearchLMDecoder', dict(lm_path=cfg.lm_path, **kw)


def build_decoder(cfg, log_probs: bool, transitions=None):
    """``transitions``: the criterion of an ASG model (decoder=asg_beam|asg_beam_lm read its transitions at every call)"""
    from . import beam_search, decoder
    name, kw = decoder_spec(cfg, log_probs)
    if name.startswith('ASG'):
        from . import asg_beam
        return getattr(asg_beam, name)(transitions=transitions, **kw)
    return getattr(decoder if name == 'GreedyDecoder' else beam_search, name)(**kw)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    cfg = build_config(argv)
    import torch
    from .data import label_sets
    from .data.data_loader import BatchAudioDataLoader, SpectrogramDataset
    from .evaluate import evaluate
    from .train import name_to_model
    if type(cfg.model.labels) is str:
        cfg.model.labels = list(label_sets.labels_map[cfg.model.labels])
    if isinstance(cfg.model.get('decoder'), dict):
        cfg.model.decoder.labels = cfg.model.labels
    if not torch.cuda.is_available():
        raise RuntimeError('wav2letter_pytorch_amd runs on MI355X only (no CPU path)')
    torch.cuda.set_device(0)
    model = name_to_model[cfg.model.name](cfg.model).cuda()
    ck = torch.load(cfg.model_path, map_location='cpu')
    model.load_state_dict(ck['state_dict'] if 'state_dict' in ck else ck)
    from .engine import invalidate_packed
    invalidate_packed(model)
    ds = SpectrogramDataset(cfg.data.test_manifest, cfg.data.audio_conf, cfg.model.labels, mel_spec=cfg.data.mel_spec,
                            resample=_truth(cfg.data.get('resample', False)), wildcard=getattr(model, 'wildcard', None),
                            wildcard_ends=_truth(cfg.data.get('wildcard_ends', False)))
    loader = BatchAudioDataLoader(ds, batch_size=cfg.data.batch_size)
    if cfg.decoder in ASG_DECODERS:
        dec = build_decoder(cfg, True, transitions=model.criterion)
    elif cfg.model.get('criterion', 'ctc') == 'asg':
        dec = model.ctc_decoder              # decoder=greedy under asg: the model's Viterbi decoder, bound to its transitions
    else:
        dec = build_decoder(cfg, bool(getattr(model, 'infer_log_probs', True)))
    metrics, records = evaluate(model, loader, decoder=dec, word_times=cfg.word_times,
                                **({'error_counts': True} if cfg.error_counts else {}))
    shown = len(records) if cfg.print_all else min(cfg.print_samples, len(records))
    for r in records[:shown]:
        print(f'reference : {r["text"]}')
        print(f'hypothesis: {r["hypothesis"]}')
    if cfg.output:
        with open(cfg.output, 'w') as f:
            for r in records:
                f.write(json.dumps(r) + '\n')
    print('test ' + ' '.join(f'{k}={v:.6g}' for k, v in metrics.items()) + f' utterances={len(records)}', flush=True)
    return metrics, records


if __name__ == '__main__':
    main()

"""Command-line transcription of recordings of any length:

    python -m wav2letter_pytorch_amd.transcribe [--config-dir /path/to/configuration] model_path=run/epoch=4-step=900.ckpt \\
           audio=a.wav[,b.wav] [model=jasper] [model.mid_layers=20] \\
           [decoder=greedy|beam|beam_lm|asg_beam|asg_beam_lm] [lm_path=lm.arpa] [beam.k=5] [beam.alpha=0.3] [beam.beta=5] \\
           [beam.prune=1e-3] [lexicon_path=words.txt | lexicon_from_lm=true] [hotwords_path=words.txt [hotword_weight=1.0]] \\
           [segment.max_seconds=20] [segment.on_db=10] [segment.hyst_db=3] [segment.q=0.05] [segment.abs_min=1e-10] \\
           [segment.min_silence=0.3] [segment.min_speech=0.1] [segment.pad=0.2] [segment.on_dbfs=-40 [segment.off_dbfs=-43]] \\
           [word_times=true] [batch_size=8] [output=out.jsonl] [mbr=word|char [mbr_scale=1.0]]

``test.py``'s override syntax, config tree and decoder keys (the decoder is built by ``test.decoder_spec`` /
``test.build_decoder``).  Every file is cut at its pauses on the GPU and transcribed piece by piece
(``ConvCTCASR.transcribe_long``, segmentation.py); the text of each file is printed, ``output=`` writes one JSON line per file:
path, text and the segments with their start / end seconds (and each word's with ``word_times=true``)."""
from __future__ import annotations

import json
import sys

SEGMENT_KEYS = ('max_seconds', 'q', 'on_db', 'hyst_db', 'abs_min', 'min_silence', 'min_speech', 'pad', 'on_dbfs', 'off_dbfs')
_NO_MANIFEST = '<transcribe: no manifest>'


def build_config(argv):
    """the config tree of ``test.build_config`` (the same decoder keys and checks) plus: ``audio`` (required; one path or
    several separated by commas), ``segment.*`` (numbers; an unknown key is an error naming the known ones), ``batch_size``
    (a positive int, default 8).  ``data.test_manifest`` is not needed."""
    from . import test as T
    argv = list(argv)
    if not any(a.startswith('data.test_manifest=') for a in argv):
        argv.append(f'data.test_manifest={_NO_MANIFEST}')
    cfg = T.build_config(argv)
    audio = cfg.get('audio')
    if audio in (None, '???', ''):
        raise SystemExit('audio is required (e.g. audio=/path/to/a.wav or audio=a.wav,b.wav)')
    if isinstance(audio, str):
        audio = [a.strip() for a in audio.split(',') if a.strip()]
    cfg['audio'] = [str(a) for a in audio]
    if not cfg.audio:
        raise SystemExit('audio names no file')
    seg = dict(cfg.get('segment') or {})
    unknown = sorted(set(seg) - set(SEGMENT_KEYS))
    if unknown:
        raise SystemExit(f'unknown segment option(s) {unknown}: ' + ', '.join('segment.' + k for k in SEGMENT_KEYS))
    for k, v in seg.items():
        try:
            seg[k] = float(v)
        except (TypeError, ValueError):
            raise SystemExit(f'segment.{k}={v!r} is not a number')
    seg.setdefault('max_seconds', 20.0)
    cfg['segment'] = type(cfg)(seg)
    try:
        cfg['batch_size'] = 8 if cfg.get('batch_size') in (None, '') else int(cfg.get('batch_size'))
    except (TypeError, ValueError):
        raise SystemExit(f'batch_size={cfg.get("batch_size")!r} is not an integer')
    if cfg.batch_size < 1:
        raise SystemExit(f'batch_size={cfg.batch_size} must be at least 1')
    return cfg


def vad_config(cfg):
    """the segmentation.VadConfig of the ``segment.*`` keys at the model's frame rate (ValueError for numbers it refuses)"""
    from .segmentation import VadConfig
    kw = {k: v for k, v in cfg.segment.items() if k != 'max_seconds'}
    return VadConfig.for_model(cfg.model.audio_conf, **kw)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    cfg = build_config(argv)
    vad = vad_config(cfg)
    vad.numbers(cfg.segment.max_seconds)
    import torch
    from . import test as T
    from .data import label_sets
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
    if cfg.decoder in T.ASG_DECODERS:
        dec = T.build_decoder(cfg, True, transitions=model.criterion)
    elif cfg.model.get('criterion', 'ctc') == 'asg':
        dec = model.ctc_decoder
    else:
        dec = T.build_decoder(cfg, bool(getattr(model, 'infer_log_probs', True)))
    results = model.transcribe_long(cfg.audio, max_seconds=cfg.segment.max_seconds, batch_size=cfg.batch_size, decoder=dec,
                                    word_times=cfg.word_times, vad=vad)
    records = [dict(path=p, **r) for p, r in zip(cfg.audio, results)]
    for r in records:
        print(f'{r["path"]}: {r["text"]}', flush=True)
    if cfg.output:
        with open(cfg.output, 'w') as f:
            for r in records:
                f.write(json.dumps(r) + '\n')
    return records


if __name__ == '__main__':
    main()

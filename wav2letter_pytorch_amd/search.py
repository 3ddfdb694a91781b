"""Command-line keyword search in recordings of any length:

    python -m wav2letter_pytorch_amd.search [--config-dir /path/to/configuration] model_path=run/epoch=4-step=900.ckpt \\
           audio=a.wav[,b.wav] keywords=kw.txt [threshold=-1.0] [max_hits=8] [model=jasper] [model.mid_layers=20] \\
           [segment.max_seconds=20] [segment.on_db=10] ... [batch_size=8] [output=hits.jsonl]

``transcribe.py``'s override syntax, config tree and ``segment.*`` keys.  ``keywords``: a text file with one phrase per line
(empty lines are skipped).  Every file is cut at its pauses on the GPU and every piece's posteriors are searched
(``ConvCTCASR.find_keywords``, keyword_search.py).  ``threshold`` is in nats per character; -1.0 is a convention, not a tuned
value.  ``max_hits`` bounds the hits per phrase and piece.  Every hit is printed; ``output=`` writes one JSON line per file:
path and its hits ({'keyword', 'start', 'end', 'score'}, seconds on the recording's clock)."""
from __future__ import annotations

import json
import sys


def read_keywords(path):
    """one phrase per line, surrounding whitespace and empty lines dropped"""
    try:
        with open(path) as f:
            phrases = [line.strip() for line in f]
    except OSError as e:
        raise SystemExit(f'keywords={path}: {e}')
    phrases = [p for p in phrases if p]
    if not phrases:
        raise SystemExit(f'keywords={path} holds no phrase')
    return phrases


def build_config(argv):
    """the config tree of ``transcribe.build_config`` plus: ``keywords`` (required; the path of the phrase file), ``threshold``
    (a number, default -1.0), ``max_hits`` (1..64, default 8)"""
    from . import transcribe as TR
    from .keyword_search import MAX_HITS
    cfg = TR.build_config(argv)
    if cfg.get('keywords') in (None, '???', ''):
        raise SystemExit('keywords is required (e.g. keywords=/path/to/phrases.txt, one phrase per line)')
    try:
        cfg['threshold'] = -1.0 if cfg.get('threshold') in (None, '') else float(cfg.get('threshold'))
    except (TypeError, ValueError):
        raise SystemExit(f'threshold={cfg.get("threshold")!r} is not a number')
    if cfg.threshold != cfg.threshold:
        raise SystemExit('threshold is NaN')
    try:
        cfg['max_hits'] = 8 if cfg.get('max_hits') in (None, '') else int(cfg.get('max_hits'))
    except (TypeError, ValueError):
        raise SystemExit(f'max_hits={cfg.get("max_hits")!r} is not an integer')
    if not 1 <= cfg.max_hits <= MAX_HITS:
        raise SystemExit(f'max_hits={cfg.max_hits} must lie in 1..{MAX_HITS}')
    if cfg.model.get('criterion', 'ctc') == 'asg':
        raise SystemExit('model.criterion=asg: the keyword search is the CTC recurrence; it is not built for ASG')
    return cfg


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    cfg = build_config(argv)
    from . import transcribe as TR
    vad = TR.vad_config(cfg)
    vad.numbers(cfg.segment.max_seconds)
    phrases = read_keywords(str(cfg.keywords))
    import torch
    from .data import label_sets
    from .keyword_search import KeywordTable
    from .train import name_to_model
    if type(cfg.model.labels) is str:
        cfg.model.labels = list(label_sets.labels_map[cfg.model.labels])
    if isinstance(cfg.model.get('decoder'), dict):
        cfg.model.decoder.labels = cfg.model.labels
    try:
        table = KeywordTable(phrases, labels=list(cfg.model.labels), blank=0)
    except ValueError as e:
        raise SystemExit(f'keywords={cfg.keywords}: {e}')
    if not torch.cuda.is_available():
        raise RuntimeError('wav2letter_pytorch_amd runs on MI355X only (no CPU path)')
    torch.cuda.set_device(0)
    model = name_to_model[cfg.model.name](cfg.model).cuda()
    ck = torch.load(cfg.model_path, map_location='cpu')
    model.load_state_dict(ck['state_dict'] if 'state_dict' in ck else ck)
    from .engine import invalidate_packed
    invalidate_packed(model)
    results = model.find_keywords(cfg.audio, table, threshold=cfg.threshold, max_hits=cfg.max_hits,
                                  max_seconds=cfg.segment.max_seconds, batch_size=cfg.batch_size, vad=vad)
    records = [dict(path=p, hits=r) for p, r in zip(cfg.audio, results)]
    for r in records:
        for h in r['hits']:
            print(f'{r["path"]}: {h["start"]:.2f}-{h["end"]:.2f} s  {h["keyword"]!r}  {h["score"]:.3f}', flush=True)
    if cfg.output:
        with open(cfg.output, 'w') as f:
            for r in records:
                f.write(json.dumps(r) + '\n')
    return records


if __name__ == '__main__':
    main()

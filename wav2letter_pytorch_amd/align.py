"""Command-line alignment of one recording of any length to its whole transcript:

    python -m wav2letter_pytorch_amd.align [--config-dir /path/to/configuration] model_path=run/epoch=4-step=900.ckpt \\
           audio=a.wav text=a.txt [model=jasper] [model.mid_layers=20] [segment.max_seconds=20] [segment.on_db=10] ... \\
           [batch_size=8] [output=a.jsonl]

``transcribe.py``'s override syntax, config tree and ``segment.*`` keys.  ``audio``: ONE file.  ``text``: a text file, one
line or sentence per line (empty lines are skipped); every line becomes one segment.  The recording is cut at its pauses on the
GPU, the pieces' posteriors are concatenated and the whole text is aligned to them (``ConvCTCASR.align_transcript``,
alignment.ctc_forced_align_long).  Every segment is printed; ``output=`` writes one JSON line per segment ({'text', 'start',
'end', 'score', 'words': [{'word', 'start', 'end', 'score'}]}, seconds on the recording's clock; ``score``: mean log-posterior
per frame, what bad lines are filtered by)."""
from __future__ import annotations

import json
import sys


def read_lines(path):
    """one line per line, runs of whitespace collapsed, empty lines dropped"""
    try:
        with open(path) as f:
            lines = [' '.join(line.split()) for line in f]
    except OSError as e:
        raise SystemExit(f'text={path}: {e}')
    lines = [ln for ln in lines if ln]
    if not lines:
        raise SystemExit(f'text={path} holds no line')
    return lines


def build_config(argv):
    """the config tree of ``transcribe.build_config`` plus ``text`` (required; the path of the transcript); ``audio`` names one
    file"""
    from . import transcribe as TR
    cfg = TR.build_config(argv)
    if cfg.get('text') in (None, '???', ''):
        raise SystemExit('text is required (e.g. text=/path/to/a.txt, one line or sentence per line)')
    if len(cfg.audio) != 1:
        raise SystemExit(f'audio names {len(cfg.audio)} files: one transcript is aligned to one recording')
    if cfg.model.get('criterion', 'ctc') == 'asg':
        raise SystemExit('model.criterion=asg: the long alignment is the CTC recurrence; it is not built for ASG')
    return cfg


def segment_words(result):
    """the words of ``align_transcript``'s result dealt to its segments: segment i takes as many words as its text holds"""
    words, at, out = result['words'], 0, []
    for seg in result['segments']:
        n = len(seg['text'].split(' '))
        out.append(dict(seg, words=words[at: at + n]))
        at += n
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    cfg = build_config(argv)
    from . import transcribe as TR
    vad = TR.vad_config(cfg)
    vad.numbers(cfg.segment.max_seconds)
    lines = read_lines(str(cfg.text))
    import torch
    from .data import label_sets
    from .train import name_to_model
    if type(cfg.model.labels) is str:
        cfg.model.labels = list(label_sets.labels_map[cfg.model.labels])
    if isinstance(cfg.model.get('decoder'), dict):
        cfg.model.decoder.labels = cfg.model.labels
    known = set(cfg.model.labels)
    for i, line in enumerate(lines):
        for ch in line:
            if ch not in known:
                raise SystemExit(f'text={cfg.text}: character {ch!r} of line {i + 1} is not in the model\'s labels')
    if not torch.cuda.is_available():
        raise RuntimeError('wav2letter_pytorch_amd runs on MI355X only (no CPU path)')
    torch.cuda.set_device(0)
    model = name_to_model[cfg.model.name](cfg.model).cuda()
    ck = torch.load(cfg.model_path, map_location='cpu')
    model.load_state_dict(ck['state_dict'] if 'state_dict' in ck else ck)
    from .engine import invalidate_packed
    invalidate_packed(model)
    result = model.align_transcript(cfg.audio[0], lines, max_seconds=cfg.segment.max_seconds, batch_size=cfg.batch_size, vad=vad)
    records = segment_words(result)
    for r in records:
        print(f'{r["start"]:.2f}-{r["end"]:.2f} s  {r["score"]:.3f}  {r["text"]}', flush=True)
    if cfg.output:
        with open(cfg.output, 'w') as f:
            for r in records:
                f.write(json.dumps(r) + '\n')
    return records


if __name__ == '__main__':
    main()

"""Minimal config objects: attribute + .get access over dicts, lists stay lists
(``cfg.layers[:mid_layers]`` must slice).  Used when Hydra/OmegaConf are absent; an
OmegaConf DictConfig works with the models unchanged."""
from __future__ import annotations

import importlib
import os
import re
from typing import Any


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def to_cfg(o: Any):
    if isinstance(o, dict):
        return Cfg({k: to_cfg(v) for k, v in o.items()})
    if isinstance(o, (list, tuple)):
        return [to_cfg(v) for v in o]
    return o


CRITERIA = ('ctc', 'asg')


def criterion_name(model_cfg) -> str:
    """``model.criterion`` of a model config: ``ctc`` (the default, also when the key is absent) or ``asg`` (asg.ASGLoss, the
    criterion of the Wav2Letter paper); anything else is a ValueError naming the two"""
    name = model_cfg.get('criterion', None) if hasattr(model_cfg, 'get') else None
    name = 'ctc' if name is None else name
    if name not in CRITERIA:
        raise ValueError(f'model.criterion={name!r} is not a criterion: the valid values are ctc and asg')
    return name


def wildcard_options(model_cfg, labels=None):
    """``model.wildcard`` (the mark character of a transcript that stands for "speech without text here", e.g. ``'*'``; absent or
    empty: the feature is off) and ``model.wildcard_penalty`` (log-domain cost per wildcard frame, <= 0, default 0) ->
    (mark or None, penalty).  The mark is one character and none of the model's labels (ValueError); with
    ``model.criterion=asg`` it is a NotImplementedError: the wildcard is defined for CTC only."""
    get = model_cfg.get if hasattr(model_cfg, 'get') else (lambda k, d=None: d)
    mark = get('wildcard', None)
    if mark is None or mark == '':
        return None, 0.0
    mark = str(mark)
    if len(mark) != 1:
        raise ValueError(f'model.wildcard={mark!r}: the wildcard mark is one character')
    labels = get('labels', None) if labels is None else labels
    if labels is not None and not isinstance(labels, str) and mark in list(labels):
        raise ValueError(f'model.wildcard={mark!r} is one of the model\'s labels: choose a character the transcripts do not use')
    if criterion_name(model_cfg) == 'asg':
        raise NotImplementedError('model.wildcard with model.criterion=asg: the wildcard target is implemented for ctc only')
    penalty = float(get('wildcard_penalty', 0.0) or 0.0)
    if penalty > 0:
        raise ValueError(f'model.wildcard_penalty={penalty}: a log-domain cost per frame, it must be <= 0')
    return mark, penalty


def strip_wildcard(text: str, mark) -> str:
    """the transcript the string metrics score: the wildcard mark removed and whitespace collapsed.  What was spoken where the
    mark stands is unknown, so the hypothesis' words there count as insertions: CER and WER of such an utterance are upper
    bounds"""
    if not mark or mark not in text:
        return text
    return ' '.join(text.replace(mark, ' ').split())


SCHEDULER_INTERVALS = ('epoch', 'step')


def scheduler_interval(model_cfg) -> str:
    """``model.scheduler_interval``: ``epoch`` (the default, also when the key is absent: the scheduler steps once per epoch, as
    the reference runs it) or ``step`` (once per optimizer step: warm-up schedules, OneCycleLR); anything else is a ValueError"""
    name = model_cfg.get('scheduler_interval', None) if hasattr(model_cfg, 'get') else None
    name = 'epoch' if name is None else name
    if name not in SCHEDULER_INTERVALS:
        raise ValueError(f'model.scheduler_interval={name!r} is not an interval: the valid values are epoch and step')
    return name


def _flag(v) -> bool:
    return v is True or (isinstance(v, str) and v.lower() in ('1', 'true', 'yes'))


def bucket_options(data_cfg) -> dict:
    """The length-bucketing keys of ``data`` (data/bucketing.py) with their defaults, validated: ``bucket_rungs`` (0: off; K > 0:
    batches are padded to one of K widths), ``bucket_align`` (16: every width is a multiple of it), ``bucket_shuffle`` (true),
    ``bucket_seed`` (0), ``drop_last`` (false: the one short batch is kept).  A config tree without the keys means off."""
    get = data_cfg.get if hasattr(data_cfg, 'get') else (lambda k, d=None: d)
    rungs, align = get('bucket_rungs', 0), get('bucket_align', 16)
    for name, v, low in (('bucket_rungs', rungs, 0), ('bucket_align', align, 1)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < low):
            raise ValueError(f'data.{name}={v!r} is not an integer of at least {low}')
    seed = get('bucket_seed', 0)
    return dict(rungs=int(rungs or 0), align=int(align or 16), shuffle=_flag(get('bucket_shuffle', True)), seed=int(seed or 0),
                drop_last=_flag(get('drop_last', False)))


_ALIASES = {
    # reference module paths -> this package (config.yaml:14-16 names decoder.GreedyDecoder)
    'decoder': 'wav2letter_pytorch_amd.decoder',
    'novograd': 'wav2letter_pytorch_amd.novograd',
}


def instantiate(cfg, **kwargs):
    """hydra.utils.instantiate for the ``_target_`` nodes the reference uses
    (base_asr_models.py:22,74,75)."""
    try:
        from hydra.utils import instantiate as hydra_instantiate  # type: ignore
        from omegaconf import DictConfig  # type: ignore
        if isinstance(cfg, DictConfig):
            return hydra_instantiate(cfg, **kwargs)
    except ImportError:
        pass
    args = {k: v for k, v in dict(cfg).items() if k != '_target_'}
    args.update(kwargs)
    mod_name, attr = dict(cfg)['_target_'].rsplit('.', 1)
    try:
        mod = importlib.import_module(mod_name)
    except ImportError:
        if mod_name not in _ALIASES:
            raise
        mod = importlib.import_module(_ALIASES[mod_name])
    return getattr(mod, attr)(**args)


def _interpolate(node, root):
    pat = re.compile(r'\$\{([^}]+)\}')

    def lookup(path):
        cur = root
        for part in path.split('.'):
            cur = cur[part]
        return cur

    if isinstance(node, dict):
        for k, v in list(node.items()):
            node[k] = _interpolate(v, root)
        return node
    if isinstance(node, list):
        return [_interpolate(v, root) for v in node]
    if isinstance(node, str):
        m = pat.fullmatch(node)
        if m:
            return _interpolate(lookup(m.group(1)), root)
        return pat.sub(lambda mm: str(lookup(mm.group(1))), node)
    return node


_FLOAT_RE = re.compile(r'^[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$')


def override_value(key: str, text: str):
    """the value of a command-line override ``key=text``: YAML, except that ``model.wildcard`` is the text itself, less one pair
    of quotes (``model.wildcard='*'`` reaches the program as ``*`` from a shell, and a bare ``*`` or ``#`` is YAML syntax)"""
    if key == 'model.wildcard':
        if len(text) >= 2 and text[0] == text[-1] and text[0] in '\'"':
            text = text[1:-1]
        return text or None
    return _yaml_load(text)


def _yaml_load(text):
    """yaml.safe_load plus OmegaConf's number rule: `1e-5` (no dot) is a float, not a string
    (optimizer/exp_lr_optimizer.yaml:4 relies on it)."""
    import yaml

    def fix(node):
        if isinstance(node, dict):
            return {k: fix(v) for k, v in node.items()}
        if isinstance(node, list):
            return [fix(v) for v in node]
        if isinstance(node, str) and _FLOAT_RE.match(node) and not node.isdigit():
            return float(node)
        return node

    return fix(yaml.safe_load(text))


def load_config(config_dir: str, overrides=()):
    """Hydra-less loader for the reference's config tree (configuration/config.yaml:1-28):
    defaults list, ``# @package model`` groups, ``${a.b}`` interpolation, ``a.b=c`` overrides
    (``model=jasper`` style group overrides select the group file)."""
    with open(os.path.join(config_dir, 'config.yaml')) as f:
        root = _yaml_load(f.read())
    defaults = root.pop('defaults', [])
    groups = {}
    for d in defaults:
        (g, name), = d.items()
        groups[g] = name
    plain = []
    for ov in overrides:
        k, v = ov.split('=', 1)
        if k in groups and '.' not in k:
            groups[k] = v
        else:
            plain.append((k, v))
    merged = {}
    for g, name in groups.items():
        path = os.path.join(config_dir, g, name + '.yaml')
        with open(path) as f:
            text = f.read()
        node = _yaml_load(text) or {}
        m = re.search(r'#\s*@package\s+(\S+)', text)
        pkg = m.group(1) if m else g
        dst = merged.setdefault(pkg, {})
        _deep_update(dst, node)
    _deep_update(merged, root)
    for k, v in plain:
        cur = merged
        parts = k.split('.')
        for p in parts[:-1]:
            cur = cur.setdefault(p, {})
        cur[parts[-1]] = override_value(k, v)
    merged.pop('hydra', None)
    _interpolate(merged, merged)
    if isinstance(merged.get('model'), dict):
        criterion_name(merged['model'])          # validated only: an absent key stays absent (and means ctc)
        scheduler_interval(merged['model'])
    return to_cfg(merged)


def _deep_update(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _deep_update(dst[k], v)
        else:
            dst[k] = v

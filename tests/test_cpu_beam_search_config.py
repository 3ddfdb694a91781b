"""The device beam-search decoder is reachable the way configurations name decoders (``_target_: decoder.X``), and its
constructor refuses a language model.  Construction only: no device work."""
import importlib
import sys

import pytest

from wav2letter_pytorch_amd.config import instantiate, to_cfg
from wav2letter_pytorch_amd.data.label_sets import english_labels


def test_target_resolves_to_the_device_decoder():
    from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder
    cfg = to_cfg({'_target_': 'decoder.GPUPrefixBeamSearchDecoder', 'lm_path': None, 'labels': english_labels, 'k': 16,
                  'beta': 2, 'prune': 1e-4})
    if 'decoder' in sys.modules:                     # another test put dropin/ on the path: it must resolve there too
        assert sys.modules['decoder'].GPUPrefixBeamSearchDecoder is GPUPrefixBeamSearchDecoder
    dec = instantiate(cfg)
    assert type(dec) is GPUPrefixBeamSearchDecoder
    assert (dec.k, dec.beta, dec.prune, dec.log_probs, dec.blank_index) == (16, 2, 1e-4, False, 0)
    assert list(dec.labels) == list(english_labels)


def test_decoder_module_resolves_lazily():
    mod = importlib.import_module('wav2letter_pytorch_amd.decoder')
    from wav2letter_pytorch_amd import beam_search
    assert mod.GPUPrefixBeamSearchDecoder is beam_search.GPUPrefixBeamSearchDecoder
    assert mod.prefix_beam_search_gpu is beam_search.prefix_beam_search_gpu
    with pytest.raises(AttributeError):
        mod.NoSuchDecoder


def test_language_model_is_refused():
    from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder
    with pytest.raises(ValueError, match='PrefixBeamSearchLMDecoder'):
        GPUPrefixBeamSearchDecoder('model.arpa', english_labels, alpha=0.5)


def test_label_flags():
    from wav2letter_pytorch_amd.beam_search import _label_info
    info, end = _label_info(['_', 'a', ' ', 'a', '>', '|', '_'], 0, '>')
    assert end == 4
    assert [v & 0xff for v in info] == [0, 1, 2, 1, 4, 5, 0]
    assert [(v >> 8) & 1 for v in info] == [1, 0, 0, 0, 0, 0, 1]          # the blank's character
    assert [(v >> 9) & 1 for v in info] == [1, 1, 0, 1, 0, 0, 1]          # \w ('_' is a word character)
    assert [(v >> 10) & 1 for v in info] == [0, 0, 1, 0, 1, 1, 0]         # [\s|>]
    assert _label_info(['_', 'a'], 0, '>')[1] == -1
    with pytest.raises(ValueError):
        _label_info(['_', 'ab'], 0, '>')

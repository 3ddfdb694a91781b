"""Alias so `_target_: decoder.GreedyDecoder` (configuration/config.yaml:15) resolves to the MI355X decoder."""
from wav2letter_pytorch_amd.decoder import Decoder, GreedyDecoder  # noqa: F401
from wav2letter_pytorch_amd.beam_search import (GPUPrefixBeamSearchDecoder, GPUPrefixBeamSearchLMDecoder,  # noqa: F401,E402
                                                PrefixBeamSearchLMDecoder, get_time_per_word, prefix_beam_search,
                                                prefix_beam_search_gpu)
from wav2letter_pytorch_amd.alignment import ctc_forced_align, viterbi_align_host  # noqa: F401,E402

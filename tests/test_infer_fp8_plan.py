"""Host logic of the fused fp8 inference path: which copies (bf16, e4m3) of each activation ``infer`` writes
(engine.infer_copies), the launch budget that follows from it, and the new entry points' place in the ABI tables."""
import os
import re

import torch

from wav2letter_pytorch_amd import _lib
from wav2letter_pytorch_amd.engine import ConvSpec, UnitSpec, infer_copies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conv(cin, cout, k=3, stride=1):
    return ConvSpec(torch.zeros(cout, cin, k), None, k, stride, 1, k // 2, k // 2, 0)


def _chain(widths, strides=None, cin=64):
    units = []
    for i, c in enumerate(widths):
        units.append(UnitSpec(_conv(cin, c, stride=(strides or {}).get(i, 1)), src=i))
        cin = c
    return units


def test_wav2letter_shaped_stack_is_bytes_only_between_the_wide_units():
    # first convolution: 64 -> 256 with stride 2 (bf16 operands: the input has no e4m3 copy), then stride-1 wide units
    units = _chain([256, 256, 384, 1024], strides={0: 2})
    copies = infer_copies(units, True, True, 64)
    assert copies[0] == (True, False)                      # the spectrogram: bf16 only
    assert copies[1] == (False, True)                      # read by a stride-1 dense convolution alone: bytes only
    assert copies[2] == (False, True) and copies[3] == (False, True)
    assert copies[4] == (True, False)                      # the classifier reads bf16, nothing reads e4m3
    # not an fp8 engine: every activation bf16 only
    assert infer_copies(units, True, False, 64) == [(True, False)] * 5


def test_narrow_strided_and_depthwise_consumers_keep_bf16():
    units = _chain([256, 192, 256, 256, 256], strides={3: 2})
    units[4].dw = _conv(256, 256)                           # a separable unit: its depthwise kernel reads bf16
    copies = infer_copies(units, True, True, 64)
    assert copies[1] == (False, True)                      # 256 channels, read by a stride-1 dense convolution
    assert copies[2] == (True, False)                      # 192 channels: not a multiple of 128
    assert copies[3] == (True, False)                      # its only reader is strided
    assert copies[4] == (True, False)                      # its only reader is a depthwise kernel
    assert copies[5] == (True, False)


def test_residual_reader_counts_as_a_consumer():
    units = _chain([256, 256, 256])
    units[2].res = _conv(256, 256, k=1)
    units[2].res_src = 1                                   # activation 1 is read by unit 1 (dense) and by unit 2's 1x1 branch
    copies = infer_copies(units, True, True, 64)
    assert copies[1] == (False, True) and copies[2] == (False, True)
    units[2].res = _conv(256, 256, k=1, stride=2)          # a strided branch reads bf16: both copies then
    assert infer_copies(units, True, True, 64)[1] == (True, True)


def test_every_activation_has_a_copy_and_a_128_multiple_input_without_head():
    units = _chain([128, 128], cin=128)
    for head in (True, False):
        for c in infer_copies(units, head, True, 128):
            assert c[0] or c[1]
    assert infer_copies(units, True, True, 128)[0] == (True, False)       # the input never carries an e4m3 copy in infer()


def test_new_entry_points_are_declared_bound_and_named():
    hdr = open(os.path.join(ROOT, 'include', 'w2l_hip.h')).read()
    for name in ('w2l_conv1d_igemm_bnact_fp8', 'w2l_conv1d_igemm_bnact_fp8_tune'):
        assert re.search(r'\bint ' + name + r'\(', hdr), name
        assert name in _lib.SIGNATURES if hasattr(_lib, 'SIGNATURES') else hasattr(_lib.lib, name)
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.TRACE_NAMES['w2l_conv1d_igemm_bnact_fp8'] == 'conv_igemm_fp8_kernel/bnact'
    # the descriptor's layout did not change: the extra outputs travel as arguments
    assert [f[0] for f in _lib.BnActEpi._fields_] == ['scale', 'shift', 'res', 'res_lo', 'act', 'lens', 'out_hi', 'out_lo',
                                                      'out_rows', 'pad_l', 'pad_r', 'pad_mode']

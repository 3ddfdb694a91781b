"""CPU-only checks of the two records the backward pass is scheduled with: engine._WgradJob (one weight gradient: its
strides, row counts and pointers into the shared-halo dy buffer and the padded input) and engine._GradSource (the gradient
wrt one activation).  Every expected value is the formula of include/w2l_hip.h written out with the numbers of the case:

  dy   [halo zero rows][utt 0: Tout rows][halo zero rows][utt 1: Tout rows] ... [halo zero rows], CoutP elements per row
       -> utterance 0 starts halo rows in, utterances are (Tout + halo) * CoutP elements apart
  x    [N][pad_l + T + pad_r][CP]; the convolution's own padding is conv.pad_l of the buffer's pad_l rows
       -> it enters src.pad_l - conv.pad_l rows in, utterances are rows * CP elements apart, and N * rows minus that offset
          rows are left from there to the end of the buffer

Nothing is launched: data_ptr() of CPU tensors stands in for device addresses."""
import pytest
import torch

from wav2letter_pytorch_amd.engine import PAD_ZERO, Act, ConvSpec, _GradSource, _PackedW, _WgradJob


def _job(N, Tout, halo, cout, cin, coutp, cinp, kw, T, src_pad, conv_pad, f8=False):
    conv = ConvSpec(torch.zeros(cout, cin, kw), None, kw, 1, 1, conv_pad[0], conv_pad[1], PAD_ZERO)
    z = torch.zeros(1)
    pk = _PackedW(0, z, None, z, None, cinp, coutp)
    rows = src_pad[0] + T + src_pad[1]
    src = Act(torch.zeros(N, rows, cinp, dtype=torch.bfloat16), None, N, T, cin, cinp, src_pad[0], src_pad[1], PAD_ZERO,
              q=torch.zeros(N, rows, cinp, dtype=torch.uint8) if f8 else None)
    dy_rows = halo + N * (Tout + halo)
    dy_hi = torch.zeros(dy_rows, coutp, dtype=torch.bfloat16)
    pair = (torch.zeros(dy_rows, coutp, dtype=torch.uint8), torch.zeros(1)) if f8 else None
    return _WgradJob(conv, pk, dy_hi, None, halo, Tout, src, pair)


def test_wgrad_job_layout_terms():
    # N=2, Tout=5, halo=3, CoutP=CinP=64, Kw=3; the input has pad_l 4 against the convolution's 1, and 4 + 7 + 2 = 13 rows != T
    job = _job(2, 5, 3, 40, 48, 64, 64, 3, 7, (4, 2), (1, 1), f8=True)
    assert job.src.rows == 13 != job.src.T
    assert job.N == 2
    assert job.row_off == 4 - 1 == 3
    assert job.dy_bstride == (5 + 3) * 64
    assert job.x_bstride == 13 * 64
    assert job.x_rows_total == 2 * 13 - 3
    assert job.dw_shape == (3, 64, 64)
    assert job.flops == 2.0 * 2 * 5 * 40 * 48 * 3           # (of the logical problem: Cout x Cin of the parameter)
    for esize, dy, x in ((2, job.dy_hi, job.src.hi), (1, job.f8[0], job.src.q)):
        assert job.dy_ptr(dy, esize).value == dy.data_ptr() + 3 * 64 * esize
        assert job.x_ptr(x, esize).value == x.data_ptr() + 3 * 64 * esize
        # the last byte a kernel may touch from those pointers is inside the buffers
        assert 3 * 64 * esize + ((2 - 1) * job.dy_bstride + 5 * 64) * esize <= dy.numel() * dy.element_size()
        assert 3 * 64 * esize + job.x_rows_total * 64 * esize == x.numel() * x.element_size()
    held = job.held()
    assert [id(t) for t in held] == [id(t) for t in (job.dy_hi, job.src.hi, job.src.q, job.f8[0], job.f8[1])]
    assert (job.token, job.order, job.at) == (None, 0, None)


def test_wgrad_job_without_halo_and_offset():
    job = _job(2, 5, 0, 64, 64, 64, 64, 3, 5, (1, 1), (1, 1))
    assert job.src.rows == 7
    assert job.row_off == 0
    assert job.dy_bstride == 5 * 64
    assert job.x_bstride == 7 * 64
    assert job.x_rows_total == 2 * 7
    assert job.dw_shape == (3, 64, 64)
    assert job.flops == 2.0 * 2 * 5 * 64 * 64 * 3
    for esize in (1, 2):
        assert job.dy_ptr(job.dy_hi, esize).value == job.dy_hi.data_ptr()
        assert job.x_ptr(job.src.hi, esize).value == job.src.hi.data_ptr()
    assert [id(t) for t in job.held()] == [id(job.dy_hi), id(job.src.hi)]


def test_wgrad_job_halo_and_offset_are_not_confused():
    # halo 2 rows of 128 channels on the dy side, offset 5 rows of 64 channels on the input side: no two terms coincide
    job = _job(3, 6, 2, 128, 64, 128, 64, 2, 9, (6, 0), (1, 0))
    assert (job.row_off, job.src.rows) == (5, 15)
    assert job.dy_bstride == (6 + 2) * 128
    assert job.x_bstride == 15 * 64
    assert job.x_rows_total == 3 * 15 - 5
    assert job.dw_shape == (2, 128, 64)
    for esize in (1, 2):
        assert job.dy_ptr(job.dy_hi, esize).value == job.dy_hi.data_ptr() + 2 * 128 * esize
        assert job.x_ptr(job.src.hi, esize).value == job.src.hi.data_ptr() + 5 * 64 * esize


def test_wgrad_job_is_a_cheap_record_compared_by_identity():
    a = _job(2, 5, 3, 64, 64, 64, 64, 3, 7, (4, 2), (1, 1))
    b = _WgradJob(a.conv, a.pk, a.dy_hi, a.dy_lo, a.halo, a.Tout, a.src)
    assert not hasattr(a, '__dict__')                       # __slots__: no per-instance dict
    assert a != b and a == a                                # held-back jobs are told apart with ``is``
    a.token, a.order, a.at = 7, -1, 2                       # (what a held-back job is given later)
    with pytest.raises(AttributeError):
        a.no_such_field = 1


def test_grad_source_is_the_old_five_tuple():
    buf = torch.zeros(2, 9, 64)
    s = _GradSource(buf, 4, 2, PAD_ZERO, 9)
    g, pl, pr, mode, per = s[:5]
    assert g is buf and (pl, pr, mode, per) == (4, 2, PAD_ZERO, 9)
    assert s.partial is None and len(s) == 6
    g, pl, pr, mode, per, *rest = s
    assert g is buf and per == 9 and rest == [None]
    assert (s.buf, s.pad_l, s.pad_r, s.pad_mode, s.per) == (buf, 4, 2, PAD_ZERO, 9)
    partial = torch.zeros(1, 2, 64)
    assert _GradSource(buf, 4, 2, PAD_ZERO, 9, partial)[5] is partial

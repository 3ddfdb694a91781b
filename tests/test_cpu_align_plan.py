"""The alignment plan's host arithmetic, pinned.  tests/golden/align_plans.json was recorded by tools/record_align_plans.py from
the library as it was BEFORE csrc/align_core.h existed, when ctc_align.hip and asg_beam.hip each had a plan function of their
own.  The workspace queries are the plan's whole visible side: 0 = the moves live in LDS, N * bytes of one utterance's moves =
they live in the workspace (which gives away the block shape), -1 = no plan.  Rows: "ctc": [N, T, Smax, bytes], "asg":
[N, T, A, Smax, bytes]; the grid (both sides of every block-shape step and of every LDS-to-workspace switch) is described in
the recorder."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'align_plans.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_grid_is_the_one_the_plans_were_recorded_on(golden):
    """every N, T, Smax the grid must hold is there, for both criteria, and each plan with a switch has both of its sides"""
    steps = {'ctc': [0, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096],
             'asg': [0, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096]}
    for name, smaxes in steps.items():
        rows = golden[name]
        seen = {(r[0], r[1], r[-2]) for r in rows}
        for n in (1, 3):
            for smax in smaxes:
                for t in (1, 16, 17, 500, 32768, 32769):
                    assert (n, t, smax) in seen, (name, n, t, smax)
        by = {}
        for r in rows:
            if r[0] == 1 and 1 <= r[1] <= 32768 and r[-1] >= 0:
                by.setdefault(r[-2], {})[r[1]] = r[-1]
        for smax in smaxes[:-1]:
            switch = [t for t in by[smax] if by[smax][t] == 0 and by[smax].get(t + 1, 0) > 0]
            assert len(switch) == 1, (name, smax, switch)


def test_ctc_plans_unchanged(golden):
    from wav2letter_pytorch_amd._lib import lib
    for n, t, smax, want in golden['ctc']:
        assert lib.w2l_ctc_align_workspace_bytes(n, t, smax) == want, (n, t, smax)


def test_asg_plans_unchanged(golden):
    from wav2letter_pytorch_amd._lib import lib
    for n, t, a, smax, want in golden['asg']:
        assert lib.w2l_asg_align_workspace_bytes(n, t, a, smax) == want, (n, t, a, smax)

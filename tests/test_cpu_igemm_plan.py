"""The implicit-GEMM launcher's host arithmetic, pinned.  tests/golden/igemm_plans.json was recorded from the launcher as it
was BEFORE plan() existed (the values its launch `switch` was reached with, driven with dummy pointers, no GPU): configuration
index, K-loop structure, blocks per tile, stream-K blocks, grid blocks, block threads, LDS bytes, feasible -- for every
convolution shape of the default Wav2Letter and Jasper 10x5 configurations (forward and flat data gradient, N = 1 / 8 / 16 / 32
at 1000 frames, statistics flag 0..3, with the full split-K workspace, none, and the ticket page alone), edge shapes, every
forced index of three shapes, and lookups after w2l_tune_load.  w2l_conv_plan / w2l_conv_plan_fp8 run the very plan() every
launch goes through and must reproduce each record exactly.

The file is compact.  A plan is 0 (refused) or [index, row]: row into "rows", the table of the distinct [blocks per tile,
stream-K blocks, grid blocks, block threads, LDS bytes]; the K-loop structure is the index's (index % 52) // 26, 0 for e4m3.
  problems:    [N, Cin, Cout, Tout, Kw, stride, dil, w2l_conv_splitk_workspace_bytes, flag 0, flag 1, flag 2, flag 3, e4m3]
               -- per statistics flag one plan, or three where the workspace (full, none, 65536 bytes) changes it; e4m3: the
               plans of flags 0, 1, 3, or of flag 0 alone (stride taken as 1)
  sweeps:      [N, Cin, Cout, Tout, Kw, stride, dil, flag, ws_bytes, [row + 1 or 0 of forced index 0, 1, 2, ...]]
  fp8_sweeps:  [N, Cin, Cout, Tout, Kw, dil, flag, [row + 1 or 0 of forced index 0, 1, 2, ...]]
  plans:       [N, Cin, Cout, Tout, Kw, stride, dil, flag, ws_bytes, forced index, plan]
  sk_ranges:   {idx: [...], cases: [[N, Cin, Cout, Tout, Kw, stride, dil, ws_bytes, [w2l_conv_streamk_ranges per idx]]]}
  after_cache: plans (11 fields) and e4m3 plans ([N, Cin, Cout, Tout, Kw, dil, flag, forced index, plan]) taken after
               w2l_tune_load of the lines under the key cache"""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'igemm_plans.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _query(L, fn, *args):
    out = (C.c_int * 8)(*([7] * 8))
    rc = getattr(L.lib, fn)(*args, out)
    got = list(out)
    assert (rc == 0) == (got[7] == 1)
    if rc != 0:
        assert got == [-1, 0, 0, 0, 0, 0, 0, 0] and L.lib.w2l_last_error()
        return 0
    return got


def _plan(golden, ref, fp8, forced=None):
    """a stored plan as the query's out[8]"""
    if ref == 0:
        return 0
    idx, row = (forced, ref - 1) if forced is not None else ref
    return [idx, 0 if fp8 else (idx % (2 * golden['num_cfgs'])) // golden['num_cfgs'], *golden['rows'][row], 1]


def test_plans_match_the_recorded_launcher(golden):
    from wav2letter_pytorch_amd import _lib as L
    assert (golden['num_cfgs'], golden['num_splits'], golden['num_f8_cfgs']) == (26, 8, 15)
    n_plans = 0
    for rec in golden['problems']:
        pr, full, f8 = rec[:7], rec[7], rec[12]
        assert L.lib.w2l_conv_splitk_workspace_bytes(pr[0], pr[2], pr[3]) == full, rec
        for flag in range(4):
            per_ws = rec[8 + flag]
            per_ws = per_ws if per_ws != 0 and len(per_ws) == 3 else [per_ws] * 3
            for ws, ref in zip((full, 0, 65536), per_ws):
                assert _query(L, 'w2l_conv_plan', *pr, flag, ws, -1) == _plan(golden, ref, False), (rec, flag, ws)
                n_plans += 1
        for flag, ref in zip((0, 1, 3) if len(f8) == 3 else (0,), f8):
            assert _query(L, 'w2l_conv_plan_fp8', *pr[:5], pr[6], flag, -1) == _plan(golden, ref, True), (rec, flag)
    assert n_plans > 1500
    for rec in golden['sweeps']:
        assert len(rec[-1]) == 2 * 26 * 8 + 1 and rec[-1][-1] == 0                     # every index, and one past the end
        for idx, ref in enumerate(rec[-1]):
            assert _query(L, 'w2l_conv_plan', *rec[:9], idx) == _plan(golden, ref, False, idx), (rec[:9], idx)
    assert len({tuple(r[:7]) for r in golden['sweeps']}) == 3                          # three shapes
    for rec in golden['fp8_sweeps']:
        assert len(rec[-1]) == 15 + 1 and rec[-1][-1] == 0
        for idx, ref in enumerate(rec[-1]):
            assert _query(L, 'w2l_conv_plan_fp8', *rec[:7], idx) == _plan(golden, ref, True, idx), (rec[:7], idx)
    for rec in golden['plans']:
        assert _query(L, 'w2l_conv_plan', *rec[:10]) == _plan(golden, rec[10], False), rec
    for group in golden['sk_ranges']:
        for case in group['cases']:
            for idx, want in zip(group['idx'], case[8]):
                assert L.lib.w2l_conv_streamk_ranges(idx, *case[:8]) == want, (idx, case[:8])
    # the query leaves the per-thread hooks alone and needs none of them: a forced index is an argument
    assert _query(L, 'w2l_conv_plan', 8, 256, 256, 500, 11, 1, 1, 0, 0, 3)[0] == 3
    assert _query(L, 'w2l_conv_plan', 8, 256, 256, 500, 11, 1, 1, 4, 0, -1) == 0       # no such statistics flag
    assert _query(L, 'w2l_conv_plan_fp8', 8, 256, 256, 500, 11, 1, 2, -1) == 0         # the e4m3 kernel has no slot rows


def test_a_remembered_choice_wins_over_the_cost_model(golden, tmp_path):
    """shapes no other test measures or loads (N = 5; one flat stream-K shape): the records were taken after w2l_tune_load of
    the same lines, so the lookup -- and how a remembered split / stream-K choice degrades without its workspace -- is pinned"""
    from wav2letter_pytorch_amd import _lib as L
    path = tmp_path / 'tune.txt'
    path.write_text('\n'.join(golden['cache']) + '\n')
    assert L.lib.w2l_tune_load(str(path).encode()) == len(golden['cache']) - 1
    got = {}
    for rec in golden['after_cache']:
        fp8 = len(rec) == 9
        got[tuple(rec[:-1])] = _query(L, 'w2l_conv_plan_fp8' if fp8 else 'w2l_conv_plan', *rec[:-1])
        assert got[tuple(rec[:-1])] == _plan(golden, rec[-1], fp8), rec
    full = [v for k, v in got.items() if k[:8] == (5, 256, 256, 500, 11, 1, 1, 0) and k[9] == -1]
    assert [v[0] for v in full] == [142] * 3 and sorted(v[2] for v in full) == [1, 1, 3]
    assert any(len(k) == 10 and v != 0 and v[3] > 0 for k, v in got.items())          # a stream-K plan among them

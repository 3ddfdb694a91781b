"""The weight-gradient launcher's host arithmetic, pinned.  tests/golden/wgrad_plans.json was recorded from the launcher as it
was BEFORE plan() existed (what w2l_conv1d_wgrad_ws was about to launch, driven with dummy pointers, no GPU) by
tools/record_wgrad_plans.py, and recorded again, to the same bytes, from w2l_wgrad_launch_plan, which runs the very plan() every
launch goes through.  This test reproduces every record, and the answers of the kept queries beside it.

The file is compact.  A launch is a number: row + 1 into "rows", the table of the distinct launches (columns: "fields"); 0 =
refused; -1 = refused, and w2l_wgrad_needs_zero_x still says 1.
  problems, edges, after_cache:
      [N, Cin, Cout, Tout, Kw, stride, dil, w2l_wgrad_workspace_bytes, w2l_wgrad_dealt_workspace_bytes, w2l_wgrad_needs_zero,
       w2l_wgrad_plan, [w2l_wgrad_needs_zero_ws per workspace], [w2l_wgrad_group_tiles per "group_forms"],
       [launch per workspace], [the same under w2l_wgrad_deterministic(1)]]
      -- workspaces: none, 65536 bytes, the two sizes above, the larger of them.  problems: every convolution of the default
      Wav2Letter and Jasper 10x5 tables at N = 1 / 8 / 16 / 32 and 1000 frames; after_cache: taken after w2l_tune_load of "cache"
  sweeps: {shape, ws, per_order: for every order value 0..127 an index into refs, refs: [launch per "counts"]} -- forced through
      the query's arguments; where ws = 0 also, under the same plan pinned with w2l_wgrad_force_plan: needs_zero (one character
      of w2l_wgrad_needs_zero per order x count) and w2l_wgrad_plan of orders 1 and 33 per count"""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_plans.json')
NF = 24


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture()
def L():
    from wav2letter_pytorch_amd import _lib
    _lib.lib.w2l_wgrad_force_plan(0, -1)
    _lib.lib.w2l_wgrad_deterministic(0)
    yield _lib
    _lib.lib.w2l_wgrad_force_plan(0, -1)
    _lib.lib.w2l_wgrad_deterministic(0)


def _launch(L, golden, shape, ws, splits=0, order=-1):
    """the query's answer in the file's notation (without the needs_zero_x part of a refusal)"""
    out = (C.c_int * NF)(*([7] * NF))
    rc = L.lib.w2l_wgrad_launch_plan(*shape, ws, splits, order, out)
    got = list(out)
    assert (rc == 0) == (got[-1] == 1)
    if rc != 0:
        assert not any(got) and L.lib.w2l_last_error()
        return None
    return got[:-1]


def _expect(golden, ref):
    return golden['rows'][ref - 1] if ref > 0 else None


def _check_problem(L, golden, rec):
    shape, (n, cin, cout, tout, kw) = rec[:7], rec[:5]
    full, dealt, nz, plan, nz_ws, tiles, launches = rec[7], rec[8], rec[9], rec[10], rec[11], rec[12], rec[13:15]
    assert L.lib.w2l_wgrad_workspace_bytes(cin, cout, kw) == full and L.lib.w2l_wgrad_dealt_workspace_bytes(cin, cout, kw) == dealt
    assert L.lib.w2l_wgrad_needs_zero(n, cin, cout, tout, kw) == nz, rec
    assert L.lib.w2l_wgrad_plan(n, cin, cout, tout, kw) == plan, rec
    wss = [0, 65536, full, dealt, max(full, dealt)]
    assert [L.lib.w2l_wgrad_needs_zero_ws(n, cin, cout, tout, kw, ws) for ws in wss] == nz_ws, rec
    assert [L.lib.w2l_wgrad_group_tiles(cin, cout, kw, f) for f in golden['group_forms']] == tiles, rec
    count = 0
    for det in (0, 1):
        L.lib.w2l_wgrad_deterministic(det)
        for ws, ref in zip(wss, launches[det]):
            want = _expect(golden, ref)
            assert _launch(L, golden, shape, ws) == want, (rec, det, ws)
            nzx = want[golden['fields'].index('needs_zero')] if want is not None else -ref
            assert L.lib.w2l_wgrad_needs_zero_x(*shape, ws) == nzx, (rec, det, ws)
            count += 1
    L.lib.w2l_wgrad_deterministic(0)
    return count


def test_plans_match_the_recorded_launcher(L, golden):
    assert len(golden['fields']) == NF - 1
    n = sum(_check_problem(L, golden, rec) for rec in golden['problems'])
    # (five workspaces x deterministic off / on per problem; the two tables have at least 22 distinct convolutions)
    assert n == 10 * len(golden['problems']) >= 10 * 4 * 22 and {r[0] for r in golden['problems']} == {1, 8, 16, 32}
    assert (64, 256, 11, 2, 1) in {tuple(r[1:3] + r[4:7]) for r in golden['problems']}
    assert (896, 896, 29, 1, 2) in {tuple(r[1:3] + r[4:7]) for r in golden['problems']}
    for rec in golden['edges']:
        _check_problem(L, golden, rec)
    F = golden['fields']
    rows = [dict(zip(F, golden['rows'][ref - 1])) for rec in golden['edges'] for per in rec[13:15] for ref in per if ref > 0]
    assert any(r['total_steps'] == 1 for r in rows) and any(r['tiles'] > 1024 for r in rows)
    assert any(ref <= 0 for rec in golden['edges'] for ref in rec[13])                     # launches that are refused


def test_every_forced_plan_of_three_shapes(L, golden):
    F, counts = golden['fields'], golden['counts']
    assert counts == [1, 2, 3, 5, 18, 32, 40, 97, 256, 512, 1024, 1025]
    assert len({tuple(s['shape']) for s in golden['sweeps']}) == 3 and any(s['shape'][5] > 1 for s in golden['sweeps'])
    seen = set()
    for sw in golden['sweeps']:
        shape, ws, key = sw['shape'], sw['ws'], sw['shape'][:5]
        assert len(sw['per_order']) == 128
        for order, li in enumerate(sw['per_order']):
            for ci, (s, ref) in enumerate(zip(counts, sw['refs'][li])):
                want = _expect(golden, ref)
                assert _launch(L, golden, shape, ws, s, order) == want, (shape, ws, s, order)
                # the same plan through the per-thread hook, as the launch and the kept queries see it
                L.lib.w2l_wgrad_force_plan(s, order)
                nzx = want[F.index('needs_zero')] if want is not None else -ref
                assert L.lib.w2l_wgrad_needs_zero_x(*shape, ws) == nzx, (shape, ws, s, order)
                if ws == 0:
                    assert L.lib.w2l_wgrad_needs_zero(*key) == int(sw['needs_zero'][order * len(counts) + ci]), (shape, s, order)
                    base = sw['plans_order33' if order & 32 else 'plans_order1'][ci]
                    assert L.lib.w2l_wgrad_plan(*key) == (base & ~0xff) | order, (shape, s, order)
                L.lib.w2l_wgrad_force_plan(0, -1)
                if want is not None:
                    r = dict(zip(F, want))
                    seen.add(('dealt' if r['G'] else 'streamk' if r['streamk'] else 'slabs' if r['slabs'] else
                              'atomic' if r['atomic'] else 'unsplit', r['kwblk'], r['m32']))
    # every path the launcher has occurs: the reductions, the block forms (1 / 2 / 3 / 4 / 6 taps per block, 32x32x16)
    assert {s[0] for s in seen} == {'dealt', 'streamk', 'slabs', 'atomic', 'unsplit'}
    assert {s[1] for s in seen} >= {2, 3, 4, 6} and any(s[2] for s in seen)


def test_the_query_leaves_the_hook_alone(L):
    """forcing is an argument of w2l_wgrad_launch_plan: it neither reads the w2l_wgrad_force_plan hook nor disturbs it"""
    shape = (3, 192, 320, 333, 7, 1, 1)
    auto = _launch(L, None, shape, 0)
    L.lib.w2l_wgrad_force_plan(3, 16)
    assert _launch(L, None, shape, 0) == auto                                   # not read
    assert L.lib.w2l_wgrad_plan(*shape[:5]) == 16 | (3 << 8)
    forced = _launch(L, None, shape, 0, 5, 4)
    assert forced != auto and forced[0] == 5 and forced[6] == 1
    assert L.lib.w2l_wgrad_plan(*shape[:5]) == 16 | (3 << 8)                    # not disturbed
    L.lib.w2l_wgrad_force_plan(0, -1)
    assert _launch(L, None, shape, 0) == auto
    assert L.lib.w2l_replay_op(b'w2l_wgrad_launch_plan') == -1                  # a host-only query is recorded control flow
    assert _launch(L, None, (3, 100, 320, 333, 7, 1, 1), 0) is None             # channels must be multiples of 64
    assert _launch(L, None, (0, 192, 320, 333, 7, 1, 1), 0) is None


def test_a_remembered_choice_wins_over_the_cost_model(L, golden, tmp_path):
    """shapes no other test measures or loads (N = 7): the records were taken after w2l_tune_load of the same lines -- the
    format the launcher has always written -- so the lookup and how a remembered dealt / stream-K / atomic / three-tap plan
    narrows on a layer or a workspace that does not admit it are pinned; w2l_tune_save writes the lines back"""
    path = tmp_path / 'tune.txt'
    path.write_text('\n'.join(golden['cache']) + '\n')
    assert L.lib.w2l_tune_load(str(path).encode()) == 5                                # two of the seven lines are not plans
    for rec in golden['after_cache']:
        _check_problem(L, golden, rec)
    F = golden['fields']
    rows = [dict(zip(F, golden['rows'][ref - 1])) for rec in golden['after_cache'] for ref in rec[13] if ref > 0]
    assert any(r['G'] == 512 for r in rows) and any(r['streamk'] for r in rows) and any(r['taps3'] for r in rows)
    dil5 = [rec for rec in golden['after_cache'] if rec[:7] == [7, 896, 896, 500, 29, 1, 5]][0]
    assert all(golden['rows'][ref - 1][F.index('taps3')] == 0 for ref in dil5[13])
    saved = tmp_path / 'saved.txt'
    assert L.lib.w2l_tune_save(str(saved).encode()) == 0
    lines = saved.read_text().splitlines()
    assert all(line in lines for line in golden['cache'][:6]) and not any(line in lines for line in golden['cache'][6:])

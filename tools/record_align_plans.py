"""Record tests/golden/align_plans.json: what w2l_ctc_align_workspace_bytes and w2l_asg_align_workspace_bytes answer -- which is
the whole visible side of the alignment plan (csrc/align_core.h: block shape, LDS bytes, moves in LDS or in the workspace) --
over the grid that tests/test_cpu_align_plan.py replays.  No GPU: both are host-only queries.

    python tools/record_align_plans.py [out.json]          (W2L_LIB=<another build> records that build)

The file was recorded from the library as it was before align_core.h existed, when each criterion had its own plan function.
Rows: "ctc": [N, T, Smax, bytes], "asg": [N, T, A, Smax, bytes]; bytes -1 = no plan.  The grid: N 1 and 3; Smax 0 and both
sides of every block-shape step, the first refused length included; T 1, 16, 17, 500, 32768, 32769 and, for every Smax with
a plan, the two T either side of the switch from moves in LDS to moves in the workspace, found by bisecting the query."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd import _lib as L  # noqa: E402

NS = [1, 3]
TS = [1, 16, 17, 500, 32768, 32769]
CTC_SMAX = [0, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096]
ASG_SMAX = [0, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096]
ASG_A = 29
ASG_A_EDGES = [0, 1, 64, 65]               # at N = 1, T = 500, Smax = 64


def last_lds_t(query, smax):
    """the largest T in [1, 32768] whose moves still fit in LDS (the query is 0), or None: no plan, none fits, or all fit"""
    if query(1, smax) != 0 or query(32768, smax) == 0:
        return None
    lo, hi = 1, 32768                       # query(lo) == 0 < query(hi); the bytes grow with T
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if query(mid, smax) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def grid(query, smaxes):
    rows = []
    for smax in smaxes:
        edge = last_lds_t(lambda t, s: query(1, t, s), smax)
        ts = TS + ([edge, edge + 1] if edge is not None else [])
        rows += [[n, t, smax, int(query(n, t, smax))] for n in NS for t in ts]
    return rows


def record():
    ctc = grid(L.lib.w2l_ctc_align_workspace_bytes, CTC_SMAX)
    asg = [r[:2] + [ASG_A] + r[2:] for r in grid(lambda n, t, s: L.lib.w2l_asg_align_workspace_bytes(n, t, ASG_A, s), ASG_SMAX)]
    asg += [[1, 500, a, 64, int(L.lib.w2l_asg_align_workspace_bytes(1, 500, a, 64))] for a in ASG_A_EDGES]
    ctc += [[0, 500, 64, int(L.lib.w2l_ctc_align_workspace_bytes(0, 500, 64))],
            [1, 0, 64, int(L.lib.w2l_ctc_align_workspace_bytes(1, 0, 64))]]
    asg += [[0, 500, ASG_A, 64, int(L.lib.w2l_asg_align_workspace_bytes(0, 500, ASG_A, 64))],
            [1, 0, ASG_A, 64, int(L.lib.w2l_asg_align_workspace_bytes(1, 0, ASG_A, 64))]]
    return {'ctc': ctc, 'asg': asg}


def dumps(gold):
    return '{' + ',\n '.join('"%s": [\n%s]' % (k, ',\n'.join(json.dumps(r, separators=(',', ':')) for r in gold[k]))
                             for k in ('ctc', 'asg')) + '}\n'


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             'tests', 'golden', 'align_plans.json')
    text = dumps(record())
    with open(out, 'w') as f:
        f.write(text)
    print('%s: %d bytes' % (out, len(text)))

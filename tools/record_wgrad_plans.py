"""Record tests/golden/wgrad_plans.json: what the weight-gradient launcher (csrc/conv_wgrad.hip) decides on the host, for every
shape and forced plan that tests/test_cpu_wgrad_plan.py replays.  No GPU: everything goes through the host-only queries
w2l_wgrad_launch_plan, w2l_wgrad_needs_zero / _ws / _x, w2l_wgrad_plan and w2l_wgrad_group_tiles.

    python tools/record_wgrad_plans.py [out.json]          (W2L_LIB=<another build> records that build)

The file was first recorded from the launcher as it was before plan() existed (a throw-away build of it whose launch entry
point wrote down what it was about to launch), then again from this query: the two recordings are the same bytes.  Layout:
the docstring of tests/test_cpu_wgrad_plan.py."""
import ctypes as C
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd import _lib as L  # noqa: E402
from wav2letter_pytorch_amd import defaults  # noqa: E402

FIELDS = ['splits', 'steps_per_split', 'tsteps', 'total_steps', 'order', 'streamk', 'tg2', 'm32', 'taps3', 'kwb', 'kwblk',
          'kgroups', 'tiles', 'G', 'dealt_b', 'slabs', 'atomic', 'needs_zero', 'xrows_lds', 'lds', 'grid_x', 'grid_y', 'threads']
NF = len(FIELDS) + 1                      # + the last int: 1 = a launch, 0 = refused
COUNTS = [1, 2, 3, 5, 18, 32, 40, 97, 256, 512, 1024, 1025]
GROUP_FORMS = [0, 1, 4, 5, 8, 16, 17, 20, 21]
SWEEP_SHAPES = [(3, 192, 320, 335, 7, 1, 1), (8, 64, 256, 500, 11, 2, 1), (32, 896, 896, 500, 29, 1, 2)]
# shapes no test measures (N = 7): a dealt plan, a stream-K plan, a split that adds atomically beside a workspace (bit 6), a
# three-tap plan (queried at dilation 2, at dilation 5 and at stride 2, which it does not fit), a six-tap plan; two lines
# that w2l_tune_load must skip (more splits than steps; 32x32x16 together with three taps)
CACHE = ['w2l-tune v2 gfx950', 'wgrad 7 256 256 500 11 512 33', 'wgrad 7 384 384 500 13 1 3', 'wgrad 7 512 512 500 17 4 65',
         'wgrad 7 896 896 500 29 3 17', 'wgrad 7 640 640 500 21 2 21', 'wgrad 7 64 64 500 3 9999 1', 'wgrad 7 64 64 500 3 4 24']
CACHE_TAKEN = 5
CACHE_QUERIES = [(7, 256, 256, 500, 11, 1, 1), (7, 384, 384, 500, 13, 1, 1), (7, 512, 512, 500, 17, 1, 1),
                 (7, 896, 896, 500, 29, 1, 2), (7, 896, 896, 500, 29, 1, 5), (7, 896, 896, 500, 29, 2, 1),
                 (7, 640, 640, 500, 21, 1, 1), (7, 640, 640, 500, 21, 1, 4), (7, 64, 64, 500, 3, 1, 1)]


def model_shapes():
    """(Cin, Cout, Kw, stride, dilation) of every convolution of the default Wav2Letter table (with its classifier, padded to
    64 outputs) and of Jasper 10x5, first occurrence order"""
    shapes = []

    def add(*sh):
        if sh not in shapes:
            shapes.append(sh)
    cin = 64
    for c, k, s, d, _ in defaults.W2L_LAYERS:
        add(cin, c, k, s, d)
        cin = c
    add(cin, 64, 1, 1, 1)
    cin = 64
    for b in defaults.jasper10x5_model().jasper_blocks:
        c, k, s, d = b['layer_size'], b['kernel_size'], b['stride'], b.get('dilation', 1)
        k = k + 1 if k % 2 == 0 else k
        for r in range(b.get('repeat', 1)):
            add(cin if r == 0 else c, c, k, s, d)
        if b['residual']:
            add(cin, c, 1, 1, 1)
        cin = c
    add(cin, 64, 1, 1, 1)
    return shapes


EDGE_SHAPES = [(2, 128, 128, 40, 5, 1, 1), (1, 64, 64, 64, 3, 1, 1), (1, 256, 256, 1, 11, 1, 1),      # Tout < 64; one total step
               (4, 256, 384, 200, 1, 1, 1), (4, 256, 384, 200, 2, 1, 1), (4, 256, 384, 200, 3, 1, 1),
               (4, 256, 384, 200, 7, 1, 4), (4, 256, 384, 200, 7, 1, 5), (16, 128, 256, 300, 9, 2, 1),
               (16, 128, 256, 300, 3, 2, 3), (16, 64, 64, 700, 5, 1, 1), (2, 2048, 2048, 130, 9, 1, 1),   # 1280 tiles
               (2, 1024, 1024, 130, 31, 1, 1),                                                           # 1024 two-tap tiles
               (4, 256, 256, 200, 3, 1, 200), (4, 256, 256, 200, 3, 4, 40)]                            # LDS windows that do not fit


class Rows:
    def __init__(self):
        self.rows, self.index = [], {}

    def ref(self, rc, out, nzx):
        """row + 1 of a launch; a refused launch: 0, or -1 where w2l_wgrad_needs_zero_x still says 1"""
        assert (rc == 0) == (out[-1] == 1), (rc, out)
        if rc != 0:
            assert not any(out), out
            return -nzx
        assert out[FIELDS.index('needs_zero')] == nzx, (out, nzx)
        key = tuple(out[:-1])
        if key not in self.index:
            self.index[key] = len(self.rows)
            self.rows.append(list(key))
        return self.index[key] + 1


def query(shape, ws, splits=0, order=-1):
    out = (C.c_int * NF)(*([7] * NF))
    rc = L.lib.w2l_wgrad_launch_plan(*shape, ws, splits, order, out)
    return rc, list(out)


def workspaces(cin, cout, kw):
    a, b = L.lib.w2l_wgrad_workspace_bytes(cin, cout, kw), L.lib.w2l_wgrad_dealt_workspace_bytes(cin, cout, kw)
    return [0, 65536, a, b, max(a, b)]


def problem(rows, shape):
    n, cin, cout, tout, kw, stride, dil = shape
    wss = workspaces(cin, cout, kw)
    rec = list(shape) + [wss[2], wss[3], L.lib.w2l_wgrad_needs_zero(n, cin, cout, tout, kw), L.lib.w2l_wgrad_plan(n, cin, cout, tout, kw),
                         [L.lib.w2l_wgrad_needs_zero_ws(n, cin, cout, tout, kw, ws) for ws in wss],
                         [L.lib.w2l_wgrad_group_tiles(cin, cout, kw, f) for f in GROUP_FORMS]]
    for det in (0, 1):
        L.lib.w2l_wgrad_deterministic(det)
        rec.append([rows.ref(*query(shape, ws), L.lib.w2l_wgrad_needs_zero_x(*shape, ws)) for ws in wss])
    L.lib.w2l_wgrad_deterministic(0)
    return rec


def sweep(rows, shape, ws):
    """every order value x COUNTS, forced through the query's arguments; under the same plan pinned with w2l_wgrad_force_plan:
    w2l_wgrad_needs_zero as a string of 0 / 1 per order, and w2l_wgrad_plan of orders 1 and 33 (a dealt plan's count is not
    bounded by the step count)"""
    refs, nz5, plans = [], [], {1: [], 33: []}
    key = shape[:5]
    for order in range(128):
        per = []
        for s in COUNTS:
            rc, out = query(shape, ws, s, order)
            L.lib.w2l_wgrad_force_plan(s, order)
            nzx = L.lib.w2l_wgrad_needs_zero_x(*shape, ws)
            per.append(rows.ref(rc, out, nzx))
            if ws == 0:
                nz5.append(str(L.lib.w2l_wgrad_needs_zero(*key)))
                if order in plans:
                    plans[order].append(L.lib.w2l_wgrad_plan(*key))
            L.lib.w2l_wgrad_force_plan(0, -1)
        refs.append(per)
    lists = []                            # many orders narrow to the same launches: the distinct per-order lists, and which one
    for per in refs:
        if per not in lists:
            lists.append(per)
    rec = {'shape': list(shape), 'ws': ws, 'per_order': [lists.index(per) for per in refs], 'refs': lists}
    if ws == 0:
        rec.update(needs_zero=''.join(nz5), plans_order1=plans[1], plans_order33=plans[33])
    return rec


def after_cache(rows):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'tune.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(CACHE) + '\n')
        assert L.lib.w2l_tune_load(path.encode()) == CACHE_TAKEN
    return [problem(rows, sh) for sh in CACHE_QUERIES]


def record():
    rows = Rows()
    L.lib.w2l_wgrad_force_plan(0, -1)
    gold = {'fields': FIELDS, 'counts': COUNTS, 'group_forms': GROUP_FORMS}
    probs = []
    for n in (1, 8, 16, 32):
        for cin, cout, kw, stride, dil in model_shapes():
            probs.append(problem(rows, (n, cin, cout, 500, kw, stride, dil)))     # 1000 frames through the stride-2 first layer
    gold['problems'] = probs
    gold['edges'] = [problem(rows, sh) for sh in EDGE_SHAPES]
    gold['sweeps'] = [sweep(rows, sh, ws) for sh in SWEEP_SHAPES for ws in (0, workspaces(sh[1], sh[2], sh[4])[4])]
    gold['cache'] = CACHE
    gold['after_cache'] = after_cache(rows)
    gold['rows'] = rows.rows
    return gold


def dumps(gold):
    def js(v):
        return json.dumps(v, separators=(',', ':'))
    parts = ['"fields": ' + js(gold['fields']), '"counts": ' + js(gold['counts']), '"group_forms": ' + js(gold['group_forms']),
             '"rows": ' + js(gold['rows'])]
    for key in ('problems', 'edges', 'after_cache'):
        parts.append('"%s": [\n%s]' % (key, ',\n'.join(js(r) for r in gold[key])))
    sw = []
    for s in gold['sweeps']:
        head = {k: v for k, v in s.items() if k != 'refs'}
        sw.append(js(head)[:-1] + ',"refs":[\n' + ',\n'.join(js(r) for r in s['refs']) + ']}')
    parts.append('"sweeps": [\n%s]' % ',\n'.join(sw))
    parts.append('"cache": ' + js(gold['cache']))
    return '{' + ',\n '.join(parts) + '}\n'


if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             'tests', 'golden', 'wgrad_plans.json')
    text = dumps(record())
    with open(out, 'w') as f:
        f.write(text)
    print('%s: %d bytes' % (out, len(text)))

"""References of the MBR / edit-distance tests (test_cpu_mbr.py, test_gpu_mbr.py): the edit distance with its counts by the
recurrence of mbr.py, cell for cell in Python integers; the tokenisers; the selection in Python floats (IEEE double, the device's
order); and ``cases()``, the one generator of the inputs both test files use.  Nothing here imports the library.

``defect=`` plants one wrong reading of the definitions (DEFECTS); test_cpu_mbr.py shows that each changes an integer output
or a pick on ``cases()`` -- the cases can tell the readings apart."""
import math

import numpy as np

ENGLISH = ['_', "'"] + [chr(ord('A') + i) for i in range(26)] + [' ']      # data.label_sets.english_labels
SMALL = ['_', 'A', 'B', 'C', 'D', ' ']                                      # the end-to-end tests' six labels
MAX_TOKENS = 4095
U = 2.0 ** -53
# ulp errors of exp in float64: the device's (ROCm's OCML documents 1 ulp for the double-precision exp), the host's (glibc's exp
# is within 1 ulp)
DEVICE_EXP_ULP = 1
HOST_EXP_ULP = 1

DEFECTS = ('swap_del_ins', 'boundary_row', 'tie_order', 'keep_spaces', 'no_scale', 'tie_higher_rank', 'hash_words')


def risk_bound_c(k: int) -> float:
    """|risk_dev - risk_host| <= c(k) * u * risk, u = 2^-53, all terms being non-negative.  Both sides form scale * (w_j - m)
    with the same two IEEE operations, so the arguments of exp are the same numbers and e_j differs by the two exps' errors
    only: (DEVICE_EXP_ULP + HOST_EXP_ULP) ulps = 2 (D + H) u.  The sum S of k positive e_j: that, plus k - 1 roundings a side,
    2 (k - 1) u.  p_j = e_j / S: e_j's and S's differences plus a rounding a side: 4 (D + H) u + 2 (k - 1) u + 2 u.
    p_j * d (d an exact integer): + 2 u.  The sum of k such terms: + 2 (k - 1) u.  Total 4 k + 4 (D + H)."""
    return 4.0 * k + 4.0 * (DEVICE_EXP_ULP + HOST_EXP_ULP)


# ------------------------------------------------------------------------------------------------------------ edit distance
def edit_ops(a, b, defect=None):
    """(d, sub, del, ins) of reference ``a`` against hypothesis ``b``: D[0][0] = 0, D[i][0] = i deletions, D[0][j] = j
    insertions; for i, j >= 1 the candidates diagonal (+ a substitution if a[i-1] != b[j-1]), deletion, insertion in this order,
    the first of the smallest distance wins with its counts."""
    a, b = list(a), list(b)
    na, nb = len(a), len(b)
    off = 1 if defect == 'boundary_row' else 0
    prev = [(j + (off if j else 0), 0, 0, j) for j in range(nb + 1)]
    for i in range(1, na + 1):
        cur = [(i, 0, i, 0)]
        for j in range(1, nb + 1):
            d, s, dl, n = prev[j - 1]
            diag = (d, s, dl, n) if a[i - 1] == b[j - 1] else (d + 1, s + 1, dl, n)
            d, s, dl, n = prev[j]
            dele = (d + 1, s, dl + 1, n)
            d, s, dl, n = cur[j - 1]
            ins = (d + 1, s, dl, n + 1)
            if defect == 'swap_del_ins':
                dele, ins = (dele[0], dele[1], dele[2] - 1, dele[3] + 1), (ins[0], ins[1], ins[2] + 1, ins[3] - 1)
            order = (ins, dele, diag) if defect == 'tie_order' else (diag, dele, ins)
            best = order[0]
            for c in order[1:]:
                if c[0] < best[0]:
                    best = c
            cur.append(best)
        prev = cur
    return prev[nb]


def brute_alignments(a, b):
    """every (d, sub, del, ins) an alignment of ``a`` to ``b`` can have (matches free), by exhaustive enumeration"""
    seen = set()

    def walk(i, j, s, dl, n):
        if i == len(a) and j == len(b):
            seen.add((s + dl + n, s, dl, n))
            return
        if i < len(a) and j < len(b):
            walk(i + 1, j + 1, s + (a[i] != b[j]), dl, n)
        if i < len(a):
            walk(i + 1, j, s, dl + 1, n)
        if j < len(b):
            walk(i, j + 1, s, dl, n + 1)

    walk(0, 0, 0, 0, 0)
    return seen


# --------------------------------------------------------------------------------------------------------------- tokenisers
def word_hash(word) -> int:
    """csrc/edit_distance.hip's word filter over label indices: h = h * 17 + label (mod 2^32)"""
    h = 0
    for v in word:
        h = (h * 17 + int(v)) & 0xFFFFFFFF
    return h


def decode_ref(row, repeat: int):
    """ASG: a repeat label becomes the decoded label before it, leading ones are dropped (``repeat`` < 0: CTC, the row itself)"""
    out = []
    for v in row:
        v = int(v)
        if repeat < 0 or v != repeat:
            out.append(v)
        elif out:
            out.append(out[-1])
    return out


def text_tokens(text: str, unit: str, defect=None):
    """what Decoder.wer (``word``) / Decoder.cer (``char``) compare"""
    if unit == 'word':
        words = []
        cur = ''
        for ch in text:
            if ch.isspace():
                if cur:
                    words.append(cur)
                cur = ''
            else:
                cur += ch
        if cur:
            words.append(cur)
        return words
    return [ch for ch in text if defect == 'keep_spaces' or ch != ' ']


def row_text(row, labels, repeat: int = -1) -> str:
    return ''.join(labels[v] for v in decode_ref(row, repeat))


def row_tokens(row, labels, unit: str, repeat: int = -1, defect=None):
    toks = text_tokens(row_text(row, labels, repeat), unit, defect)
    if unit == 'word' and defect == 'hash_words':
        return [word_hash([labels.index(ch) for ch in w]) for w in toks]
    return toks


# ---------------------------------------------------------------------------------------------------------------- selection
def mbr_select_ref(tokens, weights, scale: float = 1.0, defect=None):
    """``tokens[j]``: the token list of row j, or None for an empty slot; ``weights[j]``: its log weight -> (pick, risk [k] with
    NaN for empty slots, dist [k, k] with -1 against them).  m = the greatest weight of a present row, e_j = exp(scale (w_j -
    m)), p_j = e_j / sum e_j, risk_i = sum_j p_j dist(i, j), everything in order j = 0..k-1; the least risk wins, a tie goes to
    the lower rank; no present row: pick 0."""
    k = len(tokens)
    here = [j for j in range(k) if tokens[j] is not None]
    dist = np.full((k, k), -1, dtype=np.int32)
    for i in here:
        dist[i, i] = 0
        for j in here:
            if i < j:
                dist[i, j] = dist[j, i] = edit_ops(tokens[i], tokens[j], defect)[0]
    risk = np.full(k, np.nan)
    if not here:
        return 0, risk, dist
    m = max(float(weights[j]) for j in here)
    sc = 1.0 if defect == 'no_scale' else float(scale)
    e = {j: math.exp(sc * (float(weights[j]) - m)) for j in here}
    total = 0.0
    for j in here:
        total += e[j]
    for i in here:
        r = 0.0
        for j in here:
            r += e[j] / total * float(dist[i, j])
        risk[i] = r
    pick = here[0]
    for i in here[1:]:
        if risk[i] < risk[pick] or (defect == 'tie_higher_rank' and risk[i] == risk[pick]):
            pick = i
    return pick, risk, dist


def risk_margin_ok(risk, k: int) -> bool:
    """the two smallest risks are exactly equal, or further apart than twice the bound on either"""
    r = np.sort(risk[~np.isnan(risk)])
    if len(r) < 2 or r[0] == r[1]:
        return True
    return r[1] - r[0] > 2.0 * risk_bound_c(k) * U * r[1]


# ------------------------------------------------------------------------------------------------------------------- cases
def _encode(text, labels=ENGLISH):
    return [labels.index(ch) for ch in text]


def _nbest_case(name, texts, weights, t, repeat=-1, scale=1.0, units=('word', 'char'), labels=ENGLISH, rows=None, lens=None):
    """texts[n][r]: the row's text over the labels, or None for an empty slot (``rows`` / ``lens``, where given, override the
    encoded labels / the lengths: encoded ASG rows, a length past T) -> the case as the arrays of a search's out buffer; what
    lies behind a row's length is filler that nothing may read as labels"""
    n, k = len(texts), len(texts[0])
    score = np.zeros((n, k), dtype=np.float64)
    length = np.full((n, k), -1, dtype=np.int32)
    lab = np.full((n, k, t), -7, dtype=np.int32)
    for u in range(n):
        for r in range(k):
            score[u, r] = weights[u][r]
            if texts[u][r] is None:
                score[u, r] = -np.inf
                continue
            enc = rows[u][r] if rows is not None and rows[u][r] is not None else _encode(texts[u][r], labels)
            assert len(enc) <= t, (name, u, r, len(enc))
            lab[u, r, :len(enc)] = enc
            length[u, r] = len(enc)
    if lens is not None:
        for (u, r), v in lens.items():
            length[u, r] = v
    return dict(kind='nbest', name=name, labels=labels, n=n, k=k, t=t, score=score, len=length, rows=lab, repeat=repeat,
                scale=scale, units=units)


def _descending(rng, k, step=0.7):
    return (-np.cumsum(rng.uniform(0.05, step, size=k))).tolist()


def _pair_case(name, seqs, pairs):
    return dict(kind='pairs', name=name, seqs=[np.asarray(s, dtype=np.int32) for s in seqs],
                pairs=np.asarray(pairs, dtype=np.int32).reshape(-1, 2))


LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 257)
LONG_WORD = 'ABCDEFGHIJKLMNOPQRSTUVWXYZABCDEFGHIJKLMN'          # 40 labels
COLLIDING = ('CAT', 'CBC')                                      # equal hashes: (4*17 + 2)*17 + 21 = (4*17 + 3)*17 + 4


def cases():
    """the inputs of both test files, small first.  kind 'pairs': sequences and (reference, hypothesis) index pairs for
    w2l_edit_distance; kind 'nbest': a search's out buffer for w2l_nbest_mbr"""
    assert word_hash(_encode(COLLIDING[0])) == word_hash(_encode(COLLIDING[1]))
    # ---- pairs: the lengths crossed, three alphabets
    for alphabet in (2, 4, 1000):
        rng = np.random.RandomState(alphabet)
        seqs = [rng.randint(0, alphabet, size=m) for m in LENGTHS]
        seqs += [rng.randint(0, alphabet, size=m) for m in LENGTHS]
        m = len(LENGTHS)
        yield _pair_case('crossed/a%d' % alphabet, seqs, [(i, m + j) for i in range(m) for j in range(m)])
    rng = np.random.RandomState(7)
    same = [rng.randint(0, 4, size=m) for m in (1, 64, 65, 200)]
    yield _pair_case('identical', same, [(i, i) for i in range(len(same))])
    low = [rng.randint(0, 5, size=m) for m in (3, 64, 130)]
    high = [rng.randint(5, 10, size=m) for m in (1, 70, 129, 0)]
    yield _pair_case('disjoint', low + high, [(i, len(low) + j) for i in range(len(low)) for j in range(len(high))])
    yield _pair_case('one-pair', [[1, 2, 3, 4], [1, 3, 4, 4, 5]], [(0, 1)])
    short = [rng.randint(0, 3, size=rng.randint(0, 12)) for _ in range(200)]
    yield _pair_case('5000-short', short, rng.randint(0, len(short), size=(5000, 2)))
    hub = [rng.randint(0, 4, size=90)] + [rng.randint(0, 4, size=rng.randint(60, 120)) for _ in range(40)]
    yield _pair_case('hub-500', hub, [(0, 1 + i % 40) if i % 2 else (1 + i % 40, 0) for i in range(500)])

    # ---- n-best lists, T = 40
    t = 40
    cat, cbc = COLLIDING
    eight = [['THE CAT SAT', 'THE %s SAT' % cbc, 'THE CAT SAT ON', None, 'THE CAR SAT', 'THE BAT SAT', 'THE CATS SAT', None],
             ['A B C', '', ' A  B C ', 'A B', LONG_WORD, "IT'S A B C", None, None],
             [None] * 8]
    rng = np.random.RandomState(11)
    yield _nbest_case('k8', eight, [_descending(rng, 8) for _ in range(3)], t)
    yield _nbest_case('k8/scale', [['X Y', 'A B', 'A C', None, None, None, None, None]] * 3,
                      [[math.log(0.40), math.log(0.35), math.log(0.25)] + [0.0] * 5] * 3, t, scale=3.0)
    yield _nbest_case('k1', [['THE CAT'], [None], ['']], [[-1.0], [0.0], [-2.5]], t)
    yield _nbest_case('k2/tie', [['A B', 'A C'], ['AB', None], [None, 'C D']], [[-1.5, -1.5]] * 3, t)
    yield _nbest_case('k4/tie', [['A B C', 'A B D', 'A E C', 'F B C']] * 3, [[-2.0] * 4] * 3, t)
    vocab = ['THE', 'CAT', cbc, 'SAT', 'A', 'ON', 'MAT', 'CATS', "IT'S", 'I']
    wide = []
    for u in range(3):
        rows = []
        for r in range(64):
            words = [vocab[i] for i in rng.randint(0, len(vocab), size=rng.randint(0, 8))]
            rows.append(None if (u == 1 and r % 5 == 3) or (u == 2 and r > 40) else ' '.join(words)[:t])
        wide.append(rows)
    yield _nbest_case('k64', wide, [_descending(rng, 64, 0.3) for _ in range(3)], t)
    # a length the buffer cannot hold: status 1 for that utterance only
    yield _nbest_case('k2/len-past-T', [['A B', 'A C'], ['A B', 'A C'], ['A', None]], [[-1.0, -1.2]] * 3, t, lens={(1, 1): t + 1})
    # ASG: '_' (label 0) is the repeat label; rows are encoded -- no two equal neighbours --, one starts with the repeat label
    rep = 0
    enc = [[_encode('AL_ CAL_S'), _encode('_AL_ CAL'), _encode('AL CAL_S'), None],
           [_encode('BO_K'), _encode('BOK'), _encode('_BO_K A'), _encode('_')],
           [None] * 4]
    asg_texts = [[None if row is None else row_text(row, ENGLISH, rep) for row in rows] for rows in enc]
    yield _nbest_case('k4/asg', asg_texts, [_descending(rng, 4) for _ in range(3)], t, repeat=rep, rows=enc)
    # one row of 4096 characters: over the token limit in the char unit
    long_t = 4100
    yield _nbest_case('k2/4096-chars', [['AB' * 2048, 'AB']], [[-1.0, -2.0]], long_t, units=('char',))


# ---- end to end: N = 3 utterances of T = 40 frames over SMALL, k = 8
E2E_SEEDS = (1, 2)
E2E_N, E2E_T, E2E_K = 3, 40, 8
E2E_LEXICON = ['A', 'AB', 'BA', 'BAD', 'CAB', 'DAD', 'ADD', 'CD', 'DA', 'ABC', 'B', 'DC']
E2E_HOTWORDS = ['BAD', 'CAB', 'DC']


def e2e_posteriors(seed: int, asg: bool = False):
    """[N, T, 6] float32: CTC posteriors (softmax rows), or with ``asg`` log-softmax scores.  Stretches of frames share a
    preferred label, so that the n-best list differs in whole words, not only in one character"""
    rng = np.random.RandomState(1000 + seed)
    z = rng.normal(size=(E2E_N, E2E_T, len(SMALL))) * 1.2
    for u in range(E2E_N):
        t = 0
        while t < E2E_T:
            run = rng.randint(1, 4)
            z[u, t:t + run, rng.randint(0, len(SMALL))] += 1.5
            t += run
    z -= z.max(axis=2, keepdims=True)
    p = np.exp(z)
    p /= p.sum(axis=2, keepdims=True)
    return (np.log(p) if asg else p).astype(np.float32)


def e2e_transitions(seed: int):
    """[6, 6] float32 ASG transitions"""
    return (np.random.RandomState(50 + seed).normal(size=(len(SMALL), len(SMALL))) * 0.3).astype(np.float32)


def nbest_ref(case, unit, defect=None):
    """w2l_nbest_mbr's section for a 'nbest' case -> dict(pick, status, risk, dist, pick_len, pick_labels)"""
    n, k, t = case['n'], case['k'], case['t']
    out = dict(pick=np.zeros(n, dtype=np.int32), status=np.zeros(n, dtype=np.int32), risk=np.full((n, k), np.nan),
               dist=np.full((n, k, k), -1, dtype=np.int32), pick_len=np.zeros(n, dtype=np.int32),
               pick_labels=np.zeros((n, t), dtype=np.int32))
    for u in range(n):
        tokens = []
        bad = False
        for r in range(k):
            m = int(case['len'][u, r])
            if m < 0:
                tokens.append(None)
                continue
            if m > t:
                bad = True
                break
            tokens.append(row_tokens(case['rows'][u, r, :m], case['labels'], unit, case['repeat'], defect))
            bad |= len(tokens[-1]) > MAX_TOKENS
        if bad:
            out['status'][u] = 1
        else:
            out['pick'][u], out['risk'][u], out['dist'][u] = mbr_select_ref(tokens, case['score'][u], case['scale'], defect)
        out['pick_len'][u] = case['len'][u, out['pick'][u]]
        out['pick_labels'][u] = case['rows'][u, out['pick'][u]]
    return out

"""Float64 references of the BatchNorm / dropout / activation family (csrc/bn_act.hip), restated from the formulas in
include/w2l_hip.h and the kernels -- plain NumPy, nothing of the engine's Python.  Pinned by tests/test_cpu_bn_refs.py (torch
float64 autograd, the published Philox known answers, planted defects), used by tests/test_gpu_bn_direct.py.  At the end: the
data gradient fused with the backward reduce (conv_igemm.hip, EPI = 1), pinned by tests/test_cpu_dgrad_bnreduce_refs.py and
used by tests/test_gpu_dgrad_bnreduce_direct.py.

Bounds are carried as ``Tr`` (value, magnitude sum, rounding depth) exactly as kernel_refs.py derives them.  What is particular
to this family:
  * scale / shift / mean / invstd that an activation or backward kernel READS are inputs: the fp32 values are exact.
  * dropout: z' = z * inv_keep is one more product; inv_keep = float32(1) / float32(1 - p) is computed by the host: an input.
  * a column sum over M rows has depth M (any order) while M < 5000; above, the depth of the kernel's own tree
    (``general_sum_depth``, ``slots_sum_depth``).
  * 1 / M is computed on the device in fp32: one rounding (Tr(1 / M, d = 1)).
  * the statistics finalize sums in double: its error, (rows + 8) 2^-53 (E[x^2] + mu^2) / (var + eps) relative, is asserted to
    be below u / 2 and is covered by the two spare u of Tr.bound; what remains are the casts to float and the fp32 products.
  * gates: a float64 gate and the fp32 gate of the device can differ only where z' is within its own bound of 0 or 20.  The
    case generator leaves no such element (``gate_ambiguous``), so gates -- and the q_clipped count -- must be EQUAL; z that
    is exactly 0 or 20 (planted, exactly computed on both sides) stays in.
"""
import dataclasses
import functools

import numpy as np

from kernel_refs import Tr, U, R_BF16, R_SPLIT, bf16_rne, bf16_to_f32, split_bf16, f32  # noqa: F401

AMAX_SLOTS = 64
SLAB = 64
SENTINEL = 1e4            # rows the kernels must never read


# ---- Philox4x32-10 (Salmon et al., SC'11) ------------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k, rounds=10):
    """counter c[4], key k[2] (arrays or scalars of 32-bit words) -> four arrays of 32-bit words, vectorised on uint64"""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & _M32 for x in c)
    k0, k1 = (np.asarray(x, dtype=np.uint64) & _M32 for x in k)
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c0            # 32 x 32 bits: no overflow of 64
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def keep_threshold(p, defect=None):
    p32 = np.float32(p)
    return int(np.uint32(p32 * np.float32(65535.0 if defect == 'thresh65535' else 65536.0)))


def keep_bits(seed, offset, gidx, p, defect=None):
    """the byte of 8-channel group ``gidx``: counter (gidx lo, gidx hi, offset lo, offset hi), key (seed lo, seed hi); bit 2j
    from the low half of word j, bit 2j+1 from the high half; kept iff u16 >= (uint32)(float32(p) * 65536)"""
    gidx = np.asarray(gidx, dtype=np.uint64)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    w = philox4x32_10((gidx & _M32, gidx >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    th = np.uint64(keep_threshold(p, defect))
    bits = np.zeros(gidx.shape, dtype=np.uint64)
    for j in range(4):
        bits |= ((w[j] & np.uint64(0xFFFF)) >= th).astype(np.uint64) << np.uint64(2 * j)
        bits |= ((w[j] >> np.uint64(16)) >= th).astype(np.uint64) << np.uint64(2 * j + 1)
    return bits.astype(np.uint8)


def unpack_keep(mask, N, T, C):
    """mask bytes [N*T*C/8] -> bool [N][T][C]"""
    m = np.asarray(mask, dtype=np.uint8).reshape(N, T, C // 8, 1)
    return ((m >> np.arange(8, dtype=np.uint8)) & 1).astype(bool).reshape(N, T, C)


def inv_keep_f32(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ---- OCP e4m3 ---------------------------------------------------------------------------------------------------------------

def e4m3_decode_table():
    t = np.zeros(256)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        t[c] = np.nan if (c & 0x7F) == 0x7F else (-v if c & 0x80 else v)
    return t


E4M3 = e4m3_decode_table()


def e4m3_rne_sat(x):
    """float64 -> e4m3 code: clamp to +-448, round to nearest, ties to even (3 mantissa bits, subnormal step 2^-9)"""
    x = np.asarray(x, dtype=np.float64)
    ax = np.minimum(np.abs(x), 448.0)
    m, e = np.frexp(np.where(ax < 2.0 ** -6, 1.0, ax))          # ax = m 2^e, m in [0.5, 1)
    q = np.rint((2 * m - 1) * 8).astype(np.int64)               # mantissa steps above 2^(e-1)
    ex = e - 1 + (q == 8)
    q = np.where(q == 8, 0, q)
    normal = ((ex + 7) << 3) | q
    sub = np.rint(ax * 2.0 ** 9).astype(np.int64)               # 0..8; 8 is the code of 2^-6
    code = np.where(ax < 2.0 ** -6, sub, normal)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def e4m3_bound(aq, q_scale):
    """|decode(code) - clamp(ref qs, +-448)| <= 2^-4 |ref qs| + 2^-10 + bound(a qs): half an ulp of 3 mantissa bits, half a
    subnormal step, the fp32 error carried through (aq = a * q_scale as Tr: the product is one more rounding)"""
    return 2.0 ** -4 * np.abs(aq.v) + 2.0 ** -10 + aq.bound()


# ---- the launchers' geometry (bn_act.hip), restated -----------------------------------------------------------------------------

def bwd_rows_per_wave(rows, C):
    rw = (rows * (C // SLAB) + 4095) // 4096
    rw = (rw + 7) // 8 * 8
    return min(max(rw, 16), 64)


def bwd_blocks(N, T, C):
    """rows of w2l_bn_act_bwd_reduce's partial buffer (w2l_bn_bwd_blocks)"""
    if N <= 0 or T <= 0 or C < SLAB:
        return 0
    rw = bwd_rows_per_wave(N * T, C)
    return (N * T + rw - 1) // rw


def apply_rows_per_block(rows, C):
    r = rows * (C // SLAB) // 1536
    r = (r + 31) // 32 * 32
    return min(max(r, 64), 1024)


def fwd_rows_per_block(rows, C):
    nb = (rows * (C // SLAB) + 32 * 2560 - 1) // (32 * 2560)
    return min(max(nb, 1), 16) * 32


def bn_loop_iters(rows, T, C):
    """row groups per wave of the looped backward kernels, 0 = the one-shot kernels (no W2L_BN_LOOP_ITERS in the environment)"""
    it = 4 if (rows >= 12000 and rows * C >= 8000000) else 0
    if T < 8:
        it = 0
    while it > 1 and rows < 4 * it * 8 * 4:
        it >>= 1
    return it


def apply_slots_groups(rows, T, C, amax):
    it = bn_loop_iters(rows, T, C)
    return it if it > 0 else (4 if amax else (2 if C <= 384 else 1))


def general_sum_depth(N, T, C, fin):
    """w2l_bn_act_bwd_reduce then w2l_bn_bwd_finalize (fin = 'finalize') or apply_fin's prologue (fin = 'apply_fin'): the
    lane's chain over its rows of the chunk, 3 shuffle levels; then the finalize kernel's chain over every eighth partial row
    and its 8 LDS adds, or the prologue's chain over every fourth row and 2 LDS adds"""
    rows = N * T
    if rows < 5000:
        return rows
    nb = bwd_blocks(N, T, C)
    tail = -(-nb // 8) + 8 if fin == 'finalize' else -(-nb // 4) + 2
    return bwd_rows_per_wave(rows, C) // 8 + 3 + tail


def slots_sum_depth(N, T, C, slots, nrows):
    """w2l_bn_act_bwd_reduce_slots then apply_slots' prologue: the lane's chain over its row groups, 3 shuffle levels, 2 LDS
    adds, the adds onto one slot address (at most ceil(chunks / slots), any order), slot_column_sums' chain over nrows"""
    rows = N * T
    if rows < 5000:
        return rows
    it = bn_loop_iters(rows, T, C)
    groups = it if it > 0 else 2
    chunks = -(-rows // (32 * groups))
    return groups + 3 + 2 + -(-chunks // slots) + nrows


def pad_src_rows(R, T, pad_l, pad_r, pad_mode):
    """source frame of every row of a padded [R] buffer: the frame itself, its mirror image under reflect padding, -1 = zero"""
    src = np.full(R, -1, dtype=np.int64)
    for r in range(R):
        t = r - pad_l
        if 0 <= t < T:
            src[r] = t
        elif pad_mode == 1 and -pad_l <= t < 0 and -t < T:
            src[r] = -t
        elif pad_mode == 1 and T <= t < T + pad_r and 2 * (T - 1) - t >= 0:
            src[r] = 2 * (T - 1) - t
    return src


def lens_limits(N, T, lens):
    return [T] * N if lens is None else [max(0, min(T, int(l))) for l in lens]


# ---- statistics finalize ---------------------------------------------------------------------------------------------------------

def bn_finalize_ref(partial, C, count, gamma, beta, eps, momentum, running_mean, running_var, defect=None):
    """train (partial [rows][2][C]) or eval (partial None) form.  Returns a dict of Tr: mean, invstd, scale, shift and,
    when running statistics are given in train form, running_mean / running_var after the update."""
    eps, mom = f32(eps), f32(momentum)
    ga = Tr(np.ones(C) if gamma is None else gamma)
    be = Tr(np.zeros(C) if beta is None else beta)
    out = {}
    if partial is not None:
        pr = np.asarray(partial, dtype=np.float64)
        rows = pr.shape[0]
        s1, s2 = pr[:, 0].sum(0), pr[:, 1].sum(0)
        mu = s1 / count
        var = np.maximum(s2 / count - mu * mu, 0.0)
        dbl = (rows + 8) * 2.0 ** -53 * (np.abs(pr[:, 1]).sum(0) / count + mu * mu) / (var + eps)
        assert (dbl < U / 2).all(), 'the double-precision sums are not negligible here'
        vn = var * count / (count - 1) if (defect == 'unbiased_invstd' and count > 1) else var
        M, I = Tr(mu, None, 1), Tr(1.0 / np.sqrt(vn + eps), None, 1)
        if running_mean is not None:
            unb = Tr(var * count / (count - 1) if count > 1 else var, None, 1)
            one, mo = Tr(1.0), Tr(mom)
            out['running_mean'] = (one - mo) * Tr(running_mean) + mo * M
            out['running_var'] = (one - mo) * Tr(running_var) + mo * unb
    else:
        M = Tr(running_mean)
        I = Tr(1.0) / (Tr(running_var) + Tr(eps)).sqrt()
    out['mean'], out['invstd'] = M, I
    out['scale'] = ga * I
    out['shift'] = be - M * ga * I
    return out


# ---- forward -------------------------------------------------------------------------------------------------------------------

def preact(y, scale, shift, y2=None, scale2=None, shift2=None):
    """z = y*scale + shift [+ y2*scale2 + shift2] as Tr; a NULL scale is the identity (y * 1 + 0: exact).  y and y2 may be
    tracked values themselves (the accumulators of a convolution: conv_refs.infer_ref) and then bring their magnitude and depth;
    a plain array is an exact input, as before"""
    tr = lambda a: a if isinstance(a, Tr) else Tr(a)
    z = tr(y) if scale is None else tr(y) * Tr(scale) + Tr(shift)
    if y2 is not None:
        z = z + (tr(y2) if scale2 is None else tr(y2) * Tr(scale2) + Tr(shift2))
    return z


def activate(v, act):
    return np.clip(v, 0.0, 20.0) if act == 1 else (np.maximum(v, 0.0) if act == 2 else v)


def bn_act_fwd_ref(N, T, C, y, scale, shift, y2=None, scale2=None, shift2=None, act=0, p=0.0, seed=0, offset=0, lens=None,
                   out_rows=None, pad_l=0, pad_r=0, pad_mode=0, q_scale=None, defect=None):
    """Returns dict: a (Tr, padded [N][R][C]), mask (uint8 [N*T*C/8] or None), mask_written (the bytes the kernel writes: the
    primary rows of frames t < lens[n]; a masked frame is written as zeros without being evaluated, and the backward pass never
    looks at its bits), src (row map), and with q_scale: aq (Tr of
    a * q_scale), codes (uint8, e4m3_rne_sat of the exact value), clipped (count over primary rows of |a| > 448 / q_scale),
    clip_margin (|a| - limit, primary rows)."""
    G = C // 8
    R = pad_l + T + pad_r if out_rows is None else out_rows
    src = pad_src_rows(R, T, pad_l, pad_r, pad_mode)
    z = preact(y, scale, shift, y2, scale2, shift2)
    live = src >= 0
    sc = np.where(live, src, 0)
    zv, za, d = z.v.reshape(N, T, C)[:, sc], z.a.reshape(N, T, C)[:, sc], z.d
    mask = None
    if p > 0:
        gidx = np.arange(N * T * G, dtype=np.uint64)
        mask = keep_bits(seed, offset, gidx, p, defect)
        keep = unpack_keep(mask, N, T, C)[:, sc]
        if defect == 'halo_fresh_bits':          # a halo copy draws bits of its own row index instead of its source frame's
            own = keep_bits(seed, offset, np.arange(N * R * G, dtype=np.uint64), p)
            halo = live & (np.arange(R) - pad_l != src)
            keep[:, halo] = unpack_keep(own, N, R, C)[:, halo]
        ik = inv_keep_f32(p)
        zv, za, d = np.where(keep, zv * ik, 0.0), np.where(keep, za * ik, 0.0), d + 1
    rowok = np.broadcast_to(live[None, :, None], (N, R, 1)).copy()
    for n, lim in enumerate(lens_limits(N, T, lens)):
        rowok[n, :, 0] &= sc < lim
    av = np.where(rowok, activate(zv, act), 0.0)
    aa = np.where(rowok, za, 0.0)
    if defect == 'tail_unwritten':
        av[:, pad_l + T + pad_r:] = np.nan
    written = np.zeros((N, T, G), dtype=bool)           # a frame t >= lens[n] is not evaluated: its mask bytes are not written
    for n, lim in enumerate(lens_limits(N, T, lens)):
        written[n, :lim] = True
    out = dict(a=Tr(av, aa, d), mask=mask, mask_written=written.reshape(-1), src=src)
    if q_scale is not None:
        qs = f32(q_scale)
        aq = Tr(av, aa, d) * Tr(qs)
        prim = np.arange(R) - pad_l == src
        margin = np.abs(av[:, prim]) - 448.0 / qs
        out.update(aq=aq, codes=e4m3_rne_sat(aq.v), clipped=int((margin > 0).sum()), clip_margin=margin,
                   clip_bound=Tr(av, aa, d).bound()[:, prim])
    return out


# ---- backward ------------------------------------------------------------------------------------------------------------------

def fold_grad(dxp, N, T, C, pad_l, pad_r, pad_mode, defect=None):
    """gradient of every frame from a padded source [N][rows][C]: its own row plus, under reflect padding, the halo rows that
    mirror it (t in [1, pad_l] on the left, t in [T-1-pad_r, T-2] on the right).  Returns (sum, sum of |.|, terms).
    A tracked source (Tr: a gradient that is itself a computed value, dgrad_bnreduce_ref) folds its own magnitude sum; its
    depth is the caller's to add (bn_act_bwd_ref)."""
    mag = dxp.a if isinstance(dxp, Tr) else None
    dxp = np.asarray(dxp.v if isinstance(dxp, Tr) else dxp, dtype=np.float64)
    mag = np.abs(dxp) if mag is None else mag
    g = dxp[:, pad_l:pad_l + T].copy()
    a = mag[:, pad_l:pad_l + T].copy()
    terms = np.ones(T, dtype=np.int64)
    if pad_mode == 1:
        for t in range(1, min(pad_l, T - 1) + 1):
            g[:, t] += dxp[:, pad_l - t]
            a[:, t] += mag[:, pad_l - t]
            terms[t] += 1
        hi = T - 3 if defect == 'fold_right_T2' else T - 2
        for t in range(max(T - 1 - pad_r, 0), hi + 1):
            g[:, t] += dxp[:, pad_l + 2 * (T - 1) - t]
            a[:, t] += mag[:, pad_l + 2 * (T - 1) - t]
            terms[t] += 1
    return g, a, terms


def bn_act_bwd_ref(N, T, C, y, scale, shift, mean, invstd, srcs, y2=None, scale2=None, shift2=None, mean2=None, invstd2=None,
                   act=0, p=0.0, mask=None, lens=None, halo=0, halo2=0, sums=None, sum_depth=None, defect=None):
    """srcs: one or two (dxp [N][rows][C], pad_l, pad_r, pad_mode).  sums: the device's published sums [ncomp][C], taken as
    exact inputs (w2l_bn_act_bwd_apply reads them), or None: the reference's own, with their Tr carried into dy.
    Returns dict: sums (Tr [ncomp][C]), dy / dy2 (Tr in the shared-halo layout [h + N*(T+h)][C]; dy2 None without a residual
    branch), amax1 / amax2 (max |dy| before the output rounding)."""
    M = N * T
    y = np.asarray(y, dtype=np.float64).reshape(N, T, C)
    has2 = y2 is not None
    if has2:
        y2 = np.asarray(y2, dtype=np.float64).reshape(N, T, C)
    z = preact(y, scale, shift, y2, scale2, shift2)
    gv, ga, terms, src_d = None, None, 0, 0
    for dxp, pl, pr_, pm in srcs:
        v, a, t = fold_grad(dxp, N, T, C, pl, pr_, pm, defect)
        gv, ga = (v, a) if gv is None else (gv + v, ga + a)
        terms = terms + t
        src_d = max(src_d, dxp.d if isinstance(dxp, Tr) else 0)        # a tracked source brings its own depth
    gate = np.ones((N, T, C), dtype=bool)
    for n, lim in enumerate(lens_limits(N, T, lens)):
        gate[n, lim:] = False
    masked = ~gate[:, :, :1]
    zv = z.v
    gk = Tr(1.0)
    gd = int(terms.max()) - 1 + src_d
    if p > 0:
        ik = inv_keep_f32(p)
        zv = zv * ik
        gate &= unpack_keep(mask, N, T, C)
        if defect != 'no_inv_keep_grad':
            gk = Tr(ik)
    if act == 1:
        gate &= (zv >= 0) & ((zv < 20) if defect == 'gate_open_20' else (zv <= 20))
    elif act == 2:
        gate &= (zv >= 0) if defect == 'relu_closed_0' else (zv > 0)
    g = Tr(np.where(gate, gv, 0.0), np.where(gate, ga, 0.0) if gd else None, gd)
    if p > 0:
        g = g * gk
    depth = (M if sum_depth is None else sum_depth)
    assert M < 5000 or sum_depth is not None

    def branch(yb, mean_b, invstd_b, scale_b, xh_for_sums=None):
        if mean_b is None:
            return None, None
        xh = (Tr(yb) - Tr(mean_b)) * Tr(invstd_b)
        xs = xh if xh_for_sums is None else xh_for_sums
        gx = g * xs
        sg = Tr(g.v.sum((0, 1)), g.a.sum((0, 1)), g.d + depth)
        sgx = Tr(gx.v.sum((0, 1)), gx.a.sum((0, 1)), gx.d + depth)
        return xh, (sg, sgx)

    xh1, s1 = branch(y, mean, invstd, scale)
    xh2, s2 = branch(y2, mean2, invstd2, scale2, xh1 if defect == 'res_sumgx_xhat1' else None) if has2 else (None, None)
    ncomp = 4 if has2 else 2
    zero = Tr(np.zeros(C))
    own = [s1[0] if s1 else Tr(g.v.sum((0, 1)), g.a.sum((0, 1)), g.d + depth), s1[1] if s1 else zero]
    if has2:
        own += [own[0], s2[1] if s2 else zero]
    sums_tr = Tr(np.stack([s.v for s in own]), np.stack([s.a for s in own]), max(s.d for s in own))
    invM = Tr(1.0 / (M - 1 if defect == 'sum_g_M1' else M), None, 1)
    invMx = Tr(1.0 / M, None, 1)

    def dy_of(k, xh, scale_b, h):
        sc = Tr(np.ones(C)) if scale_b is None else Tr(scale_b)
        if xh is None:
            d = g * sc if scale_b is not None else g
        else:
            if sums is None:
                sg, sgx = own[2 * k], own[2 * k + 1]
            elif isinstance(sums, Tr):                  # sums of given partial rows: exact values, their own depth
                sg, sgx = (Tr(sums.v[j], sums.a[j], sums.d) for j in (2 * k, 2 * k + 1))
            else:
                sg, sgx = Tr(sums[2 * k]), Tr(sums[2 * k + 1])
            xt = xh
            if defect == 'masked_xhat_dropped':
                xt = Tr(np.where(masked, 0.0, xh.v), np.where(masked, 0.0, xh.a), xh.d)
            d = sc * (g - sg * invM - xt * sgx * invMx)
        rows = h + N * (T + h)
        v, a = np.zeros((rows, C)), np.zeros((rows, C))
        for n in range(N):
            r = h + n * (T + h)
            v[r:r + T], a[r:r + T] = d.v[n], d.a[n]
        return Tr(v, a, d.d)

    dy = dy_of(0, xh1, scale, halo)
    dy2 = dy_of(1, xh2, scale2, halo2) if has2 else None
    return dict(sums=sums_tr, ncomp=ncomp, dy=dy, dy2=dy2, uses=(xh1 is not None, xh2 is not None), amax1=float(np.abs(dy.v).max()),
                amax2=float(np.abs(dy2.v).max()) if has2 else 0.0)


# ---- dynamic e4m3 scale ------------------------------------------------------------------------------------------------------

def quantize_dyn_ref(amax_slots):
    """s = 2^floor(log2(224 / max(slots))), exactly (the binade is read off the mantissa: 224 / (m 2^e), m in [0.5, 1), lies in
    [2^7, 2^8) 2^-e for m > 0.875 and in [2^8, 2^9) 2^-e otherwise); s = 1 at 0.  Returns (s, 1 / s)"""
    a = float(np.max(np.asarray(amax_slots, dtype=np.float64)))
    if not a > 0:
        return 1.0, 1.0
    m, e = np.frexp(a)
    k = (7 if m > 0.875 else 8) - int(e)
    return 2.0 ** k, 2.0 ** -k


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    N: int
    T: int
    C: int
    y_f32: int = 0
    bn1: int = 1          # 0: branch 1 without BatchNorm (scale = mean = NULL)
    res: int = 0          # 0 none; 1 residual branch with its own BatchNorm; 2 residual branch without (scale2 = mean2 = NULL)
    act: int = 1
    p: float = 0.0
    lens: str = 'none'    # 'none', 'ragged' (a 0 included), 'over' (a value above T)
    pad_l: int = 0
    pad_r: int = 0
    pad_mode: int = 0
    tail: int = 0         # rows behind pad_l + T + pad_r (forward: zero-filled; a gradient source's: never read)
    g_f32: int = 0
    two_src: int = 0
    q_scale: float = 0.0  # forward: e4m3 copy
    seed: int = 1

    @property
    def R(self):
        return self.pad_l + self.T + self.pad_r + self.tail

    @property
    def G(self):
        return self.C // 8

    def src2_geom(self):
        """the second gradient source: the other padding mode, its own pads and row count"""
        pl, pr_ = min(2, self.T - 1), min(3, self.T - 1)
        return pl, pr_, 1 - self.pad_mode, pl + self.T + pr_ + 1

    def sizes(self, halo=0, halo2=0):
        """element counts of every buffer of a direct call, from the geometry alone"""
        N, T, C = self.N, self.T, self.C
        return dict(y=N * T * C, out=N * self.R * C, mask=N * T * C // 8, src1=N * self.R * C, src2=N * self.src2_geom()[3] * C,
                    dy=(halo + N * (T + halo)) * C, dy2=(halo2 + N * (T + halo2)) * C,
                    partial=bwd_blocks(N, T, C) * (4 if self.res else 2) * C, sums=4 * C, amax=2 * AMAX_SLOTS)


PLANT = np.array([0.0, 20.0, 19.875, 20.125])          # z exactly 0, 20 and the bf16 neighbours of 20
PLANT_SCALE = np.array([1.0, 2.0, 0.5, 1.0])            # channels 0..3: scale a power of two, shift 0


def case_lens(kind, N, T):
    if kind == 'none':
        return None
    if kind == 'ragged':
        return np.array(([T, T // 2, 0] * N)[:N], dtype=np.int32)
    return np.array(([T + 5, T - 2, T + 1000] * N)[:N], dtype=np.int32)


def _bf16_round(x):
    return bf16_to_f32(bf16_rne(np.asarray(x, dtype=np.float32)))


def z_prime(c, D):
    """z' of every element as if kept (Tr)"""
    z = preact(D['y'], D['scale'], D['shift'], D['y2'], D['scale2'], D['shift2'])
    return z * Tr(inv_keep_f32(c.p)) if c.p > 0 else z


def gate_ambiguous(c, D):
    """elements whose gate (or whose count in q_clipped) a float64 and an fp32 evaluation could decide differently: z' within
    its own bound of 0 or 20 without being an exactly computed (planted) 0 or 20; |a| within its bound of 448 / q_scale"""
    z = z_prime(c, D)
    b = z.bound()
    amb = np.zeros(z.v.shape, dtype=bool)
    if c.act:
        for edge in ((0.0, 20.0) if c.act == 1 else (0.0,)):
            amb |= np.abs(z.v - edge) <= b
        amb &= ~D['planted']
    if c.q_scale:
        amb |= np.abs(np.abs(activate(z.v, c.act)) - 448.0 / f32(c.q_scale)) <= b
    return amb


@functools.lru_cache(maxsize=4)
def make_case(c):
    """host inputs of a case (float32 arrays holding the values the device gets; bf16 operands are bf16 values)"""
    rng = np.random.default_rng(1000 + c.seed)
    N, T, C = c.N, c.T, c.C
    wide = c.act == 1

    def draw(n):
        v = (rng.standard_normal(n) * (8 if wide else 3) + (8 if wide else 1)).astype(np.float32)
        return v if c.y_f32 else _bf16_round(v)

    D = dict(y2=None, scale=None, shift=None, mean=None, invstd=None, scale2=None, shift2=None, mean2=None, invstd2=None)
    D['y'] = draw(N * T * C).reshape(N, T, C)
    if c.bn1:
        D['scale'] = (rng.random(C) + 0.5).astype(np.float32)
        D['shift'] = (rng.standard_normal(C) * 0.5).astype(np.float32)
        D['scale'][:4], D['shift'][:4] = PLANT_SCALE, 0.0
    if c.res:
        D['y2'] = (draw(N * T * C) * np.float32(0.5)).reshape(N, T, C)       # (a power of two: bf16 values stay bf16 values)
        D['y2'][:, :, :4] = 0.0
        if c.res == 1:
            D['scale2'] = (rng.random(C) + 0.5).astype(np.float32)
            D['shift2'] = (rng.standard_normal(C) * 0.5).astype(np.float32)
            D['scale2'][:4], D['shift2'][:4] = 1.0, 0.0
    ps = PLANT_SCALE if c.bn1 else np.ones(4)
    pat = PLANT[(np.arange(N * T).reshape(N, T, 1) + np.arange(4)) % 4] / ps
    D['y'][:, :, :4] = pat.astype(np.float32)
    D['planted'] = np.zeros((N, T, C), dtype=bool)
    D['planted'][:, :, :4] = True
    for _ in range(20):                                 # resample: a safeguard (the set is empty at the first look as a rule)
        amb = gate_ambiguous(c, D)
        D['resampled'] = D.get('resampled', 0) + int(amb.sum())
        if not amb.any():
            break
        D['y'][amb] = draw(int(amb.sum()))
    else:
        raise AssertionError('gate-ambiguous elements survive resampling')
    eps = 1e-3
    for k, yk in (('', 'y'), ('2', 'y2')):
        if (k == '' and c.bn1) or (k == '2' and c.res == 1):
            y64 = D[yk].astype(np.float64)
            D['mean' + k] = y64.mean((0, 1)).astype(np.float32)
            D['invstd' + k] = (1.0 / np.sqrt(y64.var((0, 1)) + eps)).astype(np.float32)
    D['lens'] = case_lens(c.lens, N, T)
    D['seed'], D['offset'] = 0x9E3779B97F4A7C15 ^ c.seed, 3 + c.seed
    D['mask'] = keep_bits(D['seed'], D['offset'], np.arange(N * T * c.G, dtype=np.uint64), c.p) if c.p > 0 else None

    def grad(rows, pad_l, pad_r, pad_mode):
        g = rng.standard_normal((N, rows, C)).astype(np.float32)
        g = g if c.g_f32 else _bf16_round(g)
        if pad_mode == 0:                               # zero padding: the halo is skipped
            g[:, :pad_l] = SENTINEL
            g[:, pad_l + T:] = SENTINEL
        g[:, pad_l + T + pad_r:] = SENTINEL
        return g

    D['srcs'] = [(grad(c.R, c.pad_l, c.pad_r, c.pad_mode), c.pad_l, c.pad_r, c.pad_mode)]
    if c.two_src:
        pl, pr_, pm, rows = c.src2_geom()
        D['srcs'].append((grad(rows, pl, pr_, pm), pl, pr_, pm))
    return D


def fwd_ref_of(c, D, **kw):
    args = dict(act=c.act, p=c.p, seed=D['seed'], offset=D['offset'], lens=D['lens'], out_rows=c.R, pad_l=c.pad_l, pad_r=c.pad_r,
                pad_mode=c.pad_mode, q_scale=c.q_scale or None)
    args.update(kw)
    return bn_act_fwd_ref(c.N, c.T, c.C, D['y'], D['scale'], D['shift'], D['y2'], D['scale2'], D['shift2'], **args)


def bwd_ref_of(c, D, chunk=128, **kw):
    """bn_act_bwd_ref of a case; channels are independent, so a wide case is evaluated ``chunk`` channels at a time (memory)"""
    N, T, C = c.N, c.T, c.C
    parts = []
    for c0 in range(0, C, chunk):
        s = slice(c0, min(c0 + chunk, C))
        w = s.stop - s.start
        cut = lambda v: None if v is None else v[..., s]
        args = dict(y2=cut(D['y2']), scale2=cut(D['scale2']), shift2=cut(D['shift2']), mean2=cut(D['mean2']),
                    invstd2=cut(D['invstd2']), act=c.act, p=c.p, lens=D['lens'],
                    mask=None if D['mask'] is None else D['mask'].reshape(N * T, C // 8)[:, c0 // 8: s.stop // 8].reshape(-1))
        args.update(kw)
        if isinstance(args.get('sums'), Tr):
            args['sums'] = Tr(args['sums'].v[:, s], args['sums'].a[:, s], args['sums'].d)
        elif args.get('sums') is not None:
            args['sums'] = np.asarray(args['sums'], dtype=np.float64)[:, s]
        srcs = [(g[..., s], pl, pr_, pm) for g, pl, pr_, pm in D['srcs']]
        parts.append(bn_act_bwd_ref(N, T, w, D['y'][..., s], cut(D['scale']), cut(D['shift']), cut(D['mean']), cut(D['invstd']),
                                    srcs, **args))
    if len(parts) == 1:
        return parts[0]

    def cat(key):
        if parts[0][key] is None:
            return None
        return Tr(np.concatenate([q[key].v for q in parts], -1), np.concatenate([q[key].a for q in parts], -1),
                  max(q[key].d for q in parts))

    return dict(sums=cat('sums'), ncomp=parts[0]['ncomp'], dy=cat('dy'), dy2=cat('dy2'), uses=parts[0]['uses'], amax1=max(q['amax1'] for q in parts),
                amax2=max(q['amax2'] for q in parts))


def redepth(res, delta):
    """the same reference under a summation tree ``delta`` roundings deeper: the sums' depth enters the depth of the sums and
    of dy additively (the xhat * sum_gx / M term is the longest path of dy: max(d_x, d_y) + 1 picks it at every step); the dy of
    a branch without BatchNorm reads no sums and keeps its depth"""
    up = lambda t, on=True: None if t is None else Tr(t.v, t.a, t.d + (delta if on else 0))
    return dict(res, sums=up(res['sums']), dy=up(res['dy'], res['uses'][0]), dy2=up(res['dy2'], res['uses'][1]))


# general path (fwd, fwd_q, reduce + finalize, apply, apply_amax, apply_fin).  N = 3, T = 37 unless the point is another size.
GENERAL = [
    Case('clamp', 3, 37, 64, act=1, pad_l=3, pad_r=5, pad_mode=1, tail=3, seed=1),
    Case('clamp_f32_drop_lens', 3, 37, 64, y_f32=1, g_f32=1, act=1, p=0.3, lens='ragged', pad_l=36, pad_r=36, pad_mode=1, seed=2),
    Case('relu_res_drop_two', 3, 37, 128, res=1, act=2, p=0.3, lens='over', pad_l=2, pad_r=7, pad_mode=0, tail=1, two_src=1,
         q_scale=16.0, seed=3),
    Case('relu_res_nobn2_f32y', 3, 37, 64, y_f32=1, res=2, act=2, lens='ragged', seed=4),
    Case('none_nobn_gf32', 3, 37, 64, bn1=0, act=0, g_f32=1, pad_l=1, pad_r=0, pad_mode=1, two_src=1, seed=5),
    Case('relu_q', 3, 37, 64, act=2, pad_l=4, pad_r=4, pad_mode=1, q_scale=16.0, p=0.5, seed=6),
    Case('t3_n40', 40, 3, 64, act=1, p=0.3, pad_l=2, pad_r=2, pad_mode=1, seed=7),
    Case('mid_rows', 5, 1031, 960, act=2, lens='over', pad_l=1, pad_r=1, pad_mode=1, seed=8),      # rows per wave 24, ragged
    Case('wide_rows', 8, 1825, 1024, act=1, seed=9),      # rows per wave 64 (the smallest such), apply rows per block 160
]
# forward only: C = 8 / 24 (G = 1 / 3: the reciprocal division's fix-up), ragged last block of the grid's x
FWD_ONLY = [
    Case('c8', 3, 37, 8, act=1, p=0.3, pad_l=36, pad_r=36, pad_mode=1, tail=3, seed=11),
    Case('c24', 3, 37, 24, y_f32=1, act=2, lens='ragged', pad_l=5, pad_r=0, pad_mode=0, seed=12),
    Case('ragged_grid', 2, 160, 24, act=0, res=2, pad_l=5, pad_r=6, pad_mode=1, seed=13),      # R * G = 171 * 3 = 513 = 2 * 256 + 1
]
# the slot chain (bf16 y and gradient, one branch, one source, BatchNorm present, C % 64 == 0)
SLOTS = [
    Case('u1', 3, 37, 448, act=1, p=0.3, lens='ragged', pad_l=36, pad_r=36, pad_mode=1, seed=21),
    Case('u2', 3, 37, 128, act=2, pad_l=2, pad_r=3, pad_mode=0, tail=2, seed=22),
    Case('t5', 27, 5, 64, act=0, p=0.3, lens='over', pad_l=4, pad_r=4, pad_mode=1, seed=23),
]
# the looped kernels and their neighbours, reached by shape (bn_loop_iters)
LOOPED = [
    Case('loop_threshold', 24, 500, 704, act=1, pad_l=7, pad_r=7, pad_mode=1, seed=31),
    Case('loop_t8', 1500, 8, 704, act=2, p=0.5, lens='ragged', seed=32),
    Case('oneshot_t7', 1715, 7, 704, act=1, pad_l=6, pad_r=6, pad_mode=1, seed=33),
    Case('oneshot_below', 23, 521, 704, act=2, lens='over', pad_l=3, pad_r=0, pad_mode=1, seed=34),
]
BIG_APPLY = Case('grid_stride', 26, 500, 640, act=2, lens='ragged', pad_l=2, pad_r=2, pad_mode=1, seed=41)   # > 4096 x 256 items
FWD_FIN_BIG = Case('fwd_fin_two_batches', 12, 480, 896, act=1, pad_l=10, pad_r=10, pad_mode=1, seed=51)
FWD_FIN_SMALL = Case('fwd_fin_small', 3, 37, 128, res=1, act=2, p=0.3, lens='ragged', pad_l=3, pad_r=2, pad_mode=1, tail=3,
                     q_scale=16.0, seed=52)
ALL_CASES = GENERAL + FWD_ONLY + SLOTS + LOOPED + [BIG_APPLY, FWD_FIN_BIG, FWD_FIN_SMALL]


def is_big(c):
    return c.N * c.T * c.C > (1 << 21)


# statistics partials of w2l_bn_finalize / w2l_bn_act_fwd_fin: (rows, C, elements per row)
def make_partial(rows, C, per_row, seed, const_channel=None):
    """fp32 partial sums / sums of squares of random data, [rows][2][C]; const_channel: a channel of constant y = 1.5 (its
    sums are exact: the variance is exactly 0 and clamps there)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, per_row, C)) * 2 + rng.standard_normal(C)
    if const_channel is not None:
        x[:, :, const_channel] = 1.5
    pr = np.stack([x.sum(1), (x * x).sum(1)], axis=1).astype(np.float32)
    return pr, rows * per_row


# ---- the data gradient fused with the BatchNorm-backward reduce (conv_igemm_kernel EPI = 1, w2l_conv1d_dgrad_bnreduce_ws) ----

DG_DEFECTS = ('dead_rows_counted', 'mirror_own_gate', 'lens_on_halo_row', 'mask_nibble', 'no_gk_grad')


def dgrad_ref(dy, w, Kw, dil, halo, flat_rows):
    """the flat data gradient of a stride-1 convolution over the WHOLE shared-halo buffer dy [halo + flat_rows][Cout] as one
    sequence (w2l_conv1d_igemm_ws(N = 1, Tout = flat_rows) on the flipped-tap operand): row v reads dy rows v + (halo - hb) + k dil,
    hb = (Kw - 1) dil, with w[:, :, Kw - 1 - k] (w [Cout][Cin][Kw]).  Returns Tr [flat_rows][Cin]: A = sum |dy| |w|, depth Kw Cout."""
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    Cout, Cin, _ = w.shape
    hb = (Kw - 1) * dil
    assert halo >= hb and dy.shape == (halo + flat_rows, Cout)
    v, a = np.zeros((flat_rows, Cin)), np.zeros((flat_rows, Cin))
    for k in range(Kw):
        r0 = halo - hb + k * dil
        v += dy[r0:r0 + flat_rows] @ w[:, :, Kw - 1 - k]
        a += np.abs(dy[r0:r0 + flat_rows]) @ np.abs(w[:, :, Kw - 1 - k])
    return Tr(v, a, Kw * Cout)


def _swap_nibbles(mask):
    m = np.asarray(mask, dtype=np.uint8)
    return ((m << 4) | (m >> 4)).astype(np.uint8)


def _rowwise_sums(dx, per, N, T, C, y, scale, shift, mean, invstd, act, p, mask, lens, pad_l, pad_r, pad_mode, defect):
    """a WRONG epilogue, for the planted defects only: every padded row (n, u) counted by itself with the gate and xhat of a
    frame ts(u) -- the formulation in which the defects are mistakes of one line.  (defect = None is the right answer computed
    the other way round; test_cpu_dgrad_bnreduce_refs.py holds it against the fold-first reference.)"""
    Tp = pad_l + T + pad_r
    u = np.arange(per)
    raw = u - pad_l
    live = np.broadcast_to(u < Tp if defect != 'dead_rows_counted' else np.ones(per, dtype=bool), (N, per)).copy()
    out = (raw < 0) | (raw >= T)
    if pad_mode == 1:
        ts = np.where(raw < 0, -raw, np.where(raw >= T, 2 * (T - 1) - raw, raw))
    else:
        ts = raw
        live &= ~out
    ts = np.clip(ts, 0, T - 1)
    if defect == 'mirror_own_gate':
        ts = np.clip(raw, 0, T - 1)
    lims = np.asarray(lens_limits(N, T, lens))
    if lens is not None:
        live &= (raw[None, :] if defect == 'lens_on_halo_row' else ts[None, :]) < lims[:, None]
    z = preact(np.asarray(y, dtype=np.float64).reshape(N, T, C), scale, shift).v
    gate = np.ones((N, T, C), dtype=bool)
    gk = 1.0
    if p > 0:
        ik = inv_keep_f32(p)
        z = z * ik
        gate &= unpack_keep(_swap_nibbles(mask) if defect == 'mask_nibble' else mask, N, T, C)
        gk = 1.0 if defect == 'no_gk_grad' else ik
    if act == 1:
        gate &= (z >= 0) & (z <= 20)
    elif act == 2:
        gate &= z > 0
    w8 = (gate[:, ts] & live[:, :, None]) * gk                                     # [N][per][C]
    xh = np.zeros((N, T, C)) if mean is None else (np.asarray(y, dtype=np.float64).reshape(N, T, C) - mean) * invstd
    gv, ga = dx.v.reshape(N, per, C) * w8, dx.a.reshape(N, per, C) * w8
    d = dx.d + (1 if p > 0 else 0) + N * Tp
    return Tr(np.stack([gv.sum((0, 1)), (gv * xh[:, ts]).sum((0, 1))]),
              np.stack([ga.sum((0, 1)), (ga * np.abs(xh[:, ts])).sum((0, 1))]), d + 3)


def bnreduce_sums_ref(dx, per, N, T, C, y, scale, shift, mean, invstd, act, p, mask, lens, pad_l, pad_r, pad_mode, defect=None):
    """sums [2][C] (Tr) of g gate gk and g gate gk xhat from the flat gradient dx (Tr [N * per][C]; a plain array counts as
    exact): bn_act_bwd_ref fed with the first pad_l + T + pad_r rows of every utterance as its single gradient source -- folded
    onto the frames first, gated second.  The row sum has depth N (pad_l + T + pad_r): what the device adds up, row by row."""
    dx = dx if isinstance(dx, Tr) else Tr(dx)
    assert dx.v.shape == (N * per, C) and per >= pad_l + T + pad_r
    if defect is not None:
        assert defect in DG_DEFECTS
        return _rowwise_sums(dx, per, N, T, C, y, scale, shift, mean, invstd, act, p, mask, lens, pad_l, pad_r, pad_mode, defect)
    Tp = pad_l + T + pad_r
    src = Tr(dx.v.reshape(N, per, C)[:, :Tp], dx.a.reshape(N, per, C)[:, :Tp], dx.d)
    res = bn_act_bwd_ref(N, T, C, y, scale, shift, mean, invstd, [(src, pad_l, pad_r, pad_mode)], act=act, p=p, mask=mask,
                         lens=lens, sum_depth=N * Tp)
    return res['sums']


def dgrad_bnreduce_ref(dy, w, Kw, dil, halo, per, flat_rows, N, T, C, y, scale, shift, mean, invstd, act, p, mask, lens, pad_l,
                       pad_r, pad_mode, defect=None):
    """w2l_conv1d_dgrad_bnreduce_ws: dict(dx = the flat gradient (Tr [flat_rows][C], dead rows included), sums = Tr [2][C])"""
    assert flat_rows == N * per and np.asarray(w).shape[1] == C
    dx = dgrad_ref(dy, w, Kw, dil, halo, flat_rows)
    return dict(dx=dx, sums=bnreduce_sums_ref(dx, per, N, T, C, y, scale, shift, mean, invstd, act, p, mask, lens, pad_l, pad_r,
                                              pad_mode, defect))


@dataclasses.dataclass(frozen=True)
class DgCase:
    """a stride-1 convolution (Cout, Kw, dil) whose input is the padded activation of the producer unit ``u`` (a Case: N, T, C,
    act, p, lens, pads), and the shared-halo geometry of its dy: Tout = pad_l + T + pad_r - hb frames per utterance, ``halo``
    rows between them, per = Tout + halo rows of dx per utterance of which the first pad_l + T + pad_r are the padded rows"""
    u: Case
    Cout: int
    Kw: int
    dil: int
    halo: int

    @property
    def name(self):
        return self.u.name

    @property
    def hb(self):
        return (self.Kw - 1) * self.dil

    @property
    def Tp(self):
        return self.u.pad_l + self.u.T + self.u.pad_r

    @property
    def Tout(self):
        return self.Tp - self.hb

    @property
    def per(self):
        return self.Tout + self.halo

    @property
    def flat_rows(self):
        return self.u.N * self.per


def engine_halo(Tout, hb):
    """the engine's: the utterances of the flat sequence start on 64-row boundaries"""
    return max(hb, (Tout + 63) // 64 * 64 - Tout)


@functools.lru_cache(maxsize=16)
def make_dg_case(g, variant=0, zero_halo=False):
    """make_case of the producer plus dy (the WHOLE shared-halo buffer random bf16 values, halo rows too, unless zero_halo: the
    kernel is the plain convolution over the buffer whatever it holds, and only so are the dead rows of dx non-zero) and the
    conv weight [Cout][C][Kw] (bf16 values).  variant: other dy and w for the same producer (a second consumer)."""
    D = dict(make_case(g.u))
    rng = np.random.default_rng(7000 + 10 * g.u.seed + variant)
    c = g.u
    dy = _bf16_round(rng.standard_normal((g.halo + g.flat_rows, g.Cout)).astype(np.float32))
    if zero_halo:
        fr = (np.arange(g.halo + g.flat_rows) - g.halo) % g.per
        dy[(np.arange(g.halo + g.flat_rows) < g.halo) | (fr >= g.Tout)] = 0.0
    D['dy'] = dy
    D['w'] = _bf16_round((rng.standard_normal((g.Cout, c.C, g.Kw)) / np.sqrt(g.Cout * g.Kw)).astype(np.float32))
    return D


def dg_ref_of(g, D, defect=None, dx=None):
    """dgrad_bnreduce_ref of a case; dx given (exact accumulators): the sums alone"""
    c = g.u
    tail = (c.N, c.T, c.C, D['y'], D['scale'], D['shift'], D['mean'], D['invstd'], c.act, c.p, D['mask'], D['lens'], c.pad_l, c.pad_r,
            c.pad_mode, defect)
    if dx is not None:
        return bnreduce_sums_ref(dx, g.per, *tail)
    return dgrad_bnreduce_ref(D['dy'], D['w'], g.Kw, g.dil, g.halo, g.per, g.flat_rows, *tail)


def dg_defect_applies(g, defect):
    """whether a defect can show on a case at all, from its geometry alone"""
    c = g.u
    reflect = c.pad_mode == 1 and (c.pad_l or c.pad_r)
    return {'dead_rows_counted': reflect and g.per > g.Tp, 'mirror_own_gate': bool(reflect),
            'lens_on_halo_row': bool(reflect) and c.lens != 'none', 'mask_nibble': c.p > 0, 'no_gk_grad': c.p > 0}[defect]


# the cases of tests/test_gpu_dgrad_bnreduce_direct.py (C % 64 == 0; N per = 459 .. 576 flat rows)
DG_A = DgCase(Case('A_per153', 3, 141, 192, act=1, p=0.25, lens='ragged', pad_l=6, pad_r=6, pad_mode=1, seed=71), 128, 7, 2, 12)
DG_B = DgCase(Case('B_engine_per', 3, 141, 192, act=1, p=0.25, lens='ragged', pad_l=6, pad_r=6, pad_mode=1, seed=72), 128, 7, 2,
              engine_halo(141, 12))
DG_C = DgCase(Case('C_zero_relu', 5, 97, 320, act=2, pad_l=3, pad_r=3, pad_mode=0, seed=73), 128, 7, 1, 9)
DG_D = DgCase(Case('D_longest_mirror', 12, 19, 128, act=1, p=0.25, lens='ragged', pad_l=6, pad_r=18, pad_mode=1, seed=74), 192, 7, 4,
              27)
DG_E = DgCase(Case('E_no_batchnorm', 3, 141, 192, bn1=0, act=2, p=0.25, lens='ragged', pad_l=6, pad_r=6, pad_mode=1, seed=75), 128,
              7, 2, 15)
DG_CASES = [DG_A, DG_B, DG_C, DG_D, DG_E]

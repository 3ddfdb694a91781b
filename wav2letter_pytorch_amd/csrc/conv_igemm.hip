// Conv1d forward / data-gradient as an implicit GEMM on CDNA4 MFMA (gfx950).
//
//   y[n][t][co] (+)= bias[co] + sum_{kw} sum_{ci} w[kw][co][ci] * xp[n][t*s + kw*d][ci]
//
// GEMM view: M = co (A = weights, K-contiguous), N = t (B = activations,
// K-contiguous because activations are channels-last), K = (kw, ci).
// The B operand is never materialised (no im2col): for one 64-channel chunk a
// block stages ONE time window of (BN-1)*s + (Kw-1)*d + 1 rows in LDS and every
// tap kw reads it at a row offset kw*d, so activation traffic is amortised over
// the Kw taps.  Weights stream one [BM x 64] tile per (chunk, tap) step.
// Both tiles are filled by LDS-DMA (global_load_lds_dwordx4), double-buffered,
// with the 16-byte-chunk XOR swizzle applied on the *source* address and on the
// ds_read_b128 address (the LDS image itself is lane-linear).
//
// Replaces nn.Conv1d at wav2letter.py:35-36,42 / jasper.py:96-105,127 (forward) and
// its autograd data gradient.  Padding is physical: the producer kernel writes the
// reflect (wav2letter.py:28-34) or zero halo, so the hot loop has no padding logic.
#include "common.h"
#include "../../include/w2l_hip.h"
#include <algorithm>
#include <array>
#include <map>
#include <vector>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <utility>

namespace {

constexpr int BK = 64;                 // channels per K chunk (128-byte LDS rows)
constexpr int ROWB = BK * 2;           // bytes per LDS row

struct IgemmParams {
    const bf16_raw* x;
    const bf16_raw* w;
    void* y;
    const float* bias;
    union { float* stats; uint8_t* fz_q; };       // fz_q (EPI == 2, which writes no statistics): the e4m3 copy of the output
    int stats_slots;          // 0: one statistics row per 128-column tile (plain stores); S: added onto row (tile mod S) with fp32 atomics
    int64_t x_rows_per_utt;   // x_bstride / Cin
    int64_t x_max_row;        // last readable flat row
    int N, Cin, Cout, Tout, Kw, stride, dil;
    int tiles_t, ncols, xrows_lds;
    int y_f32, accumulate;
    // split-K (w2l_conv1d_igemm_ws): `splits` blocks share one output tile, each reducing a contiguous range of the
    // (chunk, tap) steps; partial tiles go through fp32 slabs, the block that draws the last ticket sums and stores
    int splits;
    float* slabs;             // [tiles][splits][BM*BN]
    unsigned* tickets;        // [tiles], zero between launches
    // stream-K (SK kernels): the grid is sk_ranges blocks; block r owns steps [W*r/G, W*(r+1)/G) of the tile-major
    // (tile, step) space, W = sk_total = tiles * steps per tile, and walks the tiles that range touches one after the other.
    // A tile cut by range boundaries is combined exactly like a split-K tile (slab id = range + tile: unique, and the pieces
    // of one tile are consecutive), a whole tile inside one range goes straight to the epilogue
    int sk_ranges, sk_total;
    float descale;            // F8 kernels: y = acc * descale (+ bias), descale = 1 / (activation scale * weight scale)
    // descale_dev: optional further factor in device memory (scale derived from a device-side amax), EPI != 2 only
    // fz_clip (EPI == 2): optional counter of the elements that saturate the e4m3 copy
    union { const float* descale_dev; unsigned long long* fz_clip; };
    // EPI == 1 (data gradient fused with the BatchNorm-backward reduction of the layer that produced the conv's input):
    // the output tile IS the gradient wrt that layer's padded activation, so the epilogue also forms, per channel,
    // sum g*gate and sum g*gate*xhat over its rows (what bn_act_bwd_reduce_kernel computes in a pass of its own)
    // EPI == 2 (inference, w2l_conv1d_igemm_bnact): the whole unit in the epilogue -- BatchNorm as the per-channel affine map
    // it is with running statistics, the residual branch, the activation, the length mask -- stored as bf16 straight into the
    // consumer's padded operand, halo rows included; no y, no statistics.  Its fields (fz_*) SHARE the storage of the EPI == 1
    // fields, which a launch never uses together with them: the struct -- the kernel argument of every instantiation -- keeps
    // its size and offsets, and with them the code of the EPI == 0 / 1 kernels.
    // F8 && EPI == 2 (w2l_conv1d_igemm_bnact_fp8): the same epilogue on e4m3 operands, v = acc * descale + bias first; the
    // output is written as e4m3 bytes (fz_q, value * fz_qscale, from the fp32 value) and / or as bf16 (fz_out may be NULL).
    union { const bf16_raw* bn_y; const bf16_raw* fz_res; };          // bn_y: that layer's conv output [N][T][C] (C = this launch's Cout)
                                                                      // fz_res: optional dense [N][Tout][Cout] second branch
    union { const float* bn_scale; const float* fz_scale; };          // bn_*: its BatchNorm scale / shift / mean / invstd
    union { const float* bn_shift; const float* fz_shift; };          // fz_scale / fz_shift: the folded affine map, NULL: identity
    union { const float* bn_mean; const bf16_raw* fz_res_lo; };       // fz_res_lo: the second branch's lo half (split-bf16 mode)
    union { const float* bn_invstd; bf16_raw* fz_out; };              // fz_out: [N][fz_rows][Cout], frame t at row fz_pad_l + t
    union { const uint8_t* bn_mask; bf16_raw* fz_out_lo; };           // bn_mask: dropout keep bits (one byte per 8 channels) or NULL
                                                                      // fz_out_lo: optional lo half of the output
    union { const int32_t* bn_lens; const int32_t* fz_lens; };        // optional [N] valid lengths (fz: frames beyond are stored as 0)
    union { int bn_T; int fz_rows; };
    union { int bn_pad_l; int fz_pad_l; };
    union { int bn_pad_mode; int fz_pad_mode; };
    union { int bn_per; int fz_pad_r; };
    int bn_Tp;
    union { int bn_act; int fz_act; };
    union { float bn_gk; float fz_qscale; };   // bn_gk: 1 / (1 - p) with dropout, else 1; fz_qscale: scale of the e4m3 copy
};

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
// one 16x16x128 MFMA on OCP e4m3 operands (cbsz = blgp = 0) with unit E8M0 block scales (127 = 2^0): per-tensor scaling
// is applied by the producer kernels and undone in the epilogue.  The 32 operand bytes of a lane are two ds_read_b128
// chunks; A and B take the same 32 channels of a row per lane group, so the products pair up whatever order the
// instruction walks its k range in.
__device__ __forceinline__ f32x4 mfma_e4m3_k128(bf16x8 a_lo, bf16x8 a_hi, bf16x8 b_lo, bf16x8 b_hi, f32x4 c) {
    const v4i al = __builtin_bit_cast(v4i, a_lo), ah = __builtin_bit_cast(v4i, a_hi);
    const v4i bl = __builtin_bit_cast(v4i, b_lo), bh = __builtin_bit_cast(v4i, b_hi);
    const v8i av = __builtin_shufflevector(al, ah, 0, 1, 2, 3, 4, 5, 6, 7);
    const v8i bv = __builtin_shufflevector(bl, bh, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_dst_wave_base, 16, 0, 0);
}

// MW x NW waves, each owning MS x NS MFMA tiles of 16x16: block tile BM = 16*MW*MS (co) x BN = 16*NW*NS (t)
// S = conv stride (compile time: the fragment reads then use immediate LDS offsets)
// F8: operands are OCP e4m3 bytes (x [.][rows][Cin], w [Kw][Cout][Cin], one byte per element): a 128-byte LDS row is 128
// channels, a K step is one tap of a 128-channel chunk, and its MS x NS MFMAs are v_mfma_scale_f32_16x16x128_f8f6f4 (twice
// the bf16 rate); LDS-DMA, swizzle, window reuse, split-K and the epilogue are the bf16 kernel's.  PIPE = 0 only.
// One piece of a stream-K range: the tile the range's cursor w_cur is in, the steps [s_begin, s_end) of that tile the range owns,
// how many ranges share the tile (nsplit), this range's place among them (split) and the first of the tile's consecutive slab ids.
// Range r owns steps [W r / G, W (r + 1) / G) of the tile-major space, W = tiles * S_; the range holding step w is
// ceil((w + 1) G / W) - 1.  Host and device run this same function (w2l_conv_streamk_pieces: the CPU test of the decomposition).
// G e4m3 dwords of one lane as one store (the fused e4m3 epilogue)
template <int G> struct QVec { typedef unsigned type __attribute__((ext_vector_type(G))); };
template <> struct QVec<1> { typedef unsigned type; };

struct SkPiece { int tile, s_begin, s_end, nsplit, split; int64_t slab_base; };
__host__ __device__ inline SkPiece sk_piece(int W, int G, int S_, int r, int w_cur, int w_end) {
    SkPiece q;
    q.tile = w_cur / S_;
    q.s_begin = w_cur - q.tile * S_;
    q.s_end = q.s_begin + (w_end - w_cur) < S_ ? q.s_begin + (w_end - w_cur) : S_;
    const int r_lo = (int)((((int64_t)q.tile * S_ + 1) * G + W - 1) / W) - 1;
    const int r_hi = (int)((((int64_t)q.tile * S_ + S_) * G + W - 1) / W) - 1;
    q.nsplit = r_hi - r_lo + 1;
    q.split = r - r_lo;
    q.slab_base = (int64_t)r_lo + q.tile;
    return q;
}

template <int MW, int NW, int MS, int NS, int S, int PIPE, bool F8 = false, int EPI = 0, bool SK = false>
__global__ __launch_bounds__(64 * MW * NW, 2) void conv_igemm_kernel(IgemmParams p) {
    static_assert(!SK || (!F8 && EPI == 0 && S == 1), "stream-K is built for the plain bf16 stride-1 kernels");
    static_assert(!(F8 && PIPE != 0), "the e4m3 kernel is built for K-loop structure 0 only");
    static_assert(EPI != 1 || (!F8 && S == 1), "the fused BatchNorm-backward epilogue belongs to bf16 data gradients");
    constexpr int ESZ = F8 ? 1 : 2;                // bytes per operand element
    constexpr int BKE = ROWB / ESZ;                // channels per K chunk (one 128-byte LDS row)
    constexpr int BM = 16 * MW * MS, BN = 16 * NW * NS, NWAVES = MW * NW, NT = 64 * NWAVES;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NW, wn = wave % NW;

    // consecutive logical ids share an XCD (xcd_remap): the `splits` blocks of one tile run next to each other in time and
    // place, so their slabs meet in that XCD's L2
    const int lin = xcd_remap(blockIdx.x, gridDim.x);
    // (consecutive ranges of a stream-K launch share tiles: the same remap keeps them on one XCD)
    int w_cur = 0, w_end = 0;
    if constexpr (SK) {
        w_cur = (int)(((int64_t)p.sk_total * lin) / p.sk_ranges);
        w_end = (int)(((int64_t)p.sk_total * (lin + 1)) / p.sk_ranges);
    }
    do {                                               // one pass per tile this block works on (exactly one unless SK)
    int split, tile, nsplit, sk_begin = 0, sk_end = 0;
    int64_t slab_base;
    if constexpr (SK) {
        __syncthreads();                               // the previous tile's LDS (ticket word, statistics scratch) is dead
        const SkPiece q = sk_piece(p.sk_total, p.sk_ranges, (p.Cin / (ROWB / (F8 ? 1 : 2))) * p.Kw, lin, w_cur, w_end);
        tile = q.tile;
        sk_begin = q.s_begin;
        sk_end = q.s_end;
        w_cur += sk_end - sk_begin;
        nsplit = q.nsplit;
        split = q.split;
        slab_base = q.slab_base;
    } else {
        nsplit = p.splits;
        split = nsplit > 1 ? lin % nsplit : 0;
        tile = nsplit > 1 ? lin / nsplit : lin;
        slab_base = (int64_t)tile * nsplit;
    }
    const int tm = tile / p.ncols;
    const int col = tile - tm * p.ncols;
    const int n = col / p.tiles_t;
    const int tt = col - n * p.tiles_t;
    const int m0 = tm * BM;
    const int t0 = tt * BN;

    constexpr int s = S;
    const int d = p.dil, Kw = p.Kw, Cin = p.Cin;
    const int xrows = p.xrows_lds;                 // multiple of 8
    char* wbuf0 = smem;
    char* wbuf1 = smem + BM * ROWB;
    char* xbuf0 = smem + 2 * BM * ROWB;
    char* xbuf1 = xbuf0 + xrows * ROWB;

    const int64_t xrow0 = (int64_t)n * p.x_rows_per_utt + (int64_t)t0 * s;

    // ---- staging (each wave-instruction writes 8 LDS rows = 1 KiB by LDS-DMA) ----
    // The main loop is issue-bound (VALU + MFMA share a SIMD's issue port), so everything that does not
    // change from step to step is hoisted: a weight tile's source address is a wave-uniform slab base
    // (tap, chunk) plus a per-lane 32-bit offset computed once.
    const int srow = lane >> 3;                    // row within the 8-row group
    const int schunk = lane & 7;                   // LDS chunk this lane fills
    const int gchunk = schunk ^ srow;              // source chunk (groups are 8-row aligned: row&7 == srow)
    constexpr int WGROUPS = BM / 8;
    constexpr int W_PER_WAVE = (WGROUPS + NWAVES - 1) / NWAVES;
    unsigned w_voff[W_PER_WAVE];
#pragma unroll
    for (int i = 0; i < W_PER_WAVE; ++i) {
        int co = m0 + (wave + i * NWAVES) * 8 + srow;
        co = co < p.Cout ? co : p.Cout - 1;
        w_voff[i] = (unsigned)co * (unsigned)Cin * (unsigned)ESZ + (unsigned)gchunk * 16u;
    }
    const int64_t w_tap_bytes = (int64_t)p.Cout * Cin * ESZ;
    auto stage_w = [&](char* dst, int kw, int c) {
        W2L_DIAG_SKIP_DMA(p);
        const char* slab = reinterpret_cast<const char*>(p.w) + kw * w_tap_bytes + c * (BK * 2);   // wave-uniform
#pragma unroll
        for (int i = 0; i < W_PER_WAVE; ++i) {
            const int grp = wave + i * NWAVES;
            if ((WGROUPS % NWAVES == 0) || grp < WGROUPS) glds16(slab + w_voff[i], dst + grp * 1024);
        }
    };
    auto stage_x = [&](char* dst, int c) {
        W2L_DIAG_SKIP_DMA(p);
        const int ngrp = xrows >> 3;
        for (int grp = wave; grp < ngrp; grp += NWAVES) {
            int64_t r = xrow0 + grp * 8 + srow;
            r = r < p.x_max_row ? r : p.x_max_row;
            const char* src = reinterpret_cast<const char*>(p.x) + (r * Cin + (int64_t)c * BKE) * ESZ + gchunk * 16;
            glds16(src, dst + grp * 1024);
        }
    };

    f32x4 acc[MS][NS];
#pragma unroll
    for (int i = 0; i < MS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nchunks = Cin / BKE;
    // this block's share of the nchunks * Kw (chunk-major) steps; a range may start in the middle of a chunk
    const int total_steps = nchunks * Kw;
    const int s_begin = SK ? sk_begin : (nsplit > 1 ? (int)(((int64_t)total_steps * split) / nsplit) : 0);
    const int s_end = SK ? sk_end : (nsplit > 1 ? (int)(((int64_t)total_steps * (split + 1)) / nsplit) : total_steps);
    const int nsteps = s_end - s_begin;
    const int c_first = s_begin / Kw, kw_first = s_begin - c_first * Kw;

    // per-lane fragment offsets (constant over the whole K loop)
    const int fr = lane & 15, fq = lane >> 4;
    // bf16: k-substep 0 reads 16-byte chunk fq of the row, k-substep 1 chunk 4+fq.  e4m3: the lane group's 32 channels
    // are chunks 2fq and 2fq+1, both operands of the one MFMA of the step.
    constexpr int CH1_XOR = F8 ? 16 : 64;          // byte distance (under the XOR swizzle) between the two chunks of a lane
    const int ch0 = F8 ? 2 * fq : fq;
    const int a_lane0 = (wm * MS * 16 + fr) * ROWB + ((ch0 ^ (fr & 7)) << 4);
    const int a_lane1 = a_lane0 ^ CH1_XOR;
    const int b_row0 = (wn * NS * 16 + fr) * s;      // tile rows ni*16*s further down share (row & 7): NS reads per base

    // Two K-loop structures are built for every block shape; which one is faster depends on the shape and the
    // pass (measured by w2l_conv1d_igemm_tune): PIPE = 0 keeps the barrier at the top of a step, PIPE = 1 moves it
    // to the middle so that the next step's first fragment reads overlap this step's last MFMAs.
    if constexpr (PIPE == 0) {
        stage_x((c_first & 1) ? xbuf1 : xbuf0, c_first);
        stage_w(wbuf0, kw_first, c_first);

        int kw = kw_first, c = c_first;
        for (int step = 0; step < nsteps; ++step) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            // prefetch the next step's tiles into the other buffers
            int kw_n = kw + 1, c_n = c;
            if (kw_n == Kw) { kw_n = 0; c_n = c + 1; }
            if (step + 1 < nsteps) {
                stage_w((step & 1) ? wbuf0 : wbuf1, kw_n, c_n);
                if (kw_n == 0) stage_x((c_n & 1) ? xbuf1 : xbuf0, c_n);
            }
            const char* wb = (step & 1) ? wbuf1 : wbuf0;
            const char* xb = (c & 1) ? xbuf1 : xbuf0;
            const char* A0 = wb + a_lane0;
            const char* A1 = wb + a_lane1;
            const int tsh = b_row0 + kw * d;             // LDS row of this lane's first B tile for this tap
            const int sw0 = ((ch0 ^ (tsh & 7)) << 4);
            const char* Bb = xb + (tsh << 7);
            const char* B0 = Bb + sw0;
            const char* B1 = Bb + (sw0 ^ CH1_XOR);       // bf16: chunk 4+fq == (chunk fq) ^ 4; e4m3: chunk 2fq+1
            // both k-substeps' fragments are requested up front (16 ds_read_b128 in flight); the second half lands
            // while the first half's MFMAs run.  sched_barrier pins that order against the register-pressure scheduler.
            bf16x8 a0[MS], b0[NS], a1[MS], b1[NS];
    #pragma unroll
            for (int mi = 0; mi < MS; ++mi) a0[mi] = *reinterpret_cast<const bf16x8*>(A0 + mi * 16 * ROWB);
    #pragma unroll
            for (int ni = 0; ni < NS; ++ni) b0[ni] = *reinterpret_cast<const bf16x8*>(B0 + ni * 16 * S * ROWB);
    #pragma unroll
            for (int mi = 0; mi < MS; ++mi) a1[mi] = *reinterpret_cast<const bf16x8*>(A1 + mi * 16 * ROWB);
    #pragma unroll
            for (int ni = 0; ni < NS; ++ni) b1[ni] = *reinterpret_cast<const bf16x8*>(B1 + ni * 16 * S * ROWB);
            if constexpr (F8) {
    #pragma unroll
                for (int mi = 0; mi < MS; ++mi)
    #pragma unroll
                    for (int ni = 0; ni < NS; ++ni)
                        acc[mi][ni] = mfma_e4m3_k128(a0[mi], a1[mi], b0[ni], b1[ni], acc[mi][ni]);
            } else {
    #pragma unroll
                for (int mi = 0; mi < MS; ++mi)
    #pragma unroll
                    for (int ni = 0; ni < NS; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[mi], b0[ni], acc[mi][ni], 0, 0, 0);
    #pragma unroll
                for (int mi = 0; mi < MS; ++mi)
    #pragma unroll
                    for (int ni = 0; ni < NS; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[mi], b1[ni], acc[mi][ni], 0, 0, 0);
                // schedule: ks0 fragment reads, then ks1 reads slotted one per MFMA into the ks0 MFMAs, then the rest
                __builtin_amdgcn_sched_group_barrier(0x100, MS + NS, 0);
    #pragma unroll
                for (int i = 0; i < MS + NS; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * MS * NS - (MS + NS), 0);
            }
            kw = kw_n;
            c = c_n;
        }

    } else {
        // fragments of k-substep ks (0/1) of the step whose weights sit in W buffer (stp & 1), for tap kk of chunk cc
        auto load_frags = [&](int ks, int stp, int cc, int kk, bf16x8* a, bf16x8* b) {
            const char* wb = (stp & 1) ? wbuf1 : wbuf0;
            const char* xb = (cc & 1) ? xbuf1 : xbuf0;
            const char* A = wb + (ks ? a_lane1 : a_lane0);
            const int tsh = b_row0 + kk * d;             // LDS row of this lane's first B tile for this tap
            const int sw0 = ((ch0 ^ (tsh & 7)) << 4);
            const char* B = xb + (tsh << 7) + (ks ? (sw0 ^ CH1_XOR) : sw0);      // chunk 4+fq == (chunk fq) ^ 4
            W2L_DIAG_SKIP_FRAGS(p, stp);
    #pragma unroll
            for (int mi = 0; mi < MS; ++mi) a[mi] = *reinterpret_cast<const bf16x8*>(A + mi * 16 * ROWB);
    #pragma unroll
            for (int ni = 0; ni < NS; ++ni) b[ni] = *reinterpret_cast<const bf16x8*>(B + ni * 16 * S * ROWB);
        };
        auto mfma_all = [&](const bf16x8* a, const bf16x8* b) {
            W2L_DIAG_SKIP_MFMA(p);
    #pragma unroll
            for (int mi = 0; mi < MS; ++mi)
    #pragma unroll
                for (int ni = 0; ni < NS; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        };
        // schedule of one half step: MS+NS fragment reads slotted one per MFMA into the first MFMAs, then the rest
        auto sched_half = [&]() {
    #pragma unroll
            for (int i = 0; i < MS + NS; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, MS * NS - (MS + NS), 0);
        };
        auto advance = [&](int kk, int cc, int& kk2, int& cc2) {
            kk2 = kk + 1;
            cc2 = cc;
            if (kk2 == Kw) { kk2 = 0; cc2 = cc + 1; }
        };

        // ---- K loop.  The block-wide barrier sits in the MIDDLE of a step: while the MFMAs of k-substep 1 run, the LDS-DMA
        // for step+2 is issued and the k-substep-0 fragments of step+1 are already being read, so neither the barrier
        // skew nor the first fragment reads of a step are exposed (they used to be, once per step, right after the barrier).
        //   top of step:  a0/b0 (substep 0 of this step) requested; DMA of step+1 in flight into the other buffers
        //   1. request a1/b1 (substep 1, same buffers), run the substep-0 MFMAs
        //   2. vmcnt(0) + barrier: every wave has finished READING this step's buffers, and step+1's tiles have landed
        //   3. DMA step+2 into this step's (now dead) buffers; request a0/b0 of step+1; run the substep-1 MFMAs
        stage_x((c_first & 1) ? xbuf1 : xbuf0, c_first);
        stage_w(wbuf0, kw_first, c_first);
        int kw = kw_first, c = c_first, kw_n, c_n;
        advance(kw, c, kw_n, c_n);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (nsteps > 1) {
            stage_w(wbuf1, kw_n, c_n);
            if (kw_n == 0) stage_x((c_n & 1) ? xbuf1 : xbuf0, c_n);
        }
        bf16x8 a0[MS], b0[NS], a1[MS], b1[NS];
        load_frags(0, 0, c, kw, a0, b0);
        W2L_DIAG_CLK_BEGIN();
        for (int step = 0; step + 1 < nsteps; ++step) {
            load_frags(1, step, c, kw, a1, b1);
            mfma_all(a0, b0);
            sched_half();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            int kw_nn, c_nn;
            advance(kw_n, c_n, kw_nn, c_nn);
            if (step + 2 < nsteps) {
                stage_w((step & 1) ? wbuf1 : wbuf0, kw_nn, c_nn);
                if (kw_nn == 0) stage_x((c_nn & 1) ? xbuf1 : xbuf0, c_nn);
            }
            load_frags(0, step + 1, c_n, kw_n, a0, b0);
            mfma_all(a1, b1);
            sched_half();
            kw = kw_n; c = c_n;
            kw_n = kw_nn; c_n = c_nn;
        }
        W2L_DIAG_CLK_END(tid);
        load_frags(1, nsteps - 1, c, kw, a1, b1);
        mfma_all(a0, b0);
        mfma_all(a1, b1);

    }

    // ---- split-K: publish the partial tile, draw a ticket; the last arriver sums all partials IN SPLIT ORDER (so the result
    // does not depend on which block arrived last) and goes on to the epilogue.  No block ever waits for another one.
    // (agent-scope release before the ticket, agent-scope acquire after it: correct for any placement of the blocks on XCDs)
    if (nsplit > 1) {
        float* slab = p.slabs + (slab_base + split) * (BM * BN);
#pragma unroll
        for (int mi = 0; mi < MS; ++mi)
#pragma unroll
            for (int ni = 0; ni < NS; ++ni)
                *reinterpret_cast<f32x4*>(slab + ((mi * NS + ni) * NT + tid) * 4) = acc[mi][ni];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                               // every wave's stores are issued and complete; main-loop LDS is dead
        unsigned* flag = reinterpret_cast<unsigned*>(smem);
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            *flag = __hip_atomic_fetch_add(&p.tickets[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        const unsigned ticket = *flag;
        if (ticket != (unsigned)(nsplit - 1)) continue;        // (not the last piece of this tile: on to the next tile, or out)
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(&p.tickets[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // clean for the next launch
        }
        __syncthreads();
        const float* base = p.slabs + slab_base * (BM * BN);
#pragma unroll
        for (int mi = 0; mi < MS; ++mi)
#pragma unroll
            for (int ni = 0; ni < NS; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < nsplit; ++sp) {
            const float* sl = base + (int64_t)sp * (BM * BN);
#pragma unroll
            for (int mi = 0; mi < MS; ++mi)
#pragma unroll
                for (int ni = 0; ni < NS; ++ni)
                    acc[mi][ni] += *reinterpret_cast<const f32x4*>(sl + ((mi * NS + ni) * NT + tid) * 4);
        }
        __syncthreads();                               // `flag` shares LDS with the statistics scratch below
    }

    // ---- epilogue: bias, optional accumulate, store, BatchNorm partial statistics ----
    // acc[mi][ni][r] = y[co = m0 + (wm*MS+mi)*16 + fq*4 + r][t = t0 + (wn*NS+ni)*16 + fr]
    const int Cout = p.Cout, Tout = p.Tout;
    const float descale = F8 ? p.descale * (EPI != 2 && p.descale_dev ? p.descale_dev[0] : 1.f) : 1.f;
    if constexpr (EPI == 2 && F8) {
        // ---- inference epilogue on e4m3 operands: the sequence of the bf16 form below on v = acc * descale + bias, stored as
        // e4m3 bytes a * fz_qscale (round to nearest even, saturating: quant8_e4m3's conversion, from the fp32 a) and, where
        // something reads it, as bf16.  A lane holds 4 channels of one frame = 4 bytes; the 4 lanes that share a frame (fq = 0..3)
        // hold the 16 channels of one MFMA tile, and G = 4 consecutive tiles (mi) are transposed among them with two lane
        // exchanges, so that lane fq stores the 16 bytes of tile mi0 + fq: 64 contiguous bytes per frame and store
        // instruction instead of 16 (G = 2, the remainder of MS = 6 / 3: 8 bytes per lane; G = 1: the plain dword).
        const int pl = p.fz_pad_l, pr = p.fz_pad_r;
        const int len_n = p.fz_lens ? p.fz_lens[n] : Tout;
        bf16_raw* const obase = p.fz_out ? p.fz_out + (int64_t)n * p.fz_rows * Cout : nullptr;
        uint8_t* const qbase = p.fz_q ? p.fz_q + (int64_t)n * p.fz_rows * Cout : nullptr;
        const float qs = p.fz_qscale, q_limit = 448.f / qs;
        unsigned clipped = 0;
        auto put = [&](int row, int co, u16x4 hi) { *reinterpret_cast<u16x4*>(obase + (int64_t)row * Cout + co) = hi; };
        auto group = [&](auto gc, const int mi0) {
            constexpr int G = decltype(gc)::value;
            typedef typename QVec<G>::type qvec;
            f32x4 bias4[G], sc4[G], sh4[G];
            bool co_ok[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int co = m0 + (wm * MS + mi0 + g) * 16 + fq * 4;
                co_ok[g] = co < Cout;
                bias4[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                sc4[g] = f32x4{1.f, 1.f, 1.f, 1.f};
                sh4[g] = bias4[g];
                if (p.bias && co_ok[g]) bias4[g] = *reinterpret_cast<const f32x4*>(p.bias + co);
                if (p.fz_scale && co_ok[g]) {
                    sc4[g] = *reinterpret_cast<const f32x4*>(p.fz_scale + co);
                    sh4[g] = *reinterpret_cast<const f32x4*>(p.fz_shift + co);
                }
            }
            // after the exchanges this lane holds G * 4 bytes of tile mi0 + (fq mod G), from byte (fq / G) * G * 4 of its 16
            const int co_q = m0 + (wm * MS + mi0 + (fq & (G - 1))) * 16 + (fq / G) * (G * 4);
            const bool coq_ok = co_q < Cout;
            auto putq = [&](int row, qvec v) { *reinterpret_cast<qvec*>(qbase + (int64_t)row * Cout + co_q) = v; };
#pragma unroll
            for (int ni = 0; ni < NS; ++ni) {
                const int tl = (wn * NS + ni) * 16 + fr;       // column inside the tile
                const int t = t0 + tl;
                unsigned q[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int co = m0 + (wm * MS + mi0 + g) * 16 + fq * 4;
                    const bool ok = co_ok[g] && t < Tout;
                    f32x4 v = acc[mi0 + g][ni] * descale + bias4[g];
                    v = v * sc4[g] + sh4[g];
                    if (p.fz_res && ok) {
                        const u16x4 rv = *reinterpret_cast<const u16x4*>(p.fz_res + ((int64_t)n * Tout + t) * Cout + co);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += bf16_bits_to_f32(rv[r]);
                    }
                    u16x4 hi;
                    float a[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        a[r] = v[r];
                        if (p.fz_act == 1) a[r] = fminf(fmaxf(a[r], 0.f), 20.f);
                        else if (p.fz_act == 2) a[r] = fmaxf(a[r], 0.f);
                        if (t >= len_n) a[r] = 0.f;
                        hi[r] = f32_to_bf16_bits(a[r]);
                        if (ok && fabsf(a[r]) > q_limit) ++clipped;
                        a[r] = fminf(fmaxf(a[r] * qs, -448.f), 448.f);
                    }
                    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
                    w = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], w, true);
                    q[g] = (unsigned)w;
                    if (obase && ok) {
                        put(pl + t, co, hi);
                        if (p.fz_pad_mode == 1) {              // nn.ReflectionPad1d: frame j is row pl - j, frame T-1-j row pl+T-1+j
                            if (t >= 1 && t <= pl) put(pl - t, co, hi);
                            const int j = Tout - 1 - t;
                            if (j >= 1 && j <= pr) put(pl + Tout - 1 + j, co, hi);
                        }
                    }
                    if (obase && p.fz_pad_mode != 1 && tt == 0 && co_ok[g]) {   // zero halo: the utterance's first tile
                        const u16x4 z = u16x4{0, 0, 0, 0};
                        if (tl < pl) put(tl, co, z);
                        if (tl < pr) put(pl + Tout + tl, co, z);
                    }
                }
                // transpose the G x G dwords among the lanes fq = 0..G-1 of this frame (every lane takes part: no branch here)
#pragma unroll
                for (int b = 1; b < G; b <<= 1) {
                    const bool up = (fq & b) != 0;
#pragma unroll
                    for (int i = 0; i < G; ++i) {
                        if (i & b) continue;
                        const unsigned send = up ? q[i] : q[i | b];
                        const unsigned recv = (unsigned)__shfl_xor((int)send, 16 * b, 64);
                        if (up) q[i] = recv; else q[i | b] = recv;
                    }
                }
                if (qbase) {
                    qvec qv = {}, z = {};
                    if constexpr (G == 1) {
                        qv = q[0];
                    } else {
#pragma unroll
                        for (int g = 0; g < G; ++g) qv[g] = q[g];
                    }
                    if (coq_ok && t < Tout) {
                        putq(pl + t, qv);
                        if (p.fz_pad_mode == 1) {
                            if (t >= 1 && t <= pl) putq(pl - t, qv);
                            const int j = Tout - 1 - t;
                            if (j >= 1 && j <= pr) putq(pl + Tout - 1 + j, qv);
                        }
                    }
                    if (p.fz_pad_mode != 1 && tt == 0 && coq_ok) {
                        if (tl < pl) putq(tl, z);
                        if (tl < pr) putq(pl + Tout + tl, z);
                    }
                }
            }
        };
#pragma unroll
        for (int g4 = 0; g4 < MS / 4; ++g4) group(std::integral_constant<int, 4>{}, g4 * 4);
        if constexpr ((MS & 3) >= 2) group(std::integral_constant<int, 2>{}, (MS / 4) * 4);
        if constexpr (MS & 1) group(std::integral_constant<int, 1>{}, MS - 1);
        if (p.fz_clip) {                               // one atomic per block, and only from a block that saw a saturation
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) clipped += __shfl_xor(clipped, m, 64);
            __syncthreads();                           // main-loop LDS is dead from here
            unsigned* red = reinterpret_cast<unsigned*>(smem);
            if (lane == 0) red[wave] = clipped;
            __syncthreads();
            if (tid == 0) {
                unsigned total = 0;
                for (int w = 0; w < NWAVES; ++w) total += red[w];
                if (total) atomicAdd(p.fz_clip, (unsigned long long)total);
            }
        }
    } else if constexpr (EPI == 2) {
        // ---- inference epilogue: v = act((acc + bias [+ y]) * scale + shift [+ residual]), masked, as bf16 into the consumer's
        // padded buffer.  Halo rows are written by the block that owns the frame they mirror (reflect), or by the first
        // column tile of the utterance (zeros): every pad is shorter than a tile (checked by the launcher).
        const int pl = p.fz_pad_l, pr = p.fz_pad_r;
        const int len_n = p.fz_lens ? p.fz_lens[n] : Tout;
        bf16_raw* const obase = p.fz_out + (int64_t)n * p.fz_rows * Cout;
        bf16_raw* const obase_lo = p.fz_out_lo ? p.fz_out_lo + (int64_t)n * p.fz_rows * Cout : nullptr;
        auto put = [&](int row, int co, u16x4 hi, u16x4 lo) {
            const int64_t o = (int64_t)row * Cout + co;
            *reinterpret_cast<u16x4*>(obase + o) = hi;
            if (obase_lo) *reinterpret_cast<u16x4*>(obase_lo + o) = lo;
        };
#pragma unroll
        for (int mi = 0; mi < MS; ++mi) {
            const int co = m0 + (wm * MS + mi) * 16 + fq * 4;
            const bool co_ok = co < Cout;
            f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f}, sc4 = f32x4{1.f, 1.f, 1.f, 1.f}, sh4 = bias4;
            if (p.bias && co_ok) bias4 = *reinterpret_cast<const f32x4*>(p.bias + co);
            if (p.fz_scale && co_ok) {
                sc4 = *reinterpret_cast<const f32x4*>(p.fz_scale + co);
                sh4 = *reinterpret_cast<const f32x4*>(p.fz_shift + co);
            }
#pragma unroll
            for (int ni = 0; ni < NS; ++ni) {
                const int tl = (wn * NS + ni) * 16 + fr;       // column inside the tile
                const int t = t0 + tl;
                const bool ok = co_ok && t < Tout;
                if (ok) {
                    const int64_t off = ((int64_t)n * Tout + t) * Cout + co;
                    f32x4 v = acc[mi][ni] + bias4;
                    if (p.accumulate) v += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.y) + off);
                    v = v * sc4 + sh4;
                    if (p.fz_res) {
                        const u16x4 rv = *reinterpret_cast<const u16x4*>(p.fz_res + off);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += bf16_bits_to_f32(rv[r]);
                        if (p.fz_res_lo) {
                            const u16x4 rl = *reinterpret_cast<const u16x4*>(p.fz_res_lo + off);
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] += bf16_bits_to_f32(rl[r]);
                        }
                    }
                    u16x4 hi, lo = u16x4{0, 0, 0, 0};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float a = v[r];
                        if (p.fz_act == 1) a = fminf(fmaxf(a, 0.f), 20.f);
                        else if (p.fz_act == 2) a = fmaxf(a, 0.f);
                        if (t >= len_n) a = 0.f;
                        hi[r] = f32_to_bf16_bits(a);
                        if (obase_lo) lo[r] = f32_to_bf16_bits(a - bf16_bits_to_f32(hi[r]));
                    }
                    put(pl + t, co, hi, lo);
                    if (p.fz_pad_mode == 1) {                  // nn.ReflectionPad1d: frame j is row pl - j, frame T-1-j row pl+T-1+j
                        if (t >= 1 && t <= pl) put(pl - t, co, hi, lo);
                        const int j = Tout - 1 - t;
                        if (j >= 1 && j <= pr) put(pl + Tout - 1 + j, co, hi, lo);
                    }
                }
                if (p.fz_pad_mode != 1 && tt == 0 && co_ok) {  // zero halo: the utterance's first tile writes both ends
                    const u16x4 z = u16x4{0, 0, 0, 0};
                    if (tl < pl) put(tl, co, z, z);
                    if (tl < pr) put(pl + Tout + tl, co, z, z);
                }
            }
        }
    } else {
    float s1[MS][4], s2[MS][4];
#pragma unroll
    for (int mi = 0; mi < MS; ++mi) {
        const int co = m0 + (wm * MS + mi) * 16 + fq * 4;
        const bool co_ok = co < Cout;
        f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.bias && co_ok) bias4 = *reinterpret_cast<const f32x4*>(p.bias + co);
#pragma unroll
        for (int r = 0; r < 4; ++r) { s1[mi][r] = 0.f; s2[mi][r] = 0.f; }
#pragma unroll
        for (int ni = 0; ni < NS; ++ni) {
            const int t = t0 + (wn * NS + ni) * 16 + fr;
            const bool ok = co_ok && t < Tout;
            f32x4 v = F8 ? acc[mi][ni] * descale + bias4 : acc[mi][ni] + bias4;
            const int64_t off = ((int64_t)n * Tout + t) * Cout + co;
            if (ok) {
                if (p.y_f32) {
                    float* yp = reinterpret_cast<float*>(p.y) + off;
                    if (p.accumulate) v += *reinterpret_cast<const f32x4*>(yp);
                    *reinterpret_cast<f32x4*>(yp) = v;
                } else {
                    u16x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16_bits(v[r]);
                    *reinterpret_cast<u16x4*>(reinterpret_cast<bf16_raw*>(p.y) + off) = o;
                }
                if constexpr (EPI == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) { s1[mi][r] += v[r]; s2[mi][r] += v[r] * v[r]; }
                }
            }
        }
    }
    if constexpr (EPI == 1) {
        // ---- BatchNorm-backward sums of the layer that produced this conv's input (see IgemmParams).  Flat output row t is
        // padded row u of utterance nu; its gradient belongs to source frame ts (itself, or its mirror image when the row is
        // a reflected halo row -- the fold of bn_act.hip add_grad8 is linear, so every padded row simply counts with its
        // source frame's gate and xhat).  The y / mask loads of CH channel blocks are issued together, from clamped (always
        // valid) addresses and outside any branch, so they overlap instead of forming one dependent chain per element.
        int64_t yrow[NS];
        bool live[NS];
#pragma unroll
        for (int ni = 0; ni < NS; ++ni) {
            const int t = t0 + (wn * NS + ni) * 16 + fr;
            const int tc = t < Tout ? t : Tout - 1;
            const int nu = (int)((unsigned)tc / (unsigned)p.bn_per);
            const int u = tc - nu * p.bn_per;
            int ts = u - p.bn_pad_l;
            bool lv = t < Tout && u < p.bn_Tp;
            if (ts < 0 || ts >= p.bn_T) {
                if (p.bn_pad_mode == 1) ts = ts < 0 ? -ts : 2 * (p.bn_T - 1) - ts;
                else lv = false;
            }
            ts = ts < 0 ? 0 : (ts >= p.bn_T ? p.bn_T - 1 : ts);
            if (lv && p.bn_lens && ts >= p.bn_lens[nu]) lv = false;          // masked frame: no gradient through it
            live[ni] = lv;
            yrow[ni] = (int64_t)nu * p.bn_T + ts;
        }
        constexpr int CH = MS % 4 == 0 ? 4 : (MS % 2 == 0 ? 2 : 1);
        __syncthreads();                               // main-loop LDS is dead from here: the sums go straight into it
        float* red = reinterpret_cast<float*>(smem);   // [NW][2][BM]
#pragma unroll
        for (int m0i = 0; m0i < MS; m0i += CH) {
            u16x4 yv[CH][NS];
            unsigned mb[CH][NS];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                int co = m0 + (wm * MS + m0i + c) * 16 + fq * 4;
                co = co < Cout ? co : Cout - 4;
#pragma unroll
                for (int ni = 0; ni < NS; ++ni) {
                    yv[c][ni] = *reinterpret_cast<const u16x4*>(p.bn_y + yrow[ni] * Cout + co);
                    mb[c][ni] = p.bn_mask ? (unsigned)p.bn_mask[yrow[ni] * (Cout >> 3) + (co >> 3)] : 0xFFu;
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int mi = m0i + c;
                const int co = m0 + (wm * MS + mi) * 16 + fq * 4;
                const bool co_ok = co < Cout;
                const int cc = co_ok ? co : Cout - 4;
                f32x4 bsc = f32x4{1.f, 1.f, 1.f, 1.f}, bsh = f32x4{0.f, 0.f, 0.f, 0.f}, bmu = bsh, bis = bsh;
                if (p.bn_scale) { bsc = *reinterpret_cast<const f32x4*>(p.bn_scale + cc); bsh = *reinterpret_cast<const f32x4*>(p.bn_shift + cc); }
                if (p.bn_mean) { bmu = *reinterpret_cast<const f32x4*>(p.bn_mean + cc); bis = *reinterpret_cast<const f32x4*>(p.bn_invstd + cc); }
#pragma unroll
                for (int ni = 0; ni < NS; ++ni) {
                    const bool on = live[ni] && co_ok;
                    const unsigned bits = mb[c][ni] >> (co & 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float yf = bf16_bits_to_f32(yv[c][ni][r]);
                        const bool keep = (bits >> r) & 1u;
                        float z = yf * bsc[r] + bsh[r];
                        z = keep ? z * p.bn_gk : 0.f;
                        bool pass = keep && on;
                        if (p.bn_act == 1) pass = pass && z >= 0.f && z <= 20.f;
                        else if (p.bn_act == 2) pass = pass && z > 0.f;
                        const float g = pass ? acc[mi][ni][r] * p.bn_gk : 0.f;
                        s1[mi][r] += g;
                        s2[mi][r] += g * ((yf - bmu[r]) * bis[r]);
                    }
                }
                // this channel block is complete: combine the 16 column lanes and park the sums in LDS right away (keeping
                // all MS blocks' sums in registers next to the accumulators spills)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float a = s1[mi][r], b = s2[mi][r];
#pragma unroll
                    for (int m = 1; m < 16; m <<= 1) {
                        a += __shfl_xor(a, m, 64);
                        b += __shfl_xor(b, m, 64);
                    }
                    if (fr == 0) {
                        const int cl = (wm * MS + mi) * 16 + fq * 4 + r;
                        red[(wn * 2 + 0) * BM + cl] = a;
                        red[(wn * 2 + 1) * BM + cl] = b;
                    }
                }
            }
        }
    }
    if (p.stats) {
        // statistics rows are laid out per 128-column tile (w2l_conv_stat_tiles); a 256-column block owns two
        constexpr int HALVES = BN / 128;
        constexpr int WPH = NW / HALVES;               // N-waves per 128-column half
        static_assert(BN % 128 == 0 || true, "");
        float* red = reinterpret_cast<float*>(smem);   // [NW][2][BM]
        if constexpr (EPI == 0) {
            __syncthreads();                           // main-loop LDS is dead from here
#pragma unroll
            for (int mi = 0; mi < MS; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float a = s1[mi][r], b = s2[mi][r];
#pragma unroll
                    for (int m = 1; m < 16; m <<= 1) {
                        a += __shfl_xor(a, m, 64);
                        b += __shfl_xor(b, m, 64);
                    }
                    if (fr == 0) {
                        const int cl = (wm * MS + mi) * 16 + fq * 4 + r;
                        red[(wn * 2 + 0) * BM + cl] = a;
                        red[(wn * 2 + 1) * BM + cl] = b;
                    }
                }
        }
        __syncthreads();
        if (p.stats_slots) {
            // w2l_conv_stats_mode(S): the block's sums -- all its NW column waves, whatever the block shape -- ADDED onto row
            // (column tile mod S) of the zero-filled [S][2][Cout] buffer; its reader re-reduces the S rows
            float* dst = p.stats + (((int64_t)n * p.tiles_t + tt) % p.stats_slots) * 2 * Cout;
            for (int cl = tid; cl < BM; cl += NT) {
                if (m0 + cl < Cout) {
                    float a = 0.f, b = 0.f;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        a += red[(w * 2 + 0) * BM + cl];
                        b += red[(w * 2 + 1) * BM + cl];
                    }
                    atomicAdd(dst + m0 + cl, a);
                    atomicAdd(dst + Cout + m0 + cl, b);
                }
            }
        } else {
        const int tiles128 = (Tout + 127) / 128;
        for (int idx = tid; idx < BM * HALVES; idx += NT) {
            const int h = idx / BM, cl = idx - h * BM;
            const int trow = tt * HALVES + h;          // 128-column tile index inside the utterance
            if (m0 + cl < Cout && trow < tiles128) {
                float a = 0.f, b = 0.f;
#pragma unroll
                for (int w = 0; w < WPH; ++w) {
                    a += red[((h * WPH + w) * 2 + 0) * BM + cl];
                    b += red[((h * WPH + w) * 2 + 1) * BM + cl];
                }
                const int64_t srow = (int64_t)n * tiles128 + trow;
                float* dst = p.stats + srow * 2 * Cout;
                dst[m0 + cl] = a;
                dst[Cout + m0 + cl] = b;
            }
        }
        }
    }
    }
    } while (SK && w_cur < w_end);
}

struct TileCfg { int mw, nw, ms, ns; float eff; };
// candidate block shapes (BM = 16*mw*ms output channels x BN = 16*nw*ns time rows) with their measured
// relative MFMA efficiency at full occupancy (tools/bench_conv.py --sweep, MI355X)
constexpr TileCfg kCfgs[] = {
    {2, 2, 2, 4, 0.83f}, {2, 2, 3, 4, 1.00f}, {2, 2, 4, 4, 1.00f}, {2, 2, 5, 4, 1.01f},   // BN 128, 4 waves
    {4, 2, 3, 4, 0.90f}, {4, 2, 4, 4, 0.92f},                                               // BN 128, 8 waves
    {2, 3, 2, 3, 0.80f}, {2, 3, 3, 3, 0.97f}, {2, 3, 4, 3, 0.97f}, {2, 3, 5, 3, 0.98f},   // BN 144, 6 waves
    {2, 4, 2, 4, 0.85f}, {2, 4, 3, 4, 0.97f}, {2, 4, 4, 4, 1.00f}, {2, 4, 5, 4, 1.04f},   // BN 256, 8 waves, 1 block/CU
    {2, 4, 6, 4, 1.10f}, {2, 4, 7, 4, 1.06f}, {2, 4, 8, 4, 1.12f},
    {2, 3, 4, 6, 1.00f}, {2, 3, 5, 6, 1.00f}, {2, 3, 6, 6, 1.00f}, {2, 3, 7, 6, 1.00f},   // BN 288, 6 waves, 1 block/CU
    // BN 384, 8 waves (round 3): a weight tile serves 384 columns instead of 256 -- a third less LDS-DMA per MFMA, the
    // instruction a K step spends a third of its issue time on (in-kernel stamps).  Useful where the column count
    // tiles well: the flat data gradients of the 640-wide layers +12-14 %, 768-wide +1-4 %; never the per-utterance forward
    // pass (500 columns = 2 tiles of 384)
    {2, 4, 4, 6, 1.00f}, {2, 4, 5, 6, 1.00f}, {2, 4, 6, 6, 1.00f},
    {2, 4, 4, 7, 1.00f}, {2, 4, 5, 7, 1.00f},                                               // BN 448, 8 waves
};
constexpr int kNumCfgs = sizeof(kCfgs) / sizeof(kCfgs[0]);
constexpr int kSpillCfg = 20;                           // 2x3x7x6 spills: never chosen, kept only for index stability

constexpr size_t kLdsBytes = 160 * 1024;                // LDS of a CU
constexpr int kCUs = 256;
constexpr size_t kTicketBytes = 64 * 1024;              // head of the split-K workspace: one counter per output tile
constexpr int kFzMaxPad = 96;                           // halo rows a fused tile writes: fewer than the narrowest tile's columns
// waves a CU holds of these kernels: <= 16 at their VGPR budget -- what the cost model and the tuner's split-K filter count
// with; a stream-K launch sizes its grid with eight (what two 4-wave blocks hold), one or two blocks per CU
constexpr int kWaveCap = 16, kSkWaveCap = 8;

// ---- what a launch is asked to do: the problem, and the epilogue fused onto it ----
struct ConvProblem {                                    // (in the order of the entry points' arguments)
    const void* x;
    int64_t x_bstride, x_rows_total;
    const void* w;
    void* y;
    int y_f32, accumulate;
    const float* bias;
    float* stats;
    int N, Cin, Cout, Tout, Kw, stride, dil;
    void* ws;                                           // split-K workspace or NULL
    int64_t ws_bytes;
    hipStream_t stream;
    bool f8 = false;                                    // e4m3 operands: stride 1, no workspace
    float descale = 1.f;
    const float* descale_dev = nullptr;
    int stats_slots = 0;                                // w2l_conv_stats_mode, where stats is given (set by run())
};

enum EpiKind { kEpiNone = 0, kEpiBnReduce, kEpiInfer, kEpiInferF8 };
struct Epilogue {
    EpiKind kind;
    struct { const w2l_bnact_t* d; int pad_l, pad_r, pad_mode, per; } bn;       // kEpiBnReduce (w2l_conv1d_dgrad_bnreduce_ws)
    const w2l_bnact_epi_t* fz;                                                  // kEpiInfer / kEpiInferF8
    void* out_q;                                                                // kEpiInferF8: the e4m3 output ...
    float q_scale;
    int64_t* q_clipped;                                                         // ... and its saturation counter
};
constexpr Epilogue kNoEpilogue{};
static inline bool is_infer(const Epilogue* ep) { return ep->kind == kEpiInfer || ep->kind == kEpiInferF8; }

// statistics flag of a shape key: 0 none, 1 one row per 128-column tile (block shapes of 128 / 256 columns only), 2 added onto
// slot rows (w2l_conv_stats_mode: every block shape; bf16 only)
// 3: a fused inference launch (w2l_conv1d_igemm_bnact[_fp8]) -- measured, remembered and looked up as itself; split-K forms
// included (the combining block runs the epilogue), stream-K forms not
static int stats_flag(const ConvProblem& pr, const Epilogue* ep) {
    if (is_infer(ep)) return 3;
    return pr.stats == nullptr ? 0 : (!pr.f8 && pr.stats_slots > 0 ? 2 : 1);
}

// ---- the geometry of one block shape on one problem ----
struct TileGeom {
    int bm, bn, xrows, waves, tiles_m, tiles_t;
    size_t lds;
    int64_t blocks;                                     // one block per output tile
};
static TileGeom tile_geom(const TileCfg& c, const ConvProblem& pr) {
    TileGeom g;
    g.bm = 16 * c.mw * c.ms;
    g.bn = 16 * c.nw * c.ns;
    g.xrows = ((g.bn - 1) * pr.stride + (pr.Kw - 1) * pr.dil + 1 + 7) & ~7;
    g.waves = c.mw * c.nw;
    g.tiles_m = (pr.Cout + g.bm - 1) / g.bm;
    g.tiles_t = (pr.Tout + g.bn - 1) / g.bn;
    g.lds = 2 * (size_t)g.bm * ROWB + 2 * (size_t)g.xrows * ROWB;
    g.blocks = (int64_t)g.tiles_m * pr.N * g.tiles_t;
    return g;
}
// a problem of which only the window matters (feasibility of a block shape)
static ConvProblem window_only(int Kw, int stride, int dil) {
    ConvProblem pr{};
    pr.Kw = Kw; pr.stride = stride; pr.dil = dil;
    return pr;
}
static int blocks_per_cu(const TileGeom& g, int wave_cap) {
    const int by_lds = (int)(kLdsBytes / g.lds), by_waves = wave_cap / g.waves;
    const int per_cu = by_lds < by_waves ? by_lds : by_waves;
    return per_cu < 1 ? 1 : per_cu;
}
// fill of the last round when `blocks` blocks run `slots` at a time
static double last_round_fill(int64_t blocks, int64_t slots) {
    return (double)blocks / (double)(((blocks + slots - 1) / slots) * slots);
}
// BatchNorm partial statistics are per 128-column tile: the epilogue assumes whole waves per tile
static bool bn128_ok(const TileGeom& g) { return g.bn % 128 == 0 && g.bn <= 256; }

// the cost model: time ~ rounds of resident blocks on the CUs x (work per block) x (blocks sharing a CU) / efficiency, larger
// tiles preferred.  low_occ: factor on the efficiency with fewer than 8 waves per CU; tie: stable tie-break
static double tile_cost(const TileGeom& g, float eff, double low_occ, int tie) {
    const int per_cu = blocks_per_cu(g, kWaveCap);
    const int64_t slots = (int64_t)kCUs * per_cu, rounds = (g.blocks + slots - 1) / slots;
    const double e = eff * (per_cu * g.waves >= 8 ? 1.0 : low_occ);
    double cost = (double)rounds * g.bm * g.bn * per_cu / e;
    cost *= 1.0 + 1e-3 * tie;
    return cost;
}

// ---- a planned launch: everything host arithmetic decides, and the kernel's argument ----
struct ConvPlan {
    int idx;                                            // configuration index (bf16: see kSplits; e4m3: into kF8Cfgs)
    int shape, pipe, splits, sk_ranges;                 // kCfgs row, K-loop structure, blocks per tile, stream-K blocks or 0
    int epi;                                            // the kernel's EPI
    bool f8;
    unsigned grid, threads;
    size_t lds;
    hipStream_t stream;
    IgemmParams p;
};

template <typename K>
int launch_kernel(K kern, const ConvPlan& pl) {
    W2L_CHECK_HIP(w2l_allow_big_lds((const void*)kern));
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(pl.threads), pl.lds, pl.stream, pl.p);
    W2L_CHECK_LAUNCH();
    return 0;
}

template <int MW, int NW, int MS, int NS, int PIPE>
int launch_cfg1(const ConvPlan& pl) {
    constexpr bool k128x128 = MW == 2 && NW == 2 && MS == 4 && NS == 4;          // the one shape with stride-2 forms
    if (pl.epi == 1) {
        // statistics rows are per 128-column tile -- unless the sums are added onto slot rows (w2l_conv_stats_mode): any shape then
        if ((16 * NW * NS) % 128 == 0 && 16 * NW * NS <= 256 ? true : pl.p.stats_slots > 0)
            return launch_kernel(conv_igemm_kernel<MW, NW, MS, NS, 1, PIPE, false, 1>, pl);
        w2l_set_error("conv1d_igemm: the fused BatchNorm-backward epilogue needs a block shape of 128-column tiles");
        return 1;
    }
    if (pl.p.stride == 2 && !k128x128) {
        w2l_set_error("conv1d_igemm: stride 2 is only built for the 128x128 block shape");
        return 1;
    }
    if (pl.epi == 2) {
        if constexpr (k128x128)
            if (pl.p.stride == 2) return launch_kernel(conv_igemm_kernel<2, 2, 4, 4, 2, PIPE, false, 2>, pl);
        return launch_kernel(conv_igemm_kernel<MW, NW, MS, NS, 1, PIPE, false, 2>, pl);
    }
    if constexpr (k128x128)
        if (pl.p.stride == 2) return launch_kernel(conv_igemm_kernel<2, 2, 4, 4, 2, PIPE>, pl);
    if (pl.sk_ranges > 0) return launch_kernel(conv_igemm_kernel<MW, NW, MS, NS, 1, PIPE, false, 0, true>, pl);
    return launch_kernel(conv_igemm_kernel<MW, NW, MS, NS, 1, PIPE>, pl);
}

template <int MW, int NW, int MS, int NS>
int launch_cfg(const ConvPlan& pl) {
    return pl.pipe ? launch_cfg1<MW, NW, MS, NS, 1>(pl) : launch_cfg1<MW, NW, MS, NS, 0>(pl);
}

// e4m3 launches: K-loop structure 0, stride 1, a subset of the block shapes (indices into kCfgs); a configuration index of the
// e4m3 kernel is an index into this list
constexpr int kF8Cfgs[] = {2, 5, 12, 14, 16, 1, 3, 8, 9, 11, 13, 18, 19, 21, 24};     // (the first five were round 2's first set;
                                                                              //  21 / 24: the 384- / 448-column shapes, round 3)
constexpr int kNumF8Cfgs = sizeof(kF8Cfgs) / sizeof(kF8Cfgs[0]);

// block shapes the fused e4m3 form (EPI = 2) is built for: all of kF8Cfgs but the four whose epilogue spills next to 96 or more
// accumulator registers -- 2x4x6x4 (2 VGPRs), 2x4x8x4 (35), 2x3x5x6 (68), 2x3x6x6 (85)
constexpr bool f8_fused_built(int nw, int ms, int ns) { return !((ms == 6 && ns == 4) || ms == 8 || (nw == 3 && ns == 6)); }

template <int MW, int NW, int MS, int NS>
int launch_f8(const ConvPlan& pl) {
    if (pl.epi == 2) {
        if constexpr (f8_fused_built(NW, MS, NS)) {
            return launch_kernel(conv_igemm_kernel<MW, NW, MS, NS, 1, 0, true, 2>, pl);
        } else {
            w2l_set_error("conv1d_igemm_bnact_fp8: block shape not built for the fused epilogue");
            return 1;
        }
    }
    return launch_kernel(conv_igemm_kernel<MW, NW, MS, NS, 1, 0, true>, pl);
}

// index -> instantiation, generated from kCfgs (and kF8Cfgs) themselves: a row of the table IS the template arguments
typedef int (*LaunchFn)(const ConvPlan&);
template <int I> constexpr LaunchFn kLaunchCfg = &launch_cfg<kCfgs[I].mw, kCfgs[I].nw, kCfgs[I].ms, kCfgs[I].ns>;
template <int I> constexpr LaunchFn kLaunchF8 = &launch_f8<kCfgs[I].mw, kCfgs[I].nw, kCfgs[I].ms, kCfgs[I].ns>;
template <size_t... I>
constexpr std::array<LaunchFn, sizeof...(I)> cfg_launchers(std::index_sequence<I...>) { return {{kLaunchCfg<(int)I>...}}; }
template <size_t... K>
constexpr std::array<LaunchFn, sizeof...(K)> f8_launchers(std::index_sequence<K...>) { return {{kLaunchF8<kF8Cfgs[K]>...}}; }
constexpr auto kCfgLaunchers = cfg_launchers(std::make_index_sequence<kNumCfgs>{});
constexpr auto kF8Launchers = f8_launchers(std::make_index_sequence<kNumF8Cfgs>{});

int launch(const ConvPlan& pl) { return (pl.f8 ? kF8Launchers[pl.idx] : kCfgLaunchers[pl.shape])(pl); }

}  // namespace

// A configuration index is (block shape) + kNumCfgs * (K-loop structure PIPE) + 2 * kNumCfgs * (split-K option).
// Split option 0 = stream-K (round 5): one block per resident slot, each an equal share of ALL the launch's (tile, step) pairs
constexpr int kSplits[] = {1, 2, 3, 4, 5, 6, 8, 0};
constexpr int kNumSplits = sizeof(kSplits) / sizeof(kSplits[0]);
constexpr int kMaxSplit = 8;
constexpr int kSkMinSteps = 8;                          // a stream-K range is at least this many steps
constexpr int kBaseCfgs = 2 * kNumCfgs;
// the three per-thread hooks of the ABI, each read in one place (run()).  thread-local: a forced configuration holds for
// launches made by the CALLING thread only -- a backward running on an autograd worker thread never sees another thread's
static thread_local int g_force_cfg = -1;
static thread_local int g_force_f8 = -1;
static thread_local int g_stats_slots = 0;
extern "C" void w2l_conv_stats_mode(int slots) { g_stats_slots = slots < 0 ? 0 : (slots > 64 ? 64 : slots); }
extern "C" void w2l_conv_force_tile_config(int idx) { g_force_cfg = idx; }
// testing / profiling hook (per calling thread): pin the e4m3 kernel's block shape (index into kF8Cfgs), -1 = automatic
extern "C" void w2l_conv_force_fp8_config(int idx) { g_force_f8 = idx; }
W2L_DIAG_IGEMM_EXPORTS

// measured choices (the _tune entry points): shape -> configuration index; the e4m3 kernel's in a table of its own (same key,
// stride always 1, value = index into kF8Cfgs)
typedef std::tuple<int, int, int, int, int, int, int, int> ShapeKey;
static std::map<ShapeKey, int> g_tuned, g_tuned_f8;
static std::mutex g_tuned_mu;
static ShapeKey shape_key(const ConvProblem& pr, int sflag) {
    return ShapeKey(pr.N, pr.Cin, pr.Cout, pr.Tout, pr.Kw, pr.stride, pr.dil, sflag);
}

static bool cfg_feasible(int idx, const ConvProblem& pr, int sflag) {
    if (idx < 0 || idx >= kBaseCfgs * kNumSplits) return false;
    const int i = idx % kNumCfgs;
    const TileGeom g = tile_geom(kCfgs[i], pr);
    if (sflag == 1 && !bn128_ok(g)) return false;
    if (pr.stride != 1 && i != 2) return false;             // strided convs (first layer only) use the 128x128 shape
    if (i == kSpillCfg) return false;
    return g.lds <= kLdsBytes;
}

static bool f8_feasible(int k, const ConvProblem& pr, int sflag) {
    if (k < 0 || k >= kNumF8Cfgs) return false;
    const TileCfg& c = kCfgs[kF8Cfgs[k]];
    const TileGeom g = tile_geom(c, pr);
    if (sflag == 3 && (!f8_fused_built(c.nw, c.ms, c.ns) || g.bn <= kFzMaxPad)) return false;   // (a tile writes the halo
                                                                                // rows: every pad is shorter than it)
    if (sflag == 1 && !bn128_ok(g)) return false;
    return g.lds <= kLdsBytes;
}

// pick the configuration: the forced one, else a measured choice if this shape was tuned, else the cost model (which only
// ranks the PIPE = 0, one-block-per-tile variants).  -1: nothing fits
static int choose_cfg(const ConvProblem& pr, int sflag, int forced) {
    if (forced >= 0) return (pr.f8 ? f8_feasible(forced, pr, sflag) : cfg_feasible(forced, pr, sflag)) ? forced : -1;
    {
        std::lock_guard<std::mutex> lock(g_tuned_mu);
        const auto& tuned = pr.f8 ? g_tuned_f8 : g_tuned;
        auto it = tuned.find(shape_key(pr, sflag));
        if (it != tuned.end()) return it->second;
    }
    int best = -1;
    double best_cost = 1e30;
    for (int k = 0; k < (pr.f8 ? kNumF8Cfgs : kNumCfgs); ++k) {
        if (!(pr.f8 ? f8_feasible(k, pr, sflag) : cfg_feasible(k, pr, sflag))) continue;
        const TileCfg& c = kCfgs[pr.f8 ? kF8Cfgs[k] : k];
        const double cost = tile_cost(tile_geom(c, pr), c.eff, pr.f8 ? 1.0 : 0.75, k);
        if (cost < best_cost) { best_cost = cost; best = k; }
    }
    return best;
}

extern "C" int w2l_conv_stat_tiles(int N, int Tout) { return N * ((Tout + 127) / 128); }

// bytes of split-K workspace for `splits` slabs per tile (+ the tickets)
static size_t splitk_bytes(const TileGeom& g, int splits) {
    return kTicketBytes + (size_t)g.blocks * splits * g.bm * g.bn * sizeof(float);
}

// blocks of a stream-K launch of this shape: the slots the chip has for it (one or two blocks per CU)
static int sk_ranges(const TileGeom& g) { return kCUs * blocks_per_cu(g, kSkWaveCap); }

static bool sk_feasible(const TileGeom& g, const ConvProblem& pr) {
    if (pr.ws == nullptr || pr.stride != 1) return false;
    const int64_t tiles = g.blocks, steps = (int64_t)(pr.Cin / BK) * pr.Kw, G = sk_ranges(g);
    if (tiles * steps / G < kSkMinSteps || (tiles * steps + steps) * G >= (1LL << 31)) return false;
    return tiles * (int64_t)sizeof(unsigned) <= (int64_t)kTicketBytes &&
           (int64_t)kTicketBytes + (tiles + G) * g.bm * g.bn * (int64_t)sizeof(float) <= pr.ws_bytes;
}

static bool split_feasible(const TileGeom& g, int splits, const ConvProblem& pr) {
    if (splits == 1) return true;
    if (pr.ws == nullptr || (pr.Cin / BK) * pr.Kw < 2 * splits) return false;
    return (size_t)g.blocks * sizeof(unsigned) <= kTicketBytes && splitk_bytes(g, splits) <= (size_t)pr.ws_bytes;
}

// the fused inference descriptor, as the bf16 and the e4m3 launch both need it
static int check_infer_epi(const w2l_bnact_epi_t* e, int Tout, const char* who) {
    W2L_CHECK_ARG(e->pad_l >= 0 && e->pad_r >= 0 && e->pad_l <= kFzMaxPad && e->pad_r <= kFzMaxPad &&
                  e->out_rows >= e->pad_l + Tout + e->pad_r,
                  "%s: bad output geometry (pads %d,%d of at most %d; %d rows for %d frames)", who, e->pad_l, e->pad_r,
                  kFzMaxPad, e->out_rows, Tout);
    W2L_CHECK_ARG(e->pad_mode != 1 || (e->pad_l < Tout && e->pad_r < Tout), "%s: reflect pad (%d,%d) needs pad < T=%d", who,
                  e->pad_l, e->pad_r, Tout);
    W2L_CHECK_ARG((e->scale == nullptr) == (e->shift == nullptr) && e->act >= 0 && e->act <= 2 && (e->res || !e->res_lo),
                  "%s: scale/shift come together, act is 0..2, res_lo needs res", who);
    return 0;
}

// Everything a launch decides on the host: checks the problem and its epilogue, picks the configuration (`forced` >= 0: that
// one or an error), sizes the grid and fills the kernel's argument.  No HIP call, no state but the table of measured choices.
static int plan(const ConvProblem& pr, const Epilogue* ep, int forced, ConvPlan& pl) {
    const char* who = pr.f8 ? "conv1d_igemm_fp8" : "conv1d_igemm";
    W2L_CHECK_ARG(pr.x && pr.w && (pr.y || is_infer(ep)), "%s: null pointer", who);
    W2L_CHECK_ARG(pr.f8 ? ep->kind == kEpiNone || ep->kind == kEpiInferF8 : ep->kind != kEpiInferF8,
                  "%s: epilogue of the other operand type", who);
    W2L_CHECK_ARG(pr.N > 0 && pr.Tout > 0 && pr.Kw > 0 && (pr.stride == 1 || (pr.stride == 2 && !pr.f8)) && pr.dil > 0,
                  "%s: bad sizes (stride must be 1 or 2; e4m3: 1)", who);
    const int cin_unit = pr.f8 ? 128 : 64;
    W2L_CHECK_ARG(pr.Cin % cin_unit == 0 && pr.Cin > 0, "%s: Cin=%d must be a positive multiple of %d", who, pr.Cin, cin_unit);
    W2L_CHECK_ARG(pr.Cout % 64 == 0 && pr.Cout > 0, "%s: Cout=%d must be a positive multiple of 64", who, pr.Cout);
    W2L_CHECK_ARG(pr.x_bstride % pr.Cin == 0, "%s: x_bstride must be a multiple of Cin", who);
    W2L_CHECK_ARG(!(pr.accumulate && !pr.y_f32), "%s: accumulate needs fp32 output", who);
    W2L_CHECK_ARG(pr.descale > 0.f, "%s: descale must be positive", who);
    IgemmParams& p = pl.p;
    p.x = (const bf16_raw*)pr.x;
    p.w = (const bf16_raw*)pr.w;
    p.y = pr.y;
    p.bias = pr.bias;
    p.stats = pr.stats;
    p.stats_slots = pr.stats ? pr.stats_slots : 0;
    p.x_rows_per_utt = pr.x_bstride / pr.Cin;
    p.x_max_row = pr.x_rows_total - 1;
    p.N = pr.N; p.Cin = pr.Cin; p.Cout = pr.Cout; p.Tout = pr.Tout; p.Kw = pr.Kw; p.stride = pr.stride; p.dil = pr.dil;
    p.y_f32 = pr.y_f32; p.accumulate = pr.accumulate;
    p.descale = pr.descale;
    p.descale_dev = pr.descale_dev;
    pl.epi = 0;
    if (ep->kind == kEpiBnReduce) {
        const w2l_bnact_t* d = ep->bn.d;
        const int pad_l = ep->bn.pad_l, pad_r = ep->bn.pad_r, per = ep->bn.per;
        W2L_CHECK_ARG(d && d->y && !d->y_f32 && !d->y2 && pr.stats && !pr.y_f32 && !pr.accumulate && !pr.bias && pr.N == 1 &&
                      pr.stride == 1,
                      "conv1d_dgrad_bnreduce: needs a bf16 single-branch layer, a statistics buffer and a flat bf16 output");
        // flat_rows == N * per exactly: the epilogue derives the utterance of a row as row / per with no upper limit, so a row
        // beyond N * per would be counted with the y, mask and lens of an utterance that does not exist
        W2L_CHECK_ARG(d->C == pr.Cout && per > 0 && pad_l >= 0 && pad_r >= 0 && d->N > 0 && (int64_t)d->N * per == pr.Tout &&
                      per >= pad_l + d->T + pad_r,
                      "conv1d_dgrad_bnreduce: geometry mismatch (C=%d vs %d, per=%d, N=%d, rows=%d)", d->C, pr.Cout, per, d->N,
                      pr.Tout);
        W2L_CHECK_ARG(d->drop_p == 0.f || d->mask, "conv1d_dgrad_bnreduce: dropout needs the recorded mask");
        p.bn_y = (const bf16_raw*)d->y;
        p.bn_scale = d->scale; p.bn_shift = d->shift; p.bn_mean = d->mean; p.bn_invstd = d->invstd;
        p.bn_mask = d->drop_p > 0.f ? d->mask : nullptr;
        p.bn_lens = d->lens;
        p.bn_T = d->T; p.bn_pad_l = pad_l; p.bn_pad_mode = ep->bn.pad_mode; p.bn_per = per;
        p.bn_Tp = pad_l + d->T + pad_r;
        p.bn_act = d->act;
        p.bn_gk = d->drop_p > 0.f ? 1.f / (1.f - d->drop_p) : 1.f;
        pl.epi = 1;
    } else if (is_infer(ep)) {
        const w2l_bnact_epi_t* e = ep->fz;
        const bool q = ep->kind == kEpiInferF8 && ep->out_q != nullptr;
        const char* who_fz = pr.f8 ? "conv1d_igemm_bnact_fp8" : "conv1d_igemm_bnact";
        if (pr.f8) {                                    // the e4m3-only conditions
            W2L_CHECK_ARG(e && (e->out_hi || q) && !e->out_lo && !e->res_lo && !pr.y && !pr.stats && !pr.descale_dev,
                          "conv1d_igemm_bnact_fp8: needs an e4m3 or a bf16 output and takes no lo halves");
            W2L_CHECK_ARG(!q || (ep->q_scale > 0.f && ((uintptr_t)ep->out_q & 15) == 0),
                          "conv1d_igemm_bnact_fp8: the e4m3 output needs a positive scale and 16-byte alignment");
        } else {
            W2L_CHECK_ARG(e && pr.stats == nullptr && e->out_hi, "conv1d_igemm_bnact: null output / bad combination");
        }
        if (int rc = check_infer_epi(e, pr.Tout, who_fz)) return rc;
        p.stats_slots = 0;
        p.fz_q = q ? (uint8_t*)ep->out_q : nullptr;     // (shares storage with stats / descale_dev, both NULL here)
        p.fz_qscale = q ? ep->q_scale : 1.f;
        p.fz_clip = q ? (unsigned long long*)ep->q_clipped : nullptr;
        p.fz_scale = e->scale; p.fz_shift = e->shift;
        p.fz_res = (const bf16_raw*)e->res; p.fz_res_lo = (const bf16_raw*)e->res_lo;
        p.fz_lens = e->lens;
        p.fz_out = (bf16_raw*)e->out_hi; p.fz_out_lo = (bf16_raw*)e->out_lo;
        p.fz_rows = e->out_rows; p.fz_pad_l = e->pad_l; p.fz_pad_r = e->pad_r; p.fz_pad_mode = e->pad_mode;
        p.fz_act = e->act;
        pl.epi = 2;
    }
    // the last valid output row must only need rows that exist in the padded buffer
    const int64_t need = (int64_t)(pr.N - 1) * p.x_rows_per_utt + (int64_t)(pr.Tout - 1) * pr.stride + (int64_t)(pr.Kw - 1) * pr.dil;
    W2L_CHECK_ARG(need <= p.x_max_row, "%s: padded input too small (need row %lld, have %lld)", who, (long long)need,
                  (long long)p.x_max_row);
    // (a fused data gradient shares the table with forward launches: its N = 1, Tout = flat rows shape never coincides with
    // one of theirs)
    pl.idx = choose_cfg(pr, stats_flag(pr, ep), forced);
    W2L_CHECK_ARG(pl.idx >= 0, "%s: no block shape fits LDS (Kw=%d dil=%d stride=%d)", who, pr.Kw, pr.dil, pr.stride);
    pl.f8 = pr.f8;
    pl.shape = pr.f8 ? kF8Cfgs[pl.idx] : pl.idx % kNumCfgs;
    pl.pipe = pr.f8 ? 0 : (pl.idx % kBaseCfgs) / kNumCfgs;
    const TileCfg& c = kCfgs[pl.shape];
    const TileGeom g = tile_geom(c, pr);
    p.tiles_t = g.tiles_t;
    p.ncols = pr.N * g.tiles_t;
    p.xrows_lds = g.xrows;
    // a split-K choice (measured with a workspace) silently degrades to one block per tile when the caller brings none.
    // (A fused inference launch may split K: the block that combines the slabs holds the whole tile in registers and runs
    // the epilogue; the fused epilogues never run stream-K)
    int splits = pr.f8 ? 1 : kSplits[pl.idx / kBaseCfgs];
    p.sk_ranges = 0;
    p.sk_total = 0;
    if (splits == 0) {
        if (pl.epi == 0 && sk_feasible(g, pr)) {
            p.sk_ranges = sk_ranges(g);
            p.sk_total = g.tiles_m * p.ncols * ((pr.Cin / BK) * pr.Kw);
        }
        splits = 1;
    }
    if (!split_feasible(g, splits, pr)) splits = 1;
    p.splits = splits;
    p.tickets = (unsigned*)pr.ws;
    p.slabs = pr.ws ? (float*)((char*)pr.ws + kTicketBytes) : nullptr;
    pl.splits = splits;
    pl.sk_ranges = p.sk_ranges;
    pl.grid = p.sk_ranges > 0 ? (unsigned)p.sk_ranges : (unsigned)(g.tiles_m * splits * p.ncols);
    pl.threads = 64 * g.waves;
    pl.lds = g.lds;
    pl.stream = pr.stream;
    return 0;
}

// ---- measure-and-pick (the _tune entry points; EXPLICITLY synchronising: warm-up only) ----
struct EventPair {                                      // destroyed on every return path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// one launch of the plan `make` yields (which also validates it), then `n` launches timed between the two events;
// < 0: the candidate did not run
template <typename MakePlan>
static float time_candidate(const MakePlan& make, int n, const EventPair& ev) {
    ConvPlan pl;
    if (make(pl) != 0 || launch(pl) != 0) return -1.f;
    (void)hipEventRecord(ev.e0, pl.stream);
    for (int r = 0; r < n; ++r) launch(pl);
    (void)hipEventRecord(ev.e1, pl.stream);
    if (hipEventSynchronize(ev.e1) != hipSuccess) return -1.f;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess) return -1.f;
    return ms;
}

// Measure every feasible configuration for this problem on the caller's device and remember the fastest.  Call it once per
// shape during warm-up, never inside a captured / latency-critical region.  The output is simply rewritten (accumulate == 0).
static int tune(const ConvProblem& pr, const Epilogue* ep, int reps) {
    const int sflag = stats_flag(pr, ep);
    const ShapeKey key = shape_key(pr, sflag);
    auto& table = pr.f8 ? g_tuned_f8 : g_tuned;
    {
        std::lock_guard<std::mutex> lock(g_tuned_mu);
        if (table.count(key)) return 0;
    }
    EventPair ev;
    W2L_CHECK_HIP(hipEventCreate(&ev.e0));
    W2L_CHECK_HIP(hipEventCreate(&ev.e1));
    if (reps < 1) reps = 1;
    if (pr.ws) (void)hipMemsetAsync(pr.ws, 0, kTicketBytes, pr.stream);      // tickets start from zero whatever ran before
    auto time_cfg = [&](int i, int n) -> float {
        float ms = time_candidate([&](ConvPlan& pl) { return plan(pr, ep, i, pl); }, n, ev);
        // a stream-K form has to win by 3 %: level with the best one-block-per-tile form it buys the step nothing (plan files
        // with and without it: 12.79 / 12.82 ms) and moves 40-45 MB more per launch through its slabs
        if (!pr.f8 && kSplits[i / kBaseCfgs] == 0) ms *= 1.03f;
        return ms;
    };
    int best = -1;
    if (pr.f8) {                                        // the e4m3 kernel's few shapes: a single pass
        float best_ms = 1e30f;
        for (int k = 0; k < kNumF8Cfgs; ++k) {
            if (!f8_feasible(k, pr, sflag)) continue;
            const float ms = time_cfg(k, reps);
            if (ms >= 0.f && ms < best_ms) { best_ms = ms; best = k; }
        }
    } else {
        std::vector<std::pair<float, int>> timed;
        for (int i = 0; i < kBaseCfgs * kNumSplits; ++i) {
            if (!cfg_feasible(i, pr, sflag)) continue;
            const int splits = kSplits[i / kBaseCfgs];
            const TileGeom g = tile_geom(kCfgs[i % kNumCfgs], pr);
            if (splits == 0) {
                // stream-K where one block per tile fills the last round to 85 % or less (and never under a fused epilogue)
                if (ep->kind != kEpiNone || !sk_feasible(g, pr)) continue;
                const int64_t slots = sk_ranges(g);
                if (last_round_fill(g.blocks, slots) > 0.85 || g.blocks > 4 * slots) continue;   // (at 92 % fill it measured 3 % ahead alone and level in the step,
                                                                       //  for 48 MB more traffic per launch: every finisher's acquire empties its XCD's L2)
            } else if (splits > 1) {
                // split-K is only a candidate where one block per tile leaves CUs idle (a partly filled last round, or fewer
                // tiles than CUs) and where it does not flood the chip with short blocks
                if (!split_feasible(g, splits, pr)) continue;
                const int64_t slots = (int64_t)kCUs * blocks_per_cu(g, kWaveCap);
                if (last_round_fill(g.blocks, slots) > 0.92 || g.blocks * splits > 6 * slots ||
                    (pr.Cin / BK) * pr.Kw / splits < 8)
                    continue;
            }
            const float ms = time_cfg(i, reps);
            if (ms >= 0.f) timed.emplace_back(ms, i);
        }
        // the first pass ranks ~50 candidates on `reps` launches each -- the clock the chip holds drifts over such a sweep by
        // more than the best candidates differ --, so the kFinalists fastest are timed again, interleaved (common.h)
        std::sort(timed.begin(), timed.end());
        best = timed.empty() ? -1 : timed[0].second;
        const int finalists = timed.size() < kFinalists ? (int)timed.size() : kFinalists;
        if (finalists > 1) {
            float total[kFinalists] = {};
            for (int round = 0; round < kFinalRounds; ++round)
                for (int k = 0; k < finalists; ++k) {
                    const float ms = time_cfg(timed[k].second, 4 * reps);
                    total[k] += ms >= 0.f ? ms : 1e30f;
                }
            int kb = 0;
            for (int k = 1; k < finalists; ++k)
                if (total[k] < total[kb]) kb = k;
            best = timed[kb].second;
        }
    }
    W2L_CHECK_ARG(best >= 0, "%s_tune: no feasible block shape", pr.f8 ? "conv1d_igemm_fp8" : "conv1d_igemm");
    std::lock_guard<std::mutex> lock(g_tuned_mu);
    table[key] = best;
    return 0;
}

// what every entry point ends in -- reps == 0: plan and launch; reps > 0: measure and remember.  The one reader of the hooks.
static int run(ConvProblem pr, const Epilogue* ep, int reps = 0) {
    pr.stats_slots = pr.stats ? g_stats_slots : 0;
    if (reps != 0) return tune(pr, ep, reps);
    ConvPlan pl;
    if (int rc = plan(pr, ep, pr.f8 ? g_force_f8 : g_force_cfg, pl)) return rc;
    return launch(pl);
}

extern "C" int w2l_conv1d_igemm_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y,
                                   int y_f32, int accumulate, const float* bias, float* stats_partial, int N, int Cin,
                                   int Cout, int Tout, int Kw, int stride, int dil, void* splitk_ws, int64_t splitk_ws_bytes,
                                   void* stream) {
    return run({xp, x_bstride, x_rows_total, w, y, y_f32, accumulate, bias, stats_partial, N, Cin, Cout, Tout, Kw, stride, dil,
                splitk_ws, splitk_ws_bytes, (hipStream_t)stream}, &kNoEpilogue);
}

// the flat data gradient with the BatchNorm-backward reduction in its epilogue, and its measure-and-pick (the candidates run
// with the fused epilogue)
extern "C" int w2l_conv1d_dgrad_bnreduce_ws(const void* dy, int64_t dy_rows_total, const void* w_dgr, void* dxp, float* partial,
                                            const w2l_bnact_t* d, int pad_l, int pad_r, int pad_mode, int per, int Cconv_out,
                                            int flat_rows, int Kw, int dil, void* splitk_ws, int64_t splitk_ws_bytes,
                                            void* stream) {
    W2L_CHECK_ARG(d != nullptr, "conv1d_dgrad_bnreduce: null descriptor");
    const Epilogue ep{kEpiBnReduce, {d, pad_l, pad_r, pad_mode, per}};
    return run({dy, dy_rows_total * Cconv_out, dy_rows_total, w_dgr, dxp, 0, 0, nullptr, partial, 1, Cconv_out, d->C, flat_rows,
                Kw, 1, dil, splitk_ws, splitk_ws_bytes, (hipStream_t)stream}, &ep);
}

extern "C" int w2l_conv1d_igemm(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y,
                                int y_f32, int accumulate, const float* bias, float* stats_partial, int N, int Cin,
                                int Cout, int Tout, int Kw, int stride, int dil, void* stream) {
    return w2l_conv1d_igemm_ws(xp, x_bstride, x_rows_total, w, y, y_f32, accumulate, bias, stats_partial, N, Cin, Cout, Tout,
                               Kw, stride, dil, nullptr, 0, stream);
}

// ---- inference: convolution + BatchNorm (running statistics) + residual + activation + mask + the consumer's padding ----
extern "C" int w2l_conv1d_igemm_bnact_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w,
                                         const float* acc_in, const float* bias, const w2l_bnact_epi_t* e, int N, int Cin,
                                         int Cout, int Tout, int Kw, int stride, int dil, void* splitk_ws,
                                         int64_t splitk_ws_bytes, void* stream) {
    W2L_CHECK_ARG(e != nullptr, "conv1d_igemm_bnact: null descriptor");
    const Epilogue ep{kEpiInfer, {}, e};
    return run({xp, x_bstride, x_rows_total, w, (void*)acc_in, 1, acc_in != nullptr, bias, nullptr, N, Cin, Cout, Tout, Kw,
                stride, dil, splitk_ws, splitk_ws_bytes, (hipStream_t)stream}, &ep);
}

extern "C" int w2l_conv1d_igemm_bnact(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w,
                                      const float* acc_in, const float* bias, const w2l_bnact_epi_t* e, int N, int Cin, int Cout,
                                      int Tout, int Kw, int stride, int dil, void* stream) {
    return w2l_conv1d_igemm_bnact_ws(xp, x_bstride, x_rows_total, w, acc_in, bias, e, N, Cin, Cout, Tout, Kw, stride, dil,
                                     nullptr, 0, stream);
}

// measure-and-pick for a fused inference launch: the candidates run with the fused epilogue and are remembered under a key of
// their own (SYNCHRONISING; warm-up only).  The output is written like a normal launch.
extern "C" int w2l_conv1d_igemm_bnact_tune_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w,
                                              const float* bias, const w2l_bnact_epi_t* e, int N, int Cin, int Cout, int Tout,
                                              int Kw, int stride, int dil, int reps, void* splitk_ws, int64_t splitk_ws_bytes,
                                              void* stream) {
    W2L_CHECK_ARG(e != nullptr, "conv1d_igemm_bnact_tune: null descriptor");
    const Epilogue ep{kEpiInfer, {}, e};
    return run({xp, x_bstride, x_rows_total, w, nullptr, 1, 0, bias, nullptr, N, Cin, Cout, Tout, Kw, stride, dil, splitk_ws,
                splitk_ws_bytes, (hipStream_t)stream}, &ep, reps < 1 ? 1 : reps);
}

// blocks of the stream-K launch configuration idx would make of this problem with a workspace of ws_bytes; 0: the launch
// falls back to one block per tile (no stream-K form of that configuration, ranges too short, workspace too small)
extern "C" int w2l_conv_streamk_ranges(int idx, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int64_t ws_bytes) {
    static char dummy;
    ConvProblem pr = window_only(Kw, stride, dil);
    pr.N = N; pr.Cin = Cin; pr.Cout = Cout; pr.Tout = Tout; pr.ws = &dummy; pr.ws_bytes = ws_bytes;
    if (!cfg_feasible(idx, pr, 0) || kSplits[idx / kBaseCfgs] != 0) return 0;
    const TileGeom g = tile_geom(kCfgs[idx % kNumCfgs], pr);
    return sk_feasible(g, pr) ? sk_ranges(g) : 0;
}

// the pieces of a stream-K launch of `tiles` tiles x `steps` steps over G ranges, in range order, as the kernel walks them:
// out[7 * i] = range, tile, first step, end step, ranges sharing the tile, this range's place among them, slab id (-1: the
// tile is whole).  Returns the piece count, -1 if cap is too small or the sizes are out of the kernel's 32-bit range.
extern "C" int w2l_conv_streamk_pieces(int tiles, int steps, int G, int* out, int cap) {
    if (tiles <= 0 || steps <= 0 || G <= 0 || ((int64_t)tiles * steps + steps) * G >= (1LL << 31)) return -1;
    const int W = tiles * steps;
    int n = 0;
    for (int r = 0; r < G; ++r) {
        int w_cur = (int)(((int64_t)W * r) / G);
        const int w_end = (int)(((int64_t)W * (r + 1)) / G);
        while (w_cur < w_end) {
            const SkPiece q = sk_piece(W, G, steps, r, w_cur, w_end);
            if (n >= cap) return -1;
            int* o = out + 7 * n++;
            o[0] = r; o[1] = q.tile; o[2] = q.s_begin; o[3] = q.s_end; o[4] = q.nsplit; o[5] = q.split;
            o[6] = q.nsplit > 1 ? (int)(q.slab_base + q.split) : -1;
            w_cur += q.s_end - q.s_begin;
        }
    }
    return n;
}

// bytes of split-K workspace that let every configuration of this problem run (slabs of the largest split + the tickets)
extern "C" int64_t w2l_conv_splitk_workspace_bytes(int N, int Cout, int Tout) {
    ConvProblem pr{};
    pr.N = N; pr.Cout = Cout; pr.Tout = Tout;
    size_t need = 0;
    for (int i = 0; i < kNumCfgs; ++i) need = std::max(need, splitk_bytes(tile_geom(kCfgs[i], pr), kMaxSplit));
    return (int64_t)need;
}

extern "C" int w2l_conv1d_igemm_tune_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y,
                                        int y_f32, const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout,
                                        int Kw, int stride, int dil, int reps, void* splitk_ws, int64_t splitk_ws_bytes,
                                        void* stream) {
    return run({xp, x_bstride, x_rows_total, w, y, y_f32, 0, bias, stats_partial, N, Cin, Cout, Tout, Kw, stride, dil, splitk_ws,
                splitk_ws_bytes, (hipStream_t)stream}, &kNoEpilogue, reps < 1 ? 1 : reps);
}

extern "C" int w2l_conv1d_dgrad_bnreduce_tune_ws(const void* dy, int64_t dy_rows_total, const void* w_dgr, void* dxp,
                                                 float* partial, const w2l_bnact_t* d, int pad_l, int pad_r, int pad_mode,
                                                 int per, int Cconv_out, int flat_rows, int Kw, int dil, int reps,
                                                 void* splitk_ws, int64_t splitk_ws_bytes, void* stream) {
    W2L_CHECK_ARG(d != nullptr, "conv1d_dgrad_bnreduce_tune: null descriptor");
    const Epilogue ep{kEpiBnReduce, {d, pad_l, pad_r, pad_mode, per}};
    return run({dy, dy_rows_total * Cconv_out, dy_rows_total, w_dgr, dxp, 0, 0, nullptr, partial, 1, Cconv_out, d->C, flat_rows,
                Kw, 1, dil, splitk_ws, splitk_ws_bytes, (hipStream_t)stream}, &ep, reps < 1 ? 1 : reps);
}

extern "C" int w2l_conv1d_igemm_tune(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y,
                                     int y_f32, const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout,
                                     int Kw, int stride, int dil, int reps, void* stream) {
    return w2l_conv1d_igemm_tune_ws(xp, x_bstride, x_rows_total, w, y, y_f32, bias, stats_partial, N, Cin, Cout, Tout, Kw,
                                    stride, dil, reps, nullptr, 0, stream);
}

// ---- e4m3 operands (BASELINE config 5: fp8 MFMA) ----
extern "C" int w2l_conv1d_igemm_fp8(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq, void* y, int y_f32,
                                    float descale, const float* descale_dev, const float* bias, float* stats_partial, int N,
                                    int Cin, int Cout, int Tout, int Kw, int dil, void* stream) {
    W2L_CHECK_ARG(y, "conv1d_igemm_fp8: null pointer");
    return run({xq, x_bstride, x_rows_total, wq, y, y_f32, 0, bias, stats_partial, N, Cin, Cout, Tout, Kw, 1, dil, nullptr, 0,
                (hipStream_t)stream, true, descale, descale_dev}, &kNoEpilogue);
}

// ---- inference on e4m3 operands: the whole unit in the e4m3 kernel's epilogue (conv_igemm_kernel<F8, EPI = 2>) ----
extern "C" int w2l_conv1d_igemm_bnact_fp8(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq, float descale,
                                          const float* bias, const w2l_bnact_epi_t* e, void* out_q, float q_scale,
                                          int64_t* q_clipped, int N, int Cin, int Cout, int Tout, int Kw, int dil, void* stream) {
    W2L_CHECK_ARG(e != nullptr, "conv1d_igemm_bnact_fp8: null descriptor");
    const Epilogue ep{kEpiInferF8, {}, e, out_q, q_scale, q_clipped};
    return run({xq, x_bstride, x_rows_total, wq, nullptr, 0, 0, bias, nullptr, N, Cin, Cout, Tout, Kw, 1, dil, nullptr, 0,
                (hipStream_t)stream, true, descale}, &ep);
}

// measure the e4m3 block shapes for this problem and remember the fastest (SYNCHRONISING: warm-up only)
extern "C" int w2l_conv1d_igemm_fp8_tune(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq, void* y,
                                         int y_f32, const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout,
                                         int Kw, int dil, int reps, void* stream) {
    return run({xq, x_bstride, x_rows_total, wq, y, y_f32, 0, bias, stats_partial, N, Cin, Cout, Tout, Kw, 1, dil, nullptr, 0,
                (hipStream_t)stream, true}, &kNoEpilogue, reps < 1 ? 1 : reps);
}

// measure-and-pick for the fused e4m3 launch: the candidates run WITH the epilogue (descale 1: the time does not depend on it) and
// are remembered under flag 3 of the e4m3 table (SYNCHRONISING; warm-up only).  The saturation counter is not passed on: the
// measuring launches must not count.  The outputs are written like a normal launch's, to be overwritten by the one that follows.
extern "C" int w2l_conv1d_igemm_bnact_fp8_tune(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq,
                                               const float* bias, const w2l_bnact_epi_t* e, void* out_q, float q_scale, int N,
                                               int Cin, int Cout, int Tout, int Kw, int dil, int reps, void* stream) {
    W2L_CHECK_ARG(e != nullptr, "conv1d_igemm_bnact_fp8_tune: null descriptor");
    const Epilogue ep{kEpiInferF8, {}, e, out_q, q_scale, nullptr};
    return run({xq, x_bstride, x_rows_total, wq, nullptr, 0, 0, bias, nullptr, N, Cin, Cout, Tout, Kw, 1, dil, nullptr, 0,
                (hipStream_t)stream, true}, &ep, reps < 1 ? 1 : reps);
}

// ---- host-only queries ----
// The plan a launch of this problem would get, without a stream or a buffer: out = configuration index, K-loop structure,
// blocks per tile, stream-K blocks, grid blocks, block threads, LDS bytes, feasible.  stats_flag as in the shape key;
// forced_idx < 0: the tuned choice or the cost model.  Returns 0 and out[7] = 1, or 1 with out = {-1, 0...} and the error set.
static int plan_query(bool f8, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int sflag, int64_t ws_bytes,
                      int forced_idx, int* out) {
    static char dummy[16];
    w2l_bnact_epi_t e{};
    e.out_hi = dummy;
    e.out_rows = Tout;
    const Epilogue ep{sflag == 3 ? (f8 ? kEpiInferF8 : kEpiInfer) : kEpiNone, {}, &e};
    const int64_t rows = (int64_t)(Tout - 1) * stride + (int64_t)(Kw - 1) * dil + 1;
    ConvProblem pr{dummy, Cin > 0 ? rows * Cin : 0, rows * N, dummy, sflag == 3 ? nullptr : dummy, 1, 0, nullptr,
                   sflag == 1 || sflag == 2 ? (float*)dummy : nullptr, N, Cin, Cout, Tout, Kw, stride, dil,
                   ws_bytes > 0 ? dummy : nullptr, ws_bytes, nullptr, f8};
    pr.stats_slots = sflag == 2 ? 1 : 0;
    ConvPlan pl;
    out[0] = -1;
    for (int i = 1; i < 8; ++i) out[i] = 0;
    W2L_CHECK_ARG(sflag >= 0 && sflag <= 3 && !(f8 && sflag == 2), "conv_plan: stats_flag is 0..3 (e4m3: 0, 1 or 3)");
    if (int rc = plan(pr, &ep, forced_idx, pl)) return rc;
    const int v[8] = {pl.idx, pl.pipe, pl.splits, pl.sk_ranges, (int)pl.grid, (int)pl.threads, (int)pl.lds, 1};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return 0;
}

extern "C" int w2l_conv_plan(int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int stats_flag, int64_t ws_bytes,
                             int forced_idx, int* out) {
    return plan_query(false, N, Cin, Cout, Tout, Kw, stride, dil, stats_flag, ws_bytes, forced_idx, out);
}

extern "C" int w2l_conv_plan_fp8(int N, int Cin, int Cout, int Tout, int Kw, int dil, int stats_flag, int forced_idx, int* out) {
    return plan_query(true, N, Cin, Cout, Tout, Kw, 1, dil, stats_flag, 0, forced_idx, out);
}

// Tuning-cache (de)serialisation used by w2l_tune_save / w2l_tune_load (runtime.hip): "<tag> <the 8 key fields> <index>"
static void tune_dump(FILE* f, const char* tag, const std::map<ShapeKey, int>& table) {
    std::lock_guard<std::mutex> lock(g_tuned_mu);
    for (const auto& kv : table) {
        const ShapeKey& k = kv.first;
        fprintf(f, "%s %d %d %d %d %d %d %d %d %d\n", tag, std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k),
                std::get<4>(k), std::get<5>(k), std::get<6>(k), std::get<7>(k), kv.second);
    }
}
void w2l_igemm_tune_dump(FILE* f) { tune_dump(f, "igemm", g_tuned); }
void w2l_igemm_fp8_tune_dump(FILE* f) { tune_dump(f, "igemmf8", g_tuned_f8); }

bool w2l_igemm_fp8_tune_put(const int* v) {      // v[0..7] = key, v[8] = index into kF8Cfgs
    const int sflag = v[7] == 3 ? 3 : (v[7] != 0 ? 1 : 0);
    if (v[5] != 1 || v[0] < 1 || v[3] < 1 || !f8_feasible(v[8], window_only(v[4], 1, v[6]), sflag)) return false;
    std::lock_guard<std::mutex> lock(g_tuned_mu);
    g_tuned_f8[ShapeKey(v[0], v[1], v[2], v[3], v[4], 1, v[6], sflag)] = v[8];
    return true;
}

bool w2l_igemm_tune_put(const int* v) {          // v[0..7] = key, v[8] = configuration index
    if (v[7] < 0 || v[7] > 3 || !cfg_feasible(v[8], window_only(v[4], v[5], v[6]), v[7])) return false;
    if (v[7] == 3 && kSplits[v[8] / kBaseCfgs] == 0) return false; // (fused inference launches have no stream-K form)
    std::lock_guard<std::mutex> lock(g_tuned_mu);
    g_tuned[ShapeKey(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7])] = v[8];
    return true;
}

// Energy voice-activity detection and segmentation of long recordings on gfx950 (segmentation.py; the rule is stated in
// DESIGN.md and restated, sequentially, by tests/vad_refs.py).  Two launches for a batch of N padded recordings:
//
// w2l_vad_power   grid (run of frames, recording).  A block takes `fpb` consecutive frames, stages their sample span
//                 [f0 hop, (f0 + fpb - 1) hop + win) into LDS once with 16-byte loads (the win - hop overlap of neighbouring
//                 frames is served from there), then lane = frame and wave = one eighth of the frame's samples: a lane adds
//                 double(x[i])^2 over its slice sample after sample (no cross-lane reduction), and the eight slice sums of a
//                 frame are added in slice order.  The order is fixed, so two runs give the same bits; every sample is read
//                 from memory once (plus the win - hop samples two neighbouring blocks share).
// w2l_vad_segments one workgroup of 1024 threads per recording; everything below happens inside it, with the run lists in a
//                 caller-owned workspace:
//                   statistics   peak = max, floor = the floor(q (F - 1))-th smallest power by a 4 x 8-bit radix select on the
//                                bit patterns (non-negative floats order as unsigned integers);
//                   hysteresis   per frame one of the maps {keep, set 0, set 1}; the composition "the right one unless it is
//                                keep" is associative: inside a wave it is two ballots and a count-leading-zeros, across the 16
//                                waves and across 1024-frame tiles a carry;
//                   runs         edge flags -> exclusive scan -> compaction into (start, end) lists; closing gaps, dropping short
//                                runs and padding + merging are three more flag / scan / compact passes over the lists;
//                   forced split one wave per run: argmin over the window (lowest index among equal minima), repeated; the
//                                pieces are counted first, the counts scanned into offsets, then written in order.
// No cross-workgroup dependence, no atomics on global memory, no scratch.
#include <math.h>
#include "common.h"
#include "../../include/w2l_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- frame power
constexpr int VP_THREADS = 512;
constexpr int VP_PARTS = VP_THREADS / 64;                // a frame's samples are split into this many slices, one per wave
constexpr int VP_MAX_FPB = 64;                           // frames a block takes at the most: one per lane
constexpr int VP_MAX_SPAN = W2L_VAD_MAX_SPAN;            // floats of LDS a block may stage
constexpr int VP_BATCH = 4;                              // 16-byte loads a thread has in flight while staging

struct PowerParams {
    const float* x;
    const int32_t* lens;
    float* power;
    int64_t x_stride, power_stride;
    int win, hop, fpb;
};

__global__ __launch_bounds__(VP_THREADS) void vad_power_kernel(PowerParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* part = reinterpret_cast<double*>(lds_raw);                           // [VP_PARTS][64]
    float* xs = reinterpret_cast<float*>(lds_raw + VP_PARTS * 64 * sizeof(double));
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t n = p.lens[row];
    n = n < 0 ? 0 : (n > p.x_stride ? p.x_stride : n);   // a length outside its row reads nothing outside it
    const int64_t F = (n + p.hop - 1) / p.hop;
    const int64_t f0 = (int64_t)blockIdx.x * p.fpb;
    const int64_t f1 = f0 + p.fpb < p.power_stride ? f0 + p.fpb : p.power_stride;    // this block writes frames [f0, f1)
    float* out = p.power + (int64_t)row * p.power_stride;
    const int64_t fe = F < f1 ? F : f1;                  // ... of which [f0, fe) are frames of the recording
    for (int64_t f = (fe > f0 ? fe : f0) + tid; f < f1; f += VP_THREADS) out[f] = 0.f;
    if (fe <= f0) return;

    // ---- the samples of frames [f0, fe) into LDS, the first one rounded down to a float4 boundary of the row; VP_BATCH loads
    // are issued before the first of them is stored
    const float* x = p.x + (int64_t)row * p.x_stride;
    const int64_t s0 = f0 * p.hop;
    const int64_t last = (fe - 1) * p.hop + p.win;
    const int64_t hi = last < n ? last : n;
    const int64_t lo = s0 & ~(int64_t)3;
    const int lead = (int)(s0 - lo);
    const int n_stage = (int)(hi - lo);                  // <= (fpb - 1) hop + win + 3: the host sized the LDS array for it
    const bool vec_ok = ((p.x_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.x) & 15) == 0);
    for (int i0 = 4 * tid; i0 < n_stage; i0 += 4 * VP_THREADS * VP_BATCH) {
        f32x4 v[VP_BATCH];
#pragma unroll
        for (int u = 0; u < VP_BATCH; ++u) {
            const int i = i0 + u * 4 * VP_THREADS;
            const int64_t g = lo + i;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < n_stage) {
                if (vec_ok && g + 3 < n) {
                    v[u] = *reinterpret_cast<const f32x4*>(x + g);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (g + e < n) v[u][e] = x[g + e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < VP_BATCH; ++u) {
            const int i = i0 + u * 4 * VP_THREADS;
            if (i < n_stage) *reinterpret_cast<f32x4*>(xs + i) = v[u];          // the LDS array holds whole float4s past n_stage
        }
    }
    __syncthreads();

    // ---- lane = frame, wave = slice of the frame's samples.  A lane adds its slice one sample after the other into two
    // alternating fp64 sums, starting `lane` samples into the slice when hop is even: the lanes of a wave then read LDS
    // addresses lane * (hop + 1) + const apart, an odd stride, which no two lanes of a 32-lane group share a bank at.  The
    // order depends on the frame's place in its block only: two runs give the same bits.
    const int64_t f = f0 + lane;
    double a0 = 0.0, a1 = 0.0;
    if (f < fe) {
        const int64_t left = n - f * p.hop;              // >= 1
        const int cnt = left < p.win ? (int)left : p.win;
        const int q = (p.win + VP_PARTS - 1) / VP_PARTS;
        const int qlo = wave * q;
        const int qhi = qlo + q < cnt ? qlo + q : cnt;
        const int qlen = qhi - qlo;
        if (qlen > 0) {
            const float* s = xs + lead + lane * p.hop;
            int idx = qlo + ((p.hop & 1) ? 0 : lane % qlen);
            int k = 0;
            for (; k + 1 < qlen; k += 2) {
                const double v0 = (double)s[idx];
                idx = idx + 1 == qhi ? qlo : idx + 1;
                const double v1 = (double)s[idx];
                idx = idx + 1 == qhi ? qlo : idx + 1;
                a0 = fma(v0, v0, a0);                    // v * v is exact in double: the same bits as multiply, then add
                a1 = fma(v1, v1, a1);
            }
            if (k < qlen) {
                const double v0 = (double)s[idx];
                a0 = fma(v0, v0, a0);
            }
        }
    }
    part[wave * 64 + lane] = a0 + a1;
    __syncthreads();
    if (wave == 0 && f < fe) {
        double acc = part[lane];
#pragma unroll
        for (int w = 1; w < VP_PARTS; ++w) acc += part[w * 64 + lane];
        out[f] = (float)(acc / (double)p.win);           // a partial last frame is divided by win too
    }
}

// ---------------------------------------------------------------------------------------------------------------- decisions
constexpr int VS_THREADS = 1024;
constexpr int VS_WAVES = VS_THREADS / 64;
constexpr int VS_HEADER = W2L_VAD_HEADER_BYTES;

struct SegParams {
    const float* power;
    int64_t power_stride;
    const int32_t* nframes;
    w2l_vad_params_t v;
    int cap;
    int32_t* ws;             // per recording 5 int32 arrays of run_cap: starts A, ends A, starts B, ends B, piece counts
    int64_t run_cap;
    char* out;
    int64_t out_stride;      // bytes per recording: VS_HEADER + 8 cap
};

// a power as every decision reads it: NaN and negative values count as 0 (status bit 1 reports them), -0 as +0
__device__ __forceinline__ float read_power(const float* P, int f) {
    float p = P[f];
    if (!(p >= 0.f)) p = 0.f;
    return p == 0.f ? 0.f : p;
}

// exclusive prefix sum of one int per thread over the workgroup, and the total; `lds` holds VS_WAVES ints
__device__ __forceinline__ int block_scan_excl(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < VS_WAVES; ++w) {
        const int c = lds[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    __syncthreads();                                     // lds may be written again
    total = tot;
    return base + inc - v;
}

// the pieces of the run [a, b) under the forced split, by one wave: returns their number; with `write` piece j goes to
// seg[base + j] while base + j < cap
__device__ __forceinline__ int split_run(const float* P, int a, int b, int maxf, int h, int32_t* seg, int base, int cap, bool write) {
    const int lane = threadIdx.x & 63;
    int j = 0;
    while (b - a > maxf) {
        const int lo = a + h;
        const int hi = a + maxf < b - h ? a + maxf : b - h;     // lo < hi: maxf > h, and b - a > maxf >= 2 h
        float bv = INFINITY;
        int bi = 0x7fffffff;
        for (int i = lo + lane; i < hi; i += 64) {
            const float pw = read_power(P, i);
            if (pw < bv) { bv = pw; bi = i; }            // strict: the lowest index of this lane's minimum
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        const int c = (bi < lo || bi >= hi) ? lo : bi;   // (bi is always inside the window: powers read as finite or +inf)
        if (write && lane == 0 && base + j < cap) {
            seg[2 * (base + j)] = a;
            seg[2 * (base + j) + 1] = c;
        }
        ++j;
        a = c;
    }
    if (write && lane == 0 && base + j < cap) {
        seg[2 * (base + j)] = a;
        seg[2 * (base + j) + 1] = b;
    }
    return j + 1;
}

__global__ __launch_bounds__(VS_THREADS) void vad_segments_kernel(SegParams p) {
    __shared__ unsigned hist[256];
    __shared__ int sc[VS_WAVES];
    __shared__ int wmap[VS_WAVES];
    __shared__ unsigned sh_peak, sh_bad, sh_prefix;
    __shared__ int sh_k;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const w2l_vad_params_t& v = p.v;
    const float* P = p.power + (int64_t)row * p.power_stride;
    int F = p.nframes[row];
    F = F < 0 ? 0 : ((int64_t)F > p.power_stride ? (int)p.power_stride : F);
    int32_t* SA = p.ws + (int64_t)row * 5 * p.run_cap;
    int32_t* EA = SA + p.run_cap;
    int32_t* SB = EA + p.run_cap;
    int32_t* EB = SB + p.run_cap;
    int32_t* PC = EB + p.run_cap;
    char* rec = p.out + (int64_t)row * p.out_stride;
    int32_t* seg = reinterpret_cast<int32_t*>(rec + VS_HEADER);

    // ---- statistics: bad values, peak, and the k-th smallest power, k = floor(q (F - 1))
    if (tid == 0) {
        sh_peak = 0u;
        sh_bad = 0u;
        sh_prefix = 0u;
        int64_t k = F > 0 ? (int64_t)floor(v.q * (double)(F - 1)) : 0;
        sh_k = (int)(k < 0 ? 0 : (k > F - 1 ? (F > 0 ? F - 1 : 0) : k));
    }
    __syncthreads();
    {
        unsigned lmax = 0u;
        bool lbad = false;
        for (int f = tid; f < F; f += VS_THREADS) {
            if (!(P[f] >= 0.f)) lbad = true;
            const unsigned key = __float_as_uint(read_power(P, f));
            lmax = key > lmax ? key : lmax;
        }
        atomicMax(&sh_peak, lmax);                       // (LDS)
        if (lbad) atomicOr(&sh_bad, 2u);
    }
    unsigned prefix = 0u;
    for (int pass = 0; pass < 4 && F > 0; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        for (int i = tid; i < 256; i += VS_THREADS) hist[i] = 0u;
        __syncthreads();
        for (int f = tid; f < F; f += VS_THREADS) {
            const unsigned key = __float_as_uint(read_power(P, f));
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int kk = sh_k;
            unsigned d = 0;
            for (; d < 255u; ++d) {
                const int c = (int)hist[d];
                if (kk < c) break;
                kk -= c;
            }
            sh_k = kk;
            sh_prefix = prefix | (d << shift);
        }
        __syncthreads();
        prefix = sh_prefix;
    }
    __syncthreads();
    const float floor_p = __uint_as_float(prefix), peak_p = __uint_as_float(sh_peak);

    // ---- thresholds, in double from the fp32 statistics (every thread forms the same values)
    double thr_on, thr_off;
    if (v.absolute) {
        thr_on = v.thr_on;
        thr_off = v.thr_off;
    } else {
        const double a = (double)floor_p * v.r_on;
        const double g = sqrt((double)floor_p * (double)peak_p);         // correctly rounded; the product is exact
        const double m = a < g ? a : g;
        thr_on = v.abs_min > m ? v.abs_min : m;
        thr_off = thr_on * v.r_hyst;
    }

    // ---- hysteresis and the raw runs: starts into SA, ends into EA
    int state = 0, nS = 0, nE = 0;
    for (int t0 = 0; t0 < F; t0 += VS_THREADS) {
        const int f = t0 + tid;
        int map = 0;                                     // 0 keep, 1 set 0, 2 set 1
        if (f < F) {
            const double pw = (double)read_power(P, f);
            map = pw >= thr_on ? 2 : (pw < thr_off ? 1 : 0);
        }
        const unsigned long long D = __ballot(map != 0), O = __ballot(map == 2);
        if (lane == 0) wmap[wave] = D ? (int)((O >> (63 - __clzll((long long)D))) & 1ull) + 1 : 0;
        __syncthreads();
        int in = state, carry = state;                   // the state entering this wave, and the one leaving the tile
#pragma unroll
        for (int w = 0; w < VS_WAVES; ++w) {
            const int m = wmap[w];
            if (m) {
                carry = m - 1;
                if (w < wave) in = m - 1;
            }
        }
        const unsigned long long le = D & (~0ull >> (63 - lane));
        const int s = le ? (int)((O >> (63 - __clzll((long long)le))) & 1ull) : in;
        int sp = __shfl_up(s, 1);
        if (lane == 0) sp = in;
        const int is_start = (f < F) && s && !sp, is_end = (f < F) && !s && sp;
        int total;
        const int ex = block_scan_excl(is_start | (is_end << 16), sc, total);      // (its barriers also free wmap)
        if (is_start) SA[nS + (ex & 0xffff)] = f;
        if (is_end) EA[nE + (ex >> 16)] = f;
        nS += total & 0xffff;
        nE += total >> 16;
        state = carry;
    }
    if (state) {
        if (tid == 0) EA[nE] = F;
        ++nE;
    }
    __syncthreads();
    int R = nS;

    // ---- 1. close gaps shorter than min_silence: (SA, EA, R) -> (SB, EB, R1)
    int R1 = 0;
    for (int t0 = 0; t0 < R; t0 += VS_THREADS) {
        const int i = t0 + tid;
        const int head = i < R && (i == 0 || SA[i] - EA[i - 1] >= v.min_silence);
        int total;
        const int m = R1 + block_scan_excl(head, sc, total);
        if (head) {
            SB[m] = SA[i];
            if (i > 0) EB[m - 1] = EA[i - 1];
        }
        R1 += total;
    }
    if (R > 0 && tid == 0) EB[R1 - 1] = EA[R - 1];
    __syncthreads();

    // ---- 2. drop runs shorter than min_speech: (SB, EB, R1) -> (SA, EA, R2)
    int R2 = 0;
    for (int t0 = 0; t0 < R1; t0 += VS_THREADS) {
        const int i = t0 + tid;
        int s = 0, e = 0;
        if (i < R1) { s = SB[i]; e = EB[i]; }
        const int keep = i < R1 && e - s >= v.min_speech;
        int total;
        const int m = R2 + block_scan_excl(keep, sc, total);
        if (keep) { SA[m] = s; EA[m] = e; }
        R2 += total;
    }
    __syncthreads();

    // ---- 3. widen by pad, clip to [0, F), merge what touches or overlaps: (SA, EA, R2) -> (SB, EB, R3)
    int R3 = 0;
    for (int t0 = 0; t0 < R2; t0 += VS_THREADS) {
        const int i = t0 + tid;
        int s = 0, head = 0;
        if (i < R2) {
            s = SA[i] - v.pad;
            s = s < 0 ? 0 : s;
            int pe = 0;
            if (i > 0) {
                pe = EA[i - 1] + v.pad;
                pe = pe > F ? F : pe;
            }
            head = i == 0 || s > pe;
        }
        int total;
        const int m = R3 + block_scan_excl(head, sc, total);
        if (head) {
            SB[m] = s;
            if (i > 0) {
                const int pe = EA[i - 1] + v.pad;
                EB[m - 1] = pe > F ? F : pe;
            }
        }
        R3 += total;
    }
    if (R2 > 0 && tid == 0) {
        const int pe = EA[R2 - 1] + v.pad;
        EB[R3 - 1] = pe > F ? F : pe;
    }
    __syncthreads();

    // ---- forced split, one wave per run: count the pieces, scan the counts, write the pieces
    const int h = v.max_frames / 2;
    for (int r = wave; r < R3; r += VS_WAVES) {
        const int c = split_run(P, SB[r], EB[r], v.max_frames, h, seg, 0, 0, false);
        if (lane == 0) PC[r] = c;
    }
    __syncthreads();
    int count = 0;
    for (int t0 = 0; t0 < R3; t0 += VS_THREADS) {
        const int i = t0 + tid;
        const int c = i < R3 ? PC[i] : 0;
        int total;
        const int ex = block_scan_excl(c, sc, total);
        if (i < R3) PC[i] = count + ex;
        count += total;
    }
    __syncthreads();
    for (int r = wave; r < R3; r += VS_WAVES) split_run(P, SB[r], EB[r], v.max_frames, h, seg, PC[r], p.cap, true);

    if (tid == 0) {
        int32_t* hi = reinterpret_cast<int32_t*>(rec);
        hi[0] = count;
        hi[1] = (int)sh_bad | (count > p.cap ? 1 : 0);
        double* hd = reinterpret_cast<double*>(rec + 8);
        hd[0] = thr_on;
        hd[1] = thr_off;
        float* hf = reinterpret_cast<float*>(rec + 24);
        hf[0] = floor_p;
        hf[1] = peak_p;
    }
}

inline int64_t run_cap_of(int64_t Fmax) { return Fmax / 2 + 2; }

}  // namespace

extern "C" int w2l_vad_power(const float* x, int64_t x_stride, const int32_t* lens_dev, int N, int win, int hop, float* power,
                             int64_t power_stride, void* stream) {
    W2L_CHECK_ARG(x && lens_dev && power, "vad_power: null pointer");
    W2L_CHECK_ARG(N > 0 && N <= 65535 && x_stride > 0, "vad_power: bad sizes (N=%d, x_stride=%lld)", N, (long long)x_stride);
    W2L_CHECK_ARG(hop >= 1 && hop <= win, "vad_power: hop=%d must lie in [1, win=%d]", hop, win);
    W2L_CHECK_ARG(win <= VP_MAX_SPAN - 8, "vad_power: win=%d is above the supported %d", win, VP_MAX_SPAN - 8);
    W2L_CHECK_ARG(power_stride >= 1 && power_stride < (1LL << 24), "vad_power: power_stride=%lld frames outside [1, 2^24)",
                  (long long)power_stride);
    W2L_CHECK_ARG(power_stride >= (x_stride + hop - 1) / hop, "vad_power: power_stride=%lld is below ceil(x_stride / hop) = %lld frames",
                  (long long)power_stride, (long long)((x_stride + hop - 1) / hop));
    int fpb = (VP_MAX_SPAN - 8 - win) / hop + 1;
    fpb = fpb > VP_MAX_FPB ? VP_MAX_FPB : fpb;
    const int64_t lds_floats = (((int64_t)(fpb - 1) * hop + win + 3 + 3) & ~(int64_t)3) + VP_PARTS * 64 * 2;     // + the slice sums
    PowerParams p;
    p.x = x; p.lens = lens_dev; p.power = power; p.x_stride = x_stride; p.power_stride = power_stride;
    p.win = win; p.hop = hop; p.fpb = fpb;
    dim3 grid((unsigned)((power_stride + fpb - 1) / fpb), N);
    hipLaunchKernelGGL(vad_power_kernel, grid, dim3(VP_THREADS), (size_t)lds_floats * sizeof(float), (hipStream_t)stream, p);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t w2l_vad_workspace_bytes(int N, int Fmax) {
    if (N <= 0 || Fmax <= 0) return 0;
    return (int64_t)N * 5 * run_cap_of(Fmax) * (int64_t)sizeof(int32_t);
}

extern "C" int w2l_vad_segments(const float* power, int64_t power_stride, const int32_t* nframes_dev, int N, const w2l_vad_params_t* vp,
                                int cap, void* workspace, int64_t workspace_bytes, void* out, void* stream) {
    W2L_CHECK_ARG(power && nframes_dev && vp && workspace && out, "vad_segments: null pointer");
    W2L_CHECK_ARG(N > 0 && N <= 65535, "vad_segments: N=%d outside [1, 65535]", N);
    W2L_CHECK_ARG(power_stride >= 1 && power_stride < (1LL << 24), "vad_segments: power_stride=%lld frames outside [1, 2^24)",
                  (long long)power_stride);
    W2L_CHECK_ARG(vp->q >= 0.0 && vp->q <= 1.0, "vad_segments: q=%g outside [0, 1]", vp->q);
    W2L_CHECK_ARG(vp->max_frames >= 2, "vad_segments: max_frames=%d must be at least 2", vp->max_frames);
    W2L_CHECK_ARG(vp->min_silence >= 0 && vp->min_speech >= 0 && vp->pad >= 0 && vp->min_silence <= (1 << 24) &&
                      vp->min_speech <= (1 << 24) && vp->pad <= (1 << 24) && vp->max_frames <= (1 << 24),
                  "vad_segments: frame counts outside [0, 2^24] (min_silence=%d, min_speech=%d, pad=%d, max_frames=%d)",
                  vp->min_silence, vp->min_speech, vp->pad, vp->max_frames);
    if (vp->absolute) {
        W2L_CHECK_ARG(isfinite(vp->thr_on) && isfinite(vp->thr_off) && vp->thr_off <= vp->thr_on,
                      "vad_segments: absolute thresholds must be finite with thr_off <= thr_on (%g, %g)", vp->thr_on, vp->thr_off);
    } else {
        W2L_CHECK_ARG(isfinite(vp->r_on) && isfinite(vp->r_hyst) && isfinite(vp->abs_min) && vp->r_on > 0.0 && vp->r_hyst > 0.0 &&
                          vp->r_hyst <= 1.0 && vp->abs_min >= 0.0,
                      "vad_segments: ratios must be finite with r_on > 0, 0 < r_hyst <= 1, abs_min >= 0 (%g, %g, %g)", vp->r_on,
                      vp->r_hyst, vp->abs_min);
    }
    W2L_CHECK_ARG(cap >= 1 && cap <= (1 << 24), "vad_segments: cap=%d outside [1, 2^24]", cap);
    const int64_t need = w2l_vad_workspace_bytes(N, (int)power_stride);
    W2L_CHECK_ARG(workspace_bytes >= need, "vad_segments: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    W2L_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                  "vad_segments: workspace must be 4-byte and out 8-byte aligned");
    SegParams p;
    p.power = power; p.power_stride = power_stride; p.nframes = nframes_dev; p.v = *vp; p.cap = cap;
    p.ws = static_cast<int32_t*>(workspace); p.run_cap = run_cap_of(power_stride);
    p.out = static_cast<char*>(out); p.out_stride = VS_HEADER + 8 * (int64_t)cap;
    hipLaunchKernelGGL(vad_segments_kernel, dim3(N), dim3(VS_THREADS), 0, (hipStream_t)stream, p);
    W2L_CHECK_LAUNCH();
    return 0;
}

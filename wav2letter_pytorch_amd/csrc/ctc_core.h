// The CTC lattice shared by ctc.hip (w2l_ctc_loss) and wctc.hip (w2l_wctc_loss): the log-sum-exp helpers, the alpha/beta
// recursion, the gradient and loss-reduction kernels, the plan (block shape, LDS bytes) and the alpha/beta launcher with its
// (NT, SPT) switch.  Each kernel is a __global__ template over its caller's params type P (CtcParams, WctcParams: each stays in
// its file with its own field order); what a wildcard gap adds stands under `if constexpr (P::kWild)`, so each instantiation
// compiles to the code of a kernel written out for that type alone (profiles/ctc_core_refactor.txt).  A shared
// __device__ body called from two kernels does not.
//
// CTC structure: the alpha and the beta recursions are independent chains over time, so they run CONCURRENTLY in two workgroups
// per utterance (grid = N x 2), one lane per extended-label state, previous-step values exchanged through LDS, the next frame's
// log-probs prefetched into registers while the current step's log-sum-exp runs.  A third, fully parallel kernel turns
// alpha+beta into posteriors and the gradient.  A wildcard gap (wctc.hip) is a blank state whose emission is the constant
// p.penalty in place of lp[t][blank]: one more per-state constant and one select on the emission.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr float NEG_INF = -INFINITY;

// The recursion is a 500-step serial chain per utterance, so the per-step latency is what matters: the
// hardware v_exp_f32 / v_log_f32 forms (~1 ulp-level relative error) are used instead of libm's expf/logf.
// The log-domain values reach magnitudes of ~1e3 where one fp32 ulp (1.2e-4) already dominates that error.
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m));
}
// (one of the three terms is exp(0): with v_max3 / v_med3 / v_min3 -- one instruction each -- only the two smaller ones cost a
// transcendental; the recursion is bound by the quarter-rate v_exp / v_log issue of its waves, see ctc_alpha_beta_kernel)
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = __builtin_fmaxf(__builtin_fmaxf(a, b), c);
    if (m == NEG_INF) return NEG_INF;
    const float lo = __builtin_fminf(__builtin_fminf(a, b), c);
    const float md = __builtin_amdgcn_fmed3f(a, b, c);
    return m + __logf(1.f + __expf(md - m) + __expf(lo - m));
}

// ---------------------------------------------------------------- alpha / beta
// NT = block size (the states rounded up to whole waves, at most 1024), SPT = states per thread (1 up to 1024 states).  LP_LDS: the utterance's whole log-prob matrix (T x C fp32,
// 58 KB at T'=500) is staged in LDS once, so a time step never waits on an L2 round trip; otherwise the
// emissions are prefetched from global memory one step ahead (long utterances, T*C*4 > ~150 KB).
// P::kWild: the labels are the parsed row's (p.lab, p.S, p.status of wctc_parse_kernel) and a gap state may be a wildcard.
template <class P, int NT, int SPT, bool LP_LDS>
__global__ __launch_bounds__(NT) void ctc_alpha_beta_kernel(P p) {
    extern __shared__ float sh[];              // [2][Lpad + 4] (two guard cells on each side) | [T*C] log-probs
    const int n = blockIdx.x;
    const bool is_beta = blockIdx.y == 1;
    const int tid = threadIdx.x;
    if constexpr (P::kWild) {
        if (p.status[n] == 2) {                // a bad entry: loss and gradient 0 (block-uniform)
            if (!is_beta && tid == 0) p.nll[n] = 0.f;
            return;
        }
    }
    int S;
    if constexpr (P::kWild) S = p.S[n];
    else S = min(max(p.tg_len[n], 0), p.Smax);
    const int Tn = min(max(p.in_len[n], 0), p.T);
    const int L = 2 * S + 1;
    const int Lp = SPT * NT + 4;
    float* buf0 = sh + 2;
    float* buf1 = sh + Lp + 2;
    const float* lp = p.lp + (int64_t)n * p.T * p.C;
    if (LP_LDS) {
        float* lds_lp = sh + 2 * Lp;
        const int total = Tn * p.C;            // rows are contiguous: one linear, coalesced copy
        for (int i = tid; i < total; i += NT) lds_lp[i] = lp[i];
        lp = lds_lp;
        __syncthreads();
    }
    float* dst = (is_beta ? p.beta : p.alpha) + (int64_t)n * p.T * p.L;
    const int32_t* tg;
    [[maybe_unused]] const int32_t* wl = nullptr;
    if constexpr (P::kWild) {
        tg = p.lab + (int64_t)n * p.Smax;
        wl = p.wild + (int64_t)n * (p.Smax + 1);
    } else {
        tg = p.targets + (int64_t)n * p.Smax;
    }

    // per-state constants: label, whether the skip transition (s-2 / s+2) is allowed, whether the state is a wildcard gap
    int lab[SPT];
    bool skip[SPT], wild[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * NT;
        lab[k] = p.blank;
        skip[k] = false;
        wild[k] = false;
        if (s < L && (s & 1)) {
            lab[k] = tg[s >> 1];
            if (!is_beta) skip[k] = s >= 3 && tg[(s >> 1) - 1] != lab[k];
            else skip[k] = s + 2 < L && tg[(s >> 1) + 1] != lab[k];
        } else if constexpr (P::kWild) {
            if (s < L) wild[k] = wl[s >> 1] != 0;
        }
    }
    if (tid < 2) { buf0[-2 + tid] = NEG_INF; buf1[-2 + tid] = NEG_INF; }       // guards below state 0
    if (tid < 2) { buf0[Lp - 4 + tid] = NEG_INF; buf1[Lp - 4 + tid] = NEG_INF; }  // guards above

    if (Tn == 0) {                             // wildcard: +inf unless there is nothing to explain; its reduction applies zero_infinity
        if (!is_beta && tid == 0) {
            if constexpr (P::kWild) p.nll[n] = S == 0 ? 0.f : INFINITY;
            else p.nll[n] = S == 0 ? 0.f : (p.zero_inf ? 0.f : INFINITY);
        }
        return;
    }
    // initial column
    const int t_first = is_beta ? Tn - 1 : 0;
    float cur[SPT], nxt_lp[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * NT;
        float v = NEG_INF;
        if (s < L) {
            const bool init = is_beta ? (s >= L - 2) : (s <= 1);
            if (init) {
                if constexpr (P::kWild) v = wild[k] ? p.penalty : lp[(int64_t)t_first * p.C + lab[k]];
                else v = lp[(int64_t)t_first * p.C + lab[k]];
            }
            dst[(int64_t)t_first * p.L + s] = v;
        }
        cur[k] = v;
        buf0[s] = v;
        nxt_lp[k] = 0.f;
    }
    const int dir = is_beta ? -1 : 1;
    if (Tn > 1) {
#pragma unroll
        for (int k = 0; k < SPT; ++k)
            if (tid + k * NT < L) {
                if constexpr (P::kWild) nxt_lp[k] = wild[k] ? p.penalty : lp[(int64_t)(t_first + dir) * p.C + lab[k]];
                else nxt_lp[k] = lp[(int64_t)(t_first + dir) * p.C + lab[k]];
            }
    }
    __syncthreads();
    float* prev = buf0;
    float* next = buf1;
    for (int i = 1; i < Tn; ++i) {
        const int t = t_first + dir * i;
        float e[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) e[k] = nxt_lp[k];
        if (i + 1 < Tn) {                                   // prefetch the following frame's emissions
#pragma unroll
            for (int k = 0; k < SPT; ++k)
                if (tid + k * NT < L) {
                    if constexpr (P::kWild) nxt_lp[k] = wild[k] ? p.penalty : lp[(int64_t)(t + dir) * p.C + lab[k]];
                    else nxt_lp[k] = lp[(int64_t)(t + dir) * p.C + lab[k]];
                }
        }
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int s = tid + k * NT;
            const float a0 = cur[k];
            const float a1 = prev[s - dir];
            const float a2 = skip[k] ? prev[s - 2 * dir] : NEG_INF;
            float v = lse3(a0, a1, a2) + e[k];
            if (s >= L) v = NEG_INF;
            cur[k] = v;
            next[s] = v;
            if (s < L) dst[(int64_t)t * p.L + s] = v;
        }
        // LDS-only barrier: the alpha/beta stores and the emission prefetch stay in flight across it
        // (__syncthreads() would drain vmcnt: one L2 round trip per time step on a 500-step serial chain)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        float* tmp = prev; prev = next; next = tmp;
    }
    if (!is_beta && tid == 0) {
        const float a = prev[L - 1];
        const float b = L > 1 ? prev[L - 2] : NEG_INF;
        float nll = -lse2(a, b);
        p.nll[n] = nll;                                      // may be +inf; the grad kernel applies zero_infinity
    }
}

// ---------------------------------------------------------------- gradient, loss
// CTC:      grad[n][t][c] = (exp(lp) - posterior(t,c)) * gscale_n                       for t < in_len[n], else 0
// wildcard: grad[n][t][c] = (exp(lp) * (1 - omega(t)) - posterior(t,c)) * gscale_n
// gamma_t(s) = exp(alpha_t(s) + beta_t(s) - emission_t(s) + nll) is the state posterior (the gammas of a frame sum to 1);
// posterior(t,c) sums it over the states that emit c, omega(t) over the wildcard gaps (the 65th slot beside the 64 label
// slots).  Both are summed in the linear domain relative to the per-frame maximum of (alpha+beta-emission), whose exponent
// offset (max + nll) lies in [-log L, 0].  A wildcard gap's emission does not depend on the logits, so under
// lp = log_softmax(logits) the softmax term is weighted by what the other states hold, 1 - omega.
template <class P>
__global__ __launch_bounds__(256) void ctc_grad_kernel(P p, float* grad) {
    __shared__ float acc_all[4][P::kWild ? 65 : 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int t = blockIdx.x * 4 + w;
    if (t >= p.T) return;
    float* acc = acc_all[w];
    int S;
    if constexpr (P::kWild) S = p.S[n];
    else S = min(max(p.tg_len[n], 0), p.Smax);
    const int Tn = min(max(p.in_len[n], 0), p.T);
    const int L = 2 * S + 1;
    const float nll = p.nll[n];
    const bool inf = !(nll < INFINITY);
    float* g = grad + ((int64_t)n * p.T + t) * p.C;
    const auto bad_row = [&]() -> bool {       // a wildcard row with a bad entry; read last, only where the rest lets the frame through
        if constexpr (P::kWild) return p.status[n] == 2;
        else return false;
    };
    if (t >= Tn || (inf && p.zero_inf) || bad_row()) {
        for (int c = lane; c < p.C; c += 64) g[c] = 0.f;
        return;
    }
    const float* lp = p.lp + ((int64_t)n * p.T + t) * p.C;
    const float* al = p.alpha + ((int64_t)n * p.T + t) * p.L;
    const float* be = p.beta + ((int64_t)n * p.T + t) * p.L;
    const int32_t* tg;
    [[maybe_unused]] const int32_t* wl = nullptr;
    if constexpr (P::kWild) {
        tg = p.lab + (int64_t)n * p.Smax;
        wl = p.wild + (int64_t)n * (p.Smax + 1);
        acc[lane] = 0.f;
        if (lane == 0) acc[64] = 0.f;
    } else {
        tg = p.targets + (int64_t)n * p.Smax;
        for (int c = lane; c < 64; c += 64) acc[c] = 0.f;
    }
    float m = NEG_INF;
    for (int s = lane; s < L; s += 64) {
        [[maybe_unused]] bool wild = false;
        if constexpr (P::kWild) wild = !(s & 1) && wl[s >> 1] != 0;
        const int c = (s & 1) ? tg[s >> 1] : p.blank;
        const float v = al[s] + be[s];
        if constexpr (P::kWild) {
            if (v > NEG_INF) m = fmaxf(m, v - (wild ? p.penalty : lp[c]));
        } else {
            if (v > NEG_INF) m = fmaxf(m, v - lp[c]);
        }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    __builtin_amdgcn_wave_barrier();
    if (m > NEG_INF) {
        for (int s = lane; s < L; s += 64) {
            [[maybe_unused]] bool wild = false;
            if constexpr (P::kWild) wild = !(s & 1) && wl[s >> 1] != 0;
            const int c = (s & 1) ? tg[s >> 1] : p.blank;
            const float v = al[s] + be[s];
            if constexpr (P::kWild) {
                if (v > NEG_INF) atomicAdd(&acc[wild ? 64 : c], expf(v - (wild ? p.penalty : lp[c]) - m));
            } else {
                if (v > NEG_INF) atomicAdd(&acc[c], expf(v - lp[c] - m));
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    const float gs = 1.f / ((float)p.N * (float)max(S, 1));
    const float post_scale = m > NEG_INF ? expf(m + nll) : 0.f;
    if constexpr (P::kWild) {
        const float omega = acc[64] * post_scale;
        for (int c = lane; c < p.C; c += 64) {
            const float post = acc[c] * post_scale;
            const float e = expf(lp[c]);
            g[c] = ((e - post) - e * omega) * gs;           // omega == 0: the CTC expression, bit for bit
        }
    } else {
        for (int c = lane; c < p.C; c += 64) {
            const float post = acc[c] * post_scale;
            g[c] = (expf(lp[c]) - post) * gs;
        }
    }
}

// loss = mean over the batch of nll / max(S, 1); zero_infinity applied to nll in place.  The wildcard form also writes
// status = 1 where no path is finite (a bad row's nll is 0: its status stays 2).
// len: CTC's target lengths as the caller gave them (clamped to Smax here), the wildcard form's parsed label counts; status is
// the wildcard form's alone (CTC passes null), Smax is CTC's alone.  Plain arguments in this order, not P by value: it is the
// order on which both instantiations keep the registers and the code length of the kernels they replace.
template <class P>
__global__ void ctc_loss_reduce_kernel(float* nll, const int32_t* len, int32_t* status, int N, int zero_inf, int Smax,
                                       float* loss) {
    // single block; N is a batch size
    __shared__ float red[256];
    float s = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) {
        float v = nll[n];
        if constexpr (P::kWild) {
            if (!(v < INFINITY)) {
                status[n] = 1;
                if (zero_inf) { v = 0.f; nll[n] = 0.f; }
            }
            s += v / (float)max(len[n], 1);
        } else {
            if (zero_inf && !(v < INFINITY)) { v = 0.f; nll[n] = 0.f; }
            const int S = min(max(len[n], 0), Smax);
            s += v / (float)max(S, 1);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0] / (float)N;
}

// ---------------------------------------------------------------- host: plan and launch
struct CtcPlan {
    int nt, spt;           // block size, states per thread
    size_t lds;            // dynamic LDS bytes of the alpha/beta launch
    bool lp_lds;           // the log-probs are staged in LDS
};

// One extended-label state per thread while a block can hold them (L <= 1024: every utterance of <= ~80 s), the block just
// wide enough in waves; beyond that 1024 threads with up to 8 states each (S <= 4095: the T = 16 000 frame utterances of
// BASELINE config 5).  Round 6 measured what bounds a time step: not the barrier or the LDS round trip but the waves'
// transcendental issue (v_exp / v_log at a quarter of the rate) -- fewer, fatter threads are slower in proportion (L = 321:
// 64 x 6 states 509 us, 128 x 3 320, 256 x 2 224, 384 x 1 156 for loss + gradient at N = 32, T' = 500), idle state slots
// cost like busy ones, and two waves per SIMD hide each other's latency.
// L = 2 * Smax + 1 <= 8192 (the caller has checked it): the width of the padded row, which for wildcard rows is the raw row's.
inline CtcPlan ctc_plan(int L, int T, int C) {
    static const int kWide[] = {64, 128, 192, 256, 320, 384, 448, 512, 640, 768, 896, 1024};
    CtcPlan pl;
    pl.nt = 1024;
    for (int w : kWide)
        if (L <= w) { pl.nt = w; break; }
    pl.spt = (L + pl.nt - 1) / pl.nt;
    if (pl.spt > 1) pl.spt = pl.spt <= 4 ? pl.spt : (pl.spt <= 6 ? 6 : 8);    // the instantiated variants of the 1024-thread form
    pl.lds = 2 * (size_t)(pl.spt * pl.nt + 4) * sizeof(float);
    const size_t lp_bytes = (size_t)T * C * sizeof(float);
    pl.lp_lds = pl.lds + lp_bytes <= 150 * 1024;
    if (pl.lp_lds) pl.lds += lp_bytes;
    return pl;
}

// launches ctc_alpha_beta_kernel<P, pl.nt, pl.spt, pl.lp_lds> over p.N x 2 workgroups
template <class P>
int ctc_launch_alpha_beta(const P& p, const CtcPlan& pl, void* stream) {
    dim3 grid(p.N, 2), block(pl.nt);
#define W2L_CTC_LAUNCH(NT, SPT)                                                                                       \
    do {                                                                                                              \
        if (pl.lp_lds) {                                                                                              \
            W2L_CHECK_HIP(w2l_allow_big_lds((const void*)ctc_alpha_beta_kernel<P, NT, SPT, true>));                   \
            hipLaunchKernelGGL((ctc_alpha_beta_kernel<P, NT, SPT, true>), grid, block, pl.lds, (hipStream_t)stream, p);  \
        } else {                                                                                                      \
            hipLaunchKernelGGL((ctc_alpha_beta_kernel<P, NT, SPT, false>), grid, block, pl.lds, (hipStream_t)stream, p); \
        }                                                                                                             \
    } while (0)
    if (pl.spt == 1) {
        switch (pl.nt) {
            case 64: W2L_CTC_LAUNCH(64, 1); break;
            case 128: W2L_CTC_LAUNCH(128, 1); break;
            case 192: W2L_CTC_LAUNCH(192, 1); break;
            case 256: W2L_CTC_LAUNCH(256, 1); break;
            case 320: W2L_CTC_LAUNCH(320, 1); break;
            case 384: W2L_CTC_LAUNCH(384, 1); break;
            case 448: W2L_CTC_LAUNCH(448, 1); break;
            case 512: W2L_CTC_LAUNCH(512, 1); break;
            case 640: W2L_CTC_LAUNCH(640, 1); break;
            case 768: W2L_CTC_LAUNCH(768, 1); break;
            case 896: W2L_CTC_LAUNCH(896, 1); break;
            default: W2L_CTC_LAUNCH(1024, 1); break;
        }
    } else {
        switch (pl.spt) {
            case 2: W2L_CTC_LAUNCH(1024, 2); break;
            case 3: W2L_CTC_LAUNCH(1024, 3); break;
            case 4: W2L_CTC_LAUNCH(1024, 4); break;
            case 6: W2L_CTC_LAUNCH(1024, 6); break;
            default: W2L_CTC_LAUNCH(1024, 8); break;
        }
    }
#undef W2L_CTC_LAUNCH
    W2L_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// Wildcard CTC (gfx950): CTC whose target may hold a wildcard mark, "here is speech the transcript has no text for" (the common
// core of W-CTC, wild cards at the ends, and Star Temporal Classification, wild cards between the words).  The definition is in
// include/w2l_hip.h at w2l_wctc_loss; with no mark in a row it is w2l_ctc_loss, value for value.
//
// Structure: ctc.hip's.  A parse kernel turns each raw row (labels and marks) into labels + gap flags on the device (a block
// prefix count, no host synchronisation); then the alpha and the beta recursions run concurrently in two workgroups per utterance,
// one lane per extended-label state; a third kernel turns alpha + beta into posteriors and the gradient.  The recursion is
// ctc_alpha_beta_kernel's, restated here so that ctc.hip -- the training step's loss and this file's yardstick -- compiles to the
// code it always did: what a wildcard gap changes is one select on the emission (the constant `penalty` in place of lp[t][blank]).
// What ctc.hip's comments record as measured holds here: one state per thread while a block holds them on the same width ladder,
// the log-probabilities staged in LDS when they fit, the LDS-only barrier in the time loop.
#include "common.h"
#include <math.h>
#include <stdlib.h>

namespace {

constexpr float NEG_INF = -INFINITY;

// the hardware v_exp_f32 / v_log_f32 forms, as in ctc.hip: the per-step latency of the serial chain is what matters
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = __builtin_fmaxf(__builtin_fmaxf(a, b), c);
    if (m == NEG_INF) return NEG_INF;
    const float lo = __builtin_fminf(__builtin_fminf(a, b), c);
    const float md = __builtin_amdgcn_fmed3f(a, b, c);
    return m + __logf(1.f + __expf(md - m) + __expf(lo - m));
}

// workspace layout: log_alpha [N][T][L] | log_beta [N][T][L] (floats, L = 2*Smax+1) | labels [N][Smax] | gap flags [N][Smax+1] |
// label counts [N] (int32)
struct WctcParams {
    const float* lp;           // [N][T][C]
    const int32_t* targets;    // [N][Smax] raw rows: labels and marks
    const int32_t* in_len;
    const int32_t* tg_len;     // raw row lengths R
    int N, T, C, Smax, L, blank, zero_inf, star;
    float penalty;
    float* alpha;
    float* beta;
    float* nll;                // [N]
    int32_t* lab;              // [N][Smax]   z_1..z_S
    int32_t* wild;             // [N][Smax+1] w_0..w_S
    int32_t* S;                // [N]
    int32_t* status;           // [N]
};

// One block per raw row.  A label's place among the labels is the count of labels before it: per chunk of 256 entries a ballot
// and a popcount of the lanes below inside a wave, the four waves' totals through LDS, the chunks' running total in a register.
// Gap j's flag is written by the thread that holds label j+1 (the entry before it is a mark), the trailing gap's by thread 0, so
// every flag of 0..S is written exactly once and nothing needs clearing first.
__global__ __launch_bounds__(256) void wctc_parse_kernel(WctcParams p) {
    __shared__ int wave_cnt[4];
    __shared__ int bad_any;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int R = min(max(p.tg_len[n], 0), p.Smax);
    const int32_t* tg = p.targets + (int64_t)n * p.Smax;
    int32_t* lab = p.lab + (int64_t)n * p.Smax;
    int32_t* wild = p.wild + (int64_t)n * (p.Smax + 1);
    if (tid == 0) bad_any = 0;
    __syncthreads();
    int base = 0;
    bool bad = false;
    for (int i0 = 0; i0 < R; i0 += 256) {
        const int i = i0 + tid;
        const int v = i < R ? tg[i] : p.star;
        const bool is_lab = i < R && v != p.star;
        if (is_lab && (v < 0 || v >= p.C || v == p.blank)) bad = true;
        const unsigned long long m = __ballot(is_lab);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[w] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int k = 0; k < w; ++k) off += wave_cnt[k];
        if (is_lab) {
            const int j = off + below;                       // j < S <= R <= Smax
            lab[j] = v;
            wild[j] = i > 0 && tg[i - 1] == p.star;
        }
        base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    if (bad) bad_any = 1;
    __syncthreads();
    if (tid == 0) {
        wild[base] = R > 0 && tg[R - 1] == p.star;           // base == S <= Smax
        p.S[n] = base;
        p.status[n] = bad_any ? 2 : 0;
    }
}

// ctc_alpha_beta_kernel with the parsed labels and one more per-state constant: wild.  NT = block size, SPT = states per thread,
// LP_LDS: the utterance's log-prob matrix staged in LDS (see ctc.hip for what was measured about each).
template <int NT, int SPT, bool LP_LDS>
__global__ __launch_bounds__(NT) void wctc_alpha_beta_kernel(WctcParams p) {
    extern __shared__ float sh[];              // [2][Lpad + 4] (two guard cells on each side) | [T*C] log-probs
    const int n = blockIdx.x;
    const bool is_beta = blockIdx.y == 1;
    const int tid = threadIdx.x;
    if (p.status[n] == 2) {                    // a bad entry: loss and gradient 0 (block-uniform)
        if (!is_beta && tid == 0) p.nll[n] = 0.f;
        return;
    }
    const int S = p.S[n];
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
    const int32_t* tg = p.lab + (int64_t)n * p.Smax;
    const int32_t* wl = p.wild + (int64_t)n * (p.Smax + 1);

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
        } else if (s < L) {
            wild[k] = wl[s >> 1] != 0;
        }
    }
    if (tid < 2) { buf0[-2 + tid] = NEG_INF; buf1[-2 + tid] = NEG_INF; }       // guards below state 0
    if (tid < 2) { buf0[Lp - 4 + tid] = NEG_INF; buf1[Lp - 4 + tid] = NEG_INF; }  // guards above

    if (Tn == 0) {                             // +inf unless there is nothing to explain; the reduction applies zero_infinity
        if (!is_beta && tid == 0) p.nll[n] = S == 0 ? 0.f : INFINITY;
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
            if (init) v = wild[k] ? p.penalty : lp[(int64_t)t_first * p.C + lab[k]];
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
            if (tid + k * NT < L) nxt_lp[k] = wild[k] ? p.penalty : lp[(int64_t)(t_first + dir) * p.C + lab[k]];
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
                if (tid + k * NT < L) nxt_lp[k] = wild[k] ? p.penalty : lp[(int64_t)(t + dir) * p.C + lab[k]];
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
        // LDS-only barrier: the alpha/beta stores and the emission prefetch stay in flight across it (see ctc.hip)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        float* tmp = prev; prev = next; next = tmp;
    }
    if (!is_beta && tid == 0) {
        const float a = prev[L - 1];
        const float b = L > 1 ? prev[L - 2] : NEG_INF;
        p.nll[n] = -lse2(a, b);                              // may be +inf; the grad kernel applies zero_infinity
    }
}

// grad[n][t][c] = (exp(lp) * (1 - omega(t)) - posterior(t,c)) * gscale_n   for t < in_len[n], else 0
// gamma_t(s) = exp(alpha_t(s) + beta_t(s) - emission_t(s) + nll) is the state posterior (the gammas of a frame sum to 1);
// posterior(t,c) sums it over the label and plain-gap states that emit c, omega(t) over the wildcard gaps (the 65th slot beside
// the 64 label slots).  A wildcard gap's emission does not depend on the logits, so under lp = log_softmax(logits) the softmax
// term is weighted by what the other states hold, 1 - omega; with omega == 0 this is ctc_grad_kernel's formula.
__global__ __launch_bounds__(256) void wctc_grad_kernel(WctcParams p, float* grad) {
    __shared__ float acc_all[4][65];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int t = blockIdx.x * 4 + w;
    if (t >= p.T) return;
    float* acc = acc_all[w];
    const int S = p.S[n];
    const int Tn = min(max(p.in_len[n], 0), p.T);
    const int L = 2 * S + 1;
    const float nll = p.nll[n];
    const bool inf = !(nll < INFINITY);
    float* g = grad + ((int64_t)n * p.T + t) * p.C;
    if (t >= Tn || (inf && p.zero_inf) || p.status[n] == 2) {
        for (int c = lane; c < p.C; c += 64) g[c] = 0.f;
        return;
    }
    const float* lp = p.lp + ((int64_t)n * p.T + t) * p.C;
    const float* al = p.alpha + ((int64_t)n * p.T + t) * p.L;
    const float* be = p.beta + ((int64_t)n * p.T + t) * p.L;
    const int32_t* tg = p.lab + (int64_t)n * p.Smax;
    const int32_t* wl = p.wild + (int64_t)n * (p.Smax + 1);
    acc[lane] = 0.f;
    if (lane == 0) acc[64] = 0.f;
    float m = NEG_INF;
    for (int s = lane; s < L; s += 64) {
        const bool wild = !(s & 1) && wl[s >> 1] != 0;
        const int c = (s & 1) ? tg[s >> 1] : p.blank;
        const float v = al[s] + be[s];
        if (v > NEG_INF) m = fmaxf(m, v - (wild ? p.penalty : lp[c]));
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    __builtin_amdgcn_wave_barrier();
    if (m > NEG_INF) {
        for (int s = lane; s < L; s += 64) {
            const bool wild = !(s & 1) && wl[s >> 1] != 0;
            const int c = (s & 1) ? tg[s >> 1] : p.blank;
            const float v = al[s] + be[s];
            if (v > NEG_INF) atomicAdd(&acc[wild ? 64 : c], expf(v - (wild ? p.penalty : lp[c]) - m));
        }
    }
    __builtin_amdgcn_wave_barrier();
    const float gs = 1.f / ((float)p.N * (float)max(S, 1));
    const float post_scale = m > NEG_INF ? expf(m + nll) : 0.f;
    const float omega = acc[64] * post_scale;
    for (int c = lane; c < p.C; c += 64) {
        const float post = acc[c] * post_scale;
        const float e = expf(lp[c]);
        g[c] = ((e - post) - e * omega) * gs;               // omega == 0: ctc_grad_kernel's expression, bit for bit
    }
}

__global__ void wctc_loss_reduce_kernel(float* nll, const int32_t* S_of, int32_t* status, int N, int zero_inf, float* loss) {
    // single block; N is a batch size
    __shared__ float red[256];
    float s = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) {
        float v = nll[n];
        if (!(v < INFINITY)) {
            status[n] = 1;                                   // no finite path (a bad row's nll is 0: its status stays 2)
            if (zero_inf) { v = 0.f; nll[n] = 0.f; }
        }
        s += v / (float)max(S_of[n], 1);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0] / (float)N;
}

}  // namespace

extern "C" int64_t w2l_wctc_workspace_bytes(int N, int T, int Smax) {
    if (N <= 0 || T <= 0 || Smax < 0) return 0;
    return 2 * (int64_t)N * T * (2 * Smax + 1) * (int64_t)sizeof(float) + (int64_t)N * (2 * Smax + 2) * (int64_t)sizeof(int32_t);
}

extern "C" int w2l_wctc_loss(const float* log_probs, const int32_t* targets, const int32_t* input_lengths,
                             const int32_t* target_lengths, int N, int T, int C, int Smax, int blank, int zero_infinity, int star,
                             float penalty, float* nll, float* loss, float* grad, int32_t* status, void* workspace,
                             void* stream) {
    W2L_CHECK_ARG(log_probs && input_lengths && target_lengths && nll && loss && status && workspace, "wctc_loss: null pointer");
    W2L_CHECK_ARG(targets || Smax == 0, "wctc_loss: null targets");
    W2L_CHECK_ARG(N > 0 && T > 0 && C > 0 && C <= 64 && Smax >= 0 && blank >= 0 && blank < C, "wctc_loss: bad sizes");
    W2L_CHECK_ARG(star != blank, "wctc_loss: the wildcard id %d is the blank", star);
    W2L_CHECK_ARG(penalty <= 0.f, "wctc_loss: penalty %g must be <= 0 (a log-domain cost per frame)", (double)penalty);
    const int L = 2 * Smax + 1;
    W2L_CHECK_ARG(L <= 8 * 1024, "wctc_loss: target length %d too long (max 4095)", Smax);
    WctcParams p;
    p.lp = log_probs; p.targets = targets; p.in_len = input_lengths; p.tg_len = target_lengths;
    p.N = N; p.T = T; p.C = C; p.Smax = Smax; p.L = L; p.blank = blank; p.zero_inf = zero_infinity;
    p.star = star; p.penalty = penalty;
    p.alpha = (float*)workspace;
    p.beta = p.alpha + (int64_t)N * T * L;
    p.nll = nll;
    p.lab = (int32_t*)(p.beta + (int64_t)N * T * L);
    p.wild = p.lab + (int64_t)N * Smax;
    p.S = p.wild + (int64_t)N * (Smax + 1);
    p.status = status;
    hipLaunchKernelGGL(wctc_parse_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, p);
    W2L_CHECK_LAUNCH();
    // the block width by the raw row width (S <= Smax): w2l_ctc_loss's ladder and its rounding of the states per thread
    static const int kWide[] = {64, 128, 192, 256, 320, 384, 448, 512, 640, 768, 896, 1024};
    int nt = 1024;
    for (int w : kWide)
        if (L <= w) { nt = w; break; }
    int spt = (L + nt - 1) / nt;
    if (spt > 1) spt = spt <= 4 ? spt : (spt <= 6 ? 6 : 8);    // the instantiated variants of the 1024-thread form
    dim3 grid(N, 2), block(nt);
    size_t lds = 2 * (size_t)(spt * nt + 4) * sizeof(float);
    const size_t lp_bytes = (size_t)T * C * sizeof(float);
    const bool lp_lds = lds + lp_bytes <= 150 * 1024;
    if (lp_lds) lds += lp_bytes;
#define W2L_WCTC_LAUNCH(NT, SPT)                                                                              \
    do {                                                                                                      \
        if (lp_lds) {                                                                                         \
            W2L_CHECK_HIP(w2l_allow_big_lds((const void*)wctc_alpha_beta_kernel<NT, SPT, true>));             \
            hipLaunchKernelGGL((wctc_alpha_beta_kernel<NT, SPT, true>), grid, block, lds, (hipStream_t)stream, p);  \
        } else {                                                                                              \
            hipLaunchKernelGGL((wctc_alpha_beta_kernel<NT, SPT, false>), grid, block, lds, (hipStream_t)stream, p); \
        }                                                                                                     \
    } while (0)
    if (spt == 1) {
        switch (nt) {
            case 64: W2L_WCTC_LAUNCH(64, 1); break;
            case 128: W2L_WCTC_LAUNCH(128, 1); break;
            case 192: W2L_WCTC_LAUNCH(192, 1); break;
            case 256: W2L_WCTC_LAUNCH(256, 1); break;
            case 320: W2L_WCTC_LAUNCH(320, 1); break;
            case 384: W2L_WCTC_LAUNCH(384, 1); break;
            case 448: W2L_WCTC_LAUNCH(448, 1); break;
            case 512: W2L_WCTC_LAUNCH(512, 1); break;
            case 640: W2L_WCTC_LAUNCH(640, 1); break;
            case 768: W2L_WCTC_LAUNCH(768, 1); break;
            case 896: W2L_WCTC_LAUNCH(896, 1); break;
            default: W2L_WCTC_LAUNCH(1024, 1); break;
        }
    } else {
        switch (spt) {
            case 2: W2L_WCTC_LAUNCH(1024, 2); break;
            case 3: W2L_WCTC_LAUNCH(1024, 3); break;
            case 4: W2L_WCTC_LAUNCH(1024, 4); break;
            case 6: W2L_WCTC_LAUNCH(1024, 6); break;
            default: W2L_WCTC_LAUNCH(1024, 8); break;
        }
    }
#undef W2L_WCTC_LAUNCH
    W2L_CHECK_LAUNCH();
    if (grad) {
        hipLaunchKernelGGL(wctc_grad_kernel, dim3((T + 3) / 4, N), dim3(256), 0, (hipStream_t)stream, p, grad);
        W2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(wctc_loss_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nll, p.S, status, N, zero_infinity,
                       loss);
    W2L_CHECK_LAUNCH();
    return 0;
}

// Wildcard CTC (gfx950): CTC whose target may hold a wildcard mark, "here is speech the transcript has no text for" (the common
// core of W-CTC, wild cards at the ends, and Star Temporal Classification, wild cards between the words).  The definition is in
// include/w2l_hip.h at w2l_wctc_loss; with no mark in a row it is w2l_ctc_loss, value for value.
//
// This file holds what only the wildcard form has: its params and the parse kernel, which turns each raw row (labels and marks)
// into labels + gap flags on the device (a block prefix count, no host synchronisation).  The alpha/beta recursion, the gradient
// and the loss reduction that follow are ctc_core.h's kernels instantiated on WctcParams (kWild: the labels come from the parsed
// row, a wildcard gap's emission is the constant `penalty` in place of lp[t][blank], the reduction writes the status), on
// ctc_core.h's plan and launcher: the same width ladder, LDS staging and LDS-only barrier as w2l_ctc_loss.
#include "ctc_core.h"
#include <stdlib.h>

namespace {

// workspace layout: log_alpha [N][T][L] | log_beta [N][T][L] (floats, L = 2*Smax+1) | labels [N][Smax] | gap flags [N][Smax+1] |
// label counts [N] (int32)
struct WctcParams {
    static constexpr bool kWild = true;
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
    // the block width by the raw row width (S <= Smax): the labels are counted on the device, the host never reads them
    const CtcPlan pl = ctc_plan(L, T, C);
    if (int rc = ctc_launch_alpha_beta(p, pl, stream)) return rc;
    if (grad) {
        hipLaunchKernelGGL(ctc_grad_kernel<WctcParams>, dim3((T + 3) / 4, N), dim3(256), 0, (hipStream_t)stream, p, grad);
        W2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ctc_loss_reduce_kernel<WctcParams>, dim3(1), dim3(256), 0, (hipStream_t)stream, nll,
                       (const int32_t*)p.S, status, N, zero_infinity, Smax, loss);
    W2L_CHECK_LAUNCH();
    return 0;
}

// log_softmax / softmax over the label axis, CTC loss (alpha-beta, log domain) with its
// gradient, and the greedy-decode argmax (gfx950).
//
// Replaces F.log_softmax / F.softmax (wav2letter.py:86-87, jasper.py:469-473),
// nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True) forward AND backward
// (base_asr_models.py:23,81,90; torch native _ctc_loss / _ctc_loss_backward) and
// torch.max(probs, 2) (decoder.py:136).
//
// The CTC kernels (alpha/beta recursion, gradient, loss reduction), their plan and their launcher are ctc_core.h's, shared
// with wctc.hip; this file holds the params they are instantiated on and the entry point.
#include "ctc_core.h"
#include <stdlib.h>

namespace {

// ---------------------------------------------------------------- softmax family
// one wave per row; C <= 64 * PER (label sets here: 29)
__global__ __launch_bounds__(256) void log_softmax_fwd_kernel(const float* logits, int64_t rows, int C, int CP, int mode,
                                                               float* out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* src = logits + row * CP;
    float m = NEG_INF;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, src[c]);
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(src[c] - m);
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
    const float lse = m + logf(s);
    for (int c = lane; c < C; c += 64) {
        const float lp = src[c] - lse;
        out[row * C + c] = mode == 0 ? lp : expf(lp);
    }
}

// mode 0: g_logit = g - exp(out) * sum(g);  mode 1 (softmax): g_logit = out * (g - sum(g*out))
__global__ __launch_bounds__(256) void log_softmax_bwd_kernel(const float* gout, const float* out, int64_t rows, int C,
                                                               int mode, float* glogits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* g = gout + row * C;
    const float* o = out + row * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += mode == 0 ? g[c] : g[c] * o[c];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
    for (int c = lane; c < C; c += 64)
        glogits[row * C + c] = mode == 0 ? g[c] - expf(o[c]) * s : o[c] * (g[c] - s);
}

// ---------------------------------------------------------------- CTC
// what ctc_core.h's kernels are instantiated on here; workspace layout (floats): log_alpha [N][T][L] | log_beta [N][T][L],
// L = 2*Smax+1
struct CtcParams {
    static constexpr bool kWild = false;
    const float* lp;           // [N][T][C]
    const int32_t* targets;    // [N][Smax]
    const int32_t* in_len;
    const int32_t* tg_len;
    int N, T, C, Smax, L, blank, zero_inf;
    float* alpha;
    float* beta;
    float* nll;                // [N]
};

// ---------------------------------------------------------------- argmax (ties -> lowest index)
__global__ __launch_bounds__(256) void argmax_kernel(const float* probs, int64_t rows, int C, int32_t* idx) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const float* p = probs + row * C;
    float best = p[0];
    int bi = 0;
    bool nan_found = best != best;
    for (int c = 1; c < C && !nan_found; ++c) {
        const float v = p[c];
        if (v != v) { bi = c; nan_found = true; }          // torch.max propagates the first NaN
        else if (v > best) { best = v; bi = c; }
    }
    idx[row] = bi;
}

}  // namespace

extern "C" int w2l_log_softmax_fwd(const float* logits, int N, int T, int C, int CP, int mode, float* out, void* stream) {
    W2L_CHECK_ARG(logits && out && N > 0 && T > 0 && C > 0 && CP >= C, "log_softmax_fwd: bad arguments");
    const int64_t rows = (int64_t)N * T;
    hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       logits, rows, C, CP, mode, out);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int w2l_log_softmax_bwd(const float* gout, const float* out, int N, int T, int C, int mode, float* glogits,
                                   void* stream) {
    W2L_CHECK_ARG(gout && out && glogits && N > 0 && T > 0 && C > 0, "log_softmax_bwd: bad arguments");
    const int64_t rows = (int64_t)N * T;
    hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, gout,
                       out, rows, C, mode, glogits);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t w2l_ctc_workspace_bytes(int N, int T, int Smax) {
    if (N <= 0 || T <= 0 || Smax < 0) return 0;
    return 2 * (int64_t)N * T * (2 * Smax + 1) * (int64_t)sizeof(float);
}

extern "C" int w2l_ctc_loss(const float* log_probs, const int32_t* targets, const int32_t* input_lengths,
                            const int32_t* target_lengths, int N, int T, int C, int Smax, int blank, int zero_infinity,
                            float* nll, float* loss, float* grad, void* workspace, void* stream) {
    W2L_CHECK_ARG(log_probs && input_lengths && target_lengths && nll && loss && workspace, "ctc_loss: null pointer");
    W2L_CHECK_ARG(targets || Smax == 0, "ctc_loss: null targets");
    W2L_CHECK_ARG(N > 0 && T > 0 && C > 0 && C <= 64 && Smax >= 0 && blank >= 0 && blank < C, "ctc_loss: bad sizes");
    const int L = 2 * Smax + 1;
    W2L_CHECK_ARG(L <= 8 * 1024, "ctc_loss: target length %d too long (max 4095)", Smax);
    CtcParams p;
    p.lp = log_probs; p.targets = targets; p.in_len = input_lengths; p.tg_len = target_lengths;
    p.N = N; p.T = T; p.C = C; p.Smax = Smax; p.L = L; p.blank = blank; p.zero_inf = zero_infinity;
    p.alpha = (float*)workspace;
    p.beta = p.alpha + (int64_t)N * T * L;
    p.nll = nll;
    const CtcPlan pl = ctc_plan(L, T, C);
    if (int rc = ctc_launch_alpha_beta(p, pl, stream)) return rc;
    if (grad) {
        hipLaunchKernelGGL(ctc_grad_kernel<CtcParams>, dim3((T + 3) / 4, N), dim3(256), 0, (hipStream_t)stream, p, grad);
        W2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ctc_loss_reduce_kernel<CtcParams>, dim3(1), dim3(256), 0, (hipStream_t)stream, nll, target_lengths,
                       (int32_t*)nullptr, N, zero_infinity, Smax, loss);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int w2l_argmax(const float* probs, int64_t rows, int C, int32_t* idx, void* stream) {
    W2L_CHECK_ARG(probs && idx && rows > 0 && C > 0, "argmax: bad arguments");
    hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, probs, rows,
                       C, idx);
    W2L_CHECK_LAUNCH();
    return 0;
}

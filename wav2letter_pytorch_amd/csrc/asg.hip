// Auto Segmentation criterion (ASG, Collobert et al. 2016, "Wav2Letter", section 2.3) and its Viterbi decoder (gfx950).
//
// The criterion of the Wav2Letter paper, which the reference replaces by CTC (its README, "Differences from article").  No blank
// label; a learned A x A transition matrix g[i][j] (label j at frame t after label i at frame t-1); normalised over ALL label
// paths:  loss = Z_full - Z_tgt with
//   Z_full = logsumexp over the A^T frame paths of  sum_t x[t][pi_t] + sum_{t>=1} g[pi_{t-1}][pi_t]
//   Z_tgt  = the same sum over the paths that read the (repeat-encoded) target, every label held for at least one frame.
//
// Structure, after ctc.hip: the four recursions of an utterance -- full alpha, full beta, target alpha, target beta -- are
// independent chains over time and run CONCURRENTLY in four workgroups (grid = N x 4), log domain, the next frame's emissions
// prefetched into registers while the current frame's log-sum-exp runs.
//   full chains    one wave; lane j keeps column g[:, j] (beta: row g[j, :]) in registers, the previous frame's A values are
//                  read across the wave (v_readlane with constant lane numbers: scalars, no LDS), a max pass and a sum-exp
//                  pass per frame, the loop unrolled over the label count padded to 32 or 64 with -inf in the padding.
//   target chains  one lane per target state, neighbours exchanged through LDS with one LDS-only barrier per frame, exactly
//                  as ctc_alpha_beta_kernel; the stay / advance scores are read from g through the target labels once.
//   The repetition encoding of the transcripts (label `repeat` stands for "the previous letter again") happens in the target
//   chains' prologue, in LDS.
// A fully parallel combine kernel (grid = frame chunks x N) turns the four tables into d loss / d x and one slab of
// d loss / d g per block; the last kernel adds the slabs in a fixed order (no float atomics anywhere: the results are
// bit-reproducible from run to run) and reduces the loss.
#include "common.h"
#include <math.h>

namespace {

constexpr float NEG_INF = -INFINITY;
constexpr int TCH = 64;            // frames per block of the combine kernel
constexpr int TP_MAX = 8192;       // floats of its target-posterior staging buffer (>= the largest Smax)
constexpr int VIT_CH = 512;        // frames of back-pointers staged in LDS per back-trace chunk

__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m));
}
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float exp_or_zero(float v) { return v > NEG_INF ? expf(v) : 0.f; }

struct AsgParams {
    const float* x;            // [N][T][A]
    const float* g;            // [A][A]
    const int32_t* targets;    // [N][Smax] raw transcripts
    const int32_t* in_len;
    const int32_t* tg_len;
    int N, T, A, Smax, Sp, repeat, reduction, chunks;
    float* fa;                 // [N][T][A]   full alpha
    float* fb;                 // [N][T][A]   full beta (includes the frame's own emission)
    float* ta;                 // [N][T][Sp]  target alpha
    float* tb;                 // [N][T][Sp]  target beta
    int32_t* yenc;             // [N][Sp]     encoded targets
    float* zf;                 // [N]
    float* zt;                 // [N]
    float* slabs;              // [N][chunks][A*A]
    int32_t* status;           // [N] 0 ok, 1 infeasible (S = 0 or S > T_n), 2 bad label
};

// ---------------------------------------------------------------- full recursion: one wave
// alpha_t(j) = x[t][j] + lse_i(alpha_{t-1}(i) + g[i][j]);  beta_t(i) = x[t][i] + lse_j(g[i][j] + beta_{t+1}(j))
template <int AP>
__device__ __forceinline__ void asg_full_chain(const AsgParams& p, int n, bool is_beta) {
    const int lane = threadIdx.x;
    const int A = p.A;
    const int Tn = min(max(p.in_len[n], 0), p.T);
    if (Tn == 0) {
        if (!is_beta && lane == 0) p.zf[n] = 0.f;
        return;
    }
    const bool live = lane < A;
    float gc[AP];
#pragma unroll
    for (int k = 0; k < AP; ++k) {
        float v = NEG_INF;
        if (live && k < A) v = is_beta ? p.g[lane * A + k] : p.g[k * A + lane];
        gc[k] = v;
    }
    const float* x = p.x + (int64_t)n * p.T * A;
    float* dst = (is_beta ? p.fb : p.fa) + (int64_t)n * p.T * A;
    const int dir = is_beta ? -1 : 1;
    int t = is_beta ? Tn - 1 : 0;
    float cur = live ? x[(int64_t)t * A + lane] : NEG_INF;
    if (live) dst[(int64_t)t * A + lane] = cur;
    float nxt = 0.f;
    if (Tn > 1 && live) nxt = x[(int64_t)(t + dir) * A + lane];
    for (int i = 1; i < Tn; ++i) {
        t += dir;
        const float e = nxt;
        if (i + 1 < Tn && live) nxt = x[(int64_t)(t + dir) * A + lane];      // prefetch the following frame's emission
        float m = NEG_INF;
#pragma unroll
        for (int k = 0; k < AP; ++k) m = fmaxf(m, lane_value(cur, k) + gc[k]);
        const float ms = m == NEG_INF ? 0.f : m;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < AP; ++k) s += __expf(lane_value(cur, k) + gc[k] - ms);
        float v = e + ms + __logf(s);
        if (!live) v = NEG_INF;
        cur = v;
        if (live) dst[(int64_t)t * A + lane] = v;
    }
    if (!is_beta) {
        float m = cur;
#pragma unroll
        for (int k = 32; k > 0; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
        float s = m == NEG_INF ? 0.f : expf(cur - m);
#pragma unroll
        for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
        if (lane == 0) p.zf[n] = m == NEG_INF ? NEG_INF : m + logf(s);
    }
}

// ---------------------------------------------------------------- target recursion: one lane per target state
// alpha_t(s) = x[t][y_s] + lse(alpha_{t-1}(s) + g[y_s][y_s], alpha_{t-1}(s-1) + g[y_{s-1}][y_s]), starts in state 0;
// beta_t(s)  = x[t][y_s] + lse(beta_{t+1}(s) + g[y_s][y_s],  beta_{t+1}(s+1) + g[y_s][y_{s+1}]),  starts in state S-1
template <int NT, int SPT>
__device__ __forceinline__ void asg_target_chain(const AsgParams& p, int n, bool is_beta, float* sh) {
    constexpr int Lw = NT * SPT;
    // LDS: int flag, pad[3] | int yl[Lw] | float [2][Lw + 2] columns (one guard cell on each side); the raw transcript is
    // staged in the columns' space before they are used
    int* sh_flag = (int*)sh;
    int* yl = (int*)sh + 4;
    float* buf0 = sh + 4 + Lw + 1;
    float* buf1 = buf0 + Lw + 2;
    int* raw = (int*)(sh + 4 + Lw);
    const int tid = threadIdx.x;
    const int A = p.A;
    const int S = min(max(p.tg_len[n], 0), p.Smax);
    const int Tn = min(max(p.in_len[n], 0), p.T);
    const int32_t* tg = p.targets + (int64_t)n * p.Smax;
    if (tid == 0) sh_flag[0] = 0;
    for (int s = tid; s < S; s += NT) raw[s] = tg[s];
    __syncthreads();
    // repetition encoding: the 2nd, 4th, ... member of a run of equal labels becomes `repeat`
    bool bad = false;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * NT;
        int enc = 0;
        if (s < S) {
            const int v = raw[s];
            if (v < 0 || v >= A || v == p.repeat) bad = true;
            int back = 0;
            while (s - back - 1 >= 0 && raw[s - back - 1] == v) ++back;
            enc = (back & 1) ? p.repeat : v;
        }
        yl[s] = enc;
    }
    if (bad) sh_flag[0] = 1;
    __syncthreads();
    const int status = sh_flag[0] ? 2 : ((S == 0 || S > Tn) ? 1 : 0);
    if (!is_beta) {
        for (int s = tid; s < S; s += NT) p.yenc[(int64_t)n * p.Sp + s] = status == 2 ? 0 : yl[s];
        if (tid == 0) {
            p.status[n] = status;
            if (status != 0) p.zt[n] = 0.f;
        }
    }
    if (status != 0) return;

    const float* x = p.x + (int64_t)n * p.T * A;
    float* dst = (is_beta ? p.tb : p.ta) + (int64_t)n * p.T * p.Sp;
    const int dir = is_beta ? -1 : 1;
    int lab[SPT];
    float g_stay[SPT], g_adv[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * NT;
        lab[k] = 0;
        g_stay[k] = NEG_INF;
        g_adv[k] = NEG_INF;
        if (s < S) {
            lab[k] = yl[s];
            g_stay[k] = p.g[lab[k] * A + lab[k]];
            if (!is_beta && s >= 1) g_adv[k] = p.g[yl[s - 1] * A + lab[k]];
            if (is_beta && s + 1 < S) g_adv[k] = p.g[lab[k] * A + yl[s + 1]];
        }
    }
    __syncthreads();                                   // every read of yl / raw is done: the columns take raw's space
    if (tid == 0) { buf0[-1] = NEG_INF; buf1[-1] = NEG_INF; buf0[Lw] = NEG_INF; buf1[Lw] = NEG_INF; }
    const int t_first = is_beta ? Tn - 1 : 0;
    const int s_first = is_beta ? S - 1 : 0;
    float cur[SPT], nxt[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * NT;
        float v = NEG_INF;
        if (s == s_first) v = x[(int64_t)t_first * A + lab[k]];
        if (s < S) dst[(int64_t)t_first * p.Sp + s] = v;
        cur[k] = v;
        buf0[s] = v;
        nxt[k] = 0.f;
        if (Tn > 1 && s < S) nxt[k] = x[(int64_t)(t_first + dir) * A + lab[k]];
    }
    __syncthreads();
    float* prev = buf0;
    float* next = buf1;
    for (int i = 1; i < Tn; ++i) {
        const int t = t_first + dir * i;
        float e[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) e[k] = nxt[k];
        if (i + 1 < Tn) {
#pragma unroll
            for (int k = 0; k < SPT; ++k)
                if (tid + k * NT < S) nxt[k] = x[(int64_t)(t + dir) * A + lab[k]];
        }
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int s = tid + k * NT;
            float v = lse2(cur[k] + g_stay[k], prev[s - dir] + g_adv[k]) + e[k];
            if (s >= S) v = NEG_INF;
            cur[k] = v;
            next[s] = v;
            if (s < S) dst[(int64_t)t * p.Sp + s] = v;
        }
        // LDS-only barrier (as ctc_alpha_beta_kernel): the table stores and the emission prefetch stay in flight across it
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        float* tmp = prev; prev = next; next = tmp;
    }
    if (!is_beta && tid == 0) p.zt[n] = prev[S - 1];
}

template <int AP, int NT, int SPT>
__global__ __launch_bounds__(NT) void asg_chains_kernel(AsgParams p) {
    extern __shared__ float sh[];
    const int n = blockIdx.x;
    const int role = blockIdx.y;                       // 0 full alpha, 1 full beta, 2 target alpha, 3 target beta
    if (role < 2) {
        if (threadIdx.x < 64) asg_full_chain<AP>(p, n, role == 1);
        return;
    }
    asg_target_chain<NT, SPT>(p, n, role == 3, sh);
}

// ---------------------------------------------------------------- gradients
// block (c, n): frames [c * TCH, (c + 1) * TCH) of utterance n.
//   d/dx[t][i]  = w_n (P_full(pi_t = i) - P_tgt(pi_t = i))
//   slab[i][j]  = w_n sum_{t in chunk, t >= 1} (P_full(pi_{t-1} = i, pi_t = j) - P_tgt(...)), every sum in a fixed order
// w_n = 1 / (N max(S_n, 1)) ('mean') or 1 ('sum').
__global__ __launch_bounds__(256) void asg_grad_kernel(AsgParams p, float* grad_x, int tpn) {
    extern __shared__ float sh[];
    const int A = p.A, AA = A * A;
    float* fa_l = sh;                                  // [(TCH + 1)][A]: rows t0 - 1 .. t1 - 1
    float* fb_l = fa_l + (TCH + 1) * A;                // [TCH][A]
    int* yl = (int*)(fb_l + TCH * A);                  // [Sp]
    float* stay = (float*)(yl + p.Sp);                 // [Sp]
    float* adv = stay + p.Sp;                          // [Sp]
    float* tp = adv + p.Sp;                            // [tpn]
    const int tid = threadIdx.x;
    const int n = blockIdx.y, c = blockIdx.x;
    const int t0 = c * TCH, t1 = min(t0 + TCH, p.T);
    const int S = min(max(p.tg_len[n], 0), p.Smax);
    const int Tn = min(max(p.in_len[n], 0), p.T);
    const int te = min(t1, Tn);
    float* gx = grad_x + (int64_t)n * p.T * A;
    float* slab = p.slabs + ((int64_t)n * p.chunks + c) * AA;
    if (p.status[n] != 0 || t0 >= Tn) {
        for (int i = tid; i < (t1 - t0) * A; i += 256) gx[(int64_t)t0 * A + i] = 0.f;
        for (int i = tid; i < AA; i += 256) slab[i] = 0.f;
        return;
    }
    const float w = p.reduction == 0 ? 1.f / ((float)p.N * (float)max(S, 1)) : 1.f;
    const float zf = p.zf[n], zt = p.zt[n];
    const float* x = p.x + (int64_t)n * p.T * A;
    const float* fa = p.fa + (int64_t)n * p.T * A;
    const float* fb = p.fb + (int64_t)n * p.T * A;
    const float* ta = p.ta + (int64_t)n * p.T * p.Sp;
    const float* tb = p.tb + (int64_t)n * p.T * p.Sp;
    const int nf = te - t0;                            // valid frames of the chunk, >= 1
    for (int i = tid; i < (nf + 1) * A; i += 256) {
        const int64_t src = (int64_t)(t0 - 1) * A + i;
        fa_l[i] = src >= 0 ? fa[src] : 0.f;
    }
    for (int i = tid; i < nf * A; i += 256) fb_l[i] = fb[(int64_t)t0 * A + i];
    for (int s = tid; s < S; s += 256) yl[s] = p.yenc[(int64_t)n * p.Sp + s];
    __syncthreads();
    const int tlo = max(t0, 1);
    // target transitions of the chunk, one thread per state, frames in order
    for (int s = tid; s < S; s += 256) {
        const int y = yl[s];
        const float gs = p.g[y * A + y];
        const float ga = s > 0 ? p.g[yl[s - 1] * A + y] : 0.f;
        float acc_s = 0.f, acc_a = 0.f;
        for (int t = tlo; t < te; ++t) {
            const float b = tb[(int64_t)t * p.Sp + s];
            acc_s += exp_or_zero(ta[(int64_t)(t - 1) * p.Sp + s] + gs + b - zt);
            if (s > 0) acc_a += exp_or_zero(ta[(int64_t)(t - 1) * p.Sp + s - 1] + ga + b - zt);
        }
        stay[s] = acc_s;
        adv[s] = acc_a;
    }
    __syncthreads();
    // one thread per (i, j): the full transitions of the chunk, minus the target's through the encoded labels
    for (int q = tid; q < AA; q += 256) {
        const int i = q / A, j = q - i * A;
        const float gij = p.g[q];
        float acc = 0.f;
        for (int t = tlo; t < te; ++t) acc += exp_or_zero(fa_l[(t - t0) * A + i] + gij + fb_l[(t - t0) * A + j] - zf);
        float sub = 0.f;
        if (i == j) {
            for (int s = 0; s < S; ++s)
                if (yl[s] == i) sub += stay[s];
        } else {
            for (int s = 1; s < S; ++s)
                if (yl[s] == j && yl[s - 1] == i) sub += adv[s];
        }
        slab[q] = (acc - sub) * w;
    }
    // emissions, in passes of as many frames as the target-posterior buffer holds
    const int fb_frames = max(1, tpn / max(S, 1));
    for (int ps = t0; ps < te; ps += fb_frames) {
        const int pe = min(ps + fb_frames, te);
        __syncthreads();
        for (int i = tid; i < (pe - ps) * S; i += 256) {
            const int r = i / S, s = i - r * S, t = ps + r;
            const float v = ta[(int64_t)t * p.Sp + s] + tb[(int64_t)t * p.Sp + s];
            tp[i] = v > NEG_INF ? expf(v - x[(int64_t)t * A + yl[s]] - zt) : 0.f;
        }
        __syncthreads();
        for (int q = tid; q < (pe - ps) * A; q += 256) {
            const int r = q / A, i = q - r * A, t = ps + r;
            const int s_lo = max(0, S - (Tn - t)), s_hi = min(S - 1, t);      // the states a path can be in at frame t
            float pt = 0.f;
            for (int s = s_lo; s <= s_hi; ++s)
                if (yl[s] == i) pt += tp[r * S + s];
            const float v = fa_l[(t - t0 + 1) * A + i] + fb_l[(t - t0) * A + i];
            const float pf = v > NEG_INF ? expf(v - x[(int64_t)t * A + i] - zf) : 0.f;
            gx[(int64_t)t * A + i] = (pf - pt) * w;
        }
    }
    for (int i = tid; i < (t1 - te) * A; i += 256) gx[(int64_t)te * A + i] = 0.f;
}

// slabs added in (utterance, chunk) order; block 0 also forms nll[n] and the reduced loss
__global__ __launch_bounds__(256) void asg_finish_kernel(AsgParams p, float* nll, float* loss, float* grad_trans) {
    const int AA = p.A * p.A;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (grad_trans != nullptr && q < AA) {
        float acc = 0.f;
        const int64_t total = (int64_t)p.N * p.chunks;
        for (int64_t k = 0; k < total; ++k) acc += p.slabs[k * AA + q];
        grad_trans[q] = acc;
    }
    if (blockIdx.x != 0) return;
    for (int n = threadIdx.x; n < p.N; n += 256) nll[n] = p.status[n] == 0 ? p.zf[n] - p.zt[n] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int n = 0; n < p.N; ++n) {
            const int S = min(max(p.tg_len[n], 0), p.Smax);
            s += p.reduction == 0 ? nll[n] / (float)max(S, 1) : nll[n];
        }
        loss[0] = p.reduction == 0 ? s / (float)p.N : s;
    }
}

// ---------------------------------------------------------------- Viterbi: one wave per utterance
// score_t(j) = x[t][j] + max_i(score_{t-1}(i) + g[i][j]), ties -> the lowest i; the best final label, ties -> the lowest;
// one byte of back-pointer per (frame, label) in the workspace (rows of AP bytes), walked back by lane 0 through LDS chunks
template <int AP>
__global__ __launch_bounds__(64) void asg_viterbi_kernel(const float* xs, const float* g, const int32_t* in_len, int N, int T,
                                                        int A, uint8_t* ws, int32_t* path_out, float* score) {
    __shared__ uint32_t bp_l[VIT_CH * AP / 4];
    const int lane = threadIdx.x;
    const int n = blockIdx.x;
    const int Tn = in_len ? min(max(in_len[n], 0), T) : T;
    int32_t* path = path_out + (int64_t)n * T;
    for (int t = Tn + lane; t < T; t += 64) path[t] = -1;
    if (Tn == 0) {
        if (lane == 0) score[n] = 0.f;
        return;
    }
    const bool live = lane < A;
    float gc[AP];
#pragma unroll
    for (int k = 0; k < AP; ++k) gc[k] = (live && k < A) ? g[k * A + lane] : NEG_INF;
    const float* x = xs + (int64_t)n * T * A;
    uint8_t* bp = ws + (int64_t)n * T * AP;
    float cur = live ? x[lane] : NEG_INF;
    float nxt = 0.f;
    if (Tn > 1 && live) nxt = x[A + lane];
    for (int t = 1; t < Tn; ++t) {
        const float e = nxt;
        if (t + 1 < Tn && live) nxt = x[(int64_t)(t + 1) * A + lane];
        float best = NEG_INF;
        int bi = 0;
#pragma unroll
        for (int k = 0; k < AP; ++k) {
            const float v = lane_value(cur, k) + gc[k];
            if (v > best) { best = v; bi = k; }
        }
        cur = live ? e + best : NEG_INF;
        if (lane < AP) bp[(int64_t)t * AP + lane] = (uint8_t)bi;
    }
    float val = cur;
    int idx = lane;
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        const float ov = __shfl_xor(val, k, 64);
        const int oi = __shfl_xor(idx, k, 64);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
    if (lane == 0) score[n] = val;
    __syncthreads();                                   // the back-pointer stores have landed
    int lab = idx;
    const uint32_t* bp32 = (const uint32_t*)bp;        // (rows of AP bytes: every row is 4-byte aligned)
    for (int cb = ((Tn - 1) / VIT_CH) * VIT_CH; cb >= 0; cb -= VIT_CH) {
        const int hi = min(cb + VIT_CH, Tn);
        const int words = (hi - cb) * (AP / 4);
        for (int i = lane; i < words; i += 64) bp_l[i] = bp32[(int64_t)cb * (AP / 4) + i];
        __syncthreads();
        if (lane == 0) {
            const uint8_t* b = (const uint8_t*)bp_l;
            for (int t = hi - 1; t >= cb; --t) {
                path[t] = lab;
                if (t > 0) lab = b[(t - cb) * AP + lab];
            }
        }
        __syncthreads();
    }
}

struct AsgPlan {
    int ap, nt, spt, sp, chunks, tpn;
    size_t lds_chain, lds_grad;
    int64_t off_fb, off_ta, off_tb, off_yenc, off_zf, off_zt, off_slabs, bytes;
};

// the shapes alone decide block shape and workspace layout (the workspace query and the launch must agree)
bool asg_plan(int N, int T, int A, int Smax, AsgPlan* pl) {
    if (N <= 0 || T <= 0 || T > (1 << 20) || A <= 0 || A > 64 || Smax < 0 || Smax > 4095) return false;
    pl->ap = A <= 32 ? 32 : 64;
    pl->sp = Smax > 0 ? Smax : 1;
    static const int kWide[] = {64, 128, 256, 512, 1024};
    int nt = 1024;
    for (int w : kWide)
        if (pl->sp <= w) { nt = w; break; }
    int spt = (pl->sp + nt - 1) / nt;
    if (spt == 3) spt = 4;
    pl->nt = nt;
    pl->spt = spt;
    pl->chunks = (T + TCH - 1) / TCH;
    pl->tpn = (int)((int64_t)TCH * pl->sp < TP_MAX ? TCH * pl->sp : TP_MAX);
    const size_t lw = (size_t)nt * spt;
    pl->lds_chain = (4 + lw + 2 * (lw + 2)) * sizeof(float);
    pl->lds_grad = ((size_t)(2 * TCH + 1) * A + 3 * (size_t)pl->sp + (size_t)pl->tpn) * sizeof(float);
    const int64_t full = (int64_t)N * T * A, tgt = (int64_t)N * T * pl->sp;
    int64_t off = full;                                // (in floats; fa at 0)
    pl->off_fb = off; off += full;
    pl->off_ta = off; off += tgt;
    pl->off_tb = off; off += tgt;
    pl->off_yenc = off; off += (int64_t)N * pl->sp;
    pl->off_zf = off; off += N;
    pl->off_zt = off; off += N;
    pl->off_slabs = off; off += (int64_t)N * pl->chunks * A * A;
    pl->bytes = off * (int64_t)sizeof(float);
    return true;
}

}  // namespace

extern "C" int64_t w2l_asg_workspace_bytes(int N, int T, int A, int Smax) {
    AsgPlan pl;
    return asg_plan(N, T, A, Smax, &pl) ? pl.bytes : -1;
}

extern "C" int w2l_asg_loss(const float* x, const float* transitions, const int32_t* targets, const int32_t* input_lengths,
                            const int32_t* target_lengths, int N, int T, int A, int Smax, int repeat_index, int reduction,
                            float* nll, float* loss, float* grad_x, float* grad_trans, int32_t* status, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    W2L_CHECK_ARG(x && transitions && input_lengths && target_lengths && nll && loss && status && workspace,
                  "asg_loss: null pointer");
    W2L_CHECK_ARG(targets || Smax == 0, "asg_loss: null targets");
    W2L_CHECK_ARG((grad_x == nullptr) == (grad_trans == nullptr), "asg_loss: grad_x and grad_trans go together");
    W2L_CHECK_ARG(reduction == 0 || reduction == 1, "asg_loss: reduction is 0 (mean) or 1 (sum)");
    AsgPlan pl;
    W2L_CHECK_ARG(asg_plan(N, T, A, Smax, &pl), "asg_loss: N=%d T=%d A=%d (max 64) Smax=%d (max 4095) out of range", N, T, A,
                  Smax);
    W2L_CHECK_ARG(repeat_index >= 0 && repeat_index < A, "asg_loss: repeat_index %d outside [0, %d)", repeat_index, A);
    W2L_CHECK_ARG(workspace_bytes >= pl.bytes, "asg_loss: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)pl.bytes);
    AsgParams p;
    p.x = x; p.g = transitions; p.targets = targets; p.in_len = input_lengths; p.tg_len = target_lengths;
    p.N = N; p.T = T; p.A = A; p.Smax = Smax; p.Sp = pl.sp; p.repeat = repeat_index; p.reduction = reduction;
    p.chunks = pl.chunks;
    float* ws = (float*)workspace;
    p.fa = ws; p.fb = ws + pl.off_fb; p.ta = ws + pl.off_ta; p.tb = ws + pl.off_tb;
    p.yenc = (int32_t*)(ws + pl.off_yenc); p.zf = ws + pl.off_zf; p.zt = ws + pl.off_zt; p.slabs = ws + pl.off_slabs;
    p.status = status;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(N, 4), block(pl.nt);
#define W2L_ASG_LAUNCH(AP, NT, SPT) \
    hipLaunchKernelGGL((asg_chains_kernel<AP, NT, SPT>), grid, block, pl.lds_chain, st, p)
#define W2L_ASG_SHAPES(AP)                                      \
    do {                                                        \
        if (pl.spt == 4) W2L_ASG_LAUNCH(AP, 1024, 4);           \
        else if (pl.spt == 2) W2L_ASG_LAUNCH(AP, 1024, 2);      \
        else if (pl.nt == 64) W2L_ASG_LAUNCH(AP, 64, 1);        \
        else if (pl.nt == 128) W2L_ASG_LAUNCH(AP, 128, 1);      \
        else if (pl.nt == 256) W2L_ASG_LAUNCH(AP, 256, 1);      \
        else if (pl.nt == 512) W2L_ASG_LAUNCH(AP, 512, 1);      \
        else W2L_ASG_LAUNCH(AP, 1024, 1);                       \
    } while (0)
    if (pl.ap == 32) W2L_ASG_SHAPES(32);
    else W2L_ASG_SHAPES(64);
#undef W2L_ASG_SHAPES
#undef W2L_ASG_LAUNCH
    W2L_CHECK_LAUNCH();
    if (grad_x != nullptr) {
        if (pl.lds_grad > 64 * 1024) W2L_CHECK_HIP(w2l_allow_big_lds((const void*)asg_grad_kernel));
        hipLaunchKernelGGL(asg_grad_kernel, dim3(pl.chunks, N), dim3(256), pl.lds_grad, st, p, grad_x, pl.tpn);
        W2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(asg_finish_kernel, dim3((A * A + 255) / 256), dim3(256), 0, st, p, nll, loss, grad_trans);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t w2l_asg_viterbi_workspace_bytes(int N, int T, int A) {
    if (N <= 0 || T <= 0 || T > (1 << 20) || A <= 0 || A > 64) return -1;
    return (int64_t)N * T * (A <= 32 ? 32 : 64);
}

extern "C" int w2l_asg_viterbi(const float* x, const float* transitions, const int32_t* input_lengths, int N, int T, int A,
                               void* workspace, int64_t workspace_bytes, int32_t* path, float* score, void* stream) {
    W2L_CHECK_ARG(x && transitions && workspace && path && score, "asg_viterbi: null pointer");
    const int64_t need = w2l_asg_viterbi_workspace_bytes(N, T, A);
    W2L_CHECK_ARG(need >= 0, "asg_viterbi: N=%d T=%d A=%d (max 64) out of range", N, T, A);
    W2L_CHECK_ARG(workspace_bytes >= need, "asg_viterbi: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)need);
    if (A <= 32)
        hipLaunchKernelGGL(asg_viterbi_kernel<32>, dim3(N), dim3(64), 0, (hipStream_t)stream, x, transitions, input_lengths, N,
                           T, A, (uint8_t*)workspace, path, score);
    else
        hipLaunchKernelGGL(asg_viterbi_kernel<64>, dim3(N), dim3(64), 0, (hipStream_t)stream, x, transitions, input_lengths, N,
                           T, A, (uint8_t*)workspace, path, score);
    W2L_CHECK_LAUNCH();
    return 0;
}

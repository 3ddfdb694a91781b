// CTC forced alignment (gfx950): the Viterbi (max instead of sum) form of the CTC recursion of ctc.hip, with back-pointers,
// the back-trace and the per-token first / last frames written by the same launch.
//
// Gives the beam-search decoders the character offsets the reference's decoder refuses (decoder.py:238, "Prefix beam search
// does not support offsets (yet)"), in GreedyDecoder's format (decoder.py:104-119), and users forced alignment of a known
// transcript (alignment.ctc_forced_align; host model: alignment.viterbi_align_host).
//
// Structure: one workgroup per utterance, one lane per extended-label state (1024 threads with several states each above
// 1024 states), the previous column exchanged through LDS with one LDS-only barrier per frame, emissions prefetched PF frames
// ahead into registers.  The loop holds compares and adds only.  A state's moves (0 stay, 1 from s-1, 2 from s-2) are packed
// over TIME, 16 frames to a 32-bit word per state, so packing needs no cross-lane traffic and a word store is coalesced over
// states; the words live in LDS when they fit, else in the caller's workspace.  Wave 0 walks the moves back, then every thread
// turns the state sequence into labels, starts and ends.
//
// The params struct, the plan (block shape, LDS or workspace), the workspace query and the launcher are align_core.h's, shared
// with w2l_asg_align; asg_align_kernel (asg_beam.hip) has this kernel's structure with ASG's recurrence.
#include "align_core.h"

namespace {

struct CtcRule {                               // what align_core.h's plan and launcher ask of a criterion
    static constexpr const char* NAME = "ctc_align";
    static constexpr int GUARD = 2, MAX_SPT = 8, MAX_STATES = 8 * 1024;
    static int states(int S) { return 2 * S + 1; }
    static size_t lds_round(size_t bytes) { return bytes; }
};

struct AlignParams {
    const float* x;            // [N][T][A] log-probabilities, or probabilities if is_prob
    const int32_t* in_len;     // [N] or null (all T)
    const int32_t* targets;    // row n at targets + n * tg_stride
    const int32_t* tg_len;     // utterance n at tg_len[n * len_stride]
    int64_t tg_stride, len_stride;
    int N, T, A, Smax, blank, is_prob, bp_lds;
    uint32_t* bp_global;       // [N][chunks][Lw] when !bp_lds
    float* score;              // [N]
    int32_t* status;           // [N]
    int32_t* path;             // [N][T]
    int32_t* starts;           // [N][Smax]
    int32_t* ends;             // [N][Smax]
};

// NT threads, SPT states per thread (state s = tid + k * NT), PF = frames of emissions held ahead in registers.
template <int NT, int SPT>
__global__ __launch_bounds__(NT) void ctc_align_kernel(AlignParams p) {
    constexpr int PF = SPT == 1 ? 8 : (SPT == 2 ? 4 : 2);
    constexpr int Lw = NT * SPT;
    // all LDS is dynamic (a static array beside a 160 KiB dynamic limit is refused): int flag[2] (bad input seen, end state),
    // float score, pad | [2][Lw + 2] columns (two guard cells below state 0) | uint16 st[T] | moves (bp_lds)
    extern __shared__ float sh_all[];
    int* sh_flag = (int*)sh_all;
    float& sh_score = sh_all[2];
    float* sh = sh_all + 4;
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    const int S = min(max(p.tg_len[(int64_t)n * p.len_stride], 0), p.Smax);
    const int Tn = p.in_len ? min(max(p.in_len[n], 0), p.T) : p.T;
    const int L = 2 * S + 1;
    const int chunks = (p.T + 15) >> 4;
    float* buf0 = sh + 2;
    float* buf1 = sh + (Lw + 2) + 2;
    uint16_t* st = (uint16_t*)(sh + 2 * (Lw + 2));
    uint32_t* bp_l = (uint32_t*)(st + ((p.T + 1) & ~1));
    uint32_t* bp_g = p.bp_global + (int64_t)n * chunks * Lw;
    const float* x = p.x + (int64_t)n * p.T * p.A;
    const int32_t* tg = p.targets + (int64_t)n * p.tg_stride;
    int32_t* path = p.path + (int64_t)n * p.T;
    int32_t* starts = p.starts + (int64_t)n * p.Smax;
    int32_t* ends = p.ends + (int64_t)n * p.Smax;

    if (tid < 2) { buf0[-2 + tid] = NEG_INF; buf1[-2 + tid] = NEG_INF; sh_flag[tid] = 0; }
    __syncthreads();

    // per-state constants; a target outside [0, A) or equal to the blank is an error, and is never used as an index
    int lab[SPT];
    bool skip[SPT];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * NT;
        lab[k] = p.blank;
        skip[k] = false;
        if (s < L && (s & 1)) {
            const int v = tg[s >> 1];
            if (v < 0 || v >= p.A || v == p.blank) bad = true;
            else lab[k] = v;
            skip[k] = s >= 3 && tg[(s >> 1) - 1] != v;
        }
    }
    if (p.is_prob) {                   // every probability of the valid frames: negative or NaN is an error
        const int64_t total = (int64_t)Tn * p.A;
        for (int64_t i = tid; i < total; i += NT) bad |= !(x[i] >= 0.f);
    }
    if (bad) sh_flag[0] = 1;
    __syncthreads();
    int status = sh_flag[0] ? 2 : 0;
    float best_score = NEG_INF;

    if (status == 0 && Tn > 0) {
        // ---- forward: column 0, then frames 1 .. Tn-1 in blocks of PF frames whose emissions were loaded a block earlier
        float cur[SPT], e_nxt[PF][SPT];
        uint32_t bw[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int s = tid + k * NT;
            float v = NEG_INF;
            if (s < L && s <= 1) {
                v = x[lab[k]];
                if (p.is_prob) v = logf(v);
            }
            cur[k] = v;
            buf0[s] = v;
            bw[k] = 0;
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int tt = min(1 + j, Tn - 1);
#pragma unroll
            for (int k = 0; k < SPT; ++k) e_nxt[j][k] = x[(int64_t)tt * p.A + lab[k]];
        }
        __syncthreads();
        float* prev = buf0;
        float* next = buf1;
        for (int tb = 1; tb < Tn; tb += PF) {
            float e[PF][SPT];
#pragma unroll
            for (int j = 0; j < PF; ++j)
#pragma unroll
                for (int k = 0; k < SPT; ++k) e[j][k] = p.is_prob ? logf(e_nxt[j][k]) : e_nxt[j][k];
            if (tb + PF < Tn) {
#pragma unroll
                for (int j = 0; j < PF; ++j) {
                    const int tt = min(tb + PF + j, Tn - 1);
#pragma unroll
                    for (int k = 0; k < SPT; ++k) e_nxt[j][k] = x[(int64_t)tt * p.A + lab[k]];
                }
            }
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int t = tb + j;
                if (t >= Tn) break;
#pragma unroll
                for (int k = 0; k < SPT; ++k) {
                    const int s = tid + k * NT;
                    float best = cur[k];                                   // ties: stay, then s-1, then s-2
                    uint32_t mv = 0;
                    const float a1 = prev[s - 1];
                    const float a2 = skip[k] ? prev[s - 2] : NEG_INF;
                    if (a1 > best) { best = a1; mv = 1; }
                    if (a2 > best) { best = a2; mv = 2; }
                    float v = best == NEG_INF ? NEG_INF : best + e[j][k];
                    if (s >= L) v = NEG_INF;
                    cur[k] = v;
                    next[s] = v;
                    bw[k] |= mv << (2 * (t & 15));
                }
                if ((t & 15) == 15 || t == Tn - 1) {
#pragma unroll
                    for (int k = 0; k < SPT; ++k) {
                        const int s = tid + k * NT;
                        if (p.bp_lds) bp_l[(t >> 4) * Lw + s] = bw[k];
                        else bp_g[(int64_t)(t >> 4) * Lw + s] = bw[k];
                        bw[k] = 0;
                    }
                }
                // LDS-only barrier (as ctc_alpha_beta_kernel): prefetched emissions and move stores stay in flight across it
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                float* tmp = prev; prev = next; next = tmp;
            }
        }
        if (tid == 0) {                                                    // end: the last label wins a tie with the blank
            const float a = prev[L - 1];
            const float b = L > 1 ? prev[L - 2] : NEG_INF;
            int s_end = L - 1;
            float sc = a;
            if (L > 1 && b >= a) { s_end = L - 2; sc = b; }
            sh_flag[1] = s_end;
            sh_score = sc;
        }
        __syncthreads();                                                   // also drains the move stores to the workspace
        best_score = sh_score;
        if (!(best_score > NEG_INF)) status = 1;
        if (status == 0 && tid < 64) {
            // ---- back-trace, wave 0, every lane the same walk (lane 0 records it).  Moves in the workspace: one coalesced
            // load of the 64 states at and below the current one per 16-frame chunk (a chunk moves down at most 32 states).
            int s = sh_flag[1];
            for (int c = (Tn - 1) >> 4; c >= 0; --c) {
                const int base = s - 63;
                uint32_t w = 0;
                if (!p.bp_lds && base + tid >= 0) w = bp_g[(int64_t)c * Lw + base + tid];
                const int t_hi = min(Tn - 1, c * 16 + 15), t_lo = max(c * 16, 1);
                for (int t = t_hi; t >= t_lo; --t) {
                    const uint32_t word = p.bp_lds ? bp_l[c * Lw + s] : (uint32_t)__shfl((int)w, s - base, 64);
                    if (tid == 0) st[t] = (uint16_t)s;
                    s -= (int)((word >> (2 * (t & 15))) & 3u);
                }
            }
            if (tid == 0) st[0] = (uint16_t)s;
        }
        __syncthreads();
    } else if (status == 0) {          // no frames: only the empty target has a path (the empty one)
        if (S > 0) status = 1;
        else best_score = 0.f;
    }

    // ---- outputs: labels of the walked states, first / last frame of each token's own state, -1 elsewhere
    const bool ok = status == 0;
    for (int t = tid; t < p.T; t += NT) {
        int label = -1;
        if (ok && t < Tn) {
            const int s = st[t];
            label = p.blank;
            if (s & 1) {
                label = tg[s >> 1];
                if (t == 0 || st[t - 1] != s) starts[s >> 1] = t;
                if (t == Tn - 1 || st[t + 1] != s) ends[s >> 1] = t;
            }
        }
        path[t] = label;
    }
    for (int j = (ok ? S : 0) + tid; j < p.Smax; j += NT) { starts[j] = -1; ends[j] = -1; }
    if (tid == 0) {
        p.score[n] = ok ? best_score : NEG_INF;
        p.status[n] = status;
    }
}

struct CtcAlignKernels {
    template <int NT, int SPT>
    static auto get() { return ctc_align_kernel<NT, SPT>; }
};

}  // namespace

extern "C" int64_t w2l_ctc_align_workspace_bytes(int N, int T, int Smax) { return align_workspace_bytes<CtcRule>(N, T, Smax); }

extern "C" int w2l_ctc_align(const float* x, const int32_t* input_lengths, const int32_t* targets, int64_t target_stride,
                             const int32_t* target_lengths, int64_t length_stride, int N, int T, int A, int Smax, int blank,
                             int log_probs, void* workspace, int64_t workspace_bytes, float* score, int32_t* status,
                             int32_t* path, int32_t* starts, int32_t* ends, void* stream) {
    W2L_CHECK_ARG(x && target_lengths && score && status && path, "ctc_align: null pointer");
    W2L_CHECK_ARG(Smax == 0 || (targets && starts && ends), "ctc_align: null targets / starts / ends");
    W2L_CHECK_ARG(N > 0 && T > 0 && A > 0 && Smax >= 0 && blank >= 0 && blank < A, "ctc_align: bad sizes");
    W2L_CHECK_ARG(target_stride >= Smax && length_stride >= 1, "ctc_align: bad strides");
    AlignParams p;
    p.x = x; p.in_len = input_lengths; p.targets = targets; p.tg_len = target_lengths;
    p.tg_stride = target_stride; p.len_stride = length_stride;
    p.N = N; p.T = T; p.A = A; p.Smax = Smax; p.blank = blank; p.is_prob = !log_probs;
    p.score = score; p.status = status; p.path = path; p.starts = starts; p.ends = ends;
    return align_launch<CtcRule, CtcAlignKernels>(p, workspace, workspace_bytes, stream);
}

// CTC keyword search (gfx950): where in the posteriors is a phrase said, and how well?  Forced alignment (ctc_align.hip) with
// a free start and a free end, for many keywords at once, scored against the best unconstrained path (keyword_search.py has
// the definition; host model: keyword_search.keyword_scan_host / pick_hits_host).  No reference counterpart.
//
// With b[t] = max_a lp[t][a] and e[t][s] = lp[t][lab(s)] - b[t] <= 0, over a keyword's 2 S - 1 extended states c_1, blank,
// c_2, ..., c_S (no leading or trailing blank):
//   D[t][s] = e[t][s] + max(D[t-1][s], D[t-1][s-1], skip(s) ? D[t-1][s-2] : -inf, first(s) ? 0 : -inf)
// a candidate wins on a strict > only, in that order (stay, s-1, s-2, enter), and B[t][s] -- the frame at which the winning
// path entered -- travels with D (t for "enter"), so there are no back-pointers and no back-trace.  end_score[t] = D[t][last],
// end_start[t] = B[t][last].
//
// Three launches:
//   kws_frame_max_kernel  b[N][T] once per utterance (in the log domain; NaN marks a frame that is an error), status[n] = 0 / 2
//   kws_scan_kernel<NT>   the states of many keywords concatenated into blocks of NT lanes (keyword_search.KeywordTable packs
//                         them; a keyword is never split), one lane per state, one workgroup per (block, utterance); the loop
//                         is ctc_align_kernel's: the previous column (D and B side by side, one 8-byte LDS cell per state) goes
//                         through LDS with one LDS-only barrier per frame, emissions are prefetched PF frames ahead, the body
//                         holds compares, adds and selects only; lanes of last states write the two curves each frame
//   kws_pick_kernel       one wave per (utterance, keyword): up to max_hits rounds of a masked arg-max over the curve under the
//                         key (score descending, start ascending, end descending), then the hits in start order
// The table is device memory the entry point never reads: the kernels bound every index they take from it.
#include "align_core.h"
#include "../../include/w2l_hip.h"

namespace {

// meta = keyword index << 4 | flags (LABEL: a label's state, else the blank between two labels); -1: a lane without a state
constexpr int KWS_FIRST = 1, KWS_LAST = 2, KWS_SKIP = 4, KWS_LABEL = 8;
constexpr int KWS_MAX_T = 32768, KWS_MAX_K = 4096, KWS_MAX_HITS = 64, KWS_MAX_N = 65535;

struct KwsParams {
    const float* x;            // [N][T][A] log-probabilities, or probabilities if is_prob
    const int32_t* in_len;     // [N] or null (all T)
    const int32_t* labels;     // [n_blocks][width]
    const int32_t* meta;       // [n_blocks][width]
    const int32_t* block_kw;   // [n_blocks + 1]
    const float* thr;          // [K]
    int N, T, A, K, blank, is_prob, n_blocks, max_hits;
    float* bmax;               // [N][T]
    int32_t* frame_bad;        // [N]: the frame pass's verdict, which the scan reads (status also takes the scan's own)
    float* end_score;          // [N][K][T]
    int32_t* end_start;        // [N][K][T]
    int32_t* hit_count;        // [N][K]
    w2l_kws_hit_t* hits;       // [N][K][max_hits]
    int32_t* status;           // [N]
};

__device__ __forceinline__ int kws_frames(const KwsParams& p, int n) { return p.in_len ? min(max(p.in_len[n], 0), p.T) : p.T; }

// one workgroup per utterance, one thread per frame: the frame's maximum in the log domain.  An error (status 2): a NaN, a
// negative probability, or no finite maximum (all -inf, all zero, +inf).
__global__ __launch_bounds__(256) void kws_frame_max_kernel(KwsParams p) {
    __shared__ int sh_bad;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int Tn = kws_frames(p, n);
    const float* x = p.x + (int64_t)n * p.T * p.A;
    float* bm = p.bmax + (int64_t)n * p.T;
    if (tid == 0) sh_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int t = tid; t < p.T; t += 256) {
        float m = NEG_INF;
        if (t < Tn) {
            const float* row = x + (int64_t)t * p.A;
            bool nan = false;
            for (int a = 0; a < p.A; ++a) {
                const float v = row[a];
                nan |= p.is_prob ? !(v >= 0.f) : v != v;
                m = fmaxf(m, v);
            }
            if (p.is_prob) m = logf(m);
            if (nan || !(m > NEG_INF) || !(m < INFINITY)) { m = __builtin_nanf(""); bad = true; }
        }
        bm[t] = m;
    }
    if (bad) sh_bad = 1;
    __syncthreads();
    if (tid == 0) { p.status[n] = sh_bad ? 2 : 0; p.frame_bad[n] = sh_bad; }
}

// block (blockIdx.x, utterance blockIdx.y): NT lanes, lane = state.  PF = frames of emissions held ahead in registers.
template <int NT>
__global__ __launch_bounds__(NT) void kws_scan_kernel(KwsParams p) {
    constexpr int PF = 8;
    __shared__ int2 col[2][NT + 2];            // (D as bits, B); two guard cells at -inf below state 0
    __shared__ int sh_bad;
    const int blk = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int Tn = kws_frames(p, n);
    const float* x = p.x + (int64_t)n * p.T * p.A;
    const float* bm = p.bmax + (int64_t)n * p.T;
    const int2 dead = make_int2(__float_as_int(NEG_INF), -1);

    // per-state constants; a label outside [0, A) or equal to the blank is an error and never an index
    const int m = p.meta[(int64_t)blk * NT + tid];
    const int kw = m >> 4;
    const bool active = m >= 0 && kw < p.K;
    const bool first = active && (m & KWS_FIRST), last = active && (m & KWS_LAST), skip = active && (m & KWS_SKIP);
    int lab = p.blank;
    bool bad = false;
    if (active && (m & KWS_LABEL)) {
        const int v = p.labels[(int64_t)blk * NT + tid];
        if (v < 0 || v >= p.A || v == p.blank) bad = true;
        else lab = v;
    }
    if (tid == 0) sh_bad = 0;
    if (tid < 2) { col[0][tid] = dead; col[1][tid] = dead; }
    __syncthreads();
    if (bad) sh_bad = 1;
    col[0][tid + 2] = dead;
    __syncthreads();
    const bool bad_block = sh_bad != 0;
    if (bad_block && tid == 0) atomicOr(&p.status[n], 2);
    const bool run = !bad_block && p.frame_bad[n] == 0;
    // the keywords of this block, for the cooperative fills (bounded: the table is not trusted)
    const int k0 = min(max(p.block_kw[blk], 0), p.K), k1 = min(max(p.block_kw[blk + 1], k0), p.K);
    const int t_done = run ? Tn : 0;

    if (run && Tn > 0) {
        float* out_d = p.end_score + ((int64_t)n * p.K + (last ? kw : 0)) * p.T;
        int32_t* out_b = p.end_start + ((int64_t)n * p.K + (last ? kw : 0)) * p.T;
        float cur_d = NEG_INF;
        int cur_b = -1;
        float x_nxt[PF], b_nxt[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int tt = min(j, Tn - 1);
            x_nxt[j] = x[(int64_t)tt * p.A + lab];
            b_nxt[j] = bm[tt];
        }
        int2* prev = col[0] + 2;
        int2* next = col[1] + 2;
        for (int tb = 0; tb < Tn; tb += PF) {
            float e[PF];
#pragma unroll
            for (int j = 0; j < PF; ++j) e[j] = (p.is_prob ? logf(x_nxt[j]) : x_nxt[j]) - b_nxt[j];
            if (tb + PF < Tn) {
#pragma unroll
                for (int j = 0; j < PF; ++j) {
                    const int tt = min(tb + PF + j, Tn - 1);
                    x_nxt[j] = x[(int64_t)tt * p.A + lab];
                    b_nxt[j] = bm[tt];
                }
            }
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int t = tb + j;
                if (t >= Tn) break;
                const int2 c1 = prev[tid - 1], c2 = prev[tid - 2];
                float best = cur_d;                                    // ties: stay, s-1, s-2, enter
                int bb = cur_b;
                const float a1 = first ? NEG_INF : __int_as_float(c1.x);
                const float a2 = skip ? __int_as_float(c2.x) : NEG_INF;
                if (a1 > best) { best = a1; bb = c1.y; }
                if (a2 > best) { best = a2; bb = c2.y; }
                if (first && 0.f > best) { best = 0.f; bb = t; }
                float v = active ? best + e[j] : NEG_INF;
                if (!(v > NEG_INF)) { v = NEG_INF; bb = -1; }
                cur_d = v;
                cur_b = bb;
                next[tid] = make_int2(__float_as_int(v), bb);
                if (last) { out_d[t] = v; out_b[t] = bb; }
                // LDS-only barrier (as ctc_align_kernel): prefetched emissions and curve stores stay in flight across it
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                int2* tmp = prev; prev = next; next = tmp;
            }
        }
    }
    // frames from the utterance's length on (all of them where nothing ran): -inf and -1, coalesced along t
    const int64_t tail = p.T - t_done;
    for (int64_t i = tid; i < (int64_t)(k1 - k0) * tail; i += NT) {
        const int64_t at = ((int64_t)n * p.K + k0 + i / tail) * p.T + t_done + i % tail;
        p.end_score[at] = NEG_INF;
        p.end_start[at] = -1;
    }
}

// (score descending, start ascending, end descending): does candidate a come before b?  A frame index of -1 is "none".
struct KwsCand { float sc; int st, en; };
__device__ __forceinline__ bool kws_before(const KwsCand& a, const KwsCand& b) {
    if (b.en < 0) return a.en >= 0;
    if (a.en < 0) return false;
    if (a.sc != b.sc) return a.sc > b.sc;
    if (a.st != b.st) return a.st < b.st;
    return a.en > b.en;
}

// one wave per (keyword blockIdx.x, utterance blockIdx.y)
__global__ __launch_bounds__(64) void kws_pick_kernel(KwsParams p) {
    __shared__ int acc_s[KWS_MAX_HITS], acc_e[KWS_MAX_HITS];
    __shared__ float acc_v[KWS_MAX_HITS];
    const int k = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    const int64_t row = (int64_t)n * p.K + k;
    const float* sc = p.end_score + row * p.T;
    const int32_t* st = p.end_start + row * p.T;
    const int Tn = p.status[n] == 0 ? kws_frames(p, n) : 0;
    const float thr = p.thr[k];
    int count = 0;
    for (int r = 0; r < p.max_hits; ++r) {
        KwsCand best = {NEG_INF, -1, -1};
        for (int t = lane; t < Tn; t += 64) {
            const KwsCand c = {sc[t], st[t], t};
            if (!(c.sc >= thr) || c.st < 0 || c.st > t) continue;
            bool free_ = true;
            for (int h = 0; h < count; ++h) free_ &= c.st > acc_e[h] || acc_s[h] > t;
            if (free_ && kws_before(c, best)) best = c;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            KwsCand o;
            o.sc = __shfl_xor(best.sc, d, 64);
            o.st = __shfl_xor(best.st, d, 64);
            o.en = __shfl_xor(best.en, d, 64);
            if (kws_before(o, best)) best = o;
        }
        if (best.en < 0) break;                                        // (the same answer in every lane)
        if (lane == 0) { acc_s[count] = best.st; acc_e[count] = best.en; acc_v[count] = best.sc; }
        ++count;
        __syncthreads();
    }
    // accepted segments do not overlap, so their starts are distinct: a hit's place is the number of earlier starts
    w2l_kws_hit_t* out = p.hits + row * p.max_hits;
    if (lane < count) {
        int rank = 0;
        for (int h = 0; h < count; ++h) rank += acc_s[h] < acc_s[lane];
        out[rank].start = acc_s[lane];
        out[rank].end = acc_e[lane];
        out[rank].score = acc_v[lane];
    } else if (lane < p.max_hits) {
        out[lane].start = -1;
        out[lane].end = -1;
        out[lane].score = NEG_INF;
    }
    if (lane == 0) p.hit_count[row] = count;
}

bool kws_plan(int N, int T, int K, int max_hits) {
    return N >= 1 && N <= KWS_MAX_N && T >= 1 && T <= KWS_MAX_T && K >= 1 && K <= KWS_MAX_K && max_hits >= 1 &&
           max_hits <= KWS_MAX_HITS;
}

}  // namespace

extern "C" int64_t w2l_ctc_kws_workspace_bytes(int N, int T, int K, int max_hits) {
    if (!kws_plan(N, T, K, max_hits)) return -1;
    return (int64_t)N * T * (int64_t)sizeof(float) + (int64_t)N * (int64_t)sizeof(int32_t);
}

extern "C" int w2l_ctc_kws(const float* x, const int32_t* input_lengths, int N, int T, int A, int blank, int log_probs,
                           const w2l_kws_table_t* table, const float* thr, int max_hits, int phases, void* workspace,
                           int64_t workspace_bytes, float* end_score, int32_t* end_start, int32_t* hit_count,
                           w2l_kws_hit_t* hits, int32_t* status, void* stream) {
    W2L_CHECK_ARG(x && table && thr && workspace && end_score && end_start && hit_count && hits && status,
                  "ctc_kws: null pointer");
    W2L_CHECK_ARG(table->labels && table->meta && table->block_kw, "ctc_kws: a table with a null pointer in it");
    W2L_CHECK_ARG(A > 0 && blank >= 0 && blank < A, "ctc_kws: bad sizes (A=%d, blank=%d)", A, blank);
    W2L_CHECK_ARG(kws_plan(N, T, table->n_keywords, max_hits),
                  "ctc_kws: N=%d (max 65535), T=%d (max 32768), %d keywords (max 4096) or max_hits=%d (1..64) out of range", N, T,
                  table->n_keywords, max_hits);
    const int W = table->width;
    W2L_CHECK_ARG(W == 64 || W == 128 || W == 256 || W == 512 || W == 1024, "ctc_kws: block width %d is not one of 64..1024", W);
    W2L_CHECK_ARG(table->n_blocks >= 1 && table->n_blocks <= table->n_keywords, "ctc_kws: %d blocks for %d keywords",
                  table->n_blocks, table->n_keywords);
    W2L_CHECK_ARG(phases >= 1 && phases <= 7, "ctc_kws: phases=%d is no mask of 1 (frame maximum), 2 (scan), 4 (pick)", phases);
    const int64_t need = w2l_ctc_kws_workspace_bytes(N, T, table->n_keywords, max_hits);
    W2L_CHECK_ARG(workspace_bytes >= need, "ctc_kws: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)need);
    KwsParams p;
    p.x = x; p.in_len = input_lengths; p.labels = table->labels; p.meta = table->meta; p.block_kw = table->block_kw; p.thr = thr;
    p.N = N; p.T = T; p.A = A; p.K = table->n_keywords; p.blank = blank; p.is_prob = !log_probs; p.n_blocks = table->n_blocks;
    p.max_hits = max_hits;
    p.bmax = (float*)workspace; p.frame_bad = (int32_t*)(p.bmax + (int64_t)N * T); p.end_score = end_score; p.end_start = end_start; p.hit_count = hit_count; p.hits = hits;
    p.status = status;
    hipStream_t s = (hipStream_t)stream;
    if (phases & 1) {
        hipLaunchKernelGGL(kws_frame_max_kernel, dim3(N), dim3(256), 0, s, p);
        W2L_CHECK_LAUNCH();
    }
    if (phases & 2) {
        const dim3 grid(table->n_blocks, N);
        switch (W) {
            case 64: hipLaunchKernelGGL(kws_scan_kernel<64>, grid, dim3(64), 0, s, p); break;
            case 128: hipLaunchKernelGGL(kws_scan_kernel<128>, grid, dim3(128), 0, s, p); break;
            case 256: hipLaunchKernelGGL(kws_scan_kernel<256>, grid, dim3(256), 0, s, p); break;
            case 512: hipLaunchKernelGGL(kws_scan_kernel<512>, grid, dim3(512), 0, s, p); break;
            default: hipLaunchKernelGGL(kws_scan_kernel<1024>, grid, dim3(1024), 0, s, p); break;
        }
        W2L_CHECK_LAUNCH();
    }
    if (phases & 4) {
        hipLaunchKernelGGL(kws_pick_kernel, dim3(table->n_keywords, N), dim3(64), 0, s, p);
        W2L_CHECK_LAUNCH();
    }
    return 0;
}

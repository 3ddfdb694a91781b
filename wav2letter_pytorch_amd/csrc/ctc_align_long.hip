// CTC forced alignment of ONE long recording to its whole transcript (gfx950): w2l_ctc_align's definition (ctc_align.hip: the
// recurrence over the L = 2 S + 1 extended states, the tie rules, "a maximum of -inf stays -inf", is_prob, the statuses) for
// N = 1, with the trellis cut in both directions so that it neither has to fit one workgroup nor runs on one CU.
//
// Time blocks: block b holds the frames [b * tb, (b + 1) * tb) (tb a multiple of 16, so a block owns whole 16-frame move
// words); one launch per block, ordered by the stream alone -- no grid barrier, no cooperative launch, no flag anybody waits
// on.  State tiles: inside a launch workgroup i owns the sb states from i * sb.  Cell (t, s) reads (t-1, s), (t-1, s-1) and
// (t-1, s-2) only, so given the column before the block the tiles are independent: a workgroup loads that column for its own
// states and a halo of at least 2 * tb states below them, runs ctc_align_kernel's loop over the whole window (column through
// LDS, one LDS-only barrier per frame, emissions prefetched), and stores the last column and the moves of its OWN states only.
// The window's lowest cells see -inf guards in place of the states below the window and are wrong; the wrongness climbs two
// states per frame and after the block's tb frames has covered exactly the halo (DESIGN 8s has the argument).  A max is exact
// and the adds run along a path, so every owned cell carries the bits the one-workgroup kernel would give it.
//
// Kernels: init (column 0, the target and probability checks -> the status word in the workspace, which every later kernel
// reads: the host never waits between launches), fwd<SPT> (one launch per time block), back (one workgroup: per time block,
// last to first, the move words the walk can touch are loaded into LDS cooperatively and walked there), out (path, starts,
// ends, the -1 fills, score and status).  Moves keep ctc_align_kernel's packing: 2 bits per cell, 16 frames to a word per state,
// words [ceil(T / 16)][Lp] with Lp = L rounded up to a multiple of sb; all move indexing is 64-bit; states are int32.
#include "common.h"
#include "../../include/w2l_hip.h"
#include <math.h>

namespace {

constexpr float NEG_INF = -INFINITY;
constexpr int kBackThreads = 256;

struct LongParams {
    const float* x;            // [T][A] log-probabilities, or probabilities if is_prob
    const int32_t* targets;    // [S]
    int T, A, S, blank, is_prob, tb, sb, Lp;
    int32_t* stat;             // [4]: status (0 ok, 1 no path, 2 bad input), end state, score bits, -
    float* col[2];             // [Lp] each: the column a time block reads and the one it writes, swapped per block
    int32_t* st;               // [T] the walked states
    uint32_t* moves;           // [ceil(T / 16)][Lp]
    float* score;
    int32_t *status, *path, *starts, *ends;
};

struct LongPlan {
    int tb, sb, tiles, Lp, nt, spt, blocks;
    int64_t o_col, o_st, o_moves, bytes;
};

// the shapes w2l_ctc_align_long takes (w2l_hip.h states them), the default (tb, sb) (the winner of tools/bench_align_long.py,
// DESIGN 8s) and the workspace layout: status words | two columns | states | moves, every section 16-byte aligned
bool long_plan(int T, int S, int tb, int sb, LongPlan* pl) {
    if (T < 1 || T > W2L_ALIGN_LONG_MAX_T || S < 0 || S > W2L_ALIGN_LONG_MAX_S) return false;
    if ((tb == 0) != (sb == 0)) return false;
    if (tb == 0) { tb = W2L_ALIGN_LONG_TB; sb = W2L_ALIGN_LONG_SB; }
    if (tb < 16 || tb > W2L_ALIGN_LONG_MAX_TB || tb % 16 || sb < 64 || sb > W2L_ALIGN_LONG_MAX_SB || sb % 64) return false;
    const int L = 2 * S + 1;
    pl->tb = tb;
    pl->sb = sb;
    pl->tiles = (L + sb - 1) / sb;
    pl->Lp = pl->tiles * sb;
    const int window = sb + 2 * tb;                        // <= 2048 + 512
    pl->spt = window <= 1024 ? 1 : (window <= 2048 ? 2 : 4);
    pl->nt = (window + 64 * pl->spt - 1) / (64 * pl->spt) * 64;
    pl->blocks = (T + tb - 1) / tb;
    pl->o_col = 16;
    pl->o_st = pl->o_col + 2 * (int64_t)pl->Lp * 4;
    pl->o_moves = pl->o_st + ((int64_t)T * 4 + 15) / 16 * 16;
    pl->bytes = pl->o_moves + (int64_t)((T + 15) >> 4) * pl->Lp * 4;
    return true;
}

// column 0, and the checks whose failure is status 2: a target outside [0, A) or equal to the blank (never used as an index),
// a negative or NaN probability anywhere in the T frames.  stat[] was zeroed on the stream before.
__global__ __launch_bounds__(256) void ctc_align_long_init(LongParams p) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int L = 2 * p.S + 1;
    bool bad = false;
    for (int64_t s = gid; s < p.Lp; s += stride) {
        float v = NEG_INF;
        if (s < L) {
            int lab = p.blank;
            if (s & 1) {
                lab = p.targets[s >> 1];
                if (lab < 0 || lab >= p.A || lab == p.blank) { bad = true; lab = -1; }
            }
            if (s <= 1 && lab >= 0) {
                v = p.x[lab];
                if (p.is_prob) v = logf(v);
            }
        }
        p.col[0][s] = v;
    }
    if (p.is_prob) {
        const int64_t total = (int64_t)p.T * p.A;
        for (int64_t i = gid; i < total; i += stride) bad |= !(p.x[i] >= 0.f);
    }
    if (bad) p.stat[0] = 2;                                // every writer writes the same word
}

// The frames [t0, t1) of one time block (t0 >= 1: frame 0 is the init kernel's) for the tile of blockIdx.x.  blockDim.x * SPT
// cells (local cell j = tid + k * blockDim.x) end at the tile's top state: the owned states are the window's last sb cells,
// everything below them is halo (>= 2 * tb cells; cells below state 0 hold -inf and stay there).  PF as ctc_align_kernel.
template <int SPT>
__global__ __launch_bounds__(1024) void ctc_align_long_fwd(LongParams p, int t0, int t1, int flip) {
    constexpr int PF = SPT == 1 ? 8 : (SPT == 2 ? 4 : 2);
    extern __shared__ float sh_all[];                      // pad[2] | [2][Lw + 2] columns, two guard cells below each
    if (p.stat[0] != 0) return;                            // bad input, found by an earlier launch: the same for every thread
    const int NT = blockDim.x, Lw = NT * SPT, tid = threadIdx.x;
    const int L = 2 * p.S + 1;
    const int base = (int)blockIdx.x * p.sb + p.sb - Lw;   // the state of local cell 0
    const int own = Lw - p.sb;                             // the first owned local cell
    float* buf0 = sh_all + 4;
    float* buf1 = sh_all + 4 + (Lw + 2);
    const float* cin = p.col[flip];
    float* cout = p.col[flip ^ 1];
    if (tid < 2) { buf0[-2 + tid] = NEG_INF; buf1[-2 + tid] = NEG_INF; }

    int lab[SPT];
    bool skip[SPT];
    float cur[SPT], e_nxt[PF][SPT];
    uint32_t bw[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int j = tid + k * NT, s = base + j;
        lab[k] = p.blank;
        skip[k] = false;
        if (s >= 0 && s < L && (s & 1)) {
            lab[k] = p.targets[s >> 1];
            skip[k] = s >= 3 && p.targets[(s >> 1) - 1] != lab[k];
        }
        cur[k] = s >= 0 ? cin[s] : NEG_INF;                // s < Lp: the window ends at the tile's top
        buf0[j] = cur[k];
        bw[k] = 0;
    }
#pragma unroll
    for (int j = 0; j < PF; ++j) {
        const int tt = min(t0 + j, t1 - 1);
#pragma unroll
        for (int k = 0; k < SPT; ++k) e_nxt[j][k] = p.x[(int64_t)tt * p.A + lab[k]];
    }
    __syncthreads();
    float* prev = buf0;
    float* next = buf1;
    for (int tf = t0; tf < t1; tf += PF) {
        float e[PF][SPT];
#pragma unroll
        for (int j = 0; j < PF; ++j)
#pragma unroll
            for (int k = 0; k < SPT; ++k) e[j][k] = p.is_prob ? logf(e_nxt[j][k]) : e_nxt[j][k];
        if (tf + PF < t1) {
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int tt = min(tf + PF + j, t1 - 1);
#pragma unroll
                for (int k = 0; k < SPT; ++k) e_nxt[j][k] = p.x[(int64_t)tt * p.A + lab[k]];
            }
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = tf + j;
            if (t >= t1) break;
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int c = tid + k * NT;
                float best = cur[k];                                       // ties: stay, then s-1, then s-2
                uint32_t mv = 0;
                const float a1 = prev[c - 1];
                const float a2 = skip[k] ? prev[c - 2] : NEG_INF;
                if (a1 > best) { best = a1; mv = 1; }
                if (a2 > best) { best = a2; mv = 2; }
                float v = best == NEG_INF ? NEG_INF : best + e[j][k];
                if (base + c >= L) v = NEG_INF;
                cur[k] = v;
                next[c] = v;
                bw[k] |= mv << (2 * (t & 15));
            }
            if ((t & 15) == 15 || t == t1 - 1) {                           // t1 - 1: the recording's last, partial word
#pragma unroll
                for (int k = 0; k < SPT; ++k) {
                    const int c = tid + k * NT;
                    if (c >= own) p.moves[(int64_t)(t >> 4) * p.Lp + (base + c)] = bw[k];
                    bw[k] = 0;
                }
            }
            // LDS-only barrier (as ctc_align_kernel): prefetched emissions and move stores stay in flight across it
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            float* tmp = prev; prev = next; next = tmp;
        }
    }
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int c = tid + k * NT;
        if (c >= own) cout[base + c] = cur[k];
    }
}

// One workgroup.  The end state and score from the last column, then the walk, one time block at a time from the last: a block
// of n frames entered at state s reads moves of the states s - 2 (n - 1) .. s only, so the 2 tb - 1 states at and below s, in
// the block's tb / 16 words each, are loaded into LDS by all threads and thread 0 walks them there; the block's states leave
// through LDS too, as one coalesced store.
__global__ __launch_bounds__(kBackThreads) void ctc_align_long_back(LongParams p, int flip) {
    extern __shared__ uint32_t sh_back[];                  // int[4] | int st_l[tb] | uint32 win[tb / 16][2 tb - 1]
    int* sh_s = (int*)sh_back;
    int* st_l = (int*)sh_back + 4;
    uint32_t* win = sh_back + 4 + p.tb;
    const int tid = threadIdx.x, W = 2 * p.tb - 1;
    if (p.stat[0] != 0) return;
    const int L = 2 * p.S + 1;
    if (tid == 0) {                                        // end: the last label wins a tie with the blank
        const float* col = p.col[flip];
        const float a = col[L - 1];
        const float b = L > 1 ? col[L - 2] : NEG_INF;
        int s_end = L - 1;
        float sc = a;
        if (L > 1 && b >= a) { s_end = L - 2; sc = b; }
        sh_s[0] = s_end;
        sh_s[1] = sc > NEG_INF;
        p.stat[1] = s_end;
        p.stat[2] = __float_as_int(sc);
        if (!(sc > NEG_INF)) p.stat[0] = 1;
    }
    __syncthreads();
    if (!sh_s[1]) return;
    for (int b = (p.T - 1) / p.tb; b >= 0; --b) {
        const int t_lo = max(b * p.tb, 1), t_hi = min((b + 1) * p.tb, p.T) - 1;
        if (t_lo > t_hi) continue;                         // T == 1
        const int c0 = (b * p.tb) >> 4, nc = (t_hi >> 4) - c0 + 1;
        const int s_top = sh_s[0], wbase = s_top - (W - 1);
        for (int i = tid; i < nc * W; i += kBackThreads) {
            const int c = i / W, s = wbase + (i - c * W);
            win[i] = s >= 0 ? p.moves[(int64_t)(c0 + c) * p.Lp + s] : 0u;
        }
        __syncthreads();
        if (tid == 0) {
            int s = s_top;
            for (int t = t_hi; t >= t_lo; --t) {
                st_l[t - b * p.tb] = s;
                s -= (int)min((win[((t >> 4) - c0) * W + (s - wbase)] >> (2 * (t & 15))) & 3u, 2u);     // (3 is never stored)
                s = max(s, 0);                             // never taken on moves the forward pass wrote: keeps what the
            }                                              // output kernel indexes by st[] in range whatever the workspace holds
            sh_s[0] = s;
        }
        __syncthreads();
        for (int t = t_lo + tid; t <= t_hi; t += kBackThreads) p.st[t] = st_l[t - b * p.tb];
    }
    if (tid == 0) p.st[0] = sh_s[0];
}

// labels of the walked states, first / last frame of each token's own state; -1 everywhere unless status 0
__global__ __launch_bounds__(256) void ctc_align_long_out(LongParams p) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int status = p.stat[0];
    const bool ok = status == 0;
    for (int64_t t = gid; t < p.T; t += stride) {
        int label = -1;
        if (ok) {
            const int s = p.st[t];
            label = p.blank;
            if (s & 1) {
                label = p.targets[s >> 1];
                if (t == 0 || p.st[t - 1] != s) p.starts[s >> 1] = (int)t;
                if (t == p.T - 1 || p.st[t + 1] != s) p.ends[s >> 1] = (int)t;
            }
        }
        p.path[t] = label;
    }
    if (!ok)
        for (int64_t j = gid; j < p.S; j += stride) { p.starts[j] = -1; p.ends[j] = -1; }
    if (gid == 0) {
        *p.score = ok ? __int_as_float(p.stat[2]) : NEG_INF;
        *p.status = status;
    }
}

}  // namespace

extern "C" int64_t w2l_ctc_align_long_workspace_bytes(int T, int S, int tb, int sb) {
    LongPlan pl;
    return long_plan(T, S, tb, sb, &pl) ? pl.bytes : -1;
}

extern "C" int w2l_ctc_align_long_phases(const float* x, int T, int A, const int32_t* targets, int S, int blank, int log_probs,
                                         int tb, int sb, int phases, void* workspace, int64_t workspace_bytes, float* score,
                                         int32_t* status, int32_t* path, int32_t* starts, int32_t* ends, void* stream) {
    W2L_CHECK_ARG(x && score && status && path && workspace, "ctc_align_long: null pointer");
    W2L_CHECK_ARG(S == 0 || (targets && starts && ends), "ctc_align_long: null targets / starts / ends");
    W2L_CHECK_ARG(A > 0 && blank >= 0 && blank < A, "ctc_align_long: bad sizes");
    LongPlan pl;
    W2L_CHECK_ARG(long_plan(T, S, tb, sb, &pl),
                  "ctc_align_long: T=%d (1..%d), target length %d (max %d) or plan (tb=%d, sb=%d) out of range", T,
                  W2L_ALIGN_LONG_MAX_T, S, W2L_ALIGN_LONG_MAX_S, tb, sb);
    W2L_CHECK_ARG(workspace_bytes >= pl.bytes, "ctc_align_long: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)pl.bytes);
    W2L_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ctc_align_long: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    LongParams p;
    p.x = x; p.targets = targets; p.T = T; p.A = A; p.S = S; p.blank = blank; p.is_prob = !log_probs;
    p.tb = pl.tb; p.sb = pl.sb; p.Lp = pl.Lp;
    p.stat = (int32_t*)ws;
    p.col[0] = (float*)(ws + pl.o_col);
    p.col[1] = p.col[0] + pl.Lp;
    p.st = (int32_t*)(ws + pl.o_st);
    p.moves = (uint32_t*)(ws + pl.o_moves);
    p.score = score; p.status = status; p.path = path; p.starts = starts; p.ends = ends;

    W2L_CHECK_ARG(phases >= 1 && phases <= 7, "ctc_align_long: phases=%d outside 1..7", phases);
    int flip = 0;                                          // the column the last time block wrote
    for (int b = 0; b < pl.blocks; ++b) flip ^= (b == 0 ? 1 : b * pl.tb) < T;
    if (phases & 1) {
        W2L_CHECK_HIP(hipMemsetAsync(p.stat, 0, 16, st));
        const int64_t init_work = p.is_prob ? (int64_t)T * A : 0;
        const int64_t init_blocks = ((init_work > pl.Lp ? init_work : pl.Lp) + 255) / 256;
        hipLaunchKernelGGL(ctc_align_long_init, dim3((unsigned)(init_blocks < 2048 ? init_blocks : 2048)), dim3(256), 0, st, p);
        W2L_CHECK_LAUNCH();
        const size_t lds = (4 + 2 * ((size_t)pl.nt * pl.spt + 2)) * sizeof(float);
        int in = 0;
        for (int b = 0; b < pl.blocks; ++b) {
            const int t0 = b == 0 ? 1 : b * pl.tb, t1 = (b + 1) * pl.tb < T ? (b + 1) * pl.tb : T;
            if (t0 >= t1) continue;                        // T == 1
            if (pl.spt == 1) hipLaunchKernelGGL(ctc_align_long_fwd<1>, dim3(pl.tiles), dim3(pl.nt), lds, st, p, t0, t1, in);
            else if (pl.spt == 2) hipLaunchKernelGGL(ctc_align_long_fwd<2>, dim3(pl.tiles), dim3(pl.nt), lds, st, p, t0, t1, in);
            else hipLaunchKernelGGL(ctc_align_long_fwd<4>, dim3(pl.tiles), dim3(pl.nt), lds, st, p, t0, t1, in);
            in ^= 1;
        }
        W2L_CHECK_LAUNCH();
    }
    if (phases & 2) {
        const size_t lds_back = (4 + (size_t)pl.tb + (size_t)(pl.tb / 16) * (2 * pl.tb - 1)) * sizeof(uint32_t);
        hipLaunchKernelGGL(ctc_align_long_back, dim3(1), dim3(kBackThreads), lds_back, st, p, flip);
        W2L_CHECK_LAUNCH();
    }
    if (phases & 4) {
        const int64_t out_blocks = ((T > S ? T : S) + 255) / 256;
        hipLaunchKernelGGL(ctc_align_long_out, dim3((unsigned)(out_blocks < 2048 ? out_blocks : 2048)), dim3(256), 0, st, p);
        W2L_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int w2l_ctc_align_long(const float* x, int T, int A, const int32_t* targets, int S, int blank, int log_probs, int tb,
                                  int sb, void* workspace, int64_t workspace_bytes, float* score, int32_t* status, int32_t* path,
                                  int32_t* starts, int32_t* ends, void* stream) {
    return w2l_ctc_align_long_phases(x, T, A, targets, S, blank, log_probs, tb, sb, 7, workspace, workspace_bytes, score, status,
                                     path, starts, ends, stream);
}

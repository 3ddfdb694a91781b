// Edit distance on the device (gfx950), and what stands on it: minimum-Bayes-risk selection over a beam search's n-best list
// (mbr.py has the definitions; host models: tests/mbr_refs.edit_ops, mbr.mbr_select_host).  No reference counterpart.
//
// The recurrence (reference a[0..na), hypothesis b[0..nb)): D[0][0] = 0, D[i][0] = i deletions, D[0][j] = j insertions; for
// i, j >= 1 the candidates in this order -- diagonal D[i-1][j-1] (+ one substitution if a[i-1] != b[j-1]), deletion
// D[i-1][j] + 1, insertion D[i][j-1] + 1 -- and the cell takes the FIRST candidate of the smallest distance, with its counts.
// ins - del = j - i and sub = d - del - ins hold at every cell, so a cell is (d, del), here one 32-bit word d << 16 | del
// (both <= 4095); a candidate is one add, the choice two compares on the upper half.
//
// ed_core: one wavefront per pair.  The columns are cut into tiles of 64, one column per lane; inside a tile the wave sweeps
// the anti-diagonals: at step s lane l computes row i = s - l of its column.  What a cell needs is in registers -- the cell
// above (the lane's own previous result), the cell to the left (lane l-1's previous result: one __shfl_up per step) and the
// diagonal (the left cell of the step before) -- except at the tile's left edge: the last column of the tile before, na + 1
// words in LDS, which lane 63 overwrites in place 63 steps after lane 0 has read the same row.  The reference tokens sit in
// LDS too (lanes read consecutive words).  So a pair holds 2 (na + 1) words of LDS and no matrix anywhere; a tile costs
// na + 63 steps, a pair ceil(nb / 64) (na + 63) -- the skew wastes 63 steps a tile, which is why the wave takes the columns
// 64 at a time and not all at once with several per lane.  No atomics, no waits, nothing shared between workgroups.
//
// Token equality is a functor: plain keys (w2l_edit_distance, and the char unit of MBR) compare the 32-bit keys alone; the word
// unit of MBR keys a word by a hash and, on equal hashes, compares length and labels -- the hash is only a filter (it is
// h = h * 17 + label, which collides readily: CAT and CBC over the English labels, (4*17 + 2)*17 + 21 = (4*17 + 3)*17 + 4).
//
// w2l_nbest_mbr, three launches behind the search on its stream, reading its out buffer where it lies:
//   mbr_tokenise_kernel   one wave per (utterance, rank): ASG repeat decoding (decode_repeats: a repeat label becomes the decoded
//                         label before it, leading ones are dropped), each label replaced by the first index of its character,
//                         then the tokens -- char: the labels that are not ' '; word: the maximal runs of non-whitespace, each
//                         with start, length and hash -- compacted with ballots, 64 positions a round
//   mbr_dist_kernel       one wave per (utterance, pair i < j of ranks): ed_core, both halves of dist[n][.][.]
//   mbr_risk_kernel       one workgroup per utterance, thread i = rank i: posterior, risk (float64, j = 0..k-1 in order), the
//                         pick, the copy of the picked row
// Every length these kernels read from device memory is compared with its limit before it bounds a loop or an LDS index.
#include "common.h"
#include "../../include/w2l_hip.h"

namespace {

constexpr int ED_MAX_LEN = 4095;           // tokens per sequence (w2l_ctc_align's target limit); d and del fit 16 bits each
constexpr int ED_MAX_GRID = 4096;          // workgroups of w2l_edit_distance: more pairs than that go round the grid
constexpr int MBR_MAX_K = 64, MBR_MAX_T = 32768, MBR_MAX_N = 65535, MBR_MAX_A = 128;
constexpr int MBR_EMPTY = -1, MBR_BAD = -2;        // ntok of an empty slot / of a row outside the limits
constexpr int CLS_ID = 0xFF, CLS_SPACE = 0x100, CLS_WS = 0x200;   // label class: first index of the character | ' ' | whitespace

__device__ __forceinline__ uint32_t ed_pack(int d, int del) { return (uint32_t)d << 16 | (uint32_t)del; }

struct KeyEq {                              // equal keys are equal tokens
    __device__ __forceinline__ bool operator()(int, int) const { return true; }
};

// D[na][nb] as d << 16 | del, the same in every lane.  a_g / b_g: the 32-bit keys of the two sequences; eq(i, j): called where
// a_g[i] == b_g[j], says whether the tokens are equal.  sh_a: na words, sh_bnd: na + 1 words of LDS.  0 <= na, nb <= ED_MAX_LEN
// is the caller's to check.  Called by all 64 lanes of a one-wave workgroup.
template <class Eq>
__device__ uint32_t ed_core(const int32_t* __restrict__ a_g, int na, const int32_t* __restrict__ b_g, int nb, int32_t* sh_a,
                            uint32_t* sh_bnd, Eq eq) {
    const int lane = threadIdx.x;
    if (na == 0) return ed_pack(nb, 0);
    if (nb == 0) return ed_pack(na, na);
    for (int i = lane; i < na; i += 64) sh_a[i] = a_g[i];
    for (int i = lane; i <= na; i += 64) sh_bnd[i] = ed_pack(i, i);          // column 0: i deletions
    __syncthreads();
    uint32_t up = 0;
    for (int j0 = 0; j0 < nb; j0 += 64) {
        const int j = j0 + lane + 1;                     // this lane's column
        const bool act = j <= nb;
        const int32_t tb = act ? b_g[j - 1] : 0;
        up = ed_pack(j, 0);                              // row 0: j insertions
        uint32_t diag = ed_pack(j - 1, 0);
        const int steps = na + min(64, nb - j0) - 1;
        for (int s = 1; s <= steps; ++s) {
            const uint32_t recv = __shfl_up(up, 1);      // D[i][j-1]: what the lane to the left computed in the step before
            const int i = s - lane;
            if (act && i >= 1 && i <= na) {
                const uint32_t left = lane == 0 ? sh_bnd[i] : recv;
                const bool same = sh_a[i - 1] == tb && eq(i - 1, j - 1);
                uint32_t best = diag + (same ? 0u : 0x10000u);
                uint32_t c = up + 0x10001u;
                if ((c >> 16) < (best >> 16)) best = c;
                c = left + 0x10000u;
                if ((c >> 16) < (best >> 16)) best = c;
                diag = left;
                up = best;
                if (lane == 63) sh_bnd[i] = best;        // the next tile's left edge
            }
        }
        if (lane == 0) sh_bnd[0] = ed_pack(j0 + 64, 0);
        __syncthreads();
    }
    return __shfl(up, (nb - 1) & 63);
}

// ------------------------------------------------------------------------------------------------------- w2l_edit_distance
struct EdParams {
    const int32_t* tokens;     // [n_tokens]
    const int32_t* offsets;    // [S + 1]
    const int32_t* pairs;      // [P][2]: reference sequence, hypothesis sequence
    int64_t n_tokens;
    int S, P, max_len;
    int32_t* dist;             // [P]
    int32_t* counts;           // [P][3] or null: sub, del, ins
    int32_t* status;           // [P]
};

// the tokens of sequence q: false where the pair's index or the offsets are out of range
__device__ __forceinline__ bool ed_sequence(const EdParams& p, int q, int& lo, int& n) {
    if (q < 0 || q >= p.S) return false;
    const int64_t a = p.offsets[q], b = p.offsets[q + 1];
    if (a < 0 || b < a || b > p.n_tokens || b - a > p.max_len) return false;
    lo = (int)a;
    n = (int)(b - a);
    return true;
}

__global__ __launch_bounds__(64) void edit_distance_kernel(EdParams p) {
    extern __shared__ int32_t ed_lds[];
    int32_t* sh_a = ed_lds;
    uint32_t* sh_bnd = (uint32_t*)(ed_lds + p.max_len);
    for (int q = blockIdx.x; q < p.P; q += gridDim.x) {
        const int ra = p.pairs[2 * q], rb = p.pairs[2 * q + 1];
        int lo_a = 0, lo_b = 0, na = 0, nb = 0;
        const int st = (ra < 0 || ra >= p.S || rb < 0 || rb >= p.S) ? 2
                       : (ed_sequence(p, ra, lo_a, na) && ed_sequence(p, rb, lo_b, nb)) ? 0 : 1;
        if (st) {                                        // uniform: nothing of the pair is read
            if (threadIdx.x == 0) {
                p.dist[q] = -1;
                p.status[q] = st;
                if (p.counts) p.counts[3 * q] = p.counts[3 * q + 1] = p.counts[3 * q + 2] = -1;
            }
            continue;
        }
        const uint32_t cell = ed_core(p.tokens + lo_a, na, p.tokens + lo_b, nb, sh_a, sh_bnd, KeyEq());
        if (threadIdx.x == 0) {
            const int d = (int)(cell >> 16), del = (int)(cell & 0xFFFF), ins = del + nb - na;
            p.dist[q] = d;
            p.status[q] = 0;
            if (p.counts) {
                p.counts[3 * q] = d - del - ins;
                p.counts[3 * q + 1] = del;
                p.counts[3 * q + 2] = ins;
            }
        }
        __syncthreads();                                 // the LDS rows are the next pair's
    }
}

// ----------------------------------------------------------------------------------------------------------- w2l_nbest_mbr
struct MbrParams {
    const double* score;       // [N][k]     the search's out buffer, in place
    const int32_t* len;        // [N][k]
    const int32_t* labels;     // [N][k][T]
    int N, k, T, A, unit, repeat;
    double scale;
    int32_t* dec;              // [N][k][T]  workspace: decoded rows, every label the first index of its character
    int32_t* tok;              // [N][k][T]  token keys (char: the label; word: the hash)
    int32_t* wstart;           // [N][k][T]  word unit: where in dec the word starts
    int32_t* wlen;             // [N][k][T]  and its labels
    int32_t* ntok;             // [N][k]     tokens, MBR_EMPTY or MBR_BAD
    int32_t* pick;             // [N]        outputs
    int32_t* status;           // [N]
    double* risk;              // [N][k]
    int32_t* dist;             // [N][k][k]
    int32_t* pick_len;         // [N]
    int32_t* pick_labels;      // [N][T]
    uint16_t cls[MBR_MAX_A];   // per label: CLS_ID | CLS_SPACE | CLS_WS
};

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

__global__ __launch_bounds__(64) void mbr_tokenise_kernel(MbrParams p) {
    const int lane = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.y * p.k + blockIdx.x;
    const int len = p.len[row];
    if (len < 0 || len > p.T) {                          // an empty slot; a length the buffer cannot hold
        if (lane == 0) p.ntok[row] = len < 0 ? MBR_EMPTY : MBR_BAD;
        return;
    }
    const int32_t* e = p.labels + row * p.T;
    int32_t* dec = p.dec + row * p.T;
    // decode: position pos holds label v, or under ASG the last label before it that is no repeat label
    int lead = 0, carry = -1;
    bool bad = false;
    for (int base = 0; base < len; base += 64) {
        const int pos = base + lane;
        const bool in = pos < len;
        const int v = in ? e[pos] : 0;
        bad |= in && (v < 0 || v >= p.A);
        const bool rep = in && v == p.repeat;
        const uint64_t solid = __ballot(in && !rep);
        const uint64_t before = solid & lanes_below(lane);
        const int src = before ? 63 - __clzll((long long)before) : 0;
        const int from = __shfl(v, src);
        const int d = !rep ? v : before ? from : carry;
        if (carry < 0) {                                 // repeat labels before the first label that is none: dropped
            const int first = solid ? __ffsll((long long)solid) - 1 : 64;
            lead += min(first, len - base);
        }
        if (in && d >= 0 && d < p.A) dec[pos - lead] = p.cls[d] & CLS_ID;
        if (solid) carry = __shfl(v, 63 - __clzll((long long)solid));
    }
    if (__any(bad)) {
        if (lane == 0) p.ntok[row] = MBR_BAD;
        return;
    }
    const int dlen = len - lead;
    __syncthreads();                                     // dec is read back below, by other lanes
    int32_t* tok = p.tok + row * p.T;
    int cnt = 0;
    if (p.unit == 1) {                                   // char: what is not ' '
        for (int base = 0; base < dlen; base += 64) {
            const int q = base + lane;
            const int c = q < dlen ? dec[q] : 0;
            const bool keep = q < dlen && !(p.cls[c] & CLS_SPACE);
            const uint64_t m = __ballot(keep);
            if (keep) tok[cnt + __popcll(m & lanes_below(lane))] = c;
            cnt += __popcll(m);
        }
    } else {                                             // word: maximal runs of what is not whitespace
        int32_t* wstart = p.wstart + row * p.T;
        int32_t* wlen = p.wlen + row * p.T;
        bool prev = false;                               // was the position before this round's first one in a word?
        for (int base = 0; base < dlen; base += 64) {
            const int q = base + lane;
            const int c = q < dlen ? dec[q] : 0;
            const bool solid = q < dlen && !(p.cls[c] & CLS_WS);
            const uint64_t m = __ballot(solid);
            const bool before = lane ? (m >> (lane - 1)) & 1 : prev;
            const bool start = solid && !before;
            const uint64_t ms = __ballot(start);
            if (start) {
                uint32_t h = 0;
                int l = 0;
                for (int z = q; z < dlen; ++z, ++l) {
                    const int cz = dec[z];
                    if (p.cls[cz] & CLS_WS) break;
                    h = h * 17u + (uint32_t)cz;
                }
                const int w = cnt + __popcll(ms & lanes_below(lane));
                tok[w] = (int32_t)h;
                wstart[w] = q;
                wlen[w] = l;
            }
            cnt += __popcll(ms);
            prev = (m >> 63) & 1;
        }
    }
    if (lane == 0) p.ntok[row] = cnt > ED_MAX_LEN ? MBR_BAD : cnt;
}

struct WordEq {                             // two words of equal hash: the same length and the same labels?
    const int32_t *dec_a, *start_a, *len_a, *dec_b, *start_b, *len_b;
    int T;
    __device__ bool operator()(int i, int j) const {
        const int l = len_a[i], sa = start_a[i], sb = start_b[j];
        if (l != len_b[j]) return false;
        if (l < 0 || sa < 0 || sb < 0 || sa + (int64_t)l > T || sb + (int64_t)l > T) return false;
        for (int z = 0; z < l; ++z)
            if (dec_a[sa + z] != dec_b[sb + z]) return false;
        return true;
    }
};

__global__ __launch_bounds__(64) void mbr_dist_kernel(MbrParams p, int max_len) {
    extern __shared__ int32_t ed_lds[];
    const int n = blockIdx.y;
    int i = 0, rem = blockIdx.x;                         // the pair (i, j), i < j, of this workgroup
    while (rem >= p.k - 1 - i) {
        rem -= p.k - 1 - i;
        ++i;
    }
    const int j = i + 1 + rem;
    const int64_t ra = (int64_t)n * p.k + i, rb = (int64_t)n * p.k + j;
    const int na = p.ntok[ra], nb = p.ntok[rb];
    int d = -1;
    if (na >= 0 && nb >= 0 && na <= max_len && nb <= max_len) {
        uint32_t* sh_bnd = (uint32_t*)(ed_lds + max_len);
        const int32_t *ta = p.tok + ra * p.T, *tb = p.tok + rb * p.T;
        uint32_t cell;
        if (p.unit == 1)
            cell = ed_core(ta, na, tb, nb, ed_lds, sh_bnd, KeyEq());
        else
            cell = ed_core(ta, na, tb, nb, ed_lds, sh_bnd,
                           WordEq{p.dec + ra * p.T, p.wstart + ra * p.T, p.wlen + ra * p.T, p.dec + rb * p.T,
                                  p.wstart + rb * p.T, p.wlen + rb * p.T, p.T});
        d = (int)(cell >> 16);
    }
    if (threadIdx.x == 0) {
        int32_t* dist = p.dist + (int64_t)n * p.k * p.k;
        dist[i * p.k + j] = d;
        dist[j * p.k + i] = d;
    }
}

__global__ __launch_bounds__(64) void mbr_risk_kernel(MbrParams p) {
    __shared__ double sh_e[MBR_MAX_K], sh_risk[MBR_MAX_K];
    __shared__ int sh_nt[MBR_MAX_K], sh_pick;
    const int n = blockIdx.x, i = threadIdx.x, k = p.k;
    const int64_t row0 = (int64_t)n * k;
    const int nt = i < k ? p.ntok[row0 + i] : MBR_EMPTY;
    const bool bad = __any(nt == MBR_BAD);
    const double nan = __builtin_nan("");
    int32_t* dist = p.dist + row0 * k;
    sh_nt[i] = nt;
    __syncthreads();
    double m = -INFINITY;                                // the greatest weight of a present row
    for (int j = 0; j < k; ++j)
        if (sh_nt[j] >= 0) m = fmax(m, p.score[row0 + j]);
    sh_e[i] = nt >= 0 ? exp(p.scale * (p.score[row0 + i] - m)) : 0.0;
    __syncthreads();
    if (i < k) {
        double risk = nan;
        if (bad) {
            for (int j = 0; j < k; ++j) dist[i * k + j] = -1;
        } else {
            dist[i * k + i] = nt >= 0 ? 0 : -1;
            if (nt >= 0) {
                double sum = 0.0;
                for (int j = 0; j < k; ++j)
                    if (sh_nt[j] >= 0) sum += sh_e[j];
                risk = 0.0;
                for (int j = 0; j < k; ++j)
                    if (sh_nt[j] >= 0) risk += sh_e[j] / sum * (double)(j == i ? 0 : dist[i * k + j]);
            }
        }
        p.risk[row0 + i] = risk;
        sh_risk[i] = risk;
    }
    __syncthreads();
    if (i == 0) {
        int best = -1;
        if (!bad)
            for (int j = 0; j < k; ++j)
                if (sh_nt[j] >= 0 && (best < 0 || sh_risk[j] < sh_risk[best])) best = j;      // a tie stays with the lower rank
        sh_pick = max(best, 0);
        p.pick[n] = sh_pick;
        p.status[n] = bad ? 1 : 0;
        p.pick_len[n] = p.len[row0 + sh_pick];
    }
    __syncthreads();
    const int32_t* src = p.labels + (row0 + sh_pick) * p.T;
    for (int t = i; t < p.T; t += 64) p.pick_labels[(int64_t)n * p.T + t] = src[t];
}

bool mbr_plan(int N, int k, int T) { return N >= 1 && N <= MBR_MAX_N && k >= 1 && k <= MBR_MAX_K && T >= 1 && T <= MBR_MAX_T; }

}  // namespace

extern "C" int64_t w2l_edit_distance_workspace_bytes(int64_t n_tokens, int S, int P, int max_len) {
    if (n_tokens < 0 || n_tokens > INT32_MAX || S < 1 || P < 1 || max_len < 0 || max_len > ED_MAX_LEN) return -1;
    return 0;                                            // a pair's two rows live in LDS
}

extern "C" int w2l_edit_distance(const int32_t* tokens, int64_t n_tokens, const int32_t* offsets, int S, const int32_t* pairs,
                                 int P, int max_len, void* workspace, int64_t workspace_bytes, int32_t* dist, int32_t* counts,
                                 int32_t* status, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    W2L_CHECK_ARG((tokens || n_tokens == 0) && offsets && pairs && dist && status, "edit_distance: null pointer");
    W2L_CHECK_ARG(w2l_edit_distance_workspace_bytes(n_tokens, S, P, max_len) >= 0,
                  "edit_distance: %lld tokens (max 2^31 - 1), S=%d, P=%d (at least 1 each) or max_len=%d (max %d) out of range",
                  (long long)n_tokens, S, P, max_len, ED_MAX_LEN);
    EdParams p;
    p.tokens = tokens; p.offsets = offsets; p.pairs = pairs; p.n_tokens = n_tokens; p.S = S; p.P = P; p.max_len = max_len;
    p.dist = dist; p.counts = counts; p.status = status;
    const size_t lds = (size_t)(2 * max_len + 1) * sizeof(int32_t);
    hipLaunchKernelGGL(edit_distance_kernel, dim3(P < ED_MAX_GRID ? P : ED_MAX_GRID), dim3(64), lds, (hipStream_t)stream, p);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t w2l_nbest_mbr_workspace_bytes(int N, int k, int T) {
    if (!mbr_plan(N, k, T)) return -1;
    return ((int64_t)N * k * T * 4 + (int64_t)N * k) * (int64_t)sizeof(int32_t);
}

extern "C" int w2l_nbest_mbr(const void* search_out, int N, int k, int T, const int32_t* label_class_host, int A, int unit,
                             int repeat_index, double scale, void* workspace, int64_t workspace_bytes, void* mbr_out,
                             void* stream) {
    W2L_CHECK_ARG(search_out && label_class_host && workspace && mbr_out, "nbest_mbr: null pointer");
    W2L_CHECK_ARG(mbr_plan(N, k, T), "nbest_mbr: N=%d (max %d), k=%d (1..%d) or T=%d (max %d) out of range", N, MBR_MAX_N, k,
                  MBR_MAX_K, T, MBR_MAX_T);
    W2L_CHECK_ARG(A >= 1 && A <= MBR_MAX_A && repeat_index >= -1 && repeat_index < A,
                  "nbest_mbr: %d labels (1..%d) or repeat_index=%d out of range", A, MBR_MAX_A, repeat_index);
    W2L_CHECK_ARG(unit == 0 || unit == 1, "nbest_mbr: unit=%d is neither 0 (word) nor 1 (char)", unit);
    W2L_CHECK_ARG(scale >= 0.0 && scale < INFINITY, "nbest_mbr: scale=%g is not a finite number >= 0", scale);
    W2L_CHECK_ARG(((uintptr_t)search_out & 7) == 0 && ((uintptr_t)mbr_out & 7) == 0,
                  "nbest_mbr: the search's buffer and the MBR section must be 8-byte aligned");
    const int64_t need = w2l_nbest_mbr_workspace_bytes(N, k, T);
    W2L_CHECK_ARG(workspace_bytes >= need, "nbest_mbr: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)need);
    MbrParams p;
    const int64_t nk = (int64_t)N * k, nkt = nk * T;
    p.score = (const double*)search_out;
    p.len = (const int32_t*)((const char*)search_out + 8 * nk);
    p.labels = p.len + nk + N;
    p.N = N; p.k = k; p.T = T; p.A = A; p.unit = unit; p.repeat = repeat_index; p.scale = scale;
    p.dec = (int32_t*)workspace; p.tok = p.dec + nkt; p.wstart = p.tok + nkt; p.wlen = p.wstart + nkt; p.ntok = p.wlen + nkt;
    p.pick = (int32_t*)mbr_out; p.status = p.pick + N; p.risk = (double*)(p.status + N); p.dist = (int32_t*)(p.risk + nk);
    p.pick_len = p.dist + nk * k; p.pick_labels = p.pick_len + N;
    for (int a = 0; a < MBR_MAX_A; ++a) p.cls[a] = 0;
    for (int a = 0; a < A; ++a) {
        const int32_t c = label_class_host[a];
        W2L_CHECK_ARG((c & CLS_ID) < A && !(c & ~(CLS_ID | CLS_SPACE | CLS_WS)), "nbest_mbr: label %d has class %d", a, c);
        p.cls[a] = (uint16_t)c;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mbr_tokenise_kernel, dim3(k, N), dim3(64), 0, s, p);
    W2L_CHECK_LAUNCH();
    if (k > 1) {
        const int max_len = T < ED_MAX_LEN ? T : ED_MAX_LEN;
        hipLaunchKernelGGL(mbr_dist_kernel, dim3(k * (k - 1) / 2, N), dim3(64), (size_t)(2 * max_len + 1) * sizeof(int32_t), s, p,
                           max_len);
        W2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mbr_risk_kernel, dim3(N), dim3(64), 0, s, p);
    W2L_CHECK_LAUNCH();
    return 0;
}

// Decoding an ASG model beyond Viterbi (gfx950): the prefix beam search over emissions plus learned transitions, with an
// optional word n-gram model, lexicon and hotword list (w2l_asg_beam_search_tables, which launches
// asg_beam_search_kernel<lm != NULL, lexicon != NULL, hotwords != NULL>, and w2l_asg_beam_search, the same call without the two
// word lists; host restatement: asg_beam.asg_prefix_beam_search; what it shares with the CTC search -- workspace, output
// stage, argument checks, the trie steps of the word tables -- is beam_core.h's and beam_lm.h's),
// and the forced alignment of a given label sequence (w2l_asg_align; host: asg_beam.asg_viterbi_align_host).
//
// ---- the search.  ASG has no blank: a hypothesis is an ENCODED label sequence e_1 .. e_m (no two neighbours equal, the
// repeat label r standing for "the previous letter again"), and it carries ONE mass per frame, the log-sum over the frame
// paths that read it (consecutive equal frames merge):
//   M_0((c)) = x[0][c]
//   M_t(e)   = lae( M_{t-1}(e) + g[l][l] + x[t][l],  M_{t-1}(e minus its last label) + g[l'][l] + x[t][l] ),   l = last(e)
// restricted to the k best hypotheses of every frame, plus -- as the CTC search keeps it -- the previous mass of an extension
// that was a candidate one frame earlier and fell off the beam.  Structure and identity of a hypothesis are those of
// ctc_beam_search_kernel (beam_search.hip): one workgroup per utterance, trie nodes interned by the exact key (parent, label),
// candidate entries E(i, c) (member of slot i extended by label c) and S(i) (a member whose parent is not in the beam),
// frame phases P1 (slot bookkeeping, the frame's labels), P2 (one thread per entry: its mass in the host's order of
// contributions, rank key, first-insertion key), P3 (rank by counting, the k first are interned as the next beam).
// What differs: one mass per entry; the transitions in LDS (fp32, A <= 64); label c takes part in a frame if x[t][c] >
// log(prune) or it is the frame's first argmax, so the beam never empties; there is no end character; the text that counts
// words and feeds the LM is the DECODED one, so every trie node carries its last decoded character, its word count and (LM)
// a state that spells the decoded character (an r after a letter spells the letter again; a leading r spells nothing).
// mem[] / redir[] are bytes (slot + 1) that the lane which set one clears a frame later, so that k = 64 with A = 64 fits LDS.
//
// With a lexicon (LEX) and with hotwords (HOT) every beam slot carries what the CTC kernel's carries (lex_trie: the lexicon's
// trie node of its partial word; hot_st: the hotword walk of its string; static LDS, nothing per interned node), stepped by
// the DECODED character an extension spells: slot i extended by label c spells d = (c == r ? dec[i] : c).  d < 0 (a leading
// r) spells nothing: the states are the parent's and the extension is legal.  Otherwise the states step with d's canonical
// label; the only separator is the space (an r after a space spells a second space, legal as doubled spaces are).  P2: the
// extension entry of a non-member must stay in the lexicon to get mass (last frame's mass of a string that fell off the beam
// included), and the rank key gains gamma * h; P3: a carried member copies its slot's states, a new member repeats its
// parent slot's step; output: with complete_only the members whose partial word is empty or a whole word, in rank order (all
// members if there is none).
// The participation rule under a lexicon.  "x[t][c] > log(prune) or c is the frame's first argmax" keeps the beam alive only
// because every participating label can extend; with a lexicon every participating extension can be illegal while no member's
// last label takes part.  So with LEX -- and only then -- label c also takes part in frame t if t == 0 (every label: a
// non-empty lexicon has a legal first label) or c is the last label of a member of the current beam (every member can stay).
// It is still one ascending set per frame, for stays and extensions alike.
//
// ---- the alignment: Viterbi form of Z_tgt over the S states of the encoded target, fp32, in the structure of
// ctc_align_kernel (one lane per state, columns through LDS, moves packed over time, back-trace by wave 0) with ASG's
// recurrence: transitions added on the way, a tie stays, one state per encoded label.  The params struct, plan, workspace
// query and launcher are align_core.h's, shared with w2l_ctc_align.
#include "align_core.h"
#include "beam_core.h"

namespace {

constexpr int AB_THREADS = 256;
constexpr int AB_KMAX = 64;          // beam slots live in one wave (P1)
constexpr int AB_AMAX = 64;          // one label per lane of the frame-loading wave
constexpr int AB_NOSEQ = 0x7fff;

struct AsgLabelInfo {
    // bits 0-7: canonical (first) index of the label's character; 9: a word character (\w); 10: a word separator ([\s|>])
    int32_t v[AB_AMAX];
};

struct AsgBeam {                      // one frame's beam, slot-indexed (chr: last label, dec: last decoded label, -1 none)
    int node[AB_KMAX], parent[AB_KMAX], chr[AB_KMAX], dec[AB_KMAX], words[AB_KMAX], len[AB_KMAX], ps[AB_KMAX],
        prevslot[AB_KMAX];
    double mass[AB_KMAX], score[AB_KMAX];
};

// nd_info of a trie node: bits 0-7 last decoded label + 1 (0: none), from bit 8 the word count
__device__ __forceinline__ int pack_info(int dec, int words) { return (dec + 1) | (words << 8); }

template <bool LM, bool LEX, bool HOT>
__global__ __launch_bounds__(AB_THREADS) void asg_beam_search_kernel(
    const float* __restrict__ x, const float* __restrict__ trans, const int32_t* __restrict__ sizes, int T, int A,
    AsgLabelInfo info, int rep, int k, double beta, double prune, char* __restrict__ ws, int64_t ws_per_utt, int hash_cap,
    double* __restrict__ out_score, int32_t* __restrict__ out_len, int32_t* __restrict__ out_status,
    int32_t* __restrict__ out_labels, LmArgs lmargs, float* __restrict__ out_lm, LexArgs lex, HotArgs hot) {
    __shared__ AsgBeam beams[2];
    __shared__ double lm_w[2][LM ? AB_KMAX : 1];          // LM weight (natural log) of each beam slot
    __shared__ int lm_on[2][LM ? AB_KMAX : 1];             // ... and whether it applies (a non-space character)
    __shared__ int lex_trie[2][LEX ? AB_KMAX : 1];        // lexicon trie node of each beam slot's partial word
    __shared__ HotState hot_st[2][HOT ? AB_KMAX : 1];     // hotword walk of each beam slot's string
    __shared__ double xd[AB_AMAX];
    __shared__ int act[AB_AMAX], lab[AB_AMAX];
    __shared__ int s_m[2], s_count, s_bad;
    extern __shared__ __attribute__((aligned(16))) double dyn[];

    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nE = k * A + k;                              // E(i, c) = i*A + c, S(i) = k*A + i
    double* mass = dyn;                                    // [2 frames][nE]
    double* lsc = mass + 2 * nE;                           // live candidates: rank score
    uint32_t* lpk = (uint32_t*)(lsc + nE);                 //                  first-insertion key << 16 | entry index
    float* gl = (float*)(lpk + nE);                        // [A][A] transitions
    uint8_t* mem = (uint8_t*)(gl + A * A);                 // [k][A] 1 + slot of the member that is E(i, c)
    uint8_t* redir = mem + k * A;                          // [k][A] 1 + previous slot whose S entry is E(i, c)

    const TrieWs w = carve_ws<3>(ws, n, ws_per_utt, T, k, hash_cap, lmargs.state_off);
    int32_t* nd_parent = w.nd_parent;
    int32_t* nd_chr = w.nd_chr;
    int32_t* nd_info = w.nd_info;
    NodeLM* nd_lm = w.nd_lm;                               // LM only

    bool bad_g = false;
    for (int i = tid; i < hash_cap; i += AB_THREADS) w.hkeys[i] = BS_EMPTY;
    for (int i = tid; i < 2 * k * A; i += AB_THREADS) mem[i] = 0;         // mem and redir
    for (int i = tid; i < A * A; i += AB_THREADS) {
        const float v = trans[i];
        gl[i] = v;
        bad_g |= v != v;
    }
    for (int i = tid; i < A; i += AB_THREADS) { lab[i] = info.v[i]; act[i] = 0; }
    if (tid == 0) {
        nd_parent[0] = -1;
        nd_chr[0] = -1;
        nd_info[0] = pack_info(-1, 0);
        AsgBeam& b0 = beams[0];                            // the root: extended by frame 0, never a hypothesis itself
        b0.node[0] = 0; b0.parent[0] = -1; b0.chr[0] = -1; b0.dec[0] = -1; b0.words[0] = 0; b0.len[0] = 0;
        b0.prevslot[0] = -1; b0.mass[0] = 0.0; b0.score[0] = 0.0;
        if constexpr (LM) {
            nd_lm[0] = lm_root(lmargs);
            lm_w[0][0] = 0.0;
            lm_on[0][0] = 0;
        }
        if constexpr (LEX) lex_trie[0][0] = 0;
        if constexpr (HOT) hot_st[0][0] = HotState{0, 0, 0};
        s_m[0] = 1;
        s_m[1] = 0;
        s_bad = 0;
    }
    int Tn = T;
    if (sizes) Tn = min(max(sizes[n], 0), T);
    const float* xn = x + (int64_t)n * T * A;
    const double log_prune = prune > 0 ? log(prune) : -INFINITY;
    float nxt = 0.f;                                       // wave 2: the frame to come, one label per lane
    if (wave == 2 && Tn > 0 && lane < A) nxt = xn[lane];
    int my_mem = -1, my_redir = -1;                        // the mem / redir byte this lane set in the previous frame
    __threadfence();
    __syncthreads();
    if (bad_g) s_bad = 1;

    int cur = 0;                                           // parity of the current beam and of this frame's masses
    for (int t = 0; t < Tn; ++t) {
        const int m = s_m[cur], mprev = s_m[cur ^ 1];
        if (m == 0) break;                                 // (uniform: read after a barrier)
        AsgBeam& B = beams[cur];
        const AsgBeam& P = beams[cur ^ 1];
        // ---------------------------------------------------------------- P1
        // mem[] / redir[] are bytes for the LDS budget, so a frame's marks are cleared one by one instead of outliving a
        // stamp.  The byte a lane clears may be the byte ANOTHER lane of the same wave sets for this frame: the clear and the
        // set are two separate masked LDS stores of one wave, which execute in program order, so the set always lands last.
        // (Only wave 0 touches mem[] and only wave 1 redir[] in P1; every other access is behind a workgroup barrier.)
        if (wave == 0) {
            if (my_mem >= 0) { mem[my_mem] = 0; my_mem = -1; }
            if (lane < m) {
                int ps = -1;
                for (int j = 0; j < m; ++j) if (B.node[j] == B.parent[lane]) { ps = j; break; }
                B.ps[lane] = ps;
                if (ps >= 0) { my_mem = ps * A + B.chr[lane]; mem[my_mem] = (uint8_t)(lane + 1); }
            }
            if (lane == 0) s_count = 0;
        } else if (wave == 1) {
            // a previous member that had its own S entry and whose parent is now in the beam: its extension entry finds
            // last frame's mass there
            if (my_redir >= 0) { redir[my_redir] = 0; my_redir = -1; }
            if (t > 0 && lane < mprev && P.ps[lane] < 0 && P.parent[lane] >= 0) {
                for (int j = 0; j < m; ++j)
                    if (B.node[j] == P.parent[lane]) {
                        my_redir = j * A + P.chr[lane];
                        redir[my_redir] = (uint8_t)(lane + 1);
                        break;
                    }
            }
        } else if (wave == 2) {
            const float v = nxt;
            if (lane < A && t + 1 < Tn) nxt = xn[(int64_t)(t + 1) * A + lane];   // the next frame's load hides behind this one
            float bv = lane < A ? v : -INFINITY;
            int bi = lane < A ? lane : 64;
            if (lane < A && v != v) s_bad = 1;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {      // the frame's first argmax
                const float ov = __shfl_xor(bv, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            [[maybe_unused]] uint64_t last = 0;            // LEX: the last labels of the beam's members, one bit per label
            if constexpr (LEX) {
                // (B.chr is stable here: wave 0 writes only ps in P1; from frame 1 on every member has a label in [0, A))
                if (t > 0 && prune > 0)
                    for (int j = 0; j < m; ++j) last |= 1ull << B.chr[j];
            }
            if (lane < A) {
                xd[lane] = (double)v;
                bool pass = prune <= 0 || (double)v > log_prune || lane == bi;
                if constexpr (LEX) pass = pass || t == 0 || ((last >> lane) & 1);   // so that the beam cannot die (file head)
                act[lane] = pass ? t + 1 : 0;
            }
        }
        __syncthreads();
        // ---------------------------------------------------------------- P2
        const double* mprev_tab = mass + (cur ^ 1) * nE;
        double* mcur = mass + cur * nE;
        for (int e = tid; e < m * A + m; e += AB_THREADS) {
            const int ent = e < m * A ? e : k * A + (e - m * A);
            double acc = -INFINITY;
            int seq = AB_NOSEQ;
            bool live = false;
            int words = 0;
            [[maybe_unused]] int hchars = 0;               // HOT: h of the entry's string
            if (e < m * A) {
                const int i = e / A, c = e - i * A;
                const int s = (int)mem[ent] - 1;
                const int l = B.chr[i];
                bool ext = act[c] == t + 1 && c != l;
                [[maybe_unused]] int canon = -1;           // LEX / HOT: the canonical label the extension spells (-1: nothing)
                if constexpr (LEX || HOT) {
                    const int d = c == rep ? B.dec[i] : c;
                    if (d >= 0) canon = lab[d] & 0xff;
                }
                if constexpr (LEX) {                       // ... and the extension stays in the lexicon
                    if (ext && s < 0 && canon >= 0) ext = lex_step(lex, lex_trie[cur][i], canon, -1) >= 0;
                }
                if (ext || s >= 0) {
                    live = true;
                    // slot i extended by c; where the extension is no member, last frame's mass of the same string joins
                    auto parent_part = [&]() {
                        if (!ext) return;
                        double v = B.mass[i] + (l >= 0 ? (double)gl[l * A + c] : 0.0) + xd[c];
                        if constexpr (LM) {                // a word closes: the member's LM weight
                            // (lm_on: the text has a non-space character, so dec >= 0; checked anyway before it indexes)
                            if ((lab[c] & 0xff) == lmargs.space && lm_on[cur][i] && B.dec[i] >= 0 &&
                                (lab[B.dec[i]] & 0xff) != lmargs.space)
                                v += lm_w[cur][i];
                        }
                        acc = lae(acc, v);
                        seq = min(seq, i * (A + 1) + 1 + c);
                        if (s < 0) {
                            int pidx = -1;
                            if (B.prevslot[i] >= 0) {
                                pidx = B.prevslot[i] * A + c;
                            } else {
                                const int rv = redir[ent];
                                if (rv) pidx = k * A + rv - 1;
                            }
                            if (pidx >= 0) acc = lae(acc, mprev_tab[pidx] + (double)gl[c * A + c] + xd[c]);
                        }
                    };
                    if (s < 0) {
                        parent_part();
                        const int pd = B.dec[i], d = c == rep ? pd : c;
                        words = B.words[i] + (d >= 0 && pd >= 0 && (lab[d] & 0x400) && (lab[pd] & 0x200));
                        if constexpr (HOT)
                            hchars = hot_chars(canon >= 0 ? hot_step(hot, hot_st[cur][i], canon, -1) : hot_st[cur][i]);
                    } else {
                        words = B.words[s];
                        if constexpr (HOT) hchars = hot_chars(hot_st[cur][s]);
                        if (i < s) parent_part();
                        if (act[c] == t + 1) {             // member s stays on its last label
                            acc = lae(acc, B.mass[s] + (double)gl[c * A + c] + xd[c]);
                            seq = min(seq, s * (A + 1));
                        }
                        if (i > s) parent_part();
                    }
                }
            } else {
                const int s = e - m * A;
                if (B.ps[s] < 0 && B.parent[s] >= 0) {     // a member whose parent is not in the beam (never the root)
                    live = true;
                    words = B.words[s];
                    if constexpr (HOT) hchars = hot_chars(hot_st[cur][s]);
                    const int l = B.chr[s];
                    if (act[l] == t + 1) {
                        acc = B.mass[s] + (double)gl[l * A + l] + xd[l];
                        seq = s * (A + 1);
                    }
                }
            }
            mcur[ent] = acc;
            if (live && acc > -INFINITY) {
                const int slot = atomicAdd(&s_count, 1);
                if constexpr (HOT) lsc[slot] = acc + beta * log((double)(words + 1)) + hot.gamma * (double)hchars;
                else lsc[slot] = acc + beta * log((double)(words + 1));
                lpk[slot] = ((uint32_t)seq << 16) | (uint32_t)ent;
            }
        }
        __syncthreads();
        // ---------------------------------------------------------------- P3
        const int M = s_count;
        AsgBeam& NB = beams[cur ^ 1];
        for (int xi = tid; xi < M; xi += AB_THREADS) {
            const double sx = lsc[xi];
            const uint32_t kx = lpk[xi] >> 16;
            int r = 0;
            for (int y = 0; y < M && r < k; ++y) {
                const double sy = lsc[y];
                r += sy > sx || (sy == sx && (lpk[y] >> 16) < kx);
            }
            if (r >= k) continue;
            const int ent = (int)(lpk[xi] & 0xffffu);
            int s, i = -1, c = -1;
            if (ent < k * A) {
                i = ent / A;
                c = ent - i * A;
                s = (int)mem[ent] - 1;
            } else {
                s = ent - k * A;
            }
            if (s >= 0) {
                NB.node[r] = B.node[s]; NB.parent[r] = B.parent[s]; NB.chr[r] = B.chr[s]; NB.dec[r] = B.dec[s];
                NB.words[r] = B.words[s]; NB.len[r] = B.len[s]; NB.prevslot[r] = s;
                if constexpr (LM) { lm_w[cur ^ 1][r] = lm_w[cur][s]; lm_on[cur ^ 1][r] = lm_on[cur][s]; }
                if constexpr (LEX) lex_trie[cur ^ 1][r] = lex_trie[cur][s];
                if constexpr (HOT) hot_st[cur ^ 1][r] = hot_st[cur][s];
            } else {
                const int par = B.node[i];
                if constexpr (LEX || HOT) {                // the step of P2 again: nothing is kept per interned node
                    const int d = c == rep ? B.dec[i] : c;
                    const int canon = d >= 0 ? lab[d] & 0xff : -1;
                    if constexpr (LEX)                     // (>= 0: P2 let it live)
                        lex_trie[cur ^ 1][r] = canon >= 0 ? lex_step(lex, lex_trie[cur][i], canon, -1) : lex_trie[cur][i];
                    if constexpr (HOT)
                        hot_st[cur ^ 1][r] = canon >= 0 ? hot_step(hot, hot_st[cur][i], canon, -1) : hot_st[cur][i];
                }
                const uint64_t key = ((uint64_t)par << 8) | (uint64_t)c;
                uint32_t h = key_hash(key) & (hash_cap - 1);
                int node = -1, dec = -1, words = 0;
                while (node < 0) {                         // probe by claiming: one round trip per slot
                    const uint64_t cur_key =
                        atomicCAS((unsigned long long*)&w.hkeys[h], (unsigned long long)BS_EMPTY, (unsigned long long)key);
                    if (cur_key == BS_EMPTY) {             // a new string: its node id is reserved by (frame, rank)
                        node = 1 + t * k + r;
                        const int pd = B.dec[i];
                        dec = c == rep ? pd : c;
                        words = B.words[i] + (dec >= 0 && pd >= 0 && (lab[dec] & 0x400) && (lab[pd] & 0x200));
                        w.hvals[h] = node;
                        nd_parent[node] = par;
                        nd_chr[node] = c;
                        nd_info[node] = pack_info(dec, words);
                        if constexpr (LM) {                // the decoded character is spelled; a leading r spells nothing
                            const NodeLM ns = dec >= 0 ? lm_extend(lmargs, nd_lm[par], lab[dec] & 0xff, -1) : nd_lm[par];
                            nd_lm[node] = ns;
                            lm_w[cur ^ 1][r] = lmargs.alpha_ln10 * (double)ns.total;
                            lm_on[cur ^ 1][r] = ns.nonspace;
                        }
                    } else if (cur_key == key) {           // interned in an earlier frame
                        node = w.hvals[h];
                        const int pk = nd_info[node];
                        dec = (pk & 0xff) - 1;
                        words = pk >> 8;
                        if constexpr (LM) {
                            lm_w[cur ^ 1][r] = lmargs.alpha_ln10 * (double)nd_lm[node].total;
                            lm_on[cur ^ 1][r] = nd_lm[node].nonspace;
                        }
                    } else {
                        h = (h + 1) & (hash_cap - 1);
                    }
                }
                NB.node[r] = node; NB.parent[r] = par; NB.chr[r] = c; NB.dec[r] = dec;
                NB.words[r] = words;
                NB.len[r] = B.len[i] + 1;
                NB.prevslot[r] = -1;
            }
            NB.mass[r] = mcur[ent];
            NB.score[r] = sx;
        }
        if (tid == 0) s_m[cur ^ 1] = min(M, k);
        __threadfence();                                   // interned nodes are read by other waves in later frames
        __syncthreads();
        cur ^= 1;
    }
    // ---------------------------------------------------------------- output: backtrack the final beam
    const int m = s_m[cur];
    const AsgBeam& B = beams[cur];
    int src = tid, mout = m;                               // slot tid of the output holds beam member src (if tid < mout)
    if constexpr (LEX) {
        // complete_only: the members whose partial word is empty or a whole word, in rank order (all of them if there is none)
        if (wave == 0 && lex.complete_only) {
            const uint64_t done = __ballot(tid < m && lex_complete(lex, lex_trie[cur][tid]));
            if (done) {
                mout = __popcll(done);
                uint64_t rest = done;                      // the tid-th set bit
                for (int j = 0; j < tid && rest; ++j) rest &= rest - 1;
                src = rest ? __ffsll((unsigned long long)rest) - 1 : 0;
            }
        }
    }
    if (tid < k)
        write_result<LM>(B, tid < mout ? src : -1, (int64_t)n * k + tid, T, w, out_score, out_len, out_labels, out_lm);
    if (tid == 0) out_status[n] = s_bad;
}

int64_t lds_bytes(int k, int A) {
    const int64_t nE = (int64_t)k * A + k;
    return nE * (2 * 8 + 8 + 4) + (int64_t)A * A * 4 + 2 * (int64_t)k * A;
}

bool search_range(int N, int T, int A, int k) {
    return N > 0 && T > 0 && T < (1 << 24) && A >= 1 && A <= AB_AMAX && k >= 1 && k <= AB_KMAX && (int64_t)k * T < (1 << 29);
}

// what the eight instantiations are launched with: the arguments checked, the tables in their device form
struct AsgSearch {
    const float* x;
    const float* transitions;
    const int32_t* sizes;
    int N, T, A, repeat_index, k;
    double beta, prune;
    AsgLabelInfo info;
    void* workspace;
    int64_t ws_per_utt;
    void* out;
    void* stream;
    LmArgs lm;
    LexArgs lex;
    HotArgs hot;
};

template <bool LM, bool LEX, bool HOT>
int launch_search(const char* name, const AsgSearch& s) {
    const int64_t lds = lds_bytes(s.k, s.A);
    if (int rc = lds_args(name, (const void*)asg_beam_search_kernel<LM, LEX, HOT>, lds, s.k, s.A)) return rc;
    const OutSections o = out_sections(s.out, s.N, s.T, s.k, LM);
    hipLaunchKernelGGL((asg_beam_search_kernel<LM, LEX, HOT>), dim3(s.N), dim3(AB_THREADS), (size_t)lds, (hipStream_t)s.stream,
                       s.x, s.transitions, s.sizes, s.T, s.A, s.info, s.repeat_index, s.k, s.beta, s.prune, (char*)s.workspace,
                       s.ws_per_utt, hash_capacity(s.T, s.k), o.score, o.len, o.status, o.labels, s.lm, o.lm, s.lex, s.hot);
    W2L_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// Nothing is kept per interned node for a lexicon or for hotwords (see the head of this file): only an LM adds to the workspace.
extern "C" int64_t w2l_asg_beam_search_workspace_bytes(int N, int T, int A, int k, int order) {
    return search_range(N, T, A, k) ? search_ws_bytes(N, T, k, order, 3) : -1;
}

extern "C" int w2l_asg_beam_search_tables(const float* x, const float* transitions, const int32_t* sizes, int N, int T, int A,
                                          const int32_t* label_info_host, int repeat_index, int space_index, int k,
                                          double alpha, double beta, double prune, const w2l_ngram_lm_t* lm, int order,
                                          const w2l_lexicon_t* lexicon, int complete_only, const w2l_lexicon_t* hotwords,
                                          double hotword_weight, void* workspace, int64_t workspace_bytes, void* out,
                                          void* stream) {
    const char* name = "asg_beam_search";
    // every check of the arguments comes before the first HIP call (launch_search)
    W2L_CHECK_ARG(x && transitions && label_info_host && workspace && out && N > 0 && T > 0, "%s: bad arguments", name);
    W2L_CHECK_ARG(A >= 1 && A <= AB_AMAX, "%s: %d labels, supported 1..%d", name, A, AB_AMAX);
    W2L_CHECK_ARG(k >= 1 && k <= AB_KMAX, "%s: beam width k=%d, supported 1..%d", name, k, AB_KMAX);
    W2L_CHECK_ARG(repeat_index >= 0 && repeat_index < A, "%s: repeat_index %d outside %d labels", name, repeat_index, A);
    W2L_CHECK_ARG((int64_t)k * T < (1 << 29) && T < (1 << 24), "%s: k*T = %lld too large", name, (long long)k * T);
    AsgSearch s{x, transitions, sizes, N, T, A, repeat_index, k, beta, prune};
    if (int rc = label_info_args(name, label_info_host, A, s.info.v, AB_AMAX)) return rc;
    if (lm || lexicon || hotwords)
        if (int rc = space_args(name, label_info_host, A, space_index)) return rc;
    if (lm)
        if (int rc = lm_args(name, space_index, alpha, lm, order, T, k, 3, &s.lm)) return rc;
    if (lexicon) {
        if (int rc = trie_args(name, "lexicon", space_index, lexicon, &s.lex)) return rc;
        s.lex.complete_only = complete_only != 0;
    }
    if (hotwords) {
        W2L_CHECK_ARG(std::isfinite(hotword_weight), "%s: the hotword weight is not finite", name);
        if (int rc = trie_args(name, "hotword", space_index, hotwords, &s.hot)) return rc;
        s.hot.gamma = hotword_weight;
    }
    const int64_t need = w2l_asg_beam_search_workspace_bytes(N, T, A, k, lm ? order : 0);
    W2L_CHECK_ARG(need > 0 && workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", name,
                  (long long)workspace_bytes, (long long)need);
    s.workspace = workspace;
    s.ws_per_utt = lm ? lm_ws_stride(T, k, 3) : ws_stride(T, k, 3);
    s.out = out;
    s.stream = stream;
    switch ((lm ? 4 : 0) | (lexicon ? 2 : 0) | (hotwords ? 1 : 0)) {          // the one dispatch: a NULL table is a false flag
        case 0: return launch_search<false, false, false>(name, s);
        case 1: return launch_search<false, false, true>(name, s);
        case 2: return launch_search<false, true, false>(name, s);
        case 3: return launch_search<false, true, true>(name, s);
        case 4: return launch_search<true, false, false>(name, s);
        case 5: return launch_search<true, false, true>(name, s);
        case 6: return launch_search<true, true, false>(name, s);
        default: return launch_search<true, true, true>(name, s);
    }
}

// the search without a lexicon and without hotwords: the symbol that predates the two tables, kept for its positional callers
extern "C" int w2l_asg_beam_search(const float* x, const float* transitions, const int32_t* sizes, int N, int T, int A,
                                   const int32_t* label_info_host, int repeat_index, int space_index, int k, double alpha,
                                   double beta, double prune, const w2l_ngram_lm_t* lm, int order, void* workspace,
                                   int64_t workspace_bytes, void* out, void* stream) {
    return w2l_asg_beam_search_tables(x, transitions, sizes, N, T, A, label_info_host, repeat_index, space_index, k, alpha, beta,
                                      prune, lm, order, nullptr, 1, nullptr, 0.0, workspace, workspace_bytes, out, stream);
}

// ============================================================================================================ alignment
namespace {

// the encoded label of position s: a row that is already encoded is read as it is; in a raw one the 2nd, 4th, ... member of a
// run of equal labels becomes `repeat` (w2l_asg_loss's rule)
__device__ __forceinline__ int encoded_label(const int32_t* tg, int s, int repeat, int encoded) {
    const int v = tg[s];
    if (encoded) return v;
    int back = 0;
    while (s - back - 1 >= 0 && tg[s - back - 1] == v) ++back;
    return (back & 1) ? repeat : v;
}

struct AsgRule {                               // what align_core.h's plan and launcher ask of a criterion
    static constexpr const char* NAME = "asg_align";
    static constexpr int GUARD = 1, MAX_SPT = 4, MAX_STATES = 4095;
    static int states(int S) { return S; }
    static size_t lds_round(size_t bytes) { return (bytes + 3) & ~(size_t)3; }
};

struct AsgAlignParams {
    const float* x;            // [N][T][A] scores
    const float* g;            // [A][A] transitions
    const int32_t* in_len;     // [N] or null (all T)
    const int32_t* targets;    // row n at targets + n * tg_stride
    const int32_t* tg_len;     // utterance n at tg_len[n * len_stride]
    int64_t tg_stride, len_stride;
    int N, T, A, Smax, repeat, encoded, bp_lds;
    uint32_t* bp_global;       // [N][chunks][Lw] when !bp_lds
    float* score;              // [N]
    int32_t* status;           // [N]
    int32_t* path;             // [N][T]
    int32_t* starts;           // [N][Smax]
    int32_t* ends;             // [N][Smax]
};

// NT threads, SPT states per thread (state s = tid + k * NT), PF = frames of emissions held ahead in registers.
template <int NT, int SPT>
__global__ __launch_bounds__(NT) void asg_align_kernel(AsgAlignParams p) {
    constexpr int PF = SPT == 1 ? 8 : (SPT == 2 ? 4 : 2);
    constexpr int Lw = NT * SPT;
    // all LDS is dynamic: int flag[2] (bad target seen, unused), float score, pad | [2][Lw + 1] columns (a guard cell below
    // state 0) | uint16 st[T] | moves (bp_lds)
    extern __shared__ float sh_all[];
    int* sh_flag = (int*)sh_all;
    float& sh_score = sh_all[2];
    float* sh = sh_all + 4;
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    const int S = min(max(p.tg_len[(int64_t)n * p.len_stride], 0), p.Smax);
    const int Tn = p.in_len ? min(max(p.in_len[n], 0), p.T) : p.T;
    const int chunks = (p.T + 15) >> 4;
    float* buf0 = sh + 1;
    float* buf1 = sh + (Lw + 1) + 1;
    uint16_t* st = (uint16_t*)(sh + 2 * (Lw + 1));
    uint32_t* bp_l = (uint32_t*)(st + ((p.T + 1) & ~1));
    uint32_t* bp_g = p.bp_global + (int64_t)n * chunks * Lw;
    const float* x = p.x + (int64_t)n * p.T * p.A;
    const int32_t* tg = p.targets + (int64_t)n * p.tg_stride;
    int32_t* path = p.path + (int64_t)n * p.T;
    int32_t* starts = p.starts + (int64_t)n * p.Smax;
    int32_t* ends = p.ends + (int64_t)n * p.Smax;

    if (tid == 0) { buf0[-1] = NEG_INF; buf1[-1] = NEG_INF; sh_flag[0] = 0; sh_flag[1] = 0; }
    __syncthreads();

    // per-state constants.  A label outside [0, A), a raw label equal to the repeat label, or two equal neighbours of an
    // encoded row are errors, and are never used as an index
    int lab[SPT];
    float g_stay[SPT], g_move[SPT];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int s = tid + k * NT;
        lab[k] = 0;
        g_stay[k] = 0.f;
        g_move[k] = 0.f;
        if (s < S) {
            const int raw = tg[s];
            if (raw < 0 || raw >= p.A || (!p.encoded && raw == p.repeat)) {
                bad = true;
            } else {
                const int v = encoded_label(tg, s, p.repeat, p.encoded);
                lab[k] = v;
                g_stay[k] = p.g[v * p.A + v];
                if (s >= 1) {
                    const int rawp = tg[s - 1];
                    if (rawp >= 0 && rawp < p.A) {
                        const int u = encoded_label(tg, s - 1, p.repeat, p.encoded);
                        if (u == v) bad = true;
                        g_move[k] = p.g[u * p.A + v];
                    }
                }
            }
        }
    }
    if (bad) sh_flag[0] = 1;
    __syncthreads();
    int status = sh_flag[0] ? 2 : ((S < 1 || S > Tn) ? 1 : 0);
    float best_score = NEG_INF;

    if (status == 0) {
        // ---- forward: column 0, then frames 1 .. Tn-1 in blocks of PF frames whose emissions were loaded a block earlier
        float cur[SPT], e_nxt[PF][SPT];
        uint32_t bw[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int s = tid + k * NT;
            const float v = s == 0 ? x[lab[k]] : NEG_INF;
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
                for (int k = 0; k < SPT; ++k) e[j][k] = e_nxt[j][k];
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
                    const float c0 = cur[k], c1 = prev[s - 1];
                    float best = c0 == NEG_INF ? NEG_INF : c0 + g_stay[k];          // a tie goes to staying
                    uint32_t mv = 0;
                    const float a1 = c1 == NEG_INF ? NEG_INF : c1 + g_move[k];
                    if (a1 > best) { best = a1; mv = 1; }
                    float v = best == NEG_INF ? NEG_INF : best + e[j][k];
                    if (s >= S) v = NEG_INF;
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
                // LDS-only barrier (as ctc_align_kernel): prefetched emissions and move stores stay in flight across it
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                float* tmp = prev; prev = next; next = tmp;
            }
        }
        if (tid == 0) sh_score = prev[S - 1];
        __syncthreads();                                                   // also drains the move stores to the workspace
        best_score = sh_score;
        if (!(best_score > NEG_INF)) status = 1;                           // (-inf, or NaN scores)
        if (status == 0 && tid < 64) {
            // ---- back-trace, wave 0, every lane the same walk (lane 0 records it).  Moves in the workspace: one coalesced
            // load of the 64 states at and below the current one per 16-frame chunk (a chunk moves down at most 16 states).
            int s = S - 1;
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
    }

    // ---- outputs: encoded labels of the walked states, first / last frame of each state, -1 elsewhere
    const bool ok = status == 0;
    for (int t = tid; t < p.T; t += NT) {
        int label = -1;
        if (ok && t < Tn) {
            const int s = st[t];
            label = encoded_label(tg, s, p.repeat, p.encoded);
            if (t == 0 || st[t - 1] != s) starts[s] = t;
            if (t == Tn - 1 || st[t + 1] != s) ends[s] = t;
        }
        path[t] = label;
    }
    for (int j = (ok ? S : 0) + tid; j < p.Smax; j += NT) { starts[j] = -1; ends[j] = -1; }
    if (tid == 0) {
        p.score[n] = ok ? best_score : NEG_INF;
        p.status[n] = status;
    }
}

struct AsgAlignKernels {
    template <int NT, int SPT>
    static auto get() { return asg_align_kernel<NT, SPT>; }
};

}  // namespace

extern "C" int64_t w2l_asg_align_workspace_bytes(int N, int T, int A, int Smax) {
    if (A < 1 || A > AB_AMAX) return -1;
    return align_workspace_bytes<AsgRule>(N, T, Smax);
}

extern "C" int w2l_asg_align(const float* x, const float* transitions, const int32_t* input_lengths, const int32_t* targets,
                             int64_t target_stride, const int32_t* target_lengths, int64_t length_stride, int N, int T, int A,
                             int Smax, int repeat_index, int encoded, void* workspace, int64_t workspace_bytes, float* score,
                             int32_t* status, int32_t* path, int32_t* starts, int32_t* ends, void* stream) {
    W2L_CHECK_ARG(x && transitions && target_lengths && score && status && path, "asg_align: null pointer");
    W2L_CHECK_ARG(Smax == 0 || (targets && starts && ends), "asg_align: null targets / starts / ends");
    W2L_CHECK_ARG(N > 0 && T > 0 && A >= 1 && A <= AB_AMAX && Smax >= 0 && repeat_index >= 0 && repeat_index < A,
                  "asg_align: bad sizes (labels 1..%d)", AB_AMAX);
    W2L_CHECK_ARG(target_stride >= Smax && length_stride >= 1, "asg_align: bad strides");
    AsgAlignParams p;
    p.x = x; p.in_len = input_lengths; p.targets = targets; p.tg_len = target_lengths;
    p.tg_stride = target_stride; p.len_stride = length_stride;
    p.N = N; p.T = T; p.A = A; p.Smax = Smax;
    p.g = transitions; p.repeat = repeat_index; p.encoded = encoded != 0;
    p.score = score; p.status = status; p.path = path; p.starts = starts; p.ends = ends;
    return align_launch<AsgRule, AsgAlignKernels>(p, workspace, workspace_bytes, stream);
}

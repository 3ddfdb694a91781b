// Batched CTC prefix beam search (decoder.py:147-267 without a language model; host restatement:
// beam_search.prefix_beam_search, whose recursion this kernel reproduces candidate for candidate).
//
// One workgroup decodes one utterance and loops over its frames.  Masses are natural logs in fp64 (a frame's
// contributions are log-added in the host's loop order), so a long utterance cannot underflow.
//
// Identity of a prefix.  Beam members are nodes of a per-utterance trie in the global workspace (parent, char),
// interned by the exact key (parent node, char) in an open-addressing table, so one string has one node.  The
// candidates of frame t are the beam members and their one-label extensions; candidate tables are indexed by beam
// slot: E(i, c) is the beam member in slot i extended by canonical label c, S(i) is the member in slot i itself.  A
// member whose parent is also in the beam is not S(i) but the E entry of its parent slot (mem[] says which), so every
// string of the frame has exactly one entry.  The previous frame's masses (needed where an extension fell off the
// beam) are found through the slot the same string's parent had one frame earlier (prevslot), or -- where that parent
// was not in the previous beam -- through redir[], which names the previous frame's S entry of the string.
//
// Per frame, three phases, each ended by a workgroup barrier:
//   P1  slot bookkeeping (parent slot, mem[], redir[]) and the frame's labels: log-probs, pruned alphabet in order
//   P2  one thread per entry: its pb / pnb in the host's order of contributions, its rank key and tie key
//   P3  one thread per live candidate: rank by counting the candidates ahead of it (score, then first insertion);
//       the k first become the next beam, new members are interned
// LDS holds two frames of entry masses plus the live-candidate list (see lds_bytes); limits in w2l_hip.h.
//
// One entry point, w2l_ctc_beam_search, launches ctc_beam_search_kernel<lm != NULL, lexicon != NULL, hotwords != NULL>; what
// the search shares with the ASG one (asg_beam.hip) -- workspace, output stage, argument checks -- is
// beam_core.h's.
//
// With a language model (LM = true): every trie node also carries an LM state (NodeLM, after the
// intern table in the workspace), computed once by the P3 thread that interns the node from its parent's state and its
// character.  P2 adds a member's LM weight to the one contribution the host weights (parent_part, a word-closing label).
//
// With a lexicon (LEX = true): every beam slot carries the lexicon's spelling-trie node of
// its partial word (lex_trie, LDS).  The P2 thread of an extension entry that is not a beam member probes the trie once
// (lex_step); an extension that leaves the word list gets no mass, exactly like a pruned label.  The node of a new member is a
// function of its parent slot's node and its character, so P3 finds it with the same probe and nothing is kept per interned
// prefix.  The output stage keeps the members whose partial word is empty or a whole word (complete_only).
//
// With hotwords (HOT = true; any LM / LEX combination): every beam slot carries the hotword-trie walk
// of its string (hot_st, LDS: node of the partial word, its depth, the characters credited by closed hotwords).  The rank key
// gains gamma * h, h = hot_chars(state); masses are untouched.  The state of an extension is a function of its parent slot's
// state and its character (hot_step: one probe), computed by the P2 thread of a non-member extension for the key and again by
// the P3 thread that places a new member, as lex_trie is.
#include "beam_core.h"

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_KMAX = 64;          // beam slots live in one wave (P1)
constexpr int BS_AMAX = 128;         // two labels per lane of the frame-loading wave
constexpr int BS_NOT_PB = 1 << 30;   // tie key of a candidate that only ever entered pnb

struct LabelInfo {
    // bits 0-7: canonical (first) index of the label's character; 8: the blank character; 9: a word character (\w);
    // 10: a word separator ([\s|>])
    int32_t v[BS_AMAX];
};

// host loop position of an operation: beam slot i, label l (-1: the closed-hypothesis assignment), op within the label
__device__ __forceinline__ int loop_pos(int i, int A, int l, int op) { return ((i * (A + 1) + l + 1) << 2) | op; }

struct Acc {
    double b = -INFINITY, nb = -INFINITY;
    int bseq = 0x7fffffff, nbseq = 0x7fffffff;
    __device__ void add_b(double v, int pos) { b = lae(b, v); bseq = min(bseq, pos); }
    __device__ void add_nb(double v, int pos) { nb = lae(nb, v); nbseq = min(nbseq, pos); }
};

struct Beam {                         // one frame's beam, slot-indexed
    int node[BS_KMAX], parent[BS_KMAX], chr[BS_KMAX], words[BS_KMAX], len[BS_KMAX], ps[BS_KMAX], prevslot[BS_KMAX];
    double pb[BS_KMAX], pnb[BS_KMAX], score[BS_KMAX];
};

template <bool LM, bool LEX, bool HOT>
__global__ __launch_bounds__(BS_THREADS) void ctc_beam_search_kernel(
    const float* __restrict__ probs, const int32_t* __restrict__ sizes, int T, int A, LabelInfo info, int blank, int endc,
    int k, double beta, double prune, int log_probs, char* __restrict__ ws, int64_t ws_per_utt, int hash_cap,
    double* __restrict__ out_score, int32_t* __restrict__ out_len, int32_t* __restrict__ out_status,
    int32_t* __restrict__ out_labels, LmArgs lmargs, float* __restrict__ out_lm, LexArgs lex, HotArgs hot) {
    __shared__ Beam beams[2];
    __shared__ double lm_w[2][LM ? BS_KMAX : 1];          // LM weight (natural log) of each beam slot
    __shared__ int lm_on[2][LM ? BS_KMAX : 1];             // ... and whether it applies (a non-space character)
    __shared__ int lex_trie[2][LEX ? BS_KMAX : 1];        // lexicon trie node of each beam slot's partial word
    __shared__ HotState hot_st[2][HOT ? BS_KMAX : 1];     // hotword walk of each beam slot's string
    __shared__ double lpd[BS_AMAX];
    __shared__ int alph[BS_AMAX], act[BS_AMAX], lab[BS_AMAX];
    __shared__ int s_m[2], s_nalph, s_count, s_bad;
    extern __shared__ __attribute__((aligned(16))) double dyn[];

    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nE = k * A + k;                              // E(i, c) = i*A + c, S(i) = k*A + i
    double* mass = dyn;                                    // [2 frames][nE][pb, pnb]
    double* lsc = mass + 4 * nE;                           // live candidates: rank score
    int* lkey = (int*)(lsc + nE);                          //                  tie key (first insertion)
    int* lent = lkey + nE;                                 //                  entry index
    int* mem = lent + nE;                                  // [k][A] stamp | slot of the member that is E(i, c)
    int* redir = mem + k * A;                              // [k][A] stamp | previous slot whose S entry is E(i, c)

    const TrieWs w = carve_ws<2>(ws, n, ws_per_utt, T, k, hash_cap, lmargs.state_off);
    int32_t* nd_parent = w.nd_parent;
    int32_t* nd_chr = w.nd_chr;
    NodeLM* nd_lm = w.nd_lm;                               // LM only

    for (int i = tid; i < hash_cap; i += BS_THREADS) w.hkeys[i] = BS_EMPTY;
    for (int i = tid; i < 2 * k * A; i += BS_THREADS) mem[i] = 0;         // mem and redir: stamp 0 never matches
    for (int i = tid; i < A; i += BS_THREADS) { lab[i] = info.v[i]; act[i] = 0; }
    if (tid == 0) {
        nd_parent[0] = -1;
        nd_chr[0] = -1;
        Beam& b0 = beams[0];
        b0.node[0] = 0; b0.parent[0] = -1; b0.chr[0] = -1; b0.words[0] = 0; b0.len[0] = 0; b0.prevslot[0] = -1;
        b0.pb[0] = 0.0; b0.pnb[0] = -INFINITY; b0.score[0] = 0.0;
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
    const float* xn = probs + (int64_t)n * T * A;
    const double log_prune = prune > 0 ? log(prune) : -INFINITY;
    auto closed = [&](const Beam& b, int s) { return endc >= 0 && b.chr[s] == endc; };   // pre[-1] == end_char
    float nxt[2] = {0.f, 0.f};                             // wave 2: the frame to come, two labels per lane
    if (wave == 2 && Tn > 0)
        for (int h = 0; h < 2; ++h) if (lane + 64 * h < A) nxt[h] = xn[lane + 64 * h];
    __threadfence();
    __syncthreads();

    int cur = 0;                                           // parity of the current beam and of this frame's masses
    for (int t = 0; t < Tn; ++t) {
        const int m = s_m[cur], mprev = s_m[cur ^ 1];
        if (m == 0) break;                                 // the beam emptied: the result is '' (uniform: read after a barrier)
        const int stamp = (t + 1) << 7;
        Beam& B = beams[cur];
        const Beam& P = beams[cur ^ 1];
        // ---------------------------------------------------------------- P1
        if (wave == 0) {
            if (lane < m) {
                int ps = -1;
                for (int j = 0; j < m; ++j) if (B.node[j] == B.parent[lane]) { ps = j; break; }
                B.ps[lane] = ps;
                if (ps >= 0) mem[ps * A + B.chr[lane]] = stamp | lane;
            }
            if (lane == 0) s_count = 0;
        } else if (wave == 1) {
            // a previous member that had its own S entry and whose parent is now in the beam: its extension entry finds
            // last frame's mass there
            if (t > 0 && lane < mprev && P.ps[lane] < 0 && P.parent[lane] >= 0) {
                for (int j = 0; j < m; ++j)
                    if (B.node[j] == P.parent[lane]) { redir[j * A + P.chr[lane]] = stamp | lane; break; }
            }
        } else if (wave == 2) {
            int pass[2] = {0, 0};
            uint64_t mask[2];
            for (int h = 0; h < 2; ++h) {
                const int l = lane + 64 * h;
                if (l < A) {
                    const float v = nxt[h];
                    if (t + 1 < Tn) nxt[h] = xn[(int64_t)(t + 1) * A + l];      // the next frame's load hides behind this one
                    double lp;
                    if (log_probs) {
                        lp = (double)v;
                    } else {
                        if (!(v >= 0.f)) s_bad = 1;
                        lp = log((double)v);
                    }
                    lpd[l] = lp;
                    // frame > prune as the host compares it (probabilities), or lp > log(prune)
                    pass[h] = log_probs ? (prune < 0 || lp > log_prune) : (double)v > prune;
                    if (pass[h] && !(lab[l] & 0x100)) act[lab[l] & 0xff] = t + 1;
                }
                mask[h] = __ballot(pass[h]);
            }
            const int n0 = __popcll(mask[0]);
            if (pass[0]) alph[__popcll(mask[0] & ((1ull << lane) - 1))] = lane;
            if (pass[1]) alph[n0 + __popcll(mask[1] & ((1ull << lane) - 1))] = lane + 64;
            if (lane == 0) s_nalph = n0 + __popcll(mask[1]);
        }
        __syncthreads();
        // ---------------------------------------------------------------- P2
        const int L = s_nalph;
        const double pblank = lpd[blank];
        const double* mprev_tab = mass + (cur ^ 1) * 2 * nE;
        double* mcur = mass + cur * 2 * nE;
        for (int e = tid; e < m * A + m; e += BS_THREADS) {
            const int ent = e < m * A ? e : k * A + (e - m * A);
            Acc acc;
            bool live = false;
            int words = 0;
            [[maybe_unused]] int hchars = 0;                         // HOT: h of the entry's string
            if (e < m * A) {
                const int i = e / A, c = e - i * A;
                const int mv = mem[ent];
                const int s = (mv >> 7) == t + 1 ? (mv & 127) : -1;
                bool ext = act[c] == t + 1 && !closed(B, i);         // labels of c passed the prune; slot i is open
                if constexpr (LEX) {                                 // ... and the extension stays in the lexicon
                    if (ext && s < 0) ext = lex_step(lex, lex_trie[cur][i], c, endc) >= 0;
                }
                if (ext || s >= 0) {
                    live = true;
                    // contributions of slot i extended by c (beam_search.py: the non-blank branches of pre = slot i)
                    auto parent_part = [&]() {
                        if (!ext) return;
                        const bool rep = B.parent[i] >= 0 && B.chr[i] == c;
                        const double lin = rep ? B.pb[i] : lae(B.pb[i], B.pnb[i]);
                        double fb = -INFINITY, fnb = -INFINITY;
                        if (s < 0) {
                            int pidx = -1;
                            if (B.prevslot[i] >= 0) {
                                pidx = B.prevslot[i] * A + c;
                            } else {
                                const int rv = redir[ent];
                                if ((rv >> 7) == t + 1) pidx = k * A + (rv & 127);
                            }
                            if (pidx >= 0) {
                                fb = lae(mprev_tab[2 * pidx], mprev_tab[2 * pidx + 1]);
                                fnb = mprev_tab[2 * pidx + 1];
                            }
                        }
                        const double p = lpd[c];
                        for (int q = 0; q < L; ++q) {
                            const int l = alph[q];
                            if ((lab[l] & 0xff) != c || (lab[l] & 0x100)) continue;
                            if constexpr (LM) {        // a word closes: the member's LM weight (decoder.py:210-212)
                                double v = p + lin;
                                if (!rep && (c == lmargs.space || c == endc) && lm_on[cur][i]) v += lm_w[cur][i];
                                acc.add_nb(v, loop_pos(i, A, l, 0));
                            } else {
                                acc.add_nb(p + lin, loop_pos(i, A, l, 0));
                            }
                            if (s < 0) {                   // the extension fell off the beam: last frame's mass joins
                                acc.add_b(pblank + fb, loop_pos(i, A, l, 2));
                                acc.add_nb(p + fnb, loop_pos(i, A, l, 3));
                            }
                        }
                    };
                    if (s < 0) {
                        parent_part();
                        words = B.words[i] + ((lab[c] & 0x400) && B.chr[i] >= 0 && (lab[B.chr[i]] & 0x200));
                        if constexpr (HOT) hchars = hot_chars(hot_step(hot, hot_st[cur][i], c, endc));
                    } else {
                        words = B.words[s];
                        if constexpr (HOT) hchars = hot_chars(hot_st[cur][s]);
                        if (i < s) parent_part();
                        // own contributions of member s (blank, repeated character, or the closed-hypothesis assignment)
                        if (closed(B, s)) {
                            acc.b = B.pb[s];
                            acc.nb = B.pnb[s];
                            acc.bseq = min(acc.bseq, loop_pos(s, A, -1, 0));
                            acc.nbseq = min(acc.nbseq, loop_pos(s, A, -1, 1));
                        } else {
                            const double ms = lae(B.pb[s], B.pnb[s]);
                            for (int q = 0; q < L; ++q) {
                                const int l = alph[q];
                                if (lab[l] & 0x100) acc.add_b(pblank + ms, loop_pos(s, A, l, 0));
                                else if ((lab[l] & 0xff) == B.chr[s]) acc.add_nb(lpd[B.chr[s]] + B.pnb[s], loop_pos(s, A, l, 1));
                            }
                        }
                        if (i > s) parent_part();
                    }
                }
            } else {
                const int s = e - m * A;
                if (B.ps[s] < 0) {                         // a member whose parent is not in the beam (the root included)
                    live = true;
                    words = B.words[s];
                    if constexpr (HOT) hchars = hot_chars(hot_st[cur][s]);
                    if (closed(B, s)) {
                        acc.b = B.pb[s];
                        acc.nb = B.pnb[s];
                        acc.bseq = loop_pos(s, A, -1, 0);
                        acc.nbseq = loop_pos(s, A, -1, 1);
                    } else {
                        const double ms = lae(B.pb[s], B.pnb[s]);
                        const bool root = B.parent[s] < 0;
                        for (int q = 0; q < L; ++q) {
                            const int l = alph[q];
                            if (lab[l] & 0x100) acc.add_b(pblank + ms, loop_pos(s, A, l, 0));
                            else if (!root && (lab[l] & 0xff) == B.chr[s]) acc.add_nb(lpd[B.chr[s]] + B.pnb[s], loop_pos(s, A, l, 1));
                        }
                    }
                }
            }
            mcur[2 * ent] = acc.b;
            mcur[2 * ent + 1] = acc.nb;
            const double total = lae(acc.b, acc.nb);
            if (live && total > -INFINITY) {               // Counter addition keeps strictly positive masses only
                const int slot = atomicAdd(&s_count, 1);
                if constexpr (HOT) lsc[slot] = total + beta * log((double)(words + 1)) + hot.gamma * (double)hchars;
                else lsc[slot] = total + beta * log((double)(words + 1));
                lkey[slot] = acc.bseq != 0x7fffffff ? acc.bseq : BS_NOT_PB + acc.nbseq;
                lent[slot] = ent;
            }
        }
        __syncthreads();
        // ---------------------------------------------------------------- P3
        const int M = s_count;
        Beam& NB = beams[cur ^ 1];
        for (int x = tid; x < M; x += BS_THREADS) {
            const double sx = lsc[x];
            const int kx = lkey[x];
            int r = 0;
            for (int y = 0; y < M && r < k; ++y) {
                const double sy = lsc[y];
                r += sy > sx || (sy == sx && lkey[y] < kx);
            }
            if (r >= k) continue;
            const int ent = lent[x];
            int s, i = -1, c = -1;
            if (ent < k * A) {
                i = ent / A;
                c = ent - i * A;
                const int mv = mem[ent];
                s = (mv >> 7) == t + 1 ? (mv & 127) : -1;
            } else {
                s = ent - k * A;
            }
            if (s >= 0) {
                NB.node[r] = B.node[s]; NB.parent[r] = B.parent[s]; NB.chr[r] = B.chr[s];
                NB.words[r] = B.words[s]; NB.len[r] = B.len[s]; NB.prevslot[r] = s;
                if constexpr (LM) { lm_w[cur ^ 1][r] = lm_w[cur][s]; lm_on[cur ^ 1][r] = lm_on[cur][s]; }
                if constexpr (LEX) lex_trie[cur ^ 1][r] = lex_trie[cur][s];
                if constexpr (HOT) hot_st[cur ^ 1][r] = hot_st[cur][s];
            } else {
                const int par = B.node[i];
                if constexpr (LEX) lex_trie[cur ^ 1][r] = lex_step(lex, lex_trie[cur][i], c, endc);   // >= 0: P2 let it live
                if constexpr (HOT) hot_st[cur ^ 1][r] = hot_step(hot, hot_st[cur][i], c, endc);
                const uint64_t key = ((uint64_t)par << 8) | (uint64_t)c;
                uint32_t h = key_hash(key) & (hash_cap - 1);
                int node = -1;
                while (node < 0) {                         // probe by claiming: one round trip per slot
                    const uint64_t cur_key =
                        atomicCAS((unsigned long long*)&w.hkeys[h], (unsigned long long)BS_EMPTY, (unsigned long long)key);
                    if (cur_key == BS_EMPTY) {             // a new string: its node id is reserved by (frame, rank)
                        node = 1 + t * k + r;
                        w.hvals[h] = node;
                        nd_parent[node] = par;
                        nd_chr[node] = c;
                        if constexpr (LM) {
                            const NodeLM ns = lm_extend(lmargs, nd_lm[par], c, endc);
                            nd_lm[node] = ns;
                            lm_w[cur ^ 1][r] = lmargs.alpha_ln10 * (double)ns.total;
                            lm_on[cur ^ 1][r] = ns.nonspace;
                        }
                    } else if (cur_key == key) {           // interned in an earlier frame
                        node = w.hvals[h];
                        if constexpr (LM) {
                            lm_w[cur ^ 1][r] = lmargs.alpha_ln10 * (double)nd_lm[node].total;
                            lm_on[cur ^ 1][r] = nd_lm[node].nonspace;
                        }
                    } else {
                        h = (h + 1) & (hash_cap - 1);
                    }
                }
                NB.node[r] = node; NB.parent[r] = par; NB.chr[r] = c;
                NB.words[r] = B.words[i] + ((lab[c] & 0x400) && B.chr[i] >= 0 && (lab[B.chr[i]] & 0x200));
                NB.len[r] = B.len[i] + 1;
                NB.prevslot[r] = -1;
            }
            NB.pb[r] = mcur[2 * ent];
            NB.pnb[r] = mcur[2 * ent + 1];
            NB.score[r] = sx;
        }
        if (tid == 0) s_m[cur ^ 1] = min(M, k);
        __threadfence();                                   // interned nodes are read by other waves in later frames
        __syncthreads();
        cur ^= 1;
    }
    // ---------------------------------------------------------------- output: backtrack the final beam
    const int m = s_m[cur];
    const Beam& B = beams[cur];
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
    return nE * (4 * 8 + 8 + 4 + 4) + 2 * (int64_t)k * A * 4;
}

// what the eight instantiations are launched with: the arguments checked, the tables in their device form
struct CtcSearch {
    const float* probs;
    const int32_t* sizes;
    int N, T, A, blank, end_index, k, log_probs;
    double beta, prune;
    LabelInfo info;
    void* workspace;
    int64_t ws_per_utt;
    void* out;
    void* stream;
    LmArgs lm;
    LexArgs lex;
    HotArgs hot;
};

template <bool LM, bool LEX, bool HOT>
int launch_search(const char* name, const CtcSearch& s) {
    const int64_t lds = lds_bytes(s.k, s.A);
    if (int rc = lds_args(name, (const void*)ctc_beam_search_kernel<LM, LEX, HOT>, lds, s.k, s.A)) return rc;
    const OutSections o = out_sections(s.out, s.N, s.T, s.k, LM);
    hipLaunchKernelGGL((ctc_beam_search_kernel<LM, LEX, HOT>), dim3(s.N), dim3(BS_THREADS), (size_t)lds, (hipStream_t)s.stream,
                       s.probs, s.sizes, s.T, s.A, s.info, s.blank, s.end_index, s.k, s.beta, s.prune, s.log_probs,
                       (char*)s.workspace, s.ws_per_utt, hash_capacity(s.T, s.k), o.score, o.len, o.status, o.labels, s.lm, o.lm,
                       s.lex, s.hot);
    W2L_CHECK_LAUNCH();
    return 0;
}

__global__ void ngram_insert_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t n,
                                    uint64_t* __restrict__ tkeys, int32_t* __restrict__ tvals, uint32_t mask,
                                    int32_t* __restrict__ dups) {
    for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[x];
        uint32_t h = key_hash(key) & mask;
        for (;;) {
            const uint64_t prev =
                atomicCAS((unsigned long long*)&tkeys[h], (unsigned long long)BS_EMPTY, (unsigned long long)key);
            if (prev == BS_EMPTY) { tvals[h] = vals[x]; break; }
            if (prev == key) { atomicAdd(dups, 1); break; }
            h = (h + 1) & mask;
        }
    }
}

}  // namespace

extern "C" int w2l_ngram_lm_build(const uint64_t* keys, const int32_t* vals, int64_t n, uint64_t* table_keys, int32_t* table_vals,
                                  int64_t cap, int32_t* dups, void* stream) {
    W2L_CHECK_ARG(n >= 0 && table_keys && table_vals && dups && (n == 0 || (keys && vals)), "ngram_lm_build: bad arguments");
    W2L_CHECK_ARG(pow2_cap(cap) && cap >= 2 * n, "ngram_lm_build: capacity %lld for %lld keys (a power of two in [16, 2^31], "
                  ">= 2n)", (long long)cap, (long long)n);
    W2L_CHECK_HIP(hipMemsetAsync(table_keys, 0xff, (size_t)cap * 8, (hipStream_t)stream));
    W2L_CHECK_HIP(hipMemsetAsync(table_vals, 0xff, (size_t)cap * 4, (hipStream_t)stream));
    if (n == 0) return 0;
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(ngram_insert_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, keys, vals, n, table_keys,
                       table_vals, (uint32_t)(cap - 1), dups);
    W2L_CHECK_LAUNCH();
    return 0;
}

// Nothing is kept per interned prefix for a lexicon or for hotwords (see the head of this file): only an LM adds to the workspace.
extern "C" int64_t w2l_ctc_beam_search_workspace_bytes(int N, int T, int k, int order) {
    return search_ws_bytes(N, T, k, order, 2);
}

extern "C" int w2l_ctc_beam_search(const float* probs, const int32_t* sizes, int N, int T, int A,
                                   const int32_t* label_info_host, int blank, int end_index, int space_index, int k,
                                   double alpha, double beta, double prune, int log_probs, const w2l_ngram_lm_t* lm, int order,
                                   const w2l_lexicon_t* lexicon, int complete_only, const w2l_lexicon_t* hotwords,
                                   double hotword_weight, void* workspace, int64_t workspace_bytes, void* out, void* stream) {
    const char* name = "ctc_beam_search";
    // every check of the arguments comes before the first HIP call (launch_search)
    W2L_CHECK_ARG(probs && label_info_host && workspace && out && N > 0 && T > 0, "%s: bad arguments", name);
    W2L_CHECK_ARG(A >= 1 && A <= BS_AMAX, "%s: %d labels, supported 1..%d", name, A, BS_AMAX);
    W2L_CHECK_ARG(k >= 1 && k <= BS_KMAX, "%s: beam width k=%d, supported 1..%d", name, k, BS_KMAX);
    W2L_CHECK_ARG(blank >= 0 && blank < A && end_index >= -1 && end_index < A, "%s: blank %d / end %d outside %d labels",
                  name, blank, end_index, A);
    W2L_CHECK_ARG((int64_t)k * T < (1 << 29) && T < (1 << 24), "%s: k*T = %lld too large", name, (long long)k * T);
    CtcSearch s{probs, sizes, N, T, A, blank, end_index, k, log_probs, beta, prune};
    if (int rc = label_info_args(name, label_info_host, A, s.info.v, BS_AMAX)) return rc;
    if (lm || lexicon || hotwords)
        if (int rc = space_args(name, label_info_host, A, space_index)) return rc;
    if (lm)
        if (int rc = lm_args(name, space_index, alpha, lm, order, T, k, 2, &s.lm)) return rc;
    if (lexicon) {
        if (int rc = trie_args(name, "lexicon", space_index, lexicon, &s.lex)) return rc;
        s.lex.complete_only = complete_only != 0;
    }
    if (hotwords) {
        W2L_CHECK_ARG(std::isfinite(hotword_weight), "%s: the hotword weight is not finite", name);
        if (int rc = trie_args(name, "hotword", space_index, hotwords, &s.hot)) return rc;
        s.hot.gamma = hotword_weight;
    }
    const int64_t need = w2l_ctc_beam_search_workspace_bytes(N, T, k, lm ? order : 0);
    W2L_CHECK_ARG(need > 0 && workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", name,
                  (long long)workspace_bytes, (long long)need);
    s.workspace = workspace;
    s.ws_per_utt = lm ? lm_ws_stride(T, k, 2) : ws_stride(T, k, 2);
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


// The word n-gram language model on the device, shared by the beam searches (beam_search.hip: CTC; asg_beam.hip: ASG): the
// exact-key open-addressing lookup, the per-trie-node LM state and its two transitions (a word closes / a character is
// spelled).  Tables: w2l_ngram_lm_t (include/w2l_hip.h), built by w2l_ngram_lm_build; host model: ngram_lm.ArpaLM.
// Everything is internal to the including file (anonymous namespace).
#pragma once
#include "common.h"

namespace {

constexpr uint64_t BS_EMPTY = ~0ull;

__device__ __forceinline__ uint32_t key_hash(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// ------------------------------------------------------------------------------------------------------- language model
constexpr int LM_MAXORDER = 6;
constexpr int LM_EOS = 2;                     // word ids: <unk> 0, <s> 1, </s> 2

struct LmArgs {                               // w2l_ngram_lm_t on the device, plus the search's LM parameters
    const float* prob;
    const float* bo;
    const uint64_t* nkeys;
    const int32_t* nvals;
    const uint64_t* tkeys;
    const int32_t* tvals;
    const int32_t* tword;
    uint32_t nmask, tmask;
    int order, space;
    double alpha_ln10;
    int64_t state_off;                        // byte offset of the NodeLM array in an utterance's workspace
};

struct NodeLM {                               // 64 bytes per trie node
    int32_t ctx[LM_MAXORDER - 1];             // the last m words, most recent first
    float bo[LM_MAXORDER - 1];                // log10 backoff of the context ctx[L-1] .. ctx[0] (0: absent)
    int32_t m;
    float done;                               // float32 sum of the closed words' log10 q
    int32_t trie;                             // spelling-trie node of the partial word: 0 empty, -1 off the trie
    int32_t nonspace;                         // the string has a character other than ' '
    float total;                              // log10 of the string's words with </s> (0 if !nonspace)
    int32_t pad_;
};

__device__ __forceinline__ int tab_find(const uint64_t* keys, const int32_t* vals, uint32_t mask, uint64_t key) {
    uint32_t h = key_hash(key) & mask;
    for (;;) {                                // at most half full: an empty slot ends every probe sequence
        const uint64_t kk = keys[h];
        if (kk == key) return vals[h];
        if (kk == BS_EMPTY) return -1;
        h = (h + 1) & mask;
    }
}

// ------------------------------------------------------------------------------------------------------------- lexicon
struct TrieArgs {                             // a spelling trie (w2l_lexicon_t) on the device, and the word separator
    const uint64_t* tkeys;
    const int32_t* tvals;
    const int32_t* tword;
    uint32_t tmask;
    int space;
};

struct LexArgs : TrieArgs {                   // the lexicon (lexicon.Lexicon), plus the search's parameter
    int complete_only;
};

// the lexicon's trie node of (partial word at node `trie`) + canonical label c; < 0: the extension leaves the word list.
// A separator (the space, end_char) closes an empty partial word or a whole word, and the partial word is empty again.
__device__ __forceinline__ int lex_step(const LexArgs& X, int trie, int c, int endc) {
    if (c == X.space || c == endc) return trie == 0 || X.tword[trie] >= 0 ? 0 : -1;
    return tab_find(X.tkeys, X.tvals, X.tmask, ((uint64_t)trie << 8) | (uint64_t)c);
}

__device__ __forceinline__ bool lex_complete(const LexArgs& X, int trie) { return trie == 0 || X.tword[trie] >= 0; }

// ------------------------------------------------------------------------------------------------------------ hotwords
struct HotArgs : TrieArgs {                   // the hotword list's spelling trie and the bonus per character
    double gamma;
};

struct HotState {                             // of a string: h = credit + (node > 0 ? depth : 0), Lexicon.boost_chars
    int node;                                 // hotword-trie node of the partial word: 0 empty, -1 it has left the trie
    int depth;                                // characters of the partial word (kept while the node is alive)
    int credit;                               // characters of the closed words that are hotwords
};

// the state of (string of state s) + canonical label c.  A separator credits the partial word if it is a whole hotword and
// empties it; another label walks the trie (one probe) while the partial word is still on it.
__device__ __forceinline__ HotState hot_step(const HotArgs& H, HotState s, int c, int endc) {
    if (c == H.space || c == endc) {
        if (s.node > 0 && H.tword[s.node] >= 0) s.credit += s.depth;
        s.node = 0;
        s.depth = 0;
    } else if (s.node >= 0) {
        s.node = tab_find(H.tkeys, H.tvals, H.tmask, ((uint64_t)s.node << 8) | (uint64_t)c);
        s.depth += 1;
    }
    return s;
}

__device__ __forceinline__ int hot_chars(const HotState& s) { return s.credit + (s.node > 0 ? s.depth : 0); }

// log10 q(w | s) (ngram_lm.ArpaLM.q) by the reverse-suffix walk w, h_1 w, h_2 h_1 w, ...; with nx, also the state after w
__device__ float lm_word(const LmArgs& L, const NodeLM& s, int w, NodeLM* nx) {
    int e = w;
    float prob = L.prob[e];
    float nbo[LM_MAXORDER];
    nbo[0] = L.bo[e];
    int j = 0, depth = 1;
    bool alive = true;
#pragma unroll
    for (int i = 0; i < LM_MAXORDER - 1; ++i) {
        if (alive && i < s.m) {
            const int e2 = tab_find(L.nkeys, L.nvals, L.nmask, ((uint64_t)e << 32) | (uint32_t)s.ctx[i]);
            if (e2 < 0) {
                alive = false;
            } else {
                e = e2;
                depth = i + 2;
                const float p = L.prob[e];
                if (p == p) { prob = p; j = i + 1; }       // NaN: a context-only entry
                nbo[i + 1] = L.bo[e];
            }
        }
    }
    float q = prob;
#pragma unroll
    for (int i = 0; i < LM_MAXORDER - 1; ++i)
        if (i >= j && i < s.m) q += s.bo[i];               // increasing context length, float32
    if (nx) {
        const int m2 = min(s.m + 1, L.order - 1);
#pragma unroll
        for (int i = LM_MAXORDER - 2; i >= 1; --i) nx->ctx[i] = i < m2 ? s.ctx[i - 1] : 0;
        nx->ctx[0] = w;
#pragma unroll
        for (int i = 0; i < LM_MAXORDER - 1; ++i) nx->bo[i] = i < m2 && i < depth ? nbo[i] : 0.f;
        nx->m = m2;
    }
    return q;
}

// the LM state of the node (parent state s) + canonical label c
__device__ NodeLM lm_extend(const LmArgs& L, const NodeLM& s, int c, int endc) {
    NodeLM ns = s;
    if (c == L.space || c == endc) {
        if (s.trie != 0) {                                 // a word closes (a partial word off the trie is <unk>)
            int wid = s.trie > 0 ? L.tword[s.trie] : -1;
            const float q = lm_word(L, s, wid < 0 ? 0 : wid, &ns);
            ns.done = s.done + q;
            ns.trie = 0;
        }
        if (c == endc) ns.nonspace = 1;                    // (a closed string is never extended: this only shows in lm_log10)
    } else {
        ns.nonspace = 1;
        ns.trie = s.trie >= 0 ? tab_find(L.tkeys, L.tvals, L.tmask, ((uint64_t)s.trie << 8) | (uint64_t)c) : -1;
    }
    float total = 0.f;
    if (ns.nonspace) {
        if (ns.trie == 0) {
            total = ns.done + lm_word(L, ns, LM_EOS, nullptr);
        } else {
            const int wid = ns.trie > 0 ? L.tword[ns.trie] : -1;
            NodeLM tmp;
            const float d = ns.done + lm_word(L, ns, wid < 0 ? 0 : wid, &tmp);
            total = d + lm_word(L, tmp, LM_EOS, nullptr);
        }
    }
    ns.total = total;
    return ns;
}

}  // namespace

// What the two prefix beam searches (beam_search.hip: CTC; asg_beam.hip: ASG) have in common beside the language model of
// beam_lm.h.  Device side: the log-add of two masses, the root LM state, the per-utterance workspace (a trie of k*T+1 nodes
// and its intern table) and the back-tracking output stage.  (The claim-by-CAS intern probe is written out in both kernels'
// P3: as a function, whether it returns "created" or takes the new-node / found-node work as callables, it moves the
// kernels' register counts, profiles/beam_entry_refactor.txt.)  Host side: the workspace arithmetic, the sections of `out`,
// the label-info and LDS checks, and the checks that turn the C descriptors (w2l_ngram_lm_t, w2l_lexicon_t) into their
// device forms.  The frame phases P1 / P2 / P3 are the kernels' own.
// Everything is internal to the including file (anonymous namespace).
#pragma once
#include "common.h"
#include "beam_lm.h"
#include "../../include/w2l_hip.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------- device
__device__ __forceinline__ double lae(double a, double b) {          // log(exp(a) + exp(b))
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const double m = a > b ? a : b, d = a > b ? b - a : a - b;
    return m + log1p(exp(d));
}

__device__ __forceinline__ NodeLM lm_root(const LmArgs& L) {        // the LM state of the empty string: context <s>
    NodeLM r;
    for (int i = 0; i < LM_MAXORDER - 1; ++i) { r.ctx[i] = 0; r.bo[i] = 0.f; }
    r.m = min(1, L.order - 1);
    if (r.m > 0) { r.ctx[0] = 1; r.bo[0] = L.bo[1]; }
    r.done = 0.f; r.trie = 0; r.nonspace = 0; r.total = 0.f; r.pad_ = 0;
    return r;
}

// One utterance's workspace: NODE_WORDS int32 arrays of k*T+1 trie nodes (parent, label; ASG: packed decoded label and word
// count), the intern table (hash_cap keys, then values) and, with an LM, a NodeLM per node from byte state_off.
struct TrieWs {
    int32_t *nd_parent, *nd_chr, *nd_info;                 // nd_info: NODE_WORDS == 3 only
    uint64_t* hkeys;
    int32_t* hvals;
    NodeLM* nd_lm;                                         // LM only
};

template <int NODE_WORDS>
__device__ __forceinline__ TrieWs carve_ws(char* ws, int n, int64_t ws_per_utt, int T, int k, int hash_cap, int64_t state_off) {
    const int64_t nodes = (int64_t)k * T + 1;
    char* wsn = ws + (int64_t)n * ws_per_utt;
    TrieWs w;
    w.nd_parent = (int32_t*)wsn;
    w.nd_chr = w.nd_parent + nodes;
    w.nd_info = w.nd_chr + nodes;
    w.hkeys = (uint64_t*)(wsn + (nodes * 4 * NODE_WORDS + 15) / 16 * 16);
    w.hvals = (int32_t*)(w.hkeys + hash_cap);
    w.nd_lm = (NodeLM*)(wsn + state_off);
    return w;
}

// Slot o of the results: member `src` of the final beam B, its labels back-tracked through the trie; src < 0: an empty slot.
template <bool LM, class BeamT>
__device__ __forceinline__ void write_result(const BeamT& B, int src, int64_t o, int T, const TrieWs& w,
                                             double* __restrict__ out_score, int32_t* __restrict__ out_len,
                                             int32_t* __restrict__ out_labels, float* __restrict__ out_lm) {
    if (src >= 0) {
        const int len = B.len[src];
        out_score[o] = B.score[src];
        out_len[o] = len;
        if constexpr (LM) out_lm[o] = w.nd_lm[B.node[src]].total;
        int32_t* lab_out = out_labels + o * T;
        int node = B.node[src];
        for (int p = len - 1; p >= 0; --p) {
            lab_out[p] = w.nd_chr[node];
            node = w.nd_parent[node];
        }
    } else {
        out_score[o] = -INFINITY;
        out_len[o] = -1;
        if constexpr (LM) out_lm[o] = 0.f;
    }
}

// --------------------------------------------------------------------------------------------------------------- host
int hash_capacity(int T, int k) {
    int64_t need = 2 * ((int64_t)k * T + 1), cap = 1;
    while (cap < need) cap <<= 1;
    return (int)cap;
}

int64_t ws_stride(int T, int k, int node_words) {          // bytes of one utterance without an LM (carve_ws)
    const int64_t nodes = (int64_t)k * T + 1;
    const int64_t bytes = (nodes * 4 * node_words + 15) / 16 * 16 + (int64_t)hash_capacity(T, k) * 12;
    return (bytes + 255) / 256 * 256;
}

int64_t lm_state_offset(int T, int k, int node_words) { return ws_stride(T, k, node_words); }

int64_t lm_ws_stride(int T, int k, int node_words) {       // ... and with one
    const int64_t bytes = lm_state_offset(T, k, node_words) + ((int64_t)k * T + 1) * (int64_t)sizeof(NodeLM);
    return (bytes + 255) / 256 * 256;
}

// the workspace of N utterances (order 0: no LM); -1 if out of range
int64_t search_ws_bytes(int N, int T, int k, int order, int node_words) {
    if (N <= 0 || T <= 0 || k <= 0 || (int64_t)k * T >= (1 << 29) || order < 0 || order > LM_MAXORDER) return -1;
    return (int64_t)N * (order ? lm_ws_stride(T, k, node_words) : ws_stride(T, k, node_words));
}

bool pow2_cap(int64_t cap) { return cap >= 16 && cap <= (1ll << 31) && (cap & (cap - 1)) == 0; }

struct OutSections {                                       // of the `out` buffer (include/w2l_hip.h)
    double* score;
    int32_t *len, *status, *labels;
    float* lm;                                             // NULL without an LM
};

OutSections out_sections(void* out, int N, int T, int k, bool lm) {
    OutSections o;
    o.score = (double*)out;
    o.len = (int32_t*)(o.score + (int64_t)N * k);
    o.status = o.len + (int64_t)N * k;
    o.labels = o.status + N;
    o.lm = lm ? (float*)(o.labels + (int64_t)N * k * T) : nullptr;
    return o;
}

// label_info_host[A] -> the kernel's table v[amax]: every label's canonical index is a first index at or below it
int label_info_args(const char* name, const int32_t* label_info_host, int A, int32_t* v, int amax) {
    for (int i = 0; i < amax; ++i) v[i] = 0;
    for (int i = 0; i < A; ++i) {
        const int canon = label_info_host[i] & 0xff;
        W2L_CHECK_ARG(canon <= i && (label_info_host[canon] & 0xff) == canon, "%s: label %d: bad canonical index %d", name, i,
                      canon);
        v[i] = label_info_host[i];
    }
    return 0;
}

// What a word table (LM, lexicon, hotwords) asks of the labels: the space index is a first index, and no other label is
// whitespace (label-info bit 11).
int space_args(const char* name, const int32_t* label_info_host, int A, int space_index) {
    W2L_CHECK_ARG(space_index >= -1 && space_index < A && (space_index < 0 || (label_info_host[space_index] & 0xff) == space_index),
                  "%s: space index %d is not the first index of a label", name, space_index);
    for (int i = 0; i < A; ++i)
        W2L_CHECK_ARG(!(label_info_host[i] & 0x800) || (label_info_host[i] & 0xff) == space_index,
                      "%s: label %d is whitespace other than ' '", name, i);
    return 0;
}

// the checks of an n-gram model's tables, and their device form (node_words: of the search's trie, see carve_ws)
int lm_args(const char* name, int space_index, double alpha, const w2l_ngram_lm_t* lm, int order, int T, int k, int node_words,
            LmArgs* a) {
    W2L_CHECK_ARG(order >= 1 && order <= LM_MAXORDER, "%s: order %d, supported 1..%d", name, order, LM_MAXORDER);
    W2L_CHECK_ARG(lm->prob && lm->bo && lm->ngram_keys && lm->ngram_vals && lm->trie_keys && lm->trie_vals && lm->trie_word,
                  "%s: a table pointer is NULL", name);
    W2L_CHECK_ARG(lm->n_words >= 3 && lm->n_entries >= lm->n_words && lm->n_entries < (1 << 30) && lm->n_trie_nodes >= 1,
                  "%s: %d entries, %d words, %d trie nodes (3 <= words <= entries < 2^30)", name, lm->n_entries,
                  lm->n_words, lm->n_trie_nodes);
    W2L_CHECK_ARG(pow2_cap(lm->ngram_cap) && lm->ngram_cap >= 2 * (int64_t)(lm->n_entries - lm->n_words) && pow2_cap(lm->trie_cap)
                      && lm->trie_cap >= 2 * (int64_t)(lm->n_trie_nodes - 1),
                  "%s: table capacities %lld / %lld (powers of two in [16, 2^31], at most half full)", name,
                  (long long)lm->ngram_cap, (long long)lm->trie_cap);
    a->prob = lm->prob;
    a->bo = lm->bo;
    a->nkeys = lm->ngram_keys;
    a->nvals = lm->ngram_vals;
    a->tkeys = lm->trie_keys;
    a->tvals = lm->trie_vals;
    a->tword = lm->trie_word;
    a->nmask = (uint32_t)(lm->ngram_cap - 1);
    a->tmask = (uint32_t)(lm->trie_cap - 1);
    a->order = order;
    a->space = space_index;
    a->alpha_ln10 = alpha * 2.302585092994045684;
    a->state_off = lm_state_offset(T, k, node_words);
    return 0;
}

// ... and of a spelling trie (what: "lexicon" or "hotword")
int trie_args(const char* name, const char* what, int space_index, const w2l_lexicon_t* t, TrieArgs* x) {
    W2L_CHECK_ARG(t->trie_keys && t->trie_vals && t->trie_word, "%s: a %s table pointer is NULL", name, what);
    W2L_CHECK_ARG(t->n_trie_nodes >= 1 && pow2_cap(t->trie_cap) && t->trie_cap >= 2 * (int64_t)(t->n_trie_nodes - 1),
                  "%s: %s trie of %d nodes in a table of capacity %lld (a power of two in [16, 2^31], at most half full)", name,
                  what, t->n_trie_nodes, (long long)t->trie_cap);
    x->tkeys = t->trie_keys;
    x->tvals = t->trie_vals;
    x->tword = t->trie_word;
    x->tmask = (uint32_t)(t->trie_cap - 1);
    x->space = space_index;
    return 0;
}

// The kernel's static LDS plus `lds` dynamic bytes must fit the 160 KiB of a CU; past the default 64 KiB the kernel's dynamic
// limit is raised to what its static state leaves of them.
int lds_args(const char* name, const void* kern, int64_t lds, int k, int A) {
    hipFuncAttributes fa;
    W2L_CHECK_HIP(hipFuncGetAttributes(&fa, kern));
    const int64_t all = lds + (int64_t)fa.sharedSizeBytes;
    W2L_CHECK_ARG(all <= 160 * 1024, "%s: k=%d with %d labels needs %lld bytes of LDS, the limit is %d", name, k, A,
                  (long long)all, 160 * 1024);
    if (all > 64 * 1024)
        W2L_CHECK_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)fa.sharedSizeBytes));
    return 0;
}

}  // namespace

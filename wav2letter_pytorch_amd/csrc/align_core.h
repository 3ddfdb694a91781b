// The host side of Viterbi forced alignment shared by ctc_align.hip (w2l_ctc_align) and asg_beam.hip (w2l_asg_align): the
// plan (block shape, and whether the moves live in LDS or in the caller's workspace), the workspace query and the launcher
// with its (NT, SPT) switch.  The two kernels and their params structs stay in their files: one structure, written out per
// criterion, because a shared device body, and even another order of the params' fields, changed the kernels' code generation
// and their speed by percents (profiles/align_core_refactor.txt).
// A criterion is a Rule type (CtcRule, AsgRule), all static: NAME (the prefix of the launcher's messages), GUARD (cells at
// -inf below state 0 of a column, as in its kernel's layout), MAX_SPT and MAX_STATES (the widest block shape it
// instantiates, the most states it accepts), states(S) and lds_round(bytes of fixed LDS).
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr float NEG_INF = -INFINITY;

struct AlignPlan {
    int nt, spt;
    size_t lds_fixed;      // columns + state sequence
    size_t bp_bytes;       // moves of one utterance
    bool bp_lds;
};

// block shape and where the moves live, from the shapes alone (the workspace query and the launch must agree)
template <class Rule>
bool align_plan(int T, int Smax, AlignPlan* pl) {
    if (T <= 0 || T > 32768 || Smax < 0 || Rule::states(Smax) > Rule::MAX_STATES) return false;
    const int L = Rule::states(Smax) < 1 ? 1 : Rule::states(Smax);
    static const int kWide[] = {64, 128, 256, 512, 1024};
    int nt = 1024;
    for (int w : kWide)
        if (L <= w) { nt = w; break; }
    int spt = (L + nt - 1) / nt;
    if (spt > 2) spt = spt <= 4 ? 4 : 8;
    pl->nt = nt;
    pl->spt = spt;
    const size_t lw = (size_t)nt * spt;
    pl->lds_fixed = Rule::lds_round(4 * sizeof(float) + 2 * (lw + Rule::GUARD) * sizeof(float) +
                                    (size_t)((T + 1) & ~1) * sizeof(uint16_t));
    pl->bp_bytes = (size_t)((T + 15) >> 4) * lw * sizeof(uint32_t);
    pl->bp_lds = pl->lds_fixed + pl->bp_bytes <= 150 * 1024;
    return true;
}

// bytes of workspace a launch over N utterances needs (0: the moves fit in LDS), -1 where there is no plan
template <class Rule>
int64_t align_workspace_bytes(int N, int T, int Smax) {
    AlignPlan pl;
    if (N <= 0 || !align_plan<Rule>(T, Smax, &pl)) return -1;
    return pl.bp_lds ? 0 : (int64_t)N * (int64_t)pl.bp_bytes;
}

// Plans p.T x p.Smax, checks the workspace, fills p.bp_lds / p.bp_global and launches Kernels::get<NT, SPT>() (a
// void (*)(Params)) over p.N workgroups.  The caller has checked its pointers and sizes and filled the rest of p.
template <class Rule, class Kernels, class Params>
int align_launch(Params& p, void* workspace, int64_t workspace_bytes, void* stream) {
    AlignPlan pl;
    W2L_CHECK_ARG(align_plan<Rule>(p.T, p.Smax, &pl), "%s: T=%d (max 32768) or target length %d (max 4095) out of range",
                  Rule::NAME, p.T, p.Smax);
    const int64_t need = pl.bp_lds ? 0 : (int64_t)p.N * (int64_t)pl.bp_bytes;
    W2L_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace), "%s: workspace of %lld bytes, %lld needed", Rule::NAME,
                  (long long)workspace_bytes, (long long)need);
    p.bp_lds = pl.bp_lds;
    p.bp_global = (uint32_t*)workspace;
    const size_t lds = pl.lds_fixed + (pl.bp_lds ? pl.bp_bytes : 0);
    dim3 grid(p.N), block(pl.nt);
#define W2L_ALIGN_LAUNCH(NT, SPT)                                                                       \
    do {                                                                                                \
        void (*const kernel)(Params) = Kernels::template get<NT, SPT>();                                \
        W2L_CHECK_HIP(w2l_allow_big_lds((const void*)kernel));                                          \
        hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, p);                           \
    } while (0)
    static_assert(Rule::MAX_STATES <= Rule::MAX_SPT * 1024, "the plan would ask for a shape the rule does not instantiate");
    if (pl.spt == 1) {
        switch (pl.nt) {
            case 64: W2L_ALIGN_LAUNCH(64, 1); break;
            case 128: W2L_ALIGN_LAUNCH(128, 1); break;
            case 256: W2L_ALIGN_LAUNCH(256, 1); break;
            case 512: W2L_ALIGN_LAUNCH(512, 1); break;
            default: W2L_ALIGN_LAUNCH(1024, 1); break;
        }
    } else if (pl.spt == 2) {
        W2L_ALIGN_LAUNCH(1024, 2);
    } else if (pl.spt == 4) {
        W2L_ALIGN_LAUNCH(1024, 4);
    } else if constexpr (Rule::MAX_SPT >= 8) {
        W2L_ALIGN_LAUNCH(1024, 8);
    }
#undef W2L_ALIGN_LAUNCH
    W2L_CHECK_LAUNCH();
    return 0;
}

}  // namespace

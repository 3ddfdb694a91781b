// Conv1d weight gradient as an MFMA GEMM whose reduction runs over time (gfx950).
//
//   dw[kw][co][ci] (+)= sum_{n,t} dy[n][t][co] * xp[n][t*s + kw*d][ci]
//
// GEMM view per tap kw: M = co, N = ci, K = (n, t).  Both operands are
// channels-last, i.e. the reduction index t is the SLOW axis of both tiles, so
// the MFMA fragments (8 consecutive k per lane) are column reads of the LDS
// images: they are fetched with ds_read_b64_tr_b16, CDNA4's transposing LDS
// read, from row-major [t][channel] tiles that LDS-DMA fills straight from HBM.
// One block owns a [128 co x 128 ci] tile of KWB adjacent taps and a slice of the
// (n,t) range (split-K; partial tiles are combined with fp32 atomics).  The taps
// share the dy tile and read the same staged x window at row offsets tap*d, which
// halves the L2->LDS traffic per FLOP -- the kernel is fabric-bound, not MFMA-bound,
// with one tap per block (11.6 GB of tile reads for an 896x896x29 layer).
//
// Replaces the weight-gradient half of aten::convolution_backward for the
// nn.Conv1d call sites wav2letter.py:35-36,42 / jasper.py:96-105,127.
//
// The host half, top to bottom: WgradProblem (what is asked) -> plan() (pure host arithmetic: which WgradChoice, narrowed to
// what the layer admits, and the launch geometry: a WgradPlan) -> run() (a WgradPlan and the layers' pointers become
// WgradParams) -> launch() (the kernel of the plan, from a table).  Every entry point is a few lines over these.
#include "conv_wgrad_kernel.h"
#include "../../include/w2l_hip.h"
#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace {
using namespace w2l_wgrad;

template <int KWB, bool S1, bool SK, int TG = 1, bool M32 = false>
__global__ __launch_bounds__(256 * TG, TG == 1 ? 2 : 1) void conv_wgrad_kernel(WgradParams p) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    conv_wgrad_body<KWB, S1, SK, TG, M32>(p, smem);
}

}  // namespace

// ---- the three-tap kernel lives in a code object of its own (conv_wgrad3_dev.hip explains why), embedded here as bytes ----
extern "C" const unsigned char w2l_wgrad3_hsaco[];
extern "C" const unsigned int w2l_wgrad3_hsaco_len;

namespace {

// hipFunction_t of w2l_wgrad3_kernel on the calling thread's current device (module loaded once per device)
int wgrad3_function(hipFunction_t* fn, int which /* 0 four waves, 1 two tap groups (eight waves) */) {
    static std::mutex mu;
    static std::map<int, std::array<hipFunction_t, 2>> loaded;
    int dev = 0;
    W2L_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = loaded.find(dev);
    if (it == loaded.end()) {
        hipModule_t mod;
        W2L_CHECK_ARG(w2l_wgrad3_hsaco_len > 0, "conv1d_wgrad: the three-tap code object is missing from this build");
        W2L_CHECK_HIP(hipModuleLoadData(&mod, w2l_wgrad3_hsaco));
        std::array<hipFunction_t, 2> f;
        W2L_CHECK_HIP(hipModuleGetFunction(&f[0], mod, "w2l_wgrad3_kernel"));
        W2L_CHECK_HIP(hipModuleGetFunction(&f[1], mod, "w2l_wgrad3x2_kernel"));
        it = loaded.emplace(dev, f).first;
    }
    *fn = it->second[which];
    return 0;
}

// ---- what is asked, what is chosen, what runs -----------------------------------------------------------------------------
struct WgradProblem {
    int N, Cin, Cout, Tout, Kw, stride, dil;
    bool have_ws;                // the caller handed a workspace ...
    int64_t ws_bytes;            // ... of this many bytes
};

// A plan as it is measured, remembered and forced.  Its packed form -- count | bits << 16, the bits being the `order` value of
// w2l_wgrad_force_plan -- survives where it is ABI or file format: that hook, w2l_wgrad_plan, the `form` of the group calls
// and the "wgrad" lines of the tune file.
constexpr int kBlockOrder = 1;             // bit 0: block order inside a split (1 = tap group fastest)
constexpr int kStreamK = 2;                // bit 1: stream-K decomposition (then the split count is not used)
constexpr int kTapGroups2 = 4;             // bit 2: two tap groups per block (the 8-wave kernel, TG = 2)
constexpr int kMfma32 = 8;                 // bit 3: the 32x32x16 MFMA form (stride 1; not combined with bits 1 and 2)
constexpr int kTaps3 = 16;                 // bit 4: THREE taps per wave, accumulators in AGPRs (conv_wgrad3_dev.hip; stride 1, dilation <= 4)
constexpr int kDealt = 32;                 // bit 5: dealt stream-K (WgradParams::dealt; the count is the range count); needs the
                                           // workspace -- without one the launch falls back to a classic split of 2
constexpr int kAtomicSplit = 64;           // bit 6: a classic split adds its partial tiles atomically even when a workspace is given
constexpr int kOrderMask = 127;
constexpr int kDefaultOrder = kBlockOrder;
constexpr int kTaps3MaxDil = 4;
constexpr int kDealtFallbackSplits = 2;
constexpr int kResidentBlocks = 512;       // 256 CUs x 2 blocks (LDS and registers both allow two)
constexpr size_t kWgradTicketBytes = 64 * 1024;

struct WgradChoice {
    int count = 0;               // the split count, or the range count when dealt; 0 (a forced choice only): not pinned
    bool form_given = true;      // false (a forced choice only): the flags below are not pinned
    bool order = false, streamk = false, tg2 = false, m32 = false, taps3 = false, dealt = false, atomic_ws = false;
    static WgradChoice of(int count, int bits) {
        WgradChoice c;
        c.count = count;
        c.order = bits & kBlockOrder; c.streamk = bits & kStreamK; c.tg2 = bits & kTapGroups2; c.m32 = bits & kMfma32;
        c.taps3 = bits & kTaps3; c.dealt = bits & kDealt; c.atomic_ws = bits & kAtomicSplit;
        return c;
    }
    int bits() const {
        return (order ? kBlockOrder : 0) | (streamk ? kStreamK : 0) | (tg2 ? kTapGroups2 : 0) | (m32 ? kMfma32 : 0) |
               (taps3 ? kTaps3 : 0) | (dealt ? kDealt : 0) | (atomic_ws ? kAtomicSplit : 0);
    }
    static WgradChoice unpack(int packed) { return of(packed & 0xffff, packed >> 16); }
    int pack() const { return count | (bits() << 16); }
};

struct DealtPerm { int nb; std::vector<unsigned short> perm; };

// Everything a launch needs that is not a pointer.
struct WgradPlan {
    WgradProblem pr;
    WgradChoice choice;          // as forced, remembered or priced -- before the narrowing below (w2l_wgrad_plan reports it)
    int splits, steps_per_split, tsteps, total_steps;
    bool order, streamk, tg2, m32, taps3;        // the form that runs
    int kwb, kwblk, kgroups, tiles;              // taps per wave, taps per block, tap groups of the layer, tiles of the launch
    int G, dealt_b;              // G > 0: the dealt stream-K path with G ranges and dealt_b second-segment blocks
    const DealtPerm* perm;
    bool slabs, atomic;
    bool needs_zero;             // the launch ADDS into dw (atomics): the caller must hand it a zero-filled (or accumulated) dw
    int xrows_lds;
    size_t lds;
    unsigned grid_x, grid_y, threads;
};

// measured choices (w2l_conv1d_wgrad_tune) per shape.  The key has no stride and no dilation: that is why plan() narrows.
typedef std::tuple<int, int, int, int, int> WShapeKey;
std::map<WShapeKey, WgradChoice> g_wtuned;
std::mutex g_wtuned_mu;
// storage of the w2l_wgrad_force_plan hook, per calling thread like g_force_cfg of the implicit GEMM; read by hooked() alone
thread_local int g_force_splits = 0;
thread_local int g_force_order = -1;
// w2l_wgrad_deterministic(1): plans that add their partial tiles with fp32 atomics although a workspace is at hand (bit 6) lose
// that bit when planned -- a plan cache written by a default-mode run must not switch atomics back on in a run that asked
// for bit-reproducible gradients.  Process-wide (the weight gradients are launched from autograd's worker thread).
std::atomic<int> g_deterministic{0};

WgradChoice forced_choice(int splits, int order) {     // 0 / -1: automatic
    WgradChoice f = WgradChoice::of(splits > 0 ? splits : 0, order >= 0 ? (order & kOrderMask) : 0);
    f.form_given = order >= 0;
    return f;
}
WgradChoice hooked() { return forced_choice(g_force_splits, g_force_order); }

// ---- dealt stream-K: the second-segment blocks of a launch, longest first (WgradParams::dealt_perm); cached per geometry: 21
// launches per step must not sort 512 ranges each
std::map<std::tuple<int, int, int>, DealtPerm> g_dealt_perms;
std::mutex g_dealt_mu;

bool dealt_geometry_ok(int tiles, int S, int G) {
    if (G < 1 || G > W2L_WGRAD_MAX_RANGES || tiles < 1 || tiles > G) return false;
    const int64_t W = (int64_t)tiles * S;
    return W >= G && W * (G + 2) < (1LL << 31);
}

// nullptr: this geometry has no dealt form
const DealtPerm* dealt_perm(int tiles, int S, int G) {
    if (!dealt_geometry_ok(tiles, S, G)) return nullptr;
    std::lock_guard<std::mutex> lock(g_dealt_mu);
    auto key = std::make_tuple(tiles, S, G);
    auto it = g_dealt_perms.find(key);
    if (it == g_dealt_perms.end()) {
        // Blocks are dealt round-robin to the 8 XCDs, so block G + j runs where blocks j % 8 ran: the first-segment blocks of
        // XCD x own the consecutive ranges xcd_remap gives them, and the second segments of THOSE ranges (the next tiles
        // along: same dy tiles and x windows in that XCD's L2) are dealt to the same XCD, longest first -- position j of the
        // list holds the (j / 8)-th longest second segment of XCD j % 8's ranges, 0xffff where that XCD has no more.
        std::vector<std::pair<int, int>> second[8];        // per XCD: (-steps, range)
        const int q = G >> 3, rem = G & 7;
        size_t longest = 0;
        for (int x = 0; x < 8; ++x) {
            const int base = x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q, cnt = x < rem ? q + 1 : q;
            for (int r = base; r < base + cnt; ++r) {
                const DealtSeg sg = dealt_segment((unsigned)tiles, (unsigned)S, (unsigned)G, (unsigned)r, true);
                if (sg.w_end > sg.w) second[x].emplace_back(-(sg.w_end - sg.w), r);
            }
            std::sort(second[x].begin(), second[x].end());
            longest = std::max(longest, second[x].size());
        }
        DealtPerm dp;
        for (size_t i = 0; i < longest; ++i)
            for (int x = 0; x < 8; ++x) dp.perm.push_back(i < second[x].size() ? (unsigned short)second[x][i].second : (unsigned short)0xffff);
        while (!dp.perm.empty() && dp.perm.back() == 0xffff) dp.perm.pop_back();
        dp.nb = (int)dp.perm.size();
        if (dp.nb > W2L_WGRAD_MAX_RANGES) return nullptr;
        it = g_dealt_perms.emplace(key, std::move(dp)).first;
    }
    return &it->second;         // (map nodes never move and are never erased)
}

size_t dealt_ws_need(int tiles, int kwblk, int G) {
    return kWgradTicketBytes + (size_t)(G + tiles) * kwblk * BM * BNC * sizeof(float);
}

int tiles_mn(int Cin, int Cout) { return ((Cout + BM - 1) / BM) * ((Cin + BNC - 1) / BNC); }

// slabs of one launch: tiles x splits x (taps per block) x 128 x 128 floats; the tap count rounds up to the block's tap
// group, so the 4-tap form can need a little more than the 2-tap form: the need is the larger of the two
size_t wgrad_ws_need(int Cin, int Cout, int Kw, int splits) {
    size_t taps = 1;
    if (Kw > 1) {
        // (2, 4, 3 and 6 taps per block: the two-tap kernel, its two-tap-group form, the three-tap kernel and its two-tap-group form)
        const size_t t2 = (size_t)((Kw + 1) / 2) * 2, t4 = (size_t)((Kw + 3) / 4) * 4, t3 = (size_t)((Kw + 2) / 3) * 3;
        const size_t t6 = (size_t)((Kw + 5) / 6) * 6;
        taps = std::max(std::max(t2, t4), std::max(t3, t6));
    }
    return kWgradTicketBytes + (size_t)tiles_mn(Cin, Cout) * taps * splits * BM * BNC * sizeof(float);
}

// taps per wave and per block of the form in pl.taps3 / pl.tg2, the x window they stage and the block that runs them
// (`wide`: the launch has layers of more than one tap)
void block_form(WgradPlan& pl, bool wide, int stride, int dil) {
    pl.kwb = pl.taps3 ? 3 : (wide ? KWB_DEFAULT : 1);
    pl.kwblk = pl.tg2 ? 2 * pl.kwb : pl.kwb;
    const int xr = (BT - 1) * stride + (pl.kwblk - 1) * dil + 1;
    pl.xrows_lds = (xr + 3) & ~3;
    pl.lds = 2 * BT * ROWB + 2 * (size_t)pl.xrows_lds * ROWB;
    pl.threads = pl.tg2 ? 512 : 256;
}

// Split the (n,t) reduction over `splits` blocks per tile so that the grid fills whole rounds of the
// 512 resident blocks (256 CUs x 2): cost = rounds x steps-per-block (+ the fp32 atomic traffic of the
// extra partial tiles, ~1.3 TB/s chip-wide).  Non-power-of-two splits are allowed.
int cost_model_splits(const WgradProblem& pr, int total) {
    const int kwb = pr.Kw > 1 ? KWB_DEFAULT : 1;
    const int tiles = tiles_mn(pr.Cin, pr.Cout) * ((pr.Kw + kwb - 1) / kwb);
    const double t_step_us = 2.7 * kwb / 2.0;                                // one 64-row K step of a block sharing its CU
    const double out_us = (double)pr.Cout * pr.Cin * pr.Kw * 4.0 / 1.3e6;    // one full pass of fp32 atomics over dw
    int best = 1;
    double best_cost = 1e30;
    for (int s = 1; s <= 32 && s <= total; ++s) {
        const int steps = (total + s - 1) / s;
        if (s > 1 && steps < 4) break;
        const long blocks = (long)tiles * s;
        const long rounds = (blocks + 511) / 512;
        double per_step = t_step_us * (blocks <= 256 ? 0.6 : 1.0);  // a block alone on its CU runs faster
        double cost = rounds * steps * per_step + (s > 1 ? 0.5 * out_us * s : 0.0);
        if (cost < best_cost * 0.97) { best_cost = cost; best = s; }
    }
    // (the stream-K decomposition is a candidate of the measured selection only: its kernel carries ~10 % more instructions
    // per K step -- the segment loop's live scalars -- and beat the best split-K plan on one shape of the Wav2Letter table)
    return best;
}

// What a launch of this problem runs as.  Pure host arithmetic (no HIP call): shared by the launcher, the tuner and every
// query.  The checks that need the geometry come last, so a refused launch still leaves what had been decided in *out.
int plan(const WgradProblem& pr, const WgradChoice* forced, WgradPlan* out) {
    WgradPlan& pl = *out;
    pl = WgradPlan{};
    pl.pr = pr;
    W2L_CHECK_ARG(pr.N > 0 && pr.Tout > 0 && pr.Kw > 0 && pr.stride > 0 && pr.dil > 0, "conv1d_wgrad: bad sizes");
    W2L_CHECK_ARG(pr.Cin % 64 == 0 && pr.Cout % 64 == 0 && pr.Cin > 0 && pr.Cout > 0,
                  "conv1d_wgrad: channels (%d,%d) must be positive multiples of 64", pr.Cin, pr.Cout);
    pl.tsteps = (pr.Tout + BT - 1) / BT;
    const int total = pl.total_steps = pr.N * pl.tsteps;

    // ---- the choice: what is forced, else what was measured for the shape, else the cost model's split in the default order
    WgradChoice c = WgradChoice::of(0, forced && forced->form_given ? forced->bits() : kDefaultOrder);
    if (forced && forced->count > 0) {      // (a dealt plan's count is its range count: not bounded by the step count)
        c.count = c.dealt || forced->count <= total ? forced->count : total;
    } else {
        std::unique_lock<std::mutex> lock(g_wtuned_mu);
        auto it = g_wtuned.find(WShapeKey(pr.N, pr.Cin, pr.Cout, pr.Tout, pr.Kw));
        if (it != g_wtuned.end()) {
            const int bits = forced && forced->form_given ? c.bits() : it->second.bits();
            c = WgradChoice::of(it->second.count, bits);
        } else {
            lock.unlock();
            c.count = cost_model_splits(pr, total);
        }
    }
    pl.choice = c;
    if (g_deterministic.load(std::memory_order_relaxed)) c.atomic_ws = false;

    // ---- narrowed to what the layer's stride / dilation / tap count admit and to the workspace at hand
    int splits = c.count, G = 0;
    if (c.dealt && !c.streamk) { G = c.count; splits = kDealtFallbackSplits; }
    if (splits > total) splits = total;
    // (only split counts whose ranges are all non-empty: ceil(total / s) steps each leave ceil(total / that) ranges -- 32 asked of
    // 40 steps are 20 ranges of 2; an empty range would start in the NEXT tile and draw that tile's ticket)
    if (splits > 1) splits = (total + (total + splits - 1) / splits - 1) / ((total + splits - 1) / splits);
    // stream-K is the atomic path's alternative to split-K: with a workspace (deterministic slabs) the classic plan runs,
    // unless the plan says that it adds atomically whatever it is given (bit 6)
    pl.streamk = c.streamk && (!pr.have_ws || c.atomic_ws);
    if (pl.streamk) splits = 1;
    // (with stream-K: 256 persistent 8-wave blocks, one per CU -- built for stride 1 only; the plan cache is keyed without the
    // stride, so a plan measured on a stride-1 layer may reach a strided one: that launch falls back to the 4-wave stream-K kernel)
    pl.tg2 = c.tg2 && pr.Kw > 2 && !(pl.streamk && pr.stride != 1);
    // the 32x32x16 form is built for stride 1, classic split-K, one tap group
    pl.m32 = c.m32 && !pl.streamk && !pl.tg2 && pr.stride == 1;
    // three taps per block (conv_wgrad3_dev.hip): a plan measured on a layer that admits it may reach one that does not
    // (the plan cache is keyed without stride and dilation): such a launch takes the two-tap kernel
    pl.taps3 = c.taps3 && !c.m32 && !pl.streamk && pr.stride == 1 && pr.dil <= kTaps3MaxDil && pr.Kw >= 3;
    pl.order = c.order;
    block_form(pl, pr.Kw > 1, pr.stride, pr.dil);
    pl.kgroups = (pr.Kw + pl.kwblk - 1) / pl.kwblk;
    pl.tiles = tiles_mn(pr.Cin, pr.Cout) * pl.kgroups;
    const size_t ws_bytes = pr.have_ws && pr.ws_bytes > 0 ? (size_t)pr.ws_bytes : 0;
    const bool tickets_fit = (size_t)pl.tiles * sizeof(unsigned) <= kWgradTicketBytes;
    // the dealt path needs its geometry and its workspace; without either the launch is the fallback split
    if (G > 0 && !pl.streamk && pr.have_ws && dealt_geometry_ok(pl.tiles, total, G) && dealt_ws_need(pl.tiles, pl.kwblk, G) <= ws_bytes &&
        tickets_fit) {
        pl.G = G;
        splits = 1;
    }
    // a split reduces through slabs where the workspace holds them (and the plan does not ask for atomics), else atomically
    pl.slabs = pl.G > 0 || (splits > 1 && pr.have_ws && !c.atomic_ws && tickets_fit && wgrad_ws_need(pr.Cin, pr.Cout, pr.Kw, splits) <= ws_bytes);
    pl.atomic = splits > 1 && !pl.slabs;
    pl.needs_zero = pl.atomic || pl.streamk;
    pl.splits = splits;
    pl.steps_per_split = (total + splits - 1) / splits;

    // ---- the grid
    W2L_CHECK_ARG(pl.lds <= 160 * 1024, "conv1d_wgrad: stride %d / dilation %d need %zu bytes of LDS", pr.stride, pr.dil, pl.lds);
    pl.grid_x = pl.tiles;
    pl.grid_y = splits;
    if (pl.G > 0) {
        pl.perm = dealt_perm(pl.tiles, total, pl.G);
        W2L_CHECK_ARG(pl.perm != nullptr, "conv1d_wgrad: no dealt form for %d tiles x %d steps on %d ranges", pl.tiles, total, pl.G);
        pl.dealt_b = pl.perm->nb;
        pl.grid_x = (unsigned)(pl.G + pl.dealt_b);
        pl.grid_y = 1;
    }
    if (pl.streamk) {
        // one block per resident slot, but at least ~16 K steps each (short ranges are all prologue and epilogue)
        const int64_t W = (int64_t)pl.tiles * total;
        W2L_CHECK_ARG(W < (1LL << 31), "conv1d_wgrad: (tile, step) space exceeds 32 bits");
        const int64_t resident = pl.tg2 ? kResidentBlocks / 2 : kResidentBlocks;
        pl.grid_x = (unsigned)std::max<int64_t>(1, std::min(W / 16, resident));
        pl.grid_y = 1;
    }
    return 0;
}

// the plan the calling thread's launch of this problem takes, its w2l_wgrad_force_plan hook included (a refused launch: what
// plan() had decided by then, which is what these queries always answered)
WgradPlan hooked_plan(int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int64_t ws_bytes) {
    const WgradChoice f = hooked();
    WgradPlan pl;
    (void)plan(WgradProblem{N, Cin, Cout, Tout, Kw, stride, dil, ws_bytes > 0, ws_bytes}, &f, &pl);
    return pl;
}

// ---- the kernel of a plan: (taps per wave, stride-1 specialisation, stream-K, tap groups per block, 32x32x16 fragments)
struct WgradKernelRow {
    int kwb;
    bool s1, sk;
    int tg;
    bool m32;
    void (*fn)(WgradParams);     // nullptr: function `hsaco` of the embedded three-tap code object (AGPR accumulators)
    int hsaco;
    std::atomic<bool> big_lds{false};
};
WgradKernelRow g_kernels[] = {       // (in the order the kernels have always been instantiated in: the code object's layout)
    {3, true, false, 1, true, nullptr, 0},
    {3, true, false, 2, true, nullptr, 1},
    {2, true, false, 1, true, conv_wgrad_kernel<2, true, false, 1, true>, 0},
    {1, true, false, 1, true, conv_wgrad_kernel<1, true, false, 1, true>, 0},
    {2, true, true, 2, false, conv_wgrad_kernel<2, true, true, 2>, 0},
    {2, true, false, 2, false, conv_wgrad_kernel<2, true, false, 2>, 0},
    {2, false, false, 2, false, conv_wgrad_kernel<2, false, false, 2>, 0},
    {2, true, true, 1, false, conv_wgrad_kernel<2, true, true>, 0},
    {2, false, true, 1, false, conv_wgrad_kernel<2, false, true>, 0},
    {1, true, true, 1, false, conv_wgrad_kernel<1, true, true>, 0},
    {1, false, true, 1, false, conv_wgrad_kernel<1, false, true>, 0},
    {2, true, false, 1, false, conv_wgrad_kernel<2, true, false>, 0},
    {2, false, false, 1, false, conv_wgrad_kernel<2, false, false>, 0},
    {1, true, false, 1, false, conv_wgrad_kernel<1, true, false>, 0},
    {1, false, false, 1, false, conv_wgrad_kernel<1, false, false>, 0},
};

int launch(const WgradPlan& pl, const WgradParams& p, void* stream) {
    const int tg = pl.tg2 ? 2 : 1;
    const bool s1 = p.stride == 1, m32 = pl.m32 || pl.taps3;
    WgradKernelRow* row = nullptr;
    for (WgradKernelRow& r : g_kernels)
        if (r.kwb == pl.kwb && r.s1 == s1 && r.sk == pl.streamk && r.tg == tg && r.m32 == m32) row = &r;
    W2L_CHECK_ARG(row != nullptr, "conv1d_wgrad: no kernel of %d taps per wave, stride %d, stream-K %d, %d tap groups, 32x32x16 %d",
                  pl.kwb, p.stride, (int)pl.streamk, tg, (int)m32);
    if (row->fn == nullptr) {
        hipFunction_t fn;
        if (int e = wgrad3_function(&fn, row->hsaco)) return e;
        W2L_CHECK_ARG(pl.lds <= 2 * BT * ROWB + 2 * (size_t)(pl.tg2 ? 88 : 72) * ROWB, "conv1d_wgrad: the three-tap kernel's LDS window is too small");
        void* args[] = {const_cast<WgradParams*>(&p)};
        W2L_CHECK_HIP(hipModuleLaunchKernel(fn, pl.grid_x, pl.grid_y, 1, pl.threads, 1, 1, 0, (hipStream_t)stream, args, nullptr));
    } else {
        // experiment switch: W2L_WGRAD_LDS_PAD=<bytes> of unused dynamic LDS per block of the two-tap kernels -- with > 40 KB only ONE
        // four-wave block fits a CU, which leaves half its register file to the main stream's kernels
        static const size_t lds_pad = getenv("W2L_WGRAD_LDS_PAD") ? (size_t)atoll(getenv("W2L_WGRAD_LDS_PAD")) : 0;
        const size_t lds = pl.lds + lds_pad <= 160 * 1024 ? pl.lds + lds_pad : pl.lds;
        if (!row->big_lds.load(std::memory_order_relaxed)) {
            W2L_CHECK_HIP(w2l_allow_big_lds((const void*)row->fn));
            row->big_lds.store(true, std::memory_order_relaxed);
        }
        hipLaunchKernelGGL(row->fn, dim3(pl.grid_x, pl.grid_y), dim3(pl.threads), lds, (hipStream_t)stream, p);
    }
    W2L_CHECK_LAUNCH();
    return 0;
}

// One layer of a launch from its operands: the checks every entry point makes, and the layer's place in the tile pool.
// pr: the launch's N, Tout, stride and dilation (what the operands must cover); who / li: the entry point's name and the layer's
// index for the messages (li < 0: a single-layer launch)
int fill_layer(WgradLayer& l, const w2l_wgrad_item_t& it, const WgradProblem& pr, int kwblk, int tile0, const char* who, int li) {
    char where[24] = "";
    if (li >= 0) snprintf(where, sizeof(where), " (layer %d)", li);
    W2L_CHECK_ARG(it.dy && it.xp && it.dw, "%s: null pointer%s", who, where);
    W2L_CHECK_ARG(it.Cin % 64 == 0 && it.Cout % 64 == 0 && it.Cin > 0 && it.Cout > 0 && it.Kw > 0,
                  "%s: channels (%d,%d) must be positive multiples of 64", who, it.Cin, it.Cout);
    W2L_CHECK_ARG(it.dy_bstride % it.Cout == 0 && it.x_bstride % it.Cin == 0, "%s: batch strides must be whole rows", who);
    W2L_CHECK_ARG(it.x_rows_total * (int64_t)it.Cin * 2 < (1LL << 32), "%s: activation buffer exceeds 32-bit byte offsets", who);
    // (the kernel clamps its x window onto row x_rows_total - 1 and reads 64-row steps of dy: a buffer that is short of a LIVE row
    // would be clamped onto its last row and give a wrong gradient without a word)
    W2L_CHECK_ARG(it.dy_bstride / it.Cout >= pr.Tout, "%s: dy_bstride holds %lld rows per utterance, Tout=%d needs as many%s", who,
                  (long long)(it.dy_bstride / it.Cout), pr.Tout, where);
    const int64_t x_need = (int64_t)(pr.N - 1) * (it.x_bstride / it.Cin) + (int64_t)(pr.Tout - 1) * pr.stride + (int64_t)(it.Kw - 1) * pr.dil + 1;
    W2L_CHECK_ARG(it.x_rows_total >= x_need, "%s: padded input too small: x_rows_total=%lld, the last utterance's last tap reads row %lld%s",
                  who, (long long)it.x_rows_total, (long long)(x_need - 1), where);
    l.dy = (const bf16_raw*)it.dy;
    l.x = (const bf16_raw*)it.xp;
    l.dw = it.dw;
    l.dy_rows_per_utt = it.dy_bstride / it.Cout;
    l.x_rows_per_utt = it.x_bstride / it.Cin;
    l.x_max_row = it.x_rows_total - 1;
    l.Cin = it.Cin; l.Cout = it.Cout; l.Kw = it.Kw;
    l.tiles_m = (it.Cout + BM - 1) / BM;
    l.tiles_n = (it.Cin + BNC - 1) / BNC;
    l.kgroups = (it.Kw + kwblk - 1) / kwblk;
    l.tile0 = tile0;
    return 0;
}

// p.layers, p.nlayers and p.accumulate are the caller's; the plan fills in the rest
int run(const WgradPlan& pl, WgradParams& p, void* ws, void* stream) {
    p.tiles_total = pl.tiles;
    p.N = pl.pr.N; p.Tout = pl.pr.Tout; p.stride = pl.pr.stride; p.dil = pl.pr.dil;
    p.tsteps = pl.tsteps;
    p.total_steps = pl.total_steps;
    p.steps_per_split = pl.steps_per_split;
    p.splits = pl.splits;
    p.atomic = pl.atomic;
    p.order = pl.order;
    p.streamk = pl.streamk;
    p.xrows_lds = pl.xrows_lds;
    p.tickets = pl.slabs ? (unsigned*)ws : nullptr;
    p.slabs = pl.slabs ? (float*)((char*)ws + kWgradTicketBytes) : nullptr;
    p.dealt = pl.G;
    p.dealt_b = pl.dealt_b;
    if (pl.G > 0) std::copy(pl.perm->perm.begin(), pl.perm->perm.end(), p.dealt_perm);
    return launch(pl, p, stream);
}

int run_layer(const WgradPlan& pl, const w2l_wgrad_item_t& it, int accumulate, void* ws, void* stream) {
    WgradParams p;
    p.nlayers = 1;
    if (int rc = fill_layer(p.layers[0], it, pl.pr, pl.kwblk, 0, "conv1d_wgrad", -1)) return rc;
    p.accumulate = accumulate;
    return run(pl, p, ws, stream);
}

}  // namespace

extern "C" void w2l_wgrad_deterministic(int on) { g_deterministic.store(on ? 1 : 0, std::memory_order_relaxed); }

// testing / profiling hook: pin the split count (0 = automatic) and the plan's form bits (-1 = automatic; kBlockOrder ..)
extern "C" void w2l_wgrad_force_plan(int splits, int order) {
    g_force_splits = splits > 0 ? splits : 0;
    g_force_order = order >= 0 ? (order & kOrderMask) : -1;
}

// the plan a launch of this problem will take: its order bits (see w2l_wgrad_force_plan) | split or range count << 8
extern "C" int w2l_wgrad_plan(int N, int Cin, int Cout, int Tout, int Kw) {
    const WgradChoice c = hooked_plan(N, Cin, Cout, Tout, Kw, 1, 1, 0).choice;
    return (c.bits() & 0xff) | (c.count << 8);
}

// the fields of the WgradPlan a launch of this problem takes, in the order of the struct (w2l_hip.h lists them); forcing is an
// argument here (0 / -1: automatic), the per-thread hook is neither read nor touched
extern "C" int w2l_wgrad_launch_plan(int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int64_t ws_bytes,
                                     int forced_splits, int forced_order, int* out) {
    const WgradChoice f = forced_choice(forced_splits, forced_order);
    WgradPlan pl;
    for (int i = 0; i < W2L_WGRAD_PLAN_FIELDS; ++i) out[i] = 0;
    if (int rc = plan(WgradProblem{N, Cin, Cout, Tout, Kw, stride, dil, ws_bytes > 0, ws_bytes}, &f, &pl)) return rc;
    const int v[W2L_WGRAD_PLAN_FIELDS] = {pl.splits, pl.steps_per_split, pl.tsteps, pl.total_steps, pl.order, pl.streamk, pl.tg2, pl.m32,
                                          pl.taps3, pl.kwb, pl.kwblk, pl.kgroups, pl.tiles, pl.G, pl.dealt_b, pl.slabs, pl.atomic,
                                          pl.needs_zero, pl.xrows_lds, (int)pl.lds, (int)pl.grid_x, (int)pl.grid_y, (int)pl.threads, 1};
    std::copy(v, v + W2L_WGRAD_PLAN_FIELDS, out);
    return 0;
}

// must dw be zero-filled (or hold an accumulated gradient) for this launch?  _x is the general query; _ws assumes a stride-1,
// dilation-1 layer, the plain one no workspace as well
extern "C" int w2l_wgrad_needs_zero_x(int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int64_t ws_bytes) {
    return hooked_plan(N, Cin, Cout, Tout, Kw, stride, dil, ws_bytes).needs_zero ? 1 : 0;
}

extern "C" int w2l_wgrad_needs_zero_ws(int N, int Cin, int Cout, int Tout, int Kw, int64_t ws_bytes) {
    return w2l_wgrad_needs_zero_x(N, Cin, Cout, Tout, Kw, 1, 1, ws_bytes);
}

extern "C" int w2l_wgrad_needs_zero(int N, int Cin, int Cout, int Tout, int Kw) {
    const WgradPlan pl = hooked_plan(N, Cin, Cout, Tout, Kw, 1, 1, 0);
    // (a dealt plan always answered 1 here, also where its fallback split clamps to the problem's single step and adds nothing)
    return pl.needs_zero || (pl.choice.dealt && !pl.choice.streamk) ? 1 : 0;
}

extern "C" int64_t w2l_wgrad_workspace_bytes(int Cin, int Cout, int Kw) {
    return (int64_t)wgrad_ws_need(Cin, Cout, Kw, 32);      // 32 = the largest split count the tuner tries
}

// the largest workspace a dealt plan of this layer can ask for: over the block forms (2 / 3 taps per 4-wave block on 512
// or 256 ranges, 4 / 6 taps per 8-wave block on 256 ranges) that have one (tiles <= ranges)
extern "C" int64_t w2l_wgrad_dealt_workspace_bytes(int Cin, int Cout, int Kw) {
    size_t need = 0;
    const int forms[4][2] = {{2, kResidentBlocks}, {3, kResidentBlocks}, {4, kResidentBlocks / 2}, {6, kResidentBlocks / 2}};
    for (const auto& f : forms) {
        const int kwblk = Kw > 1 ? f[0] : 1, tiles = tiles_mn(Cin, Cout) * ((Kw + kwblk - 1) / kwblk);
        if (tiles <= f[1]) need = std::max(need, dealt_ws_need(tiles, kwblk, f[1]));
    }
    return (int64_t)need;
}

// test hook (host only): the blocks of a dealt launch in launch order, six ints each -- range, tile, first step, end step,
// place among the tile's segments, number of the tile's segments; returns the block count, -1 if the geometry has no dealt form
extern "C" int w2l_wgrad_dealt_segments(int tiles, int S, int G, int* out, int max_blocks) {
    const DealtPerm* dp = dealt_perm(tiles, S, G);
    if (dp == nullptr) return -1;
    const int nblk = G + dp->nb;
    for (int b = 0; b < nblk && b < max_blocks; ++b) {
        const bool second = b >= G;
        const int q = G >> 3, rem = G & 7, xcd = b & 7;          // xcd_remap, host side
        const int r = second ? dp->perm[b - G] : (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (b >> 3);
        int* o = out + 6 * b;
        if (r == 0xffff) {                                       // a padding position of the per-XCD deal: the block exits at once
            o[0] = -1; o[1] = o[2] = o[3] = o[4] = o[5] = 0;
            continue;
        }
        const DealtSeg sg = dealt_segment((unsigned)tiles, (unsigned)S, (unsigned)G, (unsigned)r, second);
        const int t = sg.w / S;
        o[0] = r; o[1] = t; o[2] = sg.w - t * S; o[3] = sg.w_end - t * S; o[4] = sg.split; o[5] = sg.nsplit;
    }
    return nblk;
}

extern "C" int w2l_conv1d_wgrad_ws(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride,
                                   int64_t x_rows_total, float* dw, int N, int Cin, int Cout, int Tout, int Kw,
                                   int stride, int dil, int accumulate, void* ws, int64_t ws_bytes, void* stream) {
    const WgradChoice f = hooked();
    WgradPlan pl;
    if (int rc = plan(WgradProblem{N, Cin, Cout, Tout, Kw, stride, dil, ws != nullptr, ws_bytes}, &f, &pl)) return rc;
    return run_layer(pl, w2l_wgrad_item_t{dy, dy_bstride, xp, x_bstride, x_rows_total, dw, Cin, Cout, Kw, 0}, accumulate, ws, stream);
}

extern "C" int w2l_conv1d_wgrad(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride,
                                int64_t x_rows_total, float* dw, int N, int Cin, int Cout, int Tout, int Kw,
                                int stride, int dil, int accumulate, void* stream) {
    return w2l_conv1d_wgrad_ws(dy, dy_bstride, xp, x_bstride, x_rows_total, dw, N, Cin, Cout, Tout, Kw, stride, dil, accumulate, nullptr, 0, stream);
}

// ---- a GROUP of layers in one launch (WgradLayer): their tiles are one pool of equal-shaped work items.  Plain stores, one
// block per tile (no split: a group exists to fill the chip without one), no workspace, stride 1.  form: plan bits 0 (block
// order inside a layer), 2 (two tap groups per 8-wave block), 3 (32x32x16 fragments), 4 (three taps per wave, AGPR accumulators).
static WgradPlan group_form(int form, bool wide, int dil) {
    const WgradChoice c = WgradChoice::of(1, form);
    WgradPlan pl{};
    pl.order = c.order; pl.tg2 = c.tg2; pl.taps3 = c.taps3;
    pl.m32 = c.m32 && !c.taps3 && !c.tg2;
    block_form(pl, wide, 1, dil);
    return pl;
}

extern "C" int w2l_wgrad_group_tiles(int Cin, int Cout, int Kw, int form) {
    const int kwblk = group_form(form, Kw > 1, 1).kwblk;
    return tiles_mn(Cin, Cout) * ((Kw + kwblk - 1) / kwblk);
}

extern "C" int w2l_conv1d_wgrad_group(const w2l_wgrad_item_t* items, int nitems, int N, int Tout, int dil, int form, void* stream) {
    W2L_CHECK_ARG(items && nitems >= 1 && nitems <= W2L_WGRAD_MAX_LAYERS, "conv1d_wgrad_group: 1..%d layers", W2L_WGRAD_MAX_LAYERS);
    W2L_CHECK_ARG(N > 0 && Tout > 0 && dil > 0, "conv1d_wgrad_group: bad sizes");
    W2L_CHECK_ARG(!(form & (kStreamK | kDealt | kAtomicSplit)), "conv1d_wgrad_group: block forms only (order bits 0, 2, 3, 4)");
    WgradPlan pl = group_form(form, true, dil);         // (the kernel of a group is the wide one whatever its layers' tap counts)
    W2L_CHECK_ARG(!pl.taps3 || dil <= kTaps3MaxDil, "conv1d_wgrad_group: the three-tap form takes dilation <= %d", kTaps3MaxDil);
    WgradParams p;
    pl.pr = WgradProblem{N, 0, 0, Tout, 0, 1, dil, false, 0};
    for (int i = 0; i < nitems; ++i) {
        if (int rc = fill_layer(p.layers[i], items[i], pl.pr, pl.kwblk, pl.tiles, "conv1d_wgrad_group", i)) return rc;
        pl.tiles += p.layers[i].tiles_m * p.layers[i].tiles_n * p.layers[i].kgroups;
    }
    p.nlayers = nitems;
    p.accumulate = 0;
    pl.tsteps = (Tout + BT - 1) / BT;
    pl.total_steps = pl.steps_per_split = N * pl.tsteps;
    pl.splits = 1;
    W2L_CHECK_ARG((int64_t)pl.tiles * pl.total_steps < (1LL << 31), "conv1d_wgrad_group: (tile, step) space exceeds 32 bits");
    W2L_CHECK_ARG(pl.lds <= 160 * 1024, "conv1d_wgrad_group: dilation %d needs %zu bytes of LDS", dil, pl.lds);
    pl.grid_x = pl.tiles;
    pl.grid_y = 1;
    return run(pl, p, nullptr, stream);
}

// Measure candidate plans for this problem on the caller's device and remember the fastest (SYNCHRONISING; warm-up only).
// `dw_scratch` is a throw-away [Kw][Cout][Cin] fp32 buffer.
// flags bit 0: classic split plans are measured (and will run) with fp32 atomics although a workspace is given -- the
// workspace then only serves the dealt stream-K plans (the default mode of the step engine; without the bit every split
// reduction goes through slabs: W2L_DETERMINISTIC=1)
extern "C" int w2l_conv1d_wgrad_tune_x(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride,
                                       int64_t x_rows_total, float* dw_scratch, int N, int Cin, int Cout, int Tout, int Kw,
                                       int stride, int dil, int reps, void* ws, int64_t ws_bytes, int flags, void* stream) {
    const WShapeKey key(N, Cin, Cout, Tout, Kw);
    {
        std::lock_guard<std::mutex> lock(g_wtuned_mu);
        if (g_wtuned.count(key)) return 0;
    }
    W2lEventPair ev;
    if (int rc = ev.create()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const WgradProblem pr{N, Cin, Cout, Tout, Kw, stride, dil, ws != nullptr, ws_bytes};
    const w2l_wgrad_item_t item{dy, dy_bstride, xp, x_bstride, x_rows_total, dw_scratch, Cin, Cout, Kw, 0};
    const int total = N * ((Tout + BT - 1) / BT);
    const int cands[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 24, 32};
    if (ws) (void)hipMemsetAsync(ws, 0, kWgradTicketBytes, st);
    if (reps < 1) reps = 1;
    const size_t bytes = (size_t)Kw * Cout * Cin * sizeof(float);
    const int ncand = 2 * (int)(sizeof(cands) / sizeof(cands[0]));
    // time `n` back-to-back launches of plan c after one warm-up launch (which also validates it); < 0: it did not run
    auto time_plan = [&](const WgradChoice& c, int n) -> float {
        WgradPlan pl;
        if (plan(pr, &c, &pl) != 0) return -1.f;
        if (c.dealt && pl.G == 0) return -1.f;                   // this form has no dealt geometry here: the launch would be its fallback
        const bool zero = pl.needs_zero;                         // atomics need a zero-filled dw
        if (zero) (void)hipMemsetAsync(dw_scratch, 0, bytes, st);
        if (run_layer(pl, item, 0, ws, stream) != 0) return -1.f;
        (void)hipEventRecord(ev.e0, st);
        for (int r = 0; r < n; ++r) {
            if (zero) (void)hipMemsetAsync(dw_scratch, 0, bytes, st);       // that fill is part of the launch's cost
            run_layer(pl, item, 0, ws, stream);
        }
        (void)hipEventRecord(ev.e1, st);
        if (hipEventSynchronize(ev.e1) != hipSuccess) return -1.f;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess) return -1.f;
        // Plans that ADD their partial tiles with fp32 atomics are priced above their stand-alone time: back to back, the next
        // launch's zero fill runs under this launch's tail (in the step it is one more dependent launch in front of its kernel:
        // 8-9 us), and beside the data gradients of the step the atomics themselves run slower than alone -- 768 -> 896 at split 3
        // measured level with the unsplit six-tap form alone (picked in two of five selections) and cost the step +0.09 ms = 17 %
        // of that layer (tools/probe/plan_cmp.sh).  The narrow layers' split plans win by 30-100 % and are not affected.
        if (zero) ms = ms * 1.08f + 0.008f * n;
        return ms;
    };
    std::vector<std::pair<float, WgradChoice>> timed;
    auto try_plan = [&](const WgradChoice& c) {
        const float ms = time_plan(c, reps);
        if (ms >= 0.f) timed.emplace_back(ms, c);
    };
    // (a stream-K form of the three-tap kernel was built and measured 10-15 % behind its classic form on every shape of the
    // table -- nearly every block then adds its output atomically, and its K loop reloads ~30 spilled scalars per step --:
    // dropped; bits 4 + 1 take the two-tap stream-K kernel)
    const int variants[] = {0, kTapGroups2, kMfma32, kTaps3, kTaps3 | kTapGroups2};
    static const bool no_taps3 = getenv("W2L_WGRAD_NO_TAPS3") != nullptr;        // A/B switch of the measured selection
    for (const int bits : variants) {
        const WgradChoice v = WgradChoice::of(0, bits);
        if (v.taps3 ? (no_taps3 || stride != 1 || dil > kTaps3MaxDil || Kw < 3 || (v.tg2 && Kw <= 3)) : ((v.tg2 && Kw <= 2) || (v.m32 && stride != 1)))
            continue;
        const bool has_sk = !v.m32 && !v.taps3 && (!v.tg2 || stride == 1);
        for (int ci = has_sk ? -2 : 0; ci < ncand; ++ci) {
            // ci = -2, -1: the stream-K decomposition in both block orders (no workspace form: skipped in deterministic mode);
            // v: the same split counts and block orders once more with two tap groups per block (the 8-wave kernel: classic
            // and stream-K -- 256 persistent blocks, the balanced form of a kernel whose 1-block-per-CU tiles quantise badly),
            // once more with 32x32x16 MFMA fragments, and with three taps per wave (4- and 8-wave blocks)
            WgradChoice c = v;
            c.streamk = ci < 0;
            if (c.streamk && ws != nullptr && !(flags & 1)) continue;
            c.count = c.streamk ? 1 : cands[ci >> 1];
            c.order = ci & 1;
            c.atomic_ws = (c.streamk || c.count > 1) && ws != nullptr && (flags & 1);     // atomics although a workspace is there
            if (!c.streamk && (c.count > total || (c.count > 1 && total / c.count < 4))) break;
            try_plan(c);
        }
        // dealt stream-K (needs the workspace): one range per resident block slot -- 512 for the 4-wave forms (also tried:
        // 256, one block per CU at a time), 256 for the 8-wave forms -- in both block orders
        if (ws != nullptr) {
            const int ranges[2] = {v.tg2 ? kResidentBlocks / 2 : kResidentBlocks, v.tg2 ? 0 : kResidentBlocks / 2};
            for (int gi = 0; gi < 2; ++gi)
                for (int bo = 0; bo < 2 && ranges[gi] > 0; ++bo) {
                    WgradChoice c = v;
                    c.dealt = true;
                    c.order = bo;
                    c.count = ranges[gi];
                    try_plan(c);
                }
        }
    }
    // (the first pass ranks ~100 plans on `reps` launches each while the chip's clock drifts: the kFinalists fastest are timed again,
    // interleaved: common.h)
    std::sort(timed.begin(), timed.end(), [](const std::pair<float, WgradChoice>& a, const std::pair<float, WgradChoice>& b) {
        return a.first != b.first ? a.first < b.first : a.second.pack() < b.second.pack();
    });
    W2L_CHECK_ARG(!timed.empty(), "conv1d_wgrad_tune: no candidate ran");
    int kb = 0;
    const int finalists = timed.size() < kFinalists ? (int)timed.size() : kFinalists;
    if (finalists > 1) {
        float total_ms[kFinalists] = {};
        for (int round = 0; round < kFinalRounds; ++round)
            for (int k = 0; k < finalists; ++k) {
                const float ms = time_plan(timed[k].second, 4 * reps);
                total_ms[k] += ms >= 0.f ? ms : 1e30f;
            }
        for (int k = 1; k < finalists; ++k)
            if (total_ms[k] < total_ms[kb]) kb = k;
    }
    std::lock_guard<std::mutex> lock(g_wtuned_mu);
    g_wtuned[key] = timed[kb].second;
    return 0;
}

extern "C" int w2l_conv1d_wgrad_tune_ws(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride,
                                        int64_t x_rows_total, float* dw_scratch, int N, int Cin, int Cout, int Tout, int Kw,
                                        int stride, int dil, int reps, void* ws, int64_t ws_bytes, void* stream) {
    return w2l_conv1d_wgrad_tune_x(dy, dy_bstride, xp, x_bstride, x_rows_total, dw_scratch, N, Cin, Cout, Tout, Kw, stride, dil, reps, ws, ws_bytes, 0, stream);
}

extern "C" int w2l_conv1d_wgrad_tune(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride,
                                     int64_t x_rows_total, float* dw_scratch, int N, int Cin, int Cout, int Tout, int Kw,
                                     int stride, int dil, int reps, void* stream) {
    return w2l_conv1d_wgrad_tune_x(dy, dy_bstride, xp, x_bstride, x_rows_total, dw_scratch, N, Cin, Cout, Tout, Kw, stride, dil, reps, nullptr, 0, 0, stream);
}

W2L_DIAG_WGRAD_EXPORTS

// Tuning-cache (de)serialisation used by w2l_tune_save / w2l_tune_load (runtime.hip).
void w2l_wgrad_tune_dump(FILE* f) {
    std::lock_guard<std::mutex> lock(g_wtuned_mu);
    for (const auto& kv : g_wtuned) {
        const WShapeKey& k = kv.first;
        fprintf(f, "wgrad %d %d %d %d %d %d %d\n", std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k),
                std::get<4>(k), kv.second.count, kv.second.bits());
    }
}

bool w2l_wgrad_tune_put(const int* v) {          // v[0..4] = key, v[5] = split (range) count, v[6] = the plan's form bits
    if (v[5] < 1 || v[5] > 0xffff || v[0] < 1 || v[3] < 1 || v[6] < 0 || v[6] > kOrderMask) return false;
    const WgradChoice c = WgradChoice::of(v[5], v[6]);
    if ((c.m32 && (c.streamk || c.tg2)) || (c.taps3 && (c.m32 || c.streamk))) return false;       // forms that were never built
    if (c.dealt ? (c.streamk || c.count > W2L_WGRAD_MAX_RANGES) : (int64_t)c.count > (int64_t)v[0] * ((v[3] + BT - 1) / BT)) return false;
    std::lock_guard<std::mutex> lock(g_wtuned_mu);
    g_wtuned[WShapeKey(v[0], v[1], v[2], v[3], v[4])] = c;
    return true;
}

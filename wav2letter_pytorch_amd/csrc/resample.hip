// Band-limited sample-rate conversion of a padded batch of waveforms on gfx950: the step in front of w2l_logmel for
// files that are not at the model's rate, and for speed perturbation (which is a rate change that is not undone).
//
// Per row: a reduced ratio P/Q = input samples advanced per output sample, n_out = ceil(n_in * Q / P), and
//   out[m] = sum_{j < K} x~[i0 - H + j] * h[phase][j],   i0 = (m P) div Q,  phase = (m P) mod Q   (64-bit integers),
// with x~ zero outside [0, n_in) and h[Q][K] the polyphase bank the host built (data/resample.py: Kaiser-windowed sinc,
// float64, rounded once to fp32).  Rows with P == Q are copied; columns n_out <= m < out_stride are written as zeros.
//
// One launch for the batch, grid (output tile, row).  A block stages the input span of its tile into LDS (16-byte loads
// where the row allows them), then every thread forms RS_PER_THREAD outputs from LDS and its outputs' bank rows.  The bank
// rows are read from memory: neighbouring outputs have different phases, so these reads are per-lane gathers served by
// L1 / L2 (the whole bank of a common ratio is tens of KB).  No atomics, no scratch, no cross-block dependence.
#include "common.h"
#include "../../include/w2l_hip.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PER_THREAD = 2;
constexpr int RS_TILE = RS_THREADS * RS_PER_THREAD;     // outputs per block (W2L_RESAMPLE_TILE)
constexpr int RS_MAX_K = W2L_RESAMPLE_MAX_K;
constexpr int RS_MAX_SPAN = W2L_RESAMPLE_MAX_SPAN;      // floats of LDS a block may stage
static_assert(RS_TILE == W2L_RESAMPLE_TILE, "include/w2l_hip.h states the tile");

struct ResampleParams {
    const float* x;
    float* out;
    const int32_t* rows;     // [N][5]: n_in, n_out, P, Q, bank
    const int32_t* banks;    // [n_banks][4]: offset (floats into taps), K, H, Q
    const float* taps;
    int64_t in_stride, out_stride;
};

// floats a tile of ratio P/Q with K taps may need in LDS: the span of its outputs' windows plus the 3 floats that
// aligning the first one down to 16 bytes can add, rounded up to whole float4s
inline int64_t tile_span(int64_t P, int64_t Q, int64_t K) {
    const int64_t span = ((Q - 1) + (int64_t)(RS_TILE - 1) * P) / Q + K + 3;
    return (span + 3) & ~(int64_t)3;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(ResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int row = blockIdx.y, tid = threadIdx.x;
    const int32_t* rd = p.rows + 5 * row;
    const int64_t n_in = rd[0], n_out = rd[1];
    const int P = rd[2], Q = rd[3];
    const int64_t m0 = (int64_t)blockIdx.x * RS_TILE;
    const float* x = p.x + (int64_t)row * p.in_stride;
    float* out = p.out + (int64_t)row * p.out_stride;

    if (m0 >= n_out || P == Q) {                         // padding columns, or a row at the target rate: zeros / a copy
#pragma unroll
        for (int u = 0; u < RS_PER_THREAD; ++u) {
            const int64_t m = m0 + tid + u * RS_THREADS;
            if (m < p.out_stride) out[m] = m < n_out ? x[m] : 0.f;
        }
        return;
    }
    const int32_t* bd = p.banks + 4 * rd[4];
    const int K = bd[1], H = bd[2];
    const float* bank = p.taps + bd[0];

    // ---- the tile's input span [lo, hi) into LDS, lo rounded down to a float4 boundary of the row
    const int64_t pos0 = m0 * P;                         // 64-bit: m P passes 2^32 within minutes of audio
    const int64_t q0 = pos0 / Q;
    const unsigned r0 = (unsigned)(pos0 - q0 * Q);
    const int64_t m_last = (m0 + RS_TILE < n_out ? m0 + RS_TILE : n_out) - 1;
    const int64_t hi = (m_last * P) / Q - H + K;
    const int64_t lo = (q0 - H) & ~(int64_t)3;
    const int lead = (int)(q0 - H - lo);                 // 0..3
    const int n_stage = (int)(hi - lo);                  // <= tile_span(P, Q, K): the host checked it against the LDS size
    const bool vec_ok = ((p.in_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.x) & 15) == 0);
    for (int i = 4 * tid; i < n_stage; i += 4 * RS_THREADS) {
        const int64_t g = lo + i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (vec_ok && g >= 0 && g + 3 < n_in) {
            v = *reinterpret_cast<const f32x4*>(x + g);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (g + e >= 0 && g + e < n_in) v[e] = x[g + e];
        }
        *reinterpret_cast<f32x4*>(xs + i) = v;           // the LDS array holds whole float4s past n_stage
    }
    __syncthreads();

    // ---- outputs: 32-bit index arithmetic relative to the tile's first position (the host bounds TILE * P + Q)
    const float* s[RS_PER_THREAD];
    const float* h[RS_PER_THREAD];
    float acc[RS_PER_THREAD];
    bool live[RS_PER_THREAD];
#pragma unroll
    for (int u = 0; u < RS_PER_THREAD; ++u) {
        const int dm = tid + u * RS_THREADS;
        live[u] = m0 + dm < n_out;
        const unsigned rel = live[u] ? r0 + (unsigned)dm * (unsigned)P : 0u;
        const unsigned di = rel / (unsigned)Q;
        const unsigned phase = rel - di * (unsigned)Q;
        s[u] = xs + lead + di;
        h[u] = bank + (int64_t)phase * K;
        acc[u] = 0.f;
    }
    for (int j = 0; j < K; j += 2) {                     // K = 2H + 2 is even; bank rows start on 8-byte boundaries
#pragma unroll
        for (int u = 0; u < RS_PER_THREAD; ++u) {
            const float2 hv = *reinterpret_cast<const float2*>(h[u] + j);
            acc[u] = fmaf(s[u][j], hv.x, acc[u]);
            acc[u] = fmaf(s[u][j + 1], hv.y, acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < RS_PER_THREAD; ++u) {
        const int64_t m = m0 + tid + u * RS_THREADS;
        if (m < p.out_stride) out[m] = live[u] ? acc[u] : 0.f;
    }
}

}  // namespace

extern "C" int w2l_resample(const float* x, int64_t in_stride, float* out, int64_t out_stride, int N, const int32_t* rows_host,
                            const int32_t* rows_dev, const int32_t* banks_host, const int32_t* banks_dev, int n_banks,
                            const float* taps, int64_t n_taps, void* stream) {
    W2L_CHECK_ARG(x && out && rows_host && rows_dev, "resample: null pointer");
    W2L_CHECK_ARG(N > 0 && N <= 65535 && in_stride > 0 && out_stride > 0, "resample: bad sizes (N=%d, strides %lld / %lld)", N,
                  (long long)in_stride, (long long)out_stride);
    W2L_CHECK_ARG(n_banks >= 0 && (n_banks == 0 || (banks_host && banks_dev && taps && n_taps > 0)),
                  "resample: null bank table or taps");
    W2L_CHECK_ARG((reinterpret_cast<uintptr_t>(taps) & 7) == 0, "resample: taps must be 8-byte aligned");
    W2L_CHECK_ARG((out_stride + RS_TILE - 1) / RS_TILE <= 0x7fffffffLL, "resample: out_stride=%lld is too long", (long long)out_stride);
    for (int b = 0; b < n_banks; ++b) {
        const int32_t* bd = banks_host + 4 * b;
        const int64_t off = bd[0], K = bd[1], H = bd[2], Q = bd[3];
        W2L_CHECK_ARG(K <= RS_MAX_K, "resample: bank %d has K=%lld taps, above the supported %d", b, (long long)K, RS_MAX_K);
        W2L_CHECK_ARG(H >= 0 && K == 2 * H + 2 && Q > 0, "resample: bank %d: K=%lld, H=%lld, Q=%lld (K must be 2H + 2)", b,
                      (long long)K, (long long)H, (long long)Q);
        W2L_CHECK_ARG(off >= 0 && (off & 1) == 0 && off + Q * K <= n_taps, "resample: bank %d [%lld, +%lld x %lld) leaves the %lld taps", b,
                      (long long)off, (long long)Q, (long long)K, (long long)n_taps);
    }
    int64_t lds_floats = 4;
    for (int n = 0; n < N; ++n) {
        const int32_t* rd = rows_host + 5 * n;
        const int64_t n_in = rd[0], n_out = rd[1], P = rd[2], Q = rd[3], bank = rd[4];
        W2L_CHECK_ARG(P > 0 && Q > 0, "resample: row %d has the ratio %lld/%lld", n, (long long)P, (long long)Q);
        W2L_CHECK_ARG(n_in >= 0 && n_in <= in_stride, "resample: row %d: n_in=%lld outside [0, in_stride=%lld]", n, (long long)n_in,
                      (long long)in_stride);
        W2L_CHECK_ARG(n_out == (n_in * Q + P - 1) / P, "resample: row %d: n_out=%lld is not ceil(n_in * Q / P) = ceil(%lld * %lld / %lld)", n,
                      (long long)n_out, (long long)n_in, (long long)Q, (long long)P);
        W2L_CHECK_ARG(n_out <= out_stride, "resample: row %d: n_out=%lld exceeds out_stride=%lld", n, (long long)n_out, (long long)out_stride);
        if (P == Q) continue;                            // copied; needs no bank
        W2L_CHECK_ARG((int64_t)RS_TILE * P + Q < (1LL << 31), "resample: row %d: ratio %lld/%lld is not reduced far enough for 32-bit tile offsets", n,
                      (long long)P, (long long)Q);
        W2L_CHECK_ARG(bank >= 0 && bank < n_banks, "resample: row %d names bank %lld of %d", n, (long long)bank, n_banks);
        const int32_t* bd = banks_host + 4 * bank;
        W2L_CHECK_ARG(bd[3] == Q, "resample: row %d has Q=%lld but its bank has %d phases", n, (long long)Q, bd[3]);
        const int64_t span = tile_span(P, Q, bd[1]);
        W2L_CHECK_ARG(span <= RS_MAX_SPAN, "resample: row %d: a tile of ratio %lld/%lld with K=%d spans %lld floats, above the supported %d", n,
                      (long long)P, (long long)Q, bd[1], (long long)span, RS_MAX_SPAN);
        lds_floats = span > lds_floats ? span : lds_floats;
    }
    ResampleParams p;
    p.x = x; p.out = out; p.rows = rows_dev; p.banks = banks_dev; p.taps = taps;
    p.in_stride = in_stride; p.out_stride = out_stride;
    dim3 grid((unsigned)((out_stride + RS_TILE - 1) / RS_TILE), N);
    hipLaunchKernelGGL(resample_kernel, grid, dim3(RS_THREADS), (size_t)lds_floats * sizeof(float), (hipStream_t)stream, p);
    W2L_CHECK_LAUNCH();
    return 0;
}

// Waveform augmentation of a padded batch on gfx950, between w2l_resample and w2l_logmel (data/augment_wave.py): room
// reverberation (a per-row FIR with a per-row impulse response) and additive noise at an exact signal-to-noise ratio.
//
// w2l_reverb.  Row n of n_in samples, response h[0..K) with its direct path at tap d:
//   out[m] = sum_{j < K} h[j] * x~[m + d - j],  0 <= m < n_in,  x~ = 0 outside [0, n_in);  out[m] = 0 for n_in <= m < out_stride.
// Toeplitz form on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit an fmaf chain, so the arithmetic is exact fp32).
// With m = 32 a + b and j = 32 c + b - e + d the sum becomes
//   out[32 a + b] = sum_c sum_{e < 32} T_c[b][e] * x~[32 (a - c) + e],   T_c[b][e] = h~[32 c + b - e + d],  h~ = 0 outside [0, K):
// a GEMM whose 32-row A operand T_c is built from h and shared by every a, with the 32-sample blocks of x as B columns.  It
// spends about K + 62 multiply-adds per output: no redundant work.  One launch, grid (tile of RV_TILE = 32 x 32 outputs, row).
// A block of 4 waves walks the blocks c in chunks of RV_CC: it stages the 32 + RV_CC - 1 blocks of x the chunk touches (row
// stride 33 floats: the B operand reads lanes at a stride of one block, which at 32 would be one bank) and the chunk's
// 32 RV_CC + 31 taps, then every wave takes 4 of the chunk's c -- one accumulator each, 16 MFMAs (e pairs) per c.  The 16 partial
// tiles of a block are summed in a fixed order through LDS: no atomics, no cross-block dependence, identical bits every call.
//
// w2l_mix_noise.  Row n with a noise clip z[0..n_z), an offset o and snr_db:
//   Ps = mean x^2,  Pz = mean z[(o + m) mod n_z]^2 over m < n_in,  g = sqrt(Ps / (Pz 10^(snr_db / 10))),  out[m] = fmaf(g, z[..], x[m]).
// Two launches in the slab idiom: a power pass, grid (tile, row), writes fp64 partial sums [row][tile][2] (every sample widened
// before squaring, block tree of fixed shape); the apply pass has each block add its row's partials in index order, form g in
// double, round it once and apply.  Rows without a clip, silent rows and silent clips are copied bit for bit.
#include "common.h"
#include "../../include/w2l_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ reverberation
constexpr int RV_THREADS = 256, RV_WAVES = 4;
constexpr int RV_TILE = 1024;                            // outputs per block: 32 blocks of 32 (W2L_REVERB_TILE)
constexpr int RV_CC = 16;                                // Toeplitz blocks per staged chunk
constexpr int RV_CHUNK = 32 * RV_CC;                     // taps per staged chunk (W2L_REVERB_CHUNK)
constexpr int RV_XBLK = 32 + RV_CC - 1;                  // blocks of x a chunk touches
constexpr int RV_XROW = 33;                              // floats between staged blocks of x
constexpr int RV_XS = RV_XBLK * RV_XROW;
constexpr int RV_HS = 32 * RV_CC + 31;                   // taps 32 c0 + d - 31 ... 32 (c0 + RV_CC - 1) + d + 31
constexpr int RV_RED = RV_WAVES * 32 * RV_XROW;          // one padded 32 x 32 tile per wave
static_assert(RV_TILE == W2L_REVERB_TILE && RV_CHUNK == W2L_REVERB_CHUNK, "include/w2l_hip.h states the tile and the chunk");
static_assert(RV_CC == 4 * RV_WAVES && RV_XS + RV_HS <= RV_RED, "4 accumulators per wave; the staging area is reused for the sum");

struct ReverbParams {
    const float* x;
    float* out;
    const int32_t* rows;     // [N][2]: n_in, bank (-1: copied)
    const int32_t* banks;    // [n_banks][3]: offset (floats into taps), K, d
    const float* taps;
    int64_t in_stride, out_stride;
};

__global__ __launch_bounds__(RV_THREADS) void reverb_kernel(ReverbParams p) {
    __shared__ float smem[RV_RED];
    float* xs = smem;
    float* hs = smem + RV_XS;
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t* rd = p.rows + 2 * row;
    const int n_in = rd[0], bank = rd[1];
    const int m0 = blockIdx.x * RV_TILE;
    const float* x = p.x + (int64_t)row * p.in_stride;
    float* out = p.out + (int64_t)row * p.out_stride;

    if (m0 >= n_in || bank < 0) {                        // padding columns, or a row without a response: zeros / a copy
        for (int i = tid; i < RV_TILE; i += RV_THREADS) {
            const int m = m0 + i;
            if (m < p.out_stride) out[m] = m < n_in ? x[m] : 0.f;
        }
        return;
    }
    const int32_t* bd = p.banks + 3 * bank;
    const float* h = p.taps + bd[0];
    const int K = bd[1], d = bd[2];
    const int a0 = m0 >> 5;
    // blocks c with a non-zero T_c (32 c + d + 31 >= 0, 32 c + d - 31 <= K - 1) that meet a block of x inside [0, n_in)
    int c_lo = -((d + 31) >> 5), c_hi = (K + 30 - d) >> 5;
    c_lo = max(c_lo, a0 - ((n_in - 1) >> 5));
    c_hi = min(c_hi, a0 + 31);

    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const int lj = lane & 31, lk = lane >> 5;            // operand lane maps: A[i = lj][k = lk], B[k = lk][j = lj]

    for (int c0 = c_lo; c0 <= c_hi; c0 += RV_CC) {
        const int g0 = m0 - 32 * (c0 + RV_CC - 1);       // sample index of the first staged block
        for (int f = tid; f < RV_XBLK * 32; f += RV_THREADS) {
            const int g = g0 + f;
            xs[(f >> 5) * RV_XROW + (f & 31)] = (g >= 0 && g < n_in) ? x[g] : 0.f;
        }
        const int j0 = 32 * c0 + d - 31;
        for (int i = tid; i < RV_HS; i += RV_THREADS) {
            const int j = j0 + i;
            hs[i] = (j >= 0 && j < K) ? h[j] : 0.f;
        }
        __syncthreads();
        // this wave's blocks of the chunk: cc = 4 q + wave, q < nq (the chunk's last blocks may lie past c_hi)
        const int left = c_hi - c0 - wave;
        const int nq = left < 0 ? 0 : (left / RV_WAVES + 1 < 4 ? left / RV_WAVES + 1 : 4);
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < nq) {
                    const int cc = 4 * q + wave;
                    const float a = hs[32 * cc + 31 + lj - lk - 2 * s];                            // T_c[lj][2 s + lk]
                    const float b = xs[(lj + RV_CC - 1 - cc) * RV_XROW + 2 * s + lk];             // x block a0 + lj - c, sample 2 s + lk
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[q], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- the block's 16 partial tiles in a fixed order: 4 accumulators in registers, 4 waves through LDS
    float* red = smem + wave * (32 * RV_XROW);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int b = (r & 3) + 8 * (r >> 2) + 4 * lk;   // C/D map of the 32x32 MFMAs: column on the lane, row from the register
        red[lj * RV_XROW + b] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
    }
    __syncthreads();
    for (int i = tid; i < RV_TILE; i += RV_THREADS) {
        const int at = (i >> 5) * RV_XROW + (i & 31);
        const float v = ((smem[at] + smem[32 * RV_XROW + at]) + smem[2 * 32 * RV_XROW + at]) + smem[3 * 32 * RV_XROW + at];
        const int m = m0 + i;
        if (m < p.out_stride) out[m] = m < n_in ? v : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------ noise mixing
constexpr int MX_THREADS = 256;
constexpr int MX_PER_THREAD = 8;
constexpr int MX_TILE = MX_THREADS * MX_PER_THREAD;      // samples per block (W2L_MIX_TILE)
static_assert(MX_TILE == W2L_MIX_TILE, "include/w2l_hip.h states the tile");

struct MixParams {
    const float* x;
    const float* z;
    float* out;
    const int32_t* rows;     // [N][3]: n_in, n_z (0: no clip), o
    const float* snr_db;     // [N]
    double* slab;            // [N][tiles][2]: sums of x^2 and of z^2 per tile
    int64_t x_stride, z_stride, out_stride;
    int tiles;
};

__global__ __launch_bounds__(MX_THREADS) void mix_power_kernel(MixParams p) {
    __shared__ double sx[MX_THREADS], sz[MX_THREADS];
    const int row = blockIdx.y, tid = threadIdx.x;
    const int32_t* rd = p.rows + 3 * row;
    const int n_in = rd[0];
    const unsigned n_z = (unsigned)rd[1], o = (unsigned)rd[2];
    const int m0 = blockIdx.x * MX_TILE;
    if (n_z == 0 || m0 >= n_in) return;                  // the apply pass reads tiles [0, ceil(n_in / tile)) of rows with a clip
    const float* x = p.x + (int64_t)row * p.x_stride;
    const float* z = p.z + (int64_t)row * p.z_stride;
    double ax = 0.0, az = 0.0;
#pragma unroll
    for (int u = 0; u < MX_PER_THREAD; ++u) {
        const int m = m0 + tid + u * MX_THREADS;
        if (m < n_in) {
            const double xv = (double)x[m], zv = (double)z[(o + (unsigned)m) % n_z];
            ax += xv * xv;
            az += zv * zv;
        }
    }
    sx[tid] = ax;
    sz[tid] = az;
    __syncthreads();
    for (int w = MX_THREADS / 2; w > 0; w >>= 1) {       // a tree of fixed shape: the same bits every call
        if (tid < w) {
            sx[tid] += sx[tid + w];
            sz[tid] += sz[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* s = p.slab + ((int64_t)row * p.tiles + blockIdx.x) * 2;
        s[0] = sx[0];
        s[1] = sz[0];
    }
}

__global__ __launch_bounds__(MX_THREADS) void mix_apply_kernel(MixParams p) {
    const int row = blockIdx.y, tid = threadIdx.x;
    const int32_t* rd = p.rows + 3 * row;
    const int n_in = rd[0];
    const unsigned n_z = (unsigned)rd[1], o = (unsigned)rd[2];
    const int m0 = blockIdx.x * MX_TILE;
    const float* x = p.x + (int64_t)row * p.x_stride;
    float* out = p.out + (int64_t)row * p.out_stride;
    float g = 0.f;
    bool mix = false;
    if (n_z != 0 && m0 < n_in) {
        const double* s = p.slab + (int64_t)row * p.tiles * 2;
        const int nt = (n_in + MX_TILE - 1) / MX_TILE;
        double px = 0.0, pz = 0.0;
        for (int t = 0; t < nt; ++t) {                   // every thread the same addresses in the same order
            px += s[2 * t];
            pz += s[2 * t + 1];
        }
        if (px > 0.0 && pz > 0.0) {                      // a silent utterance or a silent clip is copied
            g = (float)sqrt(px / (pz * pow(10.0, (double)p.snr_db[row] / 10.0)));
            mix = true;
        }
    }
    const float* z = p.z + (int64_t)row * p.z_stride;
#pragma unroll
    for (int u = 0; u < MX_PER_THREAD; ++u) {
        const int m = m0 + tid + u * MX_THREADS;
        if (m >= p.out_stride) continue;
        float v = 0.f;
        if (m < n_in) {
            v = x[m];
            if (mix) v = fmaf(g, z[(o + (unsigned)m) % n_z], v);
        }
        out[m] = v;
    }
}

}  // namespace

extern "C" int w2l_reverb(const float* x, int64_t in_stride, float* out, int64_t out_stride, int N, const int32_t* rows_host,
                          const int32_t* rows_dev, const int32_t* banks_host, const int32_t* banks_dev, int n_banks,
                          const float* taps, int64_t n_taps, void* stream) {
    W2L_CHECK_ARG(x && out && rows_host && rows_dev, "reverb: null pointer");
    W2L_CHECK_ARG(x != out, "reverb: the output must be a separate buffer");
    W2L_CHECK_ARG(N > 0 && N <= 65535 && in_stride > 0 && out_stride > 0 && in_stride <= (1LL << 30) && out_stride <= (1LL << 30),
                  "reverb: bad sizes (N=%d, strides %lld / %lld)", N, (long long)in_stride, (long long)out_stride);
    W2L_CHECK_ARG(n_banks >= 0 && (n_banks == 0 || (banks_host && banks_dev && taps && n_taps > 0)), "reverb: null bank table or taps");
    for (int b = 0; b < n_banks; ++b) {
        const int32_t* bd = banks_host + 3 * b;
        const int64_t off = bd[0], K = bd[1], d = bd[2];
        W2L_CHECK_ARG(K <= W2L_REVERB_MAX_TAPS, "reverb: response %d has K=%lld taps, above W2L_REVERB_MAX_TAPS = %d", b, (long long)K,
                      W2L_REVERB_MAX_TAPS);
        W2L_CHECK_ARG(K >= 1 && d >= 0 && d < K, "reverb: response %d: K=%lld, direct path d=%lld (need 0 <= d < K)", b, (long long)K,
                      (long long)d);
        W2L_CHECK_ARG(off >= 0 && off + K <= n_taps, "reverb: response %d [%lld, +%lld) leaves the %lld taps", b, (long long)off, (long long)K,
                      (long long)n_taps);
    }
    for (int n = 0; n < N; ++n) {
        const int64_t n_in = rows_host[2 * n], bank = rows_host[2 * n + 1];
        W2L_CHECK_ARG(n_in >= 0 && n_in <= in_stride && n_in <= out_stride, "reverb: row %d: n_in=%lld outside [0, min(in_stride=%lld, out_stride=%lld)]",
                      n, (long long)n_in, (long long)in_stride, (long long)out_stride);
        W2L_CHECK_ARG(bank >= -1 && bank < n_banks, "reverb: row %d names response %lld of %d", n, (long long)bank, n_banks);
    }
    ReverbParams p;
    p.x = x; p.out = out; p.rows = rows_dev; p.banks = banks_dev; p.taps = taps;
    p.in_stride = in_stride; p.out_stride = out_stride;
    dim3 grid((unsigned)((out_stride + RV_TILE - 1) / RV_TILE), N);
    hipLaunchKernelGGL(reverb_kernel, grid, dim3(RV_THREADS), 0, (hipStream_t)stream, p);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t w2l_mix_noise_slab_doubles(int N, int64_t out_stride) {
    if (N <= 0 || out_stride <= 0) return -1;
    return (int64_t)N * ((out_stride + MX_TILE - 1) / MX_TILE) * 2;
}

extern "C" int w2l_mix_noise(const float* x, int64_t x_stride, const float* z, int64_t z_stride, float* out, int64_t out_stride, int N,
                             const int32_t* rows_host, const int32_t* rows_dev, const float* snr_db, double* slab,
                             int64_t slab_doubles, void* stream) {
    W2L_CHECK_ARG(x && out && rows_host && rows_dev && snr_db && slab, "mix_noise: null pointer");
    W2L_CHECK_ARG(x != out, "mix_noise: the output must be a separate buffer");
    W2L_CHECK_ARG(N > 0 && N <= 65535 && x_stride > 0 && out_stride > 0 && z_stride >= 0 && x_stride <= (1LL << 30) &&
                      out_stride <= (1LL << 30) && z_stride <= (1LL << 30),
                  "mix_noise: bad sizes (N=%d, strides %lld / %lld / %lld)", N, (long long)x_stride, (long long)z_stride, (long long)out_stride);
    W2L_CHECK_ARG(slab_doubles >= w2l_mix_noise_slab_doubles(N, out_stride), "mix_noise: the slab holds %lld doubles, %lld are needed",
                  (long long)slab_doubles, (long long)w2l_mix_noise_slab_doubles(N, out_stride));
    bool any = false;
    for (int n = 0; n < N; ++n) {
        const int64_t n_in = rows_host[3 * n], n_z = rows_host[3 * n + 1], o = rows_host[3 * n + 2];
        W2L_CHECK_ARG(n_in >= 0 && n_in <= x_stride && n_in <= out_stride, "mix_noise: row %d: n_in=%lld outside [0, min(x_stride=%lld, out_stride=%lld)]",
                      n, (long long)n_in, (long long)x_stride, (long long)out_stride);
        W2L_CHECK_ARG(n_z >= 0 && n_z <= z_stride, "mix_noise: row %d: n_z=%lld outside [0, z_stride=%lld]", n, (long long)n_z, (long long)z_stride);
        W2L_CHECK_ARG(n_z == 0 ? o == 0 : (o >= 0 && o < n_z), "mix_noise: row %d: offset %lld outside its clip of %lld samples", n, (long long)o,
                      (long long)n_z);
        any = any || n_z > 0;
    }
    W2L_CHECK_ARG(!any || z, "mix_noise: null noise batch");
    MixParams p;
    p.x = x; p.z = z; p.out = out; p.rows = rows_dev; p.snr_db = snr_db; p.slab = slab;
    p.x_stride = x_stride; p.z_stride = z_stride; p.out_stride = out_stride;
    p.tiles = (int)((out_stride + MX_TILE - 1) / MX_TILE);
    dim3 grid((unsigned)p.tiles, N);
    if (any) {
        hipLaunchKernelGGL(mix_power_kernel, grid, dim3(MX_THREADS), 0, (hipStream_t)stream, p);
        W2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mix_apply_kernel, grid, dim3(MX_THREADS), 0, (hipStream_t)stream, p);
    W2L_CHECK_LAUNCH();
    return 0;
}

// Direct form of w2l_reverb on the vector ALU: built, measured against the Toeplitz / MFMA form of csrc/augment.hip and not
// selected (DESIGN Appendix B; tools/bench_augment.py builds this file into tools/probe/libreverb_direct.so and times both
// forms interleaved in one process).  Same definition and tables as w2l_reverb; no argument checks -- a probe, called with
// tables the shipped entry point has already accepted.
//
// Grid (tile of 2048 outputs, row), 256 threads, 8 consecutive outputs per thread in registers.  Per chunk of 256 taps the
// block stages the tile's input span (2048 + 255 samples) and the taps in LDS; a thread then walks the taps 8 at a time
// with a 16-sample register window: 64 fmaf per four 16-byte window loads and two broadcast tap loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr int THREADS = 256, R = 8, TILE = THREADS * R, CH = 256;

__global__ __launch_bounds__(THREADS) void reverb_direct_kernel(const float* xb, int64_t in_stride, float* ob, int64_t out_stride,
                                                                const int32_t* rows, const int32_t* banks, const float* taps) {
    __shared__ __attribute__((aligned(16))) float gs[TILE + CH];
    __shared__ __attribute__((aligned(16))) float hs[CH];
    const int row = blockIdx.y, tid = threadIdx.x;
    const int n_in = rows[2 * row], bank = rows[2 * row + 1];
    const int m0 = blockIdx.x * TILE;
    const float* x = xb + (int64_t)row * in_stride;
    float* out = ob + (int64_t)row * out_stride;
    if (m0 >= n_in || bank < 0) {
        for (int i = tid; i < TILE; i += THREADS) {
            const int m = m0 + i;
            if (m < out_stride) out[m] = m < n_in ? x[m] : 0.f;
        }
        return;
    }
    const float* h = taps + banks[3 * bank];
    const int K = banks[3 * bank + 1], d = banks[3 * bank + 2];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int j0 = 0; j0 < K; j0 += CH) {
        const int g0 = m0 + d - j0 - (CH - 1);           // gs[i] = x~[g0 + i]: output o, tap j0 + jj reads gs[o - jj + CH - 1]
        for (int i = tid; i < TILE + CH; i += THREADS) {
            const int g = g0 + i;
            gs[i] = (g >= 0 && g < n_in) ? x[g] : 0.f;
        }
        hs[tid] = j0 + tid < K ? h[j0 + tid] : 0.f;
        __syncthreads();
        for (int u0 = 0; u0 < CH; u0 += 8) {
            const int base = tid * R + CH - 8 - u0;      // a multiple of 8: 16-byte loads
            float w[16], t[8];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(gs + base + 4 * v);
                w[4 * v] = q[0]; w[4 * v + 1] = q[1]; w[4 * v + 2] = q[2]; w[4 * v + 3] = q[3];
            }
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(hs + u0 + 4 * v);
                t[4 * v] = q[0]; t[4 * v + 1] = q[1]; t[4 * v + 2] = q[2]; t[4 * v + 3] = q[3];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(t[u], w[r + 7 - u], acc[r]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < R; ++r) gs[tid * R + r] = acc[r];
    __syncthreads();
    for (int i = tid; i < TILE; i += THREADS) {
        const int m = m0 + i;
        if (m < out_stride) out[m] = m < n_in ? gs[i] : 0.f;
    }
}

}  // namespace

extern "C" int reverb_direct(const float* x, int64_t in_stride, float* out, int64_t out_stride, int N, const int32_t* rows_dev,
                             const int32_t* banks_dev, const float* taps, void* stream) {
    dim3 grid((unsigned)((out_stride + TILE - 1) / TILE), N);
    hipLaunchKernelGGL(reverb_direct_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, x, in_stride, out, out_stride, rows_dev,
                       banks_dev, taps);
    return (int)hipGetLastError();
}

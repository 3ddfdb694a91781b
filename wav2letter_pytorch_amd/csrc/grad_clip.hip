// Gradient clipping with the coefficient computed on the device: torch.nn.utils.clip_grad_norm_ / clip_grad_value_ (what
// Lightning's Trainer(gradient_clip_val=...) calls between backward() and step()) without a host read and without a pass
// that rewrites the gradients.  w2l_grad_sqnorm_multi reads every gradient ONCE (one launch over a table of tensors, then a
// one-block finalize) and leaves {total norm, coefficient, bound} in a small device buffer; the update kernels of optim.hip
// apply clamp(g * coef, -bound, bound) as they read each gradient.
//
// Deterministic: fixed grid, fixed chunk-to-block assignment, per-block partials summed in a fixed order -- no atomics on
// values.  Data-parallel replicas hold bit-identical averaged gradients and must derive bit-identical coefficients.
#include "common.h"
#include "../../include/w2l_hip.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_VEC = W2L_GNORM_CHUNK / (4 * GN_THREADS);      // float4 loads per thread per chunk
static_assert(W2L_GNORM_CHUNK % (4 * GN_THREADS) == 0, "chunk = whole float4 rows of the block");

// max that propagates NaN (torch's inf-norm is a max-reduction of |g|, and a NaN in it makes the norm NaN)
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || a > b) ? a : b; }

// grid-stride over the chunks of all rows: chunk c belongs to the last row whose first chunk is <= c (binary search over the
// table: ~6 uniform loads per 32 KB chunk).  A full chunk of a 16-byte-aligned row is GN_VEC independent float4 loads per
// thread, all issued before the first is used; anything else (the tail of a row, a misaligned row) goes element by element.
// Per thread: the squares of one chunk are summed in fp32 (32 terms), the running total is fp64.
__global__ __launch_bounds__(GN_THREADS) void grad_norm_partial_kernel(const w2l_gnorm_item_t* items, int nitems, int64_t nchunks,
                                                                      int inf_norm, double* partial) {
    __shared__ double red[GN_THREADS];
    double acc = 0.0;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        int lo = 0, hi = nitems - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (items[mid].chunk0 <= c) lo = mid;
            else hi = mid - 1;
        }
        const float* g = items[lo].g;
        const int64_t n = items[lo].n;
        const int64_t base = (c - items[lo].chunk0) * W2L_GNORM_CHUNK;
        const int64_t end = min(n, base + (int64_t)W2L_GNORM_CHUNK);
        float s = 0.f;
        if (end - base == W2L_GNORM_CHUNK && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const float4* g4 = reinterpret_cast<const float4*>(g + base);
            float4 v[GN_VEC];
#pragma unroll
            for (int k = 0; k < GN_VEC; ++k) v[k] = g4[threadIdx.x + k * GN_THREADS];
#pragma unroll
            for (int k = 0; k < GN_VEC; ++k) {
                if (inf_norm) {
                    s = nan_max(s, fabsf(v[k].x)); s = nan_max(s, fabsf(v[k].y));
                    s = nan_max(s, fabsf(v[k].z)); s = nan_max(s, fabsf(v[k].w));
                } else {
                    s += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
                }
            }
        } else {
            for (int64_t i = base + threadIdx.x; i < end; i += GN_THREADS) {
                const float x = g[i];
                if (inf_norm) s = nan_max(s, fabsf(x));
                else s += x * x;
            }
        }
        acc = inf_norm ? nan_max(acc, (double)s) : acc + (double)s;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = GN_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double a = red[threadIdx.x], b = red[threadIdx.x + w];
            red[threadIdx.x] = inf_norm ? nan_max(a, b) : a + b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one block: the partials in a fixed order, then torch.nn.utils.clip_grad_norm_'s coefficient in fp32 --
// clip_coef = max_norm / (total_norm + 1e-6), clamped to <= 1 (an inf norm gives 0, a NaN norm NaN)
__global__ __launch_bounds__(GN_THREADS) void grad_norm_finalize_kernel(const double* partial, int nblocks, int inf_norm,
                                                                       float max_norm, float* clip, float* norm_out) {
    __shared__ double red[GN_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += GN_THREADS) acc = inf_norm ? nan_max(acc, partial[i]) : acc + partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = GN_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double a = red[threadIdx.x], b = red[threadIdx.x + w];
            red[threadIdx.x] = inf_norm ? nan_max(a, b) : a + b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = inf_norm ? (float)red[0] : (float)sqrt(red[0]);
        const float c = __fdiv_rn(max_norm, __fadd_rn(total, 1e-6f));
        clip[W2L_CLIP_NORM] = total;
        clip[W2L_CLIP_COEF] = c > 1.f ? 1.f : c;
        clip[W2L_CLIP_BOUND] = __builtin_inff();
        if (norm_out != nullptr) norm_out[0] = total;
    }
}

__global__ void grad_clip_value_kernel(float* clip, float clip_value) {
    if (threadIdx.x == 0) {
        clip[W2L_CLIP_NORM] = 0.f;
        clip[W2L_CLIP_COEF] = 1.f;
        clip[W2L_CLIP_BOUND] = clip_value;
    }
}

}  // namespace

extern "C" int w2l_grad_sqnorm_multi(const w2l_gnorm_item_t* items_dev, int nitems, int64_t nchunks, int inf_norm,
                                     double* partials, float max_norm, float* clip, float* norm_out, void* stream) {
    W2L_CHECK_ARG(clip != nullptr && partials != nullptr, "grad_sqnorm_multi: null pointer");
    W2L_CHECK_ARG(nitems >= 0 && nchunks >= 0 && (items_dev != nullptr || nitems == 0) && (nitems > 0 || nchunks == 0),
                  "grad_sqnorm_multi: bad table");
    const hipStream_t st = (hipStream_t)stream;
    const int nblocks = nchunks < W2L_GNORM_BLOCKS ? (int)nchunks : W2L_GNORM_BLOCKS;
    if (nblocks > 0) {
        hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(nblocks), dim3(GN_THREADS), 0, st, items_dev, nitems, nchunks,
                           inf_norm ? 1 : 0, partials);
        W2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(GN_THREADS), 0, st, (const double*)partials, nblocks,
                       inf_norm ? 1 : 0, max_norm, clip, norm_out);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int w2l_grad_clip_value(float* clip, float clip_value, void* stream) {
    W2L_CHECK_ARG(clip != nullptr, "grad_clip_value: null pointer");
    hipLaunchKernelGGL(grad_clip_value_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, clip, clip_value);
    W2L_CHECK_LAUNCH();
    return 0;
}

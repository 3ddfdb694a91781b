// The optimizer updates (HBM-bound): every kernel that applies an update rule, and its entry point.
//   * conv weights (tap-major [Kw][Cout][Cin]): the update fused with the operand pack of the NEXT step, one 32x32 tile walk
//     (update_pack_tile) under three rules -- SGD, Adam / AdamW, Novograd;
//   * everything else (biases, BatchNorm gamma / beta, the classifier): one launch over a device table of parameters, one
//     chunked walk (small_multi_walk) under the SGD and the Adam rule;
//   * Novograd's per-tensor norm and Adam's per-step scalars.
#include "common.h"
#include "../../include/w2l_hip.h"

namespace {

// ---- gradient clipping applied on read (w2l_grad_sqnorm_multi / w2l_grad_clip_value write the float[4] clip buffer) ----
// clamp(g * coef, -bound, bound) in torch's order (clip_grad_norm_ multiplies, clip_grad_value_ clamps), before the weight decay.
// The product is rounded on its own (__fmul_rn: no contraction into the decay's FMA), so coef == 1 and bound == +inf leave the
// update bit-identical to no clipping; comparisons instead of fminf / fmaxf keep a NaN gradient (or coefficient) a NaN, as
// torch.clamp does.
__device__ __forceinline__ float clip_grad_read(float g, float coef, float bound) {
    g = __fmul_rn(g, coef);
    g = g < -bound ? -bound : g;
    return g > bound ? bound : g;
}
// how a kernel reads its gradients: as they are, or (CLIP) through the coefficient and bound of the clip buffer
template <bool CLIP>
struct grad_reader {
    float coef = 1.f, bound = 0.f;
    __device__ __forceinline__ explicit grad_reader(const float* clip) {
        if constexpr (CLIP) {
            coef = clip[W2L_CLIP_COEF];
            bound = clip[W2L_CLIP_BOUND];
        }
    }
    __device__ __forceinline__ float operator()(float g) const {
        if constexpr (CLIP) g = clip_grad_read(g, coef, bound);
        return g;
    }
};

// ---- Adam / AdamW, one element (w2l_adam_pack, w2l_adam_small_multi): torch's _single_tensor_adam, amsgrad / maximize off.
// What changes from step to step lives in device memory (the float[4] `dyn` w2l_adam_tick writes): lr, lr / (1 - beta1^t),
// sqrt(1 - beta2^t) -- a recorded launch names the buffer, not the values.
//   decoupled (AdamW): p *= 1 - lr*wd        else: g += wd*p
//   m = beta1*m + (1-beta1)*g;  v = beta2*v + (1-beta2)*g*g;  p -= dyn[1] * m / (sqrt(v)/dyn[2] + eps) ----
#define W2L_ADAM_LR 0
#define W2L_ADAM_STEP_SIZE 1
#define W2L_ADAM_BC2_SQRT 2
struct adam_scalars {
    float lr, step_size, bc2_sqrt, beta1, beta2, omb1, omb2, eps, wd;
    int decoupled;
};
__device__ __forceinline__ adam_scalars adam_load_scalars(const float* dyn, float beta1, float beta2, float eps, float wd,
                                                          int decoupled) {
    adam_scalars s;
    s.lr = dyn[W2L_ADAM_LR];
    s.step_size = dyn[W2L_ADAM_STEP_SIZE];
    s.bc2_sqrt = dyn[W2L_ADAM_BC2_SQRT];
    s.beta1 = beta1;
    s.beta2 = beta2;
    s.omb1 = 1.f - beta1;
    s.omb2 = 1.f - beta2;
    s.eps = eps;
    s.wd = wd;
    s.decoupled = decoupled;
    return s;
}
// -> the new p; m and v are updated in place
__device__ __forceinline__ float adam_update(const adam_scalars& s, float pv, float gv, float& mv, float& vv) {
    if (s.decoupled) pv *= 1.f - s.lr * s.wd;
    else if (s.wd != 0.f) gv += s.wd * pv;
    mv = s.beta1 * mv + s.omb1 * gv;
    vv = s.beta2 * vv + s.omb2 * (gv * gv);
    const float denom = sqrtf(vv) / s.bc2_sqrt + s.eps;
    return pv - s.step_size * (mv / denom);
}

// ---- conv weights: update + operand pack ---------------------------------------------------------------------------------
// The bf16 GEMM operands of the next step: w_fwd [Kw][Cout][Cin] (the master's layout) and w_dgr [Kw][Cin][Cout] with taps
// flipped, each hi (+ lo in split-bf16 mode); in fp8 mode also their e4m3 forms, quantised from the bf16-rounded value like
// w2l_quantize_e4m3 (null: not written).
struct pack_out {
    bf16_raw *fwd_hi, *fwd_lo, *dgr_hi, *dgr_lo;
    uint8_t *fwd_q, *dgr_q;
    float q_scale;
};
__device__ __forceinline__ uint8_t quant_bf16_e4m3(float v, float q_scale) {
    return quant1_e4m3(bf16_bits_to_f32(f32_to_bf16_bits(v)) * q_scale);
}
// One pass over a tap-major conv weight (fp32 master, gradient and state in the same dense layout), one 32x32 (co, ci) tile of
// one tap per block: rule(off) reads, updates and writes element `off` and returns the new p, which goes out as w_fwd at once
// and as w_dgr transposed through LDS -- instead of torch's multi-pass foreach update plus a separate pack.
template <class Rule>
__device__ __forceinline__ void update_pack_tile(const Rule& rule, int Cout, int Cin, int Kw, const pack_out& o) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32, kw = blockIdx.z;
    for (int j = ty; j < 32; j += 8) {
        const int co = co0 + j, ci = ci0 + tx;
        float v = 0.f;
        if (co < Cout && ci < Cin) {
            const int64_t off = ((int64_t)kw * Cout + co) * Cin + ci;
            v = rule(off);
            if (o.fwd_hi) put_split(o.fwd_hi, o.fwd_lo, off, v);
            if (o.fwd_q) o.fwd_q[off] = quant_bf16_e4m3(v, o.q_scale);
        }
        tile[j][tx] = v;
    }
    __syncthreads();
    if (o.dgr_hi) {
        for (int j = ty; j < 32; j += 8) {
            const int ci = ci0 + j, co = co0 + tx;
            if (co < Cout && ci < Cin) {
                const int64_t off = ((int64_t)(Kw - 1 - kw) * Cin + ci) * Cout + co;
                put_split(o.dgr_hi, o.dgr_lo, off, tile[tx][j]);
                if (o.dgr_q) o.dgr_q[off] = quant_bf16_e4m3(tile[tx][j], o.q_scale);
            }
        }
    }
}

// torch.optim.SGD (dampening 0): g += wd*p; m = first ? g : mu*m + g; g = nesterov ? g + mu*m : m; p -= lr*g.
// 24 B per parameter: read p, g, m; write p, m, 2 x bf16.
template <bool CLIP>
struct sgd_rule {
    float *p, *g, *m;
    int first;
    float lr, mu, wd;
    int nesterov, zero_grad;
    grad_reader<CLIP> read;
    __device__ __forceinline__ float operator()(int64_t off) const {
        float pv = p[off];
        float gv = read(g[off]);
        gv = gv + wd * pv;
        if (zero_grad) g[off] = 0.f;       // the buffer comes back as the next step's (split-K, atomically accumulated) dW
        float mv = first ? gv : mu * m[off] + gv;
        m[off] = mv;
        gv = nesterov ? gv + mu * mv : mv;
        pv -= lr * gv;
        p[off] = pv;
        return pv;
    }
};
template <bool CLIP>
__global__ void sgd_pack_kernel(float* p, float* g, float* m, int first, float lr, float mu, float wd,
                                int nesterov, int zero_grad, int Cout, int Cin, int Kw, bf16_raw* fwd_hi, bf16_raw* fwd_lo,
                                bf16_raw* dgr_hi, bf16_raw* dgr_lo, uint8_t* fwd_q, uint8_t* dgr_q, float q_scale,
                                const float* clip) {
    const sgd_rule<CLIP> rule{p, g, m, first, lr, mu, wd, nesterov, zero_grad, grad_reader<CLIP>(clip)};
    update_pack_tile(rule, Cout, Cin, Kw, pack_out{fwd_hi, fwd_lo, dgr_hi, dgr_lo, fwd_q, dgr_q, q_scale});
}

// torch.optim.Adam / AdamW (adam_update): 32 B per parameter where SGD moves 24 -- read p, g, m, v; write p, m, v, 2 x bf16.
template <bool CLIP>
struct adam_rule {
    float *p, *g, *m, *v;
    int zero_grad;
    adam_scalars s;
    grad_reader<CLIP> read;
    __device__ __forceinline__ float operator()(int64_t off) const {
        const float gv = read(g[off]);
        if (zero_grad) g[off] = 0.f;
        float mv = m[off], vv = v[off];
        const float pv = adam_update(s, p[off], gv, mv, vv);
        m[off] = mv;
        v[off] = vv;
        p[off] = pv;
        return pv;
    }
};
template <bool CLIP>
__global__ void adam_pack_kernel(float* p, float* g, float* m, float* v, const float* dyn, float beta1, float beta2, float eps,
                                 float wd, int decoupled, int zero_grad, int Cout, int Cin, int Kw, bf16_raw* fwd_hi,
                                 bf16_raw* fwd_lo, bf16_raw* dgr_hi, bf16_raw* dgr_lo, uint8_t* fwd_q, uint8_t* dgr_q,
                                 float q_scale, const float* clip) {
    const adam_rule<CLIP> rule{p, g, m, v, zero_grad, adam_load_scalars(dyn, beta1, beta2, eps, wd, decoupled),
                               grad_reader<CLIP>(clip)};
    update_pack_tile(rule, Cout, Cin, Kw, pack_out{fwd_hi, fwd_lo, dgr_hi, dgr_lo, fwd_q, dgr_q, q_scale});
}

// ---- Novograd (novograd.py:86-112): per-TENSOR second moment v = EMA of ||g||^2 --------------------------------
// Three launches per conv weight: deterministic partial sums of g^2, a one-block finalize that updates v (first-step
// select on the device, optional running max) and leaves denom = sqrt(v) + eps in device memory, and the update fused
// with the bf16 operand pack:  g' = g/denom + wd*p;  g' *= (1-beta1) if grad_averaging;  m = beta1*m + g';  p -= lr*m.
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* g, int64_t n, float* partial) {
    __shared__ float red[256];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = g[i];
        s += v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void novograd_finalize_kernel(const float* partial, int nblocks, float beta2, float eps,
                                                                float* v, float* vmax, float* denom) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = red[0];
        const float old = v[0];
        float nv = old == 0.f ? norm : beta2 * old + (1.f - beta2) * norm;      // novograd.py:92-95
        v[0] = nv;
        if (vmax) {                                                             // amsgrad: novograd.py:97-102
            nv = fmaxf(vmax[0], nv);
            vmax[0] = nv;
        }
        denom[0] = sqrtf(nv) + eps;
    }
}

struct novograd_rule {
    float* p;
    const float* g;
    float* m;
    float dn, lr, beta1, wd;
    int grad_averaging;
    __device__ __forceinline__ float operator()(int64_t off) const {
        float pv = p[off];
        float gv = g[off] / dn;
        if (wd != 0.f) gv += wd * pv;
        if (grad_averaging) gv *= 1.f - beta1;
        const float mv = beta1 * m[off] + gv;
        m[off] = mv;
        pv -= lr * mv;
        p[off] = pv;
        return pv;
    }
};
__global__ void novograd_pack_kernel(float* p, const float* g, float* m, const float* denom, float lr, float beta1, float wd,
                                     int grad_averaging, int Cout, int Cin, int Kw, bf16_raw* fwd_hi, bf16_raw* fwd_lo,
                                     bf16_raw* dgr_hi, bf16_raw* dgr_lo) {
    const novograd_rule rule{p, g, m, denom[0], lr, beta1, wd, grad_averaging};
    update_pack_tile(rule, Cout, Cin, Kw, pack_out{fwd_hi, fwd_lo, dgr_hi, dgr_lo, nullptr, nullptr, 1.f});
}

// ---- small parameters: one launch over a device table -------------------------------------------------------------------------
// grid = (items, chunks of SGD_SMALL_CHUNK elements): most items are one chunk (a few hundred channels); the classifier weight
// (29 x 1024) is fifteen -- one block walking it alone took 96 us on the caller's stream at every step boundary.
// update(it, i, g) applies the rule to element i of item `it`, whose gradient, read through the clip, is g.
constexpr int SGD_SMALL_CHUNK = 2048;
template <bool CLIP, class Item, class Update>
__device__ __forceinline__ void small_multi_walk(const Item* items, const float* clip, const Update& update) {
    const Item it = items[blockIdx.x];
    const int lo = blockIdx.y * SGD_SMALL_CHUNK, hi = min(it.n, lo + SGD_SMALL_CHUNK);
    const grad_reader<CLIP> read(clip);
    for (int i = lo + threadIdx.x; i < hi; i += 256) update(it, i, read(it.g[i]));
}
// torch.optim.SGD's update of one small parameter (bias, BatchNorm gamma / beta): g' = g + wd p;  m = mu m + g' (dampening 0);
// p -= lr (nesterov ? g' + mu m : m).  No momentum buffer (m null): p -= lr g'.
template <bool CLIP>
__global__ __launch_bounds__(256) void sgd_small_multi_kernel(const w2l_sgd_small_t* items, float lr, float mu, float wd, int nesterov,
                                                              const float* clip) {
    small_multi_walk<CLIP>(items, clip, [=](const w2l_sgd_small_t& it, int i, float gv) {
        float pv = it.p[i];
        if (wd != 0.f) gv += wd * pv;
        float step = gv;
        if (it.m != nullptr) {
            const float mv = mu * it.m[i] + gv;
            it.m[i] = mv;
            step = nesterov ? gv + mu * mv : mv;
        }
        it.p[i] = pv - lr * step;
    });
}
// torch.optim.Adam / AdamW's update of one small parameter (adam_update)
template <bool CLIP>
__global__ __launch_bounds__(256) void adam_small_multi_kernel(const w2l_adam_small_t* items, const float* dyn, float beta1, float beta2,
                                                               float eps, float wd, int decoupled, const float* clip) {
    const adam_scalars s = adam_load_scalars(dyn, beta1, beta2, eps, wd, decoupled);
    small_multi_walk<CLIP>(items, clip, [=](const w2l_adam_small_t& it, int i, float gv) {
        float mv = it.m[i], vv = it.v[i];
        const float pv = adam_update(s, it.p[i], gv, mv, vv);
        it.m[i] = mv;
        it.v[i] = vv;
        it.p[i] = pv;
    });
}
// the step-dependent scalars of one parameter group, advanced on the device: running products (not pow), so that a host
// loop of the same double multiplies reproduces pow1 / pow2 bit for bit; the quotients formed in fp64 and rounded once
__global__ void adam_tick_kernel(w2l_adam_state_t* st, float* dyn, double lr, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double p1 = st->pow1 * beta1, p2 = st->pow2 * beta2;
    st->step += 1;
    st->pow1 = p1;
    st->pow2 = p2;
    dyn[W2L_ADAM_LR] = (float)lr;
    dyn[W2L_ADAM_STEP_SIZE] = (float)(lr / (1.0 - p1));
    dyn[W2L_ADAM_BC2_SQRT] = (float)sqrt(1.0 - p2);
    dyn[3] = 0.f;
}

// ---- host: one launcher per kernel shape -------------------------------------------------------------------------------------
// `plain` without a clip buffer, `clipped` with one; the kernel's arguments are head..., then what is checked here, then clip
template <class Kernel, class... Head>
int launch_update_pack(const char* name, Kernel plain, Kernel clipped, int Cout, int Cin, int Kw, void* w_fwd_hi, void* w_fwd_lo,
                       void* w_dgr_hi, void* w_dgr_lo, void* w_fwd_q, void* w_dgr_q, float q_scale, const float* clip, void* stream,
                       Head... head) {
    W2L_CHECK_ARG((!w_fwd_q && !w_dgr_q) || (q_scale > 0.f && w_fwd_hi && w_dgr_hi), "%s: e4m3 operands need a scale", name);
    W2L_CHECK_ARG(Cout > 0 && Cin > 0 && Kw > 0, "%s: bad sizes", name);
    W2L_CHECK_ARG(!(w_fwd_lo && !w_fwd_hi) && !(w_dgr_lo && !w_dgr_hi), "%s: lo without hi", name);
    dim3 grid((Cin + 31) / 32, (Cout + 31) / 32, Kw), block(32, 8);
    hipLaunchKernelGGL(clip ? clipped : plain, grid, block, 0, (hipStream_t)stream, head..., Cout, Cin, Kw, (bf16_raw*)w_fwd_hi,
                       (bf16_raw*)w_fwd_lo, (bf16_raw*)w_dgr_hi, (bf16_raw*)w_dgr_lo, (uint8_t*)w_fwd_q, (uint8_t*)w_dgr_q, q_scale,
                       clip);
    W2L_CHECK_LAUNCH();
    return 0;
}
// the kernel's arguments are items_dev, hp..., clip
template <class Kernel, class Item, class... Hp>
int launch_small_multi(const char* name, Kernel plain, Kernel clipped, const Item* items_dev, int nitems, int max_n, const float* clip,
                       void* stream, Hp... hp) {
    W2L_CHECK_ARG(items_dev != nullptr || nitems == 0, "%s: null table", name);
    W2L_CHECK_ARG(max_n >= 0 && max_n <= (1 << 26), "%s: max_n (the largest item's element count) out of range", name);
    if (nitems <= 0 || max_n == 0) return 0;
    const int chunks = (max_n + SGD_SMALL_CHUNK - 1) / SGD_SMALL_CHUNK;
    hipLaunchKernelGGL(clip ? clipped : plain, dim3(nitems, chunks), dim3(256), 0, (hipStream_t)stream, items_dev, hp..., clip);
    W2L_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" int w2l_sgd_pack(float* p, float* g, float* m, int first_step, float lr, float momentum,
                            float weight_decay, int nesterov, int zero_grad, int Cout, int Cin, int Kw, void* w_fwd_hi,
                            void* w_fwd_lo, void* w_dgr_hi, void* w_dgr_lo, void* w_fwd_q, void* w_dgr_q, float q_scale,
                            void* stream) {
    W2L_CHECK_ARG(p && g && m, "sgd_pack: null pointer");
    return launch_update_pack("sgd_pack", sgd_pack_kernel<false>, sgd_pack_kernel<true>, Cout, Cin, Kw, w_fwd_hi, w_fwd_lo, w_dgr_hi,
                              w_dgr_lo, w_fwd_q, w_dgr_q, q_scale, nullptr, stream, p, g, m, first_step, lr, momentum, weight_decay,
                              nesterov, zero_grad);
}

extern "C" int w2l_sgd_pack_clip(float* p, float* g, float* m, int first_step, float lr, float momentum,
                                 float weight_decay, int nesterov, int zero_grad, int Cout, int Cin, int Kw, void* w_fwd_hi,
                                 void* w_fwd_lo, void* w_dgr_hi, void* w_dgr_lo, void* w_fwd_q, void* w_dgr_q, float q_scale,
                                 const float* clip, void* stream) {
    W2L_CHECK_ARG(p && g && m && clip, "sgd_pack_clip: null pointer");
    return launch_update_pack("sgd_pack_clip", sgd_pack_kernel<false>, sgd_pack_kernel<true>, Cout, Cin, Kw, w_fwd_hi, w_fwd_lo,
                              w_dgr_hi, w_dgr_lo, w_fwd_q, w_dgr_q, q_scale, clip, stream, p, g, m, first_step, lr, momentum,
                              weight_decay, nesterov, zero_grad);
}

extern "C" int w2l_adam_pack(float* p, float* g, float* m, float* v, const float* dyn, float beta1, float beta2, float eps,
                             float weight_decay, int decoupled, int zero_grad, int Cout, int Cin, int Kw, void* w_fwd_hi,
                             void* w_fwd_lo, void* w_dgr_hi, void* w_dgr_lo, void* w_fwd_q, void* w_dgr_q, float q_scale,
                             const float* clip, void* stream) {
    W2L_CHECK_ARG(p && g && m && v && dyn, "adam_pack: null pointer");
    W2L_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "adam_pack: betas in [0, 1), eps >= 0");
    return launch_update_pack("adam_pack", adam_pack_kernel<false>, adam_pack_kernel<true>, Cout, Cin, Kw, w_fwd_hi, w_fwd_lo,
                              w_dgr_hi, w_dgr_lo, w_fwd_q, w_dgr_q, q_scale, clip, stream, p, g, m, v, dyn, beta1, beta2, eps,
                              weight_decay, decoupled, zero_grad);
}

extern "C" int w2l_novograd_pack(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                                 float* scratch, int scratch_floats, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, int grad_averaging, int Cout, int Cin, int Kw, void* w_fwd_hi,
                                 void* w_fwd_lo, void* w_dgr_hi, void* w_dgr_lo, void* stream) {
    W2L_CHECK_ARG(p && g && exp_avg && exp_avg_sq && scratch, "novograd_pack: null pointer");
    W2L_CHECK_ARG(Cout > 0 && Cin > 0 && Kw > 0 && scratch_floats >= 2, "novograd_pack: bad sizes");
    W2L_CHECK_ARG(!(w_fwd_lo && !w_fwd_hi) && !(w_dgr_lo && !w_dgr_hi), "novograd_pack: lo without hi");
    const int64_t n = (int64_t)Cout * Cin * Kw;
    int nblocks = (int)((n + 256 * 16 - 1) / (256 * 16));          // ~16 elements per thread
    if (nblocks > scratch_floats - 1) nblocks = scratch_floats - 1;
    if (nblocks > 1024) nblocks = 1024;
    if (nblocks < 1) nblocks = 1;
    hipStream_t st = (hipStream_t)stream;
    float* denom = scratch;                                         // scratch = [denom | partial sums]
    float* partial = scratch + 1;
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nblocks), dim3(256), 0, st, g, n, partial);
    W2L_CHECK_LAUNCH();
    hipLaunchKernelGGL(novograd_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nblocks, beta2, eps, exp_avg_sq,
                       max_exp_avg_sq, denom);
    W2L_CHECK_LAUNCH();
    dim3 grid((Cin + 31) / 32, (Cout + 31) / 32, Kw), block(32, 8);
    hipLaunchKernelGGL(novograd_pack_kernel, grid, block, 0, st, p, g, exp_avg, denom, lr, beta1, weight_decay, grad_averaging,
                       Cout, Cin, Kw, (bf16_raw*)w_fwd_hi, (bf16_raw*)w_fwd_lo, (bf16_raw*)w_dgr_hi, (bf16_raw*)w_dgr_lo);
    W2L_CHECK_LAUNCH();
    return 0;
}

extern "C" int w2l_sgd_small_multi(const w2l_sgd_small_t* items_dev, int nitems, int max_n, float lr, float momentum,
                                   float weight_decay, int nesterov, void* stream) {
    return launch_small_multi("sgd_small_multi", sgd_small_multi_kernel<false>, sgd_small_multi_kernel<true>, items_dev, nitems,
                              max_n, nullptr, stream, lr, momentum, weight_decay, nesterov);
}
extern "C" int w2l_sgd_small_multi_clip(const w2l_sgd_small_t* items_dev, int nitems, int max_n, float lr, float momentum,
                                        float weight_decay, int nesterov, const float* clip, void* stream) {
    W2L_CHECK_ARG(clip != nullptr, "sgd_small_multi_clip: null clip buffer");
    return launch_small_multi("sgd_small_multi_clip", sgd_small_multi_kernel<false>, sgd_small_multi_kernel<true>, items_dev, nitems,
                              max_n, clip, stream, lr, momentum, weight_decay, nesterov);
}
extern "C" int w2l_adam_small_multi(const w2l_adam_small_t* items_dev, int nitems, int max_n, const float* dyn, float beta1,
                                    float beta2, float eps, float weight_decay, int decoupled, const float* clip, void* stream) {
    W2L_CHECK_ARG(dyn != nullptr, "adam_small_multi: null dyn buffer");
    W2L_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "adam_small_multi: betas in [0, 1), eps >= 0");
    return launch_small_multi("adam_small_multi", adam_small_multi_kernel<false>, adam_small_multi_kernel<true>, items_dev, nitems,
                              max_n, clip, stream, dyn, beta1, beta2, eps, weight_decay, decoupled);
}
// NOT in the replay table: the one call of an optimizer step whose arguments change from step to step
extern "C" int w2l_adam_tick(w2l_adam_state_t* state_dev, float* dyn_dev, double lr, double beta1, double beta2, void* stream) {
    W2L_CHECK_ARG(state_dev != nullptr && dyn_dev != nullptr, "adam_tick: null pointer");
    W2L_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_tick: betas in [0, 1)");
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_dev, dyn_dev, lr, beta1, beta2);
    W2L_CHECK_LAUNCH();
    return 0;
}

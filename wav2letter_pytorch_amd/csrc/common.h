// Shared device/host helpers for the gfx950 (MI355X / CDNA4) kernels of the
// Wav2Letter / Jasper fwd + CTC + bwd hot path.  gfx950 only: 64-wide waves,
// v_mfma_f32_16x16x32_bf16, global_load_lds_dwordx4, ds_read_b64_tr_b16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

// measure-and-pick (the _tune entry points): the first pass ranks every candidate on `reps` launches, then the kFinalists fastest
// are timed again, interleaved, kFinalRounds x 4 reps launches each (round 5: 5 x 3 x 4 reps instead of 3 x 2 x 2 reps -- the first pass's ranking
// moves by more than the best candidates differ, and a mis-pick costs the step 0.5-1 % per layer)
constexpr int kFinalists = 5, kFinalRounds = 3;
typedef unsigned short bf16_raw;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

#define W2L_WAVE 64

__device__ __forceinline__ float bf16_bits_to_f32(bf16_raw v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_raw f32_to_bf16_bits(float f) {
    __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    return __builtin_bit_cast(unsigned short, b);
}
// hi/lo split used by the "split-bf16" (near-fp32) mode: f ~= hi + lo, |f-hi-lo| <= 2^-17 |f|
__device__ __forceinline__ void f32_split_bf16(float f, bf16_raw& hi, bf16_raw& lo) {
    hi = f32_to_bf16_bits(f);
    lo = f32_to_bf16_bits(f - bf16_bits_to_f32(hi));
}

// one value -> its place in a bf16 operand buffer: hi, and lo where the split-bf16 mode keeps one
__device__ __forceinline__ void put_split(bf16_raw* hi, bf16_raw* lo, int64_t off, float v) {
    bf16_raw h, l;
    f32_split_bf16(v, h, l);
    hi[off] = h;
    if (lo) lo[off] = l;
}
// one float -> one OCP e4m3 byte (round to nearest even, saturating at +-448)
__device__ __forceinline__ uint8_t quant1_e4m3(float v) {
    v = fminf(fmaxf(v, -448.f), 448.f);
    return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xFF);
}

// ---- slots of the float[4] gradient-clip buffer, as in include/w2l_hip.h (w2l_grad_sqnorm_multi / w2l_grad_clip_value write
// it; the update kernels of optim.hip read it) ----
#ifndef W2L_CLIP_NORM
#define W2L_CLIP_NORM 0
#define W2L_CLIP_COEF 1
#define W2L_CLIP_BOUND 2
#endif

// ---- error reporting across the C ABI (no exceptions, no exit) ----
void w2l_set_error(const char* fmt, ...);
#define W2L_CHECK_ARG(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            w2l_set_error(__VA_ARGS__);          \
            return 1;                            \
        }                                        \
    } while (0)
#define W2L_CHECK_HIP(expr)                                                             \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            w2l_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return (int)_e;                                                             \
        }                                                                               \
    } while (0)
#define W2L_CHECK_LAUNCH() W2L_CHECK_HIP(hipGetLastError())

// the start / stop events of a measuring entry point: destroyed on every return path
struct W2lEventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int create() {
        W2L_CHECK_HIP(hipEventCreate(&e0));
        W2L_CHECK_HIP(hipEventCreate(&e1));
        return 0;
    }
    ~W2lEventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// ---- diagnostic hook points.  Empty here, i.e. in every shipped build; tools/ablate_igemm.py and tools/stamp_wgrad.py build
// experiment libraries that force-include csrc/diag/hooks.h, which defines bodies for them first. ----
#ifndef W2L_DIAG_SKIP_DMA
#define W2L_DIAG_SKIP_DMA(p)
#endif
#ifndef W2L_DIAG_SKIP_FRAGS
#define W2L_DIAG_SKIP_FRAGS(p, stp)
#endif
#ifndef W2L_DIAG_SKIP_MFMA
#define W2L_DIAG_SKIP_MFMA(p)
#endif
#ifndef W2L_DIAG_CLK_BEGIN
#define W2L_DIAG_CLK_BEGIN()
#define W2L_DIAG_CLK_END(tid)
#endif
#ifndef W2L_DIAG_IGEMM_EXPORTS
#define W2L_DIAG_IGEMM_EXPORTS
#endif
#ifndef W2L_DIAG_STAMP_DECL
#define W2L_DIAG_STAMP_DECL()
#define W2L_DIAG_STAMP_STEP0()
#define W2L_DIAG_STAMP_STEP1()
#define W2L_DIAG_STAMP_STEP2()
#define W2L_DIAG_STAMP_STEP3()
#define W2L_DIAG_STAMP_LOOP_BEGIN()
#define W2L_DIAG_STAMP_STORE(lane, slot_expr)
#endif
#ifndef W2L_DIAG_WGRAD_EXPORTS
#define W2L_DIAG_WGRAD_EXPORTS
#endif
#ifndef W2L_DIAG_WGRAD_TAPS
#define W2L_DIAG_WGRAD_TAPS 2
#endif

// raise a kernel's dynamic-LDS limit to the full 160 KiB of a gfx950 CU (idempotent, cheap)
hipError_t w2l_allow_big_lds(const void* kernel);

// XCD-aware bijective block remap (8 XCDs, round-robin dispatch): consecutive
// logical tiles land on the same XCD so they share that XCD's private L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

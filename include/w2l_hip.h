/*
 * w2l_hip.h -- C ABI of libw2l_hip.so: the MI355X (gfx950) kernels under the
 * Wav2Letter / Jasper forward + CTC + backward training step.
 *
 * The reference (assafmu/wav2letter_pytorch) is 100% Python and has no native
 * interface of its own; every entry point below replaces the torch ATen op the
 * reference calls at the cited site.  A binding only needs plain pointers and
 * sizes (ctypes stub: wav2letter_pytorch_amd/_lib.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - activations are channels-last "NTC" [N][rows][C] with C the padded channel
 *     count (multiple of 64, pad channels are zero); bf16 unless stated;
 *   - `stream` is a hipStream_t passed as void*; all launches are asynchronous on
 *     it, nothing synchronises, nothing is allocated or freed;
 *   - return 0 on success, otherwise a hipError_t / 1 for bad arguments, with a
 *     message retrievable through w2l_last_error() (thread-local);
 *   - re-entrant: may be called concurrently from the Python main thread
 *     (forward) and autograd worker threads (backward).
 */
#ifndef W2L_HIP_H
#define W2L_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* w2l_last_error(void);
int w2l_abi_version(void);            /* 2 (1 -> 2: w2l_bnact_t gained the trailing field q_clipped).  It counts struct
                                       * layouts, not symbols: adding or removing an entry point does not change it */

/* ---- layout / packing ---------------------------------------------------- */

/* fp32 weights w[co][ci][kw] (arbitrary element strides) ->
 *   w_fwd  [Kw][CoutP][CinP] bf16 (hi, and lo = residual if w_fwd_lo != NULL)
 *   w_dgr  [Kw][CinP][CoutP] bf16 with taps flipped: w_dgr[k][ci][co] = w[co][ci][Kw-1-k]
 * pad rows/cols are zero.  Replaces nothing in the reference; it is the operand
 * layout for nn.Conv1d (wav2letter.py:35-36, jasper.py:96-105). */
int w2l_pack_weights(const float* w, int64_t s_co, int64_t s_ci, int64_t s_kw, int Cout, int Cin, int Kw,
                     int CoutP, int CinP, void* w_fwd_hi, void* w_fwd_lo, void* w_dgr_hi, void* w_dgr_lo,
                     void* stream);

/* (csrc/optim.hip, like every entry point that applies an update rule)
 * torch.optim.SGD(momentum, nesterov, weight_decay; dampening 0) -- configuration/optimizer/exp_lr_optimizer.yaml:2-7
 * -- fused with w2l_pack_weights for a tap-major conv weight: p, g, m are dense fp32 [Kw][Cout][Cin];
 * first_step != 0 initialises the momentum buffer with the (decayed) gradient as torch does.  The bf16
 * outputs are the operands of the next step (no channel padding: Cout, Cin multiples of 64).  zero_grad != 0 writes
 * zeros back into g once it has been read: the buffer can then serve as the next step's dw without a fill launch
 * (split-K weight gradients accumulate with atomics into a zeroed buffer, see w2l_wgrad_needs_zero).  w_fwd_q / w_dgr_q
 * (optional, fp8 mode): the same two operands once more as e4m3 bytes, value * q_scale, so that the forward and the data
 * gradient of the next step need no quantisation pass over the weights. */
int w2l_sgd_pack(float* p, float* g, float* m, int first_step, float lr, float momentum, float weight_decay,
                 int nesterov, int zero_grad, int Cout, int Cin, int Kw, void* w_fwd_hi, void* w_fwd_lo, void* w_dgr_hi,
                 void* w_dgr_lo, void* w_fwd_q, void* w_dgr_q, float q_scale, void* stream);

/* input spectrogram fp32 [N][C][T] -> padded NTC bf16 [N][pad_l+T+pad_r][CP];
 * pad_mode 1 = reflect (nn.ReflectionPad1d, wav2letter.py:28-34,41), 0 = zeros
 * (Conv1d padding=, jasper.py:96-105).  lens (optional, [N] int32): rows t >= lens[n]
 * are zeroed first (MaskedConv1d, jasper.py:114-119). */
int w2l_nct_to_ntc(const float* x, int N, int C, int T, int CP, int pad_l, int pad_r, int pad_mode,
                   const int32_t* lens, void* out_hi, void* out_lo, void* stream);

/* "Shared-halo" gradient layout used for every dy buffer: rows = halo + N*(T + halo):
 *   [halo zero rows][utt 0: T rows][halo zero rows][utt 1: T rows] ... [utt N-1][halo zero rows]
 * One zero gap serves as trailing halo of utterance n and leading halo of n+1, so the data-gradient
 * convolution can run over the whole buffer as ONE long sequence (no per-utterance tile rounding) while
 * the weight-gradient kernel still sees zero rows after each utterance.
 *
 * fp32 dense [N][T][C] -> shared-halo bf16 [halo + N*(T+halo)][CP] (+ optional lo), and per-channel
 * column sums colsum[CP] (bias gradient of an un-normalised conv: the 1x1 classifier,
 * wav2letter.py:69, jasper.py:432-433). */
int w2l_pad_cast(const float* g, int N, int T, int C, int CP, int halo, void* out_hi, void* out_lo, float* colsum,
                 void* stream);

/* ---- Conv1d as implicit GEMM on MFMA (nn.Conv1d fwd: wav2letter.py:42, jasper.py:127;
 *      its dgrad: autograd of the same call sites) ---------------------------------
 * y[n][t][co] (+)= bias[co] + sum_{kw,ci} w[kw][co][ci] * xp[n][t*stride + kw*dil][ci]
 * xp is a physically padded buffer (reflect or zero halo written by the producer);
 * x_rows_total = number of rows of Cin elements readable from xp (reads are clamped).
 * y is dense [N][Tout][Cout] bf16 (y_f32=0) or fp32 (y_f32=1; accumulate=1 adds to y).
 * stats_partial (optional) [w2l_conv_stat_tiles(N,Tout)][2][Cout]: per column-tile sums of y
 * and y^2 over valid t (BatchNorm batch statistics, wav2letter.py:37,43).
 * dgrad = the same call with xp := zero-haloed dy, w := w_dgr, Cin<->Cout, stride 1. */
int w2l_conv_stat_tiles(int N, int Tout);
int w2l_conv1d_igemm(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y, int y_f32,
                     int accumulate, const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout,
                     int Kw, int stride, int dil, void* stream);

/* Autotune: time every feasible block shape for this exact problem on the caller's device (HIP events on
 * `stream`, SYNCHRONISING) and remember the fastest for later w2l_conv1d_igemm calls of the same shape.
 * Call once per shape during warm-up; no-op when already tuned.  The output is written like a normal
 * accumulate=0 launch. */
int w2l_conv1d_igemm_tune(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y, int y_f32,
                          const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout, int Kw, int stride,
                          int dil, int reps, void* stream);

/* The same two entry points with a split-K workspace (device memory, owned by the caller, >= 64 KiB, ZERO-FILLED once
 * when it is allocated; one workspace per stream of execution -- launches that may overlap must not share it).  With
 * it, the tuner may split the (chunk, tap) reduction of a tile over 2-8 blocks where one block per tile would leave CUs
 * idle (a partly filled last round -- the flat data gradient has N*(T + halo) rows, never a round number of tiles -- or
 * small batches with fewer tiles than CUs): partial tiles go through fp32 slabs in the workspace, the block that draws a
 * tile's last ticket sums them in split order (bit-reproducible) and runs the normal epilogue; no block waits for another.
 * w2l_conv_splitk_workspace_bytes: a size with which every configuration of the problem is available (any smaller size
 * just removes the split configurations that do not fit). */
int w2l_conv1d_igemm_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y, int y_f32,
                        int accumulate, const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout, int Kw,
                        int stride, int dil, void* splitk_ws, int64_t splitk_ws_bytes, void* stream);
int w2l_conv1d_igemm_tune_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, void* y, int y_f32,
                             const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout, int Kw, int stride,
                             int dil, int reps, void* splitk_ws, int64_t splitk_ws_bytes, void* stream);
int64_t w2l_conv_splitk_workspace_bytes(int N, int Cout, int Tout);
/* Stream-K configurations (indices 52 * 7 .. 52 * 8 - 1 of w2l_conv_force_tile_config; the tuner measures them beside the
 * split-K ones wherever one block per tile fills the chip's last round badly): the launch is one block per resident slot,
 * block r works on steps [W*r/G, W*(r+1)/G) of the tile-major (tile, step) space -- every block the same number of MFMA
 * steps whatever the tile count -- and a tile cut by a range boundary is combined like a split-K tile (slabs summed in
 * range order by the block that draws the tile's last ticket: deterministic).  Returns G for this problem and workspace,
 * 0 where the launch would fall back to one block per tile. */
int w2l_conv_streamk_ranges(int idx, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int64_t ws_bytes);
/* the decomposition itself, run on the host by the same function the kernel runs: the pieces of `tiles` x `steps` over G
 * ranges in range order, out[7 * i] = range, tile, first step, end step, ranges sharing the tile, place among them, slab id
 * (-1: whole tile, no slab); returns the piece count or -1 (cap too small / sizes beyond the kernel's 32-bit arithmetic) */
int w2l_conv_streamk_pieces(int tiles, int steps, int G, int* out, int cap);

/* nn.Conv1d forward (wav2letter.py:35-36,42 / jasper.py:96-105) on OCP e4m3 operands -- BASELINE config 5 "fp8 MFMA":
 *   y[n][t][co] = descale * sum_{kw,ci} wq[kw][co][ci] * xq[n][t + kw*dil][ci] (+ bias[co]),
 * xq / wq one byte per element, same layouts as the bf16 entry point (x_bstride in elements), Cin a multiple of 128,
 * stride 1; the products run on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (2x the bf16 MFMA rate), fp32
 * accumulate; descale = 1 / (activation scale * weight scale) undoes the producers' per-tensor scaling (descale_dev, optional:
 * a further factor read from device memory -- the inverse scale w2l_quantize_e4m3_dyn derived from a device-side amax, as
 * for the data gradient, where xq is the e4m3 copy of dy and wq the flipped-tap operand).  Output bf16 or
 * fp32, optional BatchNorm partial statistics as w2l_conv1d_igemm.  The _tune form measures the block shapes once per
 * shape (synchronising; warm-up only). */
int w2l_conv1d_igemm_fp8(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq, void* y, int y_f32,
                         float descale, const float* descale_dev, const float* bias, float* stats_partial, int N, int Cin,
                         int Cout, int Tout, int Kw, int dil, void* stream);
int w2l_conv1d_igemm_fp8_tune(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq, void* y, int y_f32,
                              const float* bias, float* stats_partial, int N, int Cin, int Cout, int Tout, int Kw, int dil,
                              int reps, void* stream);

/* tuning hook: force configuration idx (>= 0) for every later w2l_conv1d_igemm call MADE BY THE CALLING THREAD (the
 * setting is thread-local: launches from other threads are never affected); -1 = automatic.
 * idx = block shape (0..25) + 26 * K-loop structure (0: barrier at the top of a step, 1: barrier mid-step)
 *       + 52 * split option (0..6: 1, 2, 3, 4, 5, 6, 8 blocks per tile through the split-K workspace; 7: stream-K).
 * A call whose problem the forced configuration cannot run returns an error and launches nothing: block shape 20 (it
 * spills; kept for index stability), a shape whose tiles do not fit LDS, stride 2 on any shape but 128x128 (index 2),
 * statistics on tile rows (w2l_conv_stats_mode(0)) with a shape that is not 128 or 256 columns wide.  A split option the
 * problem or the workspace cannot carry (fewer than two K steps per block, no workspace) silently runs one block per tile,
 * and so does stream-K under a fused epilogue or where its ranges would be shorter than eight steps: w2l_conv_plan(forced
 * idx) tells what a launch really gets (out[2] blocks per tile, out[3] stream-K blocks). */
void w2l_conv_force_tile_config(int idx);
/* likewise for the e4m3 kernel: idx = index into its list of 15 block shapes; an infeasible one (statistics need 128-row
 * tiles, LDS) makes w2l_conv1d_igemm_fp8 fail with a message */
void w2l_conv_force_fp8_config(int idx);
/* Host-only plan query: what a launch of this problem would be given, decided by the very function the launches go through
 * -- no stream, no buffer, no GPU.  stats_flag as in the tune cache's key: 0 none, 1 statistics rows per 128-column tile, 2
 * statistics added onto slot rows (w2l_conv_stats_mode), 3 the fused inference epilogue.  ws_bytes: the split-K workspace the
 * launch would bring (0: none).  forced_idx < 0: the remembered (tuned / loaded) choice, else the cost model's; >= 0: as under
 * w2l_conv_force_tile_config / w2l_conv_force_fp8_config.  out[8] = configuration index, K-loop structure, blocks per tile,
 * stream-K blocks (0: one block per tile and split), grid blocks, block threads, LDS bytes, feasible.  Returns 0 with
 * out[7] = 1, or nonzero with out = {-1, 0, ...} and the reason in w2l_last_error. */
int w2l_conv_plan(int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int stats_flag, int64_t ws_bytes,
                  int forced_idx, int* out);
int w2l_conv_plan_fp8(int N, int Cin, int Cout, int Tout, int Kw, int dil, int stats_flag, int forced_idx, int* out);

/* Conv1d weight gradient (autograd of the same call sites):
 * dw[kw][co][ci] (+)= sum_{n,t} dy[n][t][co] * xp[n][t*stride + kw*dil][ci]
 * dy: bf16, pointer at utterance 0 row 0, dy_bstride elements between utterances; rows
 * [Tout, roundup(Tout,64)) of every utterance must be zero (shared-halo layout with halo >= that).
 * dw fp32 [Kw][Cout][Cin].  accumulate=1 adds to dw: where ONE block owns an element -- every unsplit plan and every plan
 * that reduces through slabs (classic split or dealt) -- with a plain read-add-store, once per element, so the result is
 * bit for bit fp32(dw_before + what accumulate=0 stores under the same plan); fp32 atomics only where several blocks add
 * into an element (an atomic split, the pieces of a stream-K launch; with accumulate=1 every stream-K tile is a piece).
 * xp: bf16, x_bstride elements between utterances, x_rows_total rows readable from xp on (the kernel clamps the rows its 64-row
 * steps and tap groups stage beyond that onto the last one; they only ever meet zero dy rows or taps >= Kw).
 * Refused with a message, nothing launched (the single and the group launches alike, per layer): dy_bstride / Cout < Tout
 * ("dy_bstride holds ..."), and x_rows_total < (N-1) * x_bstride / Cin + (Tout-1) * stride + (Kw-1) * dil + 1, the last row a
 * live product reads ("padded input too small") -- a shorter buffer would be clamped onto its last row and give a wrong
 * gradient.
 *
 * The ladder of entry points.  The GENERAL calls are w2l_conv1d_wgrad_ws (launch), w2l_conv1d_wgrad_tune_x (measure) and
 * w2l_wgrad_needs_zero_x (query); the others are shorthands of them:
 *   w2l_conv1d_wgrad         = _ws without a workspace
 *   w2l_conv1d_wgrad_tune_ws = _tune_x with flags 0;   w2l_conv1d_wgrad_tune = _tune_ws without a workspace
 *   w2l_wgrad_needs_zero_ws  = _needs_zero_x of a stride-1, dilation-1 layer;   w2l_wgrad_needs_zero = that without a workspace
 * The library may split the (n,t) reduction over blocks.  Without a workspace the partial tiles are combined with fp32
 * atomics: where the needs_zero query says so, the caller must zero-fill dw first (also with accumulate=0).  With a
 * workspace (device memory owned by the caller, >= 64 KiB, zero-filled once when allocated; one per stream of execution;
 * w2l_wgrad_workspace_bytes covers every classic split) the partial tiles go through fp32 slabs and the block that draws a
 * tile's last ticket sums them in split order and writes dw with plain stores -- no atomics, no zero-filled dw,
 * bit-reproducible gradients.  A workspace too small for the chosen split falls back to the atomic path.
 * Dealt stream-K (plan bit 5, the plan's count = the number of ranges G) needs the workspace too
 * (w2l_wgrad_dealt_workspace_bytes): the (tile, K step) space of the launch is cut into G equal ranges, one per resident
 * block slot (512 / 256), so the chip is full whatever the tile count.  A range crosses at most one tile boundary; each of
 * its one or two segments is a block of its own (the kernel stays the one-segment kernel): the first G blocks take the first
 * segments, the following blocks the second segments LONGEST FIRST, so the slot that frees first gets the longest remainder.
 * Partial tiles go through slabs, the last arriver of a tile sums them in range order: no atomics, bit-reproducible.  A
 * launch without the workspace (or of a shape without a dealt form) falls back to an atomic split of 2.
 * w2l_conv1d_wgrad_tune_x flags: bit 0 = classic split / stream-K plans are measured and run with fp32 atomics although a
 * workspace is given (plan bit 6) -- the workspace then only serves dealt plans.
 *
 * Host-only queries (no GPU needed, not replayable):
 * w2l_wgrad_plan: the plan a launch of this shape starts from (forced, measured, or the cost model's), before it is narrowed
 * to the layer: form bits (see w2l_wgrad_force_plan) | split / range count << 8.
 * w2l_wgrad_launch_plan: what a launch of this problem runs as -- the counterpart of w2l_conv_plan.  Forcing is an argument
 * (forced_splits 0 / forced_order -1: automatic); the per-thread hook is neither read nor touched.  out[W2L_WGRAD_PLAN_FIELDS]:
 * split count, K steps per split, K steps per utterance, K steps in all, block order, stream-K, two tap groups, 32x32x16,
 * three taps, taps per wave, taps per block, tap groups, tiles, dealt ranges G (0: not dealt), second-segment blocks, slabs,
 * atomic, needs_zero, x window rows in LDS, LDS bytes, grid x, grid y, block threads, 1.  A refused launch: nonzero return,
 * out all 0.
 * w2l_wgrad_dealt_segments (testing): the blocks of a dealt launch in launch order, six ints each (range, tile,
 * first step, end step, place among the tile's segments, number of them); returns the block count, -1: no dealt form. */
int w2l_conv1d_wgrad_ws(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride, int64_t x_rows_total, float* dw,
                        int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int accumulate, void* ws,
                        int64_t ws_bytes, void* stream);
int w2l_conv1d_wgrad(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride, int64_t x_rows_total,
                     float* dw, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int accumulate,
                     void* stream);
int w2l_conv1d_wgrad_tune_x(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride, int64_t x_rows_total,
                            float* dw_scratch, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int reps,
                            void* ws, int64_t ws_bytes, int flags, void* stream);
int w2l_conv1d_wgrad_tune_ws(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride, int64_t x_rows_total,
                             float* dw_scratch, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int reps,
                             void* ws, int64_t ws_bytes, void* stream);
int w2l_wgrad_needs_zero_x(int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int64_t ws_bytes);
int w2l_wgrad_needs_zero_ws(int N, int Cin, int Cout, int Tout, int Kw, int64_t ws_bytes);
int w2l_wgrad_needs_zero(int N, int Cin, int Cout, int Tout, int Kw);
int64_t w2l_wgrad_workspace_bytes(int Cin, int Cout, int Kw);
int64_t w2l_wgrad_dealt_workspace_bytes(int Cin, int Cout, int Kw);
int w2l_wgrad_plan(int N, int Cin, int Cout, int Tout, int Kw);
#define W2L_WGRAD_PLAN_FIELDS 24
int w2l_wgrad_launch_plan(int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int64_t ws_bytes, int forced_splits,
                          int forced_order, int* out);
int w2l_wgrad_dealt_segments(int tiles, int steps, int ranges, int* out, int max_blocks);

/* A GROUP of layers' weight gradients in ONE launch (round 5): layers of the same N, Tout, stride 1 and dilation (any Cin,
 * Cout, Kw) whose [128 co x 128 ci] x tap-group tiles form one pool of equal-shaped work items -- layers whose own tile
 * count fills a fraction of the chip's block slots fill whole rounds together, with no split, no partial tiles, no atomics
 * and no zero-filled dw (plain stores, accumulate = 0).  form = the block form (plan order bits 0: block order inside a
 * layer, 2: two tap groups per 8-wave block, 3: 32x32x16 fragments, 4: three taps per wave with AGPR accumulators).
 * Operand layouts per item as for w2l_conv1d_wgrad.  w2l_wgrad_group_tiles: the number of tiles a layer adds to the pool.
 * Replaces the weight half of aten::convolution_backward for several nn.Conv1d call sites at once
 * (wav2letter.py:35-36,42 / jasper.py:96-105,127). */
typedef struct {
    const void* dy;
    int64_t dy_bstride;
    const void* xp;
    int64_t x_bstride;
    int64_t x_rows_total;
    float* dw;
    int Cin, Cout, Kw, pad_;
} w2l_wgrad_item_t;
#define W2L_WGRAD_GROUP_MAX 8
int w2l_conv1d_wgrad_group(const w2l_wgrad_item_t* items, int nitems, int N, int Tout, int dil, int form, void* stream);
int w2l_wgrad_group_tiles(int Cin, int Cout, int Kw, int form);

/* Testing / profiling hook: pin the split count (0 = automatic; a dealt plan: the range count) and the plan order (-1 =
 * automatic; bit 5 = dealt stream-K, bit 6 = atomics although a workspace is given, see above; bit 0 = block order,
 * bit 1 = stream-K decomposition, bit 2 = two tap groups per 8-wave block, bit 3 = 32x32x16 MFMA tiles, bit 4 = THREE taps
 * per wave with the 192 accumulator registers in AGPRs (stride 1, dilation <= 4; alone: two 4-wave blocks per CU, with bit
 * 2: one 8-wave block of six taps per CU -- the kernels of csrc/conv_wgrad3_dev.hip, a code object of their own embedded in
 * the library); a combination the shape does not admit falls back to the nearest built variant) for launches made by the
 * calling thread (thread-local, like w2l_conv_force_tile_config). */
void w2l_wgrad_force_plan(int splits, int order);
/* W2L_DETERMINISTIC=1 (engine.py): on != 0 makes every later launch of w2l_conv1d_wgrad_ws (and w2l_wgrad_needs_zero_x) ignore
 * plan bit 6, i.e. a split reduction handed a workspace goes through slabs summed in a fixed order whatever the measured plan
 * (or a plan cache written by a default-mode run) says: bit-reproducible weight gradients.  Process-wide, not thread-local:
 * the weight gradients are launched from autograd's worker threads. */
void w2l_wgrad_deterministic(int on);

/* Autotune of the split-K factor and block order, like w2l_conv1d_igemm_tune (SYNCHRONISING, warm-up only); dw_scratch is a
 * throw-away [Kw][Cout][Cin] fp32 buffer.  Call before w2l_wgrad_needs_zero() / w2l_conv1d_wgrad for the shape. */
int w2l_conv1d_wgrad_tune(const void* dy, int64_t dy_bstride, const void* xp, int64_t x_bstride, int64_t x_rows_total,
                          float* dw_scratch, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil, int reps,
                          void* stream);

/* fp8 mode (BASELINE config 5): the weight gradient on OCP e4m3 operands, v_mfma_scale_f32_16x16x128_f8f6f4 with
 * ds_read_b64_tr_b8 fragment reads (stride 1; conv_wgrad_fp8.hip).  dyq / xq: the one-byte copies of dy and of the padded
 * input that the fp8 step already holds (w2l_quantize_e4m3_dyn / w2l_bn_act_fwd_q), same row layouts as the bf16 entry
 * point (batch strides in elements = bytes); dw = descale * (*descale_dev, if given) * sum dyq * xq, fp32, tap-major.
 * Rows the kernel reads: it walks every utterance in ceil(Tout / 128) steps of 128 frames, WITHOUT a clamp on dy, so
 *   dyq  rows [0, 128 * ceil(Tout / 128)) of every utterance are read (the last utterance's included: the buffer must hold them);
 *        rows [Tout, that) must be ZERO bytes.  dy_bstride must hold at least that many rows (the shared-halo layout with
 *        halo >= roundup(Tout, 128) - Tout does); a shorter one is refused.
 *   xq   the rows beneath them, t + kw*dil for every walked t, clamped onto row x_rows_total - 1: they run on into the next
 *        utterance's rows (or whatever follows) and meet zero dy rows there, so every byte of them must be a FINITE e4m3 code
 *        (the NaN codes 0x7F / 0xFF times zero would put NaN into dw).
 * Split-K partial tiles are added atomically: w2l_wgrad_fp8_needs_zero tells whether dw must be zero-filled; accumulate = 1 on
 * such a plan adds onto what dw holds (no zero fill then), on an unsplit plan it is a plain read-add-store.
 * Replaces aten::convolution_backward's weight half (wav2letter.py:35-36,42 / jasper.py:96-105,127) in that mode. */
int w2l_wgrad_fp8_needs_zero(int N, int Cin, int Cout, int Tout, int Kw);
int w2l_conv1d_wgrad_fp8(const void* dyq, int64_t dy_bstride, const void* xq, int64_t x_bstride, int64_t x_rows_total,
                         float* dw, int N, int Cin, int Cout, int Tout, int Kw, int dil, float descale,
                         const float* descale_dev, int accumulate, void* stream);
int w2l_conv1d_wgrad_fp8_tune(const void* dyq, int64_t dy_bstride, const void* xq, int64_t x_bstride, int64_t x_rows_total,
                              float* dw_scratch, int N, int Cin, int Cout, int Tout, int Kw, int dil, int reps, void* stream);

/* Persistence of the measured choices of w2l_conv1d_igemm_tune / w2l_conv1d_wgrad_tune (a small text file; the
 * analogue of a vendor library's find-db).  save: 0 on success.  load: number of entries taken, -1 on error; lines
 * that do not describe a feasible launch of THIS build are skipped. */
int w2l_tune_save(const char* path);
int w2l_tune_load(const char* path);

/* ---- depthwise Conv1d, groups == channels (nn.Conv1d inside MaskedConv1d, jasper.py:96-105,127,319-330) ----
 * weights fp32 tap-major w[k][c]; activations channels-last bf16 hi [+ lo]; fp32 arithmetic; HBM-bound.
 * fwd:   y[n][t][c] = sum_k w[k][c] * xp[n][t*stride + k*dil][c]; frames t >= lens[n] are written as 0
 *        (the next MaskedConv1d's masked_fill).  xp: [N][x_rows][C] zero-padded by the producer.
 * dgrad: dxp[n][v][c] = sum_k w[k][c] * dy[n][v - k*dil][c] (stride 1), v in [0, Tp); dy [N][dy_rows][C] with
 *        Tout valid frames, frames >= lens[n] count as 0.
 * wgrad: dw[k][c] += sum_{n, t < min(Tout, lens[n])} dy[n][t][c] * xp[n][t*stride + k*dil][c] (fp32 atomics into
 *        a zero-filled dw). */
int w2l_dwconv_fwd(const void* x_hi, const void* x_lo, int x_rows, const float* w, void* y_hi, void* y_lo, int N, int Tout,
                   int C, int K, int stride, int dil, const int32_t* lens, void* stream);
int w2l_dwconv_dgrad(const void* dy, int dy_f32, int dy_rows, const float* w, void* dxp, int dxp_f32, int N, int Tp, int Tout,
                     int C, int K, int dil, const int32_t* lens, void* stream);
int w2l_dwconv_wgrad(const void* dy, int dy_f32, int dy_rows, const void* x_hi, const void* x_lo, int x_rows, float* dw, int N,
                     int Tout, int C, int K, int stride, int dil, const int32_t* lens, void* stream);

/* ---- BatchNorm1d + Dropout + activation (wav2letter.py:43-46, jasper.py:363,376,448) ---- */

/* partial [ntiles][2][C] -> batch mean / biased var -> scale = gamma*invstd, shift = beta - mean*scale;
 * running stats updated with the UNBIASED variance: r = (1-momentum)*r + momentum*batch.
 * If partial == NULL (eval mode) scale/shift come from the running stats. */
int w2l_bn_finalize(const float* partial, int ntiles, int C, int64_t count, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                    float* scale, float* shift, void* stream);

typedef struct {
    int32_t N, T, C;        /* valid rows per utterance; padded channel count */
    const void* y;          /* conv output, dense [N][T][C] */
    int32_t y_f32;          /* 0: bf16, 1: fp32 */
    const float* scale;     /* NULL => identity (no BatchNorm) */
    const float* shift;
    const float* mean;      /* backward only */
    const float* invstd;
    const void* y2;         /* optional residual branch (jasper.py:400-410), same layout/dtype as y */
    const float* scale2;
    const float* shift2;
    const float* mean2;
    const float* invstd2;
    int32_t act;            /* 0 none, 1 clamp[0,20] (wav2letter.py:46), 2 ReLU (jasper.py:448) */
    float drop_p;           /* nn.Dropout p; 0 => no mask is read or written */
    uint64_t seed, offset;  /* Philox4x32-10 key / stream offset */
    uint8_t* mask;          /* keep bits, one byte per 8 channels: [N*T*C/8]; the forward pass does not write the bytes of
                               frames t >= lens[n] (written as zeros without being evaluated), the backward pass ignores them */
    const int32_t* lens;    /* optional [N]: rows t >= lens[n] produce 0 / receive 0 gradient */
    const uint64_t* offset_dev; /* optional device word ADDED to `offset` when the mask is drawn: a step counter that lives
                               in device memory, so that a captured hipGraph of the step draws fresh masks at every replay */
    uint64_t* q_clipped;    /* optional (w2l_bn_act_fwd_q with out_q): device counter incremented by the number of activation
                               elements whose e4m3 copy SATURATED (|a * q_scale| > 448): the per-tensor activation scales of
                               fp8 mode are fixed, so an unbounded activation (ReLU after a residual sum) clips silently
                               otherwise.  NULL: not counted.  (ABI version 2) */
} w2l_bnact_t;

/* a = act(dropout(y*scale+shift [+ y2*scale2+shift2])) written to a padded buffer
 * [N][pad_l+T+pad_r+tail][C] for the NEXT conv: halo rows are reflected copies (pad_mode 1) or zeros. */
int w2l_bn_act_fwd(const w2l_bnact_t* d, void* out_hi, void* out_lo, int out_rows, int pad_l, int pad_r,
                   int pad_mode, void* stream);
/* the same with a second copy of the padded activation as OCP e4m3 bytes, a * q_scale (saturating at +-448): the
 * forward operand of the next nn.Conv1d in fp8 mode (BASELINE config 5).  out_q == NULL: plain w2l_bn_act_fwd. */
int w2l_bn_act_fwd_q(const w2l_bnact_t* d, void* out_hi, void* out_lo, void* out_q, float q_scale, int out_rows,
                     int pad_l, int pad_r, int pad_mode, void* stream);
/* w2l_bn_finalize + w2l_bn_act_fwd(_q) in ONE launch (round 5; bf16 y, C a multiple of 64): every block first sums the
 * partial statistics rows of its own 64 channels and derives mean / invstd / scale / shift exactly as w2l_bn_finalize does;
 * the blocks of the first row range publish them (f->mean, invstd, scale, shift: the backward pass reads them) and update
 * the running statistics.  Meant for FEW partial rows: w2l_conv_stats_mode(S) makes the convolutions fold their per-tile
 * statistics onto S rows.  One record per branch (f2 iff d->y2); a record with partial == NULL takes scale / shift from the
 * descriptor (a branch without BatchNorm, or eval mode after w2l_bn_finalize).  The descriptor's own scale / shift pointers
 * are ignored for a branch with a record.  Same output contract as w2l_bn_act_fwd_q (out_lo: none, bf16 mode only).
 * Replaces nn.BatchNorm1d's statistics + normalisation + Dropout + clamp / ReLU (+ residual add, length mask, the next
 * convolution's reflect padding): wav2letter.py:28-34,37-38,43-46 / jasper.py:116-119,363,376,409-410,448. */
typedef struct {
    const float* partial;   /* [rows][2][C]: sums, sums of squares (w2l_conv1d_igemm* statistics rows) */
    int32_t rows;
    int64_t count;          /* N * T: elements per channel */
    const float* gamma;     /* NULL: 1 */
    const float* beta;      /* NULL: 0 */
    float eps, momentum;
    float* running_mean;    /* NULL: not tracked */
    float* running_var;
    float* mean;            /* outputs, [C] each (mean / invstd may be NULL) */
    float* invstd;
    float* scale;
    float* shift;
} w2l_bnfin_t;
int w2l_bn_act_fwd_fin(const w2l_bnact_t* d, const w2l_bnfin_t* f1, const w2l_bnfin_t* f2, void* out_hi, void* out_q,
                       float q_scale, int out_rows, int pad_l, int pad_r, int pad_mode, void* stream);
/* How the convolutions lay out their statistics rows, for launches made by the calling thread (thread-local, like
 * w2l_conv_force_tile_config): 0 (default) = one row per 128-column tile, plain stores (w2l_conv_stat_tiles rows,
 * bit-reproducible); S = 1..64: the per-tile sums are ADDED (fp32 atomics) onto row (tile mod S) of a [S][2][C] buffer the
 * caller zero-filled -- a handful of rows that w2l_bn_act_fwd_fin / w2l_bn_act_bwd_apply_fin re-reduce per block instead of
 * a finalize launch of their own.  Applies to w2l_conv1d_igemm*, w2l_conv1d_igemm_fp8 and w2l_conv1d_dgrad_bnreduce_ws.
 * With S > 0 the bf16 kernels may take ANY block shape for a launch with statistics (a block adds its whole tile's sums
 * onto row (column tile mod S)); with 0 only the shapes of 128 or 256 columns, whose waves line up with the 128-column rows. */
void w2l_conv_stats_mode(int slots);

/* dst[i] = e4m3(src[i] * scale), src bf16 (src_f32 = 0) or fp32, n a multiple of 8: per-tensor quantisation of the conv
 * weights (and of the spectrogram) for w2l_conv1d_igemm_fp8. */
int w2l_quantize_e4m3(const void* src, int src_f32, int64_t n, float scale, void* dst, void* stream);

typedef struct {
    const void* dxp;        /* gradient wrt the padded activation buffer [N][rows][C], bf16 or fp32; the first
                               pad_l+T+pad_r rows of each utterance are valid */
    int32_t f32;
    int32_t pad_l, pad_r, pad_mode;   /* fold reflected halo rows back (mode 1) or skip the halo (mode 0) */
    int32_t rows;           /* rows per utterance in dxp (>= pad_l+T+pad_r) */
} w2l_gradsrc_t;

/* sums over (n,t) of g and g*xhat per channel for each branch:
 * partial [nblocks][ncomp][C] = {sum g, sum g*xhat1 [, sum g (branch2), sum g*xhat2]}; ncomp = 4 with a residual
 * branch (d->y2 != NULL), else 2; nblocks = w2l_bn_bwd_blocks(). */
int w2l_bn_bwd_blocks(int N, int T, int C);
int w2l_bn_act_bwd_reduce(const w2l_bnact_t* d, const w2l_gradsrc_t* g1, const w2l_gradsrc_t* g2, float* partial,
                          void* stream);
/* partial -> sums [ncomp][C] (sum_g = d beta, sum_gx = d gamma), written at the front of a [4][C] buffer */
int w2l_bn_bwd_finalize(const float* partial, int nblocks, int C, int ncomp, float* sums, void* stream);
/* dy = scale*(g - sum_g/M - xhat*sum_gx/M) into shared-halo buffers [halo + N*(T+halo)][C] (hi[,lo]);
 * dy2 likewise for the residual branch (NULL if none).  The conv bias gradient under BatchNorm is
 * sum(dy) == 0 identically (the reference's value is fp32 rounding noise); it is not computed. */
int w2l_bn_act_bwd_apply(const w2l_bnact_t* d, const w2l_gradsrc_t* g1, const w2l_gradsrc_t* g2, const float* sums,
                         void* dy_hi, void* dy_lo, int halo, void* dy2_hi, void* dy2_lo, int halo2, void* stream);
/* w2l_bn_bwd_finalize + w2l_bn_act_bwd_apply(_amax) in ONE launch: every block re-reduces the partial rows of its own 64
 * channels (fixed order: all blocks of a slab get bit-identical sums), so the finalize launch on the backward critical path
 * disappears; sums [ncomp][C] (d beta, d gamma, as w2l_bn_bwd_finalize writes them) are published as a by-product.
 * partial = what w2l_bn_act_bwd_reduce or w2l_conv1d_dgrad_bnreduce_ws produced; amax optional as below. */
int w2l_bn_act_bwd_apply_fin(const w2l_bnact_t* d, const w2l_gradsrc_t* g1, const w2l_gradsrc_t* g2, const float* partial,
                             int nblocks, float* sums, void* dy_hi, void* dy_lo, int halo, void* dy2_hi, void* dy2_lo,
                             int halo2, float* amax, void* stream);
/* The backward chain in TWO launches (round 5; the fast path: bf16 y, bf16 gradient from one source, one branch, BatchNorm
 * present, C a multiple of 64 -- w2l_bn_bwd_fast_ok says whether a unit qualifies): w2l_bn_act_bwd_reduce_slots ADDS the sums
 * of g*gate and g*gate*xhat onto `slots` rows of a zero-filled partial [slots][2][C] (fp32 atomics, one 2 x 64 row segment
 * per 128-row block), w2l_bn_act_bwd_apply_slots re-reduces those rows per block (the finalize folded in; sums [2][C] = d
 * beta, d gamma published as by w2l_bn_bwd_finalize) and writes dy into its shared-halo buffer (halo rows zero-filled).  Both
 * issue every load of a wave's rows before the first use.  amax as for w2l_bn_act_bwd_apply_amax (row 0 only). */
int w2l_bn_bwd_fast_ok(const w2l_bnact_t* d, const w2l_gradsrc_t* g1, const w2l_gradsrc_t* g2);
int w2l_bn_act_bwd_reduce_slots(const w2l_bnact_t* d, const w2l_gradsrc_t* g1, float* partial, int slots, void* stream);
int w2l_bn_act_bwd_apply_slots(const w2l_bnact_t* d, const w2l_gradsrc_t* g1, const float* partial, int nrows, float* sums,
                               void* dy_hi, int halo, float* amax, void* stream);
/* the same, also leaving max |dy| and max |dy2| in device memory -- the scale of the e4m3 copy of dy that the data gradient
 * reads in fp8 mode.  amax is [2][W2L_AMAX_SLOTS] floats, zeroed by the caller: slot (block index mod W2L_AMAX_SLOTS) of row
 * 0 (dy) / row 1 (dy2) takes an integer atomic max of the bit patterns; the tensor's amax is the max over a row's slots
 * (one word per tensor would serialise every wave of the launch on one L2 address). */
#define W2L_AMAX_SLOTS 64
int w2l_bn_act_bwd_apply_amax(const w2l_bnact_t* d, const w2l_gradsrc_t* g1, const w2l_gradsrc_t* g2, const float* sums,
                              void* dy_hi, void* dy_lo, int halo, void* dy2_hi, void* dy2_lo, int halo2, float* amax,
                              void* stream);
/* dst[i] = e4m3(src[i] * s), s = 2^floor(log2(224 / max(amax[0..W2L_AMAX_SLOTS)))) read from DEVICE memory (no host round
 * trip; s = 1 when amax is 0); inv_scale[0] = 1 / s for the consumer (w2l_conv1d_igemm_fp8 descale_dev).  src bf16, n a multiple of 8. */
int w2l_quantize_e4m3_dyn(const void* src_bf16, int64_t n, const float* amax, void* dst, float* inv_scale, void* stream);

/* The data gradient of a stride-1 nn.Conv1d FUSED with w2l_bn_act_bwd_reduce of the layer that produced the conv's input
 * (d describes that layer: bf16 y, one branch).  dxp [flat_rows][d->C] bf16 is the gradient wrt the padded activation,
 * computed over the shared-halo dy buffer as one sequence exactly like w2l_conv1d_igemm_ws(N = 1, Tout = flat_rows, w =
 * the flipped-tap operand); row v of it is padded row v % per of utterance v / per (per >= pad_l + d->T + pad_r, and
 * flat_rows == d->N * per EXACTLY: a row beyond would be counted with the y, mask and lens of an utterance that does not
 * exist, so any other flat_rows is rejected).  The
 * epilogue, which holds that gradient in registers, also writes partial[tile][2][d->C] -- per 128-row tile
 * (w2l_conv_stat_tiles(1, flat_rows) rows) the sums of g*gate and g*gate*xhat, every padded row counted with the gate
 * and xhat of its source frame (itself, or its mirror under reflect padding) -- so the separate reduction pass over dxp
 * and y (and its launch on the backward critical path) disappears; w2l_bn_bwd_finalize(partial, tiles, C, 2, ...) follows.
 * Replaces the reduction half of autograd's batch_norm backward at wav2letter.py:43 / jasper.py:363. */
int w2l_conv1d_dgrad_bnreduce_ws(const void* dy, int64_t dy_rows_total, const void* w_dgr, void* dxp, float* partial,
                                 const w2l_bnact_t* d, int pad_l, int pad_r, int pad_mode, int per, int Cconv_out,
                                 int flat_rows, int Kw, int dil, void* splitk_ws, int64_t splitk_ws_bytes, void* stream);
/* measure-and-pick of the block shape for that launch (SYNCHRONISING; warm-up only) */
int w2l_conv1d_dgrad_bnreduce_tune_ws(const void* dy, int64_t dy_rows_total, const void* w_dgr, void* dxp, float* partial,
                                      const w2l_bnact_t* d, int pad_l, int pad_r, int pad_mode, int per, int Cconv_out,
                                      int flat_rows, int Kw, int dil, int reps, void* splitk_ws, int64_t splitk_ws_bytes,
                                      void* stream);

/* ---- inference: one launch per convolution unit --------------------------------------------------------------
 * nn.Conv1d + nn.BatchNorm1d in eval() (running statistics: a constant per-channel affine map) + the residual sum + the
 * activation + MaskedConv1d's length mask + the NEXT convolution's padding, all in the implicit GEMM's epilogue
 * (conv_igemm_kernel, EPI = 2).  On the fp32 accumulators, in this order:
 *   v = acc + bias[co] (+ acc_in[n][t][co]);  v = v * scale[co] + shift[co]   (scale = gamma * rsqrt(running_var + eps),
 *       shift = beta - running_mean * scale, as w2l_bn_finalize(partial = NULL) gives them; NULL: identity)
 *   v += res[n][t][co] (+ res_lo)           dense bf16 [N][Tout][Cout]: the other branch of a Jasper unit, written by a fused
 *                                           launch of its own with act = 0 and no padding
 *   v = clamp(v, 0, 20) (act 1) | max(v, 0) (act 2) | v (act 0);   v = 0 for t >= lens[n]
 *   out[n][pad_l + t][co] = bf16(v) (+ out_lo = bf16(v - hi)), out = [N][out_rows][Cout] with out_rows >= pad_l + Tout + pad_r.
 * Halo rows: pad_mode 1 (reflect) -- the block that owns frame j (1 <= j <= pad_l) also writes row pad_l - j, the owner of
 * frame Tout-1-j (1 <= j <= pad_r) row pad_l + Tout - 1 + j; pad_mode 0 -- rows [0, pad_l) and [pad_l + Tout, pad_l + Tout +
 * pad_r) are written as zeros.  Rows beyond pad_l + Tout + pad_r are not touched.  pad_l, pad_r <= 96.  No y, no statistics,
 * no mask is written.  acc_in (optional, fp32 dense [N][Tout][Cout]): partial sums of earlier plain launches -- in split-bf16
 * mode the first two products go through w2l_conv1d_igemm(y_f32 = 1) and the third launch is this one.
 * With a split-K workspace (the _ws forms; as for w2l_conv1d_igemm_ws) a tile's reduction may be split over 2-8 blocks: the
 * block that draws the tile's last ticket sums the slabs and runs the epilogue.  Stream-K plans are not candidates.  The _tune form measures the block shapes WITH the epilogue and remembers the fastest under
 * a key of its own (statistics flag 3 of the plan table), so fused and plain launches of one shape never share a choice.
 * The key is the problem shape only: it does not tell the epilogue's variants apart (residual operand, lo output, reflect
 * double stores, mask) -- the first variant measured decides the block shape for all of them -- and a launch with acc_in
 * (split-bf16 mode) is never measured: it takes the remembered choice or the cost model's.
 * Replaces, for inference, nn.Conv1d + nn.BatchNorm1d + Hardtanh-style clamp + nn.ReflectionPad1d (wav2letter.py:28-38,
 * 41-46) and MaskedConv1d + BatchNorm1d + the residual sum + ReLU (jasper.py:96-105,116-119,127,363,376,400-410,448). */
typedef struct {
    const float* scale;     /* [Cout] fp32, NULL => identity (a unit without BatchNorm) */
    const float* shift;
    const void* res;        /* optional second branch, dense bf16 [N][Tout][Cout] */
    const void* res_lo;     /* its lo half (split-bf16 mode), NULL otherwise */
    int32_t act;            /* 0 none, 1 clamp[0,20], 2 ReLU */
    const int32_t* lens;    /* optional [N] */
    void* out_hi;           /* [N][out_rows][Cout] bf16 (w2l_conv1d_igemm_bnact_fp8: NULL with an e4m3 output alone) */
    void* out_lo;           /* optional lo half */
    int32_t out_rows, pad_l, pad_r, pad_mode;
} w2l_bnact_epi_t;
int w2l_conv1d_igemm_bnact(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, const float* acc_in,
                           const float* bias, const w2l_bnact_epi_t* e, int N, int Cin, int Cout, int Tout, int Kw, int stride,
                           int dil, void* stream);
int w2l_conv1d_igemm_bnact_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, const float* acc_in,
                              const float* bias, const w2l_bnact_epi_t* e, int N, int Cin, int Cout, int Tout, int Kw,
                              int stride, int dil, void* splitk_ws, int64_t splitk_ws_bytes, void* stream);
int w2l_conv1d_igemm_bnact_tune_ws(const void* xp, int64_t x_bstride, int64_t x_rows_total, const void* w, const float* bias,
                                   const w2l_bnact_epi_t* e, int N, int Cin, int Cout, int Tout, int Kw, int stride, int dil,
                                   int reps, void* splitk_ws, int64_t splitk_ws_bytes, void* stream);

/* ---- inference on e4m3 operands: the same unit in the epilogue of the e4m3 implicit GEMM (conv_igemm_kernel, F8, EPI = 2) ----
 * xq / wq / descale as for w2l_conv1d_igemm_fp8 (stride 1, Cin % 128 == 0, Cout % 64 == 0); on the fp32 accumulators
 *   v = acc * descale + bias[co],  then the sequence of w2l_conv1d_igemm_bnact: scale / shift, + res (dense bf16), the
 *       activation, the length mask -- giving a, which is never rounded to bf16 on the way to the e4m3 copy
 *   out_q[n][pad_l + t][co] = e4m3(a * q_scale)   OCP e4m3 bytes [N][e->out_rows][Cout], round to nearest even, saturating at
 *                                                 +-448: the conversion of w2l_bn_act_fwd_q's out_q.  Optional; 16-byte aligned
 *   e->out_hi[n][pad_l + t][co] = bf16(a)         optional here (NULL when nothing reads the bf16 copy); one of the two is needed
 * Halo rows of both outputs follow e->pad_mode / pad_l / pad_r exactly as above (reflect: byte copies of the mirrored row; zero:
 * zero bytes), rows beyond pad_l + Tout + pad_r stay untouched, pad_l, pad_r <= 96.  e->out_lo, e->res_lo must be NULL (no
 * split-bf16 form), there is no acc_in, no split-K and no stream-K.  q_clipped (optional, device int64): the number of
 * elements with |a| > 448 / q_scale (frames only, halo copies not counted) is added to it, one atomic per block that saw any.
 * A lane's 4 channels are 4 bytes: 4 (2) consecutive 16-channel tiles are transposed among the 4 lanes of a frame so that the
 * stores are 16 (8) bytes per lane.  The _tune form measures the e4m3 block shapes WITH the epilogue and remembers the fastest
 * under statistics flag 3 of the e4m3 plan table ("igemmf8" lines of the tune file); it does not count saturations.  Four of the
 * e4m3 kernel's block shapes are not built in this form (their epilogue spills): 2x4x6x4, 2x4x8x4, 2x3x5x6, 2x3x6x6.
 * Replaces, for inference with precision='fp8', w2l_conv1d_igemm_fp8 + w2l_bn_finalize + w2l_bn_act_fwd_q. */
int w2l_conv1d_igemm_bnact_fp8(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq, float descale,
                               const float* bias, const w2l_bnact_epi_t* e, void* out_q, float q_scale, int64_t* q_clipped,
                               int N, int Cin, int Cout, int Tout, int Kw, int dil, void* stream);
int w2l_conv1d_igemm_bnact_fp8_tune(const void* xq, int64_t x_bstride, int64_t x_rows_total, const void* wq, const float* bias,
                                    const w2l_bnact_epi_t* e, void* out_q, float q_scale, int N, int Cin, int Cout, int Tout,
                                    int Kw, int dil, int reps, void* stream);

/* ---- log_softmax + CTC (wav2letter.py:86-87, jasper.py:469-473, base_asr_models.py:23,81,90) ---- */
/* logits fp32 [N][T][CP] (first C valid) -> out fp32 [N][T][C]; mode 0 log_softmax, 1 softmax */
int w2l_log_softmax_fwd(const float* logits, int N, int T, int C, int CP, int mode, float* out, void* stream);
/* grad wrt logits (dense [N][T][C]) from grad wrt out and out itself */
int w2l_log_softmax_bwd(const float* gout, const float* out, int N, int T, int C, int mode, float* glogits,
                        void* stream);
/* workspace bytes for w2l_ctc_loss */
int64_t w2l_ctc_workspace_bytes(int N, int T, int Smax);
/* nn.CTCLoss(blank, reduction='mean', zero_infinity): log_probs [N][T][C] fp32 (batch-major),
 * targets [N][Smax] int32 (padded), lengths int32 [N].  Outputs: nll[N] (0 where infinite and zero_infinity),
 * loss[1] = mean_n(nll_n / max(S_n,1)), grad [N][T][C] = d loss / d log_probs in torch's convention
 * (exp(lp) - posterior) * grad_scale / (N*max(S_n,1)), zero for t >= input_lengths[n]). */
int w2l_ctc_loss(const float* log_probs, const int32_t* targets, const int32_t* input_lengths,
                 const int32_t* target_lengths, int N, int T, int C, int Smax, int blank, int zero_infinity,
                 float* nll, float* loss, float* grad, void* workspace, void* stream);

/* ---- wildcard CTC: a target may say "here is speech the transcript has no text for" (W-CTC, Star Temporal Classification) ---- */
/* workspace bytes for w2l_wctc_loss: w2l_ctc_loss's alpha and beta plus the parsed rows (labels, gap flags, label counts) */
int64_t w2l_wctc_workspace_bytes(int N, int T, int Smax);
/* w2l_ctc_loss whose target rows may hold the wildcard id `star` (the Python layer passes star = C).  Row n is the first
 * R = target_lengths[n] (clamped to [0, Smax]) int32 entries of targets [N][Smax]; each is a label in [0, C) other than the
 * blank, or star.  Parsing (on the device, one block prefix count per row, no host synchronisation): the labels z_1..z_S are
 * the non-star entries in order; the gap flag w_i, i = 0..S, is 1 iff at least one star lies between z_i and z_{i+1} (w_0:
 * before z_1, w_S: after z_S); consecutive stars are one wildcard; a row of only stars has S = 0 and w_0 = 1.
 * States: CTC's L = 2S + 1 extended states, odd s the label z_{(s+1)/2}, even s the gap s/2.  Emissions: a label state
 * lp[t][z], a plain gap lp[t][blank], a wildcard gap (w = 1) the constant `penalty` <= 0 -- "any label or the blank, with
 * probability 1, times exp(penalty)" per frame.  Transitions: CTC's (s -> s, s-1 -> s, and s-2 -> s for odd s whose label
 * differs from the label two states back), so a wildcard gap between different labels may take zero frames, and between equal
 * labels at least one gap frame is needed, which for a wildcard gap may carry anything.  Start in states 0 and 1, end in L-1
 * and L-2: nll = -logsumexp(alpha_{Tn-1}(L-1), alpha_{Tn-1}(L-2)), loss[1] = mean_n(nll_n / max(S_n, 1)) -- S_n counts labels,
 * not stars.  With no star in a row this is w2l_ctc_loss value for value.  With stars the score is NOT a normalised
 * probability (one frame labelling is reached through more than one state path): nll may be negative.
 * grad [N][T][C] follows w2l_ctc_loss's convention (the gradient wrt the logits under lp = log_softmax(logits)): with
 * gamma_t(s) the state posterior, post(t,c) its sum over the non-wildcard states that emit c and omega_t its sum over the
 * wildcard gaps, grad = (exp(lp[t][c]) * (1 - omega_t) - post(t,c)) / (N * max(S_n, 1)); zero for t >= input_lengths[n]; it
 * sums to zero over c.  grad may be NULL.  zero_infinity as in w2l_ctc_loss.
 * status int32 [N]: 0 ok; 1 no finite path (nll +inf, or 0 under zero_infinity); 2 an entry that is neither a valid non-blank
 * label nor star -- that utterance gets nll, loss term and gradient 0.  Limits: C <= 64, Smax <= 4095; star != blank. */
int w2l_wctc_loss(const float* log_probs, const int32_t* targets, const int32_t* input_lengths,
                  const int32_t* target_lengths, int N, int T, int C, int Smax, int blank, int zero_infinity, int star,
                  float penalty, float* nll, float* loss, float* grad, int32_t* status, void* workspace, void* stream);

/* ---- CTC forced alignment: the offsets decoder.py:238 refuses for beam search, in the format of decoder.py:104-119 ---- */
/* workspace bytes for w2l_ctc_align: 0 while the back-pointers fit in LDS, else N * ceil(T / 16) * (states rounded up to the
 * block's) * 4; -1 if out of range */
int64_t w2l_ctc_align_workspace_bytes(int N, int T, int Smax);
/* The best CTC path of a given target (Viterbi form of w2l_ctc_loss's recursion), one workgroup per utterance, one launch.
 * x fp32 [N][T][A] contiguous: log-probabilities, or probabilities if !log_probs (one logf per emission read, log 0 = -inf);
 * input_lengths int32 [N] (NULL: all T).  Target row n is the int32 row at targets + n * target_stride, its length
 * target_lengths[n * length_stride] (clamped to [0, Smax]), so rank 0 of w2l_ctc_beam_search's out buffer is aligned in place
 * (labels: stride k * T; len: stride k, an empty slot's -1 reads as 0).  Over the L = 2 S + 1 extended states, in fp32,
 * score[t][s] = max(score[t-1][s], score[t-1][s-1], score[t-1][s-2] if ext[s] != ext[s-2] and s odd) + lp[t][ext[s]].  Ties: the
 * first of s, s-1, s-2 wins; at the end state L-2 wins a tie with L-1; a maximum of -inf stays -inf.  Outputs: score[N] (best
 * path log-probability, -inf unless status 0); status[N]: 0 ok, 1 no path of finite score, 2 a negative or NaN probability
 * in the utterance's frames or a target outside [0, A) or equal to blank; path[N][T]: the label emitted at each frame (-1
 * from input_lengths[n] on, and everywhere unless status 0); starts / ends [N][Smax]: first and last frame of each token's
 * own state (-1 beyond the target's length, and everywhere unless status 0).  Limits: T <= 32768, Smax <= 4095. */
int w2l_ctc_align(const float* x, const int32_t* input_lengths, const int32_t* targets, int64_t target_stride,
                  const int32_t* target_lengths, int64_t length_stride, int N, int T, int A, int Smax, int blank,
                  int log_probs, void* workspace, int64_t workspace_bytes, float* score, int32_t* status, int32_t* path,
                  int32_t* starts, int32_t* ends, void* stream);

/* ---- CTC forced alignment of one LONG recording to its whole transcript (alignment.ctc_forced_align_long,
 *      segmentation.align_transcript): w2l_ctc_align's definition for N = 1 beyond its limits, the trellis cut into time blocks
 *      of tb frames (one launch each, ordered by the stream alone) and state tiles of sb states (one workgroup each, with a
 *      halo of 2 tb states below its own).  Bit-equal to w2l_ctc_align wherever both take the shape.  DESIGN 8s ---- */
#define W2L_ALIGN_LONG_MAX_T (1 << 22)   /* frames */
#define W2L_ALIGN_LONG_MAX_S (1 << 20)   /* labels of the transcript */
#define W2L_ALIGN_LONG_MAX_TB 256        /* a forced tb: any multiple of 16 in 16 .. 256 */
#define W2L_ALIGN_LONG_MAX_SB 2048       /* a forced sb, the built tile widths: every multiple of 64 in 64 .. 2048 */
#define W2L_ALIGN_LONG_TB 64             /* the plan for tb = sb = 0: the measured winner (profiles/align_long_bench.txt) */
#define W2L_ALIGN_LONG_SB 128
/* workspace bytes for w2l_ctc_align_long: 16 (status words) + 2 * Lp * 4 (two columns) + T * 4 rounded up to 16 (the walked
 * states) + ceil(T / 16) * Lp * 4 (the moves), with Lp = 2 S + 1 rounded up to a multiple of sb.  tb = sb = 0: the library's
 * plan.  -1: T outside 1 .. W2L_ALIGN_LONG_MAX_T, S outside 0 .. W2L_ALIGN_LONG_MAX_S, or an invalid forced plan (only one of
 * tb, sb zero; tb not a multiple of 16 in 16 .. 256; sb not a multiple of 64 in 64 .. 2048) */
int64_t w2l_ctc_align_long_workspace_bytes(int T, int S, int tb, int sb);
/* x fp32 [T][A] contiguous (log-probabilities, or probabilities if !log_probs), targets int32 [S]; recurrence, tie rules,
 * statuses and outputs as w2l_ctc_align with N = 1 and all T frames valid: score[1], status[1], path[T], starts[S], ends[S].
 * workspace: device memory, 16-byte aligned, of at least the bytes above for the same (T, S, tb, sb); contents undefined
 * before and after.  2 + ceil(T / tb) + 2 launches and one 16-byte memset on `stream`, no host synchronisation. */
int w2l_ctc_align_long(const float* x, int T, int A, const int32_t* targets, int S, int blank, int log_probs, int tb, int sb,
                       void* workspace, int64_t workspace_bytes, float* score, int32_t* status, int32_t* path, int32_t* starts,
                       int32_t* ends, void* stream);
/* w2l_ctc_align_long (= phases 7) by parts, for measuring one part with the others' results in the workspace
 * (tools/bench_align_long.py): 1 the memset, init and the forward launches; 2 the back-trace; 4 the output kernel */
int w2l_ctc_align_long_phases(const float* x, int T, int A, const int32_t* targets, int S, int blank, int log_probs, int tb,
                              int sb, int phases, void* workspace, int64_t workspace_bytes, float* score, int32_t* status,
                              int32_t* path, int32_t* starts, int32_t* ends, void* stream);

/* ---- CTC keyword search: where in the posteriors a phrase is said, with a score (keyword_search.py; host model:
 *      keyword_scan_host / pick_hits_host).  No reference counterpart ---- */
/* The keywords of one call, packed by keyword_search.KeywordTable into n_blocks blocks of `width` lanes (64, 128, 256, 512 or
 * 1024), one lane per extended state c_1, blank, c_2, ..., c_S of a keyword (2 S - 1 states, S <= 255), keywords in their
 * given order and never split across blocks.  All three arrays are DEVICE memory; the entry point does not read them and the
 * kernels bound every index they take from them.  labels[b * width + i]: the label of a label state.  meta[b * width + i]:
 * -1 for a lane without a state, else keyword index << 4 | flags: 1 the keyword's first state, 2 its last, 4 the move from
 * two states below is allowed (a label state whose label differs from the previous label's), 8 a label state (else the blank
 * between two labels).  block_kw[b] .. block_kw[b + 1]: the keywords of block b. */
typedef struct {
    const int32_t* labels;     /* [n_blocks * width] */
    const int32_t* meta;       /* [n_blocks * width] */
    const int32_t* block_kw;   /* [n_blocks + 1] */
    int32_t n_blocks, width, n_keywords, reserved_;
} w2l_kws_table_t;
typedef struct { int32_t start, end; float score; } w2l_kws_hit_t;
/* workspace bytes for w2l_ctc_kws (the frame maxima, N * T floats, and N ints); -1 where there is no plan: N outside
 * 1..65535, T outside 1..32768, K outside 1..4096, max_hits outside 1..64 */
int64_t w2l_ctc_kws_workspace_bytes(int N, int T, int K, int max_hits);
/* x fp32 [N][T][A] contiguous: log-probabilities, or probabilities if !log_probs; input_lengths int32 [N] (NULL: all T, else
 * clamped to [0, T]); thr fp32 [K] (device).  With b[t] = max_a lp[t][a] and e[t][s] = lp[t][lab(s)] - b[t] (probabilities:
 * logf(x) - logf(b)), per keyword and frame, in fp32,
 *   D[t][s] = e[t][s] + max(D[t-1][s], D[t-1][s-1], D[t-1][s-2] if flag 4, 0 if flag 1 ("enter here")),
 * a candidate replacing the best so far on a strict > only, in that order; B[t][s] = the frame at which the winning path
 * entered (t for "enter"); a state at -inf has B = -1.  Three launches, selected by the mask `phases` (7: all; anything less
 * is for measuring one launch with the others' outputs in place): 1 the frame maxima and status; 2 the scan, which writes
 * end_score / end_start [N][K][T] = D / B of each keyword's last state (-inf / -1 from input_lengths[n] on); 4 the pick: up to
 * max_hits times the frame with end_score >= thr[k] whose segment [end_start, t] overlaps no accepted one of the same keyword,
 * best by (score descending, start ascending, end descending); hit_count [N][K], hits [N][K][max_hits] in start order (unused
 * slots: -1, -1, -inf).  status[N]: 0 ok; 2 a NaN, a negative probability or a frame without a finite maximum among the
 * utterance's frames, or a table label outside [0, A) or equal to blank (never used as an index): no hits, and the curves of
 * the keywords concerned are -inf / -1.  Argument errors launch nothing; w2l_last_error names ctc_kws. */
int w2l_ctc_kws(const float* x, const int32_t* input_lengths, int N, int T, int A, int blank, int log_probs,
                const w2l_kws_table_t* table, const float* thr, int max_hits, int phases, void* workspace,
                int64_t workspace_bytes, float* end_score, int32_t* end_start, int32_t* hit_count, w2l_kws_hit_t* hits,
                int32_t* status, void* stream);

/* ---- Auto Segmentation criterion: the loss of the Wav2Letter paper, which the reference replaces by CTC (its README,
 *      "Differences from article"; call site: base_asr_models.py:23,81,90 with model.criterion=asg, asg.ASGLoss) ---- */
/* workspace bytes for w2l_asg_loss (alpha and beta tables of both recursions, encoded targets, gradient slabs); -1 if out of
 * range: A > 64, Smax > 4095, T > 2^20 */
int64_t w2l_asg_workspace_bytes(int N, int T, int A, int Smax);
/* ASG loss and gradients.  x fp32 [N][T][A] (any real scores; batch-major), transitions fp32 [A][A] (g[i][j]: label j at frame t
 * after label i at frame t-1), targets int32 [N][Smax] RAW transcripts (padded), lengths int32 [N].  The targets are
 * repeat-encoded on the device: within a run of equal labels the 2nd, 4th, ... member becomes repeat_index.
 * loss_n = Z_full - Z_tgt: Z_full = logsumexp over all A^T frame paths of sum_t x[t][pi_t] + sum_{t>=1} g[pi_{t-1}][pi_t], Z_tgt
 * the same over the paths that read the encoded target with every label held for at least one frame.  An utterance with S = 0
 * or S > input_lengths[n] is infeasible: loss and gradient 0.  Outputs: nll[N]; loss[1] = mean_n(nll_n / max(S_n, 1))
 * (reduction 0) or sum_n nll_n (reduction 1); grad_x [N][T][A] and grad_trans [A][A] = d loss / d x, d loss / d transitions
 * (both or neither; NULL: the loss only), zero for t >= input_lengths[n], bit-reproducible (fixed summation order, no atomics);
 * status[N]: 0 ok, 1 infeasible, 2 a raw target equal to repeat_index or outside [0, A) (treated as infeasible; asg.ASGLoss
 * raises ValueError).  Three launches, no host synchronisation. */
int w2l_asg_loss(const float* x, const float* transitions, const int32_t* targets, const int32_t* input_lengths,
                 const int32_t* target_lengths, int N, int T, int A, int Smax, int repeat_index, int reduction, float* nll,
                 float* loss, float* grad_x, float* grad_trans, int32_t* status, void* workspace, int64_t workspace_bytes,
                 void* stream);
/* workspace bytes for w2l_asg_viterbi: one byte of back-pointer per (frame, label padded to 32 or 64); -1 if out of range */
int64_t w2l_asg_viterbi_workspace_bytes(int N, int T, int A);
/* The best frame path under the score of Z_full (max instead of logsumexp; asg.ASGDecoder.decode, in the place of
 * decoder.py:136's argmax): ties go to the lowest predecessor and to the lowest final label; with zero transitions it is the
 * per-frame argmax.  input_lengths int32 [N] (NULL: all T).  path int32 [N][T] (-1 from input_lengths[n] on), score[N] the
 * path's score (0 for an utterance without frames).  One launch, one wave per utterance. */
int w2l_asg_viterbi(const float* x, const float* transitions, const int32_t* input_lengths, int N, int T, int A,
                    void* workspace, int64_t workspace_bytes, int32_t* path, float* score, void* stream);

/* ---- greedy decode (decoder.py:136) + Levenshtein (decoder.py:49,60) ---- */
/* argmax over the last dim, ties -> lowest index (torch.max): probs fp32 [rows][C] -> idx int32 [rows] */
int w2l_argmax(const float* probs, int64_t rows, int C, int32_t* idx, void* stream);
/* ---- the word tables of the beam searches: an n-gram language model, a lexicon, a list of hotwords ---- */
/* Device tables of an ARPA model in reverse-suffix form (see ngram_lm.py).  Entry e of an n-gram: prob[e] (log10, NaN for a
 * context-only entry that suffix closure inserted), bo[e] (log10 backoff, 0 if none); a unigram's entry is its word id
 * (<unk> = 0, <s> = 1, </s> = 2).  The entry of h_2 h_1 w is ngram_vals[slot] where ngram_keys[slot] == (entry of h_1 w) << 32
 * | h_2 (open addressing, linear probing, w2l_ngram_lm_build's hash).  The spelling trie: trie_keys[slot] == node << 8 |
 * canonical label -> child node trie_vals[slot], root 0, trie_word[node] = the word id the node spells (-1: none).  Limits:
 * n_entries < 2^30, capacities powers of two in [16, 2^31], at most half full. */
typedef struct {
    const float* prob;
    const float* bo;
    const uint64_t* ngram_keys;
    const int32_t* ngram_vals;
    int64_t ngram_cap;
    const uint64_t* trie_keys;
    const int32_t* trie_vals;
    int64_t trie_cap;
    const int32_t* trie_word;
    int32_t n_entries;      /* prob / bo length */
    int32_t n_words;        /* vocabulary size (the unigram entries) */
    int32_t n_trie_nodes;   /* trie_word length */
} w2l_ngram_lm_t;
/* Insert n keys (each != ~0, distinct) with their values into an open-addressing table of cap slots (a power of two >= 2n),
 * one CAS per probe; the table is cleared first.  *dups (device int32, not cleared) counts keys found already present. */
int w2l_ngram_lm_build(const uint64_t* keys, const int32_t* vals, int64_t n, uint64_t* table_keys, int32_t* table_vals,
                       int64_t cap, int32_t* dups, void* stream);
/* The spelling trie of a lexicon, in the form and with the limits of w2l_ngram_lm_t's (built by w2l_ngram_lm_build):
 * trie_keys[slot] == node << 8 | canonical label -> child node trie_vals[slot], root 0; trie_word[node] >= 0 where the node
 * spells a whole word.  The trie of an n-gram model may be passed as it is. */
typedef struct {
    const uint64_t* trie_keys;
    const int32_t* trie_vals;
    int64_t trie_cap;
    const int32_t* trie_word;
    int32_t n_trie_nodes;   /* trie_word length */
} w2l_lexicon_t;
/* ---- CTC prefix beam search (decoder.py:147-267; beam_search.prefix_beam_search), optionally with a word n-gram language
 *      model (ngram_lm.ArpaLM; decoder.py:210-212 with lm_weigh), constrained to a lexicon (lexicon.Lexicon) and
 *      preferring hotwords (Lexicon.boost_chars).  One entry point: each of lm, lexicon and hotwords may be NULL,
 *      independently, and the call launches ctc_beam_search_kernel<lm != NULL, lexicon != NULL, hotwords != NULL> -- a NULL
 *      table is a search compiled without it, not the search with it at weight 0 ---- */
/* workspace bytes for w2l_ctc_beam_search: per utterance a trie of k*T+1 nodes and its intern table, plus with an LM of order
 * `order` (1..6; 0: no LM) a 64-byte LM state per trie node.  A lexicon and hotwords keep nothing per interned prefix (a beam
 * slot's trie node lives in LDS, and the node of a new member is found from its parent slot's).  -1 if out of range: N, T or
 * k < 1, k*T >= 2^29, order outside 0..6. */
int64_t w2l_ctc_beam_search_workspace_bytes(int N, int T, int k, int order);
/* One workgroup per utterance, one launch for the batch, masses as fp64 logs.  probs fp32 [N][T][A] contiguous: probabilities,
 * or log-probabilities if log_probs; sizes int32 [N] (NULL: T) = the frames decoded of each utterance.  label_info_host[A]:
 * bits 0-7 the first index of the label's character (duplicate labels: the first index wins), bit 8 the label's character
 * is the blank's, bit 9 it is a word character (\w), bit 10 a word separator ([\s|>]).  end_index: first index of end_char,
 * -1 if absent (a prefix ending in it is carried unchanged).  A frame extends with the labels whose probability is > prune
 * (lp > log(prune) for log input); ranking = mass * (words + 1)^beta, ties in the host's first-insertion order.
 * out (one buffer, one copy to the host): double score[N][k] (log of the ranking weight, -inf for an empty slot) |
 * int32 len[N][k] (-1: empty slot) | int32 status[N] (1: a probability was negative or NaN) | int32 labels[N][k][T]
 * (first label indices, the first len of each row valid); slot 0 is the best prefix.  Limits: 1 <= k <= 64, 1 <= A <= 128,
 * and the candidate tables (48 * k * (A + 1) + 8 * k * A bytes) fit in LDS beside 9 KB of fixed state: k=32 with A=64 is
 * 114 KB; an error otherwise.
 *
 * With at least one of the three tables: label_info_host bit 11 = the label's character is whitespace (only ' ' may be, an
 * error otherwise) and space_index = the first index of ' ' (-1: none) are read and checked; without any, neither is.
 *
 * lm (an order-`order` model, 1 <= order <= 6): each trie node carries an LM state (the last order-1 word ids and their
 * context backoffs, the float32 sum of the words closed so far, the spelling-trie node of the partial word: 0 empty, -1 left
 * the trie (scored as <unk>)), computed once when the node is interned.  The weight of member i, alpha * ln 10 * (log10 of
 * its words with </s>, float32 in ArpaLM.score's order), multiplies exactly one contribution: E(i, c)'s p * (pb + pnb) where
 * c is the space or end_char, c is not member i's last character and member i has a character other than ' '.  out is
 * followed by float lm_log10[N][k], the LM total of each result (0 for an empty slot or a string of spaces); 1.5 KB more of
 * static LDS.  lm NULL: alpha and order are ignored, out has no lm_log10 section, the workspace is that of order 0.
 *
 * lexicon: no mass is given to a string that leaves the word list.  A separator is the space or end_char; the partial word
 * of a string is what follows its last separator.  The extension of beam member i by label c that is not itself a beam
 * member takes part in the frame only if it is legal: c a separator and member i's partial word empty or a whole word, or c
 * another label and (partial word + c) a prefix of a word (one probe of the trie); otherwise it gets no mass, like a pruned
 * label.  complete_only != 0: out holds only the members of the final beam whose partial word is empty or a whole word, in
 * rank order, the other slots empty (all members if there is none).  512 bytes more of static LDS.  lexicon NULL:
 * complete_only is not read.
 *
 * hotwords: the spelling trie of a word list of its own (separate from lexicon's and from lm's).  h(s) = the characters of
 * the closed words of s (those followed by the space or end_char) that are hotwords, plus the characters of its partial word
 * while that is a non-empty prefix of a hotword (a provisional credit: it goes when the word leaves the trie or is closed as
 * something else).  The ranking weight becomes mass * (words + 1)^beta * exp(hotword_weight * h): the score written to out
 * includes hotword_weight * h; masses, the LM term, the prune, ties and the lexicon rule are untouched.  hotword_weight:
 * natural-log units per character, any finite real (an error otherwise); 0 gives the output of the search without hotwords.
 * One more trie probe per new candidate; 1.5 KB more of static LDS.  hotwords NULL: hotword_weight is not read.
 *
 * Argument errors (nothing is launched; w2l_last_error names ctc_beam_search): a table given with a NULL pointer in it, an
 * over-full table or a capacity that is no power of two, an order outside 1..6 with lm, a space_index that is not the first
 * index of a label, a whitespace label other than ' ', a non-finite weight, a workspace smaller than the query's answer. */
int w2l_ctc_beam_search(const float* probs, const int32_t* sizes, int N, int T, int A, const int32_t* label_info_host,
                        int blank, int end_index, int space_index, int k, double alpha, double beta, double prune,
                        int log_probs, const w2l_ngram_lm_t* lm, int order, const w2l_lexicon_t* lexicon,
                        int complete_only, const w2l_lexicon_t* hotwords, double hotword_weight, void* workspace,
                        int64_t workspace_bytes, void* out, void* stream);
/* ---- ASG prefix beam search and forced alignment (asg_beam.py; host restatements: asg_prefix_beam_search,
 *      asg_viterbi_align_host): what w2l_ctc_beam_search / w2l_ctc_align are to a CTC model, for a model trained with
 *      the ASG criterion (no blank; learned transitions; label repeat_index stands for "the previous letter again") ---- */
/* workspace bytes for w2l_asg_beam_search (per utterance: a trie of k*T+1 nodes of 12 bytes and its intern table, plus with an
 * LM of order `order` (1..6; 0: no LM) a 64-byte LM state per trie node); -1 if out of range: A outside 1..64, k outside
 * 1..64, T >= 2^24, k*T >= 2^29 or order outside 0..6 */
int64_t w2l_asg_beam_search_workspace_bytes(int N, int T, int A, int k, int order);
/* One workgroup per utterance, one launch for the batch, masses as fp64 natural logs.  x fp32 [N][T][A] contiguous (any real
 * scores), transitions fp32 [A][A] (g[i][j]: label j at frame t after label i at frame t-1), sizes int32 [N] (NULL: T).  A
 * hypothesis is an ENCODED label sequence (no two neighbours equal) with one mass, the log-sum over the frame paths that read
 * it: M_0((c)) = x[0][c]; at frame t a member e with last label l stays (M(e) + g[l][l] + x[t][l]) and is extended by every
 * c != l (M(e) + g[l][c] + x[t][c]; an extension that is no member but was a candidate of frame t-1 also keeps its own
 * M_{t-1} + g[c][c] + x[t][c]), log-added in beam order, labels ascending.  Label c takes part in frame t if x[t][c] >
 * log(prune) or it is the frame's first argmax (prune <= 0: every label).  Rank: M + beta * log(words + 1), the words of the
 * DECODED text (every repeat label read as the decoded character before it, a leading one dropped) counted as
 * w2l_ctc_beam_search counts them; ties in first-insertion order; the k best are the next beam.  No end character.
 * label_info_host[A]: bits 0-7, 9 and 10 as in w2l_ctc_beam_search.  out: that search's layout, double score[N][k] | int32
 * len[N][k] (-1: empty slot) | int32 status[N] (1: a NaN score or transition) | int32 labels[N][k][T] (ENCODED labels).
 * Limits: 1 <= k <= 64, 1 <= A <= 64 (k = 64 with A = 64 takes 138 KB of dynamic LDS beside 9 KB static).
 *
 * lm may be NULL; the call launches asg_beam_search_kernel<lm != NULL, false, false>.  With lm (tables, order, label_info_host bit 11 and
 * space_index as in w2l_ctc_beam_search, checked only here): a trie node's LM state spells its DECODED characters (an r after
 * a letter spells the letter again, an r after a space closes nothing, a leading r spells nothing).  The weight of member i,
 * alpha * ln 10 * (log10 of its text's words with </s>), is added to exactly one contribution: the extension of member i by
 * the space label, where member i's last decoded character is not the space and its text has a character other than ' '.
 * out is followed by float lm_log10[N][k].  lm NULL: space_index, alpha and order are ignored, out has no lm_log10 section,
 * the workspace is that of order 0.  Argument errors as in w2l_ctc_beam_search; w2l_last_error names asg_beam_search. */
int w2l_asg_beam_search(const float* x, const float* transitions, const int32_t* sizes, int N, int T, int A,
                        const int32_t* label_info_host, int repeat_index, int space_index, int k, double alpha, double beta,
                        double prune, const w2l_ngram_lm_t* lm, int order, void* workspace, int64_t workspace_bytes, void* out,
                        void* stream);
/* w2l_asg_beam_search with the two word lists of w2l_ctc_beam_search: each of lm, lexicon and hotwords may be
 * NULL, independently, and the call launches asg_beam_search_kernel<lm != NULL, lexicon != NULL, hotwords != NULL>.  It is a
 * second symbol, not a longer signature, because w2l_asg_beam_search has positional callers; that symbol is this call with
 * (NULL, 1, NULL, 0.0), so (NULL, NULL) here is byte for byte the older call.  w2l_asg_beam_search_workspace_bytes serves
 * both: a lexicon and hotwords keep nothing per trie node (a beam slot's states live in LDS, 2 KB more of static LDS for the
 * two).  With any table label_info_host bit 11 and space_index are read and checked as in w2l_ctc_beam_search.
 *
 * Words are spelled by DECODED characters: member i (last decoded label dec_i, -1 if none) extended by label c spells d = dec_i
 * if c is the repeat label, else c.  d < 0 (a leading repeat label) spells nothing: the extension is legal and carries its
 * parent's states.  Otherwise the lexicon node and the hotword walk step with d's canonical label as in w2l_ctc_beam_search;
 * the only separator is the space (there is no end character), and a repeat label after a space spells a second space, which
 * is legal.  lexicon: an extension that is not itself a beam member and leaves the word list gets no mass -- not the
 * extension term, not its own M_{t-1} term.  complete_only and hotwords / hotword_weight: as in w2l_ctc_beam_search (the
 * score written to out includes hotword_weight * h; weight 0 gives the output of the search without hotwords).
 *
 * The participation rule under a lexicon.  Without one, "x[t][c] > log(prune) or c is the frame's first argmax" keeps the beam
 * alive because every participating label can extend some member.  With one, every participating extension can be illegal
 * while no member's last label takes part.  So with lexicon != NULL, and only then, label c also takes part in frame t if
 * t == 0 (every label: any non-empty lexicon has a legal first label) or c is the last label of a member of the current beam
 * (every member can stay).  It is still one ascending set per frame, used for stays and extensions alike.
 *
 * Argument errors as in w2l_ctc_beam_search (nothing is launched); w2l_last_error names asg_beam_search. */
int w2l_asg_beam_search_tables(const float* x, const float* transitions, const int32_t* sizes, int N, int T, int A,
                               const int32_t* label_info_host, int repeat_index, int space_index, int k, double alpha,
                               double beta, double prune, const w2l_ngram_lm_t* lm, int order, const w2l_lexicon_t* lexicon,
                               int complete_only, const w2l_lexicon_t* hotwords, double hotword_weight, void* workspace,
                               int64_t workspace_bytes, void* out, void* stream);
/* workspace bytes for w2l_asg_align: 0 while the moves fit in LDS, else N * ceil(T / 16) * (states rounded up to the block's)
 * * 4; -1 if out of range (T > 32768, Smax > 4095, A outside 1..64) */
int64_t w2l_asg_align_workspace_bytes(int N, int T, int A, int Smax);
/* The best frame path of a given target under ASG (the Viterbi form of w2l_asg_loss's Z_tgt), fp32, one workgroup per
 * utterance.  Arguments, in-place target addressing (row and length strides) and outputs as w2l_ctc_align.  encoded = 0: rows
 * are RAW transcripts, repeat-encoded on the device as w2l_asg_loss does (a raw label equal to repeat_index: status 2);
 * encoded = 1: rows are encoded already (rank 0 of w2l_asg_beam_search's out buffer; repeat_index allowed, in front too; two
 * equal neighbours: status 2).  Over the encoded target y_0 .. y_{S-1}: score[0][0] = x[0][y_0], score[t][s] =
 * max(score[t-1][s] + g[y_s][y_s], score[t-1][s-1] + g[y_{s-1}][y_s]) + x[t][y_s], a tie goes to staying, the path ends in
 * state S-1 at the last frame.  status: 0 ok, 1 infeasible (S < 1, S > input_lengths[n], or no finite score), 2 a bad label.
 * path[N][T]: the ENCODED label of each frame; starts / ends [N][Smax]: first / last frame of each target position. */
int w2l_asg_align(const float* x, const float* transitions, const int32_t* input_lengths, const int32_t* targets,
                  int64_t target_stride, const int32_t* target_lengths, int64_t length_stride, int N, int T, int A, int Smax,
                  int repeat_index, int encoded, void* workspace, int64_t workspace_bytes, float* score, int32_t* status,
                  int32_t* path, int32_t* starts, int32_t* ends, void* stream);
/* host-side edit distance over int32 symbol arrays */
int w2l_levenshtein_host(const int32_t* a_host, int na, const int32_t* b_host, int nb);
/* workspace bytes for w2l_edit_distance: 0 (a pair's two rows live in LDS); -1 if out of range (n_tokens outside [0, 2^31),
 * S < 1, P < 1, max_len outside [0, 4095]) */
int64_t w2l_edit_distance_workspace_bytes(int64_t n_tokens, int S, int P, int max_len);
/* Levenshtein distances of P pairs of int32 sequences in one launch, one wavefront per pair (csrc/edit_distance.hip).  All
 * pointers are device memory: tokens[n_tokens] is the pool, sequence q is tokens[offsets[q] .. offsets[q+1]) (offsets[S+1]),
 * pairs[P][2] holds (reference sequence, hypothesis sequence); a sequence may stand in any number of pairs.  max_len: the
 * longest sequence the launch provides for (<= 4095; it sizes the LDS).  dist[P]; counts[P][3] (NULL: not wanted) = (sub, del,
 * ins) of the alignment this recurrence picks, reference a[0..na), hypothesis b[0..nb): D[0][0] = 0, D[i][0] = i deletions,
 * D[0][j] = j insertions; for i, j >= 1 the candidates in the order diagonal D[i-1][j-1] (+ one substitution if a[i-1] !=
 * b[j-1]), deletion D[i-1][j] + 1, insertion D[i][j-1] + 1, and the cell takes the FIRST candidate of the smallest distance
 * with that candidate's counts (so ins - del = j - i and sub = d - del - ins at every cell).  status[P]: 0 ok; 1 a sequence
 * of the pair has offsets outside the pool or out of order, or is longer than max_len; 2 a sequence index outside [0, S) --
 * then dist and counts are -1 and nothing of the pair is read.  Deterministic (no atomics); the workspace is unused. */
int w2l_edit_distance(const int32_t* tokens, int64_t n_tokens, const int32_t* offsets, int S, const int32_t* pairs, int P,
                      int max_len, void* workspace, int64_t workspace_bytes, int32_t* dist, int32_t* counts, int32_t* status,
                      void* stream);
/* workspace bytes for w2l_nbest_mbr: (4 N k T + N k) * 4 -- the decoded rows, the token keys and the words' starts and
 * lengths; -1 if out of range (N outside 1..65535, k outside 1..64, T outside 1..32768) */
int64_t w2l_nbest_mbr_workspace_bytes(int N, int k, int T);
/* Minimum-Bayes-risk selection over the n-best list of a beam search, read in the search's out buffer where it lies
 * (search_out: score[N][k] | len[N][k] | status[N] | labels[N][k][T], as w2l_ctc_beam_search / w2l_asg_beam_search_tables
 * write it; 8-byte aligned), on the search's stream right behind it.  label_class_host[A] (host memory, A <= 128): the first
 * label index of the label's character | 0x100 if the character is ' ' | 0x200 if it is whitespace.  Per present row
 * (len >= 0): under ASG (repeat_index >= 0; -1: CTC) the row is decoded first -- a repeat label becomes the decoded label
 * before it, leading ones are dropped --; its tokens are, unit 1 (char), the labels whose character is not ' ', unit 0
 * (word), the maximal runs of labels whose character is not whitespace, two words equal iff they have the same length and the
 * same characters.  dist[n][i][j]: the Levenshtein distance (w2l_edit_distance's recurrence) of rows i and j, 0 on the
 * diagonal, -1 against an empty slot.  In float64, j = 0..k-1 in order over the present rows: m = max_j w_j (w: the search's
 * log weights as they are), e_j = exp(scale * (w_j - m)), p_j = e_j / sum_j e_j, risk[n][i] = sum_j p_j * dist[n][i][j] (NaN
 * for an empty slot); pick[n]: the present row of least risk, a tie to the lower rank; 0 if every slot is empty.  scale >= 0
 * (1.0 is a convention, not a tuned value).
 * mbr_out (8-byte aligned), one section: int32 pick[N] | int32 status[N] | double risk[N][k] | int32 dist[N][k][k] |
 * int32 pick_len[N] | int32 pick_labels[N][T] -- the picked row as the search wrote it, for w2l_ctc_align / w2l_asg_align
 * with row stride T.  status[n]: 0 ok; 1 a row of the utterance has a length above T, a label outside [0, A) or more than
 * 4095 tokens: then pick = 0, the risks are NaN and dist is -1 throughout.  Deterministic; three launches (two for k = 1). */
int w2l_nbest_mbr(const void* search_out, int N, int k, int T, const int32_t* label_class_host, int A, int unit,
                  int repeat_index, double scale, void* workspace, int64_t workspace_bytes, void* mbr_out, void* stream);
/* ConvCTCASR.add_string_metrics (base_asr_models.py:53-69) for one batch in ONE host call (no device work, no interpreter
 * lock held): idx int32 [N][T] = the step's argmax indices on the host, sizes[n] (NULL: T) the valid frames of utterance n.
 * Greedy collapse as GreedyDecoder.process_string(remove_repetitions=True) (decoder.py:104-119: blanks dropped, a frame equal
 * to the previous frame dropped), labels mapped through lut[n_labels] (one Unicode code point per label), then against the
 * reference transcripts ref_cp[ref_off[n] .. ref_off[n+1]) (code points): CER numerator = edit distance with ' ' removed
 * from both (decoder.py:51-63), denominator = len(expected without ' '); WER numerator = edit distance over the words of
 * str.split() (decoder.py:31-49,65-66), denominator = the number of expected words.  totals[5] = {cer_err, cer_ref, wer_err,
 * wer_ref, sum of decoded lengths}; hyp_cp (>= N*T ints) / hyp_off (N+1), both optional, receive the decoded code points. */
int w2l_greedy_score_host(const int32_t* idx_host, int N, int T, const int32_t* sizes_host, int blank, const int32_t* lut,
                          int n_labels, const int32_t* ref_cp, const int64_t* ref_off, int64_t* totals, int32_t* hyp_cp,
                          int64_t* hyp_off);

/* Novograd step of one conv weight (novograd.py:86-112) fused with the bf16 operand pack, tap-major [Kw][Cout][Cin] fp32
 * p / g / exp_avg like w2l_sgd_pack:  v = ||g||^2 on the first step (exp_avg_sq == 0), else beta2*v + (1-beta2)*||g||^2;
 * amsgrad (max_exp_avg_sq != NULL): v <- running max;  g' = g/(sqrt(v)+eps) + weight_decay*p;  g' *= (1-beta1) if
 * grad_averaging;  exp_avg = beta1*exp_avg + g';  p -= lr*exp_avg.  exp_avg_sq / max_exp_avg_sq are device scalars;
 * scratch: >= 2 floats of device memory (1025 lets the norm use 1024 blocks).  Three launches, no host sync. */
int w2l_novograd_pack(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, float* scratch,
                      int scratch_floats, float lr, float beta1, float beta2, float eps, float weight_decay, int grad_averaging,
                      int Cout, int Cin, int Kw, void* w_fwd_hi, void* w_fwd_lo, void* w_dgr_hi, void* w_dgr_lo, void* stream);

/* ---- feature front-end (SpectrogramExtractor, data/data_loader.py:33-88) and augmentation masks ----------------
 * w2l_logmel: per utterance n (n_samples[n] samples of audio[n*audio_stride ...], fp32, device):
 *   x = audio + dither * noise (noise = N(0,1) draws, may be NULL: no dither)   data_loader.py:67
 *   x[i] -= preemph * x[i-1] for i >= 1                                         data_loader.py:68
 *   torch.stft(n_fft, hop, win_length, window, center=True [reflect pad n_fft/2]) -> 1 + n_samples/hop frames   :55-63,69
 *   power = (sqrt(re^2 + im^2))^2; mel = fb . power  (_get_spect's result: take_log == 0)            :70-72
 *   logmel = log1p(mel + log_guard)                  (take_log != 0)                                  :78-79
 * fbT is the filterbank transposed, [n_fft/2 + 1][n_mels]; fb_range (optional) [n_mels][2] int32 = first and one-past-last
 * non-zero bin of each filter (only that run is summed; NULL = all bins).  Output logmel[N][Tmax][n_mels]; frames past an utterance's
 * own count are written as 0.  Requires n_samples[n] > n_fft/2 (torch's reflect-pad rule), n_fft a power of two <= 1024.
 * w2l_feature_normalize: per (utterance, feature) mean and UNBIASED std over the utterance's frames, std += eps,
 *   out[n][m][t] = (logmel - mean) / std for t < frames(n), 0 beyond: the right-zero-padded batch layout of _collator
 *   (data_loader.py:80-88,149-158).  mean_ws / std_ws: [N][n_mels] fp32 workspaces (returned filled). */
int w2l_logmel(const float* audio, const int32_t* n_samples, const float* noise, float dither, float preemph, int N,
               int64_t audio_stride, const float* window, int win_length, int n_fft, int hop, const float* fbT,
               const int32_t* fb_range, int n_mels, int take_log, float log_guard, float* logmel, int Tmax, void* stream);
int w2l_feature_normalize(const float* logmel, const int32_t* n_samples, int hop, int N, int Tmax, int n_mels, float eps,
                          float* mean_ws, float* std_ws, float* out_nct, void* stream);
/* x[n][f0:f1][t0:t1] = 0 for each of R rectangles rects[r] = {n, f0, f1, t0, t1} (int32, device; clipped to the tensor):
 * the masked_fill of SpecAugment.forward / SpecCutout.forward (data/augmentations.py:56,97); x fp32 [N][C][T]. */
int w2l_zero_rects(float* x, int N, int C, int T, const int32_t* rects, int R, void* stream);

/* ---- sample-rate conversion in front of w2l_logmel (data/resample.py; no reference counterpart: the reference asserts the
 * rate of the first manifest row and has no speed perturbation) --------------------------------------------------------
 * x [N][in_stride] -> out [N][out_stride], fp32, device, one launch.  Row n has rows[n] = {n_in, n_out, P, Q, bank}:
 *   P/Q (reduced) = input samples advanced per output sample; n_out = ceil(n_in * Q / P);
 *   out[m] = sum_{j < K} x~[i0 - H + j] * h[phase][j],  i0 = (m P) div Q, phase = (m P) mod Q in 64-bit integers,
 *   x~ = x inside [0, n_in) and 0 outside, fp32 accumulation;  out[m] = 0 for n_out <= m < out_stride.
 * A row with P == Q is copied bit for bit (its bank is not looked at).  banks[b] = {offset, K, H, Q}: the polyphase filter
 * h[Q][K] of bank b is taps[offset ... offset + Q*K), row-major, K = 2H + 2, offset even.  The row and bank tables are passed
 * twice, the same int32 values in host memory (checked here, before anything is launched) and in device memory (read by
 * the kernel).  Rejected: null pointers, P or Q <= 0, n_in > in_stride, n_out != ceil(n_in Q / P) or > out_stride, a bank
 * index or range outside its table, a bank whose Q differs from the row's, K > W2L_RESAMPLE_MAX_K, and a ratio whose tile
 * of W2L_RESAMPLE_TILE outputs needs more than W2L_RESAMPLE_MAX_SPAN input floats in LDS ((TILE-1) P/Q + K + 4).
 * Call site: data_loader.SpectrogramExtractor.extract_batch(rates= / speeds=), data/resample.resample_batch. */
#define W2L_RESAMPLE_TILE 512
#define W2L_RESAMPLE_MAX_K 512
#define W2L_RESAMPLE_MAX_SPAN 8192
int w2l_resample(const float* x, int64_t in_stride, float* out, int64_t out_stride, int N, const int32_t* rows_host,
                 const int32_t* rows_dev, const int32_t* banks_host, const int32_t* banks_dev, int n_banks, const float* taps,
                 int64_t n_taps, void* stream);

/* ---- waveform augmentation between w2l_resample and w2l_logmel (data/augment_wave.py; no reference counterpart: the
 * reference augments spectrograms only, data/augmentations.py) -----------------------------------------------------------
 * w2l_reverb: x [N][in_stride] -> out [N][out_stride] (a separate buffer), fp32, device, one launch.  rows[n] = {n_in, bank},
 * banks[b] = {offset, K, d}: the impulse response of bank b is taps[offset ... offset + K), its direct path at tap d;
 *   out[m] = sum_{j < K} h[j] * x~[m + d - j] for 0 <= m < n_in,  x~ = x inside [0, n_in) and 0 outside, fp32 fmaf chains;
 *   out[m] = 0 for n_in <= m < out_stride.  A row with bank == -1 is copied bit for bit.
 * Grid (tile of W2L_REVERB_TILE outputs, row); a block stages W2L_REVERB_CHUNK taps at a time.  No atomics, no cross-block
 * dependence: two calls give identical bits.  The row and bank tables are passed twice, as for w2l_resample (host copy checked
 * before anything is launched, device copy read by the kernel).  Rejected: null pointers, out == x, n_in > in_stride or
 * > out_stride, a bank index outside [-1, n_banks), K < 1 or K > W2L_REVERB_MAX_TAPS, d outside [0, K), a range outside taps.
 * Call site: data/augment_wave.reverb_device (SpectrogramExtractor.extract_batch(augment=)). */
#define W2L_REVERB_TILE 1024
#define W2L_REVERB_CHUNK 512
#define W2L_REVERB_MAX_TAPS 16384
int w2l_reverb(const float* x, int64_t in_stride, float* out, int64_t out_stride, int N, const int32_t* rows_host,
               const int32_t* rows_dev, const int32_t* banks_host, const int32_t* banks_dev, int n_banks, const float* taps,
               int64_t n_taps, void* stream);
/* w2l_mix_noise: out[n][m] = fmaf(g_n, z[n][(o + m) mod n_z], x[n][m]) for m < n_in, 0 for n_in <= m < out_stride, with
 *   g = sqrt(Ps / (Pz * 10^(snr_db / 10))),  Ps = mean_{m < n_in} x[m]^2,  Pz = mean_{m < n_in} z[(o + m) mod n_z]^2,
 * so that the noise lies snr_db below the utterance over the utterance's own length (a shorter clip wraps).  rows[n] =
 * {n_in, n_z, o} (host and device copies), snr_db [N] fp32 (device), z [N][z_stride] fp32.  A row with n_z == 0, a row with
 * Ps == 0 and a row with Pz == 0 are copied bit for bit.  Two launches, grid (tile of W2L_MIX_TILE samples, row): fp64 partial
 * sums (samples widened before squaring) into slab [N][tiles][2], tiles = ceil(out_stride / W2L_MIX_TILE) -- at least
 * w2l_mix_noise_slab_doubles(N, out_stride) doubles, owned by the caller -- then every block adds its row's partials in index
 * order, forms g in double, rounds it once to fp32 and applies it.  No atomics: two calls give identical bits.
 * Call site: data/augment_wave.mix_noise_device. */
#define W2L_MIX_TILE 2048
int64_t w2l_mix_noise_slab_doubles(int N, int64_t out_stride);
int w2l_mix_noise(const float* x, int64_t x_stride, const float* z, int64_t z_stride, float* out, int64_t out_stride, int N,
                  const int32_t* rows_host, const int32_t* rows_dev, const float* snr_db, double* slab, int64_t slab_doubles,
                  void* stream);

/* ---- voice activity detection and segmentation of long recordings (segmentation.py; no reference counterpart: the reference
 * has no long-form path).  The rule is stated in DESIGN.md ("Long-form transcription") and restated by tests/vad_refs.py. ----
 * w2l_vad_power: x [N][x_stride] fp32 (device, row n valid up to lens_dev[n] samples; a length outside [0, x_stride] is
 *   clamped) -> power [N][power_stride] fp32:  F_n = ceil(len_n / hop) frames,
 *     power[n][f] = float( (sum_{i in [f hop, min(len_n, f hop + win))} double(x[i])^2) / win )   for f < F_n, 0 for f >= F_n,
 *   the sum in fp64 in a fixed order (a frame's samples in eight slices, each added sample after sample by one lane, the slice
 *   sums added in slice order): two calls give identical bits, and the result is within (win + 2) 2^-53 relative of the
 *   sequential sum before the rounding to fp32.  One launch, grid (run of 64 frames, recording); a block stages its frames'
 *   samples in LDS with 16-byte loads (at most W2L_VAD_MAX_SPAN floats), so a sample is read from memory once.  Rejected: null pointers, N outside [1, 65535],
 *   hop < 1 or hop > win, win > W2L_VAD_MAX_SPAN - 8, power_stride outside [1, 2^24) or below ceil(x_stride / hop).
 * w2l_vad_segments: power [N][power_stride] and nframes_dev [N] (clamped to [0, power_stride]) -> out, one record of
 *   W2L_VAD_HEADER_BYTES + 8 cap bytes per recording:
 *     int32 count   segments the rule yields (also when that exceeds cap; only the first cap are written)
 *     int32 status  bit 0: count > cap;  bit 1: a power was NaN or negative (such a power is read as 0 throughout)
 *     double thr_on, thr_off;  float floor, peak;  int32 seg[cap][2]   half-open frame ranges, ascending
 *   One launch, one workgroup of 1024 threads per recording, no dependence between workgroups; workspace (device, caller-owned):
 *   at least w2l_vad_workspace_bytes(N, power_stride) bytes, contents undefined before and after.  Rejected (nothing is launched):
 *   null pointers, N outside [1, 65535], power_stride outside [1, 2^24), q outside [0, 1], max_frames < 2, a frame count
 *   outside [0, 2^24], non-finite ratios / abs_min, r_on <= 0, r_hyst outside (0, 1], absolute thresholds that are not finite
 *   or have thr_off > thr_on, cap outside [1, 2^24], a short workspace, out not 8-byte aligned.
 * Neither is a replay entry.  Call site: segmentation.vad_segments (ConvCTCASR.transcribe_long). */
#define W2L_VAD_MAX_SPAN 12288
#define W2L_VAD_HEADER_BYTES 32
typedef struct {
    double q;                /* floor = the floor(q (F - 1))-th smallest power */
    double r_on;             /* adaptive: thr_on = max(abs_min, min(floor * r_on, sqrt(floor * peak))), in double */
    double r_hyst;           /* adaptive: thr_off = thr_on * r_hyst */
    double abs_min;
    double thr_on, thr_off;  /* absolute != 0: the thresholds themselves (floor and peak are still reported) */
    int32_t absolute;
    int32_t min_silence;     /* frames: a gap shorter than this joins its neighbours */
    int32_t min_speech;      /* frames: a run shorter than this is dropped (after closing gaps) */
    int32_t pad;             /* frames added on both sides of a run (after dropping), clipped; touching runs merge */
    int32_t max_frames;      /* a longer run is cut at the lowest index of the minimum power over [a + h, min(a + max_frames, b - h)), h = max_frames / 2 */
    int32_t reserved_;
} w2l_vad_params_t;
int w2l_vad_power(const float* x, int64_t x_stride, const int32_t* lens_dev, int N, int win, int hop, float* power,
                  int64_t power_stride, void* stream);
int64_t w2l_vad_workspace_bytes(int N, int Fmax);
int w2l_vad_segments(const float* power, int64_t power_stride, const int32_t* nframes_dev, int N, const w2l_vad_params_t* p, int cap,
                     void* workspace, int64_t workspace_bytes, void* out, void* stream);

/* ---- stream concurrency probe -----------------------------------------------------------------------------------------
 * Launches a chip-filling spin kernel (`rounds` waves of 2 blocks per CU, `spin_us` each) on stream_a, then a one-wave
 * kernel on stream_b that records when it started.  stamps_dev: 3 x int64, zero before the call (caller synchronises
 * before and after): [0] start of the fill, [1] end of the fill, [2] start of the stamp kernel, in 100 MHz ticks.
 * (stamps[2] - stamps[0]) / (stamps[1] - stamps[0]) ~ 0: kernels of the two streams run side by side; ~ 1: they share a
 * hardware queue / pipe and serialise.  The host uses it to choose the side streams of the step (weight gradients,
 * optimizer updates, gradient collectives) -- see streams.py; no reference counterpart (stream placement is below torch). */
int w2l_stream_probe(void* stream_a, void* stream_b, void* stamps_dev, int rounds, int spin_us);

/* ---- RCCL helpers: the exchange step of the data-parallel path ------------------------------------------------------
 * One process per GPU; every rank holds a full replica and its own utterances, the only exchange is the average of the
 * parameter gradients (what PL's Trainer(gpus=N) / torch DDP would do for the reference, README.md:40; BatchNorm stays
 * per rank, wav2letter.py:37).  For hosts without torch.distributed: rank 0 draws an id, the host ships its
 * W2L_RCCL_ID_BYTES to the other ranks by whatever channel it has (file, socket, env), every rank calls w2l_rccl_init
 * with its device current (a COLLECTIVE over the ranks), then all-reduces each gradient buffer in place on a stream
 * of its choice (asynchronous, like every other launch here), and destroys the communicator at the end.
 * RCCL itself is resolved at run time (the copy already mapped into the process, else librccl.so.1): without it these
 * entry points -- and only these -- fail with a message.  Errors: 1 = bad argument / RCCL absent, 1000 + ncclResult_t.
 *   dtype: 0 = fp32, 1 = bf16; average != 0: ncclAvg (sum / world), else ncclSum.
 *   w2l_rccl_broadcast: raw bytes from `root` (identical replicas at step 0, DDP's construction-time broadcast). */
#define W2L_RCCL_ID_BYTES 128
int w2l_rccl_available(void);
const char* w2l_rccl_library(void);          /* path of the RCCL shared object in use ("" if none) */
int w2l_rccl_unique_id(void* id_host);
int w2l_rccl_init(const void* id_host, int rank, int world, void** comm_out);
int w2l_rccl_world(void* comm, int* world_out);
int w2l_rccl_all_reduce(void* comm, void* buf, int64_t count, int dtype, int average, void* stream);
int w2l_rccl_broadcast(void* comm, void* buf, int64_t bytes, int root, void* stream);
int w2l_rccl_destroy(void* comm);

/* ---- recorded launch lists (round 6) -----------------------------------------------------------------------------------
 * The reference's host loop is PyTorch's dispatcher (one Python -> ATen transition per op of wav2letter.py:40-47,84-92 and
 * of autograd's backward); the step engine here made one Python -> ctypes transition per launch, 200-500 per step.  After
 * the tuned warm-up the engine records what a step calls -- entry point, argument values, stream, and the event records /
 * waits between its streams -- and replays every phase of the step (forward, backward, optimizer, held-back weight
 * gradients) with ONE w2l_replay call: a C loop over the very same entry points.  Not a hipGraph: each launch goes to the
 * stream it was recorded on, so side streams and the cross-step overlap of the updates behave as in the eager step.
 *   w2l_slot_t    one argument: p for pointers (and pointers to the by-reference structs, whose copies the RECORDER owns),
 *                 i for every integer type, d for float / double (narrowed to the parameter's type at the call);
 *   w2l_call_t    op = w2l_replay_op("w2l_..."), nargs = that entry point's arity, a[] = its arguments in order;
 *   w2l_replay    runs calls[0..n) in order on the calling thread (thread-local library state -- w2l_conv_stats_mode -- is
 *                 that thread's); stops at the first failing call: returns its code, *failed_at = its index, the message
 *                 is the entry point's own (w2l_last_error).  Ownership as everywhere: the caller keeps every buffer the
 *                 recorded pointers name alive and unmoved for as long as it replays the list. */
typedef union { void* p; int64_t i; double d; } w2l_slot_t;
#define W2L_REPLAY_MAX_ARGS 24
typedef struct { int32_t op; int32_t nargs; w2l_slot_t a[W2L_REPLAY_MAX_ARGS]; } w2l_call_t;
int w2l_replay_op(const char* entry_point_name);      /* -1: not a replayable entry point */
int w2l_replay_arity(int op);
int w2l_replay(const w2l_call_t* calls, int n, int* failed_at);

/* Stream order as entry points, so that it can be recorded like a launch (the eager engine used torch.cuda.Event /
 * Stream.wait_event here): events are created without timing; w2l_event_query: 0 fired, 1 not yet;
 * w2l_stream_wait_stream(waiter, signaler): `waiter` waits for everything enqueued on `signaler` so far. */
int w2l_event_create(void** event_out);
int w2l_event_destroy(void* event);
int w2l_event_record(void* event, void* stream);
int w2l_stream_wait_event(void* stream, void* event);
int w2l_event_query(void* event);
int w2l_event_synchronize(void* event);
int w2l_stream_wait_stream(void* waiter, void* signaler);

/* What the eager engine left to torch ops between its launches, as entry points: tensor.zero_() of the statistics / slot /
 * gradient pools (hipMemsetAsync); the zero- / one-padded copy of a per-channel vector (conv bias of the 29-label classifier
 * padded to 64, wav2letter.py:69); `+= delta` on a device int64 (the dropout step counter of a replayed step: the Philox
 * offset of nn.Dropout, wav2letter.py:38,44, must move every step); num_batches_tracked += 1 of every BatchNorm1d of the
 * stack in one launch (table_dev: n device pointers to int64 scalars; wav2letter.py:37); and (csrc/optim.hip)
 * torch.optim.SGD's update of all the small parameters -- biases, BatchNorm gamma / beta -- in one launch
 * (exp_lr_optimizer.yaml:2-7; dampening 0; m == NULL: no momentum buffer). */
int w2l_fill_zero(void* p, int64_t bytes, void* stream);
int w2l_pad_vec_f32(const float* src, int n, float* dst, int cp, float fill, void* stream);
int w2l_counter_add(void* counter_i64, int64_t delta, void* stream);
int w2l_add_i64_multi(void* table_dev, int n, int64_t delta, void* stream);
typedef struct { float* p; const float* g; float* m; int32_t n; int32_t pad_; } w2l_sgd_small_t;
int w2l_sgd_small_multi(const w2l_sgd_small_t* items_dev, int nitems, int max_n /* the largest items[i].n */, float lr,
                        float momentum, float weight_decay, int nesterov, void* stream);

/* ---- gradient clipping (torch.nn.utils.clip_grad_norm_ / clip_grad_value_; Lightning's Trainer(gradient_clip_val=,
 * gradient_clip_algorithm=) around the reference's fit, train.py:34-37), applied on read by the updates of csrc/optim.hip --
 * Called by optim.FusedBase.clip_grad_norm_ / clip_grad_value_ between backward() and step().
 *
 * clip: a float[4] device buffer owned by the caller: [W2L_CLIP_NORM] total norm, [W2L_CLIP_COEF] coefficient,
 * [W2L_CLIP_BOUND] clamp bound.  w2l_grad_sqnorm_multi: the total norm of all gradients in the table (norm type 2, or inf
 * if inf_norm != 0) in one launch of at most W2L_GNORM_BLOCKS blocks over the W2L_GNORM_CHUNK-element chunks of every row
 * (float4 loads where a row is 16-byte aligned), per-block fp64 partials in `partials` (>= W2L_GNORM_BLOCKS doubles), and
 * a one-block finalize that sums them in a fixed order (deterministic: no atomics) and writes
 * norm, coef = min(1, max_norm / (norm + 1e-6)) in fp32 (torch's formula: an inf norm gives 0, a NaN norm NaN), bound = +inf;
 * norm_out (optional): the norm once more (the 0-dim tensor clip_grad_norm_ returns).  Rows: g, n = element count,
 * chunk0 = sum over the rows before of ceil(n / W2L_GNORM_CHUNK) (rows with n == 0 are left out); nchunks = the total.
 * w2l_grad_clip_value: coef = 1, bound = clip_value (value mode, no reduction).
 * w2l_sgd_pack_clip / w2l_sgd_small_multi_clip: w2l_sgd_pack / w2l_sgd_small_multi reading each gradient as
 * clamp(g * coef, -bound, bound) (product rounded on its own, NaN kept) before the weight decay; with coef == 1 and
 * bound == +inf bit-identical to the unclipped entry points.  The gradient buffers are not written. */
#define W2L_CLIP_NORM 0
#define W2L_CLIP_COEF 1
#define W2L_CLIP_BOUND 2
#define W2L_GNORM_CHUNK 8192
#define W2L_GNORM_BLOCKS 2048
typedef struct { const float* g; int64_t n; int64_t chunk0; } w2l_gnorm_item_t;
int w2l_grad_sqnorm_multi(const w2l_gnorm_item_t* items_dev, int nitems, int64_t nchunks, int inf_norm, double* partials,
                          float max_norm, float* clip, float* norm_out, void* stream);
int w2l_grad_clip_value(float* clip, float clip_value, void* stream);
int w2l_sgd_pack_clip(float* p, float* g, float* m, int first_step, float lr, float momentum, float weight_decay,
                      int nesterov, int zero_grad, int Cout, int Cin, int Kw, void* w_fwd_hi, void* w_fwd_lo, void* w_dgr_hi,
                      void* w_dgr_lo, void* w_fwd_q, void* w_dgr_q, float q_scale, const float* clip, void* stream);
int w2l_sgd_small_multi_clip(const w2l_sgd_small_t* items_dev, int nitems, int max_n, float lr, float momentum,
                             float weight_decay, int nesterov, const float* clip, void* stream);

/* ---- torch.optim.Adam / AdamW (amsgrad, maximize off), the first optimizer override of model.optimizer._target_ --------------
 * Called by optim.FusedAdamW.step().  In torch's order (_single_tensor_adam), g read through the clip buffer when clip != NULL:
 *   decoupled != 0 (AdamW): p *= 1 - lr*wd      else (Adam): g += wd*p
 *   m = beta1*m + (1-beta1)*g;   v = beta2*v + (1-beta2)*g*g;   p -= dyn[1] * m / (sqrt(v)/dyn[2] + eps)
 *
 * What changes from step to step lives in DEVICE memory, so that a recorded optimizer phase (w2l_replay) stays valid under a
 * per-step learning-rate schedule: state = {step, beta1^step, beta2^step} of one parameter group and the float[4] dyn =
 * [lr, lr / (1 - beta1^step), sqrt(1 - beta2^step), 0].  w2l_adam_tick (one thread) advances them: step += 1, the powers as
 * running products in fp64 (a host loop of the same multiplies reproduces them bit for bit; a fresh state is {0, 1.0, 1.0}),
 * the two quotients formed in fp64 and rounded to fp32 once.  It is the only call of a step whose arguments change, and it
 * is deliberately NOT a replayable entry point: the caller issues it every step, in front of the recorded list.
 *
 * w2l_adam_pack: the update of a tap-major conv weight fused with the operand pack of the next step, exactly as
 * w2l_sgd_pack (p, g, m, v dense fp32 [Kw][Cout][Cin]; zero_grad, the bf16 hi/lo and e4m3 operands as there).
 * w2l_adam_small_multi: the same rule for all the small parameters in one launch, no pack; table rows {p, g, m, v, n}.
 * clip (nullable, both): the float[4] buffer above; coef == 1 and bound == +inf are bit-identical to clip == NULL. */
typedef struct { int64_t step; double pow1; double pow2; } w2l_adam_state_t;
typedef struct { float* p; const float* g; float* m; float* v; int32_t n; int32_t pad_; } w2l_adam_small_t;
int w2l_adam_tick(w2l_adam_state_t* state_dev, float* dyn_dev, double lr, double beta1, double beta2, void* stream);
int w2l_adam_pack(float* p, float* g, float* m, float* v, const float* dyn, float beta1, float beta2, float eps,
                  float weight_decay, int decoupled, int zero_grad, int Cout, int Cin, int Kw, void* w_fwd_hi, void* w_fwd_lo,
                  void* w_dgr_hi, void* w_dgr_lo, void* w_fwd_q, void* w_dgr_q, float q_scale, const float* clip /* nullable */,
                  void* stream);
int w2l_adam_small_multi(const w2l_adam_small_t* items_dev, int nitems, int max_n /* the largest items[i].n */, const float* dyn,
                         float beta1, float beta2, float eps, float weight_decay, int decoupled, const float* clip /* nullable */,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif

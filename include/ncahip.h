/* ncahip.h -- C ABI of libncahip.so: the MI355X (gfx950) NCA step hot path.
 *
 * The reference (smehra34/Video-Stylization-with-NCA) is 100 % Python/PyTorch and has no FFI
 * layer; its "plugin surface" for this path is the Python class API.  This header
 * is the boundary a maintainer binds with ctypes from those classes (INTEGRATION.md shows the
 * stub).  Every entry point names the reference code it replaces (file:line in the reference).
 *
 * Conventions (all functions):
 *   - plain C types only; every pointer is a DEVICE pointer (tensor.data_ptr()), contiguous NCHW;
 *   - the caller owns every buffer, nothing is allocated, freed or retained across calls;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t; NULL = default stream), the
 *     call never synchronises (ncahip_selftest and ncahip_check_errors excepted) and is safe from several host
 *     threads on distinct streams and devices: launch state is cached per DEVICE (the device current at the call).
 *     Process-wide are only the modes kept in csrc/nca_modes.h, each an atomic that any thread may set while others
 *     enqueue: the tuning / test hooks ncahip_cond_precision, ncahip_debug_force_generic and
 *     ncahip_debug_persist_drop_tiles (with the environment variables that give their initial values), read per
 *     launch, and the modes ncahip_dynca_precision and ncahip_dynca_direction, read once when a call enqueues;
 *   - return 0 on success, a negative NCAHIP_E* on an argument error (nothing was launched),
 *     or a positive hipError_t if the launch failed; ncahip_last_error() describes the last
 *     failure of the calling thread.
 *   - in/out buffers of one call must not alias unless stated.
 */
#ifndef NCAHIP_H
#define NCAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NCAHIP_VERSION 300 /* major*10000 + minor*100 + patch : 0.3.0 */

/* argument errors */
#define NCAHIP_EINVAL (-1)   /* null pointer / non-positive size / bad enum            */
#define NCAHIP_ERANGE (-2)   /* shape outside what the kernels are instantiated for     */
#define NCAHIP_EDEVICE 100001 /* a device-side failure was recorded (sticky error word)  */

/* F.pad modes used by DyNCA perception (ConditioneDyNCA/models/dynca.py:85, default :31) */
#define NCAHIP_PAD_ZERO      0   /* 'constant'  */
#define NCAHIP_PAD_REPLICATE 1
#define NCAHIP_PAD_CIRCULAR  2
#define NCAHIP_PAD_REFLECT   3

typedef void *ncahip_stream_t;   /* hipStream_t */

int ncahip_version(void);
const char *ncahip_last_error(void);

/* Device-side failures.  The producer/consumer step kernels hand tiles over through bounded polls; a poll that expires (a
 * stalled partner wave) cannot hang the device, but the launch then worked on a stale tile.  Such a launch sets a sticky,
 * host-visible error word of its device.  The grow drivers (ncahip_cond_grow_fwd_*) refuse to enqueue with NCAHIP_EDEVICE
 * while the word is set (checked without synchronising: it reflects launches that have completed), and
 * ncahip_check_errors synchronises `stream`, returns NCAHIP_EDEVICE if the word is set and clears it when `clear` != 0.
 * Callers that need certainty for a particular result call ncahip_check_errors after it (the Python layer does so wherever
 * it synchronises anyway).  ncahip_debug_inject_error sets bits of the word (test hook for the return-code plumbing).       */
int ncahip_check_errors(ncahip_stream_t stream, int clear);
int ncahip_debug_inject_error(unsigned bits);

/* Largest shapes the fused step kernels accept (C <= max_c, fc <= max_fc, hidden <= 64).  The fp32 DyNCA *forward* entry
 * points and ncahip_dynca_nsteps_bwd_f32 additionally take 16 < C <= 32 (BASELINE configs[4]) and fc up to 1024 (one launch
 * per 128-wide slice of the hidden layer, the later ones accumulating); the single-step DyNCA backward entry points take
 * C <= 32 with fc <= max_fc; the ConditionedNCA bf16 backward covers C <= max_c, the ConditionedNCA forward fast paths (fp32 and
 * bf16 storage) C <= 20 -- the reference's default model --, the fp32 forward any-shape kernels and the fused fp32 backward
 * C <= 32.                                                                                                                  */
int ncahip_limits(int *max_c, int *max_fc, int *max_hidden);

/* Arithmetic of the UpdateNet products in ncahip_cond_step_fwd_f32 / ncahip_cond_grow_fwd_f32 (process-wide; C in {12,16},
 * hidden = 64, aligned shapes -- other shapes always compute exactly):
 *   0  exact fp32 MFMA (default; bit-compatible with an fmaf chain -- what every parity claim and bench.py's `value` use)
 *   1  "bf16x3": each fp32 operand as a bf16 pair, three bf16 MFMAs per product block, f32 accumulation; relative error
 *      ~1e-5 per step (inside the 1e-4 bar, not exact), about twice the throughput.  The backward always recomputes exactly. */
int ncahip_cond_precision(int mode);

/* Test hook (process-wide; decoded in csrc/nca_modes.hip, the one place that knows the bit layout) selecting which kernel
 * family serves the fused steps, so every variant can be checked against the oracle on the same inputs: bit 0 = generic any-shape kernels instead of the aligned fast paths;
 * bit 1 = symmetric wave-private ConditionedNCA kernel instead of the default producer/consumer one;
 * bit 2 = ncahip_cond_grow_bwd_bf16 evaluates its matrix products in exact fp32 instead of on bf16 MFMA;
 * bit 3 = the ConditionedNCA backward runs its main kernel in the other of its two forms (one launch <-> front kernel +
 * matrix kernel; same results, each mode defaults to the faster one: an independent implementation to cross-check with);
 * bit 4 = the matrix kernel walks whole super-tiles on small grids as well (by default a grid with fewer super-tiles than half
 * the CUs gives each workgroup half a super-tile; with this bit its summation order equals the one-launch form's bit for bit);
 * bit 5 = the fp32 producer/consumer ConditionedNCA step runs perception and UpdateNet on every cell, as before firing-cell lists
 * (by default it runs them on the cells that fire only; same values, see ncahip_cond_step_fwd_f32);
 * bit 6 = the firing-cell lists of that step pad every wave tile's last group of 16 cells (by default, for C <= 16, a consumer
 * wave carries the cells of a partial group across the tiles it owns and runs UpdateNet on them once 16 have come together;
 * same bits for every cell; C > 16 always pads, so the bit changes nothing there);
 * bits 8-15 = a cap on the number of workgroups of a producer/consumer step launch, 0 = no cap (a small grid then gives every
 * workgroup many rounds: what the tests of bit 6's default need; never faster);
 * bit 7 = ncahip_cond_grow_fwd_f32 never draws its fire masks before its steps (every step draws in the kernel; same bits);
 * bits 16-23 = a cap on the steps per fire-word launch of that grow, 0 = no cap; a set cap also lets grows that are too short or
 * too small to gain from it (see ncahip_cond_grow_fwd_f32) draw beforehand, so that the path and its chunking are reachable at
 * test sizes;
 * bit 24 = ncahip_cond_grow_fwd_f32 never sends several steps out as one launch (see there: one launch per step, same bits);
 * bits 25-27 = a cap on the steps per such fused-steps launch, 0 = no cap (a chunk's steps in one launch).
 * Any bit set also keeps ncahip_cond_grow_fwd_persist_f32 from running (it returns NCAHIP_ERANGE). */
int ncahip_debug_force_generic(int on);

/* Device-side check that the MFMA operand/accumulator lane maps the kernels assume hold on
 * this GPU (exact integer data, asymmetric B).  `scratch` >= 4096 bytes of device memory;
 * returns 0 and writes 1 to ((int*)scratch)[0] when the maps hold.  Synchronises `stream`. */
int ncahip_selftest(void *scratch, ncahip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Standalone perception stencils (HBM-bound; the kernels the HBM roofline is measured on)
 * ---------------------------------------------------------------------------------------- */

/* DyNCA.perceive_torch(x, scale=0)          ConditioneDyNCA/models/dynca.py:75-100
 *   y[B,4C,H,W] = [ x | Sx*x | Sy*x | L*x ]  fixed filters :67-73, F.pad mode `pad_mode`.    */
int ncahip_dynca_perceive_f32(const float *x, float *y, int B, int C, int H, int W,
                              int pad_mode, ncahip_stream_t stream);

/* ConditionedNCA.perception_net(z)          EncoderConditioning/nca.py:99-107,177
 *   y[B,3C,H,W], y[3c+k] = wp[3c+k] (3x3, zero pad) * z[c];  wp = perception_net.weight [3C,1,3,3]. */
int ncahip_cond_perceive_f32(const float *z, const float *wp, float *y, int B, int C, int H, int W,
                             ncahip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conditioning front ends: the fixed-filter part of the encoders that produce the step's other input
 * ---------------------------------------------------------------------------------------- */

/* ImageEncoder.forward up to `embed`         EncoderConditioning/encoder.py:37-52
 *   feat[B,3+ch,H,W] = [ sobel_x(gray) | sobel_y(gray) | laplacian(gray) | gaussian_blur(img[c]) for c < ch ],
 *   gray = mean over the ch image channels; 3x3 filters k3 [3][9] = the module's sobel_x / sobel_y / laplacian weights,
 *   5x5 blur k5 [25] = gaussian_blur.weight (frozen parameters, :12-27, :60-64); zero padding.  ch <= 8.
 *   The learned convolutions (embed, :30-34) stay with the caller (MIOpen through PyTorch: their weights train).          */
int ncahip_image_encoder_front_f32(const float *img, const float *k3, const float *k5, float *feat,
                                   int B, int ch, int H, int W, ncahip_stream_t stream);

/* EdgeExtractor.forward                      ConditioneDyNCA/models/dynca.py:204-213
 *   out[B,3,H,W] = transform([ sobel_x | sobel_y | laplacian ](img[B,1,H,W])), zero padding, transform = tanh iff
 *   apply_tanh != 0 (edge_transform == 'tanh'); k3 [3][9] = the module's three frozen filters.                           */
int ncahip_edge_extractor_f32(const float *img, const float *k3, float *out, int B, int H, int W,
                              int apply_tanh, ncahip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DyNCA fused step                          ConditioneDyNCA/models/dynca.py:117-138
 *   (ExtraChannels/models/dynca.py:113-128 is the same step with c_cond = 2 or 0)
 *   x_out = x_in + (w2 relu(w1 [perc(x_in) | cond] + b1) + b2) * floor(u + update_rate)
 *   x_in,x_out [B,C,H,W]; cond [B,c_cond,H,W] = already-extracted conditioning (EdgeExtractor
 *   :204-213 or CPE2D :226-253 output; NULL iff c_cond == 0); u [B,1,H,W] = the torch.rand draw
 *   of :131, or NULL to draw it in-kernel (Philox4x32-10 keyed (seed, step, cell)).
 *   w1 [fc, 4C+c_cond], b1 [fc], w2 [C, fc], b2 [C]  (reference layouts, 1x1 dims squeezed).
 * ---------------------------------------------------------------------------------------- */
int ncahip_dynca_step_fwd_f32(const float *x_in, float *x_out, const float *cond, const float *u,
                              const float *w1, const float *b1, const float *w2, const float *b2,
                              int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                              float update_rate, uint64_t seed, uint64_t step,
                              ncahip_stream_t stream);

/* DyNCA.forward_nsteps                      ConditioneDyNCA/models/dynca.py:168-178
 *   `states` holds `ring` slots of B*C*H*W floats; slot 0 is the input state, step t reads slot
 *   t % ring and writes slot (t+1) % ring.  ring = 2: ping-pong (inference); ring = T+1: every
 *   state is kept (what the backward pass re-reads).  u: [T,B,1,H,W] or NULL (Philox, step0+t). */
int ncahip_dynca_nsteps_fwd_f32(float *states, int ring, int T, const float *cond, const float *u,
                                const float *w1, const float *b1, const float *w2, const float *b2,
                                int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                float update_rate, uint64_t seed, uint64_t step0,
                                ncahip_stream_t stream);

/* The same step / loop with TWO-SCALE perception (DyNCA(perception_scales=[0, 1]): dynca.py:75-115 -- every video model the
 * reference ships, docs/data/video_models/{small,large}/*.json, has n_perception_scales = 2; WebGL twin docs/dynca.js:288-355):
 *     y = ( perc(x) + up2( perc( down2(x) ) ) ) / 2,   down2 / up2 = F.interpolate(bilinear, align_corners=False) by 2.
 * Per step: one coarse pass (2x2 mean + fixed filters with F.pad(mode) on the coarse grid -> pc_scratch [B,4C,H/2,W/2]) and
 * the fused step kernel, which up-samples the coarse tile from LDS on the fly.  H and W even, C <= 16, fc <= 128
 * (NCAHIP_ERANGE otherwise: the Python layer then composes stencil + torch resampling).  NCAHIP_PAD_REFLECT needs a coarse
 * grid of at least 2 x 2, i.e. H, W >= 4 (NCAHIP_EINVAL otherwise, from all four two-scale entry points: F.pad(mode="reflect")
 * with pad 1 raises on a 1-wide axis, so the reference rejects such an input).                                            */
int ncahip_dynca_step_fwd_ms_f32(const float *x_in, float *x_out, const float *cond, const float *u,
                                 const float *w1, const float *b1, const float *w2, const float *b2,
                                 int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                 float update_rate, uint64_t seed, uint64_t step, float *pc_scratch,
                                 ncahip_stream_t stream);
int ncahip_dynca_nsteps_fwd_ms_f32(float *states, int ring, int T, const float *cond, const float *u,
                                   const float *w1, const float *b1, const float *w2, const float *b2,
                                   int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                   float update_rate, uint64_t seed, uint64_t step0, float *pc_scratch,
                                   ncahip_stream_t stream);

/* ---- opt-in bf16 MFMA for the DyNCA forward step ----------------------------------------------------------------------
 * Process-wide, host-only (needs no GPU), not a test hook: 0 = exact fp32 (default), 1 = both 1x1 products of the forward
 * UpdateNet on v_mfma_f32_16x16x32_bf16.  Returns the PREVIOUS mode, or NCAHIP_EINVAL for any other value (the mode is then
 * unchanged).  Arithmetic of mode 1 (the state stays fp32 in and out):
 *   - perception -- and, two-scale, its blend with the up-sampled coarse perception -- in fp32, the code of mode 0;
 *   - y = [perception | cond] rounded to bf16 (round to nearest even) as matrix operand; w1 and w2 rounded to bf16 (RNE) once
 *     per launch, when the weight images are built; b1 and b2 stay fp32: they are the accumulators' initial values;
 *   - layer 1 accumulates in fp32; ReLU; h rounded to bf16 (RNE); layer 2 accumulates in fp32;
 *   - x_out = x + dx * mask in fp32, exactly as in mode 0; K is zero-padded to the instruction's 32;
 *   - the order of k within a product is the implementation's (csrc/nca_dynca_bf16.h) and the same in every kernel of the mode:
 *     per-step kernels (vector and any-shape form, single- and two-scale) and the two one-launch kernels agree bit for bit;
 *   - fire masks (explicit u, packed bits, Philox), pad modes and conditioning are untouched; non-finite inputs are outside the
 *     contract.  Per element the result differs from mode 0 by at most about 2^-8 * sum_j |w2_cj| (|h_j| + sum_k |w1_jk| |y_k|).
 * The mode is read at enqueue time by ncahip_dynca_step_fwd_f32 / _ms_f32, ncahip_dynca_nsteps_fwd_f32 / _ms_f32,
 * ncahip_dynca_nsteps_fwd_persist_f32 / _ms_f32 and ncahip_dynca_clip_f32 / _clip_xc_f32 (once per call of each) -- and by no
 * backward entry point and no bf16-storage one.  The exact backward entry points (ncahip_dynca_step_bwd_*_f32 without "bfmma",
 * ncahip_dynca_nsteps_bwd_f32 / _ms_f32 / _bf16) always compute exactly and need a history recorded in mode 0; the entry points of the
 * bf16-MFMA training mode (ncahip_dynca_*_bfmma_f32, further down) need a history recorded in mode 1.
 * Range: C <= 16 and fc <= 128 (the NARROW range; ncahip_dynca_bf16_range below adds a second one).  For any other shape the
 * mode is IGNORED: the result is bit-equal to mode 0.                                                                        */
int ncahip_dynca_precision(int mode);

/* ---- the range of mode 1 ---------------------------------------------------------------------------------------------------
 * Process-wide, host-only, like the precision: 0 = narrow (default; the range stated above), 1 = wide.  Returns the PREVIOUS
 * value, or NCAHIP_EINVAL for any other argument (the setting is then unchanged).  It matters only while the precision is 1 and
 * is read together with it, once per call.  Under (precision 1, range 1):
 *   - a shape inside the narrow range runs exactly what (1, narrow) runs -- per-step, two-scale, both one-launch kernels, steered;
 *   - a shape outside it with 1 <= C <= 32 and 1 <= fc <= 256 runs the arithmetic of mode 1, as stated above, in the SINGLE-SCALE,
 *     UNSTEERED per-step kernels: ncahip_dynca_step_fwd_f32, ncahip_dynca_nsteps_fwd_f32 (with or without history),
 *     ncahip_dynca_clip_f32 and ncahip_dynca_clip_xc_f32 -- one launch per step for the whole hidden layer (mode 0 runs fc > 128
 *     as one launch per 128-wide slice).  With C > 16 there are two 16-row output tiles: channel c is row c % 16 of tile c / 16, both
 *     tiles are formed from the same bf16 hidden operand, and each accumulator starts at its b2 and sums the hidden units in the k
 *     order of the narrow range (csrc/nca_dynca_bf16.h, "two output tiles"); layer 1 takes up to five 8-slot chunks in ascending
 *     order, the conditioning slot last.  Vector and any-shape form agree bit for bit;
 *   - everything else is the exact fp32 call, bit for bit: shapes outside both ranges, two-scale calls at C > 16 or fc > 128 and
 *     calls with a direction field attached at such shapes.
 * No backward entry point and no bf16-storage entry point reads the setting.                                                */
int ncahip_dynca_bf16_range(int range);

/* ---- steered perception: a per-cell direction field for the DyNCA forward step ------------------------------------------
 * What the WebGL runtime does with `rotationAngle` and `alignment` (docs/dynca.js:209-225, :417-426): every cell's Sobel pair is
 * rotated by the cell's direction before the update rule sees it, which turns a trained motion model at run time.
 *   dirs: float32 [Bd,2,H,W] on the device, Bd in {1, B}; plane 0 = s, plane 1 = c (dir.x, dir.y of dynca.js:420-421).
 * For every cell and every state channel the perception [x | Sx | Sy | L] becomes
 *   Sx' = c Sx - s Sy ,  Sy' = s Sx + c Sy          (x and L untouched)
 * in fp32, on the FINAL perception (two-scale: after the blend with the up-sampled coarse level), before the conditioning channels
 * are appended and before any bf16 rounding of the operand (ncahip_dynca_precision mode 1).  (s, c) is not normalised: a non-unit
 * pair is a rotation-scale.  s = 0, c = 1 reproduces the unsteered step value for value.  The per-step kernels (all three shape
 * classes, wide hidden layers in 128-wide slices, single- and two-scale, both precisions) and the two one-launch kernels evaluate
 * the two lines with one helper and agree bit for bit.  The WebGL runtime rotates each scale at its own resolution; for a uniform
 * field the two definitions agree exactly (the rotation is linear), for a varying field they differ on the coarse half.
 * Process-wide, host-only (needs no GPU), like ncahip_dynca_precision.  dirs == NULL detaches.  Returns 0, or NCAHIP_EINVAL for a
 * non-null pointer with Bd < 1, H < 1 or W < 1 (the attachment is then unchanged).  The library keeps the POINTER, not a copy:
 * the memory must stay valid, and its contents unchanged, until every piece of work enqueued while it was attached has run.
 * While a field is attached:
 *   - ncahip_dynca_step_fwd_f32 / _ms_f32, ncahip_dynca_nsteps_fwd_f32 / _ms_f32, ncahip_dynca_nsteps_fwd_persist_f32 / _ms_f32
 *     and ncahip_dynca_clip_f32 / _clip_xc_f32 read it once per call at enqueue time and steer every step of the call; a call with
 *     another (H, W), or with B != Bd while Bd != 1, returns NCAHIP_EINVAL before anything is enqueued;
 *   - every DyNCA backward entry point and every bf16-storage forward entry point returns NCAHIP_EINVAL: they do not steer, and a
 *     silently unsteered result or gradient is what this excludes.  ncahip_dynca_perceive_f32 is untouched.                  */
int ncahip_dynca_direction(const float *dirs, int Bd, int H, int W);

/* Backward of ONE DyNCA step (autograd through dynca.py:117-138; dynca.py:123: no gradient into cond).
 *   In : x_t (the step's input state), the same cond / u (or seed, step) / weights, g_next = dL/dx_{t+1}.
 *   Out: g_x = dL/dx_t (data path through W2^T, relu', W1^T on MFMA, then the adjoint of "F.pad(mode) + fixed 3x3
 *        filters", plus the residual path), and the two operand pairs of the weight-gradient products, which the
 *        caller evaluates over all cells with ncahip_gram_rows_f32 (below):
 *            h_out  = relu(w1 y + b1)            [B,fc,H,W]     dW2 += (g_next*mask) h^T ,  db2 += sum(g_next*mask)
 *            dh_out = dL/d(w1 y + b1)            [B,fc,H,W]     dW1 += dh y^T            ,  db1 += sum(dh)
 *        (y = [ncahip_dynca_perceive_f32(x_t) | cond], mask = floor(u + rate)).  dy_scratch: [B,4C,H,W] floats. */
int ncahip_dynca_step_bwd_f32(const float *x_t, const float *cond, const float *u,
                              const float *w1, const float *b1, const float *w2, const float *b2,
                              int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                              float update_rate, uint64_t seed, uint64_t step,
                              const float *g_next, float *g_x, float *h_out, float *dh_out,
                              float *dy_scratch, ncahip_stream_t stream);

/* The same backward step with the layer-2 weight gradient fused in: h is kept in registers and never written; the kernel
 * accumulates dW2 = (g_next*mask) h^T and db2 = sum(g_next*mask) on MFMA (cell axis as K, operands transposed through LDS)
 * and gw2_out [C*fc + C] receives [dW2 | db2] of THIS step (accumulate = 0: overwritten, 1: added; per-workgroup partials
 * summed in fixed order).
 * dh_out / dy_scratch / g_x as above; dW1 | db1 = ncahip_gram_rows_f32(dh_out, perception, cond).                     */
size_t ncahip_dynca_step_bwd_w2_workspace(int B, int C, int H, int W, int fc);
int ncahip_dynca_step_bwd_w2_f32(const float *x_t, const float *cond, const float *u,
                                 const float *w1, const float *b1, const float *w2, const float *b2,
                                 int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                 float update_rate, uint64_t seed, uint64_t step,
                                 const float *g_next, float *g_x, float *dh_out, float *dy_scratch,
                                 float *gw2_out, int accumulate, void *workspace, size_t workspace_bytes,
                                 ncahip_stream_t stream);

/* Backward of ncahip_dynca_nsteps_fwd_f32      autograd through dynca.py:168-178 (experiments.py:226,254)
 *   The whole T-step loop is enqueued on the stream with caller-owned scratch (no allocation, no host round trip).  states:
 *   the T+1 slots the forward kept with ring = T+1; cond / u (or seed, step0) / weights as in the forward.  g_final = dL/dx_T
 *   (INCLUDING any cotangent of x_T itself); g_states (nullable): [T+1 slots] cotangents of the intermediate states x_t, slots
 *   0..T-1 are added where x_t's gradient is formed (forward_nsteps' return_middle_feature).  Writes dL/dx_0 and the weight
 *   gradients in the reference layouts g_w1 [fc, 4C+c_cond], g_b1 [fc], g_w2 [C, fc], g_b2 [C] (overwritten).  C <= 32,
 *   fc <= 1024: hidden layers wider than 128 run as 128-wide slices (w2 relu(w1 y + b1) is a sum over hidden units; dL/dy is
 *   accumulated over the slices, the weight gradients of different slices are independent).  Per step: perception of x_t,
 *   per slice {fused MLP-backward kernel (dh, dL/dy, dW2|db2 on MFMA), dW1|db1 = ncahip_gram_rows_f32(dh, perception, cond)},
 *   stencil adjoint.  Deterministic (fixed-order partial sums, no float atomics).                                          */
size_t ncahip_dynca_nsteps_bwd_workspace(int B, int C, int H, int W, int fc, int c_cond);
int ncahip_dynca_nsteps_bwd_f32(const float *states, int T, const float *cond, const float *u,
                                const float *w1, const float *b1, const float *w2, const float *b2,
                                int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                float update_rate, uint64_t seed, uint64_t step0,
                                const float *g_final, const float *g_states,
                                float *g_x0, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                                void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* The same backward over a bf16 history (the [T+1 slots] ncahip_dynca_nsteps_fwd_bf16 kept with ring = T+1): storage format only, as in
 * the forward -- x_t is widened exactly into scratch and the step's backward runs in fp32; every gradient is fp32.
 * B*C*H*W % 4 == 0, states 8-byte aligned; fc <= 128 (the bf16 forward's limit).                                           */
size_t ncahip_dynca_nsteps_bwd_bf16_workspace(int B, int C, int H, int W, int fc, int c_cond);
int ncahip_dynca_nsteps_bwd_bf16(const uint16_t *states, int T, const float *cond, const float *u,
                                 const float *w1, const float *b1, const float *w2, const float *b2,
                                 int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                 float update_rate, uint64_t seed, uint64_t step0,
                                 const float *g_final, const float *g_states,
                                 float *g_x0, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                                 void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* The same backward through the TWO-SCALE steps of ncahip_dynca_nsteps_fwd_ms_f32 (training with perception_scales = [0, 1]:
 * ExtraChannels/fit_video_motion.py:129-130 defaults to it).  dL/dy splits evenly over the two levels: the fine level goes
 * through the stencil adjoint as before; the coarse level through the adjoint of the bilinear x2 up-sampling, the stencil
 * adjoint on the COARSE grid (pad mode resolved there) and the adjoint of the 2x2 mean.  Even H and W, C <= 16, fc <= 128;
 * NCAHIP_PAD_REFLECT needs H, W >= 4 (NCAHIP_EINVAL otherwise, as in the forward).                                         */
size_t ncahip_dynca_nsteps_bwd_ms_workspace(int B, int C, int H, int W, int fc, int c_cond);
int ncahip_dynca_nsteps_bwd_ms_f32(const float *states, int T, const float *cond, const float *u,
                                   const float *w1, const float *b1, const float *w2, const float *b2,
                                   int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                   float update_rate, uint64_t seed, uint64_t step0,
                                   const float *g_final, const float *g_states,
                                   float *g_x0, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                                   void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* ---- opt-in "bf16-MFMA training" of DyNCA: mode-1 forward history + a backward on bf16 MFMA ---------------------------------
 * C <= 16 and fc <= 128 (NCAHIP_ERANGE otherwise), single-scale and two-scale, fp32 state history.  No process-wide state: the
 * caller records the T + 1 history slots with ncahip_dynca_precision mode 1 (ring = T + 1; the forward kernels are unchanged) and
 * hands them to the entry points below.  The exact backward entry points above keep needing a mode-0 history.
 * Backward of one step, given x_t from that history and g = dL/dx_{t+1}:
 *   - y = the fp32 perception of the forward kernels (two-scale: blended) with cond appended; yb = bf16(y);
 *     a1 = b1 + W1b yb with the rounded weights, the k order and the MFMA sequence of the forward (csrc/nca_dynca_bf16.h, one
 *     shared routine): a1 has the forward's bits, gate = a1 > 0 is the forward's gate; hb = bf16(relu(a1));
 *   - gm = g * mask in fp32 (mask as in the forward), gb = bf16(gm);
 *   - dh = (W2b^T gb) * gate with fp32 accumulation (v_mfma_f32_16x16x16_bf16, K = the channels), dhb = bf16(dh);
 *   - dL/dy[0:4C] = W1b^T dhb with fp32 accumulation (v_mfma_f32_16x16x32_bf16, K = the hidden units); no gradient into cond;
 *   - dW2 += gb hb^T, db2 += sum gb, dW1 += dhb [yb | bf16(cond)]^T, db1 += sum dhb: sums over all cells, fp32 accumulation on
 *     bf16 MFMA (products of two bf16 values are exact in fp32), per-workgroup partials added in a fixed order, no float
 *     atomics.  The bias gradients sum the ROUNDED operands (db1 rides on the MFMA as a column of ones);
 *   - dL/dx_t = g (+ g_states[t]) + stencil-adjoint(dL/dy) in fp32: the kernels of the exact backward, two-scale path included;
 *   - every rounding is to nearest even and straight-through; the k order inside each product is the implementation's and fixed:
 *     the vector and any-shape kernels agree bit for bit, and two runs give the same bits.
 * ncahip_dynca_step_bwd_bfmma_f32 mirrors ncahip_dynca_step_bwd_w2_f32 (single-scale); it also writes the two operands of the
 * layer-1 weight gradient AS BF16: y_out [B,4C,H,W] = yb[0:4C], dh_out [B,fc,H,W] = dhb (half the scratch traffic of the fp32
 * backward), so that  dW1 | db1 = ncahip_gram_rows_bf16(dh_out, y_out, cond).  dy_scratch [B,4C,H,W] floats, gw2_out [C*fc + C].
 * The *_workspace queries are host arithmetic and return 0 for a shape outside the range.                                  */
size_t ncahip_dynca_step_bwd_bfmma_workspace(int B, int C, int H, int W, int fc);
int ncahip_dynca_step_bwd_bfmma_f32(const float *x_t, const float *cond, const float *u,
                                    const float *w1, const float *b1, const float *w2, const float *b2,
                                    int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                    float update_rate, uint64_t seed, uint64_t step,
                                    const float *g_next, float *g_x, uint16_t *y_out, uint16_t *dh_out,
                                    float *dy_scratch, float *gw2_out, int accumulate, void *workspace,
                                    size_t workspace_bytes, ncahip_stream_t stream);

/* ncahip_gram_rows_f32 (below) over bf16 operands: a [B,ma,HW] and b1 [B,nb1,HW] hold bf16, b2 [B,nb2,HW] holds fp32 and is
 * rounded to bf16 (RNE) as it is loaded (b2 may be NULL with nb2 = 0).  Same output layout [ma x nb | ma], same accumulate flag,
 * same fixed-order reduction of per-workgroup partials.  The result differs from exact arithmetic on those bf16 values only by
 * fp32 summation.  ma <= 128, nb = nb1 + nb2 <= 79 (NCAHIP_ERANGE otherwise).                                               */
size_t ncahip_gram_rows_bf16_workspace(int ma, int nb, int B, int HW);
int ncahip_gram_rows_bf16(const uint16_t *a, int ma, const uint16_t *b1, int nb1, const float *b2, int nb2, int B, int HW,
                          float *out, int accumulate, void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* The T-step drivers of the mode: argument lists, outputs and refusals of ncahip_dynca_nsteps_bwd_f32 / _ms_f32; `states` is the
 * MODE-1 history.  Per step: the bf16-MFMA MLP kernel (yb, dhb, dL/dy, dW2 | db2), ncahip_gram_rows_bf16, the exact stencil
 * adjoint (two-scale: up-sampling adjoint, coarse stencil adjoint, 2x2-mean adjoint).  Deterministic.                        */
size_t ncahip_dynca_nsteps_bwd_bfmma_workspace(int B, int C, int H, int W, int fc, int c_cond);
int ncahip_dynca_nsteps_bwd_bfmma_f32(const float *states, int T, const float *cond, const float *u,
                                      const float *w1, const float *b1, const float *w2, const float *b2,
                                      int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                      float update_rate, uint64_t seed, uint64_t step0,
                                      const float *g_final, const float *g_states,
                                      float *g_x0, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                                      void *workspace, size_t workspace_bytes, ncahip_stream_t stream);
size_t ncahip_dynca_nsteps_bwd_ms_bfmma_workspace(int B, int C, int H, int W, int fc, int c_cond);
int ncahip_dynca_nsteps_bwd_ms_bfmma_f32(const float *states, int T, const float *cond, const float *u,
                                         const float *w1, const float *b1, const float *w2, const float *b2,
                                         int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                         float update_rate, uint64_t seed, uint64_t step0,
                                         const float *g_final, const float *g_states,
                                         float *g_x0, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                                         void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* ---- "bf16-MFMA training", the WIDE range: 1 <= C <= 32, 1 <= fc <= 256, single-scale, fp32 state history -------------------------
 * The contract is the one of "bf16-MFMA training" above, word for word; only the range changes.  The caller records the T + 1
 * history slots with ncahip_dynca_precision(1) plus ncahip_dynca_bf16_range(1) (ring = T + 1) and hands them to the entry points
 * below, which read NO process-wide setting: the range is in their names.
 *   - Inside the narrow range (C <= 16 and fc <= 128) they run the narrow kernels: bit-equal to ncahip_dynca_step_bwd_bfmma_f32,
 *     ncahip_gram_rows_bf16 and ncahip_dynca_nsteps_bwd_bfmma_f32.  Outside the wide range: NCAHIP_ERANGE, workspace queries 0.
 *     The narrow entry points keep refusing every shape outside their range.
 *   - Outside the narrow range the forward's layer-1 pre-activation comes from NcaDyncaBf16<CP,FC,HAS_COND>::layer1
 *     (csrc/nca_dynca_bf16.h) at the class the forward picks: <32,128> if fc <= 128; else <16,256> if C <= 16; else <32,256>.  The
 *     backward forms a1 with that class's pack_y / layer1 -- the same K1S, K1Q and chunk order -- so the gate is the forward's bit
 *     for bit.  It takes the hidden layer in 128-wide slices, one launch per slice (a <16,256> forward as two <16,128> slices, a
 *     <32,256> forward as two <32,128> slices): y_out is written once, dh_out is the full [B,fc,H,W].
 *   - dh = W2b^T gb over the 32 channel slots of C > 16 is TWO v_mfma_f32_16x16x16_bf16 products into one accumulator, channels
 *     0..15 first, then 16..31.  dL/dy = W1b^T dhb sums the hidden units slice by slice: the second slice's accumulators start at
 *     the first slice's fp32 result; inside a slice the order is the narrow range's.  dW2 | db2 take one K = 32 product per
 *     16-channel tile and hidden tile.  All of this is fixed and deterministic: two runs give the same bits, and the vector and
 *     any-shape kernels agree bit for bit.
 * ncahip_dynca_step_bwd_bfmma_wide_f32: the argument list of ncahip_dynca_step_bwd_bfmma_f32; dh_out [B,fc,H,W] and y_out
 * [B,4C,H,W] bf16, gw2_out [C*fc + C], so that  dW1 | db1 = ncahip_gram_rows_bf16_wide(dh_out, y_out, cond).
 * ncahip_gram_rows_bf16_wide: ncahip_gram_rows_bf16 with ma <= 256 and nb = nb1 + nb2 <= 132 -- same arguments, same output layout
 * [ma x nb | ma row sums], same accumulate flag; operands go from memory straight into v_mfma_f32_16x16x32_bf16, the output is
 * tiled over blocks of 128 rows x up to 80 columns, the row sums are taken once, the summation order is fixed.
 * ncahip_dynca_nsteps_bwd_bfmma_wide_f32: argument list, outputs and refusals of ncahip_dynca_nsteps_bwd_bfmma_f32 (null pointer,
 * T < 1, workspace too small or not 16-byte aligned, aliasing, an attached direction field: all before any launch).             */
size_t ncahip_dynca_step_bwd_bfmma_wide_workspace(int B, int C, int H, int W, int fc);
int ncahip_dynca_step_bwd_bfmma_wide_f32(const float *x_t, const float *cond, const float *u,
                                         const float *w1, const float *b1, const float *w2, const float *b2,
                                         int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                         float update_rate, uint64_t seed, uint64_t step,
                                         const float *g_next, float *g_x, uint16_t *y_out, uint16_t *dh_out,
                                         float *dy_scratch, float *gw2_out, int accumulate, void *workspace,
                                         size_t workspace_bytes, ncahip_stream_t stream);
size_t ncahip_gram_rows_bf16_wide_workspace(int ma, int nb, int B, int HW);
int ncahip_gram_rows_bf16_wide(const uint16_t *a, int ma, const uint16_t *b1, int nb1, const float *b2, int nb2, int B, int HW,
                               float *out, int accumulate, void *workspace, size_t workspace_bytes, ncahip_stream_t stream);
size_t ncahip_dynca_nsteps_bwd_bfmma_wide_workspace(int B, int C, int H, int W, int fc, int c_cond);
int ncahip_dynca_nsteps_bwd_bfmma_wide_f32(const float *states, int T, const float *cond, const float *u,
                                           const float *w1, const float *b1, const float *w2, const float *b2,
                                           int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                           float update_rate, uint64_t seed, uint64_t step0,
                                           const float *g_final, const float *g_states,
                                           float *g_x0, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                                           void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* Weight-gradient products of the DyNCA backward with the cell axis as K (replaces the library GEMMs over transposed
 * copies that autograd through dynca.py:127-128 amounts to):
 *     out[i*nb + j] = sum over all B*HW cells of a[., i, .] * b[., j, .]     i < ma, j < nb = nb1 + nb2
 *     out[ma*nb + i] = sum over all cells of a[., i, .]                       (the bias gradient of the same layer)
 * a [B, ma, HW]; the b rows come from two tensors, b1 [B, nb1, HW] then b2 [B, nb2, HW] (b2 may be NULL with nb2 = 0):
 * dW1 | db1 = gram(dh_out, perception, cond), dW2 | db2 = gram(g_next * mask, h_out).  Exact fp32 MFMA, per-workgroup
 * partials summed in a fixed order (deterministic).  Shapes: ma <= 128 with nb <= 80, or ma <= 32 with nb <= 128
 * -- since 0.2.0: ma <= 128 with nb <= 144 --
 * (NCAHIP_ERANGE otherwise).  out holds ma*nb + ma floats; accumulate = 0 overwrites it, 1 adds to it (the sum over the
 * steps of a backward pass without a separate add per step).                                                          */
size_t ncahip_gram_rows_workspace(int ma, int nb, int B, int HW);
int ncahip_gram_rows_f32(const float *a, int ma, const float *b1, int nb1, const float *b2, int nb2, int B, int HW,
                         float *out, int accumulate, void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ConditionedNCA fused step                 EncoderConditioning/nca.py:181-195
 *
 * The step's post-life mask (:191-193) needs the NEW alpha on a 3x3 neighbourhood, i.e. a
 * grid-wide exchange after the update.  The kernel therefore emits the state in PENDING form:
 *     x_out   = x + rand_mask * update(x)                 (:189, before :191-194)
 *     pre_out = alive(x)                                  (:185, uint8 [B,H,W])
 * and the NEXT step (or ncahip_cond_finalize_f32) resolves
 *     x'' = clamp(x_out * (pre_out & alive(x_out)), lo, hi)   (:191-194)
 * while it loads its tile (alpha halo of 3 cells).  Pass pre_in = NULL when x_in is a true
 * state (first step), or the previous call's pre_out when x_in is pending.
 *
 *   goal  [B,goal_ch,H,W] = encoder(goal) UNPADDED (nca.py:198); it is added to the LAST
 *         goal_ch channels (:199-203 pads zeros in front).  goal_ch may equal C.
 *   u     [B,1,H,W] rand_like draw (:172) or NULL (in-kernel Philox); mask = u < fire_rate.
 *   wp [3C,9]; w1 [hidden,3C], b1 [hidden]; w2 [hidden,hidden], b2 [hidden]; w3 [C,hidden].
 *   alive_ch < 0  <=>  use_living_channel=False (:153-154): every cell alive.
 * The aligned fast path (W % 4 == 0) evaluates UpdateNet for the cells whose mask is 1 only (firing-cell lists); a cell
 * whose mask is 0 keeps its resolved state.  Against x + 0*out this differs only (a) in the sign of a zero: x = -0 stays
 * -0 where the reference gives +0 (equal as values), and (b) where out is +-inf or NaN, which only weights that overflow
 * produce: the reference's cell becomes NaN, this one keeps x.  The kernels of ncahip_debug_force_generic bits 0, 1 and 5 compute
 * x + 0*out for every cell.
 * ---------------------------------------------------------------------------------------- */
int ncahip_cond_step_fwd_f32(const float *x_in, const uint8_t *pre_in, float *x_out, uint8_t *pre_out,
                             const float *goal, int goal_ch, const float *u,
                             const float *wp, const float *w1, const float *b1,
                             const float *w2, const float *b2, const float *w3,
                             int B, int C, int H, int W, int hidden,
                             int alive_ch, float alive_thr, float fire_rate,
                             float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step,
                             ncahip_stream_t stream);

/* Resolve a pending state: x_out = clamp(x_pend * (pre & alive(x_pend)), lo, hi)  nca.py:191-194.
 * x_out may alias x_pend only if alive_ch < 0.                                              */
int ncahip_cond_finalize_f32(const float *x_pend, const uint8_t *pre, float *x_out,
                             int B, int C, int H, int W, int alive_ch, float alive_thr,
                             float clamp_lo, float clamp_hi, ncahip_stream_t stream);

/* ---- bf16 state storage, DyNCA ---------------------------------------------------------------
 * DyNCA.forward / forward_nsteps (dynca.py:117-138, :168-178) with the state stored as bf16 (uint16_t bit patterns);
 * cond, uniforms and weights stay fp32.  The step computes exactly as the _f32 entry points on the widened state
 * (exact fp32 MFMA) and rounds x + dx*mask to bf16 (RNE) on store: storage format only, same kernel.               */
int ncahip_dynca_step_fwd_bf16(const uint16_t *x_in, uint16_t *x_out, const float *cond, const float *u,
                               const float *w1, const float *b1, const float *w2, const float *b2,
                               int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                               float update_rate, uint64_t seed, uint64_t step, ncahip_stream_t stream);
int ncahip_dynca_nsteps_fwd_bf16(uint16_t *states, int ring, int T, const float *cond, const float *u,
                                 const float *w1, const float *b1, const float *w2, const float *b2,
                                 int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                 float update_rate, uint64_t seed, uint64_t step0, ncahip_stream_t stream);

/* ---- bf16 state storage ---------------------------------------------------------------------
 * The same step / finalize / grow loop with the state and the goal encoding stored as bf16 (uint16_t bit patterns,
 * [B,C,H,W] contiguous) and the UpdateNet on bf16 MFMA; weights, biases and explicit uniforms stay fp32.  Rounding
 * points (restated by oracle.cond_step_bf16): perception in f32 from the widened state; the perception vector, both
 * hidden activations and the weights are rounded to bf16 (RNE) as matrix operands, accumulation in f32; x' = x + mask*out
 * in f32, rounded to bf16 on store.  Replaces the same reference code as the _f32 entry points (nca.py:181-195, :207-208)
 * for callers that keep the pool in bf16 (BASELINE configs[2]).  Needs W % 4 == 0, 8-byte aligned tensors and C <= 20 -- the
 * reference's default model (nca.py:62-94) included; ncahip_cond_grow_bwd_bf16 takes the same range -- (NCAHIP_ERANGE otherwise;
 * there is no any-shape bf16 kernel).                                                                                 */
int ncahip_cond_step_fwd_bf16(const uint16_t *x_in, const uint8_t *pre_in, uint16_t *x_out, uint8_t *pre_out,
                              const uint16_t *goal, int goal_ch, const float *u,
                              const float *wp, const float *w1, const float *b1,
                              const float *w2, const float *b2, const float *w3,
                              int B, int C, int H, int W, int hidden,
                              int alive_ch, float alive_thr, float fire_rate,
                              float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step,
                              ncahip_stream_t stream);
int ncahip_cond_finalize_bf16(const uint16_t *x_pend, const uint8_t *pre, uint16_t *x_out,
                              int B, int C, int H, int W, int alive_ch, float alive_thr,
                              float clamp_lo, float clamp_hi, ncahip_stream_t stream);
int ncahip_cond_grow_fwd_bf16(uint16_t *states, uint8_t *pre, int ring, int T, uint16_t *x_final,
                              const uint16_t *goal, int goal_ch, const float *u,
                              const float *wp, const float *w1, const float *b1,
                              const float *w2, const float *b2, const float *w3,
                              int B, int C, int H, int W, int hidden,
                              int alive_ch, float alive_thr, float fire_rate,
                              float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step0,
                              ncahip_stream_t stream);

/* The fire masks of ConditionedNCA steps step0 .. step0 + Tc - 1 as the in-kernel Philox draw (u == NULL) produces them, one
 * 64-bit word per 4 x 16 tile: words [Tc][B][H/4][W/16], bit 16 * row + col of a word <=> cell (4 ty + row, 16 tx + col) fires,
 * i.e. clamp(u, 0, 1) < fire_rate for the cell's uniform (ncahip_philox_uniform_f32; nca.py:171-174).  What
 * ncahip_cond_grow_fwd_f32 feeds its steps; exported so that the words can be tested on their own.  H % 4 == 0, W % 16 == 0,
 * Tc <= 65535, 8-byte aligned words (NCAHIP_ERANGE otherwise).
 * ncahip_debug_fire_word_launches: how many such launches the last completed ncahip_cond_grow_fwd_f32 of the process made
 * (0: its steps drew their masks themselves); a test hook. */
int ncahip_cond_fire_words(uint64_t *words, int Tc, int B, int H, int W, float fire_rate, uint64_t seed, uint64_t step0,
                           ncahip_stream_t stream);
int ncahip_debug_fire_word_launches(void);

/* ConditionedNCA.alive(x)                   EncoderConditioning/nca.py:152-163 -> uint8 [B,H,W] */
int ncahip_cond_alive_u8(const float *x, uint8_t *out, int B, int C, int H, int W,
                         int alive_ch, float alive_thr, ncahip_stream_t stream);

/* ConditionedNCA.grow's loop                EncoderConditioning/nca.py:207-208
 *   T fused steps + one finalize.  states: `ring` slots of B*C*H*W floats, slot 0 = input (true
 *   state); slot k (k>=1) receives the PENDING output of step k-1; pre: `ring` slots of B*H*W
 *   bytes, slot k pairs with states slot k (slot 0 unused).  x_final receives grow()'s result.
 *   ring = 2 ping-pong, ring = T+1 keeps every pending state for the backward pass.
 *   x_final may be used as scratch during the call: with in-kernel Philox (u == NULL) on the aligned fast path (C <= 20,
 *   W % 16 == 0, H % 4 == 0) a grow draws its fire masks before its steps (ncahip_cond_fire_words, one launch per chunk of up to
 *   32 C steps) into x_final, which is dead until the finalize writes it, and the steps read them instead of drawing: the same
 *   masks, the same results bit for bit.  It does so only when x_final's bytes are disjoint from the ring, pre, goal and the
 *   weight tensors; an x_final that is a ring slot (other than the last one, which is refused) is legal and simply keeps the
 *   steps drawing in the kernel, as do explicit uniforms, bit-packed masks, ncahip_debug_force_generic bit 7, and grows for which
 *   one more launch does not pay: with r = the 16 x 16 super-tiles per workgroup of a step launch (B * ceil(H/16) * ceil(W/16)
 *   over min(that, the device's CUs), rounded up), r < 2 or T * r < 106.
 *   Fused steps: where a grow draws its masks beforehand AND C <= 16 (the narrow-carve producer/consumer kernels) AND 2 <= r <= 12
 *   (beyond that the saved launch cost no longer pays for the path's cost per round), the steps of a chunk go out as ONE launch
 *   instead of one launch each.  A tile of step t + 1 then waits only for its 3 x 3
 *   neighbourhood of 4 x 16 tiles of step t, through one 32-bit counter per tile; the counters live in x_final behind the chunk's
 *   words (the chunk is at most 32 C - 1 steps then).  Same masks, same arithmetic, same results bit for bit.  The launch needs
 *   every one of its workgroups resident at once (one per CU, at most the device's CUs): on a device whose CUs another process
 *   holds, a tile's wait expires (bounded, about 0.2 s), the call or the next one returns NCAHIP_EDEVICE (error word bit 2), and
 *   the ring has been overwritten by then.  ncahip_debug_force_generic bit 24 switches the path off (one launch per step, the
 *   results are the same), bits 25-27 cap the steps per launch; ncahip_debug_fused_step_launches tells how many such launches the
 *   last completed ncahip_cond_grow_fwd_f32 of the process made (0: one launch per step).                                     */
int ncahip_debug_fused_step_launches(void);
/* Where that path keeps its counters in x_final (host only, no GPU call): *chunk = the steps per fire-word chunk, at most 32 C, at
 * most chunk_cap (0: no cap) and as many as leave room for the counters; *done_offset = the byte offset of the counters in x_final
 * (= *chunk * B*H*W/8, behind the words); *done_bytes = their size (B * H/4 * W/16 counters and the abort word, padded to 64 bytes).
 * *done_offset + *done_bytes <= B*C*H*W*4 always.  NCAHIP_EINVAL: null pointer, a size that is not positive, a negative cap;
 * NCAHIP_ERANGE: H % 4 != 0 or W % 16 != 0. */
int ncahip_cond_fused_steps_layout(int B, int C, int H, int W, int chunk_cap, int *chunk, uint64_t *done_offset, uint64_t *done_bytes);
int ncahip_cond_grow_fwd_f32(float *states, uint8_t *pre, int ring, int T, float *x_final,
                             const float *goal, int goal_ch, const float *u,
                             const float *wp, const float *w1, const float *b1,
                             const float *w2, const float *b2, const float *w3,
                             int B, int C, int H, int W, int hidden,
                             int alive_ch, float alive_thr, float fire_rate,
                             float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step0,
                             ncahip_stream_t stream);

/* Backward of ncahip_cond_grow_fwd_f32      autograd through nca.py:207-208 (conditioned_trainer.py:125-132)
 *   Recomputation: needs only what the forward kept with ring = T+1 -- states [T+1 slots] (slot 0 the
 *   input, slot k the pending output of step k-1) and pre [T+1 slots] -- plus the same goal / u (or seed,
 *   step0) / weights.  g_final = dL/d x_final.  Writes dL/dx0 [B,C,H,W], dL/dgoal [B,goal_ch,H,W] (summed over
 *   the T steps, nca.py:207-208 reuse the same encoding), and the weight gradients in the reference layouts
 *   (g_wp [3C,9], g_w1 [hidden,3C], g_b1, g_w2 [hidden,hidden], g_b2, g_w3 [C,hidden]); masks carry no
 *   gradient; clamp passes gradient on the closed interval (torch.clamp).  Deterministic (no float atomics).
 *   Requires W % 4 == 0 and 16-byte aligned buffers.  `workspace`: ncahip_cond_grow_bwd_workspace() bytes.
 *   T = 1 is the backward of one ncahip_cond_step_fwd_f32 + ncahip_cond_finalize_f32 pair (slot 0 = x_t, slot 1 = the
 *   pending x'_t the step wrote): there is no separate per-step entry point.                                       */
size_t ncahip_cond_grow_bwd_workspace(int B, int C, int H, int W, int hidden);
int ncahip_cond_grow_bwd_f32(const float *states, const uint8_t *pre, int T,
                             const float *goal, int goal_ch, const float *u,
                             const float *wp, const float *w1, const float *b1,
                             const float *w2, const float *b2, const float *w3,
                             int B, int C, int H, int W, int hidden,
                             int alive_ch, float alive_thr, float fire_rate,
                             float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step0,
                             const float *g_final, float *g_x0, float *g_goal,
                             float *g_wp, float *g_w1, float *g_b1, float *g_w2, float *g_b2, float *g_w3,
                             void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* The same backward over a bf16 history: states [T+1 slots] and goal as stored by ncahip_cond_grow_fwd_bf16 with ring = T+1
 * (BASELINE configs[2]: a bf16 pool halves the saved-for-backward set).  Mixed precision as in the forward: the stored values
 * are widened exactly; perception, masks, gating and every stored gradient (g_final, outputs, scratch) are fp32; the matrix
 * products -- the recomputed UpdateNet with the forward's rounding points, the data path through W3^T / W2^T / W1^T, and
 * the three weight-gradient products over the cell axis -- run on v_mfma_f32_16x16x16_bf16 with fp32 accumulation (92 MFMAs
 * of 8 cycles per 16 cells instead of 368 exact-f32 ones of 32).  Straight-through with respect to the storage rounding;
 * bound against the exact-fp32 products of the same history and against the fp32 gradients in tests/.
 * W % 4 == 0, states / goal 8-byte aligned.                                                                             */
int ncahip_cond_grow_bwd_bf16(const uint16_t *states, const uint8_t *pre, int T,
                              const uint16_t *goal, int goal_ch, const float *u,
                              const float *wp, const float *w1, const float *b1,
                              const float *w2, const float *b2, const float *w3,
                              int B, int C, int H, int W, int hidden,
                              int alive_ch, float alive_thr, float fire_rate,
                              float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step0,
                              const float *g_final, float *g_x0, float *g_goal,
                              float *g_wp, float *g_w1, float *g_b1, float *g_w2, float *g_b2, float *g_w3,
                              void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* ---- T DyNCA steps in ONE launch (B = 1 video inference) --------------------------------------------------------------
 * ConditioneDyNCA/utils/misc/video_utils.py:50-82 (forward_nsteps(h, step_n, cond_img=frame) per frame, step_n = 8 by default;
 * WebGL twin docs/dynca.js:1057-1132).  x_out = the state after T steps from x_in (x_in != x_out), bit for bit what
 * ncahip_dynca_nsteps_fwd_f32 computes, but every 16 x 16 tile is owned by one workgroup for all T steps: weights and
 * conditioning staged once, the tile's state kept in LDS, only the one-cell halo exchanged per step -- as (value, tag) pairs in
 * `workspace`, tag = epoch * 4096 + step, so neighbours need no counters and the call is ONE launch (no copy, no memset).
 * Workspace contract: ncahip_dynca_nsteps_persist_workspace bytes, 256-byte aligned, ZEROED ONCE by the caller when allocated;
 * every call on it passes a strictly larger `epoch` than the one before (1, 2, ... < 2^20; zero it again and restart at 1 when
 * that runs out) -- stale pairs of earlier launches then never match.  Because the epoch is a kernel argument the call can NOT be
 * captured into a graph and replayed (a replay would repeat the epoch and meet the previous replay's equally tagged pairs): on a
 * stream that is capturing, both entry points return NCAHIP_ERANGE after the argument checks, nothing enqueued.  Covered: C <= 16, fc <= 128, H % 16 == 0, W % 16 == 0,
 * T < 4096, and every tile's workgroup resident at once (occupancy x CUs >= B * H/16 * W/16: 1 x 256 x 256 is exactly one per CU
 * of an MI355X); NCAHIP_ERANGE otherwise -- the caller then runs ncahip_dynca_nsteps_fwd_f32.  The workspace query returns 0 for
 * shapes that are never covered.  A neighbour that never becomes resident (another process holding CUs) makes a bounded poll
 * expire: the launch still drains, bit 1 of the sticky device error word is set and ncahip_check_errors / the next driver call
 * report NCAHIP_EDEVICE (x_out is then not valid). */
size_t ncahip_dynca_nsteps_persist_workspace(int B, int C, int H, int W, int fc, int c_cond);
int ncahip_dynca_nsteps_fwd_persist_f32(const float *x_in, float *x_out, int T, const float *cond, const float *u,
                                        const float *w1, const float *b1, const float *w2, const float *b2,
                                        int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                        float update_rate, uint64_t seed, uint64_t step0,
                                        void *workspace, size_t workspace_bytes, unsigned epoch, ncahip_stream_t stream);
/* The same for perception_scales = [0, 1] (every shipped video model; dynca.py:75-115): bit for bit what
 * ncahip_dynca_nsteps_fwd_ms_f32 computes.  Tiles additionally exchange the 2 x 2 means of their coarse cells within 2 of the
 * border; same workspace, epoch and coverage rules (NCAHIP_PAD_REFLECT with H < 4 or W < 4: NCAHIP_EINVAL, as there). */
int ncahip_dynca_nsteps_fwd_persist_ms_f32(const float *x_in, float *x_out, int T, const float *cond, const float *u,
                                           const float *w1, const float *b1, const float *w2, const float *b2,
                                           int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                           float update_rate, uint64_t seed, uint64_t step0,
                                           void *workspace, size_t workspace_bytes, unsigned epoch, ncahip_stream_t stream);
/* ---- a whole ConditionedNCA grow in ONE launch (small grids: the reference's training shape, 8 x 20 x 64^2) ---------------
 * Same contract and results as ncahip_cond_grow_fwd_f32 (nca.py:152-209), bit for bit, but every 16 x 16 tile is owned by one
 * workgroup for all T steps and the final finalize: weight image and goal tile staged once, the tile's pending state in LDS, and
 * per step one exchange of each tile's border band (x' ring, alpha' 3 deep, pre mask 2 deep) as (value, tag) pairs in
 * `workspace`, tag = epoch * 4096 + step.  ring == T + 1: states slots 1..T and pre slots 1..T are written exactly as the per-step
 * driver writes them (ncahip_cond_grow_bwd_f32 consumes them unchanged); slot 0 of `states` holds the input.  ring == 2: `states`
 * slot 0 is the input and only x_final is defined (pre may be NULL).
 * Workspace contract: ncahip_cond_grow_persist_workspace bytes (pure host arithmetic; 0 for shapes that are never covered),
 * 256-byte aligned, ZEROED ONCE by the caller; every call passes a strictly larger epoch (1 .. 2^20 - 1).  Because the epoch is a
 * kernel argument the call can NOT be captured into a graph and replayed: on a stream that is capturing it returns NCAHIP_ERANGE after
 * the argument checks and the sticky-word refusal, nothing enqueued.
 * Covered: C <= 20, hidden == 64, goal_ch >= 0, alive_ch >= 0 or < 0, H % 16 == 0, W % 16 == 0, T < 4096, bit-packed fire masks
 * (NCAHIP_SEED_U_IS_BITS) or in-kernel Philox (u == NULL), 16-byte aligned states / x_final / goal, precision mode 0 and no
 * ncahip_debug_force_generic bit, and B * H/16 * W/16 tiles <= the device's CUs (one workgroup per CU, every tile resident);
 * NCAHIP_ERANGE otherwise (explicit float uniforms included) -- the caller then runs ncahip_cond_grow_fwd_f32.  Arguments are
 * checked on the host first (NCAHIP_EINVAL / NCAHIP_ERANGE, nothing enqueued); then a set sticky error word refuses the call
 * exactly as ncahip_cond_grow_fwd_f32 does (NCAHIP_EDEVICE); residency is tested last.  Every neighbour poll is bounded (2 s of
 * device wall clock); on expiry bit 1 of the sticky error word is set, the launch drains and x_final holds NaN. */
size_t ncahip_cond_grow_persist_workspace(int B, int C, int H, int W, int hidden, int goal_ch);
int ncahip_cond_grow_fwd_persist_f32(float *states, uint8_t *pre, int ring, int T, float *x_final,
                                     const float *goal, int goal_ch, const float *u, const float *wp, const float *w1,
                                     const float *b1, const float *w2, const float *b2, const float *w3, int B, int C,
                                     int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate,
                                     float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step0, void *workspace,
                                     size_t workspace_bytes, unsigned epoch, ncahip_stream_t stream);
/* Test hook: the next persistent DyNCA launches leave out their last n tiles -- what a workgroup that never becomes resident
 * looks like to its neighbours (their bounded polls expire; the launch drains; NCAHIP_EDEVICE).  0 restores normal launches.
 * (The persistent ConditionedNCA grow does not take it.) */
int ncahip_debug_persist_drop_tiles(int n);

/* ---- a whole clip per call: frame front end, DyNCA steps, image output -------------------------------------------------
 * ConditioneDyNCA/utils/misc/video_utils.py:50-83 (`save_video`): for every target frame, steps_per_frame times
 * { forward_nsteps(h, step_n, cond_img = grey(frame)); emit clip(rgb, -1, 1) * 0.5 + 0.5 }, the state carried across frames.
 * Three entry points: the conditioning of all frames of a call in one pass, one output image from a state, and the driver that
 * enqueues the existing step entry points and the image output for F frames.  Nothing here synchronises.
 *
 * Formats of frames in and images out: */
#define NCAHIP_CLIP_F32_NCHW 0   /* float32, channels first: frames [F,B,3,H,W] in network range [-1, 1]; images [B,c_out,H,W] in [0, 1] */
#define NCAHIP_CLIP_U8_NHWC  1   /* uint8, channels last (what decoders and encoders use): frames [F,B,H,W,3]; images [B,H,W,c_out]     */
/* ncahip_clip_cond: cond [F,B,3,H,W] = EdgeExtractor(grey(frame)) (dynca.py:204-213; k3 [3][9], zero padding and apply_tanh as
 *   ncahip_edge_extractor_f32), grey = gray_r * r + gray_g * g + gray_b * b: (1/3, 1/3, 1/3) is the reference's RGBToGrayscale
 *   (utils/misc/preprocess_texture.py:178-179, the channel mean), (0.2989, 0.587, 0.114) the ITU-R 601 luma.  uint8 frames are
 *   widened as preprocess_texture.py:28, :54: v = float(u8) / 255.0f (a true division), then v * 2 - 1.  Every input pixel is read once
 *   per workgroup (16 x 64 tile + halo in LDS).  ncahip_clip_cond_workspace: bytes of cond (host arithmetic; 0 for a non-positive size).
 * ncahip_clip_emit: img = (clamp(2 * state[:, :c_out], -1, 1) + 1) / 2 (video_utils.py:78-81, dynca.py:140-141), bit for bit the torch
 *   expression; uint8 output = (uint8_t)(img * 255.0f), truncating as VideoWriter.add's np.uint8 (video_utils.py:26).  1 <= c_out <= 4,
 *   c_out <= C.
 * ncahip_dynca_clip_f32: for f in 0..F-1, j in 0..steps_per_frame-1, n = f * steps_per_frame + j: step_n DyNCA steps on the state with
 *   cond[f] (c_cond = 3), then image n = ncahip_clip_emit(state) into images + n * (one image).
 *   states: 2 slots of B*C*H*W floats; slot 0 holds the state on entry and on return, slot 1 is scratch.
 *   u: NULL = in-kernel Philox, call n uses steps step0 + n * step_n ...; bit-packed masks (seed == NCAHIP_SEED_U_IS_BITS) or float
 *   uniforms of all F * steps_per_frame * step_n steps laid end to end.
 *   two_scale != 0: perception_scales = [0, 1] (the _ms_ entry points; pc_scratch [B,4C,H/2,W/2] required).
 *   The steps are the library's existing entry points, unchanged: with persist_ws != NULL each call n first goes to
 *   ncahip_dynca_nsteps_fwd_persist_f32 / _ms_f32 with epoch epoch0 + n (persist_ws as that entry point documents; NCAHIP_EINVAL when
 *   epoch0 < 1 or epoch0 + F * steps_per_frame >= 2^20); from its first NCAHIP_ERANGE on, and always with persist_ws == NULL, the calls
 *   run on ncahip_dynca_nsteps_fwd_f32 / _ms_f32 with ring 2 over `states`.  What those entry points cover, this one covers, with their
 *   bits; what they refuse, it refuses with their code.  Because the epochs are kernel arguments the persistent launches can NOT be
 *   captured into a graph and replayed: on a capturing stream the first call's persistent entry point returns NCAHIP_ERANGE, so a captured
 *   clip holds the per-step launches only (pass persist_ws == NULL there and no epoch is spent).
 *   Arguments are checked on the host before anything is enqueued (null or overlapping buffers, F, steps_per_frame, step_n <= 0, c_out,
 *   an unknown format, the epoch range: NCAHIP_EINVAL; shapes the step entry points refuse: their code); a set sticky error word refuses
 *   the call with NCAHIP_EDEVICE, as the grow drivers do; the driver stops enqueuing at the first failing launch and returns its code. */
size_t ncahip_clip_cond_workspace(int F, int B, int H, int W);
int ncahip_clip_cond(const void *frames, int frame_fmt, const float *k3, float gray_r, float gray_g, float gray_b, int apply_tanh,
                     float *cond, int F, int B, int H, int W, ncahip_stream_t stream);
int ncahip_clip_emit(const float *state, void *img, int img_fmt, int B, int C, int c_out, int H, int W, ncahip_stream_t stream);
int ncahip_dynca_clip_f32(float *states, const float *cond, void *images, int img_fmt, int F, int steps_per_frame, int step_n,
                          const float *u, const float *w1, const float *b1, const float *w2, const float *b2,
                          int B, int C, int c_out, int H, int W, int fc, int pad_mode, int two_scale, float update_rate,
                          uint64_t seed, uint64_t step0, float *pc_scratch, void *persist_ws, size_t persist_bytes,
                          unsigned epoch0, ncahip_stream_t stream);

/* ---- a whole clip per call, extra-channel models: the grey frame is the LAST state channel ----------------------------------
 * ExtraChannels/utils/misc/video_utils.py:66-82: for every target frame, steps_per_frame times
 * { h = cat(h, grey(frame)); state, rgb = forward_nsteps(h, step_n); h = state[:, :-1]; emit clip(rgb, -1, 1) * 0.5 + 0.5 }.  The model
 * has C = c_in channels, the last one the conditioning image, which evolves with the rest during a call and is replaced before the
 * next; its cond map is the positional encoding (CPE, c_cond = 2, the same for every frame) or none.  Formats as above.
 * ncahip_clip_gray: gray [F,B,H,W] = gray_r * r + gray_g * g + gray_b * b of every frame of a call in one launch; weights and the
 *   widening of uint8 frames as ncahip_clip_cond, whose loader it shares (aligned dwords at any alignment of the tensor and any W * 3).
 * ncahip_clip_emit_inject: one launch for the two things that happen between two calls.  img != NULL: img = ncahip_clip_emit(state), the
 *   same bits.  gray != NULL: state[:, C-1] = gray [B,H,W].  The image reads channels below c_out, the plane goes to channel C-1:
 *   1 <= c_out <= 4 and c_out <= C-1.  img == NULL: inject only (before the first call); gray == NULL: emit only; both NULL:
 *   NCAHIP_EINVAL.  State, image and plane must not overlap.
 * ncahip_dynca_clip_xc_f32: ncahip_dynca_clip_f32 for these models.  For call n = f * steps_per_frame + j: channel C-1 of the current
 *   state is replaced by gray[f] (before EVERY call, the repeats j > 0 included, as the reference's cat does), then step_n steps run
 *   with cond, then image n is written.  A clip is one inject launch, then per call the step launch(es) and one emit + inject launch.
 *   gray: [F,B,H,W], from ncahip_clip_gray.  cond: ONE map [B,c_cond,H,W] for all frames, c_cond = 2; or NULL with c_cond = 0.
 *   states, u, two_scale, pc_scratch, persist_ws / epoch0, the routes (persistent entry points, per-step ring from the first NCAHIP_ERANGE
 *   on), the host-side checks, the sticky error word and the return codes: as ncahip_dynca_clip_f32, with which it shares its body.  As
 *   there, the persistent launches can NOT be captured into a graph and replayed: on a capturing stream their entry point returns
 *   NCAHIP_ERANGE and the captured clip holds the per-step launches only.  In
 *   addition NCAHIP_EINVAL for gray == NULL, c_cond other than 0 or 2, a cond pointer that does not match c_cond, c_out > C-1, and gray
 *   overlapping states, cond or images.  On return slot 0 of states holds all C channels, the last one the extra channel as the last
 *   call's steps left it: dropping it (h = state[:, :-1]) is the caller's job. */
int ncahip_clip_gray(const void *frames, int frame_fmt, float gray_r, float gray_g, float gray_b, float *gray, int F, int B, int H, int W,
                     ncahip_stream_t stream);
int ncahip_clip_emit_inject(float *state, void *img, int img_fmt, const float *gray, int B, int C, int c_out, int H, int W,
                            ncahip_stream_t stream);
int ncahip_dynca_clip_xc_f32(float *states, const float *gray, const float *cond, int c_cond, void *images, int img_fmt, int F,
                             int steps_per_frame, int step_n, const float *u, const float *w1, const float *b1, const float *w2,
                             const float *b2, int B, int C, int c_out, int H, int W, int fc, int pad_mode, int two_scale,
                             float update_rate, uint64_t seed, uint64_t step0, float *pc_scratch, void *persist_ws,
                             size_t persist_bytes, unsigned epoch0, ncahip_stream_t stream);

/* ---- a whole clip per call, ConditionedNCA: fused encoder, grow per frame, image output ------------------------------------------
 * EncoderConditioning/visualisation.ipynb (ConditionedNCAVisualizer.loop with button_fn: the state is carried, the goal image changes):
 * for every frame, steps_per_frame times { state = grow(state, step_n, frame); emit clamp(state[:, :3], 0, 1) } (trainer.py:36-39,
 * utils/utils.py:34-35).  Formats as above, except that float32 frames are ToTensor output in [0, 1] and are used as they are, and uint8
 * frames are widened as float(u8) / 255.0f (a true division) with no * 2 - 1.  Nothing here synchronises.
 * ncahip_clip_encode: goal [F,B,E,H,W] = ImageEncoder(frame) (encoder.py:37-57) for every frame of a call in ONE launch, inference only:
 *   gray = mean over the ch channels; feat [3+ch] = [sobel_x(gray) | sobel_y(gray) | laplacian(gray) | blur5x5(img[c])], zero padding, k3 [3][9]
 *   and k5 [25] as ncahip_image_encoder_front_f32; h1 = relu(conv3x3(feat, w1 [E,3+ch,3,3]) + b1 [E]), zero padding; goal = conv3x3(h1,
 *   w2 [E,E,3,3]), zero padding (h1 counts as 0 outside the image), no bias.  float32 frames [F,B,ch,H,W] with ch <= 4, uint8 frames
 *   [F,B,H,W,3] (ch == 3; any alignment, any W * 3); 1 <= E <= 32; any H, W >= 1; NCAHIP_ERANGE otherwise.  Null, overlapping, non-positive or
 *   unknown-format arguments: NCAHIP_EINVAL.  All checked before the launch.  One workgroup per 16 x 16 output tile: the image tile with a
 *   4-cell halo, feat on tile + 2 and h1 on tile + 1 live in LDS; both convolutions run on the exact-f32 MFMA (16 x 16 x 4) as implicit GEMMs
 *   per tap.  No workspace beyond goal: ncahip_clip_encode_workspace returns its bytes (host arithmetic; 0 for a non-positive size).
 * ncahip_clip_emit_unit: img = clamp(state[:, :3], 0, 1), bit for bit the torch expression on the device (NaN passes through); float32
 *   [B,3,H,W], or uint8 [B,H,W,3] = (uint8_t)(img * 255.0f), truncating.  C >= 3.
 * ncahip_cond_clip_f32: for f in 0..F-1, j in 0..steps_per_frame-1, n = f * steps_per_frame + j: step_n ConditionedNCA steps and the finalize
 *   on the state with goal[f] (goal [F,B,goal_ch,H,W], from ncahip_clip_encode), then image n = ncahip_clip_emit_unit(state) into
 *   images + n * (one image).  Host code over the existing grow drivers; no step kernel of its own.
 *   states: 4 slots of B*C*H*W floats.  Slot 0 holds the state on entry and on return; slots 1..3 are scratch.  Between calls the driver keeps
 *   the state in slot 0 or 2: a persistent call reads one and writes the other; a per-step call runs the ring of that slot and the next one
 *   and finalizes into the slot it started from (step_n odd) or into the other of slots 0 / 2 (step_n even: x_final must not be the pending
 *   slot).  No copy per call n; one device-to-device copy at the end when the state ended in slot 2.  pre: 2 slots of B*H*W bytes, scratch.
 *   u: NULL = in-kernel Philox, call n uses steps step0 + n * step_n ...; bit-packed masks (seed == NCAHIP_SEED_U_IS_BITS) or float uniforms
 *   of all F * steps_per_frame * step_n steps laid end to end.
 *   With persist_ws != NULL each call n first goes to ncahip_cond_grow_fwd_persist_f32 (ring 2) with epoch epoch0 + n (persist_ws as that
 *   entry point documents; NCAHIP_EINVAL when epoch0 < 1 or epoch0 + F * steps_per_frame >= 2^20); from its first NCAHIP_ERANGE on (float
 *   uniforms included), and always with persist_ws == NULL, the calls run on ncahip_cond_grow_fwd_f32 with ring 2.  What those entry points
 *   cover, this one covers, with their bits; what they refuse, it refuses with their code.  A capturing stream is such a refusal
 *   (NCAHIP_ERANGE: the persistent grow can NOT be captured into a graph and replayed), so a captured clip holds the per-step launches only.
 *   Arguments are checked on the host before anything is enqueued (null or overlapping buffers, F, steps_per_frame, step_n <= 0, C < 3, an
 *   unknown format, the epoch range: NCAHIP_EINVAL; shapes the grow drivers refuse: their code); then a set sticky error word refuses the call
 *   with NCAHIP_EDEVICE; the driver stops enqueuing at the first failing launch and returns its code. */
size_t ncahip_clip_encode_workspace(int F, int B, int E, int H, int W);
int ncahip_clip_encode(const void *frames, int frame_fmt, const float *k3, const float *k5, const float *w1, const float *b1, const float *w2,
                       float *goal, int F, int B, int ch, int E, int H, int W, ncahip_stream_t stream);
int ncahip_clip_emit_unit(const float *state, void *img, int img_fmt, int B, int C, int H, int W, ncahip_stream_t stream);
int ncahip_cond_clip_f32(float *states, uint8_t *pre, const float *goal, int goal_ch, void *images, int img_fmt, int F, int steps_per_frame,
                         int step_n, const float *u, const float *wp, const float *w1, const float *b1, const float *w2, const float *b2,
                         const float *w3, int B, int C, int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                         float clamp_hi, uint64_t seed, uint64_t step0, void *persist_ws, size_t persist_bytes, unsigned epoch0,
                         ncahip_stream_t stream);

/* ---- a whole clip per call, ConditionedNCA on a bf16 state ------------------------------------------------------------------------
 * The entry points above for a state and a goal stored as bf16 (uint16_t bit patterns; "bf16 state storage" above: the steps are
 * ncahip_cond_step_fwd_bf16's).  Formats, codes and message words as their fp32 siblings'.  Nothing here synchronises.
 * ncahip_clip_encode_bf16: ncahip_clip_encode with the goal [F,B,E,H,W] stored as bf16: the same kernel and arithmetic, the final store
 *   rounds to bf16 (round-to-nearest-even) -- bit for bit ncahip_clip_encode followed by a cast.  Arguments, ranges and checks as
 *   ncahip_clip_encode; the goal's bytes are halved in the overlap checks and the goal is 2-byte aligned (NCAHIP_EINVAL).
 * ncahip_clip_emit_unit_bf16: ncahip_clip_emit_unit reading a bf16 state [B,C,H,W] (2-byte aligned: NCAHIP_EINVAL), every image format
 *   of that entry point, the planar ones included: bit for bit the fp32 emit of the widened state.
 * ncahip_cond_finalize_emit_bf16: ONE launch for ncahip_cond_finalize_bf16(x_pend, pre) -> x_out and then
 *   ncahip_clip_emit_unit_bf16(x_out) -> img: the alive pool, the clamp and the image in one pass over the pending state (one launch and
 *   one read of the state fewer per image); x_out and img are bit for bit those of the two launches.  Any B, H, W and C >= 3 (the image
 *   is x_out[:, :3]), 2-byte aligned states; a lane takes 4 cells of a row (2 x 4 for a planar image) -- as 8-byte words where W % 4 == 0
 *   and the states are 8-byte aligned.  x_out == x_pend only with alive_ch < 0.  NCAHIP_EINVAL: a null pointer (pre may be null with
 *   alive_ch < 0), an unknown format, a non-positive size, C < 3, alive_ch >= C, a misaligned state or float32 image, img overlapping
 *   x_pend, x_out or pre.  NCAHIP_ERANGE: a planar format with odd H or W.
 * ncahip_cond_clip_bf16: the loop of ncahip_cond_clip_f32 on the bf16 step launches.  states: 4 slots of B*C*H*W bf16 values, the state
 *   in slot 0 on entry and on return; pre: 2 slots of B*H*W bytes; goal [F,B,goal_ch,H,W] bf16 (from ncahip_clip_encode_bf16); u, seed
 *   and step0 as ncahip_cond_clip_f32 (NULL = in-kernel Philox; bit-packed masks or float uniforms of all steps laid end to end).
 *   There is no persistent bf16 grow, hence no workspace: every call n runs the ring of slots {cur, cur + 1} -- its step_n steps
 *   enqueued exactly as ncahip_cond_grow_fwd_bf16 enqueues them -- and ends with ncahip_cond_finalize_emit_bf16's launch, which writes
 *   the resolved state to slot cur (step_n odd) or to the other of slots 0 / 2 (step_n even) and image n.  At most one device-to-device
 *   copy per call of the driver, when the state ended in slot 2.  Covers what ncahip_cond_grow_fwd_bf16 covers -- C <= 20, W % 4 == 0,
 *   8-byte aligned states and goal -- and refuses the rest with that entry point's code (NCAHIP_ERANGE).  Arguments are checked on the
 *   host before anything is enqueued (null or overlapping buffers, F, steps_per_frame, step_n <= 0, C < 3, an unknown format:
 *   NCAHIP_EINVAL; a planar format with odd H or W: NCAHIP_ERANGE); then a set sticky error word refuses the call with NCAHIP_EDEVICE;
 *   the driver stops enqueuing at the first failing launch and returns its code. */
int ncahip_clip_encode_bf16(const void *frames, int frame_fmt, const float *k3, const float *k5, const float *w1, const float *b1, const float *w2,
                            uint16_t *goal, int F, int B, int ch, int E, int H, int W, ncahip_stream_t stream);
int ncahip_clip_emit_unit_bf16(const uint16_t *state, void *img, int img_fmt, int B, int C, int H, int W, ncahip_stream_t stream);
int ncahip_cond_finalize_emit_bf16(const uint16_t *x_pend, const uint8_t *pre, uint16_t *x_out, void *img, int img_fmt, int B, int C, int H, int W,
                                   int alive_ch, float alive_thr, float clamp_lo, float clamp_hi, ncahip_stream_t stream);
int ncahip_cond_clip_bf16(uint16_t *states, uint8_t *pre, const uint16_t *goal, int goal_ch, void *images, int img_fmt, int F, int steps_per_frame,
                          int step_n, const float *u, const float *wp, const float *w1, const float *b1, const float *w2, const float *b2,
                          const float *w3, int B, int C, int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                          float clamp_hi, uint64_t seed, uint64_t step0, ncahip_stream_t stream);

/* ---- a whole clip per call, decoder-sized frames: crop + resize of uint8 frames, bit for bit Pillow's 8-bit Image.resize -------------
 * A decoder delivers 1080p or 720p uint8 frames; the models run at 128^2 .. 512^2.  The reference shrinks on the host with Pillow:
 * preprocess_style_image (ConditioneDyNCA/utils/misc/preprocess_texture.py:9-33: symmetric centre cut, then Image.resize = bicubic) and
 * load_image (EncoderConditioning/utils/utils.py:5-25: square crop, then resize(..., Image.LANCZOS)).  Pillow's 8-bit resize is an integer
 * algorithm, reproduced here exactly.  The resize sees only the cropped image: `in` below is the cropped length, tap indices count from
 * the crop's first pixel and end at its last.
 * The arithmetic, per axis, for input length in, output length out and a filter f of support s (C double throughout; (int) truncates):
 *   NCAHIP_RESIZE_BICUBIC: s = 2, a = -0.5; |x| < 1: ((a + 2)|x| - (a + 3))|x|^2 + 1; |x| < 2: (((|x| - 5)|x| + 8)|x| - 4) a; else 0
 *   NCAHIP_RESIZE_LANCZOS: s = 3; sinc(x) sinc(x / 3) on -3 <= x < 3 (sinc(x) = sin(pi x) / (pi x), 1 at 0); else 0
 *   scale = in / out; fs = max(scale, 1); sup = s * fs; ksize = 2 * ceil(sup) + 1 (the row width of the table)
 *   output index i: center = (i + 0.5) * scale; xmin = max((int)(center - sup + 0.5), 0); n = min((int)(center + sup + 0.5), in) - xmin;
 *     w[j] = f((j + xmin - center + 0.5) * (1 / fs)) for j < n (Pillow multiplies by the reciprocal; so does the builder);
 *     w[j] /= sum(w) (summed in index order) when the sum is not 0;
 *     k[j] = (int)(w[j] * 2^22 + 0.5) for w[j] >= 0, (int)(w[j] * 2^22 - 0.5) otherwise; k[j] = 0 for n <= j < ksize
 *   a pass: out = clamp((2^21 + sum_{j < n} px[xmin + j] * k[j]) >> 22, 0, 255) per channel, int32 accumulation, arithmetic shift.
 *   The horizontal pass runs first and writes a uint8 image [crop_h, out_w, 3]; the vertical pass reads that image.
 * ncahip_resize_ksize: ksize of (in, out, filter); host arithmetic.  in, out <= 0 or an unknown filter: NCAHIP_EINVAL.
 * ncahip_resize_tables: fills k [out, ksize] and bounds [out, 2] = (xmin, n) in CALLER (host) memory; plain host code with floating-point
 *   contraction off, no GPU call -- usable on a machine without a GPU.  ksize must be ncahip_resize_ksize's value (NCAHIP_EINVAL
 *   otherwise).  Checks per row 255 * sum|k| + 2^21 < 2^31 and |k| < 2^23 (what the passes' int32 / 24-bit arithmetic needs; the largest
 *   sum|k| observed is 1.56 * 2^22): NCAHIP_ERANGE if a row breaks it.  This is the only implementation of the table arithmetic.
 * ncahip_clip_resize_u8: src [N,H,W,3] uint8 (any alignment, any W * 3) -> dst [N,out_h,out_w,3] uint8; the crop is columns
 *   x0 .. x0 + crop_w - 1 and rows y0 .. y0 + crop_h - 1 of every frame.  kx / bx: the tables of (crop_w -> out_w) and ky / by those of
 *   (crop_h -> out_h), copied to DEVICE memory, row widths ksize_x / ksize_y.  workspace: ncahip_clip_resize_workspace(N, crop_h, out_w) =
 *   N * crop_h * out_w * 3 bytes of device memory for the intermediate image.  Two launches for all N frames: the horizontal pass (a
 *   workgroup = a band of rows x a block of output columns; coefficient rows and the source row segments in LDS, the latter as
 *   memory-aligned dwords; a loop over the runtime tap count) and the vertical pass (a lane per 4 output bytes of a row when out_w * 3 and
 *   the buffers are 4-byte aligned, else per byte; coefficients wave-uniform).  The tables are not trusted with addresses: (xmin, n) of
 *   every row is cut to the crop before the tap loop, so a wrong table gives wrong pixels and never a read outside the frame.  Nothing
 *   synchronises.  NCAHIP_ERANGE: H, W, out_h or out_w above 16384, ksize_x or ksize_y above 2048, a crop outside the frame, a null or
 *   not 4-byte aligned table or workspace.  NCAHIP_EINVAL: null src / dst, a non-positive size, a short workspace, overlapping
 *   src / dst / workspace.  All checked before the first launch.  Same size and no crop: the tables are the identity, dst = src. */
#define NCAHIP_RESIZE_BICUBIC 0
#define NCAHIP_RESIZE_LANCZOS 1
int ncahip_resize_ksize(int in, int out, int filter);
int ncahip_resize_tables(int in, int out, int filter, int32_t *k, int32_t *bounds, int ksize);
size_t ncahip_clip_resize_workspace(int N, int crop_h, int out_w);
int ncahip_clip_resize_u8(const uint8_t *src, int N, int H, int W, int x0, int y0, int crop_w, int crop_h, const int32_t *kx,
                          const int32_t *bx, int ksize_x, const int32_t *ky, const int32_t *by, int ksize_y, uint8_t *dst, int out_h,
                          int out_w, void *workspace, size_t workspace_bytes, ncahip_stream_t stream);

/* ---- a whole clip per call, planar YUV frames: I420 / NV12 in, RGB24 on the device -------------------------------------------------
 * A decoder does not deliver RGB24: it delivers planar YUV 4:2:0, 1.5 bytes per pixel, and RGB exists only after a colour conversion.
 * The reference never sees YUV (cv2 / moviepy hand it RGB), so there is no reference arithmetic to reproduce; this section fixes one.
 * Matrix NCAHIP_YUV_BT601 (Kr = 0.299, Kb = 0.114) or NCAHIP_YUV_BT709 (Kr = 0.2126, Kb = 0.0722); Kg = 1 - Kr - Kb.
 * Range NCAHIP_YUV_LIMITED: y' = Y - 16, sy = 255/219, sc = 255/224; NCAHIP_YUV_FULL: y' = Y, sy = sc = 1.  u' = U - 128, v' = V - 128.
 * The real-valued definition:
 *   R = sy y' + 2 (1 - Kr) sc v'
 *   G = sy y' - (2 Kb (1 - Kb) / Kg) sc u' - (2 Kr (1 - Kr) / Kg) sc v'
 *   B = sy y' + 2 (1 - Kb) sc u'
 * The integer evaluation (the contract): every coefficient c is computed in C double and quantised to k = (int)(c * 2^16 + 0.5), or
 *   (int)(c * 2^16 - 0.5) for c < 0;  channel = clamp((k_y y' + k_u u' + k_v v' + 2^15) >> 16, 0, 255), int32 accumulation, arithmetic
 *   shift.  Over all 2^24 (Y, U, V) triples |accumulator| stays below 2^26, the result is never more than 1 away from the real-valued
 *   definition rounded half up, and differs from it on at most 5.2e-4 of a channel's values (bt601 full, B).
 *   (k_y, k_rv, k_gu, k_gv, k_bu):  bt601 limited 76309 104597 -25675 -53279 132201      bt601 full 65536  91881 -22553 -46802 116130
 *                                   bt709 limited 76309 117489 -13975 -34925 138438      bt709 full 65536 103206 -12276 -30679 121609
 * Chroma is nearest: pixel (x, y) uses chroma sample (x >> 1, y >> 1); no interpolation, no siting filter.
 * Layouts, per frame of h x w pixels (h, w even), uint8 [3h/2, w]: NCAHIP_YUV_I420 = the Y plane (h x w bytes), then U (h/2 x w/2), then V;
 *   NCAHIP_YUV_NV12 = the Y plane, then h/2 rows of w bytes with U and V interleaved (U first).
 * ncahip_yuv_coeffs: k[0..4] = (k_y, k_rv, k_gu, k_gv, k_bu), k[5] = the luma offset (16 or 0), into CALLER (host) memory; plain host
 *   code with floating-point contraction off, no GPU call.  An unknown matrix or range, or a null k: NCAHIP_EINVAL.  This is the only
 *   implementation of the coefficient arithmetic.
 * ncahip_clip_yuv420_to_rgb_u8: src [N, 3H/2, W] uint8 -> dst [N, crop_h, crop_w, 3] uint8, the RGB of the crop box (columns
 *   x0 .. x0 + crop_w - 1, rows y0 .. y0 + crop_h - 1; any origin and size, odd ones included).  k: ncahip_yuv_coeffs' six words in HOST
 *   memory (they travel as kernel arguments).  One launch for all N frames, nothing synchronises.  A lane writes one memory-aligned dword
 *   of the output (bytes at a frame's two ends singly) and reads every source byte out of the aligned dword that holds it, inside the
 *   tensor only: any alignment of src and dst and any W are served (plane starts such as byte H*W + H*W/4 are routinely misaligned).
 *   NCAHIP_EINVAL: a null pointer, an unknown layout, a non-positive size, overlapping src / dst.  NCAHIP_ERANGE: H or W above 16384 or
 *   odd, a crop outside the frame.  All checked before the launch.
 * ncahip_clip_resize_yuv420_u8: ncahip_clip_resize_u8 with a planar source: the same tables, workspace, limits and return codes, plus
 *   NCAHIP_EINVAL for a null k or an unknown layout and NCAHIP_ERANGE for odd H or W.  The horizontal pass stages, per row, the luma segment
 *   and the chroma samples under it as memory-aligned dwords and writes the converted RGB bytes into the LDS rows its tap loop reads; no
 *   full-size RGB image exists.  The vertical pass is the same kernel.  The result is bit for bit ncahip_clip_yuv420_to_rgb_u8 on the crop
 *   followed by ncahip_clip_resize_u8 without a crop. */
#define NCAHIP_YUV_I420 0
#define NCAHIP_YUV_NV12 1
#define NCAHIP_YUV_BT601 0
#define NCAHIP_YUV_BT709 1
#define NCAHIP_YUV_LIMITED 0
#define NCAHIP_YUV_FULL 1
int ncahip_yuv_coeffs(int matrix, int range, int32_t k[6]);
int ncahip_clip_yuv420_to_rgb_u8(const uint8_t *src, int layout, int N, int H, int W, int x0, int y0, int crop_w, int crop_h,
                                 const int32_t *k, uint8_t *dst, ncahip_stream_t stream);
int ncahip_clip_resize_yuv420_u8(const uint8_t *src, int layout, const int32_t *k, int N, int H, int W, int x0, int y0, int crop_w,
                                 int crop_h, const int32_t *kx, const int32_t *bx, int ksize_x, const int32_t *ky, const int32_t *by,
                                 int ksize_y, uint8_t *dst, int out_h, int out_w, void *workspace, size_t workspace_bytes,
                                 ncahip_stream_t stream);

/* ---- a whole clip per call, planar YUV images: I420 / NV12 out, straight from the fp32 state ------------------------------------------
 * A video encoder does not take RGB24 either: it takes planar YUV 4:2:0.  The image output of the clip entry points can write it, 1.5
 * bytes per pixel instead of 3, with no RGB image in between.  The reference never produces YUV (moviepy / cv2 take RGB), so this
 * section fixes the arithmetic, as the one above does for the way in.
 * RGB is the uint8 image the emits write: (uint8_t)(img * 255.0f), truncating, img as ncahip_clip_emit defines it for the DyNCA families
 * and as ncahip_clip_emit_unit defines it for ConditionedNCA.  Matrices, ranges, Kr / Kb / Kg and the luma offset yoff (16 or 0) as above;
 * the scales run the other way: NCAHIP_YUV_LIMITED sy = 219/255, sc = 224/255; NCAHIP_YUV_FULL sy = sc = 1.
 * The real-valued definition, with Y' = Kr R + Kg G + Kb B:
 *   Y = yoff + sy Y'        U = 128 + sc (B - Y') / (2 (1 - Kb))        V = 128 + sc (R - Y') / (2 (1 - Kr))
 * The integer evaluation (the contract): coefficients are quantised as the inverse's are, q(c) = (int)(c * 2^16 + 0.5), or
 *   (int)(c * 2^16 - 0.5) for c < 0, in C double with contraction off: k_yr = q(sy Kr), k_yb = q(sy Kb), k_ur = q(-cu Kr),
 *   k_ub = q(cu (1 - Kb)), k_vr = q(cv (1 - Kr)), k_vb = q(-cv Kb) with cu = sc / (2 (1 - Kb)), cv = sc / (2 (1 - Kr)).  In each row the
 *   green coefficient is the remainder that makes the row sum exact: k_yg = q(sy) - k_yr - k_yb, k_ug = -k_ur - k_ub, k_vg = -k_vr - k_vb
 *   (a grey pixel gives U = V = 128 exactly).
 *   Luma, per pixel:         Y = clamp(yoff + ((k_yr R + k_yg G + k_yb B + 2^15) >> 16), 0, 255)
 *   Chroma, per 2 x 2 block, from the block's channel sums (0 .. 1020), one rounding:
 *                            U = clamp(128 + ((k_ur sum R + k_ug sum G + k_ub sum B + 2^17) >> 18), 0, 255), V likewise
 *   int32 accumulation, arithmetic shift; |accumulator| stays below 2^27.  The chroma sample of block (x >> 1, y >> 1) is the block mean
 *   (centre siting): the counterpart of the nearest chroma on the way in.
 *   (R, G, B) rows of Y / U / V:  bt601 limited  16829 33039 6416 |  -9714 -19070 28784 | 28784 -24103 -4681
 *                                 bt601 full     19595 38470 7471 | -11058 -21710 32768 | 32768 -27439 -5329
 *                                 bt709 limited  11966 40254 4064 |  -6596 -22188 28784 | 28784 -26145 -2639
 *                                 bt709 full     13933 46871 4732 |  -7509 -25259 32768 | 32768 -29763 -3005
 *   Over all 2^24 flat colours (and 2^22 random channel sums for chroma) no result is more than 1 away from the real-valued definition
 *   rounded half up, at most 7.7e-4 of a plane's values differ from it (bt709 limited, U), and limited range yields Y in [16, 235] and
 *   chroma in [16, 240] before the clamp.
 * Layouts as above, per image uint8 [3H/2, W] with H and W even: NCAHIP_YUV_I420, NCAHIP_YUV_NV12.
 * NCAHIP_CLIP_YUV420(layout, matrix, range): eight more values (0x100 .. 0x107) of the IMAGE format img_fmt of ncahip_clip_emit,
 *   ncahip_clip_emit_inject, ncahip_clip_emit_unit and of the drivers ncahip_dynca_clip_f32, ncahip_dynca_clip_xc_f32 and
 *   ncahip_cond_clip_f32; image n then lies at images + n * B * 3HW/2 bytes, sample b of it at + b * 3HW/2.  c_out must be 3
 *   (NCAHIP_EINVAL), H and W even (NCAHIP_ERANGE); overlap checks use this size; any byte alignment of the image pointer is served
 *   (plane starts are routinely misaligned: with H = W = 6, V starts at byte 45 and the next image at byte 54).  The coefficients come
 *   from the builder below.  A lane owns 2 rows x 4 columns: it reads each of the three state channels once, forms the truncated bytes in
 *   registers and stores one dword of Y per row and the chroma under it (NV12: one dword of UVUV; I420: two bytes of U and two of V) --
 *   whole dwords where the row segment is 4-byte aligned in memory, 16-bit halves where it is 2-byte aligned, single bytes where a plane
 *   starts on an odd address; the last lane of a row whose W is no multiple of 4 stores half as much.  The extra-channel family's
 *   emit + inject stays one launch.
 *   The result is, bit for bit, the uint8 emit followed by ncahip_clip_rgb_to_yuv420_u8.  As a FRAME format (ncahip_clip_cond,
 *   ncahip_clip_gray, ncahip_clip_encode) these values stay NCAHIP_EINVAL: planar frames come in through the section above.
 * ncahip_rgb_yuv_coeffs: k[0..8] = the nine coefficients in the table's order, k[9] = the luma offset, into CALLER (host) memory; plain
 *   host code with floating-point contraction off, no GPU call.  An unknown matrix or range, or a null k: NCAHIP_EINVAL.  This is the only
 *   implementation of the coefficient arithmetic.
 * ncahip_clip_rgb_to_yuv420_u8: src [N,H,W,3] uint8 -> dst [N,3H/2,W] uint8 in one launch for all N; nothing synchronises.  k:
 *   ncahip_rgb_yuv_coeffs' ten words in HOST memory (they travel as kernel arguments).  Any alignment of src and dst, any even W: a lane
 *   reads its source bytes out of the memory-aligned dwords that hold them, inside the tensor only, and stores as above.  NCAHIP_EINVAL: a
 *   null pointer, an unknown layout, a non-positive size, overlapping src / dst.  NCAHIP_ERANGE: H or W odd or above 16384.  All checked
 *   before the launch. */
#define NCAHIP_CLIP_YUV420(layout, matrix, range) (0x100 | (layout) | (matrix) << 1 | (range) << 2)
int ncahip_rgb_yuv_coeffs(int matrix, int range, int32_t k[10]);
int ncahip_clip_rgb_to_yuv420_u8(const uint8_t *src, int layout, int N, int H, int W, const int32_t *k, uint8_t *dst,
                                 ncahip_stream_t stream);

/* ---- images at delivery size: the 8-bit resize with planar YUV 4:2:0 out --------------------------------------------------------------
 * The clip entry points emit images at the model grid (256^2); an encoder takes them at the size they are delivered in (1080p), as planar
 * YUV.  Enlarging an RGB24 image is ncahip_clip_resize_u8 (Pillow's 8-bit resize enlarges as it shrinks: fs = 1, ksize = 2 s + 1).
 * ncahip_clip_resize_u8_yuv420: src [N,H,W,3] uint8 and the crop, the tables kx / bx / ky / by with their row widths and the workspace
 *   (ncahip_clip_resize_workspace(N, crop_h, out_w)) exactly as ncahip_clip_resize_u8 takes them; layout NCAHIP_YUV_I420 / NCAHIP_YUV_NV12;
 *   k: ncahip_rgb_yuv_coeffs' ten words in HOST memory (they travel as kernel arguments); dst [N, 3 out_h / 2, out_w] uint8.
 *   The result is, bit for bit, ncahip_clip_resize_u8 into an RGB24 image followed by ncahip_clip_rgb_to_yuv420_u8 of that image: the RGB
 *   bytes are clamped after the vertical pass's >> 22, before any YUV arithmetic; luma per pixel; chroma from the 2 x 2 block's channel
 *   sums with one rounding.  No full-size RGB image exists: 1.5 bytes are written per delivered pixel instead of 3 written, 3 read and 1.5
 *   written.  Two launches for all N images: the horizontal pass of ncahip_clip_resize_u8, unchanged, and a vertical pass in which a lane
 *   owns 2 output rows x 4 columns -- it walks the union of the two rows' tap ranges over the intermediate image once (each row's
 *   (ymin, n) cut to the crop; a row's coefficient is 0 outside its own range), keeps 24 accumulators, forms the bytes in registers and
 *   stores as the planar emit does: one dword of Y per row and the chroma under it, whole dwords, 16-bit halves or single bytes by the
 *   segment's alignment in memory, half as much for the last lane of a row with out_w % 4 == 2.  Intermediate rows are 3 out_w bytes, a
 *   multiple of 4 only when out_w % 4 == 0: a lane's 12 bytes are read as the memory-aligned dwords that hold them, inside the workspace
 *   only.  Any alignment of src and dst.  Nothing synchronises.
 *   NCAHIP_EINVAL: null src / dst / k, an unknown layout, a non-positive size, a short workspace, overlapping src / dst / workspace.
 *   NCAHIP_ERANGE: odd out_h or out_w, H, W, out_h or out_w above 16384, ksize_x or ksize_y above 2048, a crop outside the frame, a null
 *   or not 4-byte aligned table or workspace.  All checked before the first launch.  Same size and no crop: the tables are the identity
 *   and dst = ncahip_clip_rgb_to_yuv420_u8(src). */
int ncahip_clip_resize_u8_yuv420(const uint8_t *src, int N, int H, int W, int x0, int y0, int crop_w, int crop_h, const int32_t *kx,
                                 const int32_t *bx, int ksize_x, const int32_t *ky, const int32_t *by, int ksize_y, int layout,
                                 const int32_t *k, uint8_t *dst, int out_h, int out_w, void *workspace, size_t workspace_bytes,
                                 ncahip_stream_t stream);

/* ---- fire masks as bits --------------------------------------------------------------------------------------------
 * Every entry point above that takes `u` (the per-step uniform draws of nca.py:172 / dynca.py:131) also accepts the fire
 * masks ALREADY EVALUATED and bit-packed: pass a non-NULL `u` that points at uint32_t words together with
 * seed == NCAHIP_SEED_U_IS_BITS (seed is otherwise unused when u != NULL).  Layout: per step ceil(B*H*W / 32) words, cell
 * i = (b*H + y)*W + x  <->  bit (i & 31) of word (i >> 5); the multi-step drivers advance by that many words per step.  A
 * set bit = the cell updates (ConditionedNCA: clamp(u,0,1) < fire_rate; DyNCA: floor(u + update_rate) = 1, which needs
 * 0 <= update_rate < 1).  32x smaller than the float draws: what the drop-in classes keep for the backward pass (BASELINE
 * configs[2]: 805 MB of uniforms -> 25 MB).  Needs B*H*W < 2^32.  ncahip_pack_fire_mask_u32 evaluates T steps of float
 * draws u [T][B*H*W] into bits [T][ceil(B*H*W/32)] with exactly the kernels' predicates: mode 0 = ConditionedNCA
 * (nca.py:171-174), mode 1 = DyNCA (dynca.py:131). */
#define NCAHIP_SEED_U_IS_BITS 0x5354494255ull
int ncahip_pack_fire_mask_u32(const float *u, uint32_t *bits, int T, int B, int H, int W, float rate, int mode,
                              ncahip_stream_t stream);

/* ---- relaxed-EMD part of the OT appearance loss -----------------------------------------------------------------------
 * EncoderConditioning/loss/appearance_loss.py:149-174 for one style layer and a batch: with x_i the N sampled feature vectors of
 * the style target and y_j those of generated image b,
 *     d_ij = 1 - <x_i, y_j> / (|x_i| + 1e-10) / (|y_j| + 1e-10),     remd[b] = max(mean_i min_j d_ij, mean_j min_i d_ij).
 * The N x N distances exist only in registers, forwards and backwards.  All fp32.  Covered: c a multiple of 4 up to 512,
 * 1 <= N <= 1024, 1 <= B <= 65535; NCAHIP_ERANGE otherwise.  Results are bit-reproducible from run to run (no atomics).
 *
 * ncahip_ot_gather_f32: t [1, c, HW] (target, shared by the batch) and g [B, c, HW] -> x, y [B, N, c] (row n of sample b = the
 *   feature vector at position idx[b, n]) and the norms xn, yn [B, N] = sqrt(sum v^2).  idx [B, N] int32, positions in [0, HW);
 *   NULL = every position in order (then N == HW).
 * ncahip_ot_gather_bwd_f32: its adjoint for g: dg [B, c, HW] [.., idx[b, n]] = dy [b, n, ..].  Positions of a sample must be distinct;
 *   with idx != NULL the caller zeroes dg first (only the sampled positions are written).
 * ncahip_ot_remd_fwd_f32: rmin [B, N] = min_j d_ij with rarg = its argmin, cmin / carg the same over i, remd [B], and branch [B]:
 *   0 = the row mean won the max, 1 = the column mean, 2 = they are equal.  Ties of a minimum resolve to the lowest index.  x, y and
 *   the workspace (ncahip_ot_workspace bytes: column-minimum partials, combined in a fixed order) 16-byte aligned.
 * ncahip_ot_remd_bwd_f32: dy [B, N, c] = g_remd[b] * d remd[b] / d y (x is the constant target: no gradient), through the argmins of
 *   the winning branch (both, halved, when branch == 2, as torch.maximum does); the norms are functions of x and y here:
 *   d d_ij / d y_j = -xh / s + <xh, y_j> y_j / (|y_j| s^2), xh = x_i / (|x_i| + 1e-10), s = |y_j| + 1e-10; for |y_j| = 0 the second
 *   term is taken as 0. */
size_t ncahip_ot_workspace(int B, int N, int c);
int ncahip_ot_gather_f32(const float *t, const float *g, const int32_t *idx, float *x, float *y, float *xn, float *yn,
                         int B, int c, int HW, int N, ncahip_stream_t stream);
int ncahip_ot_gather_bwd_f32(const float *dy, const int32_t *idx, float *dg, int B, int c, int HW, int N,
                             ncahip_stream_t stream);
int ncahip_ot_remd_fwd_f32(const float *x, const float *y, const float *xn, const float *yn, float *rmin, int32_t *rarg,
                           float *cmin, int32_t *carg, float *remd, int32_t *branch, int B, int N, int c,
                           void *workspace, size_t workspace_bytes, ncahip_stream_t stream);
int ncahip_ot_remd_bwd_f32(const float *x, const float *y, const float *xn, const float *yn, const int32_t *rarg,
                           const int32_t *carg, const int32_t *branch, const float *g_remd, float *dy, int B, int N, int c,
                           ncahip_stream_t stream);

/* ---- moment-matching part of the OT appearance loss -------------------------------------------------------------------
 * EncoderConditioning/loss/appearance_loss.py:176-192 for one style layer and a batch, on the x, y [B, N, c] that
 * ncahip_ot_gather_f32 produces (x the constant target, y the generated image):
 *     mom[b] = mean_k |mx_k - my_k| + mean_kl |Cx_kl - Cy_kl|,   mx = column means over the N rows,
 *     Cx = (x - mx)^T (x - mx) / (N - 1) (unbiased, as in the reference), Cy likewise.
 * The centred copies, the two c x c covariances and their difference exist only in LDS and registers.  All fp32.  Covered: c a
 * multiple of 4 up to 512, 2 <= N <= 1024 (N = 1 divides by zero in the reference), 1 <= B <= 65535; NCAHIP_ERANGE otherwise.
 * Null or aliased pointers: NCAHIP_EINVAL before any launch.  Results are bit-reproducible from run to run (no atomics).
 *
 * ncahip_ot_moment_fwd_f32: mom [B]; my [B, c] the column means of y (refined by one correction pass, so that the columns of
 *   y - my sum to zero to rounding); sgn [B, c] = sign(mx - my) as -1 / 0 / +1 floats; S [B, c, c] int8 = sign(Cx - Cy), both
 *   triangles.  x, y, my, sgn, S and the workspace (ncahip_ot_moment_workspace bytes: mx and the partial sums, combined in a
 *   fixed order) 16-byte aligned.
 * ncahip_ot_moment_bwd_f32: dy [B, N, c] += g_mom[b] * d mom[b] / d y (x gets no gradient), in closed form
 *     dy[b, n, :] += g_mom[b] * (-sgn[b, :] / (c N) - 2 / ((N - 1) c^2) * (y[b, n, :] - my[b, :]) S[b]),   sign(0) = 0;
 *   it ACCUMULATES into dy (plain read-modify-write, one owner per element): call it after ncahip_ot_remd_bwd_f32 has written the
 *   same buffer, then scatter once.  y, my, S and dy 16-byte aligned. */
size_t ncahip_ot_moment_workspace(int B, int N, int c);
int ncahip_ot_moment_fwd_f32(const float *x, const float *y, float *mom, float *my, float *sgn, int8_t *S, int B, int N, int c,
                             void *workspace, size_t workspace_bytes, ncahip_stream_t stream);
int ncahip_ot_moment_bwd_f32(const float *y, const float *my, const float *sgn, const int8_t *S, const float *g_mom, float *dy,
                             int B, int N, int c, ncahip_stream_t stream);

/* ---- position sampler of the OT appearance loss ------------------------------------------------------------------------
 * EncoderConditioning/loss/appearance_loss.py:200-203 draws, per (sample, layer larger than 32 x 32),
 * np.sort(np.random.choice(np.arange(h * w), n, replace = False)) on the host.  This is the same kind of draw on the device, from
 * a keyed stream of its own (NOT numpy's: the positions differ from the reference's, the distribution does not).  A row is one
 * (call, layer, sample) triple with a 64-bit id `row`; for position p in [0, HW)
 *     words = philox4x32_10(counter = (p >> 2, row_lo, row_hi, 0x4F5453 'OTS'), key = (seed_lo, seed_hi)),
 *     key(p) = words[p & 3] >> (32 - key_bits),
 * and the row's result is the n positions with the smallest (key, p) in lexicographic order, written in ascending p.  With
 * distinct keys every n-subset is equally likely.  Equal keys are broken by position, which matters only for a tie exactly at the
 * threshold: with key_bits = 32 (production) that has probability about HW * 2^-32 per row -- the documented deviation from an
 * exactly uniform subset.  key_bits < 32 shortens the keys and makes ties common (it exercises the tie path; not for training).
 *
 * ncahip_ot_sample_idx: idx [rows, n] int32; row r uses the id row0 + r (64-bit arithmetic: the high word is used).  One
 *   workgroup per row: a radix select of the n-th smallest key (8-bit digits, keys regenerated from Philox in every pass), then
 *   an ordered compaction; no atomics on global memory, nothing shared between rows, bit-reproducible.  Covered: 1 <= n <= 1024
 *   (the gather's limit), n <= HW <= 2^20, 1 <= rows <= 65535, 1 <= key_bits <= 32.  A null pointer, a non-positive size, n > HW
 *   or key_bits out of range: NCAHIP_EINVAL; n > 1024, HW > 2^20 or rows > 65535: NCAHIP_ERANGE; both before any launch, with
 *   the offending value in the message.  Refuses with NCAHIP_EDEVICE while the device error word is set. */
int ncahip_ot_sample_idx(int32_t *idx, int rows, int HW, int n, uint64_t seed, uint64_t row0, int key_bits,
                         ncahip_stream_t stream);

/* ---- sliced-Wasserstein style loss ------------------------------------------------------------------------------------
 * EncoderConditioning/loss/appearance_loss.py:109-140 for one level and a batch: source [B, c, n] and target [1, c, m] the
 * flattened feature maps, proj [c, 32] the unit directions (drawn by the caller),
 *     k[b, p, i] = sum_c source[b, c, i] proj[c, p],   s = k sorted ascending along i,   t = the target's keys [32, m] likewise,
 *     loss = sum_{b, p, i} (s[b, p, i] - t[p, jmap[i]])^2          (a sum, not a mean),
 * jmap [n] int32 the index map of F.interpolate(mode = "nearest") from m to n positions (the caller builds it; the kernels clamp it
 * into [0, m)).  The stages are separate entry points.  All fp32.  Covered: c = 3 or a multiple of 4 up to 512, 1 <= n, m <= 65536,
 * 1 <= B <= 1024, at most 65535 rows per sort call; NCAHIP_ERANGE otherwise, with the offending value in the message.  Null or
 * aliased pointers and a short workspace: NCAHIP_EINVAL before any launch.  No atomics: results are bit-reproducible from run to
 * run.  Non-finite inputs are outside the contract (a NaN key has no place in the order, a +inf key ties with the padding).
 *
 * ncahip_slw_workspace: bytes the loss forward and the backward need for (B, c, n, m) (host arithmetic: the larger of the
 *   forward's partial sums, one per row and 4096 positions plus one per sample, and the backward's [B, 32, n] floats); 0 for a
 *   shape outside the coverage.
 * ncahip_slw_project_f32: ks [B, 32, n] and kt [32, m], source and target in one launch, exact fp32 products (fp32 MFMA for c a
 *   multiple of 4, plain fma for c = 3).  source, target and proj 16-byte aligned.
 * ncahip_slw_sort_f32: every row of keys [rows, n] sorted ascending IN PLACE, perm [rows, n] = the original position of each
 *   sorted element.  Pairs are ordered by (key, original position), lowest position first on equal keys -- the order of a stable
 *   sort; -0.0 and +0.0 are equal keys.  Any n in range, a power of two or not.
 * ncahip_slw_loss_fwd_f32: loss [1] from sorted s [B, 32, n], sorted t [32, m] and jmap; partial sums per row in a fixed tree,
 *   combined in index order.
 * ncahip_slw_bwd_f32: dsource [B, c, n] = g_loss[0] * d loss / d source (target and proj get no gradient), in closed form:
 *     dk[b, p, perm[b, p, i]] = 2 g_loss[0] (s[b, p, i] - t[p, jmap[i]]),   dsource[b, c, i] = sum_p proj[c, p] dk[b, p, i];
 *   the residual is recomputed from s and t (nothing is kept by the forward), dk lives in the workspace.  perm must be a permutation
 *   of [0, n) per row (what ncahip_slw_sort_f32 wrote); entries outside [0, n) are skipped. */
size_t ncahip_slw_workspace(int B, int c, int n, int m);
int ncahip_slw_project_f32(const float *source, const float *target, const float *proj, float *ks, float *kt, int B, int c, int n,
                           int m, ncahip_stream_t stream);
int ncahip_slw_sort_f32(float *keys, int32_t *perm, int rows, int n, ncahip_stream_t stream);
int ncahip_slw_loss_fwd_f32(const float *s, const float *t, const int32_t *jmap, float *loss, int B, int n, int m,
                            void *workspace, size_t workspace_bytes, ncahip_stream_t stream);
int ncahip_slw_bwd_f32(const float *s, const float *t, const int32_t *jmap, const int32_t *perm, const float *proj,
                       const float *g_loss, float *dsource, int B, int c, int n, int m, void *workspace, size_t workspace_bytes,
                       ncahip_stream_t stream);

/* The [B,1,H,W] uniforms the kernels draw for (seed, step) when u == NULL (for tests/tools). */
int ncahip_philox_uniform_f32(float *u, int B, int H, int W, uint64_t seed, uint64_t step,
                              ncahip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NCAHIP_H */

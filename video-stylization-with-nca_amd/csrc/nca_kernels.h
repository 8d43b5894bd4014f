// nca_kernels.h -- internal launch interface between the C ABI (nca_capi.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "nca_modes.h"

// ---- per-DEVICE launch state (the C ABI is legal from any host thread on any device: caches are keyed by the device that is
// current at the call, never by the calling thread) -----------------------------------------------------------------------
constexpr int kNcaMaxDevices = 64;
inline int nca_device_index() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kNcaMaxDevices) d = 0;
    return d;
}
// CU count of the current device (cached per device)
inline int nca_cu_count() {
    static std::atomic<int> cus[kNcaMaxDevices];
    const int d = nca_device_index();
    int v = cus[d].load(std::memory_order_relaxed);
    if (v == 0) {
        int q = 0;
        v = 256;
        if (hipDeviceGetAttribute(&q, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && q > 0) v = q;
        cus[d].store(v, std::memory_order_relaxed);
    }
    return v;
}
// hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel instantiation, device): one static instance per launcher template
struct NcaLdsAttr {
    std::atomic<bool> done[kNcaMaxDevices];
    hipError_t ensure(const void* kern, size_t bytes) {
        const int d = nca_device_index();
        if (done[d].load(std::memory_order_acquire)) return hipSuccess;
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) done[d].store(true, std::memory_order_release);
        return e;
    }
};
// Sticky device-side error word of the current device (host-mapped, so the host reads it without synchronising): bit 0 = a
// producer/consumer hand-off poll expired (nca_cond_pc.hip).  nullptr when the allocation failed (errors are then not recorded).
unsigned* nca_error_word_device();        // device-visible pointer for kernel arguments
unsigned nca_error_word_read(bool clear); // host view of the current device's word

struct NcaDyncaArgs {
    const float* x_in;
    float* x_out;
    const float* cond;  // [B,c_cond,H,W] or null
    const float* u;     // [B,1,H,W] or null (Philox)
    const float *w1, *b1, *w2, *b2;
    int B, C, H, W, fc, c_cond, pad_mode;
    float rate;
    uint64_t seed, step;
    // backward variant only (nca_launch_dynca_step_bwd): dL/dx_{t+1} in, recomputed hidden layer / its gradient /
    // dL/dperception out, dL/dx_t out (stencil-adjoint kernel)
    const float* g_next;   // [B,C,H,W]
    float* hbuf;           // relu(w1 y + b1)                [B,fc,H,W]
    float* dhbuf;          // dL/d(pre-activation)           [B,fc,H,W]   (bf16-MFMA backward variants: points at bf16, as ybuf does)
    float* dybuf;          // dL/dy, first 4C rows           [B,4C,H,W]
    float* g_out;          // dL/dx_t                        [B,C,H,W]
    // fc > 128 runs as several launches over 128-wide slices of the hidden layer (nca_launch_dynca_step_fwd):
    int w2_ld;             // row stride of w2 (0: = fc); later slices run the accumulating instantiation (x_out += mask * slice)
    float* gw2_ws;         // backward, fused dW2: per-workgroup partials [grid][C*fc + C] (dW2 | db2); hbuf is then not written
    const float* g_extra;  // backward stencil: optional cotangent of x_t itself, added to g_out (forward_nsteps' middle features)
    const float* pc;       // two-scale perception (perception_scales = [0, 1]): coarse-level perception [B,4C,H/2,W/2], or null
    const float* coarse_add;  // backward stencil, two-scale: dL/dx of the coarse level [B,C,H/2,W/2]; 0.25 * parent is added to g_out
    int dy_half;              // backward stencil, two-scale: the fine level carries 0.5 * dL/dy
    float* ybuf;              // backward MLP kernel: if set, the recomputed perception y (two-scale: the combined one) is written here,
                              // [B,4C,H,W] in perceive_torch's row order -- the B rows of the layer-1 weight-gradient product
    int u_bits;               // u points at bit-packed fire masks (uint32 words, cell i -> bit i & 31 of word i >> 5; B*H*W < 2^32)
    // steered perception (ncahip_dynca_direction; forward variants with fp32 storage only): per-cell directions [Bd,2,H,W], plane 0 = s,
    // plane 1 = c, or null; the Sobel pair of every channel becomes (c Sx - s Sy, s Sx + c Sy) before the first 1x1 product
    const float* dirs;
    size_t dirs_bstride;      // floats between the fields of two samples: 2*H*W, or 0 when one field serves the whole batch (Bd == 1)
};

// T DyNCA steps in one launch (nca_dynca_persist.hip): one workgroup per 16 x 16 tile for all steps, neighbour counters in `flags`
struct NcaDyncaPersistArgs {
    const float* x_in;   // [B,C,H,W] input state (read at step 0 only)
    float* x_out;        // [B,C,H,W] state after T steps (written at the last step only; may alias x_in? no: tiles read neighbours' x_in cells)
    int T;               // 1 <= T < 4096
    const float* cond;   // [B,c_cond,H,W] or null
    const float* u;      // [T][B*H*W] uniforms / [T][ceil(B*H*W/32)] mask words (u_bits) / null: Philox (seed, step0 + t)
    const float *w1, *b1, *w2, *b2;
    int B, C, H, W, fc, c_cond, pad_mode;
    float rate;
    uint64_t seed, step0;
    int* flags;          // [0] = abort word: holds the epoch of a launch that gave up
    unsigned epoch;            // strictly increasing per workspace (1 .. 2^20 - 1): tags of the exchanged pairs are epoch * 4096 + step
    unsigned long long* xch;   // ring exchange: [2 parities][tile][C][60 ring cells] (value, tag) pairs; zero once, never cleared between launches
    size_t xch_words;          // pairs per parity
    unsigned* err;       // sticky error word (bit 1: a neighbour poll expired)
    int u_bits;
    int dbg;             // diagnostic knobs (NCAHIP_PERSIST_DBG, timing experiments only -- results are then NOT valid): bit 0 no neighbour
                         // polls / halo loads, bit 1 no state stores, bit 2 no ring phase, bit 3 no mask refill, bit 4 no MFMA chains.
                         // The single-scale kernel honours all five; the two-scale kernel bits 0, 1 and 4 (1 and 4 sit in shared code)
    const float* dirs;   // steered perception: per-cell directions [Bd,2,H,W] or null, as NcaDyncaArgs::dirs (staged once per launch)
    size_t dirs_bstride; // 2*H*W, or 0 for Bd == 1
};
bool nca_dynca_persist_shape_ok(int B, int C, int H, int W, int fc, int c_cond);
int nca_dynca_persist_tiles(int B, int H, int W);
// (value, tag) pairs per parity of the ring exchange: tiles x C x 60 fine ring cells (+ 48 coarse means: two_scale)
size_t nca_dynca_persist_xch_pairs(int B, int C, int H, int W, bool two_scale);
// query_only: only decide whether every workgroup can be co-resident on the current device (*fits)
// bf16_mfma: ncahip_dynca_precision mode 1 -- instantiations of their own (LDS size, occupancy cache and co-residency test per variant)
hipError_t nca_launch_dynca_persist(const NcaDyncaPersistArgs& a, hipStream_t st, bool query_only, bool* fits, bool bf16_mfma = false);
// two-scale perception (perception_scales = [0, 1]): exchanges 108 pairs per channel and tile (60 fine ring cells + 48 coarse means)
hipError_t nca_launch_dynca_persist_ms(const NcaDyncaPersistArgs& a, hipStream_t st, bool query_only, bool* fits, bool bf16_mfma = false);

// A whole ConditionedNCA grow in one launch (nca_cond_persist.hip): one workgroup per 16 x 16 tile for all T steps + finalize
struct NcaCondPersistArgs {
    const float* x0;          // [B,C,H,W] input state (states slot 0)
    float* states;            // hist: [T+1][B,C,H,W]; slots 1..T (the pending states) are written
    uint8_t* pre;             // hist: [T+1][B,H,W]; slots 1..T are written
    int hist;                 // 1: ring == T + 1 (history for the backward); 0: only x_final
    float* x_final;           // [B,C,H,W] finalized state after T steps
    const float* goal;        // [B,goal_ch,H,W] or null
    const float* u;           // bit-packed fire masks [T][ceil(B*H*W/32)] (u_bits) or null: Philox (seed, step0 + t)
    const float *wp, *w1, *b1, *w2, *b2, *w3;
    int B, C, H, W, goal_ch, alive_ch, T;
    float thr, fire_rate, lo, hi;
    uint64_t seed, step0;
    int* abort_w;             // device word: holds the epoch of a launch that gave up
    unsigned epoch;           // strictly increasing per workspace (1 .. 2^20 - 1): pair tags are epoch * 4096 + step
    unsigned long long* xch;  // [2 parities][tile][C + 1 slots][156 band cells] (value, tag) pairs; zeroed once by the caller
    size_t xch_words;         // pairs per parity
    unsigned* err;            // sticky error word (bit 1: a neighbour poll expired)
    int u_bits;
    uint64_t poll_ticks;      // bound of one neighbour poll in device wall-clock ticks (0: the launcher's default)
    unsigned long long* dbg;  // diagnostic builds (-DNCA_STAMPS) only: per-workgroup wall-clock sums of the step phases
};
bool nca_cond_persist_shape_ok(int B, int C, int H, int W, int hidden, int goal_ch);
int nca_cond_persist_tiles(int B, int H, int W);
size_t nca_cond_persist_xch_pairs(int B, int C, int H, int W);
// query_only: only decide whether every tile gets a CU of its own on the current device (*fits)
hipError_t nca_launch_cond_persist(const NcaCondPersistArgs& a, hipStream_t st, bool query_only, bool* fits);

struct NcaCondArgs {
    const float* x_in;
    const uint8_t* pre_in;  // null: x_in is a true state; else x_in is pending with this pre mask
    float* x_out;
    uint8_t* pre_out;
    const float* goal;  // [B,goal_ch,H,W]
    const float* u;
    const float *wp, *w1, *b1, *w2, *b2, *w3;
    int B, C, H, W, hidden, goal_ch, alive_ch;
    float thr, fire_rate, lo, hi;
    uint64_t seed, step;
    unsigned long long* dbg;  // diagnostic builds (-DNCA_STAMPS) only: per-wave phase time stamps
    unsigned* err;            // sticky error word (nca_error_word_device()), or null
    int u_bits;               // u points at bit-packed fire masks (uint32 words, cell i -> bit i & 31 of word i >> 5; B*H*W < 2^32)
    // this step's fire masks drawn beforehand (nca_cond_fire.hip): one word per 4 x 16 tile, [B][H/4][W/16], or null = the kernel
    // draws them.  Needs u == null, W % 16 == 0, H % 4 == 0; read by the kernels nca_cond_fire_words_ok names, ignored by every
    // other one (which then draws the same masks itself)
    const unsigned long long* fire_words;
    // Several steps of a grow in one launch (nca_cond_pc.hip, the MS kernels; ms_steps == 0: an ordinary one-step launch, nothing
    // below is read).  The launch runs steps ms_t0 .. ms_t0 + ms_steps - 1 of the grow (ms_t0 = steps the grow made before it); step t
    // reads ring slot t % ms_ring and writes slot (t + 1) % ms_ring of ms_states / ms_pre, takes no pre mask at t == 0, and reads
    // fire_words + (t - ms_t0) * (B*H*W / 64).  x_in / pre_in / x_out / pre_out describe the launch's first step as for a one-step launch.
    // ms_done: one counter per 4 x 16 tile, [B][H/4][W/16] = steps of this grow completed for the tile (zero before the grow's first
    // step), and behind them, at ms_done[B * H/4 * W/16], the abort word (zero likewise): set by a gate whose poll expired
    int ms_steps, ms_t0, ms_ring;
    char* ms_states;
    uint8_t* ms_pre;
    unsigned* ms_done;
};
// the fused-steps launch (several steps of a grow per launch) exists for `a`: narrow carve, the kernels that read fire words, at least
// two rounds per workgroup, not switched off (nca_modes.h pc_no_fused_steps)
bool nca_cond_pc_fused_steps_ok(const NcaCondArgs& a);
hipError_t nca_launch_cond_steps_fwd_pc(const NcaCondArgs& a, hipStream_t st);   // hipErrorInvalidValue where the question above says no
// bytes of ms_done (counters + abort word, padded to 64) for a grid
inline size_t nca_cond_ms_done_bytes(int B, int H, int W) { return (((size_t)B * (H / 4) * (W / 16) + 1) * 4 + 63) & ~(size_t)63; }
// the launch nca_launch_cond_step_fwd makes for `a` runs a kernel that reads a.fire_words (shape, alignment -- of a.fire_words too: 8 bytes --, test hooks)
bool nca_cond_fire_words_ok(const NcaCondArgs& a);
bool nca_cond_pc_fire_words_ok(const NcaCondArgs& a);   // the same question inside the producer/consumer family (nca_cond_pc.hip)
// fire words of steps step0 .. step0 + Tc - 1, [Tc][B][H/4][W/16] (nca_cond_fire.hip)
// done_zero: null, or the fused-steps path's per-tile step counters and abort word (NcaCondArgs::ms_done), which the launch zeroes too
hipError_t nca_launch_cond_fire_words(unsigned long long* words, int Tc, int B, int H, int W, float fire_rate, uint64_t seed, uint64_t step0,
                                      hipStream_t st, unsigned* done_zero = nullptr);

// One backward step of the ConditionedNCA grow loop (nca_cond_bwd.hip).  f describes forward step t exactly as
// it was launched (x_in = states[t], pre_in = pre[t] or null for t == 0, goal, u / seed+step, weights).
struct NcaCondBwdArgs {
    NcaCondArgs f;
    const float* x_next;    // states[t+1] = pending x'_t                      [B,C,H,W]
    const uint8_t* pre_t;   // pre[t+1]    = alive(s_t)                        [B,H,W]
    const float* g_next;    // dL/d s_{t+1}                                    [B,C,H,W]
    float* g_out;           // dL/d s_t  (written by the stencil kernel)        [B,C,H,W]
    float* gx;              // scratch: direct-path gradient dL/dx'_t           [B,C,H,W]
    float* dP;              // scratch: dL/d perception                         [B,3C,H,W]
    float* zbuf;            // scratch: z_t = s_t + goal*pre_t                  [B,C,H,W]
    float* dgoal;           // accumulated over steps                           [B,goal_ch,H,W]
    float* slabs;           // per-workgroup weight-gradient partials, accumulated   [nslab, nca_cond_bwd_slab_floats] (tile-major: SlabTM)
    float* wp_partials;     // per-block perception-weight partials             [nblk, 27] accumulated
    int nslab, nblk;
    int srows;              // rows per strip of the stencil-adjoint kernel (set by its launcher: nca_cond_bwd_srows)
    float* opimg;           // matrix kernel: its LDS operand image kept in memory across the steps of one backward pass (workspace), see opmode
    int opmode;             // 0 = every launch gathers the image from the weight tensors; 1 = ONE workgroup builds it and writes it to opimg
                            // (no tile work); 2 = the launch copies it from opimg (16-byte loads instead of ~100 scattered 4-byte gathers per thread)
    int msplit;             // matrix kernel: 1 = a workgroup takes ONE pass (half the rows) of a super-tile per walk item (small grids: twice the workgroups)
    void* pscr;             // front/matrix form: perception vectors in MFMA-operand order  (nca_cond_bwd_fm_pscr_bytes)
    void* doscr;            // front/matrix form: dL/dx'_t * fire mask, [row tile][channel][cell] (nca_cond_bwd_fm_doscr_bytes)
};
int nca_cond_bwd_slab_floats(int C, int hidden);
hipError_t nca_launch_cond_bwd_unpermute(const float* red, int C, int hidden, bool bf16_history, float* g_w1, float* g_w2, float* g_w3,
                                         float* g_b1, float* g_b2, hipStream_t st);
int nca_cond_bwd_nslab();
int nca_cond_bwd_nblk(int B, int C, int H, int W);
bool nca_cond_bwd_is_fm(const NcaCondBwdArgs& ba, bool bf16);   // the form nca_launch_cond_step_bwd will run for these arguments
constexpr size_t kNcaCondBwdOpimgBytes = 128 * 1024;            // upper bound of the matrix kernel's operand image (CP = 32: 100 KB)
hipError_t nca_launch_cond_step_bwd(const NcaCondBwdArgs& a, hipStream_t st, bool bf16 = false);   // bf16: f.x_in / x_next / f.goal hold bf16
// kernel A as two launches (nca_cond_bwd_fm.hip); mode 0 = f32 history, 1 = bf16 history / exact-f32 products, 2 = bf16 MFMA
hipError_t nca_launch_cond_step_bwd_fm(const NcaCondBwdArgs& a, hipStream_t st, int mode);
size_t nca_cond_bwd_fm_pscr_bytes(int B, int C, int H, int W);
size_t nca_cond_bwd_fm_doscr_bytes(int B, int C, int H, int W);
hipError_t nca_launch_reduce_rows(const float* src, float* dst, int n, int m, hipStream_t st, bool accumulate = false);   // dst (+)= column sums
// nca_gram.hip: out[ma*nb + ma] = [sum_n a[i][n] * b[j][n] | sum_n a[i][n]] over all B*HW cells; b rows from two tensors
int nca_dynca_bwd_grid(int B, int H, int W);   // upper bound over C (workspace sizing)
int nca_dynca_bwd_grid_c(int B, int C, int H, int W);   // the grid the backward kernel actually runs with = number of slabs it writes   // workgroups of the DyNCA backward kernel (= partial slabs of its fused dW2)
int nca_gram_grid(int B, int HW);
hipError_t nca_launch_gram_rows(const float* a, int ma, const float* b1, int nb1, const float* b2, int nb2, int B, int HW,
                                float* out, float* ws, hipStream_t st, bool accumulate = false);
// nca_gram_bf16.hip: the same product over bf16 operands (a, b1: bf16; b2: fp32, rounded as loaded); ma <= 128, nb1 + nb2 <= 79
int nca_gram_bf16_grid(int B, int HW);
// the two ranges of that product (rows ma x columns nb = nb1 + nb2): this launcher's, and nca_launch_gram_rows_bf16_wide's below
struct NcaGramBfRange { int ma, nb; };
constexpr NcaGramBfRange kNcaGramBf{128, 79}, kNcaGramBfWide{256, 132};
inline bool nca_gram_bf16_fits(const NcaGramBfRange& r, int ma, int nb) { return ma <= r.ma && nb <= r.nb; }
hipError_t nca_launch_gram_rows_bf16(const uint16_t* a, int ma, const uint16_t* b1, int nb1, const float* b2, int nb2, int B, int HW,
                                     float* out, float* ws, hipStream_t st, bool accumulate = false);
// nca_dynca_bwd_bf16.hip: MLP part of one backward step in the bf16-MFMA training mode (ybuf / dhbuf point at bf16 buffers)
hipError_t nca_launch_dynca_step_bwd_mlp_bf16(const NcaDyncaArgs& a, hipStream_t st);
// nca_dynca_bwd_bf16_wide.hip: the same in the wide range (C <= 32, fc <= 256, outside the narrow one; single-scale): one launch per 128-wide
// slice at the forward's channel class; dhbuf [B,fc,H,W] and the gw2_ws slabs [C*fc + C] have the whole layer's layout
hipError_t nca_launch_dynca_step_bwd_mlp_bf16_wide(const NcaDyncaArgs& a, hipStream_t st);
// nca_gram_bf16.hip: nca_launch_gram_rows_bf16 up to ma <= 256, nb1 + nb2 <= 132 (inside the old range: that launcher itself)
hipError_t nca_launch_gram_rows_bf16_wide(const uint16_t* a, int ma, const uint16_t* b1, int nb1, const float* b2, int nb2, int B, int HW,
                                          float* out, float* ws, hipStream_t st, bool accumulate = false);
hipError_t nca_launch_reduce_wp(const float* part, float* dst, int B, int C, int H, int W, hipStream_t st);
// nca_ot.hip: relaxed-EMD part of the OT appearance loss (gather / normalise, N x N cosine distances reduced in registers, adjoints)
int nca_ot_bands(int N);   // column-minimum partials per column (one per 32-row band)
hipError_t nca_launch_ot_gather(const float* t, const float* g, const int* idx, float* x, float* y, float* xn, float* yn, int B, int c,
                                int HW, int N, hipStream_t st);
hipError_t nca_launch_ot_scatter(const float* dy, const int* idx, float* dg, int B, int c, int HW, int N, hipStream_t st);
hipError_t nca_launch_ot_remd_fwd(const float* x, const float* y, const float* xn, const float* yn, float* rmin, int* rarg, float* cmin,
                                  int* carg, float* remd, int* branch, int B, int N, int c, void* ws, hipStream_t st);
hipError_t nca_launch_ot_remd_bwd(const float* x, const float* y, const float* xn, const float* yn, const int* rarg, const int* carg,
                                  const int* branch, const float* gup, float* dy, int B, int N, int c, hipStream_t st);
// nca_ot_moment.hip: moment-matching part of the OT appearance loss (means, covariance difference reduced to signs + partial sums, adjoint)
int nca_ot_moment_tiles(int c);   // 64-channel tiles; the covariance kernel writes one partial per pair ti <= tj
hipError_t nca_launch_ot_moment_fwd(const float* x, const float* y, float* mom, float* my, float* sgn, signed char* S, int B, int N, int c,
                                    void* ws, hipStream_t st);
hipError_t nca_launch_ot_moment_bwd(const float* y, const float* my, const float* sgn, const signed char* S, const float* gup, float* dy, int B,
                                    int N, int c, hipStream_t st);
// nca_ot_sample.hip: the OT loss's position sampler (keyed Philox draws, radix select of the n smallest, ordered compaction); one
// workgroup per row, idx [rows, n]
hipError_t nca_launch_ot_sample(int* idx, int rows, int HW, int n, uint64_t seed, uint64_t row0, int key_bits, hipStream_t st);
// nca_slw.hip: sliced-Wasserstein style loss (projection onto 32 directions, segmented stable sort of (key, index) pairs, loss, adjoint)
int nca_slw_blocks(int n);   // 4096-position blocks of a row: sort chunks, and loss partials per row
hipError_t nca_launch_slw_project(const float* src, const float* tgt, const float* proj, float* ks, float* kt, int B, int c, int n, int m,
                                  hipStream_t st);
hipError_t nca_launch_slw_sort(float* keys, int* perm, int rows, int n, hipStream_t st);
hipError_t nca_launch_slw_loss_fwd(const float* s, const float* t, const int* jmap, float* loss, int B, int n, int m, void* ws, hipStream_t st);
hipError_t nca_launch_slw_bwd(const float* s, const float* t, const int* jmap, const int* perm, const float* proj, const float* gup, float* ds, int B,
                              int c, int n, int m, void* ws, hipStream_t st);
// nca_clip.hip: the two ends of clip stylisation.  frames: N = F*B images, float32 [N,3,H,W] or (u8) uint8 [N,H,W,3] -> cond [N,3,H,W];
// state [B,C,H,W] -> image float32 [B,c_out,H,W] or (u8) uint8 [B,H,W,c_out], c_out in 1..4; frames -> grey [N,H,W]
hipError_t nca_launch_clip_cond(const void* frames, bool u8, const float* k3, float wr, float wg, float wb, int do_tanh, float* cond, int N, int H,
                                int W, hipStream_t st);
hipError_t nca_launch_clip_gray(const void* frames, bool u8, float wr, float wg, float wb, float* gray, int N, int H, int W, hipStream_t st);
// The image a clip call writes: float32 [B,c,H,W], uint8 [B,H,W,c], or planar YUV 4:2:0 uint8 [B,3H/2,W] (H and W even) with the ten
// words of nca_rgb_yuv_build_coeffs (zero for the other kinds).  nca_img_out (nca_yuv_out.hip, host) builds it from an img_fmt of
// include/ncahip.h -- NCAHIP_CLIP_F32_NCHW, NCAHIP_CLIP_U8_NHWC, NCAHIP_CLIP_YUV420(layout, matrix, range) -- and is the one place that
// knows that word's layout; false: no such format
enum NcaImgKind { kImgF32 = 0, kImgU8 = 1, kImgI420 = 2, kImgNV12 = 3 };
struct NcaImgOut {
    NcaImgKind kind;
    int32_t k[10];
    bool planar() const { return kind >= kImgI420; }
};
bool nca_img_out(int img_fmt, NcaImgOut* out);
// One launch: the image of state[:, :c_out] (img != nullptr) and the plane gray [B,H,W] over state[:, C-1] (gray != nullptr, c_out <=
// C-1); the state is only read without a grey plane.  unit: ConditionedNCA's image clamp(state[:, :3], 0, 1) (C >= 3, c_out == 3, no
// grey), also from a state stored as bf16 (bf16: unit only) -- bit for bit the image of the widened state.  A planar image has c_out ==
// 3 and is bit for bit the uint8 image followed by nca_launch_clip_rgb_to_yuv420.  hipErrorInvalidValue outside that.
struct NcaClipEmitArgs {
    void* state;        // [B,C,H,W] float32, or bf16
    bool bf16;
    void* img;          // nullptr: the grey plane only
    NcaImgOut out;
    bool unit;
    const float* gray;
    int B, C, c_out, H, W;
};
hipError_t nca_launch_clip_emit(const NcaClipEmitArgs& a, hipStream_t st);
// nca_encoder.hip: ImageEncoder.forward of N = F*B frames in one launch: float32 [N,ch,H,W] (ch <= 4) or (u8) uint8 [N,H,W,3] -> goal [N,E,H,W],
// E <= 32; w1 [E,3+ch,3,3], b1 [E], w2 [E,E,3,3]; hipErrorInvalidValue outside that range
hipError_t nca_launch_clip_encode(const void* frames, bool u8, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2,
                                  float* goal, int N, int ch, int E, int H, int W, hipStream_t st);
// the same kernel and arithmetic with the goal rounded to bf16 (RNE) on the final store: nca_launch_clip_encode, then a cast
hipError_t nca_launch_clip_encode_bf16(const void* frames, bool u8, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2,
                                       uint16_t* goal, int N, int ch, int E, int H, int W, hipStream_t st);

// nca_resize.hip: crop + Pillow-exact 8-bit resize of N uint8 frames [N,H,W,3] -> [N,out_h,out_w,3]: horizontal pass into tmp
// [N,ch,out_w,3], vertical pass into dst.  kx [out_w,ksize_x] / bx [out_w,2] and ky [out_h,ksize_y] / by [out_h,2]: device tables as
// nca_resize_build_tables fills them for (cw -> out_w) and (ch -> out_h)
hipError_t nca_launch_clip_resize(const unsigned char* src, int N, int H, int W, int x0, int y0, int cw, int ch, const int* kx, const int* bx,
                                  int ksize_x, const int* ky, const int* by, int ksize_y, unsigned char* dst, int out_h, int out_w,
                                  unsigned char* tmp, hipStream_t st);
// the same with planar YUV 4:2:0 frames [N,3H/2,W] (I420, or NV12), H and W even: the horizontal pass's loader converts with the six
// coefficient words k (HOST memory, nca_yuv_build_coeffs); the result is nca_launch_clip_yuv420_to_rgb on the crop, then the resize
hipError_t nca_launch_clip_resize_yuv420(const unsigned char* src, bool nv12, const int* k, int N, int H, int W, int x0, int y0, int cw, int ch,
                                         const int* kx, const int* bx, int ksize_x, const int* ky, const int* by, int ksize_y, unsigned char* dst,
                                         int out_h, int out_w, unsigned char* tmp, hipStream_t st);
// nca_launch_clip_resize with planar YUV 4:2:0 IMAGES: dst [N,3 out_h/2,out_w] (I420, or NV12), out_h and out_w even.  The same
// horizontal pass, then a vertical pass that writes the planes with the ten coefficient words k (HOST memory, nca_rgb_yuv_build_coeffs);
// the result is nca_launch_clip_resize, then nca_launch_clip_rgb_to_yuv420
hipError_t nca_launch_clip_resize_u8_yuv420(const unsigned char* src, int N, int H, int W, int x0, int y0, int cw, int ch, const int* kx,
                                            const int* bx, int ksize_x, const int* ky, const int* by, int ksize_y, bool nv12, const int* k,
                                            unsigned char* dst, int out_h, int out_w, unsigned char* tmp, hipStream_t st);
// nca_yuv.hip: the crop (x0, y0, cw, ch) of N planar YUV 4:2:0 frames [N,3H/2,W] -> RGB [N,ch,cw,3] uint8, one launch; any alignment
hipError_t nca_launch_clip_yuv420_to_rgb(const unsigned char* src, bool nv12, int N, int H, int W, int x0, int y0, int cw, int ch, const int* k,
                                         unsigned char* dst, hipStream_t st);
// host only: the coefficients (k_y, k_rv, k_gu, k_gv, k_bu, luma offset) of matrix 0 = BT.601 / 1 = BT.709, range 0 = limited / 1 = full
void nca_yuv_build_coeffs(int matrix, int range, int32_t k[6]);
// nca_yuv_out.hip: N RGB24 images [N,H,W,3] -> planar YUV 4:2:0 [N,3H/2,W] (H, W even), one launch; any alignment.  k: the ten words of
// nca_rgb_yuv_build_coeffs in HOST memory
hipError_t nca_launch_clip_rgb_to_yuv420(const unsigned char* src, bool nv12, int N, int H, int W, const int* k, unsigned char* dst, hipStream_t st);
void nca_rgb_yuv_build_coeffs(int matrix, int range, int32_t k[10]);
// host only (no GPU call): table row width (-1: does not fit an int), and the tables of one axis; filter 0 = bicubic, 1 = Lanczos.  The
// builder returns 0, or the 1-based row that breaks an integer bound of the passes
int nca_resize_ksize(int in, int out, int filter);
int nca_resize_build_tables(int in, int out, int filter, int32_t* k, int32_t* bounds, int ksize);

// fused steps (nca_dynca_fwd.hip, nca_dynca_bwd.hip, nca_cond_generic.hip); hipErrorInvalidValue when no instantiation covers the shape
// bf16_mfma: ncahip_dynca_precision mode 1 (both 1x1 products on bf16 MFMA, nca_dynca_bf16.h) where nca_dynca_bf16_shape_ok
// bf16_wide: with bf16_mfma, ncahip_dynca_bf16_range 1 -- a single-scale unsteered step outside the narrow range and inside
// nca_dynca_bf16_wide_shape_ok runs nca_launch_dynca_step_fwd_bf16_wide; every other call is what it is without the flag
hipError_t nca_launch_dynca_step_fwd(const NcaDyncaArgs& a, hipStream_t st, bool bf16_mfma = false, bool bf16_wide = false);
// the bf16-MFMA forward at the wide shape classes <32, 128>, <16, 256>, <32, 256> (nca_dynca_bf16_wide.hip): the whole hidden layer in one
// launch; single-scale, unsteered, a shape inside the wide and outside the narrow range (anything else: hipErrorInvalidValue)
hipError_t nca_launch_dynca_step_fwd_bf16_wide(const NcaDyncaArgs& a, hipStream_t st);
inline bool nca_dynca_bf16_wide_shape_ok(int C, int fc) { return C >= 1 && C <= 32 && fc >= 1 && fc <= 256; }
// the same ladder over the steered variants (nca_dynca_steer.hip); a.dirs must be set.  nca_launch_dynca_step_fwd goes there itself
hipError_t nca_launch_dynca_step_fwd_steered(const NcaDyncaArgs& a, hipStream_t st, bool bf16_mfma);
inline bool nca_dynca_bf16_shape_ok(int C, int fc) { return C >= 1 && C <= 16 && fc >= 1 && fc <= 128; }
hipError_t nca_launch_cond_step_fwd(const NcaCondArgs& a, hipStream_t st);
hipError_t nca_launch_dynca_step_bwd(const NcaDyncaArgs& a, hipStream_t st);
hipError_t nca_launch_dynca_step_bwd_mlp(const NcaDyncaArgs& a, hipStream_t st, bool acc);      // MLP part only (hidden-layer slices)
hipError_t nca_launch_dynca_step_bwd_stencil(const NcaDyncaArgs& a, hipStream_t st);            // stencil adjoint + residual
hipError_t nca_launch_dynca_step_fwd_bf16(const NcaDyncaArgs& a, hipStream_t st);   // x_in / x_out hold bf16
// wave-private-tile variant (nca_cond_wave.hip); needs W % 4 == 0 and 16-byte aligned x_in / goal
hipError_t nca_launch_cond_step_fwd_wave(const NcaCondArgs& a, hipStream_t st);
// producer/consumer wave-specialised variant (nca_cond_pc.hip); same preconditions
hipError_t nca_launch_cond_step_fwd_pc(const NcaCondArgs& a, hipStream_t st);
// bf16 state storage + bf16 MFMA (nca_cond_bf16.hip): x_in / x_out / goal point at bf16 data
hipError_t nca_launch_cond_step_fwd_bf16(const NcaCondArgs& a, hipStream_t st);
hipError_t nca_launch_cond_finalize_bf16(const uint16_t* x, const uint8_t* pre, uint16_t* out, int B, int C, int H, int W,
                                         int alive_ch, float thr, float lo, float hi, hipStream_t st);
// the finalize above and the unit image of its result in ONE launch (C >= 3; a planar image: H and W even)
hipError_t nca_launch_cond_finalize_emit_bf16(const uint16_t* x, const uint8_t* pre, uint16_t* out, void* img, const NcaImgOut& io, int B, int C, int H,
                                              int W, int alive_ch, float thr, float lo, float hi, hipStream_t st);

// diagnostic build hook (-DNCA_STAMPS): buffer that receives s_memtime stamps, [wave][tile][8]
void nca_debug_set_stamp_buffer(unsigned long long* p);

// stencils and small kernels (nca_stencil.hip)
hipError_t nca_launch_dynca_perceive(const float* x, float* y, int B, int C, int H, int W, int pad, hipStream_t st);
hipError_t nca_launch_image_encoder_front(const float* img, const float* k3, const float* k5, float* feat, int B, int ch, int H, int W,
                                          hipStream_t st);
hipError_t nca_launch_edge_extractor(const float* img, const float* k3, float* out, int B, int H, int W, int do_tanh, hipStream_t st);
hipError_t nca_launch_widen_bf16(const uint16_t* in, float* out, size_t n, hipStream_t st);
hipError_t nca_launch_dynca_ms_combine(float* y, const float* pc, int B, int C, int H, int W, hipStream_t st);   // y <- (y + up2(pc)) / 2
hipError_t nca_launch_dynca_ms_upT(const float* dy, float* dpc, int B, int C, int H, int W, hipStream_t st);    // dpc = 0.5 * up2^T(dy)
int nca_dynca_bwd_ms_grid(int B, int H, int W);
hipError_t nca_launch_dynca_coarse_perceive(const float* x, float* pc, int B, int C, int H, int W, int pad, hipStream_t st);
hipError_t nca_launch_cond_perceive(const float* z, const float* wp, float* y, int B, int C, int H, int W, hipStream_t st);
hipError_t nca_launch_cond_finalize(const float* x, const uint8_t* pre, float* out, int B, int C, int H, int W,
                                    int alive_ch, float thr, float lo, float hi, hipStream_t st);
hipError_t nca_launch_cond_alive(const float* x, uint8_t* out, int B, int C, int H, int W, int alive_ch, float thr,
                                 hipStream_t st);
hipError_t nca_launch_philox_uniform(float* u, int B, int H, int W, uint64_t seed, uint64_t step, hipStream_t st);
// fire masks of T steps, bit-packed: mode 0 = clamp(u,0,1) < rate (nca.py:171-174), 1 = floorf(u + rate) >= 1 (dynca.py:131)
hipError_t nca_launch_pack_fire_mask(const float* u, uint32_t* bits, int T, size_t cells, float rate, int mode, hipStream_t st);
hipError_t nca_launch_selftest(int* result, hipStream_t st);
hipError_t nca_launch_zero_words(uint32_t* p, size_t n, hipStream_t st);   // n 32-bit words of zeros from a kernel (nca_zero_async in nca_capi.hip)

// nca_dynca_step.h -- the fused DyNCA step kernel for MI355X (gfx950), fp32 exact: kernel template, its twelve named variants, the
// one launcher and the one dispatch ladder.  nca_dynca_fwd.hip instantiates the forward variants, nca_dynca_bwd.hip the backward
// ones, nca_dynca_steer.hip (a unit of its own) the steered forward variants DyncaSteered<V>, nca_dynca_bwd_bf16.hip (a unit of its
// own) the two bf16-MFMA backward variants, nca_dynca_bf16_wide.hip (a unit of its own) DyncaFwdBf at the three wide shape classes
// <32, 128>, <16, 256> and <32, 256> (its own small ladder), nca_dynca_bwd_bf16_wide.hip (a unit of its own) the sliced bf16-MFMA backward
// variants of those classes.  The generic ConditionedNCA step (nca_cond_generic.hip) has the same structure.
//
// One persistent launch per NCA step.  A workgroup (4 waves) owns TH x TW cell tiles:
//   1. the state tile (+1 halo, pad mode resolved at load time; ConditionedNCA: the pending
//      life mask of the previous step is resolved on an alpha halo of 3) is staged in LDS.
//      Every global load of a tile is issued up front (16-byte row loads, one position per
//      thread, channels in a register loop) so a tile exposes ONE memory latency, and the
//      loads are issued before the barrier that retires the previous tile;
//   2. each wave takes 4 groups of 16 W-contiguous cells; lane l = 16*g + i computes the
//      3x3 depthwise perception of channels {4c'+g} for cell i from LDS (the perception value
//      IS the MFMA B operand: B[k = g][col = i]);
//   3. the per-cell MLP runs on v_mfma_f32_16x16x4_f32 (exact f32 == fmaf chain) with cells on
//      the N/lane axis and channels on M/K: D = W * X.  A layer's accumulator tile
//      (rows 4g+r in reg r, guide sec.3) is the next layer's B operand without any lane
//      movement when that layer's k order is permuted to k(s,g) = 16*(s/4) + 4g + s%4 -- the
//      permutation is folded into the LDS weight image, built once per workgroup;
//   4. residual add + fire mask, stores straight from the accumulator layout.
// Weights live in LDS as the A-operand image [m-tile][k-step][lane]; hidden activations never
// leave registers.  Layer 1 is streamed m-tile by m-tile into layer 2's accumulators so only
// one layer-1 tile is live (keeps 2 waves/SIMD).
#pragma once
#include <type_traits>

#include "nca_step_tile.h"

namespace {

// =========================================================================================
// DyNCA step (ConditioneDyNCA/models/dynca.py:117-138)
// =========================================================================================
// BF: the bf16-MFMA forward UpdateNet (ncahip_dynca_precision mode 1): only the two weight images differ (nca_dynca_bf16.h)
template <int CP, int FC, bool HAS_COND, int TH, int TW, int NT, bool BF = false>
struct DyncaCfg {
    static constexpr int K1S = CP + (HAS_COND ? 1 : 0);  // k-steps of layer 1 (4 inputs each)
    static constexpr int M1T = FC / 16;                  // 16-row output tiles of layer 1
    static constexpr int K2S = FC / 4;
    static constexpr int M2T = (CP + 15) / 16;
    static constexpr int ROWS = TH + 2, RS = TW + 8;
    static constexpr int CS = lds_cs(ROWS, RS);
    static constexpr int TWN = TW / 16;
    static constexpr int NTILES16 = TH * TW / 16;
    static constexpr int ITERS = NTILES16 / (4 * NT);
    static constexpr int CPH = CP / 2;
    // LDS carve (floats)
    static constexpr int OFF_W1 = 0;
    static constexpr int W1_FLOATS = BF ? M1T * ((K1S + 7) / 8) * 256 : M1T * K1S * 64;    // bf16 images: eight k values per 16-byte entry
    static constexpr int W2_FLOATS = BF ? M2T * (FC / 32) * 256 : M2T * K2S * 64;
    static constexpr int OFF_W2 = OFF_W1 + W1_FLOATS;
    static constexpr int OFF_B1 = OFF_W2 + W2_FLOATS;
    static constexpr int OFF_B2 = OFF_B1 + FC;
    static constexpr int OFF_Z = OFF_B2 + M2T * 16;
    static constexpr int OFF_MK = OFF_Z + CP * CS;
    static constexpr int OFF_CN = OFF_MK + TH * TW;
    static constexpr int LDS_FLOATS = OFF_CN + (HAS_COND ? 4 * TH * TW : 0);
    // two-scale perception: coarse-level perception tile [4*CP planes][TH/2 + 2 rows][PCR], halo 1 (index-clamped: bilinear)
    static constexpr int PCR = TW / 2 + 4, PCS = (TH / 2 + 2) * PCR;
    static constexpr int OFF_PC = LDS_FLOATS;
    static constexpr int LDS_FLOATS_MS = OFF_PC + 4 * CP * PCS;
    // steered variants: the tile's directions [2][TH * TW] (s | c) go BEHIND the variant's carve (forward: LDS_FLOATS, two-scale:
    // LDS_FLOATS_MS); the unsteered variants ask for the LDS they always did
    static constexpr int DR_FLOATS = 2 * TH * TW;
    // backward variant: the transposed operands (W2^T for dh, W1^T for dL/dy) are 16-byte reads of the FORWARD images (see the
    // kernel), so the backward needs no weight images of its own.  dL/dy is produced in tiles of 16 rows = 4 channels x 4
    // filters (row i <-> channel 4mj + (i & 3), filter i >> 2): MJ = CP / 4 tiles, no conditioning rows (dynca.py:123).
    static constexpr int MJ = CP / 4;
    static constexpr int LDS_FLOATS_BWD = OFF_CN;                     // the backward reads the conditioning straight from memory (no CN tile)
    // transposition tiles [16 cells][TBS] (16-byte rows).  bf16-MFMA backward: unpadded -- lane (g, ci) writes 16 bytes at 16 ci + 4g and
    // reads word 64 s + 16 g + ci, both conflict-free, and the 2 KB saved are what lets <16, 128> with conditioning keep two workgroups per CU
    static constexpr int TBS = BF ? 16 : (M2T == 1 ? 20 : 36);
    static constexpr int OFF_TB = LDS_FLOATS_BWD;                     // fused dW2: per wave NT tiles
    static constexpr int LDS_FLOATS_BWD_W2 = OFF_TB + 4 * NT * 16 * TBS;
    static_assert(FC % 16 == 0 && CP % 4 == 0 && TW % 16 == 0, "shape");
    static_assert(NTILES16 % (4 * NT) == 0, "tile must split evenly over 4 waves x NT");
    static_assert(OFF_Z % 4 == 0 && CS % 4 == 0 && TH * TW == kThreads, "16-byte carve; one cell per thread");
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
};

// ---- the twelve variants of the step kernel: each names one combination of the six switches the kernel body reads -------------
//   BWD  the backward data path of the step instead of the forward MLP (see the kernel)
//   B16  bf16 state storage: x_in / x_out hold bf16, exact f32 compute, round-to-nearest-even on store
//   ACC  a later 128-wide slice of a wide hidden layer: adds to what the earlier launches wrote
//   W2F  backward with the layer-2 weight gradient fused in (per-workgroup dW2 | db2 partials, h is not written)
//   MS   two-scale perception: the coarse-level perception tile is staged in LDS and blended in
//   BF   both 1x1 products of the forward on bf16 MFMA (ncahip_dynca_precision mode 1); with BWD: every product of the backward on bf16
//        MFMA, y and dh written as bf16 through ybuf / dhbuf (the "bf16-MFMA training" mode of include/ncahip.h)
//   STEER the perception's Sobel pair rotated by the cell's direction (NcaDyncaArgs::dirs, ncahip_dynca_direction): DyncaSteered<V> of a
//        forward variant V with fp32 storage.  A switch and not a launch-uniform branch on the pointer: with the branch the unsteered
//        kernels took up to 60 more registers, and the bf16-MFMA and one-launch kernels spilled ("Steered perception")
//   SL   bf16-MFMA backward of the wide range (nca_dynca_bwd_bf16_wide.hip): the launch takes one 128-wide SLICE of the hidden layer at
//        the forward's channel class (one or two 16-channel tiles).  w2, dh_out and the dW2 slabs keep the row stride of the FULL layer
//        (NcaDyncaArgs::w2_ld), the caller offsets the pointers; with ACC the launch adds to the dL/dy of the earlier slices and leaves
//        y_out and db2 to the first
struct DyncaVariant { static constexpr bool BWD = false, B16 = false, ACC = false, W2F = false, MS = false, BF = false, STEER = false, SL = false; };
template <class V>
struct DyncaSteered : V { static constexpr bool STEER = true; };   // V steered: nca_dynca_steer.hip instantiates these
struct DyncaFwd : DyncaVariant {};                                                                  // forward, exact fp32
struct DyncaFwdBf : DyncaVariant { static constexpr bool BF = true; };                              // forward, bf16 MFMA
struct DyncaFwdMs : DyncaVariant { static constexpr bool MS = true; };                              // forward, two-scale
struct DyncaFwdMsBf : DyncaVariant { static constexpr bool MS = true, BF = true; };                 // forward, two-scale, bf16 MFMA
struct DyncaFwdAcc : DyncaVariant { static constexpr bool ACC = true; };                            // forward, accumulating slice
struct DyncaFwdB16 : DyncaVariant { static constexpr bool B16 = true; };                            // forward, bf16 storage
struct DyncaBwd : DyncaVariant { static constexpr bool BWD = true; };                               // backward, unfused: writes h for a library GEMM
struct DyncaBwdW2 : DyncaVariant { static constexpr bool BWD = true, W2F = true; };                 // backward, fused dW2
struct DyncaBwdW2Ms : DyncaVariant { static constexpr bool BWD = true, W2F = true, MS = true; };    // backward, fused dW2, two-scale
struct DyncaBwdW2Acc : DyncaVariant { static constexpr bool BWD = true, W2F = true, ACC = true; };  // backward, fused dW2, accumulating slice
// BWD and BF together: the "bf16-MFMA training" backward (include/ncahip.h): every product on bf16 MFMA, y and dh written as bf16.
// nca_dynca_bwd_bf16.hip (a unit of its own) instantiates these two.
struct DyncaBwdBf : DyncaVariant { static constexpr bool BWD = true, W2F = true, BF = true; };                  // backward, fused dW2, bf16 MFMA
struct DyncaBwdBfMs : DyncaVariant { static constexpr bool BWD = true, W2F = true, MS = true, BF = true; };    // the same, two-scale
// the wide range of that mode (nca_dynca_bwd_bf16_wide.hip): one launch per 128-wide slice, the first and the later ones
struct DyncaBwdBfSl : DyncaVariant { static constexpr bool BWD = true, W2F = true, BF = true, SL = true; };
struct DyncaBwdBfSlAcc : DyncaVariant { static constexpr bool BWD = true, W2F = true, BF = true, SL = true, ACC = true; };

// BWD = true: the backward data path of the same step (autograd through dynca.py:117-138).  Recomputes the
// hidden layer, then dh = (W2^T (G*mask)) * 1[h>0] and dL/dy = W1^T dh on MFMA (accumulator tile == next B
// operand, as in the forward); writes relu(h), dh and dL/dy[:4C].  The two weight-gradient GEMMs
// (dW2 = (G*mask) h^T, dW1 = dh y^T, K = all cells) are plain library GEMMs on those buffers.
template <int CP, int FC, bool HAS_COND, int TH, int TW, int NT, bool VEC, typename V>
__global__ __launch_bounds__(kThreads, (CP > 16 || V::MS || (V::BF && FC > 128)) ? 1 : 2) void dynca_step_fwd_kernel(const NcaDyncaArgs a) {   // CP > 16: 140 KB of LDS -> one workgroup per CU anyway: 512 registers (bf16 MFMA at FC = 256: 85 KB, the same)
    constexpr bool BWD = V::BWD, B16 = V::B16, ACC = V::ACC, W2F = V::W2F, MS = V::MS, BF = V::BF, STEER = V::STEER, SL = V::SL;
    // the wide range of the bf16-MFMA forward (ncahip_dynca_bf16_range 1; nca_dynca_bf16_wide.hip): two output tiles and / or FC = 256
    constexpr bool BFW = BF && (CP > 16 || FC > 128);
    static_assert(!STEER || (!BWD && !B16), "steered: the forward variants with fp32 storage");
    static_assert(!MS || (TH % 2 == 0 && TW % 2 == 0), "the two-scale step: a tile covers whole coarse cells");
    static_assert(!BFW || (BWD ? SL : (!MS && !STEER && !ACC && !B16)), "bf16 MFMA, wide range: the plain forward, and the sliced backward");
    static_assert(!SL || (BWD && BF && W2F && !MS && FC == 128), "slices: the single-scale bf16-MFMA backward, 128 hidden units per launch");
    using K = DyncaCfg<CP, FC, HAS_COND, TH, TW, NT, BF>;
    using Pos = TilePos<TH, TW>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const W1L = smem + K::OFF_W1;
    float* const W2L = smem + K::OFF_W2;
    float* const B1L = smem + K::OFF_B1;
    float* const B2L = smem + K::OFF_B2;
    float* const Z = smem + K::OFF_Z;
    float* const MK = smem + K::OFF_MK;
    float* const CN = smem + K::OFF_CN;
    float* const DR = smem + (MS ? K::LDS_FLOATS_MS : K::LDS_FLOATS);          // [2][TH * TW]; exists in the steered variants only (launch_dynca)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, ci = lane & 15;
    const int C = a.C, H = a.H, W = a.W, fc = a.fc, CC = a.c_cond;
    const int K1 = 4 * C + CC;

    // ---- A-operand weight images, once per workgroup -------------------------------------
    auto map_w1 = [&](int idx) -> long {
        const int l = idx & 63, s = (idx >> 6) % K::K1S, m = (idx >> 6) / K::K1S;
        const int gg = l >> 4, o = 16 * m + (l & 15);
        if (o >= fc) return -1;
        if (s < CP) {  // k-step s = 4c'+f : channel 4c'+g, filter f (0 id, 1 sobel_x, 2 sobel_y, 3 lap)
            const int ch = (s & ~3) + gg;
            return ch < C ? (long)o * K1 + (s & 3) * C + ch : -1;  // blocked [x|Sx|Sy|L], dynca.py:92-95
        }
        return gg < CC ? (long)o * K1 + 4 * C + gg : -1;  // conditioning k-step
    };
    auto map_w2 = [&](int idx) -> long {
        const int l = idx & 63, s = (idx >> 6) % K::K2S, m = (idx >> 6) / K::K2S;
        const int gg = l >> 4, o = 16 * m + (l & 15);
        const int k = 16 * (s >> 2) + 4 * gg + (s & 3);
        return (o < C && k < fc) ? (long)o * (a.w2_ld ? a.w2_ld : fc) + k : -1;
    };
    auto map_b1 = [&](int idx) -> long { return idx < fc ? idx : -1; };
    auto map_b2 = [&](int idx) -> long { return (idx < C && !ACC) ? idx : -1; };
    if constexpr (BF && BWD) {
        // bf16-MFMA backward: the forward's layer-1 image (same bits: same pre-activation), W2^T where the forward keeps W2 (the
        // backward never forms layer 2), W1^T behind the variant's carve; all rounded to bf16 (RNE) here, once.  b2 is not needed.
        using BFK = NcaDyncaBf16<CP, FC, HAS_COND>;
        auto bmap_w1 = [&](int idx, int hf) -> long { return BFK::w1_src(idx, hf, C, CC, fc); };
        auto bmap_w2t = [&](int idx, int hf) -> long {
            if constexpr (SL) return BFK::w2tw_src(idx, hf, C, fc, a.w2_ld ? a.w2_ld : fc);   // both channel tiles, rows of the full layer
            else return BFK::w2t_src(idx, hf, C, fc);
        };
        auto bmap_w1t = [&](int idx, int hf) -> long { return BFK::w1t_src(idx, hf, C, CC, fc); };
        constexpr int kW2tWords = (SL ? K::M2T : 1) * BFK::W2T_WORDS;
        static_assert(kW2tWords == K::W2_FLOATS, "W2^T takes the place of the forward's W2 image");
        FillP<BFK::W1_WORDS> f1;
        FillP<kW2tWords> f2;
        FillP<BFK::W1T_WORDS> f5;
        FillV<FC> f3;
        fill_issue_pk(f1, a.w1, tid, bmap_w1);
        fill_issue_pk(f2, a.w2, tid, bmap_w2t);
        fill_issue_pk(f5, a.w1, tid, bmap_w1t);
        fill_issue(f3, a.b1, tid, map_b1);
        fill_commit_pk(f1, W1L, tid, bmap_w1);
        fill_commit_pk(f2, W2L, tid, bmap_w2t);
        fill_commit_pk(f5, smem + K::LDS_FLOATS_BWD_W2 + (MS ? 4 * CP * K::PCS : 0), tid, bmap_w1t);
        fill_commit(f3, B1L, tid, map_b1);
    } else if constexpr (BFW) {   // the wide range: the same W1 image (up to 16 tiles x 5 chunks), the W2 image [out tile][pair][lane]
        using BFK = NcaDyncaBf16<CP, FC, HAS_COND>;
        static_assert(BFK::W1_WORDS == K::W1_FLOATS && BFK::W2W_WORDS == K::W2_FLOATS && BFK::M2T == K::M2T, "the carve holds both images");
        auto bmap_w1 = [&](int idx, int hf) -> long { return BFK::w1_src(idx, hf, C, CC, fc); };
        auto bmap_w2 = [&](int idx, int hf) -> long { return BFK::w2w_src(idx, hf, C, fc); };
        FillP<BFK::W1_WORDS> f1;
        FillP<BFK::W2W_WORDS> f2;
        FillV<FC> f3;
        FillV<K::M2T * 16> f4;
        fill_issue_pk(f1, a.w1, tid, bmap_w1);
        fill_issue_pk(f2, a.w2, tid, bmap_w2);
        fill_issue(f3, a.b1, tid, map_b1);
        fill_issue(f4, a.b2, tid, map_b2);
        fill_commit_pk(f1, W1L, tid, bmap_w1);
        fill_commit_pk(f2, W2L, tid, bmap_w2);
        fill_commit(f3, B1L, tid, map_b1);
        fill_commit(f4, B2L, tid, map_b2);
    } else if constexpr (BF) {   // both weights rounded to bf16 (RNE) here, once; eight k values per lane and entry in the bf16 k order
        using BFK = NcaDyncaBf16<CP, FC, HAS_COND>;
        auto bmap_w1 = [&](int idx, int hf) -> long { return BFK::w1_src(idx, hf, C, CC, fc); };
        auto bmap_w2 = [&](int idx, int hf) -> long { return BFK::w2_src(idx, hf, C, fc); };
        FillP<BFK::W1_WORDS> f1;
        FillP<BFK::W2_WORDS> f2;
        FillV<FC> f3;
        FillV<K::M2T * 16> f4;
        fill_issue_pk(f1, a.w1, tid, bmap_w1);
        fill_issue_pk(f2, a.w2, tid, bmap_w2);
        fill_issue(f3, a.b1, tid, map_b1);
        fill_issue(f4, a.b2, tid, map_b2);
        fill_commit_pk(f1, W1L, tid, bmap_w1);
        fill_commit_pk(f2, W2L, tid, bmap_w2);
        fill_commit(f3, B1L, tid, map_b1);
        fill_commit(f4, B2L, tid, map_b2);
    } else {
        FillV<K::M1T * K::K1S * 64> f1;
        FillV<K::M2T * K::K2S * 64> f2;
        FillV<FC> f3;
        FillV<K::M2T * 16> f4;
        fill_issue(f1, a.w1, tid, map_w1);
        fill_issue(f2, a.w2, tid, map_w2);
        fill_issue(f3, a.b1, tid, map_b1);
        fill_issue(f4, a.b2, tid, map_b2);
        fill_commit(f1, W1L, tid, map_w1);
        fill_commit(f2, W2L, tid, map_w2);
        fill_commit(f3, B1L, tid, map_b1);
        fill_commit(f4, B2L, tid, map_b2);
    }
    // Transposed operands of the backward, read from the forward images with ONE 16-byte LDS read each (the 64 lanes of a read
    // cover 1 KiB contiguously: conflict-free):
    //   W2^T, k-steps s = 0..3 of (m, m2):  W2[ch = 16 m2 + 4g + s][h = 16 m + ci]  = W2L[(m2*K2S + 4m + (ci&3))*64 + (ci>>2)*16 + 4g + s]
    //   W1^T, k-steps r = 0..3 of (m, mj):  W1[h = 16 m + 4g + r][row ci of tile mj] = W1L[(m*K1S + 4mj + (ci>>2))*64 + (ci&3)*16 + 4g + r]
    // with row ci of dL/dy tile mj standing for channel 4mj + (ci & 3), filter ci >> 2.
    const int w2t_lane = (ci & 3) * 64 + (ci >> 2) * 16 + 4 * g;
    const int w1t_lane = (ci >> 2) * 64 + (ci & 3) * 16 + 4 * g;

    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int ntiles = a.B * tiles_x * tiles_y;
    const size_t plane = (size_t)H * W;
    // fused dW2 (W2F): dW2[ch][hid] = sum_cells dO[ch][cell] * h[hid][cell] accumulated over the whole launch, one 16x16
    // tile per hidden tile m (rows = channels 4g+r, column = hidden 16m+ci), and db2 = sum_cells dO
    f32x4 w2acc[W2F ? K::M1T : 1][K::M2T];
    float b2acc[K::M2T][4];
#pragma unroll
    for (int m2 = 0; m2 < K::M2T; ++m2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) b2acc[m2][r] = 0.f;
#pragma unroll
        for (int m = 0; m < (W2F ? K::M1T : 1); ++m) w2acc[m][m2] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float* const TBW = smem + K::OFF_TB + wave * (NT * 16 * K::TBS);

    for (NcaTileWalk tw = nca_tile_walk(ntiles); tw.t < tw.end; tw.t += tw.stride) {
        const int txi = tw.t % tiles_x, tyi = (tw.t / tiles_x) % tiles_y, b = tw.t / (tiles_x * tiles_y);
        const int ty0 = tyi * TH, tx0 = txi * TW;
        const float* const xb = a.x_in + (size_t)b * C * plane;                                    // f32 storage
        const uint16_t* const xb16 = reinterpret_cast<const uint16_t*>(a.x_in) + (size_t)b * C * plane;   // bf16 storage

        // ---- issue every global load of the tile, then retire the previous tile ---------
        // (staging index made opaque per tile: its derived coordinates are recomputed here rather than
        //  hoisted out of the tile loop and kept live -- or spilled -- across the MFMA phase)
        int st = tid;
        asm volatile("" : "+v"(st));
        const int half = st >> 7;
        Pos ps;
        ps.template init<VEC>(st, ty0, tx0, H, W, a.pad_mode);
        float xv[K::CPH][4];
        RawB16<B16 ? K::CPH : 1> xr;
        if constexpr (B16) pos_load_b16<K::CPH>(ps, xb16, (unsigned)plane, half * K::CPH, C, xr);
        else pos_load<K::CPH>(ps, xb, (unsigned)plane, half * K::CPH, 0, C, xv);
        const int cr = st / TW, cq = st % TW, cgy = ty0 + cr, cgx = tx0 + cq;  // this thread's cell
        const bool cin = cgy < H && cgx < W;
        const size_t cell = (size_t)b * plane + (cin ? (size_t)cgy * W + cgx : 0);
        float uu = 0.0f, cnv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.u) {   // explicit uniforms, or bit-packed masks: bit 1 -> floor(1 + rate) = 1, bit 0 -> floor(0 + rate) = 0 (0 <= rate < 1)
            if (a.u_bits) uu = ((reinterpret_cast<const uint32_t*>(a.u)[cell >> 5] >> (unsigned)(cell & 31)) & 1u) ? 1.0f : 0.0f;
            else uu = a.u[cell];
        }
        if (HAS_COND && !BWD) {
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
                cnv[cc] = a.cond[((size_t)b * CC + min(cc, CC - 1)) * plane + (cell - (size_t)b * plane)];
        }
        float dsv = 0.0f, dcv = 1.0f;   // this cell's direction (s, c); lanes outside the image read cell 0 of the plane and stage the identity
        if constexpr (STEER) {
            const float* const db = a.dirs + (size_t)b * a.dirs_bstride + (cell - (size_t)b * plane);
            dsv = db[0];
            dcv = db[plane];
        }
        __syncthreads();  // previous tile fully consumed (also orders the weight image on iter 0)
        if (ps.active) {
#pragma unroll
            for (int c = 0; c < K::CPH; ++c) {
                const int ch = half * K::CPH + c;
                float v[4];
                if constexpr (B16) {   // widen now (exact): the loads have long landed
                    const unsigned lo = xr.v1[c][0], hi = xr.v1[c][1];
                    const float w4[4] = {__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u),
                                         __uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
#pragma unroll
                    for (int j = 0; j < 4; ++j) xv[c][j] = ps.vec ? w4[j] : nca_b16_to_f32(xr.v1[c][j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (ch < C && ps.ev[j]) ? xv[c][j] : 0.0f;
                pos_store(ps, Z + ch * K::CS, v);
            }
        }
        if (!a.u) uu = nca_philox_cell(a.seed, a.step, cell);
        MK[st] = cin ? floorf(uu + a.rate) : 0.0f;  // dynca.py:131
        if (HAS_COND && !BWD) {
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) CN[cc * TH * TW + st] = (cin && cc < CC) ? cnv[cc] : 0.0f;
        }
        if constexpr (STEER) {
            DR[st] = cin ? dsv : 0.0f;
            DR[TH * TW + st] = cin ? dcv : 1.0f;
        }
        if constexpr (MS) {
            // coarse perception tile: rows ty0/2 - 1 .. ty0/2 + TH/2, columns tx0/2 - 1 .. tx0/2 + TW/2, indices clamped into the
            // coarse image (what bilinear up-sampling does at the border, whatever the pad mode of the stencil was)
            constexpr int NR = TH / 2 + 2, NC = TW / 2 + 2, PER_PLANE = NR * NC;
            const int Hc = H >> 1, Wc = W >> 1;
            const float* const pcb = a.pc + (size_t)b * 4 * C * Hc * Wc;
            float* const PCL = smem + (BWD ? K::LDS_FLOATS_BWD_W2 : K::OFF_PC);
            for (int i = st; i < 4 * CP * PER_PLANE; i += kThreads) {
                const int pl = i / PER_PLANE, rc = i - pl * PER_PLANE, r = rc / NC, c = rc - r * NC;
                const int f = pl / CP, ch = pl - f * CP;
                const int sy = min(max((ty0 >> 1) - 1 + r, 0), Hc - 1), sx = min(max((tx0 >> 1) - 1 + c, 0), Wc - 1);
                PCL[pl * K::PCS + r * K::PCR + c] = ch < C ? pcb[((size_t)(f * C + ch) * Hc + sy) * Wc + sx] : 0.0f;
            }
        }
        __syncthreads();

#pragma unroll 1
        for (int it = 0; it < K::ITERS; ++it) {
            int r0[NT], q0[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int j = (it * 4 + wave) * NT + n;
                r0[n] = j / K::TWN;
                q0[n] = (j % K::TWN) * 16 + ci;
            }
            // ---- perception: B operands of layer 1 ---------------------------------------
            float P[NT][K::K1S];
#pragma unroll
            for (int cq4 = 0; cq4 < CP / 4; ++cq4) {
                const float* const zc = Z + (4 * cq4 + g) * K::CS + 3;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    float nb[3][3];
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) nb[dy][dx] = zc[(r0[n] + dy) * K::RS + q0[n] + dx];
                    P[n][4 * cq4 + 0] = nb[1][1];
                    P[n][4 * cq4 + 1] = nca_sobel_x(nb);
                    P[n][4 * cq4 + 2] = nca_sobel_y(nb);
                    P[n][4 * cq4 + 3] = nca_laplacian(nb);
                    if constexpr (MS) {
                        // + bilinear x2 up-sampling (align_corners = False) of the coarse perception, then the mean over the two
                        // scales (dynca.py:98, :105-110).  Fine row r = 2k: rows (k-1, k) with lambdas (0.25, 0.75); r = 2k+1:
                        // (k, k+1) with (0.75, 0.25); the tile has a coarse halo of 1, indices clamped at staging.
                        const int fr = r0[n], fq = q0[n];
                        const int kr = (fr >> 1) + ((fr & 1) ? 1 : 0), kq = (fq >> 1) + ((fq & 1) ? 1 : 0);   // first of the two coarse rows / cols (tile coordinates incl. halo)
                        const float h1 = (fr & 1) ? 0.25f : 0.75f, w1 = (fq & 1) ? 0.25f : 0.75f, h0 = 1.0f - h1, w0 = 1.0f - w1;
                        const float* const pcp = smem + (BWD ? K::LDS_FLOATS_BWD_W2 : K::OFF_PC) + (4 * cq4 + g) * K::PCS + kr * K::PCR + kq;
#pragma unroll
                        for (int f = 0; f < 4; ++f) {
                            const float* const q = pcp + f * CP * K::PCS;
                            P[n][4 * cq4 + f] = nca_up2_blend(P[n][4 * cq4 + f], q[0], q[1], q[K::PCR], q[K::PCR + 1], h0, h1, w0, w1);
                        }
                    }
                }
            }
            // steered perception: the final (blended) Sobel pair of every channel rotated by the cell's direction, in fp32, before the
            // conditioning rows are appended and before any bf16 rounding of the operand
            if constexpr (STEER) {
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const float ds = DR[r0[n] * TW + q0[n]], dc = DR[TH * TW + r0[n] * TW + q0[n]];
#pragma unroll
                    for (int cq4 = 0; cq4 < CP / 4; ++cq4) nca_steer(P[n][4 * cq4 + 1], P[n][4 * cq4 + 2], ds, dc);
                }
            }
            if (HAS_COND) {
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if constexpr (BWD) {   // conditioning channel g of the lane's cell, straight from memory (64-byte segments per lane group)
                        const int gy = min(ty0 + r0[n], H - 1), gx = min(tx0 + q0[n], W - 1);
                        const float cv = a.cond[((size_t)b * CC + min(g, CC - 1)) * plane + (size_t)gy * W + gx];
                        P[n][CP] = (g < CC && ty0 + r0[n] < H && tx0 + q0[n] < W) ? cv : 0.0f;
                    } else P[n][CP] = CN[g * TH * TW + r0[n] * TW + q0[n]];
                }
            }
            if constexpr (BWD && BF) {
                if constexpr (!SL) {   // the narrow range; the lines up to the else are as they were (not re-indented): these kernels' streams are held fixed
                // ---- backward data path on bf16 MFMA ("bf16-MFMA training", include/ncahip.h) -------------------------------
                // Lane (g, ci) of group n holds, in the accumulator layout throughout: a1 / dh of hidden 16m + 4g + r, gb of channel
                // 4g + r, dL/dy of (filter g, channel 4mj + r), all of cell ci.  Every operand is rounded once (RNE) and every
                // consumer reads those bits: yb feeds layer 1 and is written out, gb feeds dh, dW2 and db2, dhb feeds dL/dy and
                // is written out, hb feeds dW2.
                using BFK = NcaDyncaBf16<CP, FC, HAS_COND>;
                static_assert(NT == 2 && K::M2T == 1, "dW2 takes the pass's 2 x 16 cells as ONE K = 32 product");
                typedef short nca_s16x4 __attribute__((ext_vector_type(4)));
                typedef unsigned nca_u32x2 __attribute__((ext_vector_type(2)));
                const nca_u32x4* const W1B = reinterpret_cast<const nca_u32x4*>(W1L) + lane;
                const nca_u32x2* const W2T = reinterpret_cast<const nca_u32x2*>(W2L) + lane;
                const nca_u32x4* const W1T = reinterpret_cast<const nca_u32x4*>(smem + K::LDS_FLOATS_BWD_W2 + (MS ? 4 * CP * K::PCS : 0)) + lane;
                auto lo16 = [](unsigned w) { return __uint_as_float(w << 16); };
                auto hi16 = [](unsigned w) { return __uint_as_float(w & 0xffff0000u); };
                bool live[NT];
                size_t cello[NT];
                nca_u32x2 gbp[NT];      // gb = bf16(g * mask), channels 4g .. 4g + 3
                unsigned doTp[4];       // the same, transposed: channel ci of cells (n, 4s + g), k = 4n + s
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int gy = ty0 + r0[n], gx = tx0 + q0[n];
                    live[n] = gy < H && gx < W;
                    cello[n] = live[n] ? (size_t)gy * W + gx : 0;
                    const float mk = MK[r0[n] * TW + q0[n]];
                    const float* const gp = a.g_next + (size_t)b * C * plane + cello[n];
                    float gm[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = 4 * g + r;
                        const float gv = gp[(size_t)min(ch, C - 1) * plane];
                        gm[r] = (live[n] && ch < C) ? gv * mk : 0.0f;
                    }
                    gbp[n] = nca_u32x2{nca_pk_bf16(gm[0], gm[1]), nca_pk_bf16(gm[2], gm[3])};
                    const f32x4 gr = f32x4{lo16(gbp[n][0]), hi16(gbp[n][0]), lo16(gbp[n][1]), hi16(gbp[n][1])};
                    *reinterpret_cast<f32x4*>(TBW + n * 16 * K::TBS + ci * K::TBS + 4 * g) = gr;
#pragma unroll
                    for (int r = 0; r < 4; ++r) b2acc[0][r] += gr[r];   // db2 sums the rounded operand
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    float t4[4];
#pragma unroll
                    for (int s_ = 0; s_ < 4; ++s_) t4[s_] = TBW[n * 16 * K::TBS + (4 * s_ + g) * K::TBS + ci];
                    doTp[2 * n] = nca_pk_bf16(t4[0], t4[1]);         // exact: the values are bf16 already
                    doTp[2 * n + 1] = nca_pk_bf16(t4[2], t4[3]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                nca_u32x4 PB[NT][BFK::K1Q];
                BFK::template pack_y<NT>(P, PB);
                // yb out: slot s = 4c' + f of lane (g, cell) is row f*C + 4c' + g of perceive_torch's output (conditioning slot: not written)
                {
                    uint16_t* const yo = reinterpret_cast<uint16_t*>(a.ybuf) + (size_t)b * 4 * C * plane;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        if (!live[n]) continue;
#pragma unroll
                        for (int s = 0; s < CP; ++s)
                            if ((s & ~3) + g < C) {
                                const unsigned w = PB[n][s >> 3][(s & 7) >> 1];
                                yo[(size_t)((s & 3) * C + (s & ~3) + g) * plane + cello[n]] = (uint16_t)((s & 1) ? (w >> 16) : (w & 0xffffu));
                            }
                    }
                }
                uint16_t* const dho = reinterpret_cast<uint16_t*>(a.dhbuf) + (size_t)b * fc * plane;
                f32x4 dY[K::MJ][NT];
#pragma unroll
                for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                    for (int n = 0; n < NT; ++n) dY[mj][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int p = 0; p < BFK::M1P; ++p) {
                    nca_u32x4 dhb[NT];
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const int m = 2 * p + hf;
                        f32x4 acc1[NT], dacc[NT];
                        BFK::template layer1<NT>(W1B, B1L, m, g, PB, acc1);
                        const nca_u32x2 wt2 = W2T[m * 64];
#pragma unroll
                        for (int n = 0; n < NT; ++n)
                            dacc[n] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(nca_s16x4, wt2), __builtin_bit_cast(nca_s16x4, gbp[n]),
                                                                                f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            float hv[4], dv[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                hv[r] = __int_as_float(max(__float_as_int(acc1[n][r]), 0));   // relu, as the forward takes it
                                dv[r] = acc1[n][r] > 0.0f ? dacc[n][r] : 0.0f;                // relu' = 0 at exactly 0
                            }
                            const unsigned h01 = nca_pk_bf16(hv[0], hv[1]), h23 = nca_pk_bf16(hv[2], hv[3]);
                            const unsigned d01 = nca_pk_bf16(dv[0], dv[1]), d23 = nca_pk_bf16(dv[2], dv[3]);
                            dhb[n][2 * hf] = d01;
                            dhb[n][2 * hf + 1] = d23;
                            if (live[n]) {
                                uint16_t* const o = dho + (size_t)(16 * m + 4 * g) * plane + cello[n];
                                if (16 * m + 4 * g + 0 < fc) o[0] = (uint16_t)(d01 & 0xffffu);
                                if (16 * m + 4 * g + 1 < fc) o[plane] = (uint16_t)(d01 >> 16);
                                if (16 * m + 4 * g + 2 < fc) o[2 * plane] = (uint16_t)(d23 & 0xffffu);
                                if (16 * m + 4 * g + 3 < fc) o[3 * plane] = (uint16_t)(d23 >> 16);
                            }
                            // hb of the group, for dW2 (cells outside the image and hidden units beyond fc meet gb = 0 / are never read)
                            *reinterpret_cast<f32x4*>(TBW + n * 16 * K::TBS + ci * K::TBS + 4 * g) = f32x4{lo16(h01), hi16(h01), lo16(h23), hi16(h23)};
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        nca_u32x4 hTp;
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            float t4[4];
#pragma unroll
                            for (int s_ = 0; s_ < 4; ++s_) t4[s_] = TBW[n * 16 * K::TBS + (4 * s_ + g) * K::TBS + ci];
                            hTp[2 * n] = nca_pk_bf16(t4[0], t4[1]);
                            hTp[2 * n + 1] = nca_pk_bf16(t4[2], t4[3]);
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the tiles are rewritten by the next hidden tile
                        w2acc[m][0] = nca_mfma_bf16(nca_u32x4{doTp[0], doTp[1], doTp[2], doTp[3]}, hTp, w2acc[m][0]);
                    }
#pragma unroll
                    for (int mj = 0; mj < K::MJ; ++mj) {
                        const nca_u32x4 wt1 = W1T[(p * K::MJ + mj) * 64];
#pragma unroll
                        for (int n = 0; n < NT; ++n) dY[mj][n] = nca_mfma_bf16(wt1, dhb[n], dY[mj][n]);
                    }
                }
                // dL/dy out, fp32: tile mj, register r of lane (g, cell) = channel 4mj + r, filter g -> plane g*C + 4mj + r
                const unsigned plane4 = (unsigned)plane * 4u;
                const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(a.dybuf + (size_t)b * 4 * C * plane, 0, -1, 0x00020000);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if (!live[n]) continue;
                    const unsigned voy = (unsigned)cello[n] * 4u + (unsigned)(g * C) * plane4;
#pragma unroll
                    for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (4 * mj + r < C)
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dY[mj][n][r]), rdy, (int)voy, (int)((unsigned)(4 * mj + r) * plane4), 0);
                }
                } else {
                    // ---- the same on one 128-wide slice of a wide layer and K::M2T channel tiles (nca_dynca_bwd_bf16_wide.hip) -------
                    using BFK = NcaDyncaBf16<CP, FC, HAS_COND>;
                    // Two channel tiles (CP = 32): gb, db2 and the transposed gb exist per tile t (channels 16t + 4g + r); dh sums the two
                    // tiles' 16x16x16 products in the order t = 0, 1; dW2 | db2 take one K = 32 product per tile and hidden tile.
                    static_assert(NT == 2, "dW2 takes the pass's 2 x 16 cells as ONE K = 32 product");
                    const int fcf = a.w2_ld ? a.w2_ld : fc;   // rows of dh_out per batch item: the full layer's
                    typedef short nca_s16x4 __attribute__((ext_vector_type(4)));
                    typedef unsigned nca_u32x2 __attribute__((ext_vector_type(2)));
                    const nca_u32x4* const W1B = reinterpret_cast<const nca_u32x4*>(W1L) + lane;
                    const nca_u32x2* const W2T = reinterpret_cast<const nca_u32x2*>(W2L) + lane;
                    const nca_u32x4* const W1T = reinterpret_cast<const nca_u32x4*>(smem + K::LDS_FLOATS_BWD_W2 + (MS ? 4 * CP * K::PCS : 0)) + lane;
                    auto lo16 = [](unsigned w) { return __uint_as_float(w << 16); };
                    auto hi16 = [](unsigned w) { return __uint_as_float(w & 0xffff0000u); };
                    bool live[NT];
                    size_t cello[NT];
                    nca_u32x2 gbp[K::M2T][NT];      // gb = bf16(g * mask), channels 16t + 4g .. 16t + 4g + 3
                    unsigned doTp[K::M2T][4];       // the same, transposed: channel 16t + ci of cells (n, 4s + g), k = 4n + s
#pragma unroll
                    for (int t = 0; t < K::M2T; ++t) {   // one channel tile at a time through the wave's transposition tiles
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            if (t == 0) {
                                const int gy = ty0 + r0[n], gx = tx0 + q0[n];
                                live[n] = gy < H && gx < W;
                                cello[n] = live[n] ? (size_t)gy * W + gx : 0;
                            }
                            const float mk = MK[r0[n] * TW + q0[n]];
                            const float* const gp = a.g_next + (size_t)b * C * plane + cello[n];
                            float gm[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int ch = 16 * t + 4 * g + r;
                                const float gv = gp[(size_t)min(ch, C - 1) * plane];
                                gm[r] = (live[n] && ch < C) ? gv * mk : 0.0f;
                            }
                            gbp[t][n] = nca_u32x2{nca_pk_bf16(gm[0], gm[1]), nca_pk_bf16(gm[2], gm[3])};
                            const f32x4 gr = f32x4{lo16(gbp[t][n][0]), hi16(gbp[t][n][0]), lo16(gbp[t][n][1]), hi16(gbp[t][n][1])};
                            *reinterpret_cast<f32x4*>(TBW + n * 16 * K::TBS + ci * K::TBS + 4 * g) = gr;
#pragma unroll
                            for (int r = 0; r < 4; ++r) b2acc[t][r] += gr[r];   // db2 sums the rounded operand
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            float t4[4];
#pragma unroll
                            for (int s_ = 0; s_ < 4; ++s_) t4[s_] = TBW[n * 16 * K::TBS + (4 * s_ + g) * K::TBS + ci];
                            doTp[t][2 * n] = nca_pk_bf16(t4[0], t4[1]);         // exact: the values are bf16 already
                            doTp[t][2 * n + 1] = nca_pk_bf16(t4[2], t4[3]);
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    }
                    nca_u32x4 PB[NT][BFK::K1Q];
                    BFK::template pack_y<NT>(P, PB);
                    // yb out: slot s = 4c' + f of lane (g, cell) is row f*C + 4c' + g of perceive_torch's output (conditioning slot: not written)
                    if constexpr (!ACC) {   // later slices: the first one wrote it
                        uint16_t* const yo = reinterpret_cast<uint16_t*>(a.ybuf) + (size_t)b * 4 * C * plane;
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            if (!live[n]) continue;
#pragma unroll
                            for (int s = 0; s < CP; ++s)
                                if ((s & ~3) + g < C) {
                                    const unsigned w = PB[n][s >> 3][(s & 7) >> 1];
                                    yo[(size_t)((s & 3) * C + (s & ~3) + g) * plane + cello[n]] = (uint16_t)((s & 1) ? (w >> 16) : (w & 0xffffu));
                                }
                        }
                    }
                    uint16_t* const dho = reinterpret_cast<uint16_t*>(a.dhbuf) + (size_t)b * fcf * plane;
                    f32x4 dY[K::MJ][NT];
#pragma unroll
                    for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                        for (int n = 0; n < NT; ++n) dY[mj][n] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if constexpr (ACC) {   // a later slice: the accumulators start at the dL/dy the earlier slices wrote (cells outside the image: cell 0, never stored)
                        const unsigned pl4 = (unsigned)plane * 4u;
                        const __amdgpu_buffer_rsrc_t rprev = __builtin_amdgcn_make_buffer_rsrc(a.dybuf + (size_t)b * 4 * C * plane, 0, -1, 0x00020000);
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            const unsigned vprev = (unsigned)cello[n] * 4u + (unsigned)(g * C) * pl4;
#pragma unroll
                            for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    dY[mj][n][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rprev, (int)vprev, (int)((unsigned)min(4 * mj + r, C - 1) * pl4), 0));
                        }
                    }
#pragma unroll
                    for (int p = 0; p < BFK::M1P; ++p) {
                        nca_u32x4 dhb[NT];
#pragma unroll
                        for (int hf = 0; hf < 2; ++hf) {
                            const int m = 2 * p + hf;
                            f32x4 acc1[NT], dacc[NT];
                            BFK::template layer1<NT>(W1B, B1L, m, g, PB, acc1);
#pragma unroll
                            for (int t = 0; t < K::M2T; ++t) {
                                const nca_u32x2 wt2 = W2T[(m * K::M2T + t) * 64];
#pragma unroll
                                for (int n = 0; n < NT; ++n)
                                    dacc[n] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(nca_s16x4, wt2), __builtin_bit_cast(nca_s16x4, gbp[t][n]),
                                                                                        t == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : dacc[n], 0, 0, 0);
                            }
#pragma unroll
                            for (int n = 0; n < NT; ++n) {
                                float hv[4], dv[4];
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    hv[r] = __int_as_float(max(__float_as_int(acc1[n][r]), 0));   // relu, as the forward takes it
                                    dv[r] = acc1[n][r] > 0.0f ? dacc[n][r] : 0.0f;                // relu' = 0 at exactly 0
                                }
                                const unsigned h01 = nca_pk_bf16(hv[0], hv[1]), h23 = nca_pk_bf16(hv[2], hv[3]);
                                const unsigned d01 = nca_pk_bf16(dv[0], dv[1]), d23 = nca_pk_bf16(dv[2], dv[3]);
                                dhb[n][2 * hf] = d01;
                                dhb[n][2 * hf + 1] = d23;
                                if (live[n]) {
                                    uint16_t* const o = dho + (size_t)(16 * m + 4 * g) * plane + cello[n];
                                    if (16 * m + 4 * g + 0 < fc) o[0] = (uint16_t)(d01 & 0xffffu);
                                    if (16 * m + 4 * g + 1 < fc) o[plane] = (uint16_t)(d01 >> 16);
                                    if (16 * m + 4 * g + 2 < fc) o[2 * plane] = (uint16_t)(d23 & 0xffffu);
                                    if (16 * m + 4 * g + 3 < fc) o[3 * plane] = (uint16_t)(d23 >> 16);
                                }
                                // hb of the group, for dW2 (cells outside the image and hidden units beyond fc meet gb = 0 / are never read)
                                *reinterpret_cast<f32x4*>(TBW + n * 16 * K::TBS + ci * K::TBS + 4 * g) = f32x4{lo16(h01), hi16(h01), lo16(h23), hi16(h23)};
                            }
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            nca_u32x4 hTp;
#pragma unroll
                            for (int n = 0; n < NT; ++n) {
                                float t4[4];
#pragma unroll
                                for (int s_ = 0; s_ < 4; ++s_) t4[s_] = TBW[n * 16 * K::TBS + (4 * s_ + g) * K::TBS + ci];
                                hTp[2 * n] = nca_pk_bf16(t4[0], t4[1]);
                                hTp[2 * n + 1] = nca_pk_bf16(t4[2], t4[3]);
                            }
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the tiles are rewritten by the next hidden tile
#pragma unroll
                            for (int t = 0; t < K::M2T; ++t)
                                w2acc[m][t] = nca_mfma_bf16(nca_u32x4{doTp[t][0], doTp[t][1], doTp[t][2], doTp[t][3]}, hTp, w2acc[m][t]);
                        }
#pragma unroll
                        for (int mj = 0; mj < K::MJ; ++mj) {
                            const nca_u32x4 wt1 = W1T[(p * K::MJ + mj) * 64];
#pragma unroll
                            for (int n = 0; n < NT; ++n) dY[mj][n] = nca_mfma_bf16(wt1, dhb[n], dY[mj][n]);
                        }
                    }
                    // dL/dy out, fp32: tile mj, register r of lane (g, cell) = channel 4mj + r, filter g -> plane g*C + 4mj + r
                    const unsigned plane4 = (unsigned)plane * 4u;
                    const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(a.dybuf + (size_t)b * 4 * C * plane, 0, -1, 0x00020000);
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        if (!live[n]) continue;
                        const unsigned voy = (unsigned)cello[n] * 4u + (unsigned)(g * C) * plane4;
#pragma unroll
                        for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (4 * mj + r < C)
                                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dY[mj][n][r]), rdy, (int)voy, (int)((unsigned)(4 * mj + r) * plane4), 0);
                    }
                }
            } else if constexpr (BWD) {
                // ---- backward data path -----------------------------------------------------------------
                float dO[NT][K::M2T][4];   // dL/d(out) = G * mask, accumulator layout (channel 16 m2 + 4g + r, cell ci)
                bool live[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int gy = ty0 + r0[n], gx = tx0 + q0[n];
                    live[n] = gy < H && gx < W;
                    const float mk = MK[r0[n] * TW + q0[n]];
                    const float* const gb = a.g_next + (size_t)b * C * plane + (live[n] ? (size_t)gy * W + gx : 0);
#pragma unroll
                    for (int m2 = 0; m2 < K::M2T; ++m2)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = 16 * m2 + 4 * g + r;
                            const float gv = gb[(size_t)min(ch, C - 1) * plane];
                            dO[n][m2][r] = (live[n] && ch < C) ? gv * mk : 0.0f;
                        }
                }
                // The perception just recomputed is also the B operand of the layer-1 weight-gradient product (dW1 = dh y^T, in
                // gram_rows_kernel): written out here -- slot 4c'+f of lane (g, cell) is channel 4c'+g, filter f, i.e. row
                // f*C + 4c'+g of perceive_torch's output; lane part of the address once per n, row part a scalar offset -- instead
                // of a perception (and, two-scale, a combine) launch of its own that re-reads x_t.
                if constexpr (!ACC) {
                    if (a.ybuf) {
                        const unsigned pl4 = (unsigned)plane * 4u;
                        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.ybuf + (size_t)b * 4 * C * plane, 0, -1, 0x00020000);
#pragma unroll
                        for (int n = 0; n < NT; ++n) {
                            if (!live[n]) continue;
                            const unsigned vy = (unsigned)((ty0 + r0[n]) * W + tx0 + q0[n]) * 4u + (unsigned)g * pl4;
#pragma unroll
                            for (int cq4 = 0; cq4 < CP / 4; ++cq4)
                                if (4 * cq4 + g < C) {
#pragma unroll
                                    for (int f = 0; f < 4; ++f)
                                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(P[n][4 * cq4 + f]), ry, (int)vy,
                                                                              (int)((unsigned)(f * C + 4 * cq4) * pl4), 0);
                                }
                        }
                    }
                }
                // Output addressing: the lane's part (cell, lane-dependent row group) is ONE vector offset per n, the remaining row
                // index of each store a scalar offset -- per-store 64-bit vector address arithmetic was ~1300 VALU instructions per
                // pass, in the same issue slots as the exact-f32 MFMAs.  (Launcher: fc*H*W*4 and 4C*H*W*4 below 4 GiB.)
                const unsigned plane4 = (unsigned)plane * 4u;
                const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(a.hbuf + (size_t)b * fc * plane, 0, -1, 0x00020000);
                const __amdgpu_buffer_rsrc_t rdh = __builtin_amdgcn_make_buffer_rsrc(a.dhbuf + (size_t)b * fc * plane, 0, -1, 0x00020000);
                const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(a.dybuf + (size_t)b * 4 * C * plane, 0, -1, 0x00020000);
                unsigned vo[NT], voy[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const unsigned cellb = live[n] ? (unsigned)((ty0 + r0[n]) * W + tx0 + q0[n]) * 4u : 0u;
                    vo[n] = cellb + (unsigned)(4 * g) * plane4;             // h / dh rows 16m + 4g + r
                    voy[n] = cellb + (unsigned)(g * C) * plane4;            // dL/dy rows g*C + (4mj + r): filter g, channel 4mj + r
                }
                const int lim_h = fc - 4 * g;   // row 16m + 4g + r exists <=> 16m + r < lim_h
                // fused dW2: the A operands dO[ch = ci][cell 4s+g] of every n, transposed once per pass through the wave's
                // LDS tiles (lane (g,ci) writes its four channel rows of cell ci with one 16-byte store per channel tile)
                float doT[W2F ? NT : 1][K::M2T][4];
                if constexpr (W2F) {
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int m2 = 0; m2 < K::M2T; ++m2) {
                            *reinterpret_cast<f32x4*>(TBW + n * 16 * K::TBS + ci * K::TBS + 16 * m2 + 4 * g) =
                                f32x4{dO[n][m2][0], dO[n][m2][1], dO[n][m2][2], dO[n][m2][3]};
#pragma unroll
                            for (int r = 0; r < 4; ++r) b2acc[m2][r] += dO[n][m2][r];
                        }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int m2 = 0; m2 < K::M2T; ++m2)
#pragma unroll
                            for (int s_ = 0; s_ < 4; ++s_) doT[n][m2][s_] = TBW[n * 16 * K::TBS + (4 * s_ + g) * K::TBS + 16 * m2 + ci];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                }
                f32x4 dY[K::MJ][NT];
#pragma unroll
                for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                    for (int n = 0; n < NT; ++n) dY[mj][n] = f32x4{0.f, 0.f, 0.f, 0.f};
                // A operands are read from LDS a whole section ahead of their MFMAs (one wave per SIMD: a read issued right
                // before its use costs the full LDS round trip each time): layer-1 operands of hidden tile m+1 during the
                // dL/dy products of tile m, the transposed operands of tile m during its layer-1 chain.  The fences keep the
                // compiler from sinking the reads back to their uses.
                float wa1[K::K1S];
                f32x4 wt2[K::M2T], wt1[K::MJ];
                f32x4 bias1;
                auto fetch1 = [&](int m) {
                    const float* const w1m = W1L + m * K::K1S * 64 + lane;
#pragma unroll
                    for (int s = 0; s < K::K1S; ++s) wa1[s] = w1m[s * 64];
                    bias1 = *reinterpret_cast<const f32x4*>(B1L + 16 * m + 4 * g);
                };
                auto fetch_t = [&](int m) {
#pragma unroll
                    for (int m2 = 0; m2 < K::M2T; ++m2) wt2[m2] = *reinterpret_cast<const f32x4*>(W2L + (m2 * K::K2S + 4 * m) * 64 + w2t_lane);
#pragma unroll
                    for (int mj = 0; mj < K::MJ; ++mj) wt1[mj] = *reinterpret_cast<const f32x4*>(W1L + (m * K::K1S + 4 * mj) * 64 + w1t_lane);
                };
                // later slices of a wide hidden layer add to the dL/dy the earlier launches wrote: those partial sums are requested
                // here, a whole MFMA phase ahead of their use (one wave per SIMD: a load issued next to its use costs its full latency)
                float prev[ACC ? NT : 1][ACC ? K::MJ : 1][4];
                if constexpr (ACC) {
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                prev[n][mj][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                    rdy, (int)voy[n], (int)((unsigned)min(4 * mj + r, C - 1) * plane4), 0));
                }
                fetch1(0);
                float hT[W2F ? NT : 1][4];
                constexpr int kUnrollM1 = W2F ? K::M1T : 1;   // fused dW2: w2acc[m] is indexed by the hidden tile and must stay in registers
#pragma unroll kUnrollM1
                for (int m = 0; m < K::M1T; ++m) {
                    f32x4 acc1[NT], dacc[NT];
#pragma unroll
                    for (int n = 0; n < NT; ++n) { acc1[n] = bias1; dacc[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }
                    fetch_t(m);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int s = 0; s < K::K1S; ++s) {
#pragma unroll
                        for (int n = 0; n < NT; ++n) acc1[n] = nca_mfma(wa1[s], P[n][s], acc1[n]);
                    }
#pragma unroll
                    for (int m2 = 0; m2 < K::M2T; ++m2)
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
#pragma unroll
                            for (int n = 0; n < NT; ++n) dacc[n] = nca_mfma(wt2[m2][s], dO[n][m2][s], dacc[n]);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                    if (m + 1 < K::M1T) fetch1(m + 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float hv = fmaxf(acc1[n][r], 0.0f);
                            const float dv = acc1[n][r] > 0.0f ? dacc[n][r] : 0.0f;   // relu' = 0 at exactly 0
                            dacc[n][r] = dv;
                            if (live[n] && 16 * m + r < lim_h) {
                                const int so = (int)((unsigned)(16 * m + r) * plane4);
                                if constexpr (!W2F) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hv), rh, (int)vo[n], so, 0);
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dv), rdh, (int)vo[n], so, 0);
                            }
                            if constexpr (W2F) acc1[n][r] = (live[n] && 16 * m + r < lim_h) ? hv : 0.0f;   // h, zero outside the image / fc
                        }
                        if constexpr (W2F) *reinterpret_cast<f32x4*>(TBW + n * 16 * K::TBS + ci * K::TBS + 4 * g) = acc1[n];
                    }
                    if constexpr (W2F) {   // B operands h[cell 4s+g][hid ci]: requested here, consumed after the dL/dy products
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
                        for (int n = 0; n < NT; ++n)
#pragma unroll
                            for (int s_ = 0; s_ < 4; ++s_) hT[n][s_] = TBW[n * 16 * K::TBS + (4 * s_ + g) * K::TBS + ci];
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int mj = 0; mj < K::MJ; ++mj) {
#pragma unroll
                            for (int n = 0; n < NT; ++n) dY[mj][n] = nca_mfma(wt1[mj][r], dacc[n][r], dY[mj][n]);
                        }
                    if constexpr (W2F) {
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int n = 0; n < NT; ++n)
#pragma unroll
                            for (int m2 = 0; m2 < K::M2T; ++m2)
#pragma unroll
                                for (int s_ = 0; s_ < 4; ++s_) w2acc[m][m2] = nca_mfma(doT[n][m2][s_], hT[n][s_], w2acc[m][m2]);
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the tiles are rewritten by the next hidden tile
                    }
                }
                // dL/dy out: tile mj, register r of lane (g, cell) = channel 4mj + r, filter g -> plane g*C + 4mj + r.  Later
                // slices of a wide hidden layer (ACC) add to what the earlier launches wrote.
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if (!live[n]) continue;
#pragma unroll
                    for (int mj = 0; mj < K::MJ; ++mj)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (4 * mj + r < C) {
                                float v = dY[mj][n][r];
                                if constexpr (ACC) v += prev[n][mj][r];
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rdy, (int)voy[n],
                                                                      (int)((unsigned)(4 * mj + r) * plane4), 0);
                            }
                        }
                }
            } else {
                // ---- MLP on MFMA: layer 1 streamed tile-by-tile into layer 2 -----------------
                // Issue order (see nca_cond_tile.h, mlp_tile_regs): the A operands of hidden tile m+1 are read from LDS
                // while tile m's MFMA chain runs (an LDS read next to its use stalls the in-order pipe for the whole
                // latency), and the ReLUs are issued as ONE fenced group per tile (a VALU instruction inside an f32 MFMA
                // stream drains the matrix pipe: ~25 cycles each when scattered).
                f32x4 acc2[K::M2T][NT];
    #pragma unroll
                for (int m2 = 0; m2 < K::M2T; ++m2) {
                    const f32x4 bias = *reinterpret_cast<const f32x4*>(B2L + 16 * m2 + 4 * g);
    #pragma unroll
                    for (int n = 0; n < NT; ++n) acc2[m2][n] = bias;
                }
                // later fc slice: the partial result of the earlier launches is requested now, a whole MLP ahead of its use
                float xprev[ACC ? NT : 1][K::M2T][4];
                if constexpr (ACC) {
    #pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const int gy = min(ty0 + r0[n], H - 1), gx = min(tx0 + q0[n], W - 1);
                        const float* const ob = a.x_out + (size_t)b * C * plane + (size_t)gy * W + gx;
    #pragma unroll
                        for (int m2 = 0; m2 < K::M2T; ++m2)
    #pragma unroll
                            for (int r = 0; r < 4; ++r) xprev[n][m2][r] = ob[(size_t)min(16 * m2 + 4 * g + r, C - 1) * plane];
                    }
                }
                if constexpr (BFW) {   // the same on two output tiles and / or sixteen hidden tiles, still one pass over the perception
                    NcaDyncaBf16<CP, FC, HAS_COND>::template mlp_wide<NT>(W1L, W2L, B1L, B2L, P, lane, g, acc2);
                } else if constexpr (BF) {   // both products on bf16 MFMA, operands rounded to nearest even (nca_dynca_bf16.h)
                    NcaDyncaBf16<CP, FC, HAS_COND>::template mlp<NT>(W1L, W2L, B1L, B2L, P, lane, g, acc2[0]);
                } else {   // exact fp32: the lines up to the closing brace are as they were (not re-indented)
                float wa1[K::K1S], wa2[4][K::M2T];
                f32x4 bias1;
                auto fetch = [&](int m) {
                    const float* const w1m = W1L + m * K::K1S * 64 + lane;
    #pragma unroll
                    for (int s = 0; s < K::K1S; ++s) wa1[s] = w1m[s * 64];
                    const float* const w2m = W2L + (4 * m) * 64 + lane;
    #pragma unroll
                    for (int r = 0; r < 4; ++r)
    #pragma unroll
                        for (int m2 = 0; m2 < K::M2T; ++m2) wa2[r][m2] = w2m[(m2 * K::K2S + r) * 64];
                    bias1 = *reinterpret_cast<const f32x4*>(B1L + 16 * m + 4 * g);
                };
                fetch(0);
    #pragma unroll 1
                for (int m = 0; m < K::M1T; ++m) {
                    f32x4 acc1[NT];
    #pragma unroll
                    for (int n = 0; n < NT; ++n) acc1[n] = bias1;
    #pragma unroll
                    for (int s = 0; s < K::K1S; ++s)
    #pragma unroll
                        for (int n = 0; n < NT; ++n) acc1[n] = nca_mfma(wa1[s], P[n][s], acc1[n]);
                    float w2c[4][K::M2T];
    #pragma unroll
                    for (int r = 0; r < 4; ++r)
    #pragma unroll
                        for (int m2 = 0; m2 < K::M2T; ++m2) w2c[r][m2] = wa2[r][m2];
                    __builtin_amdgcn_sched_barrier(0);
                    if (m + 1 < K::M1T) fetch(m + 1);        // in flight across this tile's layer-2 MFMAs and the next chain
                    float h[NT][4];
    #pragma unroll
                    for (int n = 0; n < NT; ++n)
    #pragma unroll
                        for (int r = 0; r < 4; ++r) h[n][r] = __int_as_float(max(__float_as_int(acc1[n][r]), 0));   // relu
                    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                    for (int r = 0; r < 4; ++r)
    #pragma unroll
                        for (int m2 = 0; m2 < K::M2T; ++m2)
    #pragma unroll
                            for (int n = 0; n < NT; ++n) acc2[m2][n] = nca_mfma(w2c[r][m2], h[n][r], acc2[m2][n]);
                }
                }
                // ---- residual + stochastic mask (dynca.py:131-133) ---------------------------
    #pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int gy = ty0 + r0[n], gx = tx0 + q0[n];
                    if (gy < H && gx < W) {
                        const float mk = MK[r0[n] * TW + q0[n]];
                        const size_t o0 = (size_t)b * C * plane + (size_t)gy * W + gx;
                        const float* const ob = a.x_out + o0;
                        (void)ob;
                        const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(a.x_out + (size_t)b * C * plane, 0, -1, 0x00020000);
                        const unsigned ooff = (unsigned)(gy * W + gx) * 4u;
                        uint16_t* const ob16 = reinterpret_cast<uint16_t*>(a.x_out) + o0;
    #pragma unroll
                        for (int m2 = 0; m2 < K::M2T; ++m2)
    #pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int ch = 16 * m2 + 4 * g + r;
                                if (ch < C) {
                                    float xo = Z[ch * K::CS + (r0[n] + 1) * K::RS + q0[n] + 4];
                                    if constexpr (ACC) xo = xprev[n][m2][r];           // later fc slice: add to the partial result
                                    const float xn = xo + acc2[m2][n][r] * mk;
                                    if constexpr (B16) ob16[ch * plane] = nca_f32_to_b16(xn);
                                    else   // write-through (sc1): no dirty lines left for the end-of-kernel L2 write-back
                                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xn), orsrc, (int)((unsigned)ch * (unsigned)plane * 4u + ooff), 0, 16);
                                }
                            }
                    }
                }

            }
        }
    }
    if constexpr (W2F) {
        // the four waves' dW2 / db2 partials are summed through LDS (weight images and tiles are dead) into the workgroup's slab
        constexpr int CH = 16 * K::M2T, SW = CH * FC + CH;
        __syncthreads();
        float* const sw = smem + wave * SW;
#pragma unroll
        for (int m = 0; m < K::M1T; ++m)
#pragma unroll
            for (int m2 = 0; m2 < K::M2T; ++m2)
#pragma unroll
                for (int r = 0; r < 4; ++r) sw[(16 * m2 + 4 * g + r) * FC + 16 * m + ci] = w2acc[m][m2][r];
#pragma unroll
        for (int m2 = 0; m2 < K::M2T; ++m2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = b2acc[m2][r];
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) v += __shfl_xor(v, d);
                if (ci == 0) sw[CH * FC + 16 * m2 + 4 * g + r] = v;
            }
        __syncthreads();
        // SL: the slab has the full layer's layout [C x fcw | C]; the caller's gw2_ws points at this slice's first column, db2 is the first slice's
        const int fcw = SL ? (a.w2_ld ? a.w2_ld : fc) : fc;
        float* const slab = a.gw2_ws + (size_t)blockIdx.x * ((size_t)C * fcw + C);
        for (int i = tid; i < C * fc; i += kThreads) {
            const int ch = i / fc, hid = i - ch * fc, o = ch * FC + hid;
            slab[SL ? ch * fcw + hid : i] = (smem[o] + smem[SW + o]) + (smem[2 * SW + o] + smem[3 * SW + o]);
        }
        if (tid < C && !(SL && ACC)) {
            const int o = CH * FC + tid;
            slab[(size_t)C * fcw + tid] = (smem[o] + smem[SW + o]) + (smem[2 * SW + o] + smem[3 * SW + o]);
        }
    }
}
// ---- the launcher: LDS bytes, grid and workgroups per CU follow from the variant ------------------------------------------------
// One function (hence one attribute cache) per kernel instantiation: the VEC and the any-shape kernel have the same function-pointer
// type, so a cache keyed on that type would be shared between them.
template <int CP, int FC, bool HAS_COND, typename V, bool VEC>
hipError_t launch_dynca(const NcaDyncaArgs& a, hipStream_t st) {
    constexpr int TH = 8, TW = 32;               // (C = 32 ran two rows per pass while it was compiled for 256 registers)
    constexpr int NT = V::BWD ? 2 : 4;           // backward: two 16-cell groups per pass: 2 workgroups per CU at C <= 16 (registers and LDS)
    using K = DyncaCfg<CP, FC, HAS_COND, TH, TW, NT, V::BF>;
    // two-scale: the coarse perception tile follows the variant's own carve (forward: K::OFF_PC; backward: after the dW2 tiles)
    // (the bf16-MFMA backward keeps its W1^T image, FC / 32 * CP / 4 entries of 1 KiB, behind all of that)
    constexpr int LDS_FLOATS = V::BWD ? (V::W2F ? K::LDS_FLOATS_BWD_W2 : K::LDS_FLOATS_BWD) + (V::MS ? 4 * CP * K::PCS : 0) +
                                            ((V::BWD && V::BF) ? (FC / 32) * (CP / 4) * 256 : 0)
                                      : (V::MS ? K::LDS_FLOATS_MS : K::LDS_FLOATS);
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
    static_assert(!V::W2F || 4 * (16 * K::M2T * FC + 16 * K::M2T) <= K::LDS_FLOATS_BWD_W2, "the four waves' dW2 | db2 partials are summed through LDS");
    auto kern = dynca_step_fwd_kernel<CP, FC, HAS_COND, TH, TW, NT, VEC, V>;
    constexpr size_t kDirBytes = V::STEER ? (size_t)K::DR_FLOATS * sizeof(float) : 0;   // steered: the tile's directions behind the carve
    static_assert((size_t)LDS_FLOATS * 4 + kDirBytes <= 160 * 1024, "LDS budget of the steered variant");
    if (V::STEER && !a.dirs) return hipErrorInvalidValue;
    const size_t lds = (size_t)LDS_FLOATS * sizeof(float) + kDirBytes;
    static NcaLdsAttr attr;   // per instantiation; keyed by device inside
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(kern), lds); e != hipSuccess) return e;
    int grid;
    if constexpr (V::BWD) {   // the functions the caller sized the dW2 slabs with: one workgroup per CU two-scale (the coarse tile is in LDS) and at C > 16
        grid = V::MS ? nca_dynca_bwd_ms_grid(a.B, a.H, a.W) : nca_dynca_bwd_grid_c(a.B, a.C, a.H, a.W);
    } else {
        const int ntiles = a.B * ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
        grid = grid_for(ntiles, (!V::MS && lds * 2 <= 160 * 1024) ? 2 : 1);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, st, a);
    return hipGetLastError();
}

// ---- the dispatch ladder: smallest class covering (C, fc); padding lanes carry zero weights ---------------------------------------
// Shape classes (CP, FC), smallest first.  FIRST .. LAST are the classes the caller's variant exists in; a shape none of them covers
// is hipErrorInvalidValue.
enum { kDynca12x96 = 0, kDynca16x128 = 1, kDynca32x128 = 2 };

template <int CP, int FC, typename V>
hipError_t launch_dynca_class(const NcaDyncaArgs& a, hipStream_t st) {
    // 16-byte row loads (bf16 storage: 8-byte) need W % 4 == 0 and an aligned first plane.  The forward variants also test H W % 4 == 0
    // (every plane aligned), which W % 4 == 0 already implies.
    bool vec = (a.W % 4 == 0) && (((uintptr_t)a.x_in & (V::B16 ? 7u : 15u)) == 0);
    if (!V::BWD) vec = vec && (((size_t)a.H * a.W) % 4 == 0);
    if (a.c_cond > 0) return vec ? launch_dynca<CP, FC, true, V, true>(a, st) : launch_dynca<CP, FC, true, V, false>(a, st);
    return vec ? launch_dynca<CP, FC, false, V, true>(a, st) : launch_dynca<CP, FC, false, V, false>(a, st);
}

template <typename V, int FIRST, int LAST>
hipError_t dispatch_dynca(const NcaDyncaArgs& a, hipStream_t st) {
    if constexpr (FIRST <= kDynca12x96 && kDynca12x96 <= LAST)
        if (a.C <= 12 && a.fc <= 96) return launch_dynca_class<12, 96, V>(a, st);
    if constexpr (FIRST <= kDynca16x128 && kDynca16x128 <= LAST)
        if (a.C <= 16 && a.fc <= 128) return launch_dynca_class<16, 128, V>(a, st);   // the shipped video models: C = 12 / fc = 96 and C = 16 / fc = 128
    if constexpr (FIRST <= kDynca32x128 && kDynca32x128 <= LAST)
        if (a.C <= 32 && a.fc <= 128) return launch_dynca_class<32, 128, V>(a, st);   // configs[4]
    return hipErrorInvalidValue;
}

// ---- the forward ladder (nca_dynca_fwd.hip: the variants as they are; nca_dynca_steer.hip: DyncaSteered<> of each) ------------------
template <bool STEER, class V>
using DyncaSel = std::conditional_t<STEER, DyncaSteered<V>, V>;

template <bool STEER>
hipError_t launch_dynca_fwd_ladder(const NcaDyncaArgs& a, hipStream_t st, bool bf16_mfma) {
    const bool bf = bf16_mfma && nca_dynca_bf16_shape_ok(a.C, a.fc);   // ncahip_dynca_precision mode 1; shapes outside its range run exactly
    if (a.pc) {   // two-scale perception
        if ((a.H | a.W) & 1) return hipErrorInvalidValue;
        return bf ? dispatch_dynca<DyncaSel<STEER, DyncaFwdMsBf>, kDynca12x96, kDynca16x128>(a, st)
                  : dispatch_dynca<DyncaSel<STEER, DyncaFwdMs>, kDynca12x96, kDynca16x128>(a, st);
    }
    if (bf) return dispatch_dynca<DyncaSel<STEER, DyncaFwdBf>, kDynca12x96, kDynca16x128>(a, st);
    if (a.fc <= 128) return dispatch_dynca<DyncaSel<STEER, DyncaFwd>, kDynca12x96, kDynca32x128>(a, st);
    if (a.C > 32) return hipErrorInvalidValue;
    // fc > 128: the A-operand image of w1 no longer fits the LDS beside the tile.  w2 relu(w1 y + b1) is a sum over hidden
    // units, so the step runs as one launch per 128-wide slice: the first writes x + mask*(slice + b2), the others add
    // their slice to x_out (same mask: same explicit uniforms / Philox key).  Each launch recomputes the perception (steered: every
    // slice steers it).
    const int K1 = 4 * a.C + a.c_cond;
    for (int h0 = 0; h0 < a.fc; h0 += 128) {
        NcaDyncaArgs s = a;
        s.w1 = a.w1 + (size_t)h0 * K1;
        s.b1 = a.b1 + h0;
        s.w2 = a.w2 + h0;
        s.fc = a.fc - h0 < 128 ? a.fc - h0 : 128;
        s.w2_ld = a.fc;
        const hipError_t e = h0 == 0 ? dispatch_dynca<DyncaSel<STEER, DyncaFwd>, kDynca16x128, kDynca32x128>(s, st)
                                     : dispatch_dynca<DyncaSel<STEER, DyncaFwdAcc>, kDynca16x128, kDynca32x128>(s, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

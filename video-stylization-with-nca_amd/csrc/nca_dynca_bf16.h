// nca_dynca_bf16.h -- the bf16-MFMA UpdateNet of the DyNCA forward step (ncahip_dynca_precision mode 1; contract: include/ncahip.h).
// What fixes the bits of that mode lives here and is shared by the per-step kernel (nca_dynca_step.h) and the two persistent
// kernels (nca_dynca_persist.hip): the k order of both products (folded into the LDS weight images), the operand roundings and the
// MFMA sequence per accumulator.  The weight images exist once.  The layer-1 operand packing and MFMA sequence exist TWICE: inside mlp
// (every forward kernel of the narrow range) and as pack_y / layer1 (the bf16-MFMA backward, and mlp_wide), see the note at layer1; test_gpu_dynca_train_bf16.py compares
// the two on the device at both shape classes, with and without conditioning.  The narrow range is C <= 16 (one 16-row output tile)
// and fc <= 128; the wide range (ncahip_dynca_bf16_range 1: the forward per-step kernels, mlp_wide, nca_dynca_bf16_wide.hip; and the sliced
// backward of the training mode, nca_dynca_bwd_bf16_wide.hip, see w2tw_src) is C <= 32 (two output tiles) and fc <= 256.  fc is a multiple
// of 32 after padding.
//
// k order.  v_mfma_f32_16x16x32_bf16 takes eight k values per lane: lane (g, i) supplies k = 8g + j, j = 0..7.
//   layer 1: lane (g, cell) holds y slots s = 0..K1S-1 (s = 4c'+f < CP: channel 4c'+g, filter f; s = CP: conditioning channel g) --
//            the per-step kernel's perception registers.  Chunk q takes slots 8q..8q+7, zero beyond K1S: K1Q = ceil(K1S / 8) MFMAs per
//            16 hidden units instead of K1S.
//   layer 2: the accumulator registers r = 0..3 of hidden tile m are hidden units 16m + 4g + r of the lane's cell.  Pair p takes
//            tiles 2p and 2p+1: j = 4 (m & 1) + r  <->  hidden 16 (2p + j / 4) + 4g + j % 4: FC / 32 MFMAs instead of FC / 4.
//   two output tiles (the wide range, CP = 32): output tile t holds channels 16t + 4g + r in register r.  Layer 1 is the same product
//            with K1S up to 33 slots (K1Q up to 5 chunks, ascending; the conditioning slot alone in the last chunk).  Layer 2 forms
//            both tiles from the SAME operand: per pair p = 0..FC/32-1 in ascending order, one MFMA per tile t (t = 0, then t = 1) with
//            the W2 entry [t][p], whose k order is the one above.  Each accumulator therefore sums b2, then pairs 0, 1, .. in that
//            order, whatever the other tile does.  W2 image of the wide range: [out tile t][pair p][lane] (w2w_src).
// Image layout: 16-byte entries [tile][chunk | pair][lane], eight bf16 each; as 32-bit words idx = (entry * 64 + lane) * 4 + jj with
// word jj = (j = 2jj in the low half, j = 2jj + 1 in the high half).
#pragma once
#include "nca_common.h"

template <int CP, int FC, bool HAS_COND>
struct NcaDyncaBf16 {
    static constexpr int K1S = CP + (HAS_COND ? 1 : 0);
    static constexpr int K1Q = (K1S + 7) / 8;       // layer-1 MFMAs per hidden tile
    static constexpr int M1T = FC / 16, M1P = FC / 32;
    static constexpr int W1_WORDS = M1T * K1Q * 256, W2_WORDS = M1P * 256;   // 32-bit words (= floats of LDS)
    static_assert(CP % 4 == 0 && CP <= 32 && FC % 32 == 0 && FC <= 256, "bf16 UpdateNet: C <= 32, fc <= 256 padded to a multiple of 32");

    // source element in w1 [fc][K1 = 4C + CC] of half `hf` of image word idx, or -1 (zero padding)
    static __device__ __forceinline__ long w1_src(int idx, int hf, int C, int CC, int fc) {
        const int jj = idx & 3, l = (idx >> 2) & 63, q = (idx >> 8) % K1Q, m = (idx >> 8) / K1Q;
        const int s = 8 * q + 2 * jj + hf, gg = l >> 4, o = 16 * m + (l & 15), K1 = 4 * C + CC;
        if (o >= fc) return -1;
        if (s < CP) {   // blocked [x|Sx|Sy|L], dynca.py:92-95
            const int ch = (s & ~3) + gg;
            return ch < C ? (long)o * K1 + (s & 3) * C + ch : -1;
        }
        return (HAS_COND && s == CP && gg < CC) ? (long)o * K1 + 4 * C + gg : -1;
    }
    // source element in w2 [C][fc]
    static __device__ __forceinline__ long w2_src(int idx, int hf, int C, int fc) {
        const int jj = idx & 3, l = (idx >> 2) & 63, p = idx >> 8;
        const int j = 2 * jj + hf, gg = l >> 4, o = l & 15, k = 16 * (2 * p + (j >> 2)) + 4 * gg + (j & 3);
        return (o < C && k < fc) ? (long)o * fc + k : -1;
    }

    // the layer-1 B operands of NT groups: y slots 8q .. 8q+7 of chunk q rounded to bf16 (RNE), zero beyond K1S
    template <int NT>
    static __device__ __forceinline__ void pack_y(const float (&P)[NT][K1S], nca_u32x4 (&PB)[NT][K1Q]) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < K1Q; ++q)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int s = 8 * q + 2 * jj;
                    PB[n][q][jj] = nca_pk_bf16(s < K1S ? P[n][s < K1S ? s : 0] : 0.0f, s + 1 < K1S ? P[n][s + 1 < K1S ? s + 1 : 0] : 0.0f);
                }
    }
    // acc1 = b1 + W1 PB of hidden tile m (register r: hidden unit 16m + 4g + r of the lane's cell), chunks in ascending order.
    // pack_y and layer1 are the operand packing and the per-accumulator MFMA sequence of mlp below, as functions, for the bf16-MFMA
    // backward (nca_dynca_step.h): its pre-activation has the forward's bits, hence the forward's gate.  mlp keeps its own text: written
    // through these two, the forward kernels were scheduled differently (their instruction streams are held fixed).  Change all three
    // together; test_gpu_dynca_train_bf16.py (gate test) compares the two on the device.
    template <int NT>
    static __device__ __forceinline__ void layer1(const nca_u32x4* W1B, const float* B1L, int m, int g, const nca_u32x4 (&PB)[NT][K1Q],
                                                  f32x4 (&acc1)[NT]) {
        const f32x4 bias1 = *reinterpret_cast<const f32x4*>(B1L + 16 * m + 4 * g);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc1[n] = bias1;
#pragma unroll
        for (int q = 0; q < K1Q; ++q) {
            const nca_u32x4 wa = W1B[(m * K1Q + q) * 64];
#pragma unroll
            for (int n = 0; n < NT; ++n) acc1[n] = nca_mfma_bf16(wa, PB[n][q], acc1[n]);
        }
    }

    // acc2 = b2 + W2 bf16(relu(b1 + W1 bf16(P))) for NT groups of 16 cells; fp32 accumulation, biases as initial values
    template <int NT>
    static __device__ __forceinline__ void mlp(const float* W1L, const float* W2L, const float* B1L, const float* B2L,
                                               const float (&P)[NT][K1S], int lane, int g, f32x4 (&acc2)[NT]) {
        const nca_u32x4* const W1B = reinterpret_cast<const nca_u32x4*>(W1L) + lane;
        const nca_u32x4* const W2B = reinterpret_cast<const nca_u32x4*>(W2L) + lane;
        {
            const f32x4 bias = *reinterpret_cast<const f32x4*>(B2L + 4 * g);
#pragma unroll
            for (int n = 0; n < NT; ++n) acc2[n] = bias;
        }
        nca_u32x4 PB[NT][K1Q];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < K1Q; ++q)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int s = 8 * q + 2 * jj;
                    PB[n][q][jj] = nca_pk_bf16(s < K1S ? P[n][s < K1S ? s : 0] : 0.0f, s + 1 < K1S ? P[n][s + 1 < K1S ? s + 1 : 0] : 0.0f);
                }
#pragma unroll
        for (int p = 0; p < M1P; ++p) {
            nca_u32x4 hb[NT];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int m = 2 * p + hf;
                const f32x4 bias1 = *reinterpret_cast<const f32x4*>(B1L + 16 * m + 4 * g);
                f32x4 acc1[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) acc1[n] = bias1;
#pragma unroll
                for (int q = 0; q < K1Q; ++q) {
                    const nca_u32x4 wa = W1B[(m * K1Q + q) * 64];
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc1[n] = nca_mfma_bf16(wa, PB[n][q], acc1[n]);
                }
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    float h[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] = __int_as_float(max(__float_as_int(acc1[n][r]), 0));   // relu
                    hb[n][2 * hf] = nca_pk_bf16(h[0], h[1]);
                    hb[n][2 * hf + 1] = nca_pk_bf16(h[2], h[3]);
                }
            }
            const nca_u32x4 wb = W2B[p * 64];
#pragma unroll
            for (int n = 0; n < NT; ++n) acc2[n] = nca_mfma_bf16(wb, hb[n], acc2[n]);
        }
    }

    // ---- the wide range (ncahip_dynca_bf16_range 1): C <= 32, fc <= 256 in ONE launch -------------------------------------------------
    // M2T = ceil(CP / 16) output tiles.  The W1 image is the one above (up to 16 tiles x 5 chunks); the W2 image gains the output tile
    // as its slowest index: entry [t][p][lane], lane (g, i), j  <->  W2[ch = 16t + i][hidden 16 (2p + j / 4) + 4g + j % 4].
    static constexpr int M2T = (CP + 15) / 16;
    static constexpr int W2W_WORDS = M2T * M1P * 256;
    static __device__ __forceinline__ long w2w_src(int idx, int hf, int C, int fc) {
        const int jj = idx & 3, l = (idx >> 2) & 63, e = idx >> 8, p = e % M1P, t = e / M1P;
        const int j = 2 * jj + hf, gg = l >> 4, o = 16 * t + (l & 15), k = 16 * (2 * p + (j >> 2)) + 4 * gg + (j & 3);
        return (o < C && k < fc) ? (long)o * fc + k : -1;
    }
    // acc2[t] = b2[16t ..] + W2[16t ..] bf16(relu(b1 + W1 bf16(P))) for NT groups of 16 cells and both output tiles; fp32 accumulation,
    // biases as initial values.  Layer 1 is streamed pair by pair (pack_y / layer1: the sequence of mlp) into the layer-2 accumulators:
    // the hidden activations of a pair live in NT registers of four words and nowhere else.  A function of its own: mlp's instruction
    // streams are held fixed (see the note at layer1).
    template <int NT>
    static __device__ __forceinline__ void mlp_wide(const float* W1L, const float* W2L, const float* B1L, const float* B2L,
                                                    const float (&P)[NT][K1S], int lane, int g, f32x4 (&acc2)[M2T][NT]) {
        const nca_u32x4* const W1B = reinterpret_cast<const nca_u32x4*>(W1L) + lane;
        const nca_u32x4* const W2B = reinterpret_cast<const nca_u32x4*>(W2L) + lane;
#pragma unroll
        for (int t = 0; t < M2T; ++t) {
            const f32x4 bias = *reinterpret_cast<const f32x4*>(B2L + 16 * t + 4 * g);
#pragma unroll
            for (int n = 0; n < NT; ++n) acc2[t][n] = bias;
        }
        nca_u32x4 PB[NT][K1Q];
        pack_y<NT>(P, PB);
#pragma unroll
        for (int p = 0; p < M1P; ++p) {
            nca_u32x4 hb[NT];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                f32x4 acc1[NT];
                layer1<NT>(W1B, B1L, 2 * p + hf, g, PB, acc1);
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    float h[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) h[r] = __int_as_float(max(__float_as_int(acc1[n][r]), 0));   // relu
                    hb[n][2 * hf] = nca_pk_bf16(h[0], h[1]);
                    hb[n][2 * hf + 1] = nca_pk_bf16(h[2], h[3]);
                }
            }
#pragma unroll
            for (int t = 0; t < M2T; ++t) {
                const nca_u32x4 wb = W2B[(t * M1P + p) * 64];
#pragma unroll
                for (int n = 0; n < NT; ++n) acc2[t][n] = nca_mfma_bf16(wb, hb[n], acc2[t][n]);
            }
        }
    }

    // ---- the bf16-MFMA backward (the "bf16-MFMA training" mode of include/ncahip.h): two transposed weight images -----------------
    //   dh = W2b^T gb on v_mfma_f32_16x16x16_bf16 (K = the 16 channel slots, four k per lane: k = 4g + j).  Image [tile m][lane] of
    //        8 bytes: lane (g, i), j  <->  W2[ch = 4g + j][hidden 16m + i]; as words idx = (m * 64 + lane) * 2 + jj.
    //   dL/dy = W1b^T dhb on v_mfma_f32_16x16x32_bf16, K = the hidden units in the pair order of the forward's layer 2 (k = 8g + j  <->
    //        hidden 16 (2p + j / 4) + 4g + j % 4: the operand is two consecutive dh accumulator tiles as they stand).  Output tile mj,
    //        row i  <->  channel 4mj + (i & 3), filter i >> 2.  Image [pair p][tile mj][lane] of 16 bytes.
    static constexpr int MJ = CP / 4;
    static constexpr int W2T_WORDS = M1T * 128, W1T_WORDS = M1P * MJ * 256;
    static __device__ __forceinline__ long w2t_src(int idx, int hf, int C, int fc) {
        const int jj = idx & 1, l = (idx >> 1) & 63, m = idx >> 7;
        const int ch = 4 * (l >> 4) + 2 * jj + hf, k = 16 * m + (l & 15);
        return (ch < C && k < fc) ? (long)ch * fc + k : -1;
    }
    // The wide range of that backward (nca_dynca_bwd_bf16_wide.hip) takes the hidden layer in 128-wide slices at the FORWARD's channel
    // class: w1_src / w1t_src / pack_y / layer1 above on the slice's rows of w1 and b1 (K1S, K1Q and the chunk order depend on CP and
    // the conditioning alone, so a slice's a1 has the bits the forward's <CP, 256> class gives those hidden units).  W2^T of a slice
    // with M2T channel tiles: image [tile m][channel tile t][lane] of 8 bytes, lane (g, i), j  <->  W2[ch = 16t + 4g + j][hidden 16m + i],
    // rows `ld` apart (the full layer's fc); words idx = ((m * M2T + t) * 64 + lane) * 2 + jj.  dh sums the tiles in the order t = 0, 1.
    static __device__ __forceinline__ long w2tw_src(int idx, int hf, int C, int fc, int ld) {
        const int jj = idx & 1, l = (idx >> 1) & 63, e = idx >> 7, t = e % M2T, m = e / M2T;
        const int ch = 16 * t + 4 * (l >> 4) + 2 * jj + hf, k = 16 * m + (l & 15);
        return (ch < C && k < fc) ? (long)ch * ld + k : -1;
    }
    static __device__ __forceinline__ long w1t_src(int idx, int hf, int C, int CC, int fc) {
        const int jj = idx & 3, l = (idx >> 2) & 63, e = idx >> 8, mj = e % MJ, p = e / MJ;
        const int j = 2 * jj + hf, i = l & 15, k = 16 * (2 * p + (j >> 2)) + 4 * (l >> 4) + (j & 3), ch = 4 * mj + (i & 3);
        return (k < fc && ch < C) ? (long)k * (4 * C + CC) + (i >> 2) * C + ch : -1;
    }
};

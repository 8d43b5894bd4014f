// nca_cond_bf16.hip -- bf16 state storage for the ConditionedNCA step (gfx950): finalize kernel, the finalize + image kernel of the clip
// driver, and entry points.
//
// The fused step itself is the producer/consumer kernel of nca_cond_pc.hip instantiated with StBF16 (see the rounding
// points there and in include/ncahip.h): state and goal encoding travel as bf16 (90 B/cell at C=16 instead of 178), the
// UpdateNet runs on v_mfma_f32_16x16x16_bf16 with f32 accumulation.  A first, symmetric wave-private bf16 kernel (every
// wave staging and computing its own tile, 2 waves per SIMD) was latency-bound at 74.6 us/step on the bench grid -- the
// bf16 MFMA is cheap, the dependent LDS / global round trips of the staging are not -- which is why the staging runs in
// its own waves one tile ahead here as well.
// Requires W % 4 == 0 and 8-byte aligned tensors (no any-shape bf16 kernel: the entry points refuse other shapes).
#include "nca_cond_tile.h"
#include "nca_clip_unit.h"
#include "nca_yuv.h"

namespace {

__device__ __forceinline__ unsigned pk_bf16_(float lo, float hi) { return StBF16::pk2(lo, hi); }

// x_out = bf16(clamp(x_pend * (pre & alive(x_pend)), lo, hi)): every operation is exact on bf16 values
__global__ __launch_bounds__(256) void cond_finalize_bf16_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ pre,
                                                                 uint16_t* __restrict__ out, int B, int C, int H, int W,
                                                                 int alive_ch, float thr, float lo, float hi) {
    const size_t plane = (size_t)H * W;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)B * plane) return;
    const int xx = (int)(id % W), yy = (int)((id / W) % H), b = (int)(id / plane);
    const uint16_t* const xb = x + (size_t)b * C * plane;
    auto f = [](uint16_t v) { return __uint_as_float((unsigned)v << 16); };
    float life = 1.0f;
    if (alive_ch >= 0) {
        const uint16_t* const ap = xb + (size_t)alive_ch * plane;
        float m = NCA_NEG_INF;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int y2 = yy + dy, x2 = xx + dx;
                if (y2 >= 0 && y2 < H && x2 >= 0 && x2 < W) m = fmaxf(m, f(ap[(size_t)y2 * W + x2]));
            }
        life = (pre[id] != 0 && m > thr) ? 1.0f : 0.0f;
    }
    const size_t off = (size_t)yy * W + xx;
    uint16_t* const ob = out + (size_t)b * C * plane + off;
    for (int c = 0; c < C; ++c) {
        const float v = fminf(fmaxf(f(xb[(size_t)c * plane + off]) * life, lo), hi);
        ob[(size_t)c * plane] = (uint16_t)(pk_bf16_(v, 0.0f) & 0xffffu);
    }
}

// ---- finalize + image in one pass (the clip driver's last launch per image) --------------------------------------------------------
// What cond_finalize_bf16_kernel and then the unit emit of nca_clip.hip on its result do, without the second read of the state: a lane
// owns ROWS x 4 cells (ROWS = 2 for the planar formats: one 4:2:0 block of nca_yuv420_store_block; else 1) of kFinEmitCh consecutive
// channels (blockIdx.y: the channel group), resolves the cells' life mask, writes its resolved channels and -- group 0, which holds
// channels 0..2 -- the image.  The image is made of the bf16 values that were stored, so it is bit for bit the two launches'.  Every
// group resolves the life mask for itself (three or four rows of alpha, a few bytes of pre): that buys C / 4 times the waves of a
// launch that is all latency -- with one lane walking all C channels of its cells, 1 x 20 x 256^2 took 8.4 us against the 6.5 us of
// the two launches.  VEC (wave-uniform): W % 4 == 0 and 8-byte aligned state tensors -- a row's four cells travel as one 8-byte word;
// otherwise cell by cell, columns past the row's end skipped.
constexpr int kFinEmitThreads = 64;   // one wave per workgroup: small grids still reach every CU
constexpr int kFinEmitCh = 4;         // channels per lane (>= 3: the image's channels sit in one group)

__device__ __forceinline__ float widen_bf16(unsigned v) { return __uint_as_float(v << 16); }

// cells x0 .. x0 + 3 of the row at p (p = the address of cell x0), widened; cells at and past nv read as `fill`
__device__ __forceinline__ void fin_load4(const uint16_t* __restrict__ p, int nv, bool vec, float fill, float (&v)[4]) {
    if (vec) {
        const f32x4 f = StBF16::cv4(*reinterpret_cast<const u32x2*>(p));
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = f[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = i < nv ? widen_bf16(p[i]) : fill;
    }
}

template <int FMT>
__global__ __launch_bounds__(kFinEmitThreads) void cond_finalize_emit_bf16_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ pre,
                                                                                  uint16_t* __restrict__ out, void* __restrict__ img, int B, int C,
                                                                                  int H, int W, int alive_ch, float thr, float lo, float hi, int vec,
                                                                                  int img_vec, NcaRgbYuvK k) {
    constexpr int ROWS = FMT >= kImgI420 ? 2 : 1;
    const int bx = (W + 3) / 4, by = H / ROWS;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)B * by * bx) return;
    const int x0 = (int)(id % bx) * 4, y0 = (int)((id / bx) % by) * ROWS;
    const size_t b = id / ((size_t)bx * by), plane = (size_t)H * W;
    const int nv = min(4, W - x0);
    const uint16_t* const xb = x + b * C * plane;
    uint16_t* const ob = out + b * C * plane;
    const int c0 = (int)blockIdx.y * kFinEmitCh;

    float life[ROWS][4];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) life[j][i] = 1.0f;
        if (alive_ch >= 0) {
            const int y = y0 + j;
            const uint16_t* const ap = xb + (size_t)alive_ch * plane;
            float cm[6];   // per column x0 - 1 .. x0 + 4: the maximum over the in-image rows y - 1 .. y + 1
#pragma unroll
            for (int i = 0; i < 6; ++i) cm[i] = NCA_NEG_INF;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int y2 = y + dy;
                if (y2 < 0 || y2 >= H) continue;
                const uint16_t* const row = ap + (size_t)y2 * W + x0;
                float mid[4];
                fin_load4(row, nv, vec != 0, NCA_NEG_INF, mid);
#pragma unroll
                for (int i = 0; i < 4; ++i) cm[i + 1] = fmaxf(cm[i + 1], mid[i]);
                if (x0 > 0) cm[0] = fmaxf(cm[0], widen_bf16(row[-1]));
                if (x0 + 4 < W) cm[5] = fmaxf(cm[5], widen_bf16(row[4]));
            }
            const uint8_t* const pr = pre + b * plane + (size_t)y * W + x0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float m = fmaxf(fmaxf(cm[i], cm[i + 1]), cm[i + 2]);
                life[j][i] = (i < nv && pr[i] != 0 && m > thr) ? 1.0f : 0.0f;
            }
        }
    }

    float rgb[3][ROWS][4];   // group 0: the first three resolved channels, as stored (bf16 values)
    float v[kFinEmitCh][ROWS][4];
#pragma unroll
    for (int cc = 0; cc < kFinEmitCh; ++cc)      // all loads of the lane first
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
            if (c0 + cc < C) fin_load4(xb + (size_t)(c0 + cc) * plane + (size_t)(y0 + j) * W + x0, nv, vec != 0, 0.0f, v[cc][j]);
#pragma unroll
    for (int cc = 0; cc < kFinEmitCh; ++cc) {
        if (c0 + cc >= C) break;
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const size_t off = (size_t)(c0 + cc) * plane + (size_t)(y0 + j) * W + x0;
            unsigned bits[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bits[i] = pk_bf16_(fminf(fmaxf(v[cc][j][i] * life[j][i], lo), hi), 0.0f) & 0xffffu;
            if (vec) {
                *reinterpret_cast<u32x2*>(ob + off) = u32x2{bits[0] | bits[1] << 16, bits[2] | bits[3] << 16};
            } else {
                for (int i = 0; i < nv; ++i) ob[off + i] = (uint16_t)bits[i];
            }
            if (cc < 3) {
#pragma unroll
                for (int i = 0; i < 4; ++i) rgb[cc][j][i] = clip_unit_value(widen_bf16(bits[i]));
            }
        }
    }
    if (c0 != 0) return;     // the image is group 0's (C >= 3: channels 0..2 are all there)

    if constexpr (FMT == kImgF32) {          // [B,3,H,W] float32
        float* const o = static_cast<float*>(img) + b * 3 * plane + (size_t)y0 * W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (img_vec) {
                *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{rgb[c][0][0], rgb[c][0][1], rgb[c][0][2], rgb[c][0][3]};
            } else {
                for (int i = 0; i < nv; ++i) o[c * plane + i] = rgb[c][0][i];
            }
        }
    } else if constexpr (FMT == kImgU8) {    // [B,H,W,3] uint8 = (uint8_t)(img * 255.0f), truncating: the bytes of clip_emit_u8_kernel
        unsigned char px[12];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[i * 3 + c] = (unsigned char)__fmul_rn(rgb[c][0][i], 255.0f);
        unsigned char* const o = static_cast<unsigned char*>(img) + (b * plane + (size_t)y0 * W + x0) * 3;
        if (img_vec) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
                reinterpret_cast<unsigned*>(o)[d] = (unsigned)px[4 * d] | (unsigned)px[4 * d + 1] << 8 | (unsigned)px[4 * d + 2] << 16 | (unsigned)px[4 * d + 3] << 24;
        } else {
            for (int i = 0; i < nv * 3; ++i) o[i] = px[i];
        }
    } else {                       // planar YUV 4:2:0 [B,3H/2,W] of those bytes (H, W even: nv is 2 or 4)
        int p8[3][2][kYuvOutCols];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) p8[c][j][i] = (int)(unsigned char)__fmul_rn(rgb[c][j][i], 255.0f);
        nca_yuv420_store_block<FMT == kImgNV12>(static_cast<unsigned char*>(img), k, b, H, W, y0, x0, nv, p8[0], p8[1], p8[2]);
    }
}

}  // namespace

hipError_t nca_launch_cond_finalize_emit_bf16(const uint16_t* x, const uint8_t* pre, uint16_t* out, void* img, const NcaImgOut& io, int B, int C, int H,
                                              int W, int alive_ch, float thr, float lo, float hi, hipStream_t st) {
    const int fmt = io.kind;
    if (!img || C < 3 || fmt < kImgF32 || fmt > kImgNV12 || (io.planar() && ((H | W) & 1))) return hipErrorInvalidValue;
    const int rows = io.planar() ? 2 : 1;
    const size_t lanes = (size_t)B * (H / rows) * ((W + 3) / 4), blocks = (lanes + kFinEmitThreads - 1) / kFinEmitThreads;
    if (blocks == 0 || blocks > 0x7fffffffu || C > 65535 * kFinEmitCh) return hipErrorInvalidValue;
    const int vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 7) == 0;
    const int img_vec = W % 4 == 0 && ((uintptr_t)img & (fmt == kImgF32 ? 15 : 3)) == 0;
    const int32_t* const k = io.k;   // zero unless planar
    const NcaRgbYuvK yk{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9]};
    const dim3 grid((unsigned)blocks, (unsigned)((C + kFinEmitCh - 1) / kFinEmitCh)), blk(kFinEmitThreads);
    switch (fmt) {
        case kImgF32: hipLaunchKernelGGL(cond_finalize_emit_bf16_kernel<kImgF32>, grid, blk, 0, st, x, pre, out, img, B, C, H, W, alive_ch, thr, lo, hi, vec, img_vec, yk); break;
        case kImgU8: hipLaunchKernelGGL(cond_finalize_emit_bf16_kernel<kImgU8>, grid, blk, 0, st, x, pre, out, img, B, C, H, W, alive_ch, thr, lo, hi, vec, img_vec, yk); break;
        case kImgI420: hipLaunchKernelGGL(cond_finalize_emit_bf16_kernel<kImgI420>, grid, blk, 0, st, x, pre, out, img, B, C, H, W, alive_ch, thr, lo, hi, vec, img_vec, yk); break;
        default: hipLaunchKernelGGL(cond_finalize_emit_bf16_kernel<kImgNV12>, grid, blk, 0, st, x, pre, out, img, B, C, H, W, alive_ch, thr, lo, hi, vec, img_vec, yk); break;
    }
    return hipGetLastError();
}

hipError_t nca_launch_cond_finalize_bf16(const uint16_t* x, const uint8_t* pre, uint16_t* out, int B, int C, int H, int W,
                                         int alive_ch, float thr, float lo, float hi, hipStream_t st) {
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(cond_finalize_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, pre, out, B, C, H, W,
                       alive_ch, thr, lo, hi);
    return hipGetLastError();
}

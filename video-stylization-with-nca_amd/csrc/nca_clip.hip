// nca_clip.hip -- the two ends of clip stylisation (ConditioneDyNCA/utils/misc/video_utils.py:50-83) around the DyNCA steps:
//   clip_cond_kernel   frames of one call -> cond [F,B,3,H,W]: grey, then EdgeExtractor (dynca.py:204-213) in one pass
//   clip_emit_kernel   state [B,C,H,W] -> one output image (video_utils.py:78-81), float32 NCHW or uint8 NHWC
// and, for the models that carry the grey frame as their last state channel (ExtraChannels/utils/misc/video_utils.py:66-82):
//   clip_gray_kernel   frames of one call -> grey [F,B,H,W]
//   the emit kernels with INJ: the image as above and, in the same launch, a grey plane written over state channel C - 1
// and, for a video encoder behind the clip (include/ncahip.h, "planar YUV images"):
//   clip_emit_yuv420_kernel   state -> one planar YUV 4:2:0 image (I420 / NV12), the uint8 image's bytes never leaving the registers
// The three emit kernels also read a ConditionedNCA state stored as bf16 (XT = uint16_t: instantiations of their own; the widening is exact).
#include "nca_kernels.h"
#include "nca_clip_u8.h"
#include "nca_clip_unit.h"
#include "nca_yuv.h"

namespace {

constexpr int kTileW = 64, kTileH = 16;                  // output pixels per workgroup: one wave per 4 rows, one lane per column
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;  // grey tile with its one-cell halo
static_assert(kHaloW <= kClipStageCols, "a halo row must fit the staged row of nca_clip_u8.h");

// uint8 -> network range as the reference's preprocessing (preprocess_texture.py:28, :54): a true division, then v * 2 - 1
__device__ __forceinline__ float clip_widen_u8(unsigned v) {
    const float f = __fdiv_rn((float)v, 255.0f);
    return __fsub_rn(__fmul_rn(f, 2.0f), 1.0f);
}

// grey of pixel (y, x) of image n from the rows clip_stage_u8_rows staged (r: its staged row, cx0: the first staged column)
__device__ __forceinline__ float clip_staged_u8_grey(const unsigned char* base, const unsigned* raw, int r, size_t n, size_t plane, int W, int y,
                                                     int x, int cx0, float wr, float wg, float wb) {
    const unsigned char* const p = clip_staged_u8_pixel(base, raw, r, n, plane, W, y, x, cx0);
    return wr * clip_widen_u8(p[0]) + wg * clip_widen_u8(p[1]) + wb * clip_widen_u8(p[2]);
}

// One workgroup = one 16 x 64 tile of one image.  The grey tile (+ halo, zero outside the image) is staged in LDS, so every input
// pixel is read once per workgroup; a lane then walks 4 output rows of its column keeping the 3 x 3 window rows in registers.
// U8: the halo rows' bytes come in as aligned dwords (4 bytes per lane) and are unpacked from LDS.
template <bool U8>
__global__ __launch_bounds__(256) void clip_cond_kernel(const void* __restrict__ frames, const float* __restrict__ k3, float wr, float wg,
                                                        float wb, int do_tanh, float* __restrict__ cond, int N, int H, int W, int tiles_x,
                                                        int tiles_y) {
    __shared__ float grey[kHaloH][kHaloW + 1];
    __shared__ unsigned raw[U8 ? kHaloH : 1][U8 ? kRawDwords : 1];
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
    const size_t n = blk / ((size_t)tiles_x * tiles_y);   // image index f * B + b
    if (n >= (size_t)N) return;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const size_t plane = (size_t)H * W;
    // columns of the halo tile that lie inside the image: [cx0, cx1) in image coordinates
    const int cx0 = max(x0 - 1, 0), cx1 = min(x0 + kTileW + 1, W);

    if (U8) {
        const unsigned char* const base = static_cast<const unsigned char*>(frames);
        clip_stage_u8_rows<kHaloH>(base, (size_t)N * plane * 3, n, plane, H, W, y0 - 1, cx0, cx1, &raw[0][0], tid);
        __syncthreads();
        for (int i = tid; i < kHaloH * kHaloW; i += 256) {
            const int r = i / kHaloW, c = i % kHaloW;
            const int y = y0 - 1 + r, x = x0 - 1 + c;
            float g = 0.0f;
            if (y >= 0 && y < H && x >= cx0 && x < cx1) g = clip_staged_u8_grey(base, &raw[0][0], r, n, plane, W, y, x, cx0, wr, wg, wb);
            grey[r][c] = g;
        }
    } else {
        const float* const ib = static_cast<const float*>(frames) + n * 3 * plane;
        for (int i = tid; i < kHaloH * kHaloW; i += 256) {
            const int r = i / kHaloW, c = i % kHaloW;
            const int y = y0 - 1 + r, x = x0 - 1 + c;
            float g = 0.0f;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const size_t o = (size_t)y * W + x;
                g = wr * ib[o] + wg * ib[plane + o] + wb * ib[2 * plane + o];
            }
            grey[r][c] = g;
        }
    }
    __syncthreads();

    float k[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) k[i] = k3[i];
    const int col = tid & 63, row0 = (tid >> 6) * 4;
    const int x = x0 + col;
    float w0[3], w1[3], w2[3];   // window rows y - 1, y, y + 1
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        w0[j] = grey[row0][col + j];
        w1[j] = grey[row0 + 1][col + j];
    }
    float* const ob = cond + n * 3 * plane;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = y0 + row0 + r;
#pragma unroll
        for (int j = 0; j < 3; ++j) w2[j] = grey[row0 + r + 2][col + j];
        if (x < W && y < H) {
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                float acc = 0.0f;   // tap order of ncahip_edge_extractor_f32
#pragma unroll
                for (int j = 0; j < 3; ++j) acc = fmaf(k[f * 9 + j], w0[j], acc);
#pragma unroll
                for (int j = 0; j < 3; ++j) acc = fmaf(k[f * 9 + 3 + j], w1[j], acc);
#pragma unroll
                for (int j = 0; j < 3; ++j) acc = fmaf(k[f * 9 + 6 + j], w2[j], acc);
                ob[(size_t)f * plane + (size_t)y * W + x] = do_tanh ? tanhf(acc) : acc;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            w0[j] = w1[j];
            w1[j] = w2[j];
        }
    }
}

// img = (clamp(2 x, -1, 1) + 1) / 2, in the reference's order of operations (NaN passes through, as torch.clamp)
__device__ __forceinline__ float clip_image_value(float x) {
    float v = __fmul_rn(x, 2.0f);
    v = v < -1.0f ? -1.0f : v;
    v = v > 1.0f ? 1.0f : v;
    return __fmul_rn(__fadd_rn(v, 1.0f), 0.5f);
}

// UNIT selects the image definition: false = clip_image_value (the DyNCA families), true = clip_unit_value (ConditionedNCA)
template <bool UNIT>
__device__ __forceinline__ float clip_emit_value(float x) { return UNIT ? clip_unit_value(x) : clip_image_value(x); }

// a state element widened to f32: fp32 as it is; bf16 bits (a ConditionedNCA state stored as bf16) exactly
__device__ __forceinline__ float clip_ld(const float* x, size_t i) { return x[i]; }
__device__ __forceinline__ float clip_ld(const uint16_t* x, size_t i) { return __uint_as_float((unsigned)x[i] << 16); }

// One launch for both halves of the step between two calls of an extra-channel clip: EMIT writes the image of x[:, :c_out] into img,
// INJ copies the plane gray [B,H,W] over channel C - 1 of the same state (xlast = x + (C - 1) * plane; c_out <= C - 1, so the two halves
// touch different channels).  EMIT alone is the image output of the edge family.  XT: the state's element type (clip_ld; uint16_t only without INJ).
template <bool EMIT, bool INJ, bool UNIT = false, typename XT = float>
__global__ __launch_bounds__(256) void clip_emit_f32_kernel(const XT* __restrict__ x, float* __restrict__ img, float* __restrict__ xlast,
                                                            const float* __restrict__ gray, int B, int C, int c_out, size_t plane) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nc = (EMIT ? (size_t)c_out : 0) + (INJ ? 1 : 0);
    if (id >= (size_t)B * nc * plane) return;
    const size_t p = id % plane, c = (id / plane) % nc, b = id / (plane * nc);
    if (INJ && c == nc - 1) xlast[b * C * plane + p] = gray[b * plane + p];
    else img[INJ ? (b * c_out + c) * plane + p : id] = clip_emit_value<UNIT>(clip_ld(x, (b * C + c) * plane + p));
}

// uint8 NHWC: a lane owns 4 consecutive pixels of the flattened [B*H*W] axis = CO dwords, stored whole (bytes only for the last, partial
// group or an output that is not 4-byte aligned).  (uint8_t)(img * 255): truncation, as np.uint8 in VideoWriter.add.  INJ as above, for
// the lane's pixels.
template <int CO, bool INJ, bool UNIT = false, typename XT = float>
__global__ __launch_bounds__(256) void clip_emit_u8_kernel(const XT* __restrict__ x, unsigned char* __restrict__ img, float* __restrict__ xlast,
                                                           const float* __restrict__ gray, int B, int C, size_t plane, int aligned) {
    const size_t grp = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t npix = (size_t)B * plane, q0 = grp * 4;
    if (q0 >= npix) return;
    unsigned char px[4 * CO];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const size_t q = q0 + i < npix ? q0 + i : npix - 1;
        const size_t b = q / plane, p = q % plane;
#pragma unroll
        for (int c = 0; c < CO; ++c) px[i * CO + c] = (unsigned char)__fmul_rn(clip_emit_value<UNIT>(clip_ld(x, (b * C + c) * plane + p)), 255.0f);
        if (INJ && q0 + i < npix) xlast[b * C * plane + p] = gray[q];
    }
    unsigned char* const o = img + q0 * CO;
    if (aligned && q0 + 4 <= npix) {
#pragma unroll
        for (int d = 0; d < CO; ++d)
            reinterpret_cast<unsigned*>(o)[d] = (unsigned)px[4 * d] | (unsigned)px[4 * d + 1] << 8 | (unsigned)px[4 * d + 2] << 16 | (unsigned)px[4 * d + 3] << 24;
    } else {
        const size_t nb = (q0 + 4 <= npix ? 4 : npix - q0) * CO;
        for (size_t i = 0; i < nb; ++i) o[i] = px[i];
    }
}

// Planar YUV 4:2:0 [B,3H/2,W] of the uint8 image above (CO = 3), without that image: a lane owns 2 rows x 4 columns of one sample, reads the
// 4 consecutive floats of each row of the three channels once, truncates them to the bytes clip_emit_u8_kernel stores and hands them to
// nca_yuv420_store_block (nca_yuv.h: a dword of Y per row and the chroma under it; halves or bytes where a plane's phase forces them).  The
// result is bit for bit clip_emit_u8_kernel followed by rgb_to_yuv420_kernel (nca_yuv_out.hip).  INJ as above, for the lane's pixels.
template <bool NV12, bool INJ, bool UNIT, typename XT = float>
__global__ __launch_bounds__(kYuvOutThreads) void clip_emit_yuv420_kernel(const XT* __restrict__ x, unsigned char* __restrict__ img, float* __restrict__ xlast,
                                                               const float* __restrict__ gray, int C, int H, int W, int bx, size_t lanes, NcaRgbYuvK k) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= lanes) return;
    const int x0 = (int)(id % bx) * kYuvOutCols;
    const size_t row = id / bx;                                   // row pair b * H/2 + y/2
    const size_t b = row / (size_t)(H >> 1);
    const int y = (int)(row % (size_t)(H >> 1)) * 2;
    const int nv = min(kYuvOutCols, W - x0);
    const size_t plane = (size_t)H * W;
    int px[3][2][kYuvOutCols];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const XT* const xr = x + (b * C + c) * plane + (size_t)(y + j) * W;
#pragma unroll
            for (int i = 0; i < kYuvOutCols; ++i)      // columns past the row's end repeat its last pixel; nothing of them is stored
                px[c][j][i] = (int)(unsigned char)__fmul_rn(clip_emit_value<UNIT>(clip_ld(xr, (size_t)min(x0 + i, W - 1))), 255.0f);
        }
    if (INJ) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            for (int i = 0; i < nv; ++i) {
                const size_t p = (size_t)(y + j) * W + x0 + i;
                xlast[b * C * plane + p] = gray[b * plane + p];
            }
    }
    nca_yuv420_store_block<NV12>(img, k, b, H, W, y, x0, nv, px[0], px[1], px[2]);
}

// grey [N,H,W] of N = F*B frames, one 16 x 64 tile per workgroup and no halo.  U8: the tile's rows come in through clip_stage_u8_rows, the
// loader of clip_cond_kernel; float32 planes are read in place (every pixel once, coalesced), so no LDS there.
template <bool U8>
__global__ __launch_bounds__(256) void clip_gray_kernel(const void* __restrict__ frames, float wr, float wg, float wb, float* __restrict__ gray,
                                                        int N, int H, int W, int tiles_x, int tiles_y) {
    __shared__ unsigned raw[U8 ? kTileH : 1][U8 ? kRawDwords : 1];
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
    const size_t n = blk / ((size_t)tiles_x * tiles_y);
    if (n >= (size_t)N) return;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const size_t plane = (size_t)H * W;
    const int cx1 = min(x0 + kTileW, W);
    if (U8) {
        clip_stage_u8_rows<kTileH>(static_cast<const unsigned char*>(frames), (size_t)N * plane * 3, n, plane, H, W, y0, x0, cx1, &raw[0][0], tid);
        __syncthreads();
    }
    for (int i = tid; i < kTileH * kTileW; i += 256) {
        const int r = i / kTileW, y = y0 + r, x = x0 + i % kTileW;
        if (y >= H || x >= W) continue;
        const size_t o = (size_t)y * W + x;
        float g;
        if (U8) {
            g = clip_staged_u8_grey(static_cast<const unsigned char*>(frames), &raw[0][0], r, n, plane, W, y, x, x0, wr, wg, wb);
        } else {
            const float* const ib = static_cast<const float*>(frames) + n * 3 * plane;
            g = wr * ib[o] + wg * ib[plane + o] + wb * ib[2 * plane + o];
        }
        gray[n * plane + o] = g;
    }
}

}  // namespace

hipError_t nca_launch_clip_cond(const void* frames, bool u8, const float* k3, float wr, float wg, float wb, int do_tanh, float* cond, int N, int H,
                                int W, hipStream_t st) {
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
    const size_t blocks = (size_t)N * tiles_x * tiles_y;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    if (u8) hipLaunchKernelGGL(clip_cond_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, frames, k3, wr, wg, wb, do_tanh, cond, N, H, W, tiles_x, tiles_y);
    else hipLaunchKernelGGL(clip_cond_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, frames, k3, wr, wg, wb, do_tanh, cond, N, H, W, tiles_x, tiles_y);
    return hipGetLastError();
}

hipError_t nca_launch_clip_gray(const void* frames, bool u8, float wr, float wg, float wb, float* gray, int N, int H, int W, hipStream_t st) {
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
    const size_t blocks = (size_t)N * tiles_x * tiles_y;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    if (u8) hipLaunchKernelGGL(clip_gray_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, frames, wr, wg, wb, gray, N, H, W, tiles_x, tiles_y);
    else hipLaunchKernelGGL(clip_gray_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, frames, wr, wg, wb, gray, N, H, W, tiles_x, tiles_y);
    return hipGetLastError();
}

// the emit kernels of a float32 state: uint8, the DyNCA families' image, by [c_out - 1][inject]; planar by [NV12][inject][unit]
static const decltype(&clip_emit_u8_kernel<1, false>) kClipEmitU8[4][2] = {
    {clip_emit_u8_kernel<1, false>, clip_emit_u8_kernel<1, true>}, {clip_emit_u8_kernel<2, false>, clip_emit_u8_kernel<2, true>},
    {clip_emit_u8_kernel<3, false>, clip_emit_u8_kernel<3, true>}, {clip_emit_u8_kernel<4, false>, clip_emit_u8_kernel<4, true>}};
static const decltype(&clip_emit_yuv420_kernel<false, false, false>) kClipEmitYuv420[2][2][2] = {
    {{clip_emit_yuv420_kernel<false, false, false>, clip_emit_yuv420_kernel<false, false, true>},
     {clip_emit_yuv420_kernel<false, true, false>, clip_emit_yuv420_kernel<false, true, true>}},
    {{clip_emit_yuv420_kernel<true, false, false>, clip_emit_yuv420_kernel<true, false, true>},
     {clip_emit_yuv420_kernel<true, true, false>, clip_emit_yuv420_kernel<true, true, true>}}};

// One image out of a state and, with gray, the inject of the same launch (nca_kernels.h).  A lane owns an element (float32 image, or no
// image), four pixels (uint8; `aligned`: the image is 4-byte aligned) or a 2 x kYuvOutCols block (planar).
hipError_t nca_launch_clip_emit(const NcaClipEmitArgs& a, hipStream_t st) {
    const int B = a.B, C = a.C, H = a.H, W = a.W;
    const bool inj = a.gray != nullptr, planar = a.img && a.out.planar();
    if ((!a.img && !inj) || a.c_out < 1 || a.c_out > 4 || (inj && (a.unit || a.c_out > C - 1))) return hipErrorInvalidValue;
    if ((a.unit || planar) && (C < 3 || a.c_out != 3)) return hipErrorInvalidValue;
    if ((planar && ((H | W) & 1)) || (a.bf16 && !a.unit)) return hipErrorInvalidValue;
    const size_t plane = (size_t)H * W;
    float* const x = (float*)a.state;
    const uint16_t* const xh = (const uint16_t*)a.state;   // a.bf16
    float* const xlast = inj ? x + (size_t)(C - 1) * plane : nullptr;
    if (planar) {
        const int32_t* const k = a.out.k;
        const NcaRgbYuvK yk{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9]};
        const int bx = (W + kYuvOutCols - 1) / kYuvOutCols;
        const size_t lanes = (size_t)B * (H / 2) * bx, blocks = (lanes + kYuvOutThreads - 1) / kYuvOutThreads;
        if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
        const bool nv12 = a.out.kind == kImgNV12;
        auto go = [&](auto kernel, auto* xs) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kYuvOutThreads), 0, st, xs, (unsigned char*)a.img, xlast, a.gray, C, H, W, bx, lanes, yk);
        };
        if (a.bf16) go(nv12 ? clip_emit_yuv420_kernel<true, false, true, uint16_t> : clip_emit_yuv420_kernel<false, false, true, uint16_t>, xh);
        else go(kClipEmitYuv420[nv12][inj][a.unit], x);
    } else if (!a.img || a.out.kind == kImgF32) {
        const size_t n = (size_t)B * ((a.img ? a.c_out : 0) + (inj ? 1 : 0)) * plane;
        auto go = [&](auto kernel, auto* xs) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xs, (float*)a.img, xlast, a.gray, B, C, a.c_out, plane);
        };
        if (a.bf16) go(clip_emit_f32_kernel<true, false, true, uint16_t>, xh);
        else if (a.unit) go(clip_emit_f32_kernel<true, false, true, float>, x);
        else go(!a.img ? clip_emit_f32_kernel<false, true> : inj ? clip_emit_f32_kernel<true, true> : clip_emit_f32_kernel<true, false>, x);
    } else {
        const size_t groups = ((size_t)B * plane + 3) / 4;
        const int aligned = ((uintptr_t)a.img & 3) == 0;
        auto go = [&](auto kernel, auto* xs) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, xs, (unsigned char*)a.img, xlast, a.gray, B, C, plane, aligned);
        };
        if (a.bf16) go(clip_emit_u8_kernel<3, false, true, uint16_t>, xh);
        else if (a.unit) go(clip_emit_u8_kernel<3, false, true, float>, x);
        else go(kClipEmitU8[a.c_out - 1][inj], x);
    }
    return hipGetLastError();
}

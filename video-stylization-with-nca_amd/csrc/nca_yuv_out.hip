// nca_yuv_out.hip -- RGB24 images to planar YUV 4:2:0 (I420, NV12) on gfx950, what a video encoder takes, and the host-side builder of the
// conversion's integer coefficients.  The arithmetic is include/ncahip.h's ("planar YUV images"): per pixel
//     Y = clamp(yoff + ((k_yr R + k_yg G + k_yb B + 2^15) >> 16), 0, 255)
// and per 2 x 2 block, from the block's channel sums (centre siting, one rounding)
//     U = clamp(128 + ((k_ur sum R + k_ug sum G + k_ub sum B + 2^17) >> 18), 0, 255),   V likewise          (int32, arithmetic shift)
// The reference never produces YUV (moviepy / cv2 take RGB): this file is the colour conversion a caller would otherwise run on the host
// between ncahip.video's clip entry points and the encoder.  The clip drivers do not come here: their image output writes the planes
// straight from the fp32 state (clip_emit_yuv420_kernel in nca_clip.hip) with the same block writer, nca_yuv420_store_block of nca_yuv.h.
//
// rgb_to_yuv420_kernel: a lane owns 2 rows x 4 columns of one image.  Its 12 source bytes per row come in as the (at most 4)
// memory-aligned dwords that hold them -- inside the tensor only, at any alignment of src -- and are shifted into place in registers.
#include "../../include/ncahip.h"
#include "nca_common.h"
#include "nca_kernels.h"
#include "nca_yuv.h"

namespace {

constexpr int kOutThreads = kYuvOutThreads;
constexpr int kRowDwords = kYuvOutCols * 3 / 4;      // 3 dwords of RGB per lane and row

// src [N,H,W,3] u8 (`total` bytes) -> dst [N,3H/2,W] u8; bx = ceil(W / 4) lane blocks per row pair, `lanes` = N * H/2 * bx
template <bool NV12>
__global__ __launch_bounds__(kOutThreads) void rgb_to_yuv420_kernel(const unsigned char* __restrict__ src, size_t total, int H, int W, int bx,
                                                                    size_t lanes, NcaRgbYuvK k, unsigned char* __restrict__ dst) {
    const size_t id = (size_t)blockIdx.x * kOutThreads + threadIdx.x;
    if (id >= lanes) return;
    const int x0 = (int)(id % bx) * kYuvOutCols;
    const size_t row = id / bx;                                   // row pair n * H/2 + y/2
    const size_t n = row / (size_t)(H >> 1);
    const int y = (int)(row % (size_t)(H >> 1)) * 2;
    const int nv = min(kYuvOutCols, W - x0);
    const uintptr_t mis = (uintptr_t)src & 3;
    int r[2][kYuvOutCols], g[2][kYuvOutCols], b[2][kYuvOutCols];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const size_t first = ((n * H + (size_t)(y + j)) * W + x0) * 3;
        unsigned dw[kRowDwords + 1];
#pragma unroll
        for (int d = 0; d <= kRowDwords; ++d) {
            dw[d] = 0u;
            nca_stage_dword(src, total, mis, first, (size_t)nv * 3, d, dw[d]);
        }
        const unsigned ph = 8u * (unsigned)((first + mis) & 3);   // the segment's first byte within dword 0
        unsigned a[kRowDwords];
#pragma unroll
        for (int d = 0; d < kRowDwords; ++d) a[d] = ph ? (dw[d] >> ph) | (dw[d + 1] << (32u - ph)) : dw[d];
#pragma unroll
        for (int i = 0; i < kYuvOutCols; ++i) {
            r[j][i] = (int)((a[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u);
            g[j][i] = (int)((a[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u);
            b[j][i] = (int)((a[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u);
        }
    }
    nca_yuv420_store_block<NV12>(dst, k, n, H, W, y, x0, nv, r, g, b);
}

}  // namespace

hipError_t nca_launch_clip_rgb_to_yuv420(const unsigned char* src, bool nv12, int N, int H, int W, const int* k, unsigned char* dst, hipStream_t st) {
    const NcaRgbYuvK yk{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9]};
    const int bx = (W + kYuvOutCols - 1) / kYuvOutCols;
    const size_t lanes = (size_t)N * (H / 2) * bx, blocks = (lanes + kOutThreads - 1) / kOutThreads;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const size_t total = (size_t)N * H * W * 3;
    if (nv12) hipLaunchKernelGGL(rgb_to_yuv420_kernel<true>, dim3((unsigned)blocks), dim3(kOutThreads), 0, st, src, total, H, W, bx, lanes, yk, dst);
    else hipLaunchKernelGGL(rgb_to_yuv420_kernel<false>, dim3((unsigned)blocks), dim3(kOutThreads), 0, st, src, total, H, W, bx, lanes, yk, dst);
    return hipGetLastError();
}

// ---- the coefficient builder: plain host C++, no GPU call, C double with contraction off so that a host FMA cannot move a coefficient ----
#pragma clang fp contract(off)

namespace {

int rgb_yuv_quantise(double c) {
    const double v = c * 65536.0;
    return v < 0 ? (int)(v - 0.5) : (int)(v + 0.5);
}

}  // namespace

// matrix 0 = BT.601, 1 = BT.709; range 0 = limited, 1 = full (validated by the caller).  k = the (R, G, B) rows of Y, U, V, then the luma
// offset.  In every row the green coefficient is the remainder that makes the row sum exact: q(sy) for Y, 0 for U and V.
void nca_rgb_yuv_build_coeffs(int matrix, int range, int32_t k[10]) {
    const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722;
    const double sy = range == 0 ? 219.0 / 255.0 : 1.0, sc = range == 0 ? 224.0 / 255.0 : 1.0;
    const double cu = sc / (2.0 * (1.0 - kb)), cv = sc / (2.0 * (1.0 - kr));
    k[0] = rgb_yuv_quantise(sy * kr);
    k[2] = rgb_yuv_quantise(sy * kb);
    k[1] = rgb_yuv_quantise(sy) - k[0] - k[2];
    k[3] = rgb_yuv_quantise(-(cu * kr));          // U = 128 + cu (B - Y') = 128 + cu (-Kr R - Kg G + (1 - Kb) B)
    k[5] = rgb_yuv_quantise(cu * (1.0 - kb));
    k[4] = -k[3] - k[5];
    k[6] = rgb_yuv_quantise(cv * (1.0 - kr));     // V = 128 + cv (R - Y') = 128 + cv ((1 - Kr) R - Kg G - Kb B)
    k[8] = rgb_yuv_quantise(-(cv * kb));
    k[7] = -k[6] - k[8];
    k[9] = range == 0 ? 16 : 0;
}

// The image record of an img_fmt of the clip entry points (nca_kernels.h).  NCAHIP_CLIP_YUV420(layout, matrix, range) is 0x100 | layout |
// matrix << 1 | range << 2 with one bit each: nothing else takes that word apart.
bool nca_img_out(int img_fmt, NcaImgOut* out) {
    *out = NcaImgOut{img_fmt == NCAHIP_CLIP_U8_NHWC ? kImgU8 : kImgF32, {0}};
    if (img_fmt == NCAHIP_CLIP_F32_NCHW || img_fmt == NCAHIP_CLIP_U8_NHWC) return true;
    if (img_fmt < NCAHIP_CLIP_YUV420(0, 0, 0) || img_fmt > NCAHIP_CLIP_YUV420(1, 1, 1)) return false;
    out->kind = (img_fmt & 1) == NCAHIP_YUV_NV12 ? kImgNV12 : kImgI420;
    nca_rgb_yuv_build_coeffs((img_fmt >> 1) & 1, (img_fmt >> 2) & 1, out->k);
    return true;
}

// nca_yuv.hip -- planar YUV 4:2:0 (I420, NV12) clip frames to RGB24 on gfx950, and the host-side builder of the conversion's integer
// coefficients.  The arithmetic is include/ncahip.h's ("planar YUV frames"): per pixel
//     channel = clamp((k_y (Y - yoff) + k_u (U - 128) + k_v (V - 128) + 2^15) >> 16, 0, 255)          (int32, arithmetic shift)
// with the chroma sample (x >> 1, y >> 1) of pixel (x, y).  The reference never sees YUV (cv2 / moviepy hand it RGB): this file is the
// colour conversion a caller would otherwise run on the host before ncahip.video's clip entry points.  nca_resize.hip runs the same
// evaluation (nca_yuv.h) in the loader of its horizontal pass; the launch here serves frames that are already at the model's size.
//
// yuv420_to_rgb_kernel: the output of a frame, [crop_h, crop_w, 3] bytes, is one dense byte range; a lane takes one memory-aligned dword
// of it (a dword store; the range's first and last dword, shared with the neighbouring frames when crop_h * crop_w * 3 is no multiple
// of 4, are written byte by byte, each frame its own bytes).  Four bytes touch at most two pixels; every source byte comes out of the
// aligned dword that holds it, so plane starts at any byte phase cost nothing.  Offsets per frame are 64-bit.
#include "nca_common.h"
#include "nca_kernels.h"
#include "nca_yuv.h"

namespace {

constexpr int kYuvThreads = 256;

// grid (ceil(dwords / 256), frames).  src [N, 3H/2, W] u8 (`total` bytes), crop (x0, y0, cw, ch); dst [N, ch, cw, 3] u8
template <bool NV12>
__global__ __launch_bounds__(kYuvThreads) void yuv420_to_rgb_kernel(const unsigned char* __restrict__ src, size_t total, int H, int W, int x0, int y0,
                                                                    int cw, int ch, NcaYuvK k, unsigned char* __restrict__ dst) {
    const size_t n = blockIdx.y;
    const int fbytes = ch * cw * 3;                                     // <= 16384^2 * 3 < 2^31
    unsigned char* const out = dst + n * (size_t)fbytes;
    const int dmis = (int)((uintptr_t)out & 3);
    const int b0 = (int)(blockIdx.x * kYuvThreads + threadIdx.x) * 4 - dmis;      // first frame byte of this lane's dword; >= -3
    if (b0 >= fbytes) return;
    const uintptr_t mis = (uintptr_t)src & 3;
    const size_t plane = (size_t)H * W, frame = n * (plane + plane / 2);
    const int lo = max(b0, 0), hi = min(b0 + 4, fbytes);
    unsigned byte[4] = {0u, 0u, 0u, 0u};
    int pix = -1, Y = 0, U = 0, V = 0;
    for (int b = lo; b < hi; ++b) {
        const int p = b / 3, c = b - 3 * p;
        if (p != pix) {                                                 // at most twice per lane
            pix = p;
            const int py = p / cw, yy = y0 + py, xx = x0 + (p - py * cw);
            Y = nca_load_u8_dw(src, total, mis, frame + (size_t)yy * W + xx);
            if (NV12) {
                const size_t uv = frame + plane + (size_t)(yy >> 1) * W + 2 * (xx >> 1);
                U = nca_load_u8_dw(src, total, mis, uv);
                V = nca_load_u8_dw(src, total, mis, uv + 1);
            } else {
                const size_t u = frame + plane + (size_t)(yy >> 1) * (W >> 1) + (xx >> 1);
                U = nca_load_u8_dw(src, total, mis, u);
                V = nca_load_u8_dw(src, total, mis, u + plane / 4);
            }
        }
        byte[b - b0] = (unsigned)nca_yuv_channel(k, Y, U, V, c);
    }
    if (hi - lo == 4) {
        *reinterpret_cast<unsigned*>(out + b0) = nca_pack_u8x4(byte[0], byte[1], byte[2], byte[3]);
    } else {
        for (int b = lo; b < hi; ++b) out[b] = (unsigned char)byte[b - b0];
    }
}

}  // namespace

hipError_t nca_launch_clip_yuv420_to_rgb(const unsigned char* src, bool nv12, int N, int H, int W, int x0, int y0, int cw, int ch, const int* k,
                                         unsigned char* dst, hipStream_t st) {
    const NcaYuvK yk{k[0], k[1], k[2], k[3], k[4], k[5]};
    const size_t frame = (size_t)H * W / 2 * 3, fbytes = (size_t)ch * cw * 3, total = (size_t)N * frame;
    const unsigned blocks = (unsigned)((fbytes + 3 + 4 * kYuvThreads - 1) / (4 * kYuvThreads));      // + 3: the range may start at byte 3 of a dword
    for (int n0 = 0; n0 < N; n0 += 65535) {              // grid y holds at most 65535 frames
        const int nn = N - n0 < 65535 ? N - n0 : 65535;
        const unsigned char* s = src + (size_t)n0 * frame;             // the chunk's own base and the bytes from there to the tensor's end
        unsigned char* d = dst + (size_t)n0 * fbytes;
        if (nv12)
            hipLaunchKernelGGL(yuv420_to_rgb_kernel<true>, dim3(blocks, (unsigned)nn), dim3(kYuvThreads), 0, st, s, total - (size_t)n0 * frame, H, W, x0,
                               y0, cw, ch, yk, d);
        else
            hipLaunchKernelGGL(yuv420_to_rgb_kernel<false>, dim3(blocks, (unsigned)nn), dim3(kYuvThreads), 0, st, s, total - (size_t)n0 * frame, H, W, x0,
                               y0, cw, ch, yk, d);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// ---- the coefficient builder: plain host C++, no GPU call, C double with contraction off so that a host FMA cannot move a coefficient ----
#pragma clang fp contract(off)

namespace {

int yuv_quantise(double c) {
    const double v = c * 65536.0;
    return v < 0 ? (int)(v - 0.5) : (int)(v + 0.5);
}

}  // namespace

// matrix 0 = BT.601, 1 = BT.709; range 0 = limited, 1 = full (validated by the caller).  k = (k_y, k_rv, k_gu, k_gv, k_bu, luma offset)
void nca_yuv_build_coeffs(int matrix, int range, int32_t k[6]) {
    const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722;
    const double kg = 1.0 - kr - kb;
    const double sy = range == 0 ? 255.0 / 219.0 : 1.0, sc = range == 0 ? 255.0 / 224.0 : 1.0;
    k[0] = yuv_quantise(sy);
    k[1] = yuv_quantise(2.0 * (1.0 - kr) * sc);
    k[2] = yuv_quantise(-(2.0 * kb * (1.0 - kb) / kg) * sc);
    k[3] = yuv_quantise(-(2.0 * kr * (1.0 - kr) / kg) * sc);
    k[4] = yuv_quantise(2.0 * (1.0 - kb) * sc);
    k[5] = range == 0 ? 16 : 0;
}

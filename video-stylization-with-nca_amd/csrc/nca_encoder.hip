// nca_encoder.hip -- ImageEncoder.forward (EncoderConditioning/encoder.py:37-57) for every frame of a clip call in ONE launch, inference only:
//   gray = mean over channels; feat = [sobel_x(gray) | sobel_y(gray) | laplacian(gray) | blur5x5(img[c])]   (zero padding)
//   h1   = relu(conv3x3(feat, w1) + b1)                                                                   (zero padding)
//   goal = conv3x3(h1, w2)                                                                                (zero padding, no bias)
// One workgroup owns a 16 x 16 output tile of one image.  It stages the image tile with a 4-cell halo in LDS (2 for the blur, 1 for each
// convolution; every input pixel is read once per workgroup), computes feat on the tile + 2 ring and h1 on the tile + 1 ring into LDS, then
// the output.  Both convolutions are implicit GEMMs per tap on the exact-f32 MFMA (nca_mfma, 16 x 16 x 4): A = the tap's weight slice
// [16 output channels x 4 input channels], B = the input-channel vectors of 16 cells from LDS.  A wave keeps the A operands of its block of 16
// output channels in registers for the whole tile (loaded once per workgroup); no inter-workgroup synchronisation, no atomics, no workspace.
//
// Two padding rules: feat is 0 outside the image, and so is h1 -- conv2 pads with zeros, NOT with relu(b1 + ...) evaluated on the halo.
//
// LDS layout (ds_read_b32 banks are dword % 32 over 32-lane halves, i.e. MFMA lane groups g = 0, 1 or 2, 3 together): feat and h1 are
// channel-major planes whose stride is 16 mod 32, so the B reads of one half -- 16 consecutive cells of channel 4k + g and of channel
// 4k + g + 1 -- fall on disjoint banks.  (The h1 stores of a half go to channels 4 apart, a 2-way conflict: 4 stores per 18 MFMAs.)
//
// The goal leaves as fp32, or -- for a state stored as bf16 (nca_cond_bf16.hip) -- rounded to bf16 on the final store: the same kernel
// and arithmetic, one more instantiation per (NEB, U8).
#include "nca_cond_tile.h"   // StBF16
#include "nca_clip_u8.h"

namespace {

constexpr int kT = 16;                    // output tile edge
constexpr int kImgE = kT + 8;             // image tile with its 4-cell halo
constexpr int kFeatE = kT + 4;            // feat region: tile + 2 ring
constexpr int kH1E = kT + 2;              // h1 region: tile + 1 ring
constexpr int kFeatK = 8;                 // feat channels padded to two MFMA k-steps (3 + ch <= 7)
constexpr int kFeatStride = kFeatE * kFeatE;                // 400 = 16 mod 32
constexpr int kH1Cells = kH1E * kH1E;                       // 324
constexpr int kH1Groups = (kH1Cells + 15) / 16;             // 21 groups of 16 cells
constexpr int kH1Stride = kH1Groups * 16;                   // 336 = 16 mod 32
constexpr int kImgPlane = kImgE * kImgE;
static_assert(kFeatStride % 32 == 16 && kH1Stride % 32 == 16, "plane strides: the two lane groups of a half on disjoint banks");
static_assert(kImgE <= kClipStageCols, "the image tile row must fit the staged uint8 row");

// float(u8) / 255.0f with a true division: ToTensor's range [0, 1], used as it is
__device__ __forceinline__ float enc_widen_u8(unsigned v) { return __fdiv_rn((float)v, 255.0f); }

// one goal element on its way out: fp32 as it is, or rounded to bf16 (RNE, the rounding of the bf16-storage step) -- the only place
// where the two goal types differ
__device__ __forceinline__ void enc_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void enc_store(uint16_t* p, float v) { *p = (uint16_t)(StBF16::pk2(v, 0.0f) & 0xffffu); }

// NEB: blocks of 16 output channels (E padded to 16 * NEB).  256 threads = 4 waves; wave w works on channel block w % NEB.
// GT: the goal's element type, float or uint16_t (bf16 bits, for a state stored as bf16).
template <int NEB, bool U8, typename GT>
__global__ __launch_bounds__(256) void clip_encode_kernel(const void* __restrict__ frames, const float* __restrict__ k3, const float* __restrict__ k5,
                                                          const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                          GT* __restrict__ goal, int N, int ch, int E, int H, int W, int tiles_x, int tiles_y) {
    constexpr int EP = 16 * NEB, KS2 = EP / 4;
    constexpr int kImgFloats = 4 * kImgPlane, kRawFloats = U8 ? kImgE * kRawDwords : 0;
    constexpr int kFront = kImgFloats + kRawFloats, kH1Floats = EP * kH1Stride;
    // the image tile (and the raw uint8 rows) are dead once feat exists: h1 reuses their space
    __shared__ float s_feat[kFeatK * kFeatStride];
    __shared__ float s_un[kFront > kH1Floats ? kFront : kH1Floats];
    float* const s_img = s_un;
    unsigned* const s_raw = reinterpret_cast<unsigned*>(s_un + kImgFloats);
    float* const s_h1 = s_un;

    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
    const size_t n = blk / ((size_t)tiles_x * tiles_y);   // image index f * B + b
    if (n >= (size_t)N) return;
    const int x0 = tx * kT, y0 = ty * kT;
    const size_t plane = (size_t)H * W;

    // ---- 1. image tile + 4 halo, zero outside the image
    if (U8) {
        const unsigned char* const base = static_cast<const unsigned char*>(frames);
        const int cx0 = max(x0 - 4, 0), cx1 = min(x0 + kT + 4, W);
        clip_stage_u8_rows<kImgE>(base, (size_t)N * plane * 3, n, plane, H, W, y0 - 4, cx0, cx1, s_raw, tid);
        __syncthreads();
        for (int i = tid; i < kImgPlane; i += 256) {
            const int r = i / kImgE, c = i % kImgE;
            const int y = y0 - 4 + r, x = x0 - 4 + c;
            float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
            if (y >= 0 && y < H && x >= cx0 && x < cx1) {
                const unsigned char* const p = clip_staged_u8_pixel(base, s_raw, r, n, plane, W, y, x, cx0);
                v0 = enc_widen_u8(p[0]), v1 = enc_widen_u8(p[1]), v2 = enc_widen_u8(p[2]);
            }
            s_img[i] = v0, s_img[kImgPlane + i] = v1, s_img[2 * kImgPlane + i] = v2;
        }
    } else {
        const float* const ib = static_cast<const float*>(frames) + n * (size_t)ch * plane;
        for (int i = tid; i < ch * kImgPlane; i += 256) {
            const int k = i / kImgPlane, q = i % kImgPlane;
            const int y = y0 - 4 + q / kImgE, x = x0 - 4 + q % kImgE;
            s_img[i] = (y >= 0 && y < H && x >= 0 && x < W) ? ib[(size_t)k * plane + (size_t)y * W + x] : 0.0f;
        }
    }
    __syncthreads();

    // ---- 2. feat on the tile + 2 ring (0 outside the image; channels 3 + ch .. 7 are zero k-padding)
    {
        float f3[27], f5[25];
#pragma unroll
        for (int i = 0; i < 27; ++i) f3[i] = k3[i];
#pragma unroll
        for (int i = 0; i < 25; ++i) f5[i] = k5[i];
        const float fch = (float)ch;
        for (int q = tid; q < kFeatStride; q += 256) {
            const int r = q / kFeatE, c = q % kFeatE;
            const int y = y0 - 2 + r, x = x0 - 2 + c;
            float out[kFeatK];
#pragma unroll
            for (int k = 0; k < kFeatK; ++k) out[k] = 0.0f;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const float* const p = s_img + (r + 2) * kImgE + (c + 2);   // this cell in the image tile
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        float g = 0.0f;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < ch) g += p[k * kImgPlane + (dy - 1) * kImgE + (dx - 1)];
                        g = __fdiv_rn(g, fch);   // the channel mean: sum / ch
#pragma unroll
                        for (int f = 0; f < 3; ++f) out[f] = fmaf(f3[f * 9 + dy * 3 + dx], g, out[f]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= ch) break;
                    float acc = 0.0f;
#pragma unroll
                    for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
                        for (int dx = 0; dx < 5; ++dx) acc = fmaf(f5[dy * 5 + dx], p[k * kImgPlane + (dy - 2) * kImgE + (dx - 2)], acc);
                    }
                    out[3 + k] = acc;
                }
            }
#pragma unroll
            for (int k = 0; k < kFeatK; ++k) s_feat[k * kFeatStride + q] = out[k];
        }
    }

    // ---- A operands of this wave's block of 16 output channels, once per workgroup: lane l = 16 g + i holds A[row i][k g]
    const int lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int eb = wv % NEB, e_a = eb * 16 + li;
    const int K1 = 3 + ch;
    float a1[9][2], a2[9][KS2], bias[4];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int k = 4 * kk + lg;
            a1[t][kk] = (e_a < E && k < K1) ? w1[((size_t)e_a * K1 + k) * 9 + t] : 0.0f;
        }
#pragma unroll
        for (int kk = 0; kk < KS2; ++kk) {
            const int k = 4 * kk + lg;
            a2[t][kk] = (e_a < E && k < E) ? w2[((size_t)e_a * E + k) * 9 + t] : 0.0f;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = eb * 16 + 4 * lg + r;
        bias[r] = e < E ? b1[e] : 0.0f;
    }
    __syncthreads();   // feat complete; the image tile is dead from here on (h1 takes its space)

    // ---- 3. h1 on the tile + 1 ring: 21 groups of 16 cells (the last group's cells past 324 repeat cell 323 and land in the plane's padding)
    for (int grp = wv / NEB; grp < kH1Groups; grp += 4 / NEB) {
        const int q = grp * 16 + li, qc = min(q, kH1Cells - 1);
        const int r = qc / kH1E, c = qc % kH1E;
        const float* const fb = s_feat + lg * kFeatStride + r * kFeatE + c;   // tap (0, 0) of this cell, channel g
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                acc = nca_mfma(a1[t][kk], fb[kk * 4 * kFeatStride + (t / 3) * kFeatE + (t % 3)], acc);
        }
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        const bool inside = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float v = fmaxf(acc[rr] + bias[rr], 0.0f);
            s_h1[(eb * 16 + 4 * lg + rr) * kH1Stride + q] = inside ? v : 0.0f;     // conv2 pads h1 with ZEROS
        }
    }
    __syncthreads();

    // ---- 4. goal on the tile: one group = one row of 16 output cells
    GT* const ob = goal + n * (size_t)E * plane;
    for (int row = wv / NEB; row < kT; row += 4 / NEB) {
        const float* const hb = s_h1 + lg * kH1Stride + row * kH1E + li;      // tap (0, 0) of this cell, channel g
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int kk = 0; kk < KS2; ++kk)
                acc = nca_mfma(a2[t][kk], hb[kk * 4 * kH1Stride + (t / 3) * kH1E + (t % 3)], acc);
        }
        const int y = y0 + row, x = x0 + li;
        if (y < H && x < W) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int e = eb * 16 + 4 * lg + rr;
                if (e < E) enc_store(ob + (size_t)e * plane + (size_t)y * W + x, acc[rr]);
            }
        }
    }
}

template <int NEB, typename GT>
void clip_encode_launch(bool u8, dim3 grid, hipStream_t st, const void* frames, const float* k3, const float* k5, const float* w1, const float* b1,
                        const float* w2, GT* goal, int N, int ch, int E, int H, int W, int tiles_x, int tiles_y) {
    if (u8) hipLaunchKernelGGL((clip_encode_kernel<NEB, true, GT>), grid, dim3(256), 0, st, frames, k3, k5, w1, b1, w2, goal, N, ch, E, H, W, tiles_x, tiles_y);
    else hipLaunchKernelGGL((clip_encode_kernel<NEB, false, GT>), grid, dim3(256), 0, st, frames, k3, k5, w1, b1, w2, goal, N, ch, E, H, W, tiles_x, tiles_y);
}

template <typename GT>
hipError_t clip_encode_dispatch(const void* frames, bool u8, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2, GT* goal,
                                int N, int ch, int E, int H, int W, hipStream_t st) {
    if (ch < 1 || ch > 4 || (u8 && ch != 3) || E < 1 || E > 32) return hipErrorInvalidValue;
    const int tiles_x = (W + kT - 1) / kT, tiles_y = (H + kT - 1) / kT;
    const size_t blocks = (size_t)N * tiles_x * tiles_y;
    if (blocks == 0 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (E <= 16) clip_encode_launch<1>(u8, grid, st, frames, k3, k5, w1, b1, w2, goal, N, ch, E, H, W, tiles_x, tiles_y);
    else clip_encode_launch<2>(u8, grid, st, frames, k3, k5, w1, b1, w2, goal, N, ch, E, H, W, tiles_x, tiles_y);
    return hipGetLastError();
}

}  // namespace

hipError_t nca_launch_clip_encode(const void* frames, bool u8, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2,
                                  float* goal, int N, int ch, int E, int H, int W, hipStream_t st) {
    return clip_encode_dispatch(frames, u8, k3, k5, w1, b1, w2, goal, N, ch, E, H, W, st);
}

hipError_t nca_launch_clip_encode_bf16(const void* frames, bool u8, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2,
                                       uint16_t* goal, int N, int ch, int E, int H, int W, hipStream_t st) {
    return clip_encode_dispatch(frames, u8, k3, k5, w1, b1, w2, goal, N, ch, E, H, W, st);
}

// nca_resize.hip -- crop + resize of uint8 clip frames on gfx950, bit for bit what Pillow's 8-bit Image.resize computes
// (Resample.c: ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc), and the host-side builder of its coefficient tables.
//
// The reference shrinks decoder frames on the host: ConditioneDyNCA/utils/misc/preprocess_texture.py:9-33 (centre cut, bicubic resize) and
// EncoderConditioning/utils/utils.py:5-25 (square crop, Lanczos resize).  Pillow's resize of an 8-bit image is an integer algorithm: per
// axis a table of 22-bit fixed-point coefficients, one row per output index with its first tap `xmin` and tap count `n`; a pass computes
//     out = clamp((2^21 + sum_j px[xmin + j] * k[j]) >> 22, 0, 255)          (int32 accumulation, arithmetic shift)
// per channel.  The horizontal pass runs first and writes a uint8 image of crop_h x out_w pixels, the vertical pass reads that image: the
// rounding to uint8 between the passes is part of the result.  The resize sees only the cropped image, so the tables index pixels of the
// crop (0 .. crop_w - 1, 0 .. crop_h - 1).
//
// Two launches for all N frames of a call:
//   resize_h_kernel   a workgroup takes a band of rows x a block of output columns.  It keeps the block's coefficient rows in LDS and stages
//                     the source row segments the block needs (first tap of its first column .. last tap of its last column) as
//                     memory-aligned dwords, whatever the tensor's alignment, the crop origin or W * 3; then one lane per output byte
//                     loops over that column's runtime tap count.
//   resize_v_kernel   one lane per 4 output bytes of a row (dword loads and stores when out_w * 3 and the buffers allow it), or per byte;
//                     the row's coefficients are wave-uniform (scalar loads); n coalesced reads of intermediate rows.
// Planar YUV 4:2:0 sources (ncahip_clip_resize_yuv420_u8): resize_h_kernel is a template over the source format.  Its I420 / NV12
// instantiations stage the luma segment and the chroma samples under it the same way, behind the rows, and one lane per staged pixel
// writes the converted RGB bytes (nca_yuv.h: include/ncahip.h's integer arithmetic, nearest chroma) into the rows the tap loop reads;
// everything after that, the vertical pass included, is the RGB24 code, and no full-size RGB image exists.
// Planar YUV 4:2:0 images (ncahip_clip_resize_u8_yuv420): the horizontal pass is the RGB24 one, and resize_v_yuv420_kernel takes the
// vertical pass's place: a lane forms 2 rows x 4 columns of RGB bytes in registers and stores the planes with the planar emit's block
// writer (nca_yuv.h), so no full-size RGB image exists on the way out either.
// |k| < 2^23 and pixels < 2^8: the multiply-adds are 24-bit (v_mad_i32_i24).  The tables come from device memory and are not trusted with
// addresses: every row's (first tap, count) is cut to the staged segment / the crop before the tap loop, so a bad table gives wrong
// pixels, never a read outside the frame.  Offsets per image are 64-bit.
#include <cmath>

#include "nca_common.h"
#include "nca_kernels.h"
#include "nca_yuv.h"

namespace {

constexpr int kRszThreads = 256;
constexpr int kRszMaxCols = 64;            // output columns per workgroup of the horizontal pass (fewer when the rows are long)
constexpr int kRszMaxRows = 16;            // rows per band
constexpr int kRszLdsBudget = 60 * 1024;   // dynamic LDS per workgroup: coefficient rows + staged source rows

__device__ __forceinline__ int rsz_clamp_u8(int acc) { return min(max(acc >> 22, 0), 255); }

// Four accumulators -> four packed bytes (nca_pack_u8x4: the form the compiler may not fuse, see nca_yuv.h)
__device__ __forceinline__ unsigned rsz_pack_u8x4(int a0, int a1, int a2, int a3) {
    return nca_pack_u8x4((unsigned)rsz_clamp_u8(a0), (unsigned)rsz_clamp_u8(a1), (unsigned)rsz_clamp_u8(a2), (unsigned)rsz_clamp_u8(a3));
}

// Pixels a block of `cols` output columns can touch: its first column's first tap to its last column's last tap.  With
// xmin(i) >= center(i) - sup - 0.5 and xmin(i) + n(i) <= center(i) + sup + 0.5 that is at most (cols - 1) * scale + 2 * sup + 1, and
// 2 * ceil(sup) = ksize - 1.
int rsz_footprint(int cols, int in, int out, int ksize) {
    const double span = (double)(cols - 1) * (double)in / (double)out;
    const long long fp = (long long)std::ceil(span) + ksize + 1;
    return (int)(fp < in ? fp : in);
}
int rsz_row_dwords(int fp) { return (3 * fp + 3 + 3) / 4 + 1; }   // aligned dwords that cover 3 * fp bytes at any phase
int rsz_seg_dwords(int bytes) { return (bytes + 3 + 3) / 4 + 1; }  // the same for a segment of `bytes` bytes
// Planar sources stage, per row, the luma segment (fp bytes) and the chroma samples under it (at most fp / 2 + 1: two planes' segments
// for I420, one interleaved segment of twice the bytes for NV12; 2 * seg(c) >= seg(2 c) covers both)
int rsz_yuv_luma_dwords(int fp) { return rsz_seg_dwords(fp); }
int rsz_yuv_chroma_dwords(int fp) { return rsz_seg_dwords(fp / 2 + 1); }

constexpr int kSrcRgb24 = 0, kSrcI420 = 1, kSrcNv12 = 2;

// grid (column blocks * row bands, frames), block 256.  src [N,H,W,3] u8 (`total` bytes), crop (x0, y0, cw, ch); kx [out_w, ksize] and
// bx [out_w, 2] = (xmin, n) per output column; tmp [N, ch, out_w, 3] u8.  Dynamic LDS: cols * ksize coefficients, then rows * row_dw dwords.
// SRC = kSrcI420 / kSrcNv12: src is [N, 3H/2, W] u8 (H, W even).  The loader stages each row's luma segment and the chroma samples under it
// (ydw + 2 * cdw more dwords per row, after the rows) and writes the converted RGB bytes (yk; nearest chroma) into the rows at phase 0;
// the tap loop is the same.
template <int SRC>
__global__ __launch_bounds__(kRszThreads) void resize_h_kernel(const unsigned char* __restrict__ src, size_t total, int H, int W, int x0, int y0,
                                                               int cw, int ch, const int* __restrict__ kx, const int* __restrict__ bx, int ksize,
                                                               unsigned char* __restrict__ tmp, int out_w, int cols, int rows, int fp, int row_dw,
                                                               int col_blocks, NcaYuvK yk, int ydw, int cdw) {
    extern __shared__ __attribute__((aligned(16))) int rsz_lds[];
    __shared__ int s_xmin[kRszMaxCols], s_n[kRszMaxCols];
    int* const s_k = rsz_lds;
    unsigned* const raw = reinterpret_cast<unsigned*>(rsz_lds + cols * ksize);
    const int tid = threadIdx.x;
    const int cb = blockIdx.x % col_blocks, band = blockIdx.x / col_blocks;
    const size_t n = blockIdx.y;
    const int c0 = cb * cols, ncols = min(cols, out_w - c0);
    const int r0 = band * rows, nrows = min(rows, ch - r0);
    // the staged segment: fp pixels from the first column's first tap, cut to the crop
    const int sx0 = min(max(bx[2 * c0], 0), cw - 1);
    const int fpw = min(fp, cw - sx0);

    if (tid < ncols) {                         // (first tap, count) of every column, cut to the staged segment
        const int xm = min(max(bx[2 * (c0 + tid)], sx0), sx0 + fpw - 1);
        s_xmin[tid] = xm - sx0;
        s_n[tid] = min(max(bx[2 * (c0 + tid) + 1], 0), min(ksize, sx0 + fpw - xm));
    }
    for (int i = tid; i < ncols * ksize; i += kRszThreads) s_k[i] = kx[(size_t)c0 * ksize + i];

    const uintptr_t mis = (uintptr_t)src & 3;
    const size_t plane = (size_t)H * W;
    if constexpr (SRC == kSrcRgb24) {
        for (int i = tid; i < nrows * row_dw; i += kRszThreads) {
            const int r = i / row_dw, d = i - r * row_dw;
            const size_t first = (n * plane + (size_t)(y0 + r0 + r) * W + x0 + sx0) * 3;      // first byte of the row segment
            unsigned v;
            if (nca_stage_dword(src, total, mis, first, (size_t)fpw * 3, d, v)) raw[i] = v;
        }
    } else {
        const int st_dw = ydw + 2 * cdw;
        unsigned* const stage = raw + rows * row_dw;
        const size_t frame = n * (plane + plane / 2), quarter = plane / 4;
        const int px0 = x0 + sx0, cx0 = px0 >> 1;                    // first staged pixel of a row, first chroma sample under it
        const int cn = ((px0 + fpw - 1) >> 1) - cx0 + 1;             // <= fp / 2 + 1
        for (int i = tid; i < nrows * st_dw; i += kRszThreads) {
            const int r = i / st_dw, d = i - r * st_dw, yy = y0 + r0 + r;
            size_t first, len;
            int dd;
            if (d < ydw) {
                first = frame + (size_t)yy * W + px0, len = (size_t)fpw, dd = d;
            } else if (SRC == kSrcI420) {
                const int pl = (d - ydw) / cdw;                      // 0 = U, 1 = V
                first = frame + plane + pl * quarter + (size_t)(yy >> 1) * (W >> 1) + cx0, len = (size_t)cn, dd = d - ydw - pl * cdw;
            } else {
                first = frame + plane + (size_t)(yy >> 1) * W + 2 * cx0, len = 2 * (size_t)cn, dd = d - ydw;
            }
            unsigned v;
            if (nca_stage_dword(src, total, mis, first, len, dd, v)) stage[i] = v;
        }
        __syncthreads();
        for (int i = tid; i < nrows * fpw; i += kRszThreads) {       // one lane per staged pixel: three RGB bytes into its row
            const int r = i / fpw, x = i - r * fpw, yy = y0 + r0 + r;
            const unsigned char* const st = reinterpret_cast<const unsigned char*>(stage + r * st_dw);
            const int c = ((px0 + x) >> 1) - cx0;
            const int Y = st[(int)((frame + (size_t)yy * W + px0 + mis) & 3) + x];
            int U, V;
            if (SRC == kSrcI420) {
                const size_t uf = frame + plane + (size_t)(yy >> 1) * (W >> 1) + cx0;
                U = st[4 * ydw + (int)((uf + mis) & 3) + c];
                V = st[4 * (ydw + cdw) + (int)((uf + quarter + mis) & 3) + c];
            } else {
                const unsigned char* const uv = st + 4 * ydw + (int)((frame + plane + (size_t)(yy >> 1) * W + 2 * cx0 + mis) & 3) + 2 * c;
                U = uv[0], V = uv[1];
            }
            unsigned char* const o = reinterpret_cast<unsigned char*>(raw + r * row_dw) + 3 * x;
            o[0] = (unsigned char)nca_yuv_channel(yk, Y, U, V, 0);
            o[1] = (unsigned char)nca_yuv_channel(yk, Y, U, V, 1);
            o[2] = (unsigned char)nca_yuv_channel(yk, Y, U, V, 2);
        }
    }
    __syncthreads();

    const int rowb = ncols * 3;
    const unsigned char* const rawb = reinterpret_cast<const unsigned char*>(raw);
    for (int i = tid; i < nrows * rowb; i += kRszThreads) {
        const int r = i / rowb, b = i - r * rowb;
        const int col = b / 3, c = b - 3 * col;
        const size_t first = (n * plane + (size_t)(y0 + r0 + r) * W + x0 + sx0) * 3;
        const int phase = SRC == kSrcRgb24 ? (int)((first + mis) & 3) : 0;             // converted rows start at byte 0
        const unsigned char* px = rawb + (size_t)r * row_dw * 4 + phase + 3 * s_xmin[col] + c;
        const int* const kr = s_k + col * ksize;
        const int taps = s_n[col];
        int acc = 1 << 21;
        for (int j = 0; j < taps; ++j) acc = __mul24((int)px[3 * j], kr[j]) + acc;
        tmp[((n * ch + (size_t)(r0 + r)) * out_w + c0) * 3 + b] = (unsigned char)rsz_clamp_u8(acc);
    }
}

// grid (ceil(out_w * 3 / (256 * V)), out_h, frames), block 256.  tmp [N, ch, out_w, 3] -> dst [N, out_h, out_w, 3]; ky [out_h, ksize],
// by [out_h, 2] = (ymin, n).  V = 4 needs out_w * 3 % 4 == 0 and 4-byte aligned tmp and dst.
template <int V>
__global__ __launch_bounds__(kRszThreads) void resize_v_kernel(const unsigned char* __restrict__ tmp, int ch, const int* __restrict__ ky,
                                                               const int* __restrict__ by, int ksize, unsigned char* __restrict__ dst, int out_h,
                                                               int rowlen) {
    const int y = blockIdx.y;
    const size_t n = blockIdx.z;
    const int b = (blockIdx.x * kRszThreads + threadIdx.x) * V;
    if (b >= rowlen) return;
    const int ymin = min(max(by[2 * y], 0), ch - 1);                       // wave-uniform, cut to the crop
    const int taps = min(max(by[2 * y + 1], 0), min(ksize, ch - ymin));
    const int* const kr = ky + (size_t)y * ksize;
    const unsigned char* p = tmp + (n * ch + (size_t)ymin) * rowlen + b;
    unsigned char* const o = dst + (n * out_h + (size_t)y) * rowlen + b;
    if (V == 4) {
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
        for (int j = 0; j < taps; ++j, p += rowlen) {
            const unsigned v = *reinterpret_cast<const unsigned*>(p);
            const int k = kr[j];
            a0 = __mul24((int)(v & 255u), k) + a0;
            a1 = __mul24((int)((v >> 8) & 255u), k) + a1;
            a2 = __mul24((int)((v >> 16) & 255u), k) + a2;
            a3 = __mul24((int)(v >> 24), k) + a3;
        }
        *reinterpret_cast<unsigned*>(o) = rsz_pack_u8x4(a0, a1, a2, a3);
    } else {
        int acc = 1 << 21;
        for (int j = 0; j < taps; ++j, p += rowlen) acc = __mul24((int)*p, kr[j]) + acc;
        *o = (unsigned char)rsz_clamp_u8(acc);
    }
}

// The vertical pass that writes planar YUV 4:2:0 (ncahip_clip_resize_u8_yuv420): grid (ceil(ceil(out_w / 4) / 64), out_h / 2, frames),
// block 64.  tmp [N, ch, out_w, 3] (`total` bytes) -> dst [N, 3 out_h / 2, out_w]; out_h and out_w even.  A lane owns 2 output rows x 4
// columns, the planar emit's block: 12 bytes of an intermediate row serve both rows, so the lane walks the union of the two rows' tap
// ranges once and gives each row its own coefficient -- 0 outside that row's (ymin, n), which adds nothing; both are cut to the crop as
// resize_v_kernel cuts them and are wave-uniform.  24 accumulators -> the clamped RGB bytes in registers -> nca_yuv420_store_block.
// Intermediate rows are out_w * 3 bytes: a multiple of 4 only when out_w % 4 == 0.  A lane's 12 bytes are three aligned dwords when they
// start on one; otherwise (and for the 6 bytes of a row's last lane when out_w % 4 == 2) they come in as the memory-aligned dwords that
// hold them, inside the workspace only, and are shifted into place.
template <bool NV12>
__global__ __launch_bounds__(kYuvOutThreads) void resize_v_yuv420_kernel(const unsigned char* __restrict__ tmp, size_t total, int ch,
                                                                         const int* __restrict__ ky, const int* __restrict__ by, int ksize,
                                                                         unsigned char* __restrict__ dst, int out_h, int out_w, NcaRgbYuvK k) {
    constexpr int kBytes = kYuvOutCols * 3, kDw = kBytes / 4;
    const int x0 = (int)(blockIdx.x * kYuvOutThreads + threadIdx.x) * kYuvOutCols;
    if (x0 >= out_w) return;
    const int y = (int)blockIdx.y * 2;
    const size_t n = blockIdx.z;
    const int nv = min(kYuvOutCols, out_w - x0);
    int ymin[2], taps[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {                                          // wave-uniform, cut to the crop
        ymin[j] = min(max(by[2 * (y + j)], 0), ch - 1);
        taps[j] = min(max(by[2 * (y + j) + 1], 0), min(ksize, ch - ymin[j]));
    }
    const int* const kr0 = ky + (size_t)y * ksize;
    const int* const kr1 = kr0 + ksize;
    const int r0 = min(ymin[0], ymin[1]), r1 = max(ymin[0] + taps[0], ymin[1] + taps[1]);      // 0 <= r0, r1 <= ch
    const uintptr_t mis = (uintptr_t)tmp & 3;
    const size_t rowlen = (size_t)out_w * 3;
    size_t first = (n * ch + (size_t)r0) * rowlen + (size_t)x0 * 3;        // first byte of the lane's segment in row r0
    int acc[2][kBytes];
#pragma unroll
    for (int i = 0; i < kBytes; ++i) acc[0][i] = acc[1][i] = 1 << 21;
    for (int r = r0; r < r1; ++r, first += rowlen) {
        const int j0 = r - ymin[0], j1 = r - ymin[1];
        const int k0 = j0 >= 0 && j0 < taps[0] ? kr0[j0] : 0;
        const int k1 = j1 >= 0 && j1 < taps[1] ? kr1[j1] : 0;
        const unsigned ph = 8u * (unsigned)((first + mis) & 3);            // the segment's first byte within its aligned dword
        unsigned a[kDw];
        if (ph == 0u && nv == kYuvOutCols) {
            const unsigned* const p = reinterpret_cast<const unsigned*>(tmp + first);
#pragma unroll
            for (int d = 0; d < kDw; ++d) a[d] = p[d];
        } else {
            unsigned dw[kDw + 1];
#pragma unroll
            for (int d = 0; d <= kDw; ++d) {
                dw[d] = 0u;
                nca_stage_dword(tmp, total, mis, first, (size_t)nv * 3, d, dw[d]);
            }
#pragma unroll
            for (int d = 0; d < kDw; ++d) a[d] = ph ? (dw[d] >> ph) | (dw[d + 1] << (32u - ph)) : dw[d];
        }
#pragma unroll
        for (int i = 0; i < kBytes; ++i) {
            const int v = (int)((a[i >> 2] >> (8 * (i & 3))) & 255u);
            acc[0][i] = __mul24(v, k0) + acc[0][i];
            acc[1][i] = __mul24(v, k1) + acc[1][i];
        }
    }
    int r[2][kYuvOutCols], g[2][kYuvOutCols], b[2][kYuvOutCols];          // clamped after the >> 22, before any YUV arithmetic
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < kYuvOutCols; ++i) {
            r[j][i] = rsz_clamp_u8(acc[j][3 * i]);
            g[j][i] = rsz_clamp_u8(acc[j][3 * i + 1]);
            b[j][i] = rsz_clamp_u8(acc[j][3 * i + 2]);
        }
    nca_yuv420_store_block<NV12>(dst, k, n, out_h, out_w, y, x0, nv, r, g, b);
}

}  // namespace

namespace {

// What the vertical pass writes: RGB24 [N,out_h,out_w,3] (resize_v_kernel), or planar YUV 4:2:0 [N,3 out_h/2,out_w] with the ten
// coefficient words k (resize_v_yuv420_kernel; out_h and out_w even)
struct RszPlanar {
    bool on, nv12;
    NcaRgbYuvK k;
};

// src_fmt: kSrcRgb24 (src [N,H,W,3]) or kSrcI420 / kSrcNv12 (src [N,3H/2,W], converted by the horizontal pass's loader with yk)
hipError_t rsz_launch(int src_fmt, const NcaYuvK& yk, const unsigned char* src, int N, int H, int W, int x0, int y0, int cw, int ch, const int* kx,
                      const int* bx, int ksize_x, const int* ky, const int* by, int ksize_y, unsigned char* dst, int out_h, int out_w,
                      unsigned char* tmp, hipStream_t st, const RszPlanar& planar = RszPlanar{}) {
    const bool yuv = src_fmt != kSrcRgb24;
    // horizontal pass: the widest block of columns whose coefficient rows and one staged source row fit the LDS budget, then as many rows
    int cols = out_w < kRszMaxCols ? out_w : kRszMaxCols, fp = 0, row_dw = 0, ydw = 0, cdw = 0;
    size_t row_bytes = 0;                                 // LDS per row: the RGB row, and a planar source's staged segments
    for (;; cols = (cols + 1) / 2) {
        fp = rsz_footprint(cols, cw, out_w, ksize_x);
        row_dw = rsz_row_dwords(fp);
        ydw = yuv ? rsz_yuv_luma_dwords(fp) : 0;
        cdw = yuv ? rsz_yuv_chroma_dwords(fp) : 0;
        row_bytes = ((size_t)row_dw + ydw + 2 * (size_t)cdw) * 4;
        if (cols == 1 || (size_t)cols * ksize_x * 4 + row_bytes <= (size_t)kRszLdsBudget) break;
    }
    const size_t kbytes = (size_t)cols * ksize_x * 4;
    if (kbytes + row_bytes > (size_t)kRszLdsBudget) return hipErrorInvalidValue;     // the caller's limits (16384, 2048) keep this away
    int rows = (int)(((size_t)kRszLdsBudget - kbytes) / row_bytes);
    rows = rows < kRszMaxRows ? rows : kRszMaxRows;
    rows = rows < ch ? rows : ch;
    const int col_blocks = (out_w + cols - 1) / cols, bands = (ch + rows - 1) / rows;
    const size_t lds = kbytes + (size_t)rows * row_bytes;
    const size_t frame = yuv ? (size_t)H * W / 2 * 3 : (size_t)H * W * 3;
    const size_t total = (size_t)N * frame;
    const int rowlen = out_w * 3;
    const bool vec = rowlen % 4 == 0 && ((uintptr_t)tmp & 3) == 0 && ((uintptr_t)dst & 3) == 0;
    const int per_block = kRszThreads * (vec ? 4 : 1);
    const auto hk = src_fmt == kSrcI420 ? resize_h_kernel<kSrcI420> : src_fmt == kSrcNv12 ? resize_h_kernel<kSrcNv12> : resize_h_kernel<kSrcRgb24>;
    for (int n0 = 0; n0 < N; n0 += 65535) {              // grid y / z hold at most 65535 frames
        const int nn = N - n0 < 65535 ? N - n0 : 65535;
        // the frames of this chunk start at src + n0 frames, but the dword loader needs the whole tensor's extent: pass the chunk's
        // own base and the bytes from there to the tensor's end
        const unsigned char* s = src + (size_t)n0 * frame;
        unsigned char* t = tmp + (size_t)n0 * ch * rowlen;
        unsigned char* d = dst + (size_t)n0 * out_h * (planar.on ? (size_t)out_w / 2 * 3 : (size_t)rowlen);
        hipLaunchKernelGGL(hk, dim3((unsigned)(col_blocks * bands), (unsigned)nn), dim3(kRszThreads), lds, st, s, total - (size_t)n0 * frame, H, W, x0,
                           y0, cw, ch, kx, bx, ksize_x, t, out_w, cols, rows, fp, row_dw, col_blocks, yk, ydw, cdw);
        if (hipError_t e = hipGetLastError()) return e;
        if (planar.on) {
            const int lanes = (out_w + kYuvOutCols - 1) / kYuvOutCols;
            const dim3 pgrid((unsigned)((lanes + kYuvOutThreads - 1) / kYuvOutThreads), (unsigned)(out_h / 2), (unsigned)nn);
            const size_t tbytes = (size_t)nn * ch * rowlen;
            if (planar.nv12)
                hipLaunchKernelGGL(resize_v_yuv420_kernel<true>, pgrid, dim3(kYuvOutThreads), 0, st, t, tbytes, ch, ky, by, ksize_y, d, out_h, out_w,
                                   planar.k);
            else
                hipLaunchKernelGGL(resize_v_yuv420_kernel<false>, pgrid, dim3(kYuvOutThreads), 0, st, t, tbytes, ch, ky, by, ksize_y, d, out_h, out_w,
                                   planar.k);
            if (hipError_t e = hipGetLastError()) return e;
            continue;
        }
        const dim3 grid((unsigned)((rowlen + per_block - 1) / per_block), (unsigned)out_h, (unsigned)nn);
        if (vec)
            hipLaunchKernelGGL(resize_v_kernel<4>, grid, dim3(kRszThreads), 0, st, t, ch, ky, by, ksize_y, d, out_h, rowlen);
        else
            hipLaunchKernelGGL(resize_v_kernel<1>, grid, dim3(kRszThreads), 0, st, t, ch, ky, by, ksize_y, d, out_h, rowlen);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t nca_launch_clip_resize(const unsigned char* src, int N, int H, int W, int x0, int y0, int cw, int ch, const int* kx, const int* bx,
                                  int ksize_x, const int* ky, const int* by, int ksize_y, unsigned char* dst, int out_h, int out_w,
                                  unsigned char* tmp, hipStream_t st) {
    return rsz_launch(kSrcRgb24, NcaYuvK{}, src, N, H, W, x0, y0, cw, ch, kx, bx, ksize_x, ky, by, ksize_y, dst, out_h, out_w, tmp, st);
}

hipError_t nca_launch_clip_resize_yuv420(const unsigned char* src, bool nv12, const int* k, int N, int H, int W, int x0, int y0, int cw, int ch,
                                         const int* kx, const int* bx, int ksize_x, const int* ky, const int* by, int ksize_y, unsigned char* dst,
                                         int out_h, int out_w, unsigned char* tmp, hipStream_t st) {
    return rsz_launch(nv12 ? kSrcNv12 : kSrcI420, NcaYuvK{k[0], k[1], k[2], k[3], k[4], k[5]}, src, N, H, W, x0, y0, cw, ch, kx, bx, ksize_x, ky, by,
                      ksize_y, dst, out_h, out_w, tmp, st);
}

hipError_t nca_launch_clip_resize_u8_yuv420(const unsigned char* src, int N, int H, int W, int x0, int y0, int cw, int ch, const int* kx,
                                            const int* bx, int ksize_x, const int* ky, const int* by, int ksize_y, bool nv12, const int* k,
                                            unsigned char* dst, int out_h, int out_w, unsigned char* tmp, hipStream_t st) {
    const RszPlanar planar{true, nv12, NcaRgbYuvK{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9]}};
    return rsz_launch(kSrcRgb24, NcaYuvK{}, src, N, H, W, x0, y0, cw, ch, kx, bx, ksize_x, ky, by, ksize_y, dst, out_h, out_w, tmp, st, planar);
}

// ---- the table builder: plain host C++, no GPU call.  ImagingResample's precompute_coeffs + normalize_coeffs_8bpc in C double, with
// contraction off so that a host FMA cannot move a coefficient. ----
#pragma clang fp contract(off)

namespace {

double rsz_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

double rsz_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return std::sin(x) / x;
}

double rsz_lanczos(double x) {
    if (-3.0 <= x && x < 3.0) return rsz_sinc(x) * rsz_sinc(x / 3);
    return 0.0;
}

double rsz_support(int filter) { return filter == 1 ? 3.0 : 2.0; }

}  // namespace

int nca_resize_ksize(int in, int out, int filter) {
    double fs = (double)in / (double)out;
    if (fs < 1.0) fs = 1.0;
    const double ks = std::ceil(rsz_support(filter) * fs) * 2 + 1;
    return ks > 2147483647.0 ? -1 : (int)ks;
}

// k [out, ksize] and bounds [out, 2] = (xmin, n).  Returns 0, or the 1-based row whose coefficients break an integer bound of the passes
// (|k| < 2^23; 255 * sum |k| + 2^21 < 2^31).
int nca_resize_build_tables(int in, int out, int filter, int32_t* k, int32_t* bounds, int ksize) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double sup = rsz_support(filter) * fs;
    const double ss = 1.0 / fs;
    int bad = 0;
    double* const w = new double[ksize];
    for (int i = 0; i < out; ++i) {
        const double center = (i + 0.5) * scale;
        int xmin = (int)(center - sup + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + sup + 0.5);
        if (xmax > in) xmax = in;
        int n = xmax - xmin;
        if (n > ksize) n = ksize;          // cannot happen: n <= 2 * ceil(sup) + 1
        double ww = 0.0;
        for (int j = 0; j < n; ++j) {
            w[j] = filter == 1 ? rsz_lanczos((j + xmin - center + 0.5) * ss) : rsz_bicubic((j + xmin - center + 0.5) * ss);
            ww += w[j];
        }
        int32_t* const kr = k + (size_t)i * ksize;
        long long sum_abs = 0;
        for (int j = 0; j < n; ++j) {
            if (ww != 0.0) w[j] /= ww;
            const double v = w[j] * (double)(1 << 22);
            kr[j] = v < 0 ? (int)(-0.5 + v) : (int)(0.5 + v);
            const long long m = kr[j] < 0 ? -(long long)kr[j] : (long long)kr[j];
            if (m >= (1 << 23)) bad = bad ? bad : i + 1;
            sum_abs += m;
        }
        for (int j = n; j < ksize; ++j) kr[j] = 0;
        if (255 * sum_abs + (1 << 21) >= (1ll << 31)) bad = bad ? bad : i + 1;
        bounds[2 * i] = xmin;
        bounds[2 * i + 1] = n;
    }
    delete[] w;
    return bad;
}

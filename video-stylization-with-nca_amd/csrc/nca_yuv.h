// nca_yuv.h -- what nca_yuv.hip (the conversion launch) and nca_resize.hip (the loader of the horizontal resize pass) share: the integer
// YUV -> RGB evaluation of include/ncahip.h, the byte packing of four results and the aligned-dword staging of a byte segment -- and what
// nca_yuv_out.hip (RGB24 -> planar YUV) and the planar emit of nca_clip.hip share: the RGB -> YUV evaluation and the writer of a lane's block.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

// ncahip_yuv_coeffs' six words, by value in the kernel arguments
struct NcaYuvK {
    int ky, krv, kgu, kgv, kbu, yoff;
};

// Four bytes (each already 0 .. 255) -> one dword.  For clamp(a0 >> s) | clamp(a1 >> s) << 8 the compiler selects v_ashr_pk_u8_i32 and ORs
// bytes 2 and 3 into its result as if the instruction had cleared bits 16..31 of its destination; on the MI355X those bits keep what the
// register held before (observed: bytes 2 and 3 of every dword came out ORed with bits of the address that had lived there).  The empty asm
// statement (no instruction, no memory access) makes the two low bytes opaque, so the fused form is not selected.
__device__ __forceinline__ unsigned nca_pack_u8x4(unsigned b0, unsigned b1, unsigned b2, unsigned b3) {
    asm volatile("" : "+v"(b0), "+v"(b1));
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

__device__ __forceinline__ int nca_yuv_u8(int acc) { return min(max((acc + (1 << 15)) >> 16, 0), 255); }

// channel c (0 = R, 1 = G, 2 = B) of one pixel: clamp((k_y y' + k_u u' + k_v v' + 2^15) >> 16, 0, 255), int32, arithmetic shift
__device__ __forceinline__ int nca_yuv_channel(const NcaYuvK& k, int Y, int U, int V, int c) {
    const int yy = k.ky * (Y - k.yoff), u = U - 128, v = V - 128;
    return nca_yuv_u8(c == 0 ? yy + k.krv * v : c == 1 ? yy + k.kgu * u + k.kgv * v : yy + k.kbu * u);
}

// ---- the other direction (nca_yuv_out.hip, the planar emit of nca_clip.hip): RGB bytes -> planar YUV 4:2:0 ----
// ncahip_rgb_yuv_coeffs' ten words, by value in the kernel arguments: the (R, G, B) rows of Y, U and V, then the luma offset
struct NcaRgbYuvK {
    int yr, yg, yb, ur, ug, ub, vr, vg, vb, yoff;
};

constexpr int kYuvOutCols = 4;      // a lane owns 2 rows x 4 columns: one dword of luma per row and 2 + 2 chroma bytes
constexpr int kYuvOutThreads = 64;  // one wave per workgroup: a 256 x 256 image is 16384 lanes, spread over every CU

// luma of one pixel: clamp(yoff + ((k_yr R + k_yg G + k_yb B + 2^15) >> 16), 0, 255)
__device__ __forceinline__ unsigned nca_rgb_luma(const NcaRgbYuvK& k, int r, int g, int b) {
    return (unsigned)min(max(k.yoff + ((k.yr * r + k.yg * g + k.yb * b + (1 << 15)) >> 16), 0), 255);
}

// one chroma sample from a 2 x 2 block's channel sums (0 .. 1020): clamp(128 + ((k_r sr + k_g sg + k_b sb + 2^17) >> 18), 0, 255)
__device__ __forceinline__ unsigned nca_rgb_chroma(int kr, int kg, int kb, int sr, int sg, int sb) {
    return (unsigned)min(max(128 + ((kr * sr + kg * sg + kb * sb + (1 << 17)) >> 18), 0), 255);
}

// The low n (2 or 4) bytes of v to p: one dword where p is 4-byte aligned and n == 4, else 16-bit halves where p is 2-byte aligned, else
// single bytes (a plane or a row that starts on an odd address: the image pointer's alignment forces them)
__device__ __forceinline__ void nca_store_u8_seg(unsigned char* __restrict__ p, unsigned v, int n) {
    const unsigned mis = (unsigned)((uintptr_t)p & 3);
    if (n == 4 && mis == 0) {
        *reinterpret_cast<unsigned*>(p) = v;
    } else if ((mis & 1) == 0) {
        for (int i = 0; i < n; i += 2) *reinterpret_cast<unsigned short*>(p + i) = (unsigned short)(v >> (8 * i));
    } else {
        for (int i = 0; i < n; ++i) p[i] = (unsigned char)(v >> (8 * i));
    }
}

// The lane's block of image n: rows y, y + 1 and columns x0 .. x0 + nv - 1 (nv = 2 at the end of a row whose W is no multiple of 4, else
// 4; x0 a multiple of 4) from its truncated RGB bytes r/g/b[row][column] to `out` [N, 3H/2, W].  Columns at and above nv hold anything:
// nothing of them is stored.
template <bool NV12>
__device__ __forceinline__ void nca_yuv420_store_block(unsigned char* __restrict__ out, const NcaRgbYuvK& k, size_t n, int H, int W, int y, int x0,
                                                       int nv, const int (&r)[2][kYuvOutCols], const int (&g)[2][kYuvOutCols],
                                                       const int (&b)[2][kYuvOutCols]) {
    const size_t plane = (size_t)H * W;
    unsigned char* const frame = out + n * (plane + plane / 2);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        unsigned yy[kYuvOutCols];
#pragma unroll
        for (int i = 0; i < kYuvOutCols; ++i) yy[i] = nca_rgb_luma(k, r[j][i], g[j][i], b[j][i]);
        nca_store_u8_seg(frame + (size_t)(y + j) * W + x0, nca_pack_u8x4(yy[0], yy[1], yy[2], yy[3]), nv);
    }
    unsigned u[2], v[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int sr = r[0][2 * i] + r[0][2 * i + 1] + r[1][2 * i] + r[1][2 * i + 1];
        const int sg = g[0][2 * i] + g[0][2 * i + 1] + g[1][2 * i] + g[1][2 * i + 1];
        const int sb = b[0][2 * i] + b[0][2 * i + 1] + b[1][2 * i] + b[1][2 * i + 1];
        u[i] = nca_rgb_chroma(k.ur, k.ug, k.ub, sr, sg, sb);
        v[i] = nca_rgb_chroma(k.vr, k.vg, k.vb, sr, sg, sb);
    }
    if (NV12) {      // h/2 rows of w bytes, U and V interleaved: one dword per lane
        nca_store_u8_seg(frame + plane + (size_t)(y >> 1) * W + x0, nca_pack_u8x4(u[0], v[0], u[1], v[1]), nv);
    } else {         // the U plane (h/2 x w/2), then the V plane: two bytes of each per lane
        unsigned char* const pu = frame + plane + (size_t)(y >> 1) * (W >> 1) + (x0 >> 1);
        if (nv == 4) {
            nca_store_u8_seg(pu, nca_pack_u8x4(u[0], u[1], 0u, 0u), 2);
            nca_store_u8_seg(pu + plane / 4, nca_pack_u8x4(v[0], v[1], 0u, 0u), 2);
        } else {
            pu[0] = (unsigned char)u[0];
            pu[plane / 4] = (unsigned char)v[0];
        }
    }
}

// Dword `d` of the memory-aligned dwords that cover bytes first .. first + len - 1 of `src` (a tensor of `total` bytes whose address is
// `mis` mod 4): false past the segment's end; a dword that straddles an end of the tensor is put together from its bytes inside.  The
// segment's first byte sits at byte (first + mis) & 3 of dword 0.
__device__ __forceinline__ bool nca_stage_dword(const unsigned char* __restrict__ src, size_t total, uintptr_t mis, size_t first, size_t len, int d,
                                                unsigned& v) {
    const ptrdiff_t a = (ptrdiff_t)((first + mis) & ~(size_t)3) - (ptrdiff_t)mis + 4 * (ptrdiff_t)d;   // aligned in memory; >= -3
    if (a >= (ptrdiff_t)(first + len)) return false;
    if (a >= 0 && (size_t)a + 4 <= total) {
        v = *reinterpret_cast<const unsigned*>(src + a);
    } else {
        v = 0u;
        for (int k = 0; k < 4; ++k)
            if (a + k >= 0 && (size_t)(a + k) < total) v |= (unsigned)src[a + k] << (8 * k);
    }
    return true;
}

// One byte of `src` through the aligned dword that holds it (never a byte outside the tensor)
__device__ __forceinline__ int nca_load_u8_dw(const unsigned char* __restrict__ src, size_t total, uintptr_t mis, size_t off) {
    unsigned v = 0u;
    nca_stage_dword(src, total, mis, off, 1, 0, v);
    return (int)((v >> (8 * (unsigned)((off + mis) & 3))) & 255u);
}

// nca_yuv.h -- what nca_yuv.hip (the conversion launch) and nca_resize.hip (the loader of the horizontal resize pass) share: the integer
// YUV -> RGB evaluation of include/ncahip.h, the byte packing of four results and the aligned-dword staging of a byte segment.
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

// nca_clip_u8.h -- the uint8 frame loader the clip front ends share (nca_clip.hip: clip_cond_kernel, clip_gray_kernel; nca_encoder.hip:
// clip_encode_kernel): rows of a [N,H,W,3] uint8 tensor into LDS as memory-aligned dwords, and the bytes of one pixel out of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kClipStageCols = 66;                                // the widest row segment a caller stages (pixels)
constexpr int kRawDwords = (3 * kClipStageCols + 3 + 3) / 4 + 1;  // aligned dwords that cover one such row of uint8 RGB (198 bytes at any phase)

// uint8 RGB rows into LDS as memory-aligned dwords: ROWS row segments (image rows y_first .. y_first + ROWS - 1 of image n, columns
// [cx0, cx1), at most kClipStageCols of them) of a [N,H,W,3] tensor of `total` bytes, kRawDwords dwords per staged row.  The dwords are
// aligned in memory, whatever the tensor's own alignment or W * 3; one that straddles an end of the tensor is assembled from its bytes inside.
template <int ROWS>
__device__ __forceinline__ void clip_stage_u8_rows(const unsigned char* base, size_t total, size_t n, size_t plane, int H, int W, int y_first,
                                                   int cx0, int cx1, unsigned* raw, int tid) {
    const uintptr_t mis = (uintptr_t)base & 3;
    for (int i = tid; i < ROWS * kRawDwords; i += 256) {
        const int r = i / kRawDwords, d = i % kRawDwords;
        const int y = y_first + r;
        if (y < 0 || y >= H) continue;
        const size_t first = (n * plane + (size_t)y * W + cx0) * 3;          // first byte of the row segment
        const size_t last = first + (size_t)(cx1 - cx0) * 3;                 // one past its last byte
        const ptrdiff_t a0 = (ptrdiff_t)((first + mis) & ~(size_t)3) - (ptrdiff_t)mis;   // aligned start, as an offset from base (>= -3)
        const ptrdiff_t a = a0 + 4 * (ptrdiff_t)d;
        if (a >= (ptrdiff_t)last) continue;
        unsigned v;
        if (a >= 0 && (size_t)a + 4 <= total) {
            v = *reinterpret_cast<const unsigned*>(base + a);
        } else {   // the dword straddles an end of the tensor: only its bytes inside
            v = 0u;
            for (int k = 0; k < 4; ++k)
                if (a + k >= 0 && (size_t)(a + k) < total) v |= (unsigned)base[a + k] << (8 * k);
        }
        raw[r * kRawDwords + d] = v;
    }
}

// the three bytes of pixel (y, x) of image n in the rows clip_stage_u8_rows staged (r: its staged row, cx0: the first staged column)
__device__ __forceinline__ const unsigned char* clip_staged_u8_pixel(const unsigned char* base, const unsigned* raw, int r, size_t n, size_t plane,
                                                                     int W, int y, int x, int cx0) {
    const uintptr_t mis = (uintptr_t)base & 3;
    const size_t first = (n * plane + (size_t)y * W + cx0) * 3;
    const int off = (int)((first + mis) & 3) + 3 * (x - cx0);            // byte of this pixel within the staged row
    return reinterpret_cast<const unsigned char*>(raw) + (size_t)r * kRawDwords * 4 + off;
}

}  // namespace

// nca_gram_bf16.hip -- the layer-1 weight-gradient product of the DyNCA backward over bf16 operands (gfx950, v_mfma_f32_16x16x32_bf16):
//     out[i][j] = sum_n a[i][n] * b[j][n],   out[ma*nb + i] = sum_n a[i][n]         (n = all B*HW cells, the K axis)
// a [B, ma, HW] and b1 [B, nb1, HW] hold bf16, b2 [B, nb2, HW] holds fp32 and is rounded to bf16 (RNE) as it is loaded (the
// conditioning map).  The cell axis is K, so with channel-major buffers the eight consecutive k of a lane ARE one 16-byte load: both
// operands go from memory straight into the MFMA, no LDS.  Products of two bf16 values are exact in fp32; all that differs from exact
// arithmetic is the fp32 summation, whose order is fixed (per-workgroup partials, then nca_launch_reduce_rows): deterministic.
// The row sums ride on the MFMA as column nb of ones.  gram_rows_bf16_kernel covers ma <= 128, nb <= 79 in one workgroup per chunk walk;
// gram_rows_bf16_wide_kernel tiles ma <= 256, nb <= 132 over blocks of that size (the wide range of the bf16-MFMA training mode).
#include "nca_common.h"
#include "nca_kernels.h"

namespace {

constexpr int kGramBfThreads = 256, kGramBfChunk = 32;

struct GramBfArgs {
    const uint16_t* a;    // [B, ma, HW] bf16
    const uint16_t* b1;   // [B, nb1, HW] bf16
    const float* b2;      // [B, nb2, HW] fp32 or null
    float* ws;            // [grid, ma*nb + ma]
    int ma, nb1, nb2, B, HW;
};

// eight consecutive cells k0 .. k0+7 of one bf16 row; cells beyond HW read as zero
template <bool VEC>
__device__ __forceinline__ nca_u32x4 gram_load8(const uint16_t* row, int k0, int HW) {
    nca_u32x4 v{0u, 0u, 0u, 0u};
    if constexpr (VEC) {   // HW % 8 == 0 and 16-byte aligned tensors: a group of eight is inside or outside as a whole
        if (k0 < HW) v = *reinterpret_cast<const nca_u32x4*>(row + k0);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k0 + j < HW) v[j >> 1] |= (unsigned)row[k0 + j] << (16 * (j & 1));
    }
    return v;
}
template <bool VEC>
__device__ __forceinline__ nca_u32x4 gram_load8_f32(const float* row, int k0, int HW) {
    float f[8];
    if constexpr (VEC) {
        if (k0 < HW) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(row + k0), hi = *reinterpret_cast<const f32x4*>(row + k0 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = 0.0f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = k0 + j < HW ? row[k0 + j] : 0.0f;
    }
    return nca_u32x4{nca_pk_bf16(f[0], f[1]), nca_pk_bf16(f[2], f[3]), nca_pk_bf16(f[4], f[5]), nca_pk_bf16(f[6], f[7])};
}

// Wave w owns the out row tiles w and w + 4 (ma <= 128) x all NBT column tiles (nb + 1 <= 16 NBT: the last real column + 1 is the
// ones column).  A workgroup walks chunks of 32 cells, a chunk never crosses a batch item.
template <int NBT, bool VEC>
__global__ __launch_bounds__(kGramBfThreads, 2) void gram_rows_bf16_kernel(const GramBfArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, ci = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = a.nb1 + a.nb2, HW = a.HW, ma = a.ma;
    const int cpb = (HW + kGramBfChunk - 1) / kGramBfChunk, total = a.B * cpb;
    const bool second = 16 * (wave + 4) < ma;   // wave-uniform
    f32x4 acc[2][NBT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NBT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int row0 = 16 * wave + ci, row1 = 16 * (wave + 4) + ci;
    nca_u32x4 av[2][2], bv[2][NBT];
    auto issue = [&](int c, int q) {
        const int bi = c / cpb, k0 = (c - bi * cpb) * kGramBfChunk + 8 * g;
        const uint16_t* const ab = a.a + (size_t)bi * ma * HW;
        av[q][0] = row0 < ma ? gram_load8<VEC>(ab + (size_t)row0 * HW, k0, HW) : nca_u32x4{0u, 0u, 0u, 0u};
        av[q][1] = (second && row1 < ma) ? gram_load8<VEC>(ab + (size_t)row1 * HW, k0, HW) : nca_u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < NBT; ++j) {
            const int col = 16 * j + ci;
            if (col < a.nb1) bv[q][j] = gram_load8<VEC>(a.b1 + ((size_t)bi * a.nb1 + col) * HW, k0, HW);
            else if (col < nb) bv[q][j] = gram_load8_f32<VEC>(a.b2 + ((size_t)bi * a.nb2 + (col - a.nb1)) * HW, k0, HW);
            else if (col == nb) bv[q][j] = nca_u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};   // ones: a is zero beyond HW
            else bv[q][j] = nca_u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto products = [&](int q) {
#pragma unroll
        for (int j = 0; j < NBT; ++j) acc[0][j] = nca_mfma_bf16(av[q][0], bv[q][j], acc[0][j]);
        if (second) {
#pragma unroll
            for (int j = 0; j < NBT; ++j) acc[1][j] = nca_mfma_bf16(av[q][1], bv[q][j], acc[1][j]);
        }
    };
    // two chunks per trip, so that the buffer index is a literal; the next chunk's loads fly during this chunk's products
    const int G = (int)gridDim.x;
    int c = blockIdx.x;
    if (c < total) issue(c, 0);
    while (c < total) {
        if (c + G < total) issue(c + G, 1);
        products(0);
        c += G;
        if (c >= total) break;
        if (c + G < total) issue(c + G, 0);
        products(1);
        c += G;
    }
    // ---- this workgroup's partial: [ma x nb] products, then ma row sums ----------------------------------------------------------
    float* const ws = a.ws + (size_t)blockIdx.x * ((size_t)ma * nb + ma);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NBT; ++j) {
            const int col = 16 * j + ci;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * (wave + 4 * i) + 4 * g + r;
                if (o < ma && col < nb) ws[(size_t)o * nb + col] = acc[i][j][r];
                if (o < ma && col == nb) ws[(size_t)ma * nb + o] = acc[i][j][r];
            }
        }
}

// The wide product (ma <= 256, nb <= 132): the output is tiled over the kernel above's row and column tiles.  Workgroup (x, y, z) walks
// the chunks x, x + G, .. as above and owns rows 128 y .. 128 y + 127 (wave w: row tiles w and w + 4 of that block) x column tiles
// NBT z .. NBT z + NBT - 1.  The ones column (global column nb) falls into exactly one column block: the row sums are taken once.  Every
// output element is one accumulator of one workgroup per x, summed over the chunks in ascending order, then over x by
// nca_launch_reduce_rows: the order is fixed.
template <int NBT, bool VEC>
__global__ __launch_bounds__(kGramBfThreads, 2) void gram_rows_bf16_wide_kernel(const GramBfArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, ci = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = a.nb1 + a.nb2, HW = a.HW, ma = a.ma;
    const int cpb = (HW + kGramBfChunk - 1) / kGramBfChunk, total = a.B * cpb;
    const int rbase = 128 * (int)blockIdx.y, cbase = 16 * NBT * (int)blockIdx.z;
    const bool second = rbase + 16 * (wave + 4) < ma;   // wave-uniform
    f32x4 acc[2][NBT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NBT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int row0 = rbase + 16 * wave + ci, row1 = row0 + 64;
    nca_u32x4 av[2][2], bv[2][NBT];
    auto issue = [&](int c, int q) {
        const int bi = c / cpb, k0 = (c - bi * cpb) * kGramBfChunk + 8 * g;
        const uint16_t* const ab = a.a + (size_t)bi * ma * HW;
        av[q][0] = row0 < ma ? gram_load8<VEC>(ab + (size_t)row0 * HW, k0, HW) : nca_u32x4{0u, 0u, 0u, 0u};
        av[q][1] = (second && row1 < ma) ? gram_load8<VEC>(ab + (size_t)row1 * HW, k0, HW) : nca_u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < NBT; ++j) {
            const int col = cbase + 16 * j + ci;
            if (col < a.nb1) bv[q][j] = gram_load8<VEC>(a.b1 + ((size_t)bi * a.nb1 + col) * HW, k0, HW);
            else if (col < nb) bv[q][j] = gram_load8_f32<VEC>(a.b2 + ((size_t)bi * a.nb2 + (col - a.nb1)) * HW, k0, HW);
            else if (col == nb) bv[q][j] = nca_u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};   // ones: a is zero beyond HW
            else bv[q][j] = nca_u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto products = [&](int q) {
#pragma unroll
        for (int j = 0; j < NBT; ++j) acc[0][j] = nca_mfma_bf16(av[q][0], bv[q][j], acc[0][j]);
        if (second) {
#pragma unroll
            for (int j = 0; j < NBT; ++j) acc[1][j] = nca_mfma_bf16(av[q][1], bv[q][j], acc[1][j]);
        }
    };
    const int G = (int)gridDim.x;
    int c = blockIdx.x;
    if (c < total) issue(c, 0);
    while (c < total) {
        if (c + G < total) issue(c + G, 1);
        products(0);
        c += G;
        if (c >= total) break;
        if (c + G < total) issue(c + G, 0);
        products(1);
        c += G;
    }
    float* const ws = a.ws + (size_t)blockIdx.x * ((size_t)ma * nb + ma);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NBT; ++j) {
            const int col = cbase + 16 * j + ci;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = rbase + 16 * (wave + 4 * i) + 4 * g + r;
                if (o < ma && col < nb) ws[(size_t)o * nb + col] = acc[i][j][r];
                if (o < ma && col == nb) ws[(size_t)ma * nb + o] = acc[i][j][r];
            }
        }
}

template <int NBT>
hipError_t launch_gram_bf16_wide(const GramBfArgs& a, dim3 grid, bool vec, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((gram_rows_bf16_wide_kernel<NBT, true>), grid, dim3(kGramBfThreads), 0, st, a);
    else hipLaunchKernelGGL((gram_rows_bf16_wide_kernel<NBT, false>), grid, dim3(kGramBfThreads), 0, st, a);
    return hipGetLastError();
}

template <int NBT>
hipError_t launch_gram_bf16(const GramBfArgs& a, int grid, bool vec, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((gram_rows_bf16_kernel<NBT, true>), dim3(grid), dim3(kGramBfThreads), 0, st, a);
    else hipLaunchKernelGGL((gram_rows_bf16_kernel<NBT, false>), dim3(grid), dim3(kGramBfThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace

int nca_gram_bf16_grid(int B, int HW) {
    const int cus = nca_cu_count();
    const long total = (long)B * ((HW + kGramBfChunk - 1) / kGramBfChunk);
    return (int)(total < 2L * cus ? total : 2L * cus);
}

// out[ma*nb + ma] (+)= [products | row sums of a]; ws holds nca_gram_bf16_grid(B, HW) partials of that size.  ma <= 128, nb <= 79.
hipError_t nca_launch_gram_rows_bf16(const uint16_t* a, int ma, const uint16_t* b1, int nb1, const float* b2, int nb2, int B, int HW,
                                     float* out, float* ws, hipStream_t st, bool accumulate) {
    const int nb = nb1 + nb2, grid = nca_gram_bf16_grid(B, HW);
    if (ma < 1 || nb1 < 1 || nb2 < 0 || !nca_gram_bf16_fits(kNcaGramBf, ma, nb) || (nb2 > 0 && !b2)) return hipErrorInvalidValue;
    const GramBfArgs ga{a, b1, b2, ws, ma, nb1, nb2, B, HW};
    const bool vec = HW % 8 == 0 && (((uintptr_t)a | (uintptr_t)b1 | (uintptr_t)b2) & 15u) == 0;
    hipError_t e;
    switch ((nb + 16) / 16) {   // column tiles covering nb + 1 columns
        case 1: e = launch_gram_bf16<1>(ga, grid, vec, st); break;
        case 2: e = launch_gram_bf16<2>(ga, grid, vec, st); break;
        case 3: e = launch_gram_bf16<3>(ga, grid, vec, st); break;
        case 4: e = launch_gram_bf16<4>(ga, grid, vec, st); break;
        default: e = launch_gram_bf16<5>(ga, grid, vec, st); break;
    }
    if (e != hipSuccess) return e;
    return nca_launch_reduce_rows(ws, out, grid, ma * nb + ma, st, accumulate);
}

// The same up to ma <= 256, nb <= 132 (the layer-1 weight gradient of the wide bf16-MFMA backward); ws as above.  Inside the range of
// nca_launch_gram_rows_bf16 it IS that launcher.
hipError_t nca_launch_gram_rows_bf16_wide(const uint16_t* a, int ma, const uint16_t* b1, int nb1, const float* b2, int nb2, int B, int HW,
                                          float* out, float* ws, hipStream_t st, bool accumulate) {
    const int nb = nb1 + nb2, grid = nca_gram_bf16_grid(B, HW);
    if (ma < 1 || nb1 < 1 || nb2 < 0 || !nca_gram_bf16_fits(kNcaGramBfWide, ma, nb) || (nb2 > 0 && !b2)) return hipErrorInvalidValue;
    if (nca_gram_bf16_fits(kNcaGramBf, ma, nb)) return nca_launch_gram_rows_bf16(a, ma, b1, nb1, b2, nb2, B, HW, out, ws, st, accumulate);
    const GramBfArgs ga{a, b1, b2, ws, ma, nb1, nb2, B, HW};
    const bool vec = HW % 8 == 0 && (((uintptr_t)a | (uintptr_t)b1 | (uintptr_t)b2) & 15u) == 0;
    const int tiles = (nb + 16) / 16, cblocks = (tiles + 4) / 5, nbt = (tiles + cblocks - 1) / cblocks;   // column tiles covering nb + 1 columns, at most five per block
    const dim3 g3(grid, (ma + 127) / 128, cblocks);
    hipError_t e;
    switch (nbt) {
        case 1: e = launch_gram_bf16_wide<1>(ga, g3, vec, st); break;
        case 2: e = launch_gram_bf16_wide<2>(ga, g3, vec, st); break;
        case 3: e = launch_gram_bf16_wide<3>(ga, g3, vec, st); break;
        case 4: e = launch_gram_bf16_wide<4>(ga, g3, vec, st); break;
        default: e = launch_gram_bf16_wide<5>(ga, g3, vec, st); break;
    }
    if (e != hipSuccess) return e;
    return nca_launch_reduce_rows(ws, out, grid, ma * nb + ma, st, accumulate);
}

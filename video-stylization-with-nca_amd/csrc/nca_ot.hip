// nca_ot.hip -- the relaxed-EMD part of the OT appearance loss (EncoderConditioning/loss/appearance_loss.py:149-220) on gfx950.
//
// Per style layer and sample b, with x_i the N sampled feature vectors of the style target and y_j those of the generated image,
//     d_ij = 1 - <x_i, y_j> / (|x_i| + 1e-10) / (|y_j| + 1e-10),      remd = max(mean_i min_j d_ij, mean_j min_i d_ij).
// The N x N matrix is only ever reduced by row and by column, so it never exists in memory:
//   ot_gather_kernel     NCHW maps -> X, Y [B, N, c] (transpose through LDS: reads coalesced on h*w, writes on c) + the norms
//   ot_remd_fwd_kernel   one 64-row tile of X against every 64-row tile of Y on exact-f32 MFMA; row minima finished in the
//                        workgroup, column minima as one partial per 32-row band (value, index)
//   ot_remd_finish_kernel  partials combined in band order (fixed order: bit-reproducible), the two means, the max, the branch
//   ot_remd_bwd_kernel   dL/dY row by row: the backward of a min is a gather through its argmin
//   ot_scatter_kernel    adjoint of the gather (positions of a sample are distinct: plain stores)
// Ties resolve to the lowest index in both directions: every comparison is on (value, index) pairs, or strict `<` while walking
// indices upwards.  The distance uses reciprocal scales, d = 1 - <x, y> * rx_i * ry_j with rx = 1 / (|x| + 1e-10): three roundings
// of a value <= 1 instead of two divisions per entry (~1e-7 absolute; equal vectors still give equal distances).
#include "nca_common.h"
#include "nca_kernels.h"

namespace {

constexpr int kOtThreads = 256, kOtTile = 64, kOtKC = 32, kOtLS = 36;   // LDS row stride 36 floats: 16-byte aligned rows, and the 16 rows a
                                                                        // ds_read_b128 touches start at 16 distinct 4-bank groups (36 i mod 64)
constexpr float kOtEps = 1e-10f;

__device__ __forceinline__ bool ot_less(float v, int i, float ov, int oi) { return ov < v || (ov == v && oi < i); }

// ---- gather / normalise -------------------------------------------------------------------------------------------------------
// grid (ceil(N / 64), B, 2): z = 0 the target map t [1, c, HW] -> x, z = 1 the generated maps g [B, c, HW] -> y.
__global__ __launch_bounds__(kOtThreads) void ot_gather_kernel(const float* __restrict__ t, const float* __restrict__ g,
                                                               const int* __restrict__ idx, float* __restrict__ x, float* __restrict__ y,
                                                               float* __restrict__ xn, float* __restrict__ yn, int c, int HW, int N) {
    __shared__ float tile[kOtTile][kOtTile + 1];
    __shared__ float part[4][kOtTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, which = blockIdx.z;
    const float* const src = which ? g + (size_t)b * c * HW : t;
    float* const dst = (which ? y : x) + (size_t)b * N * c;
    const int n0 = blockIdx.x * kOtTile, n = n0 + lane;
    int pos = 0;
    if (n < N) pos = idx ? min(max(idx[(size_t)b * N + n], 0), HW - 1) : min(n, HW - 1);
    float ss = 0.0f;
    for (int c0 = 0; c0 < c; c0 += kOtTile) {
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {                      // lane = position: the h*w axis is the contiguous one
            const int ch = c0 + wave + 4 * k;
            const float v = (ch < c && n < N) ? src[(size_t)ch * HW + pos] : 0.0f;
            tile[wave + 4 * k][lane] = v;
            ss += v * v;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {                      // lane = channel: the c axis is the contiguous one
            const int p = wave + 4 * k, ch = c0 + lane;
            if (n0 + p < N && ch < c) dst[(size_t)(n0 + p) * c + ch] = tile[lane][p];
        }
        __syncthreads();
    }
    part[wave][lane] = ss;
    __syncthreads();
    if (wave == 0 && n < N) ((which ? yn : xn) + (size_t)b * N)[n] = sqrtf((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]));
}

// dg [B, c, HW] (zeroed by the caller when idx != null) <- dy [B, N, c]; grid (ceil(N / 64), B)
__global__ __launch_bounds__(kOtThreads) void ot_scatter_kernel(const float* __restrict__ dy, const int* __restrict__ idx,
                                                                float* __restrict__ dg, int c, int HW, int N) {
    __shared__ float tile[kOtTile][kOtTile + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int n0 = blockIdx.x * kOtTile, n = n0 + lane;
    int pos = 0;
    if (n < N) pos = idx ? min(max(idx[(size_t)b * N + n], 0), HW - 1) : min(n, HW - 1);
    const float* const src = dy + (size_t)b * N * c;
    float* const dst = dg + (size_t)b * c * HW;
    for (int c0 = 0; c0 < c; c0 += kOtTile) {
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int p = wave + 4 * k, ch = c0 + lane;
            tile[p][lane] = (n0 + p < N && ch < c) ? src[(size_t)(n0 + p) * c + ch] : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int ch = c0 + wave + 4 * k;
            if (ch < c && n < N) dst[(size_t)ch * HW + pos] = tile[lane][wave + 4 * k];
        }
        __syncthreads();
    }
}

// ---- relaxed EMD forward --------------------------------------------------------------------------------------------------------
// grid (ceil(N / 64), B).  Workgroup (rt, b) owns rows [64 rt, 64 rt + 64) of sample b and walks every 64-column tile; wave
// (wr, wc) owns the 32 x 32 quadrant (2 x 2 MFMA tiles).  K runs in chunks of 32 staged through LDS (next chunk's global loads in
// flight during this chunk's products).  Lane l = 16 g + i reads its operands as float4 at k = 16 s + 4 g + {0..3}: the four
// values feed four successive MFMAs, so one MFMA contracts k in {16 s + t, +4, +8, +12} -- A and B agree, the sum is complete.
__global__ __launch_bounds__(kOtThreads, 2) void ot_remd_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                   const float* __restrict__ xn, const float* __restrict__ yn,
                                                                   float* __restrict__ rmin, int* __restrict__ rarg,
                                                                   float* __restrict__ cminp, int* __restrict__ cargp, int N, int c) {
    __shared__ __attribute__((aligned(16))) float xs[kOtTile * kOtLS];
    __shared__ __attribute__((aligned(16))) float ys[kOtTile * kOtLS];
    __shared__ float redv[2][kOtTile];
    __shared__ int redi[2][kOtTile];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15;
    const int wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int b = blockIdx.y, rt = blockIdx.x, r0 = rt * kOtTile;
    const int nct = (N + kOtTile - 1) / kOtTile, nk = (c + kOtKC - 1) / kOtKC, P = 2 * nct;
    const float* const xb = x + (size_t)b * N * c;
    const float* const yb = y + (size_t)b * N * c;
    const float* const xnb = xn + (size_t)b * N;
    const float* const ynb = yn + (size_t)b * N;

    // staging: the 64 x 32 chunk is 512 float4; thread tid carries #tid and #tid + 256 (rows tid / 8 and 32 + tid / 8)
    const int srow = tid >> 3, sq = (tid & 7) * 4;
    const size_t xoff0 = (size_t)min(r0 + srow, N - 1) * c, xoff1 = (size_t)min(r0 + 32 + srow, N - 1) * c;   // rows beyond N: copies, masked below
    float4 px0, px1, py0, py1;
    auto issue = [&](int ct, int kc) {
        const int k = kc * kOtKC + sq;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < c) {                                        // c % 4 == 0: a float4 is inside the row or wholly beyond it
            px0 = *reinterpret_cast<const float4*>(xb + xoff0 + k);
            px1 = *reinterpret_cast<const float4*>(xb + xoff1 + k);
            py0 = *reinterpret_cast<const float4*>(yb + (size_t)min(ct * kOtTile + srow, N - 1) * c + k);
            py1 = *reinterpret_cast<const float4*>(yb + (size_t)min(ct * kOtTile + 32 + srow, N - 1) * c + k);
        } else {
            px0 = px1 = py0 = py1 = z;
        }
    };

    float rx[2][4], rv[2][4];
    int ri_[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rx[a][r] = 1.0f / (xnb[min(r0 + 32 * wr + 16 * a + 4 * g + r, N - 1)] + kOtEps);
            rv[a][r] = __builtin_huge_valf();
            ri_[a][r] = 0;
        }
    }

    issue(0, 0);
    for (int ct = 0; ct < nct; ++ct) {
        const int cb = ct * kOtTile + 32 * wc;
        float ry[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) ry[j] = 1.0f / (ynb[min(cb + 16 * j + i, N - 1)] + kOtEps);
        f32x4 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int kc = 0; kc < nk; ++kc) {
            *reinterpret_cast<float4*>(xs + srow * kOtLS + sq) = px0;
            *reinterpret_cast<float4*>(xs + (32 + srow) * kOtLS + sq) = px1;
            *reinterpret_cast<float4*>(ys + srow * kOtLS + sq) = py0;
            *reinterpret_cast<float4*>(ys + (32 + srow) * kOtLS + sq) = py1;
            __syncthreads();
            if (kc + 1 < nk) issue(ct, kc + 1);
            else if (ct + 1 < nct) issue(ct + 1, 0);
            const float* const ar = xs + (32 * wr + i) * kOtLS + 4 * g;
            const float* const br = ys + (32 * wc + i) * kOtLS + 4 * g;
#pragma unroll
            for (int s = 0; s < kOtKC / 16; ++s) {
                float4 av[2], bv[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) av[a] = *reinterpret_cast<const float4*>(ar + 16 * a * kOtLS + 16 * s);
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const float4*>(br + 16 * j * kOtLS + 16 * s);
                const float af[2][4] = {{av[0].x, av[0].y, av[0].z, av[0].w}, {av[1].x, av[1].y, av[1].z, av[1].w}};
                const float bf[2][4] = {{bv[0].x, bv[0].y, bv[0].z, bv[0].w}, {bv[1].x, bv[1].y, bv[1].z, bv[1].w}};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[a][j] = nca_mfma(af[a][q], bf[j][q], acc[a][j]);
                    }
                }
            }
            __syncthreads();
        }
        // ---- this tile's distances: acc[a][j][r] = <x_row, y_col>, row = r0 + 32 wr + 16 a + 4 g + r, col = cb + 16 j + i ----
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = cb + 16 * j + i;
            const bool cok = col < N;
            float cv = __builtin_huge_valf();
            int cix = 0;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + 32 * wr + 16 * a + 4 * g + r;
                    const float d = 1.0f - acc[a][j][r] * rx[a][r] * ry[j];
                    if (cok && d < rv[a][r]) {               // columns come in increasing order for a lane: strict < keeps the lowest
                        rv[a][r] = d;
                        ri_[a][r] = col;
                    }
                    if (row < N && d < cv) {                 // rows too
                        cv = d;
                        cix = row;
                    }
                }
            }
#pragma unroll
            for (int m = 16; m <= 32; m <<= 1) {
                const float ov = __shfl_xor(cv, m);
                const int oi = __shfl_xor(cix, m);
                if (ot_less(cv, cix, ov, oi)) {
                    cv = ov;
                    cix = oi;
                }
            }
            if (g == 0 && cok) {                             // the partial of row band 2 rt + wr
                const size_t o = ((size_t)b * P + 2 * rt + wr) * N + col;
                cminp[o] = cv;
                cargp[o] = cix;
            }
        }
    }
    // ---- row minima: across the 16 lanes of a row, then across the two column halves ----
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = rv[a][r];
            int ix = ri_[a][r];
#pragma unroll
            for (int m = 1; m <= 8; m <<= 1) {
                const float ov = __shfl_xor(v, m);
                const int oi = __shfl_xor(ix, m);
                if (ot_less(v, ix, ov, oi)) {
                    v = ov;
                    ix = oi;
                }
            }
            if (i == 0) {
                redv[wc][32 * wr + 16 * a + 4 * g + r] = v;
                redi[wc][32 * wr + 16 * a + 4 * g + r] = ix;
            }
        }
    }
    __syncthreads();
    if (tid < kOtTile && r0 + tid < N) {
        float v = redv[0][tid];
        int ix = redi[0][tid];
        if (ot_less(v, ix, redv[1][tid], redi[1][tid])) {
            v = redv[1][tid];
            ix = redi[1][tid];
        }
        rmin[(size_t)b * N + r0 + tid] = v;
        rarg[(size_t)b * N + r0 + tid] = ix;
    }
}

// grid B: column partials in band order (bands cover increasing rows: strict < keeps the lowest row), then the two means in a
// fixed tree, remd = max, branch = 0 (rows won) / 1 (columns won) / 2 (equal: torch.maximum splits the gradient in halves).
__global__ __launch_bounds__(kOtThreads) void ot_remd_finish_kernel(const float* __restrict__ rmin, const float* __restrict__ cminp,
                                                                    const int* __restrict__ cargp, float* __restrict__ cmin,
                                                                    int* __restrict__ carg, float* __restrict__ remd,
                                                                    int* __restrict__ branch, int N, int P) {
    __shared__ float sr[kOtThreads], sc[kOtThreads];
    const int tid = threadIdx.x, b = blockIdx.x;
    float ar = 0.0f, ac = 0.0f;
    for (int j = tid; j < N; j += kOtThreads) {
        float v = __builtin_huge_valf();
        int ix = 0;
        for (int p = 0; p < P; ++p) {
            const size_t o = ((size_t)b * P + p) * N + j;
            const float pv = cminp[o];
            if (pv < v) {
                v = pv;
                ix = cargp[o];
            }
        }
        cmin[(size_t)b * N + j] = v;
        carg[(size_t)b * N + j] = ix;
        ac += v;
        ar += rmin[(size_t)b * N + j];
    }
    sr[tid] = ar;
    sc[tid] = ac;
    __syncthreads();
    for (int s = kOtThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            sr[tid] += sr[tid + s];
            sc[tid] += sc[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float mr = sr[0] / (float)N, mc = sc[0] / (float)N;
        remd[b] = (mr != mr || mc != mc) ? __builtin_nanf("") : fmaxf(mr, mc);
        branch[b] = mr > mc ? 0 : (mc > mr ? 1 : 2);
    }
}

// ---- relaxed EMD backward -------------------------------------------------------------------------------------------------------
// grid (ceil(N / 4), B): one wave per output row j, lane l holds channels 4 l .. 4 l + 3 and 256 + 4 l .. (c <= 512).
//   d d_ij / d y_j = -xh / s + <xh, y_j> y_j / (|y_j| s^2),   xh = x_i / (|x_i| + 1e-10),  s = |y_j| + 1e-10;  |y_j| = 0: second term 0.
__global__ __launch_bounds__(kOtThreads) void ot_remd_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 const float* __restrict__ xn, const float* __restrict__ yn,
                                                                 const int* __restrict__ rarg, const int* __restrict__ carg,
                                                                 const int* __restrict__ branch, const float* __restrict__ gup,
                                                                 float* __restrict__ dy, int N, int c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int j = blockIdx.x * 4 + wave;
    if (j >= N) return;                                       // whole waves leave; no barrier below
    const float* const xb = x + (size_t)b * N * c;
    const float* const xnb = xn + (size_t)b * N;
    const int br = branch[b];
    const float w = (br == 2 ? 0.5f : 1.0f) * gup[b] / (float)N;
    const int k0 = 4 * lane, k1 = 256 + 4 * lane;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* const yr = y + ((size_t)b * N + j) * c;
    const float4 y0 = k0 < c ? *reinterpret_cast<const float4*>(yr + k0) : z;
    const float4 y1 = k1 < c ? *reinterpret_cast<const float4*>(yr + k1) : z;
    const float ynj = yn[(size_t)b * N + j], s = ynj + kOtEps;
    float4 g0 = z, g1 = z;
    auto add_pair = [&](int ii) {
        const float* const xr = xb + (size_t)ii * c;
        const float4 x0 = k0 < c ? *reinterpret_cast<const float4*>(xr + k0) : z;
        const float4 x1 = k1 < c ? *reinterpret_cast<const float4*>(xr + k1) : z;
        float dot = (x0.x * y0.x + x0.y * y0.y) + (x0.z * y0.z + x0.w * y0.w) + ((x1.x * y1.x + x1.y * y1.y) + (x1.z * y1.z + x1.w * y1.w));
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) dot += __shfl_xor(dot, m);      // butterfly: every lane ends with the same bits
        const float rxi = 1.0f / (xnb[ii] + kOtEps);
        const float cx = -w * rxi / s;
        const float cy = ynj > 0.0f ? w * (dot * rxi) / s / s / ynj : 0.0f;
        g0.x += cx * x0.x + cy * y0.x; g0.y += cx * x0.y + cy * y0.y; g0.z += cx * x0.z + cy * y0.z; g0.w += cx * x0.w + cy * y0.w;
        g1.x += cx * x1.x + cy * y1.x; g1.y += cx * x1.y + cy * y1.y; g1.z += cx * x1.z + cy * y1.z; g1.w += cx * x1.w + cy * y1.w;
    };
    if (br != 0) add_pair(min(max(carg[(size_t)b * N + j], 0), N - 1));   // column branch: the single pair (carg[j], j)
    if (br != 1) {                                                         // row branch: every i with rarg[i] == j, in increasing i
        const int* const ra = rarg + (size_t)b * N;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int ii = i0 + lane;
            unsigned long long m = __ballot(ii < N && ra[ii] == j);
            for (int n = 0; n < 64 && m; ++n) {                           // at most 64 set bits
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                add_pair(i0 + bit);
            }
        }
    }
    float* const o = dy + ((size_t)b * N + j) * c;
    if (k0 < c) *reinterpret_cast<float4*>(o + k0) = g0;
    if (k1 < c) *reinterpret_cast<float4*>(o + k1) = g1;
}

}  // namespace

int nca_ot_bands(int N) { return 2 * ((N + kOtTile - 1) / kOtTile); }

hipError_t nca_launch_ot_gather(const float* t, const float* g, const int* idx, float* x, float* y, float* xn, float* yn, int B, int c,
                                int HW, int N, hipStream_t st) {
    hipLaunchKernelGGL(ot_gather_kernel, dim3((N + kOtTile - 1) / kOtTile, B, 2), dim3(kOtThreads), 0, st, t, g, idx, x, y, xn, yn, c, HW, N);
    return hipGetLastError();
}

hipError_t nca_launch_ot_scatter(const float* dy, const int* idx, float* dg, int B, int c, int HW, int N, hipStream_t st) {
    hipLaunchKernelGGL(ot_scatter_kernel, dim3((N + kOtTile - 1) / kOtTile, B), dim3(kOtThreads), 0, st, dy, idx, dg, c, HW, N);
    return hipGetLastError();
}

// ws: nca_ot_bands(N) * B * N floats, then as many ints
hipError_t nca_launch_ot_remd_fwd(const float* x, const float* y, const float* xn, const float* yn, float* rmin, int* rarg, float* cmin,
                                  int* carg, float* remd, int* branch, int B, int N, int c, void* ws, hipStream_t st) {
    const int P = nca_ot_bands(N);
    float* const cminp = (float*)ws;
    int* const cargp = (int*)(cminp + (size_t)P * B * N);
    hipLaunchKernelGGL(ot_remd_fwd_kernel, dim3((N + kOtTile - 1) / kOtTile, B), dim3(kOtThreads), 0, st, x, y, xn, yn, rmin, rarg, cminp, cargp, N, c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ot_remd_finish_kernel, dim3(B), dim3(kOtThreads), 0, st, rmin, cminp, cargp, cmin, carg, remd, branch, N, P);
    return hipGetLastError();
}

hipError_t nca_launch_ot_remd_bwd(const float* x, const float* y, const float* xn, const float* yn, const int* rarg, const int* carg,
                                  const int* branch, const float* gup, float* dy, int B, int N, int c, hipStream_t st) {
    hipLaunchKernelGGL(ot_remd_bwd_kernel, dim3((N + 3) / 4, B), dim3(kOtThreads), 0, st, x, y, xn, yn, rarg, carg, branch, gup, dy, N, c);
    return hipGetLastError();
}

// nca_ot_moment.hip -- the moment-matching part of the OT appearance loss (EncoderConditioning/loss/appearance_loss.py:176-192) on gfx950.
//
// Per style layer and sample b, with X, Y [N, c] the sampled feature vectors of the style target and of the generated image
// (ot_gather_kernel's output),
//     mom = mean_k |mx_k - my_k| + mean_kl |Cx_kl - Cy_kl|,    mx = column means,   Cx = (X - mx)^T (X - mx) / (N - 1).
// The centred copies of X and Y, the two c x c covariances and their difference exist only in LDS and registers:
//   ot_mom_means_kernel   mx, my [B, c] (fixed reduction order), sign(mx - my), one partial of sum_k |mx_k - my_k| per channel tile
//   ot_mom_cov_kernel     one workgroup per (sample, pair of 64-channel tiles ti <= tj): both covariance tiles on exact-f32 MFMA with
//                         K = N in chunks through LDS, centred while staging; D = (Cx - Cy) / (N - 1) in registers; out go sign(D) as
//                         int8 (both triangles) and one partial of sum |D| (off-diagonal pairs doubled)
//   ot_mom_finish_kernel  partials combined in index order into mom [B]
//   ot_mom_bwd_kernel     dY += g * (-sign(mx - my) / (c N) - 2 / ((N - 1) c^2) * (Y - my) S): an [N, c] x [c, c] product on the same
//                         MFMA, S widened from int8 while staging (S is symmetric: its rows serve as its columns)
// No atomics: every sum has one owner and a fixed order, so results are bit-reproducible from run to run.
//
// The mean.  d mom / d Y carries the projection I - 11^T / N of the centring, i.e. the closed form has a term
// -colmean_n((Y - my) S) = -(mean_n (Y - my)) S, zero in exact arithmetic.  In fp32 it is the rounding residue of my times S.  Measured
// against float64 on relu(randn + 0.3) inputs (c = 512, N = 1000; relative L2 of (Y - my) S, the product itself exact): 3.2e-7 with a
// plainly summed fp32 mean and the term dropped, 2.1e-8 with the term included.  Including it is closer, and it is the same thing as
// centring with a better mean: (Y - my - r) S with r = mean_n (Y - my).  So the means kernel makes a second pass, my <- my + r (the
// columns of Y - my then sum to zero to rounding), every consumer centres with that mean, and the backward kernel carries no
// separate correction term: the term is included, through the mean.
#include "nca_common.h"
#include "nca_kernels.h"

namespace {

constexpr int kMoThreads = 256, kMoTile = 64, kMoKC = 32;
constexpr int kMoCS = 80;    // covariance LDS row stride (floats): rows 16-byte aligned; a ds_read_b32 of lanes (g, i), g in {0, 1}, touches
                             // banks 16 g + i (80 mod 32 = 16): conflict-free
constexpr int kMoLS = 36;    // backward LDS row stride, as in nca_ot.hip
constexpr int kMoSS = 68;    // sign tile row stride (bytes)

__device__ __forceinline__ float4 mo_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 mo_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 mo_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float mo_sign(float v) { return (float)((v > 0.0f) - (v < 0.0f)); }

// ---- means ------------------------------------------------------------------------------------------------------------------------
// grid (ceil(c / 64), B).  Thread (s, q) = (tid / 16, tid % 16) sums rows s, s + 16, .. of channels 4 q .. 4 q + 3 of its tile; the 16
// slices are combined by one thread per quad in a fixed tree.  Two passes per matrix (see the head of the file).
__global__ __launch_bounds__(kMoThreads) void ot_mom_means_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  float* __restrict__ mx, float* __restrict__ my, float* __restrict__ sgn,
                                                                  float* __restrict__ m1p, int N, int c) {
    __shared__ float4 red[16][16];
    __shared__ float4 mean_s[2][16];
    const int tid = threadIdx.x, q = tid & 15, s = tid >> 4, b = blockIdx.y;
    const int ch = blockIdx.x * kMoTile + 4 * q;
    const bool ok = ch < c;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int which = 0; which < 2; ++which) {
        const float* const src = (which ? y : x) + (size_t)b * N * c + ch;
        float4 off = z;
        for (int pass = 0; pass < 2; ++pass) {
            float4 a = z;
            if (ok) {
#pragma unroll 4
                for (int n = s; n < N; n += 16) a = mo_add(a, mo_sub(mo_ld4(src + (size_t)n * c), off));
            }
            red[s][q] = a;
            __syncthreads();
            if (tid < 16) {
                float4 t[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) t[k] = red[k][tid];
#pragma unroll
                for (int w = 8; w > 0; w >>= 1) {
#pragma unroll
                    for (int k = 0; k < w; ++k) t[k] = mo_add(t[k], t[k + w]);
                }
                const float fn = (float)N;
                float4 r = make_float4(t[0].x / fn, t[0].y / fn, t[0].z / fn, t[0].w / fn);
                if (pass) r = mo_add(mean_s[which][tid], r);    // the first pass's mean + the mean of what it left
                mean_s[which][tid] = r;
            }
            __syncthreads();
            off = mean_s[which][q];
        }
    }
    if (tid < 64) {                                             // wave 0, lanes 0 .. 15 own a quad each
        float a = 0.0f;
        if (tid < 16 && ok) {
            const float4 u = mean_s[0][tid], v = mean_s[1][tid];
            const float4 d = mo_sub(u, v);
            *reinterpret_cast<float4*>(mx + (size_t)b * c + ch) = u;
            *reinterpret_cast<float4*>(my + (size_t)b * c + ch) = v;
            *reinterpret_cast<float4*>(sgn + (size_t)b * c + ch) = make_float4(mo_sign(d.x), mo_sign(d.y), mo_sign(d.z), mo_sign(d.w));
            a = (fabsf(d.x) + fabsf(d.y)) + (fabsf(d.z) + fabsf(d.w));
        }
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) a += __shfl_xor(a, m);
        if (tid == 0) m1p[(size_t)b * gridDim.x + blockIdx.x] = a;
    }
}

// ---- covariance difference ------------------------------------------------------------------------------------------------------------
// grid (nt (nt + 1) / 2, B), nt = ceil(c / 64).  Workgroup (p, b) owns the 64 x 64 tile (ti, tj), ti <= tj, of D; wave (wr, wc) its
// 32 x 32 quadrant (2 x 2 MFMA tiles) for X and for Y.  K = N runs in chunks of 32 rows staged as [row][channel] (the layout of X in
// memory; the next chunk's loads are in flight during this chunk's products).  MFMA k-step kk contracts rows 4 kk + g: lane (g, i)
// reads A = Xc[4 kk + g][channel 32 wr + 16 a + i] and B = Xc[4 kk + g][channel 32 wc + 16 j + i] as single dwords.  Rows beyond N
// and channels beyond c are loaded as the mean itself, so that centring leaves an exact zero there.
__global__ __launch_bounds__(kMoThreads, 2) void ot_mom_cov_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                   const float* __restrict__ mx, const float* __restrict__ my,
                                                                   signed char* __restrict__ S, float* __restrict__ covp, int N, int c, int nt) {
    __shared__ __attribute__((aligned(16))) float lds[4 * kMoKC * kMoCS];
    __shared__ float wsum[4];
    float* const xa = lds;
    float* const ya = lds + kMoKC * kMoCS;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15;
    const int wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int b = blockIdx.y;
    int ti = 0, tj = blockIdx.x;
    while (tj >= nt - ti) {                                     // pairs in row-major order of the upper triangle
        tj -= nt - ti;
        ++ti;
    }
    tj += ti;
    const bool diag = ti == tj;
    float* const xb = diag ? xa : lds + 2 * kMoKC * kMoCS;      // a diagonal pair has one operand tile
    float* const yb = diag ? ya : lds + 3 * kMoKC * kMoCS;
    const float* const xg = x + (size_t)b * N * c;
    const float* const yg = y + (size_t)b * N * c;

    // staging: a 32 x 64 chunk is 512 float4; thread tid carries rows tid / 16 and 16 + tid / 16 of the quad tid % 16
    const int srow = tid >> 4, sq = (tid & 15) * 4;
    const int cha = ti * kMoTile + sq, chb = tj * kMoTile + sq;
    const bool oka = cha < c, okb = chb < c && !diag;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 mxa = oka ? mo_ld4(mx + (size_t)b * c + cha) : z, mya = oka ? mo_ld4(my + (size_t)b * c + cha) : z;
    const float4 mxb = okb ? mo_ld4(mx + (size_t)b * c + chb) : z, myb = okb ? mo_ld4(my + (size_t)b * c + chb) : z;
    float4 pxa[2], pya[2], pxb[2], pyb[2];
    auto issue = [&](int kc) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = kc * kMoKC + srow + 16 * h;
            const size_t o = (size_t)min(n, N - 1) * c;
            const bool rok = n < N;
            pxa[h] = (rok && oka) ? mo_ld4(xg + o + cha) : mxa;
            pya[h] = (rok && oka) ? mo_ld4(yg + o + cha) : mya;
            pxb[h] = (rok && okb) ? mo_ld4(xg + o + chb) : mxb;
            pyb[h] = (rok && okb) ? mo_ld4(yg + o + chb) : myb;
        }
    };

    f32x4 ax[2][2], ay[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int j = 0; j < 2; ++j) ax[a][j] = ay[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int nk = (N + kMoKC - 1) / kMoKC;
    issue(0);
    for (int kc = 0; kc < nk; ++kc) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int o = (srow + 16 * h) * kMoCS + sq;
            *reinterpret_cast<float4*>(xa + o) = mo_sub(pxa[h], mxa);
            *reinterpret_cast<float4*>(ya + o) = mo_sub(pya[h], mya);
            if (!diag) {
                *reinterpret_cast<float4*>(xb + o) = mo_sub(pxb[h], mxb);
                *reinterpret_cast<float4*>(yb + o) = mo_sub(pyb[h], myb);
            }
        }
        __syncthreads();
        if (kc + 1 < nk) issue(kc + 1);
        const int oa = g * kMoCS + 32 * wr + i, ob = g * kMoCS + 32 * wc + i;
#pragma unroll
        for (int kk = 0; kk < kMoKC / 4; ++kk) {
            float fxa[2], fxb[2], fya[2], fyb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fxa[a] = xa[4 * kk * kMoCS + oa + 16 * a];
                fya[a] = ya[4 * kk * kMoCS + oa + 16 * a];
                fxb[a] = xb[4 * kk * kMoCS + ob + 16 * a];
                fyb[a] = yb[4 * kk * kMoCS + ob + 16 * a];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    ax[a][j] = nca_mfma(fxa[a], fxb[j], ax[a][j]);
                    ay[a][j] = nca_mfma(fya[a], fyb[j], ay[a][j]);
                }
            }
        }
        __syncthreads();
    }

    // ---- D[row][col] = (ax - ay) / (N - 1), row = 64 ti + 32 wr + 16 a + 4 g + r, col = 64 tj + 32 wc + 16 j + i ----
    signed char* const st = reinterpret_cast<signed char*>(lds);          // [64][kMoSS] signs; the loop's last barrier released the staging tiles
    const float den = (float)(N - 1);
    float sum = 0.0f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = 32 * wr + 16 * a + 4 * g + r, lc = 32 * wc + 16 * j + i;
                const float d = (ax[a][j][r] - ay[a][j][r]) / den;
                const bool ok = ti * kMoTile + lr < c && tj * kMoTile + lc < c;
                st[lr * kMoSS + lc] = (signed char)((d > 0.0f) - (d < 0.0f));
                sum += ok ? fabsf(d) : 0.0f;
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum += __shfl_xor(sum, m);           // butterfly: every lane ends with the same bits
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (tid == 0) covp[(size_t)b * gridDim.x + blockIdx.x] = (diag ? 1.0f : 2.0f) * ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    signed char* const Sb = S + (size_t)b * c * c;
#pragma unroll
    for (int h = 0; h < 4; ++h) {                                         // the tile as 64 rows of 16 words
        const int e = tid + kMoThreads * h, row = e >> 4, w = e & 15;
        const int grow = ti * kMoTile + row, gcol = tj * kMoTile + 4 * w;
        if (grow < c && gcol < c) *reinterpret_cast<int*>(Sb + (size_t)grow * c + gcol) = *reinterpret_cast<const int*>(st + row * kMoSS + 4 * w);
        if (!diag) {                                                      // and its transpose into the lower triangle
            const int trow = tj * kMoTile + row, tcol = ti * kMoTile + 4 * w;
            if (trow < c && tcol < c) {
                const unsigned v = (unsigned)(unsigned char)st[(4 * w + 0) * kMoSS + row] | ((unsigned)(unsigned char)st[(4 * w + 1) * kMoSS + row] << 8) |
                                   ((unsigned)(unsigned char)st[(4 * w + 2) * kMoSS + row] << 16) | ((unsigned)(unsigned char)st[(4 * w + 3) * kMoSS + row] << 24);
                *reinterpret_cast<unsigned*>(Sb + (size_t)trow * c + tcol) = v;
            }
        }
    }
}

// one thread per sample: mom = sum_t m1p / c + sum_p covp / c^2, both in index order
__global__ __launch_bounds__(64) void ot_mom_finish_kernel(const float* __restrict__ m1p, const float* __restrict__ covp, float* __restrict__ mom,
                                                           int B, int c, int nt, int np) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float m1 = 0.0f, cv = 0.0f;
    for (int t = 0; t < nt; ++t) m1 += m1p[(size_t)b * nt + t];
    for (int p = 0; p < np; ++p) cv += covp[(size_t)b * np + p];
    mom[b] = m1 / (float)c + cv / ((float)c * (float)c);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
// grid (ceil(N / 64), ceil(c / 64), B).  Workgroup (rt, ct, b) owns rows [64 rt, +64) x channels [64 ct, +64) of dY; the product
// (Y - my) S contracts over all c channels in chunks of 32, with nca_ot.hip's operand layout: A = rows of Y - my, B = rows of S
// (= its columns).  Every element of dY is read, updated and written by the one lane that holds it.
__global__ __launch_bounds__(kMoThreads, 2) void ot_mom_bwd_kernel(const float* __restrict__ y, const float* __restrict__ my,
                                                                   const float* __restrict__ sgn, const signed char* __restrict__ S,
                                                                   const float* __restrict__ gup, float* __restrict__ dy, int N, int c) {
    __shared__ __attribute__((aligned(16))) float as[kMoTile * kMoLS];
    __shared__ __attribute__((aligned(16))) float bs[kMoTile * kMoLS];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15;
    const int wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int b = blockIdx.z, r0 = blockIdx.x * kMoTile, c0 = blockIdx.y * kMoTile;
    const int nk = (c + kMoKC - 1) / kMoKC;
    const float* const yb = y + (size_t)b * N * c;
    const float* const myb = my + (size_t)b * c;
    const signed char* const Sb = S + (size_t)b * c * c;

    const int srow = tid >> 3, sq = (tid & 7) * 4;
    const size_t yo0 = (size_t)min(r0 + srow, N - 1) * c, yo1 = (size_t)min(r0 + 32 + srow, N - 1) * c;   // rows beyond N: copies, masked at the store
    const int k0r = c0 + srow, k1r = c0 + 32 + srow;                                                       // rows of S beyond c: zeros
    float4 py0, py1, pm;
    int ps0, ps1;
    auto issue = [&](int kc) {
        const int k = kc * kMoKC + sq;
        if (k < c) {                                            // c % 4 == 0: a quad is inside the row or wholly beyond it
            pm = mo_ld4(myb + k);
            py0 = mo_ld4(yb + yo0 + k);
            py1 = mo_ld4(yb + yo1 + k);
            ps0 = k0r < c ? *reinterpret_cast<const int*>(Sb + (size_t)k0r * c + k) : 0;
            ps1 = k1r < c ? *reinterpret_cast<const int*>(Sb + (size_t)k1r * c + k) : 0;
        } else {
            pm = py0 = py1 = make_float4(0.f, 0.f, 0.f, 0.f);
            ps0 = ps1 = 0;
        }
    };
    auto widen = [](int w) {
        const unsigned u = (unsigned)w;
        return make_float4((float)((int)(u << 24) >> 24), (float)((int)(u << 16) >> 24), (float)((int)(u << 8) >> 24), (float)(w >> 24));
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    issue(0);
    for (int kc = 0; kc < nk; ++kc) {
        *reinterpret_cast<float4*>(as + srow * kMoLS + sq) = mo_sub(py0, pm);
        *reinterpret_cast<float4*>(as + (32 + srow) * kMoLS + sq) = mo_sub(py1, pm);
        *reinterpret_cast<float4*>(bs + srow * kMoLS + sq) = widen(ps0);
        *reinterpret_cast<float4*>(bs + (32 + srow) * kMoLS + sq) = widen(ps1);
        __syncthreads();
        if (kc + 1 < nk) issue(kc + 1);
        const float* const ar = as + (32 * wr + i) * kMoLS + 4 * g;
        const float* const br = bs + (32 * wc + i) * kMoLS + 4 * g;
#pragma unroll
        for (int s = 0; s < kMoKC / 16; ++s) {
            float4 av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = *reinterpret_cast<const float4*>(ar + 16 * a * kMoLS + 16 * s);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const float4*>(br + 16 * j * kMoLS + 16 * s);
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
    // acc[a][j][r] = ((Y - my) S)[row r0 + 32 wr + 16 a + 4 g + r][channel c0 + 32 wc + 16 j + i]
    const float gb = gup[b];
    const float cm = -gb / ((float)c * (float)N), cc = -2.0f * gb / (float)(N - 1) / ((float)c * (float)c);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = c0 + 32 * wc + 16 * j + i;
        if (col >= c) continue;
        const float first = cm * sgn[(size_t)b * c + col];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 32 * wr + 16 * a + 4 * g + r;
                if (row < N) {
                    float* const o = dy + ((size_t)b * N + row) * c + col;
                    *o = *o + (first + cc * acc[a][j][r]);
                }
            }
        }
    }
}

}  // namespace

int nca_ot_moment_tiles(int c) { return (c + kMoTile - 1) / kMoTile; }

// ws: mx [B, c], then the mean partials [B, nt], then the covariance partials [B, nt (nt + 1) / 2]
hipError_t nca_launch_ot_moment_fwd(const float* x, const float* y, float* mom, float* my, float* sgn, signed char* S, int B, int N, int c,
                                    void* ws, hipStream_t st) {
    const int nt = nca_ot_moment_tiles(c), np = nt * (nt + 1) / 2;
    float* const mx = (float*)ws;
    float* const m1p = mx + (size_t)B * c;
    float* const covp = m1p + (size_t)B * nt;
    hipLaunchKernelGGL(ot_mom_means_kernel, dim3(nt, B), dim3(kMoThreads), 0, st, x, y, mx, my, sgn, m1p, N, c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ot_mom_cov_kernel, dim3(np, B), dim3(kMoThreads), 0, st, x, y, (const float*)mx, (const float*)my, S, covp, N, c, nt);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ot_mom_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, (const float*)m1p, (const float*)covp, mom, B, c, nt, np);
    return hipGetLastError();
}

hipError_t nca_launch_ot_moment_bwd(const float* y, const float* my, const float* sgn, const signed char* S, const float* gup, float* dy, int B,
                                    int N, int c, hipStream_t st) {
    hipLaunchKernelGGL(ot_mom_bwd_kernel, dim3((N + kMoTile - 1) / kMoTile, nca_ot_moment_tiles(c), B), dim3(kMoThreads), 0, st, y, my, sgn, S,
                       gup, dy, N, c);
    return hipGetLastError();
}

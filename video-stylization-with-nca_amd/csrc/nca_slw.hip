// nca_slw.hip -- the sliced-Wasserstein style loss (EncoderConditioning/loss/appearance_loss.py:109-140) on gfx950.
//
// Per level, with source [B, c, n] and target [1, c, m] the flattened features and proj [c, 32] unit directions,
//     k[b, p, i] = sum_c source[b, c, i] proj[c, p],   s = sort_i k,   t = sort_i (target keys),
//     loss = sum_{b, p, i} (s[b, p, i] - t[p, j(i)])^2,   j = the nearest-resample index map of F.interpolate (m -> n).
//   slw_project_kernel     [32 x c] . [c x n] on exact-f32 MFMA for source and target in one launch; the features are read as they lie
//                          in memory (coalesced on n), K = c staged in chunks of 16 channels through LDS with the next chunk's loads
//                          in flight.  slw_project3_kernel is the c = 3 (image level) form on plain VALU.
//   slw_sort_lds_kernel    bitonic sort of (key, index) pairs, one workgroup per 4096-pair chunk of a row (32 KB of LDS: four to five
//                          workgroups, 16 to 20 waves, per CU).  <true> sorts the chunk from scratch, <false> runs the strides below the
//                          chunk size of one merge stage of a longer row.
//   slw_sort_global_kernel one compare-exchange per thread at a stride at or above the chunk size.
//   slw_loss_kernel        (s - t[j(i)])^2 summed per (row, 4096-position block) in a fixed tree; slw_finish_kernel adds the partials
//                          in index order.
//   slw_scatter_kernel     dk[b, p, perm[b, p, i]] = 2 g (s - t[j(i)]): perm is a permutation, so every element has one owner.  The
//                          residual is recomputed here from s and t instead of being kept by the forward: that costs one extra read of
//                          the (small, cached) target row and saves a write and a read of a [B, 32, n] buffer.
//   slw_bwd_kernel         dsource[b, c, i] = sum_p proj[c, p] dk[b, p, i], K = 32 on the same MFMA, written straight into [B, c, n];
//                          slw_bwd3_kernel is its c = 3 form.
// No atomics, no polling, no hand-off between workgroups: every launch is bounded by its grid, every sum has one owner and a fixed
// order, so results are bit-reproducible from run to run.
//
// The order.  Pairs compare by (key, original index), lowest index first on equal keys -- the order of torch.sort(stable = True);
// -0.0 and +0.0 are equal as floats, so their indices decide.  The network is the bitonic sorter in its one-direction form: stage k
// first compares position i with the mirrored position of its k-block (i ^ (k - 1)), then runs the strides k / 4 .. 1 (i ^ j); every
// comparator leaves the smaller pair at the lower position.  A row is padded to the next power of two with pairs (+inf, position) that
// sort last.  Such a pair is never moved by this network (whatever meets it from below is smaller, and two of them are already in
// order), so the padding of a long row is never stored: a comparator whose upper position lies at or beyond n is skipped.
// Non-finite keys are outside the contract (a NaN breaks the order, a +inf key ties with the padding).
#include "nca_common.h"
#include "nca_kernels.h"

namespace {

constexpr int kSlwThreads = 256, kSlwProj = 32;
constexpr int kSlwLogChunk = 12, kSlwChunk = 1 << kSlwLogChunk;   // pairs per LDS sort chunk, positions per loss partial
constexpr int kPjTile = 256, kPjKC = 16;
constexpr int kPjXS = kPjTile + 16;   // feature rows in LDS (floats): lanes (g, i), g in {0, 1}, read banks 16 g + i (272 mod 32 = 16)
constexpr int kPjPS = 48;             // projection rows in LDS: the same (48 mod 32 = 16)

// ---- projection -------------------------------------------------------------------------------------------------------------------
// grid (ceil(max(n, m) / 256), B + 1): sample B is the target.  Wave w owns positions [64 w, +64) of the tile for all 32 directions:
// MFMA rows = directions (two tiles of 16), columns = positions (four tiles of 16), k = channels.  Lane (g, i) reads
// A = proj[channel 4 kk + g][direction 16 a + i] and B = x[channel 4 kk + g][position 16 j + i].
__global__ __launch_bounds__(kSlwThreads) void slw_project_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                                  const float* __restrict__ proj, float* __restrict__ ks,
                                                                  float* __restrict__ kt, int B, int c, int n, int m) {
    __shared__ __attribute__((aligned(16))) float xs[kPjKC * kPjXS];
    __shared__ __attribute__((aligned(16))) float ps[kPjKC * kPjPS];
    const int b = blockIdx.y;
    const bool is_t = b == B;
    const int len = is_t ? m : n, n0 = blockIdx.x * kPjTile;
    if (n0 >= len) return;
    const float* const xb = is_t ? tgt : src + (size_t)b * c * n;
    float* const ob = is_t ? kt : ks + (size_t)b * kSlwProj * n;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15, w = tid >> 6;
    const bool vec = (len & 3) == 0;
    const int sq = 4 * (tid & 63), sr = tid >> 6;            // staging: rows sr + 4 h of the quad at positions n0 + sq ..
    const int pr = tid >> 3, pq = 4 * (tid & 7);             // threads 0 .. 127: row pr, directions pq .. pq + 3 of the projection chunk
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 px[4], pp = z;
    auto issue = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int ch = k0 + sr + 4 * h, pos = n0 + sq;
            float4 v = z;
            if (ch < c) {
                const float* const r = xb + (size_t)ch * len;
                if (vec && pos + 3 < len) {
                    v = *reinterpret_cast<const float4*>(r + pos);
                } else {
                    if (pos < len) v.x = r[pos];
                    if (pos + 1 < len) v.y = r[pos + 1];
                    if (pos + 2 < len) v.z = r[pos + 2];
                    if (pos + 3 < len) v.w = r[pos + 3];
                }
            }
            px[h] = v;
        }
        if (tid < 128) pp = k0 + pr < c ? *reinterpret_cast<const float4*>(proj + (size_t)(k0 + pr) * kSlwProj + pq) : z;
    };
    f32x4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int nk = (c + kPjKC - 1) / kPjKC;
    issue(0);
    for (int kc = 0; kc < nk; ++kc) {
#pragma unroll
        for (int h = 0; h < 4; ++h) *reinterpret_cast<float4*>(xs + (sr + 4 * h) * kPjXS + sq) = px[h];
        if (tid < 128) *reinterpret_cast<float4*>(ps + pr * kPjPS + pq) = pp;
        __syncthreads();
        if (kc + 1 < nk) issue((kc + 1) * kPjKC);
#pragma unroll
        for (int kk = 0; kk < kPjKC / 4; ++kk) {
            float fa[2], fb[4];
#pragma unroll
            for (int a = 0; a < 2; ++a) fa[a] = ps[(4 * kk + g) * kPjPS + 16 * a + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = xs[(4 * kk + g) * kPjXS + 64 * w + 16 * j + i];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[a][j] = nca_mfma(fa[a], fb[j], acc[a][j]);
            }
        }
        __syncthreads();
    }
    // acc[a][j][r] = k[direction 16 a + 4 g + r][position n0 + 64 w + 16 j + i]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + 64 * w + 16 * j + i;
        if (col >= len) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int r = 0; r < 4; ++r) ob[(size_t)(16 * a + 4 * g + r) * len + col] = acc[a][j][r];
        }
    }
}

// c = 3: one position per thread, the 96 projection weights in LDS
__global__ __launch_bounds__(kSlwThreads) void slw_project3_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                                   const float* __restrict__ proj, float* __restrict__ ks,
                                                                   float* __restrict__ kt, int B, int n, int m) {
    __shared__ float ps[3 * kSlwProj];
    const int b = blockIdx.y;
    const bool is_t = b == B;
    const int len = is_t ? m : n, pos = blockIdx.x * kSlwThreads + threadIdx.x;
    if (blockIdx.x * kSlwThreads >= len) return;
    if (threadIdx.x < 3 * kSlwProj) ps[threadIdx.x] = proj[threadIdx.x];
    __syncthreads();
    if (pos >= len) return;
    const float* const xb = is_t ? tgt : src + (size_t)b * 3 * n;
    float* const ob = is_t ? kt : ks + (size_t)b * kSlwProj * n;
    const float x0 = xb[pos], x1 = xb[(size_t)len + pos], x2 = xb[2 * (size_t)len + pos];
#pragma unroll 8
    for (int p = 0; p < kSlwProj; ++p) ob[(size_t)p * len + pos] = fmaf(x2, ps[2 * kSlwProj + p], fmaf(x1, ps[kSlwProj + p], x0 * ps[p]));
}

// ---- sort -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool slw_after(float ka, int ia, float kb, int ib) { return ka > kb || (ka == kb && ia > ib); }

__device__ __forceinline__ void slw_cx_lds(float* sk, int* sp, int l, int h) {
    const float ka = sk[l], kb = sk[h];
    const int ia = sp[l], ib = sp[h];
    if (slw_after(ka, ia, kb, ib)) {
        sk[l] = kb;
        sk[h] = ka;
        sp[l] = ib;
        sp[h] = ia;
    }
}

// grid (ceil(n / 4096), rows).  len = min(P, 4096) = 2^loglen pairs per workgroup, P the padded row length.
template <bool kFull>
__global__ __launch_bounds__(kSlwThreads) void slw_sort_lds_kernel(float* __restrict__ keys, int* __restrict__ perm, int n, int len, int loglen) {
    __shared__ float sk[kSlwChunk];
    __shared__ int sp[kSlwChunk];
    const int tid = threadIdx.x, base = blockIdx.x * kSlwChunk;
    float* const kr = keys + (size_t)blockIdx.y * n;
    int* const pr = perm + (size_t)blockIdx.y * n;
    for (int e = tid; e < len; e += kSlwThreads) {
        const int gi = base + e;
        const bool in = gi < n;
        sk[e] = in ? kr[gi] : __builtin_huge_valf();
        sp[e] = (in && !kFull) ? pr[gi] : gi;
    }
    __syncthreads();
    const int half = len >> 1;
    auto strides = [&](int lj0) {
        for (int lj = lj0; lj >= 0; --lj) {
            const int j = 1 << lj;
            for (int t = tid; t < half; t += kSlwThreads) {
                const int l = ((t >> lj) << (lj + 1)) | (t & (j - 1));
                slw_cx_lds(sk, sp, l, l + j);
            }
            __syncthreads();
        }
    };
    if (kFull) {
        for (int lk = 1; lk <= loglen; ++lk) {
            const int hm = (1 << (lk - 1)) - 1;
            for (int t = tid; t < half; t += kSlwThreads) {
                const int off = t & hm, blk = (t >> (lk - 1)) << lk;
                slw_cx_lds(sk, sp, blk + off, blk + (1 << lk) - 1 - off);
            }
            __syncthreads();
            strides(lk - 2);
        }
    } else {
        strides(loglen - 1);
    }
    for (int e = tid; e < len; e += kSlwThreads) {
        const int gi = base + e;
        if (gi < n) {
            kr[gi] = sk[e];
            pr[gi] = sp[e];
        }
    }
}

// grid (ceil(P / 2 / 256), rows): comparator t of the mirror step of stage 2^lk (flip) or of the stride 2^lj
__global__ __launch_bounds__(kSlwThreads) void slw_sort_global_kernel(float* __restrict__ keys, int* __restrict__ perm, int n, int halfp, int lk,
                                                                      int lj, int flip) {
    const int t = blockIdx.x * kSlwThreads + threadIdx.x;
    if (t >= halfp) return;
    int l, h;
    if (flip) {
        const int off = t & ((1 << (lk - 1)) - 1), blk = (t >> (lk - 1)) << lk;
        l = blk + off;
        h = blk + (1 << lk) - 1 - off;
    } else {
        l = ((t >> lj) << (lj + 1)) | (t & ((1 << lj) - 1));
        h = l + (1 << lj);
    }
    if (h >= n) return;                                          // the upper pair is padding: nothing moves
    float* const kr = keys + (size_t)blockIdx.y * n;
    int* const pr = perm + (size_t)blockIdx.y * n;
    const float ka = kr[l], kb = kr[h];
    const int ia = pr[l], ib = pr[h];
    if (slw_after(ka, ia, kb, ib)) {
        kr[l] = kb;
        kr[h] = ka;
        pr[l] = ib;
        pr[h] = ia;
    }
}

// ---- loss -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int slw_j(const int* __restrict__ jmap, int i, int m) { return min(max(jmap[i], 0), m - 1); }

// grid (ceil(n / 4096), 32 B): thread tid adds positions blk 4096 + 256 e + tid, e ascending; lanes by butterfly, waves in order
__global__ __launch_bounds__(kSlwThreads) void slw_loss_kernel(const float* __restrict__ s, const float* __restrict__ t, const int* __restrict__ jmap,
                                                               float* __restrict__ part, int n, int m) {
    __shared__ float wsum[4];
    const int row = blockIdx.y, p = row & (kSlwProj - 1), tid = threadIdx.x;
    const float* const sr = s + (size_t)row * n;
    const float* const tr = t + (size_t)p * m;
    float a = 0.0f;
#pragma unroll 4
    for (int e = 0; e < kSlwChunk / kSlwThreads; ++e) {
        const int i = blockIdx.x * kSlwChunk + e * kSlwThreads + tid;
        if (i < n) {
            const float d = sr[i] - tr[slw_j(jmap, i, m)];
            a = fmaf(d, d, a);
        }
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) a += __shfl_xor(a, k);
    if ((tid & 63) == 0) wsum[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) part[(size_t)row * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// one workgroup: thread b adds the partials of sample b (rows, then blocks, in index order), thread 0 the samples in index order
__global__ __launch_bounds__(kSlwThreads) void slw_finish_kernel(const float* __restrict__ part, float* __restrict__ persample, float* __restrict__ loss,
                                                                 int B, int nblk) {
    const int per = kSlwProj * nblk;
    for (int b = threadIdx.x; b < B; b += kSlwThreads) {
        float a = 0.0f;
        for (int k = 0; k < per; ++k) a += part[(size_t)b * per + k];
        persample[b] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.0f;
        for (int b = 0; b < B; ++b) a += persample[b];
        loss[0] = a;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// grid (ceil(n / 256), 32 B)
__global__ __launch_bounds__(kSlwThreads) void slw_scatter_kernel(const float* __restrict__ s, const float* __restrict__ t, const int* __restrict__ jmap,
                                                                  const int* __restrict__ perm, const float* __restrict__ gup, float* __restrict__ dk,
                                                                  int n, int m) {
    const int row = blockIdx.y, p = row & (kSlwProj - 1), i = blockIdx.x * kSlwThreads + threadIdx.x;
    if (i >= n) return;
    const float g2 = 2.0f * gup[0];
    const float d = s[(size_t)row * n + i] - t[(size_t)p * m + slw_j(jmap, i, m)];
    const int o = perm[(size_t)row * n + i];
    if ((unsigned)o < (unsigned)n) dk[(size_t)row * n + o] = g2 * d;
}

// grid (ceil(n / 256), ceil(c / 64), B).  Wave w owns positions [64 w, +64) of the tile and keeps its dk operands (32 directions x 64
// positions) in registers for the up to four 16-channel tiles of the workgroup: MFMA rows = channels, columns = positions, k =
// directions.  Lane (g, i) reads A = proj[channel 16 ct + i][direction 4 kk + g] and B = dk[direction 4 kk + g][position 16 j + i].
__global__ __launch_bounds__(kSlwThreads) void slw_bwd_kernel(const float* __restrict__ dk, const float* __restrict__ proj, float* __restrict__ ds,
                                                              int c, int n) {
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15, w = tid >> 6;
    const int b = blockIdx.z, n0 = blockIdx.x * kPjTile + 64 * w;
    const float* const dkb = dk + (size_t)b * kSlwProj * n;
    float fb[8][4];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + 16 * j + i;
            fb[kk][j] = col < n ? dkb[(size_t)(4 * kk + g) * n + col] : 0.0f;
        }
    }
    for (int ct = 0; ct < 4; ++ct) {
        const int c0 = 64 * blockIdx.y + 16 * ct;
        if (c0 >= c) break;
        const int ar = c0 + i;
        float fa[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) fa[kk] = ar < c ? proj[(size_t)ar * kSlwProj + 4 * kk + g] : 0.0f;
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = nca_mfma(fa[kk], fb[kk][j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + 16 * j + i;
            if (col >= n) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = c0 + 4 * g + r;
                if (ch < c) ds[((size_t)b * c + ch) * n + col] = acc[j][r];
            }
        }
    }
}

// c = 3: grid (ceil(n / 256), B), one position per thread
__global__ __launch_bounds__(kSlwThreads) void slw_bwd3_kernel(const float* __restrict__ dk, const float* __restrict__ proj, float* __restrict__ ds, int n) {
    __shared__ float ps[3 * kSlwProj];
    if (threadIdx.x < 3 * kSlwProj) ps[threadIdx.x] = proj[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y, pos = blockIdx.x * kSlwThreads + threadIdx.x;
    if (pos >= n) return;
    const float* const dkb = dk + (size_t)b * kSlwProj * n + pos;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll 8
    for (int p = 0; p < kSlwProj; ++p) {
        const float v = dkb[(size_t)p * n];
        a0 = fmaf(ps[p], v, a0);
        a1 = fmaf(ps[kSlwProj + p], v, a1);
        a2 = fmaf(ps[2 * kSlwProj + p], v, a2);
    }
    float* const o = ds + (size_t)b * 3 * n + pos;
    o[0] = a0;
    o[(size_t)n] = a1;
    o[2 * (size_t)n] = a2;
}

int slw_log2_ceil(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

}  // namespace

int nca_slw_blocks(int n) { return (n + kSlwChunk - 1) / kSlwChunk; }

hipError_t nca_launch_slw_project(const float* src, const float* tgt, const float* proj, float* ks, float* kt, int B, int c, int n, int m,
                                  hipStream_t st) {
    const int len = n > m ? n : m;
    if (c == 3) {
        hipLaunchKernelGGL(slw_project3_kernel, dim3((len + kSlwThreads - 1) / kSlwThreads, B + 1), dim3(kSlwThreads), 0, st, src, tgt, proj, ks, kt,
                           B, n, m);
    } else {
        hipLaunchKernelGGL(slw_project_kernel, dim3((len + kPjTile - 1) / kPjTile, B + 1), dim3(kSlwThreads), 0, st, src, tgt, proj, ks, kt, B, c,
                           n, m);
    }
    return hipGetLastError();
}

hipError_t nca_launch_slw_sort(float* keys, int* perm, int rows, int n, hipStream_t st) {
    const int logp = slw_log2_ceil(n), loglen = logp < kSlwLogChunk ? logp : kSlwLogChunk;
    const dim3 lds_grid(nca_slw_blocks(n), rows), blk(kSlwThreads);
    hipLaunchKernelGGL(slw_sort_lds_kernel<true>, lds_grid, blk, 0, st, keys, perm, n, 1 << loglen, loglen);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (logp <= kSlwLogChunk) return e;
    const int halfp = 1 << (logp - 1);
    const dim3 glb_grid((halfp + kSlwThreads - 1) / kSlwThreads, rows);
    for (int lk = kSlwLogChunk + 1; lk <= logp; ++lk) {
        hipLaunchKernelGGL(slw_sort_global_kernel, glb_grid, blk, 0, st, keys, perm, n, halfp, lk, 0, 1);
        for (int lj = lk - 2; lj >= kSlwLogChunk; --lj) hipLaunchKernelGGL(slw_sort_global_kernel, glb_grid, blk, 0, st, keys, perm, n, halfp, lk, lj, 0);
        hipLaunchKernelGGL(slw_sort_lds_kernel<false>, lds_grid, blk, 0, st, keys, perm, n, kSlwChunk, kSlwLogChunk);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return e;
}

// ws: the partials [32 B, ceil(n / 4096)], then one sum per sample [B]
hipError_t nca_launch_slw_loss_fwd(const float* s, const float* t, const int* jmap, float* loss, int B, int n, int m, void* ws, hipStream_t st) {
    const int nblk = nca_slw_blocks(n);
    float* const part = (float*)ws;
    float* const persample = part + (size_t)B * kSlwProj * nblk;
    hipLaunchKernelGGL(slw_loss_kernel, dim3(nblk, B * kSlwProj), dim3(kSlwThreads), 0, st, s, t, jmap, part, n, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(slw_finish_kernel, dim3(1), dim3(kSlwThreads), 0, st, (const float*)part, persample, loss, B, nblk);
    return hipGetLastError();
}

// ws: dk [B, 32, n]
hipError_t nca_launch_slw_bwd(const float* s, const float* t, const int* jmap, const int* perm, const float* proj, const float* gup, float* ds, int B,
                              int c, int n, int m, void* ws, hipStream_t st) {
    float* const dk = (float*)ws;
    hipLaunchKernelGGL(slw_scatter_kernel, dim3((n + kSlwThreads - 1) / kSlwThreads, B * kSlwProj), dim3(kSlwThreads), 0, st, s, t, jmap, perm, gup, dk,
                       n, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (c == 3) {
        hipLaunchKernelGGL(slw_bwd3_kernel, dim3((n + kSlwThreads - 1) / kSlwThreads, B), dim3(kSlwThreads), 0, st, (const float*)dk, proj, ds, n);
    } else {
        hipLaunchKernelGGL(slw_bwd_kernel, dim3((n + kPjTile - 1) / kPjTile, (c + 63) / 64, B), dim3(kSlwThreads), 0, st, (const float*)dk, proj, ds, c,
                           n);
    }
    return hipGetLastError();
}

// nca_dynca_bwd.hip -- the backward of the fused DyNCA step: the MLP part instantiates the backward variants of
// dynca_step_fwd_kernel (nca_dynca_step.h) and no other; the stencil adjoint has two kernels of its own, here.
// Built only through nca_step.hip, which includes this file: never list it in the Makefile's SRCS beside that unit (duplicate symbols).
#include "nca_dynca_step.h"

namespace {

// dL/dx_t = G + dy[0:C] + adj(Sx)(dy[C:2C]) + adj(Sy)(dy[2C:3C]) + adj(L)(dy[3C:4C]), where adj is the adjoint of
// "F.pad(mode) then 3x3 cross-correlation" (dynca.py:83-86): a cell p collects w[t] * dy[q] from every (q, t) whose
// padded source index pad(q + t) equals p.  Candidates q lie in p's 3x3 neighbourhood (wrapped for 'circular').
__device__ float dynca_bwd_cell(const NcaDyncaArgs& a, int b, int c, int py, int px) {
    const int C = a.C, H = a.H, W = a.W, pad = a.pad_mode;
    const size_t plane = (size_t)H * W;
    const float* const dy = a.dybuf + (size_t)b * 4 * C * plane;
    const size_t off = (size_t)py * W + px;
    float base = a.g_next ? a.g_next[((size_t)b * C + c) * plane + off] : 0.0f;
    if (a.g_extra) base += a.g_extra[((size_t)b * C + c) * plane + off];   // cotangent of the intermediate state itself
    if (a.coarse_add)   // two-scale perception: adjoint of the 2x2 mean, 0.25 * dL/dx_coarse of the cell's coarse parent
        base += 0.25f * a.coarse_add[((size_t)b * C + c) * (size_t)(H >> 1) * (W >> 1) + (size_t)(py >> 1) * (W >> 1) + (px >> 1)];
    float acc = dy[(size_t)c * plane + off];
    // per axis: for candidate offset iq in {-1,0,1} and tap t in {-1,0,1}: does pad(q + t) land on p ?
    int qy[3], qx[3];
    bool hy[3][3], hx[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int q = py + i - 1;
        if (pad == NCA_PAD_CIRCULAR) q = ((q % H) + H) % H;
        bool ok = q >= 0 && q < H;
        for (int k = 0; k < i; ++k) ok = ok && !(qy[k] == q);   // wrapped duplicates when H < 3
        qy[i] = ok ? q : -1;
#pragma unroll
        for (int t = 0; t < 3; ++t) hy[i][t] = ok && nca_pad_index(q + t - 1, H, pad) == py;
        q = px + i - 1;
        if (pad == NCA_PAD_CIRCULAR) q = ((q % W) + W) % W;
        ok = q >= 0 && q < W;
        for (int k = 0; k < i; ++k) ok = ok && !(qx[k] == q);
        qx[i] = ok ? q : -1;
#pragma unroll
        for (int t = 0; t < 3; ++t) hx[i][t] = ok && nca_pad_index(q + t - 1, W, pad) == px;
    }
    const float SX[3][3] = {{-1.f, 0.f, 1.f}, {-2.f, 0.f, 2.f}, {-1.f, 0.f, 1.f}};
    const float LP[3][3] = {{1.f, 2.f, 1.f}, {2.f, -12.f, 2.f}, {1.f, 2.f, 1.f}};
#pragma unroll
    for (int iy = 0; iy < 3; ++iy)
#pragma unroll
        for (int ix = 0; ix < 3; ++ix) {
            if (qy[iy] < 0 || qx[ix] < 0) continue;
            float wsx = 0.f, wsy = 0.f, wl = 0.f;
#pragma unroll
            for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                for (int tx = 0; tx < 3; ++tx)
                    if (hy[iy][ty] && hx[ix][tx]) { wsx += SX[ty][tx]; wsy += SX[tx][ty]; wl += LP[ty][tx]; }
            const size_t qo = (size_t)qy[iy] * W + qx[ix];
            acc = fmaf(wsx, dy[(size_t)(C + c) * plane + qo], acc);
            acc = fmaf(wsy, dy[(size_t)(2 * C + c) * plane + qo], acc);
            acc = fmaf(wl, dy[(size_t)(3 * C + c) * plane + qo], acc);
        }
    return base + (a.dy_half ? 0.5f * acc : acc);   // two-scale perception: the fine level carries half of dL/dy
}

// any shape: one thread per cell
__global__ __launch_bounds__(256) void dynca_step_bwd_stencil_kernel(const NcaDyncaArgs a) {
    const int C = a.C, H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)a.B * C * plane) return;
    const int px = (int)(id % W), py = (int)((id / W) % H), c = (int)((id / plane) % C), b = (int)(id / (plane * C));
    a.g_out[id] = dynca_bwd_cell(a, b, c, py, px);
}

// W % 4 == 0, 16-byte aligned planes: one thread per 4 W-contiguous cells.  Away from the image border the padding plays no
// part and the adjoint is the correlation with the flipped filters (Sobel flips sign, the Laplacian is symmetric): three
// rows of three planes, 16-byte loads plus the two edge cells (L1 hits: the neighbouring lanes fetch those lines).
// The border band (two rows top and bottom, four columns left and right) is left to separate WORKGROUPS of the same launch
// (dynca_bwd_border_block below): a few lanes of every wave running the per-cell routine would hold the whole wave for its
// ~2000 instructions.
__device__ __forceinline__ void dynca_bwd_vec_block(const NcaDyncaArgs& a, unsigned blk) {
    const int C = a.C, H = a.H, W = a.W, W4 = W >> 2;
    const size_t plane = (size_t)H * W;
    const size_t id = (size_t)blk * blockDim.x + threadIdx.x;
    if (id >= (size_t)a.B * C * H * W4) return;
    const int x0 = (int)(id % W4) * 4, py = (int)((id / W4) % H), c = (int)((id / ((size_t)W4 * H)) % C),
              b = (int)(id / ((size_t)W4 * H * C));
    float* const out = a.g_out + ((size_t)b * C + c) * plane + (size_t)py * W + x0;
    // border band of two cells: with 'reflect' a border cell's out-of-range taps land one cell INSIDE the image
    if (py < 2 || py > H - 3 || x0 < 4 || x0 + 8 > W) return;   // the border band belongs to dynca_bwd_border_block
    const float* const dy = a.dybuf + (size_t)b * 4 * C * plane + (size_t)py * W + x0;
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.g_next) gv = *reinterpret_cast<const float4*>(a.g_next + ((size_t)b * C + c) * plane + (size_t)py * W + x0);
    const float4 d0 = *reinterpret_cast<const float4*>(dy + (size_t)c * plane);
    float base[4] = {gv.x, gv.y, gv.z, gv.w};
    float acc[4] = {d0.x, d0.y, d0.z, d0.w};
    if (a.g_extra) {
        const float4 ge = *reinterpret_cast<const float4*>(a.g_extra + ((size_t)b * C + c) * plane + (size_t)py * W + x0);
        base[0] += ge.x; base[1] += ge.y; base[2] += ge.z; base[3] += ge.w;
    }
    if (a.coarse_add) {   // W % 4 == 0: the 4 cells have the coarse parents x0/2 and x0/2 + 1 (8-byte aligned pair)
        const float2 cp = *reinterpret_cast<const float2*>(a.coarse_add + ((size_t)b * C + c) * (size_t)(H >> 1) * (W >> 1) +
                                                           (size_t)(py >> 1) * (W >> 1) + (x0 >> 1));
        base[0] += 0.25f * cp.x; base[1] += 0.25f * cp.x; base[2] += 0.25f * cp.y; base[3] += 0.25f * cp.y;
    }
    float v[3][3][6];   // [filter plane][row y-1..y+1][col x0-1..x0+4]
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float* const row = dy + (size_t)((f + 1) * C + c) * plane + (ptrdiff_t)(r - 1) * W;
            const float4 m = *reinterpret_cast<const float4*>(row);
            v[f][r][0] = row[-1]; v[f][r][1] = m.x; v[f][r][2] = m.y; v[f][r][3] = m.z; v[f][r][4] = m.w; v[f][r][5] = row[4];
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // flipped Sobel-x: weight of dy1[p + (dyy, dxx)] is SX[1 - dyy][1 - dxx] = -SX[1 + dyy][1 + dxx]
        const float sx = (v[0][0][j] - v[0][0][j + 2]) + 2.0f * (v[0][1][j] - v[0][1][j + 2]) + (v[0][2][j] - v[0][2][j + 2]);
        const float sy = (v[1][0][j] + 2.0f * v[1][0][j + 1] + v[1][0][j + 2]) - (v[1][2][j] + 2.0f * v[1][2][j + 1] + v[1][2][j + 2]);
        const float lp = (v[2][0][j] + v[2][0][j + 2] + v[2][2][j] + v[2][2][j + 2]) +
                         2.0f * (v[2][0][j + 1] + v[2][1][j] + v[2][1][j + 2] + v[2][2][j + 1]) - 12.0f * v[2][1][j + 1];
        acc[j] += sx + sy + lp;
        acc[j] = base[j] + (a.dy_half ? 0.5f * acc[j] : acc[j]);
    }
    *reinterpret_cast<float4*>(out) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// the border band of every (b, c) plane, one thread per cell: 4 full rows + 8 columns of the H - 4 rows between them
__device__ __forceinline__ void dynca_bwd_border_block(const NcaDyncaArgs& a, unsigned blk) {
    const int C = a.C, H = a.H, W = a.W;
    const int per_plane = 4 * W + 8 * (H - 4);
    const size_t id = (size_t)blk * blockDim.x + threadIdx.x;
    if (id >= (size_t)a.B * C * per_plane) return;
    const int k = (int)(id % per_plane), c = (int)((id / per_plane) % C), b = (int)(id / ((size_t)per_plane * C));
    int py, px;
    if (k < 4 * W) {
        const int r = k / W;
        py = r < 2 ? r : H - 4 + r;
        px = k - r * W;
    } else {
        const int q = k - 4 * W, j = q & 7;
        py = 2 + (q >> 3);
        px = j < 4 ? j : W - 8 + j;
    }
    a.g_out[((size_t)b * C + c) * (size_t)H * W + (size_t)py * W + px] = dynca_bwd_cell(a, b, c, py, px);
}
// One launch for both: the first nborder workgroups take the border band (their threads are the slow ones: dispatched first,
// they run under the interior's memory traffic instead of after it -- as a launch of their own they were 19 us behind a 50 us
// interior pass), the rest the interior.
__global__ __launch_bounds__(256) void dynca_step_bwd_stencil_vec_kernel(const NcaDyncaArgs a, unsigned nborder) {
    if (blockIdx.x < nborder) dynca_bwd_border_block(a, blockIdx.x);
    else dynca_bwd_vec_block(a, blockIdx.x - nborder);
}

}  // namespace

// the grids the backward MLP kernel runs with = the number of dW2 | db2 slabs it writes (launch_dynca, nca_dynca_step.h)
int nca_dynca_bwd_grid_c(int B, int C, int H, int W) {
    const int ntiles = B * ((W + 31) / 32) * ((H + 7) / 8);
    return grid_for(ntiles, C > 16 ? 1 : 2);
}
int nca_dynca_bwd_grid(int B, int H, int W) { return nca_dynca_bwd_grid_c(B, 16, H, W); }   // upper bound (slab workspace sizing)
int nca_dynca_bwd_ms_grid(int B, int H, int W) { return grid_for(B * ((W + 31) / 32) * ((H + 7) / 8), 1); }

// The MLP part of one backward step (writes dh, dL/dy and, with gw2_ws, the per-workgroup dW2 | db2 partials).  acc: a later
// 128-wide slice of a wide hidden layer -- dL/dy is added to what the earlier slices wrote.
hipError_t nca_launch_dynca_step_bwd_mlp(const NcaDyncaArgs& a, hipStream_t st, bool acc) {
    if (a.pc) {   // two-scale perception (C <= 16, fc <= 128, even sizes: checked by the C ABI): one hidden slice, fused dW2 only
        if (acc || ((a.H | a.W) & 1) || !a.gw2_ws) return hipErrorInvalidValue;
        return dispatch_dynca<DyncaBwdW2Ms, kDynca12x96, kDynca16x128>(a, st);
    }
    if (a.gw2_ws)   // fused dW2 | db2: per-workgroup partials, h is not written
        return acc ? dispatch_dynca<DyncaBwdW2Acc, kDynca16x128, kDynca32x128>(a, st) : dispatch_dynca<DyncaBwdW2, kDynca12x96, kDynca32x128>(a, st);
    if (acc) return hipErrorInvalidValue;   // hidden-layer slices exist for the fused-dW2 form only
    return dispatch_dynca<DyncaBwd, kDynca12x96, kDynca32x128>(a, st);
}

// The stencil-adjoint part: g_out = g_next (+ g_extra) + adj(perception)(dybuf).
hipError_t nca_launch_dynca_step_bwd_stencil(const NcaDyncaArgs& a, hipStream_t st) {
    const size_t n = (size_t)a.B * a.C * a.H * a.W;
    const bool vec = (a.W % 4 == 0) && a.W >= 12 && a.H >= 3 && (a.g_next == nullptr || aligned16(a.g_next)) && aligned16(a.g_out) &&
                     aligned16(a.dybuf) && (a.g_extra == nullptr || aligned16(a.g_extra)) &&
                     (a.coarse_add == nullptr || (((uintptr_t)a.coarse_add & 7u) == 0 && a.H % 2 == 0));
    if (vec && a.H >= 5) {
        const size_t nb = (size_t)a.B * a.C * (4 * a.W + 8 * (a.H - 4));
        const unsigned nborder = (unsigned)((nb + 255) / 256), nvec = (unsigned)((n / 4 + 255) / 256);
        hipLaunchKernelGGL(dynca_step_bwd_stencil_vec_kernel, dim3(nborder + nvec), dim3(256), 0, st, a, nborder);
    } else {
        hipLaunchKernelGGL(dynca_step_bwd_stencil_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t nca_launch_dynca_step_bwd(const NcaDyncaArgs& a, hipStream_t st) {
    hipError_t e = nca_launch_dynca_step_bwd_mlp(a, st, false);
    if (e != hipSuccess) return e;
    return nca_launch_dynca_step_bwd_stencil(a, st);
}

// nca_cond_fire.hip -- the fire masks of a ConditionedNCA grow, drawn before its steps (gfx950).
//
// The fire mask of a step depends on (seed, step, cell) only (nca_common.h: the Philox4x32-10 stream).  The fp32
// producer/consumer step (nca_cond_pc.hip) wants it as the 64-lane ballot of a 4 x 16 wave tile; drawn inside the step every
// producer lane evaluates a whole Philox block for one of its four words, next to a consumer wave whose exact-f32 MFMAs do not
// co-issue with vector instructions.  Here each block is evaluated once, on a device that runs no MFMA at the time:
//   words[t][b][ty][tx], bit 16 * row + col  <=>  cell (4 ty + row, 16 tx + col) of batch item b fires at step step0 + t,
// the lane order of stage_tile (lane = 16 * q4 + ci).  "Fires" is the step kernels' predicate bit for bit:
//   clamp(u01(word), 0, 1) < fire_rate  on  nca_philox_group(seed, step, cell >> 2), word = cell & 3   (nca.py:171-174).
// One thread per tile: 16 block evaluations (W % 16 == 0 and H % 4 == 0 keep every block inside one tile row), one 8-byte store,
// consecutive threads on consecutive words.
#include "nca_common.h"
#include "nca_kernels.h"

namespace {

// grid (ceil(B * H/4 * W/16 / 256), Tc), block 256
__global__ __launch_bounds__(256) void cond_fire_words_kernel(unsigned long long* __restrict__ words, int B, int H, int W, float fire_rate,
                                                              uint64_t seed, uint64_t step0, unsigned* __restrict__ done_zero) {
    const int tw = W >> 4, th = H >> 2;
    const size_t per_step = (size_t)B * th * tw;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= per_step) return;
    // a grow's first chunk on the fused-steps path (nca_cond_pc.hip, MS): the tile's step counter starts at zero, and so does the abort
    // word behind the counters
    if (done_zero && blockIdx.y == 0) {
        done_zero[id] = 0u;
        if (id == 0) done_zero[per_step] = 0u;
    }
    const int tx = (int)(id % tw), ty = (int)((id / tw) % th), b = (int)(id / ((size_t)tw * th));
    const uint64_t step = step0 + blockIdx.y;
    const size_t cell0 = (size_t)b * H * W + (size_t)(4 * ty) * W + 16 * tx;
    unsigned long long word = 0ull;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t cell = cell0 + (size_t)row * W + 4 * j;   // cell & 3 == 0
            const uint4 r = nca_philox_group(seed, step, (uint32_t)(cell >> 2));
            const uint32_t w4[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const bool fires = __builtin_amdgcn_fmed3f(nca_u01(w4[l]), 0.0f, 1.0f) < fire_rate;
                word |= (unsigned long long)(fires ? 1u : 0u) << (16 * row + 4 * j + l);
            }
        }
    }
    words[(size_t)blockIdx.y * per_step + id] = word;
}

}  // namespace

// W % 16 == 0, H % 4 == 0, 1 <= Tc <= 65535, 8-byte aligned words: the callers check (nca_capi.hip)
// done_zero: null, or the per-tile step counters of the fused-steps path ([B * H/4 * W/16] + the abort word), zeroed by the same launch
hipError_t nca_launch_cond_fire_words(unsigned long long* words, int Tc, int B, int H, int W, float fire_rate, uint64_t seed, uint64_t step0,
                                      hipStream_t st, unsigned* done_zero) {
    const size_t per_step = (size_t)B * (H >> 2) * (W >> 4);
    hipLaunchKernelGGL(cond_fire_words_kernel, dim3((unsigned)((per_step + 255) / 256), (unsigned)Tc), dim3(256), 0, st, words, B, H, W,
                       fire_rate, seed, step0, done_zero);
    return hipGetLastError();
}

// nca_ot_sample.hip -- the OT appearance loss's position sampler on gfx950: what the reference draws on the host as
// np.sort(np.random.choice(np.arange(h * w), n, replace=False)) (EncoderConditioning/loss/appearance_loss.py:200-203), once per
// (sample, sampled layer), as a keyed draw on the device.
//
// A row is one (call, layer, sample) triple with a 64-bit id `row`.  Position p in [0, HW) gets the key
//     words = philox4x32_10(counter = (p >> 2, row_lo, row_hi, 'OTS' = 0x4F5453), key = (seed_lo, seed_hi)),
//     key(p) = words[p & 3] >> (32 - key_bits),                                               1 <= key_bits <= 32,
// and the row's result is the n positions with the smallest (key, p) in lexicographic order, written in ascending p (the
// reference's np.sort).  Distinct keys make every n-subset equally likely; with 32-bit keys the tie-break by position matters only
// for a tie exactly at the threshold, probability about HW * 2^-32 per row -- the documented deviation from an exactly uniform
// subset.  Small key_bits make ties the common case: that is how the tie path is tested.
//
// One workgroup per row, nothing shared between workgroups, no global atomics:
//   threshold  MSB-first radix select over the keys, 8-bit digits (the top digit narrower when key_bits % 8 != 0), at most 4
//              passes.  A pass counts, in a 256-bin LDS histogram (integer atomics: counts do not depend on order), the positions
//              whose higher digits equal the prefix found so far; wave 0 scans the bins for the digit in which the cumulative count
//              crosses the remaining quota.  Result: the threshold key tau (the n-th smallest key), m = #{key < tau}, need = n - m.
//   emit       one more pass in position order, 4096 positions per chunk: each lane flags key < tau and key == tau for its four
//              positions, wave ballots + popcounts give in-wave ranks, LDS the cross-wave bases, two running counters carry
//              across chunks.  A tie is taken iff its running tie rank is < need; idx[row, rank] = p with plain vector stores.
// Keys are regenerated from Philox in every pass (65 536 keys do not fit next to anything else in LDS): one evaluation yields four
// positions' keys, so a lane owns whole groups of 4.
#include "nca_common.h"
#include "nca_kernels.h"

namespace {

constexpr int kSmpThreads = 1024, kSmpWaves = kSmpThreads / NCA_WAVE;

__device__ __forceinline__ void smp_keys(uint32_t (&k)[4], uint32_t group, uint32_t row_lo, uint32_t row_hi, uint2 seed, int drop) {
    const uint4 r = nca_philox4x32_10(make_uint4(group, row_lo, row_hi, 0x4F5453u), seed);
    k[0] = r.x >> drop;
    k[1] = r.y >> drop;
    k[2] = r.z >> drop;
    k[3] = r.w >> drop;
}

// grid rows, block 1024.  idx [rows, n].
__global__ __launch_bounds__(kSmpThreads) void ot_sample_kernel(int* __restrict__ idx, int HW, int n, uint64_t seed, uint64_t row0,
                                                                 int key_bits) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[2];                       // the pass's digit, and the count below it
    __shared__ unsigned wtot[2][2][kSmpWaves];        // [chunk parity][key < tau / key == tau][wave]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t row = row0 + (uint64_t)blockIdx.x;
    const uint32_t row_lo = (uint32_t)row, row_hi = (uint32_t)(row >> 32);
    const uint2 sd = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const int drop = 32 - key_bits;
    const int groups = (HW + 3) >> 2;
    int* const out = idx + (size_t)blockIdx.x * n;

    // ---- threshold ----
    uint32_t prefix = 0;                              // the digits found so far
    unsigned quota = (unsigned)n;                     // how many of the positions that match the prefix are still to be taken
    for (int shift = ((key_bits - 1) >> 3) << 3; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int g = tid; g < groups; g += kSmpThreads) {
            uint32_t k[4];
            smp_keys(k, (uint32_t)g, row_lo, row_hi, sd, drop);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // 64-bit shift: shift + 8 is 32 in the first of four passes, where nothing lies above the digit and the prefix is 0
                if (4 * g + j < HW && (uint32_t)((uint64_t)k[j] >> (shift + 8)) == prefix) atomicAdd(&hist[(k[j] >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {                              // lane l holds bins 4 l .. 4 l + 3
            const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const unsigned own = (h0 + h1) + (h2 + h3);
            unsigned incl = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            unsigned below = incl - own;
            if (below < quota && quota <= incl) {     // exactly one lane: the matching positions are at least `quota` many
                unsigned digit = 4u * lane;
                if (below + h0 < quota) {
                    below += h0;
                    ++digit;
                    if (below + h1 < quota) {
                        below += h1;
                        ++digit;
                        if (below + h2 < quota) {
                            below += h2;
                            ++digit;
                        }
                    }
                }
                sel[0] = digit;
                sel[1] = below;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | sel[0];
        quota -= sel[1];
    }
    const uint32_t tau = prefix;
    const unsigned need = quota;                      // ties at tau to take, in position order (1 <= need <= #{key == tau})

    // ---- emit ----
    const unsigned long long below_me = (1ull << lane) - 1ull;
    unsigned base_lt = 0, base_eq = 0;                // positions before this chunk with key < tau / key == tau
    const int chunks = (groups + kSmpThreads - 1) / kSmpThreads;
    for (int ch = 0; ch < chunks; ++ch) {
        const int g = ch * kSmpThreads + tid;
        bool lt[4] = {false, false, false, false}, eq[4] = {false, false, false, false};
        if (g < groups) {
            uint32_t k[4];
            smp_keys(k, (uint32_t)g, row_lo, row_hi, sd, drop);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = 4 * g + j < HW;
                lt[j] = in && k[j] < tau;
                eq[j] = in && k[j] == tau;
            }
        }
        unsigned lt_before = 0, eq_before = 0, lt_wave = 0, eq_wave = 0;      // in this wave: lanes below / all lanes
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long bl = __ballot(lt[j]), be = __ballot(eq[j]);
            lt_before += __popcll(bl & below_me);
            eq_before += __popcll(be & below_me);
            lt_wave += __popcll(bl);
            eq_wave += __popcll(be);
        }
        unsigned (&wt)[2][kSmpWaves] = wtot[ch & 1];  // two buffers: the next chunk's writes cannot overtake this chunk's reads
        if (lane == 0) {
            wt[0][wave] = lt_wave;
            wt[1][wave] = eq_wave;
        }
        __syncthreads();
        unsigned lt_all = 0, eq_all = 0;
#pragma unroll
        for (int w = 0; w < kSmpWaves; ++w) {
            const unsigned a = wt[0][w], b = wt[1][w];
            if (w < wave) {
                lt_before += a;
                eq_before += b;
            }
            lt_all += a;
            eq_all += b;
        }
        unsigned nlt = base_lt + lt_before, neq = base_eq + eq_before;       // before this lane's first position
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool take = lt[j] || (eq[j] && neq < need);
            const unsigned rank = nlt + min(neq, need);
            if (take && rank < (unsigned)n) out[rank] = 4 * g + j;
            nlt += lt[j] ? 1u : 0u;
            neq += eq[j] ? 1u : 0u;
        }
        base_lt += lt_all;
        base_eq += eq_all;
    }
}

}  // namespace

hipError_t nca_launch_ot_sample(int* idx, int rows, int HW, int n, uint64_t seed, uint64_t row0, int key_bits, hipStream_t st) {
    hipLaunchKernelGGL(ot_sample_kernel, dim3(rows), dim3(kSmpThreads), 0, st, idx, HW, n, seed, row0, key_bits);
    return hipGetLastError();
}

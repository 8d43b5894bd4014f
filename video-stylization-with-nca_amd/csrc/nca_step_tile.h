// nca_step_tile.h -- what the two 8 x 32-tile step kernels share (dynca_step_fwd_kernel in nca_dynca_step.h, cond_step_fwd_kernel
// in nca_cond_generic.hip): the gathers that build the LDS weight images, the halo-1 state-tile staging and the two launch helpers.
#pragma once
#include "nca_common.h"
#include "nca_dynca_bf16.h"
#include "nca_kernels.h"

namespace {

constexpr int kThreads = 256;

constexpr int lds_cs(int rows, int rs) {  // channel stride with CS % 32 == 16 (conflict-free g/g+1 pairs)
    int cs = rows * rs;
    while (cs % 32 != 16) ++cs;
    return cs;
}

__device__ __forceinline__ float nca_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// Batched gather of a weight image: dst[idx] = map(idx) >= 0 ? src[map(idx)] : 0, 8 independent loads
// in flight per thread (a dependent-latency loop here costs tens of microseconds per launch).
template <int N, typename MapT>
__device__ __forceinline__ void fill_image(float* __restrict__ dst, const float* __restrict__ src, int tid, MapT map) {
    constexpr int U = 8;
    for (int base = tid; base < N; base += kThreads * U) {
        float v[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = base + kThreads * u;
            const long o = idx < N ? map(idx) : -1;
            ok[u] = o >= 0;
            v[u] = src[ok[u] ? o : 0];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int idx = base + kThreads * u;
            if (idx < N) dst[idx] = ok[u] ? v[u] : 0.0f;
        }
    }
}

// Two-phase form of the same gather: fill_issue requests EVERY element of an image (one register each), fill_commit writes
// them to LDS.  Issuing all images before committing any makes the workgroup's cold start ONE memory round trip instead of one
// per batch of 8 (at B = 1 -- the video loop -- a launch is one tile per workgroup and the prologue is most of it).
template <int N>
struct FillV { float v[(N + kThreads - 1) / kThreads]; };
template <int N, typename MapT>
__device__ __forceinline__ void fill_issue(FillV<N>& r, const float* __restrict__ src, int tid, MapT map) {
#pragma unroll
    for (int u = 0; u < (N + kThreads - 1) / kThreads; ++u) {
        const int idx = tid + kThreads * u;
        const long o = idx < N ? map(idx) : -1;
        r.v[u] = src[o >= 0 ? o : 0];
    }
}
template <int N, typename MapT>
__device__ __forceinline__ void fill_commit(const FillV<N>& r, float* __restrict__ dst, int tid, MapT map) {
#pragma unroll
    for (int u = 0; u < (N + kThreads - 1) / kThreads; ++u) {
        const int idx = tid + kThreads * u;
        if (idx < N) dst[idx] = map(idx) >= 0 ? r.v[u] : 0.0f;
    }
}

// bf16 weight images (nca_dynca_bf16.h): one 32-bit word = two consecutive k values of one lane, rounded to nearest even at commit
template <int N>
struct FillP { float lo[(N + kThreads - 1) / kThreads], hi[(N + kThreads - 1) / kThreads]; };
template <int N, typename MapT>
__device__ __forceinline__ void fill_issue_pk(FillP<N>& r, const float* __restrict__ src, int tid, MapT map) {
#pragma unroll
    for (int u = 0; u < (N + kThreads - 1) / kThreads; ++u) {
        const int idx = tid + kThreads * u;
        const long o0 = idx < N ? map(idx, 0) : -1, o1 = idx < N ? map(idx, 1) : -1;
        r.lo[u] = src[o0 >= 0 ? o0 : 0];
        r.hi[u] = src[o1 >= 0 ? o1 : 0];
    }
}
template <int N, typename MapT>
__device__ __forceinline__ void fill_commit_pk(const FillP<N>& r, float* __restrict__ dst, int tid, MapT map) {
#pragma unroll
    for (int u = 0; u < (N + kThreads - 1) / kThreads; ++u) {
        const int idx = tid + kThreads * u;
        if (idx < N) dst[idx] = __uint_as_float(nca_pk_bf16(map(idx, 0) >= 0 ? r.lo[u] : 0.0f, map(idx, 1) >= 0 ? r.hi[u] : 0.0f));
    }
}

// ---- halo-1 tile staging -------------------------------------------------------------------
// LDS tile Z[ch][r][zq]: r = 0..TH+1 (image row ty0-1+r), zq = q+3 where q = 0..TW+1 is the halo-1
// column (image col tx0-1+q), so the interior starts 16-byte aligned at zq = 4.  Row stride TW+8.
// Thread t of each 128-thread half owns one POSITION: an interior 4-cell group (r, 4 cols) or one
// halo cell; the two halves split the channels.  Address math happens once per thread.
template <int TH, int TW>
struct TilePos {
    static constexpr int F4 = TW / 4, ROWS = TH + 2, RS = TW + 8;
    static constexpr int NINT = ROWS * F4, NPOS = NINT + 2 * ROWS;
    static_assert(NPOS <= 128, "positions must fit one 128-thread half");
    int r, q;          // halo-1 coordinates of the first element
    bool active, interior, vec;
    unsigned eo[4];    // plane offsets of the (up to) 4 elements, always dereferenceable
    bool ev[4];        // element is real (inside the image / pad-resolved)

    template <bool VEC>
    __device__ __forceinline__ void init(int tid, int ty0, int tx0, int H, int W, int pad) {
        const int p = tid & 127;
        active = p < NPOS;
        interior = p < NINT;
        if (interior) {
            r = p / F4;
            q = 1 + 4 * (p % F4);
        } else {
            const int h = p - NINT;
            r = (h >> 1) % ROWS;
            q = (h & 1) ? TW + 1 : 0;
        }
        const int sy = nca_pad_index(ty0 - 1 + r, H, pad);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sx = nca_pad_index(tx0 - 1 + q + j, W, pad);
            ev[j] = active && sy >= 0 && sx >= 0 && (interior || j == 0);
            eo[j] = ev[j] ? (unsigned)(sy * W + sx) : 0u;
        }
        vec = VEC && interior && ev[0] && (tx0 - 1 + q + 3 < W);
    }
};

// Loads planes clamp(ch0 + c - sub, 0, C-1), c = 0..CPH-1, of this thread's position (the caller
// zeroes/ignores slots whose unclamped index is out of range).  `base` is wave-uniform; offsets are
// 32-bit (one sample's planes stay below 2^31 elements) so the loads take the saddr+voffset form.
template <int CPH, typename PosT>
__device__ __forceinline__ void pos_load(const PosT& ps, const float* __restrict__ base, unsigned plane, int ch0, int sub,
                                         int C, float (&v)[CPH][4]) {
    if (ps.vec) {
#pragma unroll
        for (int c = 0; c < CPH; ++c) {
            const unsigned ch = (unsigned)min(max(ch0 + c - sub, 0), C - 1);
            const float4 t = *reinterpret_cast<const float4*>(base + (ch * plane + ps.eo[0]));
            v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        }
    } else {  // halo cells, image-edge overhang, unaligned rows: per-element (masked elements re-read eo = 0)
#pragma unroll
        for (int c = 0; c < CPH; ++c) {
            const unsigned ch = (unsigned)min(max(ch0 + c - sub, 0), C - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = base[ch * plane + ps.eo[j]];
        }
    }
}

// bf16 storage (ncahip_dynca_*_bf16): the same positions, 2-byte elements.  Raw bits are kept until staging consumes
// them (converting at load time would wait for the load): v4 holds the 8-byte group of the vector path, v1 the four
// halfwords of the per-element path.
typedef unsigned nca_u32x2 __attribute__((ext_vector_type(2)));
template <int CPH>
struct RawB16 {
    unsigned v1[CPH][4];   // vector path: [0..1] = the 8-byte group; per-element path: one halfword each
};
template <int CPH, typename PosT>
__device__ __forceinline__ void pos_load_b16(const PosT& ps, const uint16_t* __restrict__ base, unsigned plane, int ch0, int C,
                                             RawB16<CPH>& r) {
    if (ps.vec) {
#pragma unroll
        for (int c = 0; c < CPH; ++c) {
            const unsigned ch = (unsigned)min(ch0 + c, C - 1);
            const nca_u32x2 t = *reinterpret_cast<const nca_u32x2*>(base + (ch * plane + ps.eo[0]));
            r.v1[c][0] = t[0];
            r.v1[c][1] = t[1];
        }
    } else {
#pragma unroll
        for (int c = 0; c < CPH; ++c) {
            const unsigned ch = (unsigned)min(ch0 + c, C - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) r.v1[c][j] = base[ch * plane + ps.eo[j]];
        }
    }
}
__device__ __forceinline__ float nca_b16_to_f32(unsigned bits16) { return __uint_as_float(bits16 << 16); }
// round-to-nearest-even f32 -> bf16 (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint16_t nca_f32_to_b16(float v) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    return (uint16_t)(__builtin_bit_cast(unsigned, __builtin_convertvector(f2{v, 0.0f}, b2)) & 0xffffu);
}

template <typename PosT>
__device__ __forceinline__ void pos_store(const PosT& ps, float* __restrict__ Zc /* &Z[ch][0][0] */, const float (&v)[4]) {
    float* const d = Zc + ps.r * PosT::RS + ps.q + 3;
    if (ps.interior) *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    else d[0] = v[0];
}

// ---- host-side launch helpers -------------------------------------------------------------
inline int grid_for(int ntiles, int wg_per_cu) {
    const int cap = nca_cu_count() * wg_per_cu;
    return ntiles < cap ? ntiles : cap;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

// nca_cond_generic.hip -- the generic (any-shape) fused ConditionedNCA step kernel, and the dispatch of the ConditionedNCA step
// over its kernel families (this one, nca_cond_pc.hip, nca_cond_wave.hip) with the test hooks that steer it.  Work decomposition
// and MFMA mapping are those of the DyNCA step kernel: see the header of nca_dynca_step.h.
// Built only through nca_step.hip, which includes this file: never list it in the Makefile's SRCS beside that unit (duplicate symbols).
#include <cstdlib>

#include "nca_step_tile.h"

namespace {

// =========================================================================================
// ConditionedNCA step (EncoderConditioning/nca.py:181-195), pending-life-mask protocol
// =========================================================================================
template <int CP, int TH, int TW, int NT>
struct CondCfg {
    static constexpr int HID = 64;
    static constexpr int K1S = 3 * CP / 4;
    static constexpr int M3T = (CP + 15) / 16;
    static constexpr int ROWS = TH + 2, RS = TW + 8;
    static constexpr int CS = lds_cs(ROWS, RS);
    static constexpr int PNS = TW + 2;                // pre-mask tile, halo 1
    static constexpr int A3R = TH + 6, A3S = TW + 6;  // alpha', halo 3
    static constexpr int L2R = TH + 4, L2S = TW + 4;  // life / resolved alpha, halo 2
    static constexpr int NA3 = A3R * A3S, NL2 = L2R * L2S, NPN = ROWS * PNS;
    static constexpr int KA3 = (NA3 + kThreads - 1) / kThreads, KL2 = (NL2 + kThreads - 1) / kThreads,
                         KPN = (NPN + kThreads - 1) / kThreads;
    static constexpr int WPS = 28;  // 27 taps padded
    static constexpr int TWN = TW / 16;
    static constexpr int NTILES16 = TH * TW / 16;
    static constexpr int ITERS = NTILES16 / (4 * NT);
    static constexpr int CPH = CP / 2;
    static constexpr int OFF_W1 = 0;
    static constexpr int OFF_W2 = OFF_W1 + 4 * K1S * 64;
    static constexpr int OFF_W3 = OFF_W2 + 4 * 16 * 64;
    static constexpr int OFF_B1 = OFF_W3 + M3T * 16 * 64;
    static constexpr int OFF_B2 = OFF_B1 + HID;
    static constexpr int OFF_WP = OFF_B2 + HID;
    static constexpr int OFF_Z = OFF_WP + CP * WPS;
    static constexpr int OFF_A3 = OFF_Z + CP * CS;
    static constexpr int OFF_LIFE = OFF_A3 + NA3;
    static constexpr int OFF_A2 = OFF_LIFE + NL2;
    static constexpr int OFF_PN = OFF_A2 + NL2;
    static constexpr int OFF_MK = OFF_PN + NPN;
    static constexpr int LDS_FLOATS = OFF_MK + TH * TW;
    static_assert(CP % 4 == 0 && TW % 16 == 0 && NTILES16 % (4 * NT) == 0, "shape");
    static_assert(OFF_Z % 4 == 0 && OFF_WP % 4 == 0 && CS % 4 == 0 && TH * TW == kThreads, "16-byte carve");
};

__device__ __forceinline__ float nca_max3x3(const float* p, int stride) {
    float m = fmaxf(fmaxf(p[-stride - 1], p[-stride]), p[-stride + 1]);
    m = fmaxf(m, fmaxf(fmaxf(p[-1], p[0]), p[1]));
    return fmaxf(m, fmaxf(fmaxf(p[stride - 1], p[stride]), p[stride + 1]));
}

template <int CP, int TH, int TW, int NT, bool VEC>
__global__ __launch_bounds__(kThreads, CP > 16 ? 1 : 2) void cond_step_fwd_kernel(const NcaCondArgs a) {   // CP > 16: 84+ KB of LDS -> one workgroup per CU anyway: 512 registers per lane
    using K = CondCfg<CP, TH, TW, NT>;
    using Pos = TilePos<TH, TW>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const W1L = smem + K::OFF_W1;
    float* const W2L = smem + K::OFF_W2;
    float* const W3L = smem + K::OFF_W3;
    float* const B1L = smem + K::OFF_B1;
    float* const B2L = smem + K::OFF_B2;
    float* const WPL = smem + K::OFF_WP;
    float* const Z = smem + K::OFF_Z;
    float* const A3 = smem + K::OFF_A3;
    float* const LIFE = smem + K::OFF_LIFE;
    float* const A2 = smem + K::OFF_A2;
    float* const PN = smem + K::OFF_PN;
    float* const MK = smem + K::OFF_MK;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, ci = lane & 15;
    const int C = a.C, H = a.H, W = a.W, hid = a.hidden;
    const int K1 = 3 * C;
    const int gch0 = C - a.goal_ch;  // first channel the goal encoding is added to (nca.py:199-203)
    const bool pending = a.pre_in != nullptr;
    const bool use_alive = a.alive_ch >= 0;
    const bool has_goal = a.goal_ch > 0;

    fill_image<4 * K::K1S * 64>(W1L, a.w1, tid, [&](int idx) -> long {
        const int l = idx & 63, s = (idx >> 6) % K::K1S, m = (idx >> 6) / K::K1S;
        const int gg = l >> 4, o = 16 * m + (l & 15);
        const int ch = 4 * (s / 3) + gg, f = s % 3;  // k-step s = 3c'+f : channel 4c'+g, filter f
        return (ch < C && o < hid) ? (long)o * K1 + 3 * ch + f : -1;  // out[3c+f], nca.py:99-107
    });
    fill_image<4 * 16 * 64>(W2L, a.w2, tid, [&](int idx) -> long {
        const int l = idx & 63, s = (idx >> 6) % 16, m = (idx >> 6) / 16;
        const int gg = l >> 4, o = 16 * m + (l & 15);
        const int k = 16 * (s >> 2) + 4 * gg + (s & 3);
        return (o < hid && k < hid) ? (long)o * hid + k : -1;
    });
    fill_image<K::M3T * 16 * 64>(W3L, a.w3, tid, [&](int idx) -> long {
        const int l = idx & 63, s = (idx >> 6) % 16, m = (idx >> 6) / 16;
        const int gg = l >> 4, o = 16 * m + (l & 15);
        const int k = 16 * (s >> 2) + 4 * gg + (s & 3);
        return (o < C && k < hid) ? (long)o * hid + k : -1;
    });
    fill_image<K::HID>(B1L, a.b1, tid, [&](int idx) -> long { return idx < hid ? idx : -1; });
    fill_image<K::HID>(B2L, a.b2, tid, [&](int idx) -> long { return idx < hid ? idx : -1; });
    fill_image<CP * K::WPS>(WPL, a.wp, tid, [&](int idx) -> long {
        const int ch = idx / K::WPS, j = idx % K::WPS;
        return (ch < C && j < 27) ? (long)ch * 27 + j : -1;  // [3c+f][3][3] == [c][f*9+tap]
    });

    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int ntiles = a.B * tiles_x * tiles_y;
    const size_t plane = (size_t)H * W;

    for (NcaTileWalk tw = nca_tile_walk(ntiles); tw.t < tw.end; tw.t += tw.stride) {
        const int txi = tw.t % tiles_x, tyi = (tw.t / tiles_x) % tiles_y, b = tw.t / (tiles_x * tiles_y);
        const int ty0 = tyi * TH, tx0 = txi * TW;
        const float* const xb = a.x_in + (size_t)b * C * plane;

        // ---- issue every global load of the tile ------------------------------------------
        // (staging index made opaque per tile so its derived coordinates are recomputed, not kept
        //  live -- or spilled -- across the MFMA phase)
        int st = tid;
        asm volatile("" : "+v"(st));
        const int half = st >> 7;
        // alpha' (halo 3), pre_in (halo 2), u: needed first
        float a3v[K::KA3];
        bool a3in[K::KA3];
        if (use_alive) {
#pragma unroll
            for (int k = 0; k < K::KA3; ++k) {
                const int idx = st + k * kThreads;
                const int q = idx % K::A3S, r = idx / K::A3S, gy = ty0 - 3 + r, gx = tx0 - 3 + q;
                a3in[k] = idx < K::NA3 && gy >= 0 && gy < H && gx >= 0 && gx < W;
                a3v[k] = xb[a.alive_ch * plane + (a3in[k] ? (size_t)gy * W + gx : 0)];
            }
        }
        float l2v[K::KL2];
        bool l2in[K::KL2];
#pragma unroll
        for (int k = 0; k < K::KL2; ++k) {
            const int idx = st + k * kThreads;
            const int q = idx % K::L2S, r = idx / K::L2S, gy = ty0 - 2 + r, gx = tx0 - 2 + q;
            l2in[k] = idx < K::NL2 && gy >= 0 && gy < H && gx >= 0 && gx < W;
            l2v[k] = 1.0f;
            if (pending && use_alive) l2v[k] = (float)a.pre_in[(size_t)b * plane + (l2in[k] ? (size_t)gy * W + gx : 0)];
        }
        const int cr = st / TW, cq = st % TW, cgy = ty0 + cr, cgx = tx0 + cq;  // this thread's cell
        const bool cin = cgy < H && cgx < W;
        const size_t cell = (size_t)b * plane + (cin ? (size_t)cgy * W + cgx : 0);
        float uu = 0.0f;
        if (a.u) {   // explicit uniforms, or bit-packed masks: bit 1 -> clamp(0) < rate, bit 0 -> clamp(2) = 1 < rate never (rate <= 1)
            if (a.u_bits) uu = ((reinterpret_cast<const uint32_t*>(a.u)[cell >> 5] >> (unsigned)(cell & 31)) & 1u) ? 0.0f : 2.0f;
            else uu = a.u[cell];
        }
        // state tile + goal encoding (halo 1): one position per thread, channels split over the two halves
        Pos ps;
        ps.template init<VEC>(st, ty0, tx0, H, W, NCA_PAD_ZERO);
        float xv[K::CPH][4], gv[K::CPH][4];
        pos_load<K::CPH>(ps, xb, (unsigned)plane, half * K::CPH, 0, C, xv);
        if (has_goal)  // slot c holds goal plane (half*CPH + c) - gch0 (used only when that index is >= 0)
            pos_load<K::CPH>(ps, a.goal + (size_t)b * a.goal_ch * plane, (unsigned)plane, half * K::CPH, gch0, a.goal_ch, gv);

        __syncthreads();  // previous tile fully consumed
        // ---- S1: alpha' with -inf outside the image (= max_pool2d padding), pre_in -----------
        if (use_alive) {
#pragma unroll
            for (int k = 0; k < K::KA3; ++k) {
                const int idx = st + k * kThreads;
                if (idx < K::NA3) A3[idx] = a3in[k] ? a3v[k] : NCA_NEG_INF;
            }
        }
#pragma unroll
        for (int k = 0; k < K::KL2; ++k) {
            const int idx = st + k * kThreads;
            if (idx < K::NL2) LIFE[idx] = l2in[k] ? l2v[k] : 0.0f;
        }
        __syncthreads();
        // ---- S2: life = pre & post of the PREVIOUS step; resolved alpha (nca.py:191-194) ----
        if (use_alive) {
#pragma unroll
            for (int k = 0; k < K::KL2; ++k) {
                const int idx = st + k * kThreads;
                if (idx < K::NL2) {
                    const int q = idx % K::L2S, r = idx / K::L2S;
                    const float* const ac = A3 + (r + 1) * K::A3S + q + 1;
                    float life = l2in[k] ? l2v[k] : 0.0f, av = NCA_NEG_INF;
                    if (l2in[k]) {
                        if (pending) {
                            life = (life != 0.0f && nca_max3x3(ac, K::A3S) > a.thr) ? 1.0f : 0.0f;
                            av = nca_clamp(ac[0] * life, a.lo, a.hi);
                        } else {
                            av = ac[0];
                        }
                    }
                    LIFE[idx] = life;
                    A2[idx] = av;
                }
            }
        }
        __syncthreads();
        // ---- S3: pre-life mask of THIS step (halo 1), fire mask --------------------------
#pragma unroll
        for (int k = 0; k < K::KPN; ++k) {
            const int idx = st + k * kThreads;
            if (idx < K::NPN) {
                const int q = idx % K::PNS, r = idx / K::PNS, gy = ty0 - 1 + r, gx = tx0 - 1 + q;
                float pn = 0.0f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    pn = (!use_alive || nca_max3x3(A2 + (r + 1) * K::L2S + q + 1, K::L2S) > a.thr) ? 1.0f : 0.0f;
                    if (r >= 1 && r <= TH && q >= 1 && q <= TW)
                        a.pre_out[(size_t)b * plane + (size_t)gy * W + gx] = (uint8_t)pn;
                }
                PN[idx] = pn;
            }
        }
        if (!a.u) uu = nca_philox_cell(a.seed, a.step, cell);
        MK[st] = (cin && nca_clamp(uu, 0.0f, 1.0f) < a.fire_rate) ? 1.0f : 0.0f;  // nca.py:171-174
        __syncthreads();
        // ---- S4: z = x + goal * pre (nca.py:177) on halo 1, zero outside the image -------
        if (ps.active) {
            const float* const lf = LIFE + (ps.r + 1) * K::L2S + ps.q + 1;
            const float* const pnp = PN + ps.r * K::PNS + ps.q;
            float lfv[4], pnv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool rd = ps.interior || j == 0;
                lfv[j] = rd ? lf[j] : 0.0f;
                pnv[j] = rd ? pnp[j] : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < K::CPH; ++c) {
                const int ch = half * K::CPH + c;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float t = 0.0f;
                    if (ch < C && ps.ev[j]) {
                        t = xv[c][j];
                        if (pending) t = nca_clamp(t * lfv[j], a.lo, a.hi);
                    }
                    v[j] = t;
                }
                if (has_goal && ch >= gch0 && ch < C) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ps.ev[j]) v[j] = fmaf(gv[c][j], pnv[j], v[j]);
                }
                pos_store(ps, Z + ch * K::CS, v);
            }
        }
        __syncthreads();

#pragma unroll 1
        for (int it = 0; it < K::ITERS; ++it) {
            int r0[NT], q0[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int j = (it * 4 + wave) * NT + n;
                r0[n] = j / K::TWN;
                q0[n] = (j % K::TWN) * 16 + ci;
            }
            // ---- learned depthwise perception (nca.py:99-107): P[3c'+f] for channel 4c'+g
            float P[NT][K::K1S];
#pragma unroll
            for (int cq4 = 0; cq4 < CP / 4; ++cq4) {
                const float* const zc = Z + (4 * cq4 + g) * K::CS + 3;
                float wt[28];
#pragma unroll
                for (int j4 = 0; j4 < 7; ++j4) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(WPL + (4 * cq4 + g) * K::WPS + 4 * j4);
                    wt[4 * j4 + 0] = w4[0]; wt[4 * j4 + 1] = w4[1]; wt[4 * j4 + 2] = w4[2]; wt[4 * j4 + 3] = w4[3];
                }
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    float nb[9];
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) nb[3 * dy + dx] = zc[(r0[n] + dy) * K::RS + q0[n] + dx];
#pragma unroll
                    for (int f = 0; f < 3; ++f) {
                        float acc = 0.0f;
#pragma unroll
                        for (int t = 0; t < 9; ++t) acc = fmaf(wt[9 * f + t], nb[t], acc);
                        P[n][3 * cq4 + f] = acc;
                    }
                }
            }
            // ---- UpdateNet (nca.py:40-46): 3C -> 64 -> 64 -> C ---------------------------
            f32x4 acc2[4][NT];
#pragma unroll
            for (int m2 = 0; m2 < 4; ++m2) {
                const f32x4 bias = *reinterpret_cast<const f32x4*>(B2L + 16 * m2 + 4 * g);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc2[m2][n] = bias;
            }
#pragma unroll 1
            for (int m = 0; m < 4; ++m) {
                const float* const w1m = W1L + m * K::K1S * 64 + lane;
                const f32x4 bias = *reinterpret_cast<const f32x4*>(B1L + 16 * m + 4 * g);
                f32x4 acc1[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) acc1[n] = bias;
#pragma unroll
                for (int s = 0; s < K::K1S; ++s) {
                    const float wa = w1m[s * 64];
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc1[n] = nca_mfma(wa, P[n][s], acc1[n]);
                }
                const float* const w2m = W2L + (4 * m) * 64 + lane;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int m2 = 0; m2 < 4; ++m2) {
                        const float wa = w2m[(m2 * 16 + r) * 64];
#pragma unroll
                        for (int n = 0; n < NT; ++n)
                            acc2[m2][n] = nca_mfma(wa, fmaxf(acc1[n][r], 0.0f), acc2[m2][n]);
                    }
                }
            }
            f32x4 acc3[K::M3T][NT];
#pragma unroll
            for (int m3 = 0; m3 < K::M3T; ++m3)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc3[m3][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};  // out.4 has no bias
#pragma unroll
            for (int m = 0; m < 4; ++m) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int m3 = 0; m3 < K::M3T; ++m3) {
                        const float wa = W3L[(m3 * 16 + 4 * m + r) * 64 + lane];
#pragma unroll
                        for (int n = 0; n < NT; ++n)
                            acc3[m3][n] = nca_mfma(wa, fmaxf(acc2[m][n][r], 0.0f), acc3[m3][n]);
                    }
                }
            }
            // ---- x' = x + rand_mask * out (nca.py:189); stays pending ---------------------
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int gy = ty0 + r0[n], gx = tx0 + q0[n];
                if (gy < H && gx < W) {
                    const float mk = MK[r0[n] * TW + q0[n]];
                    const float life = LIFE[(r0[n] + 2) * K::L2S + q0[n] + 2];
                    const size_t off = (size_t)gy * W + gx;
                    float* const ob = a.x_out + (size_t)b * C * plane + off;
                    float xo[K::M3T][4];
#pragma unroll
                    for (int m3 = 0; m3 < K::M3T; ++m3)
#pragma unroll
                        for (int r = 0; r < 4; ++r) xo[m3][r] = xb[min(16 * m3 + 4 * g + r, C - 1) * plane + off];
#pragma unroll
                    for (int m3 = 0; m3 < K::M3T; ++m3)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = 16 * m3 + 4 * g + r;
                            if (ch < C) {
                                float x0 = xo[m3][r];
                                if (pending) x0 = nca_clamp(x0 * life, a.lo, a.hi);
                                ob[ch * plane] = x0 + mk * acc3[m3][n][r];
                            }
                        }
                }
            }
        }
    }
}

// ---- host-side launch helpers -------------------------------------------------------------
template <int CP, bool VEC>
hipError_t launch_cond_v(const NcaCondArgs& a, hipStream_t st) {
    constexpr int TH = 8, TW = 32, NT = 4;   // (C > 16 ran two rows per pass while it was compiled for 256 registers; one workgroup per CU has 512)
    using K = CondCfg<CP, TH, TW, NT>;
    auto kern = cond_step_fwd_kernel<CP, TH, TW, NT, VEC>;
    const size_t lds = (size_t)K::LDS_FLOATS * sizeof(float);
    static NcaLdsAttr attr;   // per instantiation; keyed by device inside
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(kern), lds); e != hipSuccess) return e;
    const int ntiles = a.B * ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
    const int grid = grid_for(ntiles, lds * 2 <= 160 * 1024 ? 2 : 1);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, st, a);
    return hipGetLastError();
}

template <int CP>
hipError_t launch_cond(const NcaCondArgs& a, hipStream_t st) {
    const bool vec = (a.W % 4 == 0) && aligned16(a.x_in) && (a.goal == nullptr || aligned16(a.goal));
    return vec ? launch_cond_v<CP, true>(a, st) : launch_cond_v<CP, false>(a, st);
}

}  // namespace

// ---- the dispatch (modes: nca_modes.h): smallest instantiation that covers C; padding lanes carry zero weights ---

// the tile kernels address with 32-bit byte offsets from the batch item's base (issue_loads): H*W < 2^24, C*H*W*4 < 2^32
static bool cond_tiled(const NcaCondArgs& a) {
    const bool small = (size_t)a.H * a.W < ((size_t)1 << 24) && (size_t)(a.C <= 16 ? 16 : 20) * a.H * a.W * 4 < ((size_t)1 << 32);
    return !nca_modes().force_generic && small && (a.W % 4 == 0) && aligned16(a.x_in) && aligned16(a.x_out) && (a.goal == nullptr || aligned16(a.goal));
}

bool nca_cond_fire_words_ok(const NcaCondArgs& a) {
    return cond_tiled(a) && a.C <= 20 && nca_modes().cond_variant != 1 && a.u == nullptr && a.W % 16 == 0 && a.H % 4 == 0 && nca_cond_pc_fire_words_ok(a);
}

hipError_t nca_launch_cond_step_fwd(const NcaCondArgs& a, hipStream_t st) {
    const bool tiled = cond_tiled(a);
    if (tiled && a.C <= 16) return nca_modes().cond_variant == 1 ? nca_launch_cond_step_fwd_wave(a, st) : nca_launch_cond_step_fwd_pc(a, st);
    if (tiled && a.C <= 20) return nca_launch_cond_step_fwd_pc(a, st);   // the reference's default C = 20: producer/consumer kernel, wide carve
    if (a.C <= 12) return launch_cond<12>(a, st);
    if (a.C <= 16) return launch_cond<16>(a, st);
    // the reference's default model is C = 3 + 1 + 16 = 20 (nca.py:62-94): the generic kernel family with two output tiles
    if (a.C <= 20) return launch_cond<20>(a, st);
    if (a.C <= 24) return launch_cond<24>(a, st);
    if (a.C <= 32) return launch_cond<32>(a, st);
    return hipErrorInvalidValue;
}

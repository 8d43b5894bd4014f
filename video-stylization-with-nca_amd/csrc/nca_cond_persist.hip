// nca_cond_persist.hip -- a whole ConditionedNCA grow (T steps + the final finalize) in ONE launch for small grids, gfx950, fp32.
//
// The reference trains at C = 20, 64 x 64, batch 8 (EncoderConditioning/train.py:36-43): 128 tiles of 16 x 16, and a per-step
// launch pays its launch gap, the weight-image fill, staging and tail for 256 cells per workgroup.  Here a workgroup OWNS one
// 16 x 16 tile for all T steps (one workgroup per CU, every tile resident):
//   * the weight image (wp, W1/b1, W2/b2, W3) and the goal-encoding tile are staged into LDS once per launch; the tile's pending
//     state x'_t, its pre mask and its alpha' halo stay in LDS from step to step;
//   * the cells of step t + 1 depend on x'_t at halo 1 (all channels), on alpha'_t at halo 3 (post-mask of the halo feeds the next
//     pre-mask, which feeds z, which feeds the perception) and on the pre mask at halo 2.  All three are values the OWNING tile
//     produced, so one exchange per step suffices: a tile publishes its border band (x' ring: every channel; alpha': 3 deep; pre
//     mask: 2 deep) and recomputes its neighbours' life mask / resolved state on its own halo cells, exactly as the per-step kernels
//     recompute them from memory;
//   * the exchange is the DyNCA kernel's protocol (nca_dynca_persist.hip): 8-byte single-copy (value, tag) pairs, tag = epoch *
//     4096 + step, written and read as relaxed agent-scope atomics, two parities; a reader needs no counter, a writer no
//     acknowledgement.  A tile can only overwrite parity p after its neighbours published the step after the one they read from it;
//   * per-cell arithmetic is the producer/consumer family's (nca_cond_pc.hip / nca_cond_tile.h): the same life-mask / clamp
//     sequence, the same perceive_tile_pipe and mlp_tile_regs (exact-f32 MFMA chains in the same k order) on the same 4 x 16 wave
//     tiles -- the result equals ncahip_cond_grow_fwd_f32 bit for bit, history slots included.
//   * every poll is BOUNDED (kPollSeconds of device wall clock: long enough for a workgroup that only gets its CU when a co-tenant
//     kernel ends).  On expiry bit 1 of the sticky error word and the abort word are set; every workgroup leaves its step loop and
//     writes NaN over its tile of x_final, so a drained launch never looks like a valid state.
#include "nca_cond_tile.h"

namespace {

constexpr int kPT = 256;                  // 4 waves; wave w computes rows 4w .. 4w+3 of the tile
constexpr int PT = 16;                    // tile side
constexpr int kPollSeconds = 2;           // bound of one neighbour poll
// LDS planes: rows r = -3 .. 18 at index r + 3 (22 rows), image column tx0 + c at index c + 4 (RS = 24: max3x3's stride)
constexpr int PLR = 22, PLS = PLR * RS;   // 528 floats
constexpr int ZR = PT + 2, ZCS = ZR * RS; // z / x' tile with halo 1: rows -1 .. 16 at index r + 1; 432 floats per channel
static_assert(ZCS % 32 == 16, "bank layout (as CS)");
constexpr int XRC = 260;                  // resolved state: [channel][16 x 16], channel stride 260 ((4 * 260) % 32 == 16, as XRS)
constexpr int kBand = 156;                // cells of a tile within 2 of its border (the band its neighbours read)
constexpr int kExtra = 228 + 144;         // alpha' halo rings 1..3 + pre halo rings 1..2

template <int CP>
struct PCfgP {
    using F = WCfg<CP>;
    static constexpr int XR_ROWS = CP > 16 ? CP : 16 * F::M3T;   // mlp_tile_regs: 16 * M3T rows when CP <= 16 (rows >= CP: scratch)
    static constexpr int OFF_XZ = F::SHARED;                     // x'_t (halo 1) -> z_t in place
    static constexpr int OFF_G = OFF_XZ + CP * ZCS;              // goal encoding (halo 1), staged once
    static constexpr int OFF_AL = OFF_G + CP * ZCS;              // alpha'_t, halo 3
    static constexpr int OFF_PR = OFF_AL + PLS;                  // pre mask of x'_t (0 / 1), halo 2
    static constexpr int OFF_LF = OFF_PR + PLS;                  // life mask, halo 2
    static constexpr int OFF_A2 = OFF_LF + PLS;                  // resolved alpha, halo 2
    static constexpr int OFF_PN = OFF_A2 + PLS;                  // pre-life mask of this step, halo 1
    static constexpr int OFF_XR = OFF_PN + PLS;                  // resolved state -> x'_{t+1} in place
    static constexpr int OFF_MK = OFF_XR + XR_ROWS * XRC;        // fire mask [16 x 16]
    static constexpr int OFF_FLAG = OFF_MK + PT * PT;
    static constexpr int LDS_FLOATS = OFF_FLAG + 4;
    static constexpr int NI = (CP * 68 + kExtra + kPT - 1) / kPT;   // halo items per thread and step
    static_assert(OFF_XZ % 4 == 0 && OFF_XR % 4 == 0 && OFF_MK % 4 == 0, "16-byte carve");
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
};

__device__ __forceinline__ void st_pair(unsigned long long* p, float v, unsigned tag) {
    __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_pair(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// band cell (r, q) of a tile (min distance to its border <= 2) <-> index 0 .. 155: rows 0-2, rows 13-15, columns 0-2 / 13-15 of rows 3-12
__device__ __forceinline__ int band_index(int r, int q) {
    if (r < 3) return r * PT + q;
    if (r > 12) return 48 + (r - 13) * PT + q;
    return 96 + (r - 3) * 6 + (q < 3 ? q : q - 10);
}
__device__ __forceinline__ void band_cell(int i, int& r, int& q) {
    if (i < 48) { r = i / PT; q = i % PT; }
    else if (i < 96) { r = 13 + (i - 48) / PT; q = (i - 48) % PT; }
    else { const int k = i - 96; r = 3 + k / 6; q = k % 6; q = q < 3 ? q : q + 10; }
}
// cell i of the ring at distance h around the tile (h = 1 .. 3: halo rings; h = 0, -1, -2: the tile's own cells 0, 1, 2 from its
// border): top row, bottom row, left column, right column
__device__ __forceinline__ void ring_cell(int h, int i, int& r, int& q) {
    const int side = PT + 2 * h;
    if (i < side) { r = -h; q = i - h; }
    else if (i < 2 * side) { r = PT - 1 + h; q = i - side - h; }
    else if (i < 2 * side + side - 2) { r = i - 2 * side - h + 1; q = -h; }
    else { r = i - 3 * side + 2 - h + 1; q = PT - 1 + h; }
}

#if defined(NCA_STAMPS)
// diagnostic build only: wall-clock time spent in phase i, summed over the steps, per workgroup -> a.dbg[blockIdx.x * 8 + i]
#define NCA_PSTAMP(i)                                                                                  \
    do {                                                                                               \
        const uint64_t now_ = wall_clock64();                                                          \
        if (a.dbg && tid == 0) ph_[i] += now_ - t_ph_;                                                 \
        t_ph_ = now_;                                                                                  \
    } while (0)
#else
#define NCA_PSTAMP(i) do { } while (0)
#endif

template <int CP>
__global__ __launch_bounds__(kPT, 1) void cond_persist_kernel(const NcaCondPersistArgs a) {
    using K = WCfg<CP>;
    using PK = PCfgP<CP>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const XZ = smem + PK::OFF_XZ;
    float* const G = smem + PK::OFF_G;
    float* const AL = smem + PK::OFF_AL;
    float* const PR = smem + PK::OFF_PR;
    float* const LF = smem + PK::OFF_LF;
    float* const A2 = smem + PK::OFF_A2;
    float* const PN = smem + PK::OFF_PN;
    float* const XR = smem + PK::OFF_XR;
    float* const MK = smem + PK::OFF_MK;
    int* const lflag = reinterpret_cast<int*>(smem + PK::OFF_FLAG);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = a.C, H = a.H, W = a.W, hid = 64, K1 = 3 * C, alive = a.alive_ch, gch0 = C - a.goal_ch;
    const bool use_alive = alive >= 0, has_goal = a.goal_ch > 0;
    const size_t plane = (size_t)H * W;
    const unsigned tag0 = a.epoch << 12;
    const int tiles_x = W / PT, tiles_y = H / PT;
    const int tile = blockIdx.x, txi = tile % tiles_x, tyi = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
    const int ty0 = tyi * PT, tx0 = txi * PT;
    const size_t cell0 = (size_t)b * plane;
    auto in_img = [&](int r, int q) { return ty0 + r >= 0 && ty0 + r < H && tx0 + q >= 0 && tx0 + q < W; };
    auto pl = [](int r, int q) { return (r + 3) * RS + q + 4; };          // offset in a 22-row plane
    auto zo = [](int r, int q) { return (r + 1) * RS + q + 4; };          // offset in a z / x' channel

    // ---- once per launch: A-operand images (the producer/consumer kernel's layouts and k order), goal tile, x'_0 -------------
    {
        FillRegs<4 * K::K1S4 * 256, kPT> f1;
        FillRegs<4 * 16 * 64, kPT> f2;
        FillRegs<K::M3T * 16 * 64, kPT> f3;
        FillRegs<K::HID, kPT> fb1, fb2;
        FillRegs<CP * K::WPS, kPT> fwp;
        fill_load(f1, a.w1, tid, [&](int idx) -> long {
            const int j = idx & 3, l = (idx >> 2) & 63, q = (idx >> 8) % K::K1S4, m = (idx >> 8) / K::K1S4;
            const int s = 4 * q + j, gg = l >> 4, o = 16 * m + (l & 15);
            const int ch = 4 * (s / 3) + gg, f = s % 3;
            return (s < K::K1S && ch < C && o < hid) ? (long)o * K1 + 3 * ch + f : -1;
        });
        fill_load(f2, a.w2, tid, [&](int idx) -> long {
            const int r = idx & 3, l = (idx >> 2) & 63, m = (idx >> 8) & 3, m2 = idx >> 10;
            const int gg = l >> 4, o = 16 * m2 + (l & 15), k = 16 * m + 4 * gg + r;
            return (o < hid && k < hid) ? (long)o * hid + k : -1;
        });
        fill_load(f3, a.w3, tid, [&](int idx) -> long {
            const int r = idx & 3, l = (idx >> 2) & 63, m = (idx >> 8) & 3, m3 = idx >> 10;
            const int gg = l >> 4, o = 16 * m3 + (l & 15), k = 16 * m + 4 * gg + r;
            return (o < C && k < hid) ? (long)o * hid + k : -1;
        });
        fill_load(fb1, a.b1, tid, [&](int idx) -> long { return idx < hid ? idx : -1; });
        fill_load(fb2, a.b2, tid, [&](int idx) -> long { return idx < hid ? idx : -1; });
        fill_load(fwp, a.wp, tid, [&](int idx) -> long {
            const int ch = idx / K::WPS, j = idx % K::WPS;
            return (ch < C && j < 27) ? (long)ch * 27 + j : -1;
        });
        fill_store(f1, smem + K::OFF_W1, tid);
        fill_store(f2, smem + K::OFF_W2, tid);
        fill_store(f3, smem + K::OFF_W3, tid);
        fill_store(fb1, smem + K::OFF_B1, tid);
        fill_store(fb2, smem + K::OFF_B2, tid);
        fill_store(fwp, smem + K::OFF_WP, tid);
    }
    {
        const float* const xb = a.x0 + (size_t)b * C * plane;
        for (int i = tid; i < CP * ZR * ZR; i += kPT) {
            const int ch = i / (ZR * ZR), c = i % (ZR * ZR), r = c / ZR - 1, q = c % ZR - 1;
            const bool in = ch < C && in_img(r, q);
            XZ[ch * ZCS + zo(r, q)] = in ? xb[(size_t)ch * plane + (size_t)(ty0 + r) * W + tx0 + q] : 0.0f;
            if (ch < a.goal_ch)
                G[ch * ZCS + zo(r, q)] = in_img(r, q) ? a.goal[((size_t)b * a.goal_ch + ch) * plane + (size_t)(ty0 + r) * W + tx0 + q] : 0.0f;
        }
        // alpha' with halo 3; -inf outside the image (max_pool2d padding) -- those cells are never overwritten
        for (int i = tid; i < PLR * PLR; i += kPT) {
            const int r = i / PLR - 3, q = i % PLR - 3;
            AL[pl(r, q)] = (use_alive && in_img(r, q)) ? xb[(size_t)alive * plane + (size_t)(ty0 + r) * W + tx0 + q] : NCA_NEG_INF;
            PR[pl(r, q)] = 0.0f;
        }
        if (tid < 4) lflag[tid] = 0;
    }
    // halo items of this thread (steps >= 1): item j = tid + 256 k -- j < C*68: channel j / 68 of halo-1 cell j % 68 -> x' tile;
    // then alpha' on the rings at distance 1..3 -> AL; then the pre mask on the rings at distance 1..2 -> PR.  src = the pair's
    // index within one parity (-1: no item / outside the image), dst = LDS offset
    int src[PK::NI], dst[PK::NI];
#pragma unroll
    for (int k = 0; k < PK::NI; ++k) {
        const int j = tid + kPT * k;
        int r = 0, q = 0, slot = -1, d = -1;
        if (j < C * 68) {
            slot = j / 68;
            ring_cell(1, j % 68, r, q);
            d = PK::OFF_XZ + slot * ZCS + zo(r, q);
        } else if (use_alive && j < C * 68 + kExtra) {
            int e = j - C * 68;
            if (e < 228) {
                const int h = e < 68 ? 1 : e < 144 ? 2 : 3;
                ring_cell(h, e - (h == 1 ? 0 : h == 2 ? 68 : 144), r, q);
                slot = alive;
                d = PK::OFF_AL + pl(r, q);
            } else {
                e -= 228;
                const int h = e < 68 ? 1 : 2;
                ring_cell(h, e - (h == 1 ? 0 : 68), r, q);
                slot = C;
                d = PK::OFF_PR + pl(r, q);
            }
        }
        src[k] = -1;
        dst[k] = d;
        if (slot >= 0 && in_img(r, q)) {
            const int gy = ty0 + r, gx = tx0 + q;
            const int owner = (b * tiles_y + gy / PT) * tiles_x + gx / PT;
            src[k] = (owner * (C + 1) + slot) * kBand + band_index(gy % PT, gx % PT);
        }
    }
    // own band cells this thread publishes every step: j < C*60: channel j / 60 of border-ring cell j % 60 (from XR); then alpha'
    // on the rings 1..2 deep (XR); then the pre mask on the rings 0..1 deep (PR).  pidx = pair offset within the tile's block
    constexpr int NPUB = (CP * 60 + 208 + kPT - 1) / kPT;
    int pidx[NPUB], psrc[NPUB];
#pragma unroll
    for (int k = 0; k < NPUB; ++k) {
        const int j = tid + kPT * k;
        int r = 0, q = 0, slot = -1, o = 0;
        if (j < C * 60) {
            slot = j / 60;
            ring_cell(0, j % 60, r, q);
            o = PK::OFF_XR + slot * XRC + r * PT + q;
        } else if (use_alive && j < C * 60 + 208) {
            const int e = j - C * 60;
            if (e < 96) {
                ring_cell(e < 52 ? -1 : -2, e < 52 ? e : e - 52, r, q);
                slot = alive;
                o = PK::OFF_XR + slot * XRC + r * PT + q;
            } else {
                const int e2 = e - 96;
                ring_cell(e2 < 60 ? 0 : -1, e2 < 60 ? e2 : e2 - 60, r, q);
                slot = C;
                o = PK::OFF_PR + pl(r, q);
            }
        }
        pidx[k] = slot >= 0 ? slot * kBand + band_index(r, q) : -1;
        psrc[k] = o;
    }
    __syncthreads();

    MlpRegs<CP> Wr;
    mlp_load_regs<CP>(smem, lane, Wr);
    int* const abort_w = a.abort_w;
    const size_t slot_f = (size_t)a.B * C * plane, pslot = (size_t)a.B * plane;
    const size_t cells = (size_t)a.B * plane;
    bool stop = false;
#if defined(NCA_STAMPS)
    uint64_t ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_ph_ = wall_clock64();
#endif

    for (int t = 0;; ++t) {
        const bool pending = t > 0;
        if (t > 0) {
            // ---- S0: the neighbours' band of state t (bounded poll; every pair must carry tag epoch * 4096 + t) ----------------
            const unsigned long long* const xs = a.xch + (size_t)(t & 1) * a.xch_words;
            const unsigned want = tag0 + (unsigned)t;
            float hv[PK::NI];
            bool ok = true;
            const uint64_t t_start = wall_clock64();
            for (int spins = 0;; ++spins) {
                bool stale = false;
#pragma unroll
                for (int k = 0; k < PK::NI; ++k) {
                    unsigned long long w = (unsigned long long)want << 32;
                    if (src[k] >= 0) w = ld_pair(xs + src[k]);
                    hv[k] = __uint_as_float((unsigned)w);
                    stale = stale || (unsigned)(w >> 32) != want;
                }
                if (!__any(stale)) break;
                if ((spins & 31) == 31) {
                    const bool expired = wall_clock64() - t_start > a.poll_ticks;
                    const bool aborted = (unsigned)__hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.epoch;
                    if (expired || aborted) {
                        if (expired && lane == 0) {   // a neighbour never delivered (not resident?): record it, tell every workgroup
                            if (a.err) __hip_atomic_fetch_or(a.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            __hip_atomic_store(abort_w, (int)a.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        ok = false;
                        break;
                    }
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (ok) {
#pragma unroll
                for (int k = 0; k < PK::NI; ++k)
                    if (src[k] >= 0) smem[dst[k]] = hv[k];
            } else if (lane == 0) {
                __hip_atomic_store(lflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();
            stop = __hip_atomic_load(lflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
            if (stop) break;
        }
        NCA_PSTAMP(0);
        if (t == a.T) break;

        // ---- S1: life = pre & post of the previous step, resolved alpha, halo 2 (nca.py:191-194; stage_tile S2) ---------------
        for (int i = tid; i < 20 * 20; i += kPT) {
            const int r = i / 20 - 2, q = i % 20 - 2;
            const int o = pl(r, q);
            float life = 0.0f, av = NCA_NEG_INF;
            if (in_img(r, q)) {
                life = 1.0f;
                if (use_alive) {
                    av = AL[o];
                    if (pending) {
                        life = (PR[o] != 0.0f && max3x3(AL + o) > a.thr) ? 1.0f : 0.0f;
                        av = wclamp(av * life, a.lo, a.hi);
                    }
                }
            }
            LF[o] = life;
            A2[o] = av;
        }
        __syncthreads();
        NCA_PSTAMP(1);
        // ---- S2: pre-life mask of this step on halo 1 (history: pre slot t + 1); fire mask of the tile ------------------------
        for (int i = tid; i < ZR * ZR; i += kPT) {
            const int r = i / ZR - 1, q = i % ZR - 1;
            float pn = 0.0f;
            if (in_img(r, q)) pn = (!use_alive || max3x3(A2 + pl(r, q)) > a.thr) ? 1.0f : 0.0f;
            PN[pl(r, q)] = pn;
        }
        {
            const int r = tid >> 4, q = tid & 15;
            const unsigned pix = (unsigned)((ty0 + r) * W + tx0 + q);
            float uf;
            if (a.u_bits) {
                const uint32_t wd = reinterpret_cast<const uint32_t*>(a.u)[(size_t)t * ((cells + 31) / 32) + ((cell0 + pix) >> 5)];
                uf = ((wd >> (unsigned)((cell0 + pix) & 31)) & 1u) ? 0.0f : 2.0f;
            } else {
                uf = nca_philox_cell(a.seed, a.step0 + (uint64_t)t, cell0 + pix);
            }
            MK[tid] = wclamp(uf, 0.0f, 1.0f) < a.fire_rate ? 1.0f : 0.0f;   // nca.py:171-174
        }
        __syncthreads();
        {
            const int r = tid >> 4, q = tid & 15;
            const float pn = PN[pl(r, q)];
            PR[pl(r, q)] = pn;                                    // the pre mask of x'_{t+1}
            if (a.hist) a.pre[(size_t)(t + 1) * pslot + cell0 + (size_t)(ty0 + r) * W + tx0 + q] = (uint8_t)pn;
        }
        // ---- S3: z = x + goal * pre on halo 1 (nca.py:177), in place over x'; resolved state of the tile -> XR ------------------
        //      (stage_tile's arithmetic per element: 4-cell groups of columns 0..15, then the halo columns -1 and 16)
        for (int i = tid; i < CP * ZR * 4; i += kPT) {
            const int ch = i / (ZR * 4), c = i % (ZR * 4), r = c / 4 - 1, q = 4 * (c % 4);
            f32x4* const p = reinterpret_cast<f32x4*>(XZ + ch * ZCS + zo(r, q));
            f32x4 v = *p;
            if (pending) {
                v = v * ld4(LF + pl(r, q));
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = wclamp(v[j], a.lo, a.hi);
            }
            const bool in = ty0 + r >= 0 && ty0 + r < H;
            if (!in || ch >= C) v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r >= 0 && r < PT) st4(XR + ch * XRC + r * PT + q, v);
            if (has_goal && ch >= gch0 && ch < C && in)
                v = __builtin_elementwise_fma(ld4(G + (ch - gch0) * ZCS + zo(r, q)), ld4(PN + pl(r, q)), v);
            *p = v;
        }
        for (int i = tid; i < CP * ZR * 2; i += kPT) {
            const int ch = i / (ZR * 2), c = i % (ZR * 2), r = c / 2 - 1, q = (c & 1) ? PT : -1;
            float* const p = XZ + ch * ZCS + zo(r, q);
            float v = *p;
            if (pending) v = wclamp(v * LF[pl(r, q)], a.lo, a.hi);
            if (!in_img(r, q) || ch >= C) v = 0.0f;
            else if (has_goal && ch >= gch0) v = fmaf(G[(ch - gch0) * ZCS + zo(r, q)], PN[pl(r, q)], v);
            *p = v;
        }
        __syncthreads();
        NCA_PSTAMP(2);
        // ---- S4: perception + UpdateNet + residual on the wave's 4 x 16 rows (the producer/consumer consumer's code) ------------
#pragma unroll 1
        for (int pass = 0; pass < WTH / 2; ++pass) {
            float P[2][K::K1S];
            perceive_tile_pipe<CP, 2, ZCS>(smem, XZ + 4 * wave * RS, lane, pass * 2, P);
            mlp_tile_regs<CP, 2, XRC>(Wr, smem, XR + 4 * wave * WTW, MK + 4 * wave * WTW, lane, pass * 2, P);
        }
        __syncthreads();
        NCA_PSTAMP(3);
        // ---- S5: x'_{t+1} -> the LDS tile (and the history slot); the border band -> the neighbours ------------------------------
        {
            const int r = tid >> 4, q = tid & 15;
            const size_t go = cell0 * C + (size_t)(ty0 + r) * W + tx0 + q;
            for (int ch = 0; ch < CP; ++ch) {
                const float v = XR[ch * XRC + tid];
                XZ[ch * ZCS + zo(r, q)] = v;
                if (ch < C && a.hist) a.states[(size_t)(t + 1) * slot_f + go + (size_t)ch * plane] = v;
            }
            if (use_alive) AL[pl(r, q)] = XR[alive * XRC + tid];
        }
        {
            unsigned long long* const xd = a.xch + (size_t)((t + 1) & 1) * a.xch_words + (size_t)tile * (C + 1) * kBand;
            const unsigned tag = tag0 + (unsigned)(t + 1);
#pragma unroll
            for (int k = 0; k < NPUB; ++k)
                if (pidx[k] >= 0) st_pair(xd + pidx[k], smem[psrc[k]], tag);
        }
        // (the next iteration's S0 barrier orders these LDS writes before anything reads them)
        NCA_PSTAMP(4);
    }

    // ---- finalize (nca.py:207-208; cond_finalize_kernel) on the tile's cells, or NaN when the launch was abandoned ---------------
    if (!stop) stop = (unsigned)__hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.epoch;
    {
        const int r = tid >> 4, q = tid & 15;
        float life = 1.0f;
        if (use_alive) life = (PR[pl(r, q)] != 0.0f && max3x3(AL + pl(r, q)) > a.thr) ? 1.0f : 0.0f;
        float* const ob = a.x_final + cell0 * C + (size_t)(ty0 + r) * W + tx0 + q;
        for (int ch = 0; ch < C; ++ch)
            ob[(size_t)ch * plane] = stop ? __builtin_nanf("") : fminf(fmaxf(XZ[ch * ZCS + zo(r, q)] * life, a.lo), a.hi);
    }
#if defined(NCA_STAMPS)
    NCA_PSTAMP(5);
    if (a.dbg && tid == 0)
        for (int i = 0; i < 8; ++i) a.dbg[(size_t)blockIdx.x * 8 + i] = ph_[i];
#endif
}

template <int CP>
hipError_t launch_cond_persist(const NcaCondPersistArgs& a, hipStream_t st, bool query_only, bool* fits) {
    using PK = PCfgP<CP>;
    auto kern = cond_persist_kernel<CP>;
    // more than half a CU's LDS: ONE workgroup per CU
    const size_t lds = (size_t)PK::LDS_FLOATS * sizeof(float) > 81 * 1024 ? (size_t)PK::LDS_FLOATS * sizeof(float) : (size_t)81 * 1024;
    static NcaLdsAttr attr;
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(kern), lds); e != hipSuccess) return e;
    const int ntiles = a.B * (a.H / PT) * (a.W / PT);
    static std::atomic<int> occ[kNcaMaxDevices];
    int per_cu = occ[nca_device_index()].load(std::memory_order_relaxed);
    if (per_cu == 0) {
        if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), kPT, lds); e != hipSuccess) return e;
        occ[nca_device_index()].store(per_cu > 0 ? per_cu : -1, std::memory_order_relaxed);
    }
    // one tile per CU (not occupancy x CUs: two tiles on one CU would share its matrix pipes while another CU idles)
    *fits = per_cu >= 1 && ntiles <= nca_cu_count();
    if (!*fits || query_only) return hipSuccess;
    NcaCondPersistArgs k = a;
    if (k.poll_ticks == 0) {
        static std::atomic<long long> rate_khz[kNcaMaxDevices];
        long long r = rate_khz[nca_device_index()].load(std::memory_order_relaxed);
        if (r == 0) {
            int q = 0;
            r = (hipDeviceGetAttribute(&q, hipDeviceAttributeWallClockRate, nca_device_index()) == hipSuccess && q > 0) ? q : 100000;
            rate_khz[nca_device_index()].store(r, std::memory_order_relaxed);
        }
        k.poll_ticks = (uint64_t)r * 1000u * kPollSeconds;
    }
    hipLaunchKernelGGL(kern, dim3(ntiles), dim3(kPT), lds, st, k);
    return hipGetLastError();
}

}  // namespace

static unsigned long long* g_stamp_persist = nullptr;   // diagnostic builds: phase sums (tools/stamp_persist.py)
extern "C" void nca_debug_set_stamp_buffer_persist(void* p) { g_stamp_persist = (unsigned long long*)p; }

bool nca_cond_persist_shape_ok(int B, int C, int H, int W, int hidden, int goal_ch) {
    return B >= 1 && C >= 1 && C <= 20 && hidden == 64 && goal_ch >= 0 && goal_ch <= C && H % PT == 0 && W % PT == 0 &&
           (long)B * (H / PT) * (W / PT) <= 4096 && (size_t)C * H * W < ((size_t)1 << 31) && (size_t)B * H * W < ((size_t)1 << 31);
}
int nca_cond_persist_tiles(int B, int H, int W) { return B * (H / PT) * (W / PT); }
size_t nca_cond_persist_xch_pairs(int B, int C, int H, int W) { return (size_t)nca_cond_persist_tiles(B, H, W) * (C + 1) * kBand; }

hipError_t nca_launch_cond_persist(const NcaCondPersistArgs& a_in, hipStream_t st, bool query_only, bool* fits) {
    NcaCondPersistArgs a = a_in;
    a.err = nca_error_word_device();
#if defined(NCA_STAMPS)
    a.dbg = g_stamp_persist;
#endif
    if (a.C <= 12) return launch_cond_persist<12>(a, st, query_only, fits);
    if (a.C <= 16) return launch_cond_persist<16>(a, st, query_only, fits);
    if (a.C <= 20) return launch_cond_persist<20>(a, st, query_only, fits);
    return hipErrorInvalidValue;
}

// nca_cond_pc.hip -- ConditionedNCA fused step, producer/consumer wave specialisation (gfx950, fp32 exact).
//
// Same math, MFMA mapping and tile staging code as nca_cond_wave.hip, different division of labour.  The
// exact-f32 MFMA runs at the vector rate and does not co-execute with VALU work of its own wave, and the mask
// resolution in front of it is a chain of dependent LDS round trips: a wave that does both leaves the matrix
// pipe idle half the time even with a second such wave on the SIMD.  Here each SIMD hosts ONE consumer wave
// (perception -> MFMA chain -> 16-byte stores; nothing else) and ONE producer wave (global loads, pending
// life-mask resolution, z tile, resolved-state copy, fire mask) that works one tile ahead through a
// double-buffered LDS tile; the two hand tiles over through round counters in LDS (no workgroup barrier in the loop).
//   workgroup = 8 waves = 4 pairs; pair p owns the 4x16 tiles at rows 4p..4p+3 of each 16x16 super-tile.
#include "nca_cond_tile.h"

namespace {

#ifndef NCA_WT_STORE
#define NCA_WT_STORE 1
#endif
constexpr bool kNtStore = NCA_WT_STORE != 0;   // write-through output stores (see store_tile)

// LDS carve of the pairs.  Offsets are floats from the start of the allocation; `which` is the tile buffer (0/1).
//   CP <= 16: [weight image F::SHARED][pair 0: buf0 buf1 scratch][pair 1] ...  with XR of 16*M3T rows (whole MFMA row tiles).
//   CP  > 16 (the reference's default C = 20): the straightforward carve is 217 KB.  Two things bring it to 159 KB:
//     * XR holds exactly CP rows (mlp_tile_regs guards the rows of the last output tile), and
//     * the W1 / W2 images are dead once the consumers have moved them into registers (mlp_load_regs), so the SECOND tile buffers
//       of pairs 0 and 1 live on top of them; the producers wait at one more workgroup barrier before they stage into a second
//       buffer for the first time.  W3, the biases and the perception taps stay resident (W3 is read from LDS per pass here: 160
//       operand registers would not fit beside the rest of the consumer).
template <int CP>
struct PCfg {
    using F = WCfg<CP>;
    static constexpr bool WIDE = CP > 16;
    static constexpr int XR_ROWS = WIDE ? CP : 16 * F::M3T;
    static constexpr int SZ_Z = CP * CS, SZ_XR = XR_ROWS * XRS, SZ_MK = WTH * WTW;
    static constexpr int BUF = SZ_Z + SZ_XR + SZ_MK;               // one tile buffer (floats)
    static constexpr int SCR_A3 = 0;                               // producer scratch of a pair, not double-buffered
    static constexpr int SCR_LIFE = SCR_A3 + (WTH + 6) * RS;
    static constexpr int SCR_A2 = SCR_LIFE + (WTH + 4) * RS;
    static constexpr int SCR_FLAG = SCR_A2 + (WTH + 4) * RS;       // [0] last round staged, [1] last round consumed (ints)
    static constexpr int SCR = SCR_FLAG + 4;
    static constexpr int PAIR = 2 * BUF + SCR;                     // narrow carve: one contiguous region per pair
    // wide carve
    static constexpr int ALIAS_END = F::OFF_W3;                    // [0, OFF_W3) = the W1 and W2 images
    static constexpr int W_BUF0 = F::SHARED;                       // 4 x buf0
    static constexpr int W_SCR = W_BUF0 + 4 * BUF;                 // 4 x scratch
    static constexpr int W_XR1P1 = W_SCR + 4 * SCR;                // XR of pair 1's second buffer (its Z and MK sit in the alias region)
    static constexpr int W_BUF1 = W_XR1P1 + SZ_XR;                 // second buffers of pairs 2 and 3
    static constexpr int LDS_FLOATS = WIDE ? W_BUF1 + 2 * BUF : F::SHARED + 4 * PAIR;
    static_assert(!WIDE || BUF + SZ_Z + SZ_MK <= ALIAS_END, "pair 0's second buffer + pair 1's second Z / MK fit on the dead images");
    static_assert(BUF % 4 == 0 && SCR % 4 == 0 && SZ_Z % 4 == 0 && SZ_XR % 4 == 0 && F::SHARED % 4 == 0, "16-byte carve");
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
    struct Offs { int z, xr, mk, scr; };
    static __device__ __forceinline__ Offs offs(int pair, int which) {
        if constexpr (!WIDE) {
            const int b = F::SHARED + pair * PAIR + which * BUF;
            return Offs{b, b + SZ_Z, b + SZ_Z + SZ_XR, F::SHARED + pair * PAIR + 2 * BUF};
        } else {
            const int scr = W_SCR + pair * SCR;
            if (which == 0) {
                const int b = W_BUF0 + pair * BUF;
                return Offs{b, b + SZ_Z, b + SZ_Z + SZ_XR, scr};
            }
            if (pair == 0) return Offs{0, SZ_Z, SZ_Z + SZ_XR, scr};
            if (pair == 1) return Offs{BUF, W_XR1P1, BUF + SZ_Z, scr};
            const int b = W_BUF1 + (pair - 2) * BUF;
            return Offs{b, b + SZ_Z, b + SZ_Z + SZ_XR, scr};
        }
    }
};

// FC: the producer compacts the tile's firing cells into a list (stage_tile FCL) and the consumer runs perception and UpdateNet
// on those cells only, in groups of 16 MFMA columns (two groups per pass, one for an odd last group).  x' = x + fire * out
// (nca.py:189): a cell that does not fire keeps its resolved state, which XR already holds -- store_tile is unchanged.
// CARRY (narrow carve): a tile's last, partial group is not padded to 16 columns.  Its cells get their perception and are
// parked in the consumer's carry (FireCarry, on the dead W1 / W2 images); UpdateNet runs when 16 parked cells have come
// together, whichever tiles of the pair they came from, and once more, padded, after the pair's last round.  Only the consumer
// wave changes: hand-off, round counters, tile buffers and the producer are those of the kernel without the carry.
// FW (with FC): the producer takes each tile's fire mask from a.fire_words, drawn before the launch (issue_loads / stage_tile FW),
// instead of drawing it; the lists it writes are the same, and nothing else changes.
// MS (with FC, CARRY and FW): the launch runs a.ms_steps steps of a grow (NcaCondArgs, nca_kernels.h).  Every step walks the same
// tiles, so a workgroup owns the same super-tiles and a pair the same tiles throughout; roles, hand-off counters, tile buffers,
// lists and carry are those of the one-step kernel, and the round numbers keep counting across the steps, so a pair's pipeline runs
// from the last tile of step t straight into the first tile of step t + 1.  What a tile of step t + 1 reads -- alpha' at halo 3,
// the pre mask at halo 2, the state at halo 1 -- lies in its 3 x 3 neighbourhood of 4 x 16 tiles, so instead of a grid-wide wait
// there is one counter per tile, a.ms_done = steps of the grow completed for it:
//   * the consumer publishes a tile (counter = t + 1, one lane, agent scope) once every store to it has completed: its store_tile,
//     the store_carry of each of its cells that was parked, and the producer's pre mask bytes (complete before the hand-off);
//   * the producer waits, before it issues a tile's loads for step t, until the nine counters of its neighbourhood (inside the
//     image) have reached t (gate below).  With the static walk the neighbours finished about a step's rounds earlier: the gate
//     is almost never closed, and a slow pair delays only its neighbours, and only when they catch up with it.
// All state stores are write-through (kNtStore; stage_tile's pre mask bytes: AUX) and all state loads agent-coherent (AUX = sc1).
// The carry is flushed at the end of every step: no parked cell crosses a step.  Every workgroup must be resident (grid <= CUs,
// one workgroup per CU by its LDS): a workgroup that never runs lets its neighbours' polls expire -- bounded, recorded in the error
// word (bit 2) and in the abort word behind the counters, which every later gate reads first and then passes without polling.
template <int CP, bool EXACT, typename ST, bool SPLIT = false, bool FC = false, bool CARRY = false, bool FW = false, bool MS = false>
__global__ __launch_bounds__(kThreadsW, 2) void cond_step_fwd_pc_kernel(const NcaCondArgs a_launch) {
    static_assert(!SPLIT || ST::BYTES == 4, "bf16x3 emulation is an option of the fp32-storage kernel");
    static_assert(!FC || (ST::BYTES == 4 && !SPLIT), "firing-cell lists: the exact-f32 fp32-storage consumer");
    static_assert(!CARRY || (FC && CP <= 16), "the carry: firing-cell lists on the narrow carve");
    static_assert(!FW || FC, "fire words: the kernels with firing-cell lists");
    static_assert(!MS || (CARRY && FW && kNtStore), "several steps per launch: the narrow-carve fire-word kernels, write-through stores");
    constexpr int AUX = MS ? 16 : kAuxCoherent;   // cache policy of the state-type accesses (issue_loads)
    // MS: `a` is the view of the step a wave is working on -- its pointers are formed where a tile needs them (view_in / view_out below)
    // from two scalars of the wave and the launch's arguments; otherwise the launch's arguments themselves
    [[maybe_unused]] NcaCondArgs a_step;
    if constexpr (MS) a_step = a_launch;
    const NcaCondArgs& a = MS ? a_step : a_launch;
    constexpr bool BF = ST::BYTES == 2;   // bf16 storage: UpdateNet on bf16 MFMA (operands rounded from the same LDS image)
    using K = WCfg<CP>;
    using PK = PCfg<CP>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = EXACT ? CP : a.C, H = a.H, W = a.W, hid = EXACT ? 64 : a.hidden, K1 = 3 * C;
    const bool producer = wave >= 4;
    const int pair = wave & 3;
    NCA_KSTAMP(0);

    // 16-byte A-operand images (same layouts as nca_cond_wave.hip), built by the four consumer waves while the
    // producers already stage the first tile
    if (!producer) {
        // all loads of all images in flight together, then the LDS writes (one cold round trip instead of eight)
        FillRegs<4 * K::K1S4 * 256, 256> f1;
        FillRegs<4 * 16 * 64, 256> f2;
        FillRegs<K::M3T * 16 * 64, 256> f3;
        FillRegs<K::HID, 256> fb1, fb2;
        FillRegs<CP * K::WPS, 256> fwp;
        {
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
        }
        fill_load(fb1, a.b1, tid, [&](int idx) -> long { return idx < hid ? idx : -1; });
        fill_load(fb2, a.b2, tid, [&](int idx) -> long { return idx < hid ? idx : -1; });
        fill_load(fwp, a.wp, tid, [&](int idx) -> long {
            const int ch = idx / K::WPS, j = idx % K::WPS;
            return (ch < C && j < 27) ? (long)ch * 27 + j : -1;
        });
        {
            fill_store(f1, smem + K::OFF_W1, tid);
            fill_store(f2, smem + K::OFF_W2, tid);
            fill_store(f3, smem + K::OFF_W3, tid);
        }
        fill_store(fb1, smem + K::OFF_B1, tid);
        fill_store(fb2, smem + K::OFF_B2, tid);
        fill_store(fwp, smem + K::OFF_WP, tid);
    }

    auto lds_of = [&](int which) -> TileLds {
        const typename PK::Offs o = PK::offs(pair, which);
        float* const S = smem + o.scr;
        return TileLds{smem + o.z, smem + o.xr, S + PK::SCR_A3, S + PK::SCR_A3, S + PK::SCR_LIFE, S + PK::SCR_A2, smem + o.mk,
                       reinterpret_cast<int*>(S + PK::SCR_FLAG) + 2 + which};
    };

    // every pair walks the same super-tile sequence
    constexpr int PSTH = 16, PSTW = 16;
    const int st_x = (W + PSTW - 1) / PSTW, st_y = (H + PSTH - 1) / PSTH;
    const int halo = a.alive_ch >= 0 ? 3 : 1;
    NcaTileWalk tw = nca_tile_walk(a.B * st_x * st_y);
    // Round k of the XCD's chunk hands tile base + k*nloc + ((local + k) mod nloc) to this workgroup: the nloc workgroups
    // of an XCD still sweep nloc consecutive super-tiles together (shared halos in its L2), but the rotation walks every
    // workgroup across the columns of the image -- with the plain stride a workgroup whose first tile sits on the left or
    // right image border gets ONLY border tiles (nloc = 32 is a multiple of the 16 super-tile columns at 256^2) and
    // finishes ~8 % after the others.
    // Coordinates advance incrementally (no integer division per tile: on this target a runtime division is a ~40-instruction
    // vector sequence, and both roles walk the tiles): t_{k+1} - t_k is nloc + 1, or 1 when the rotation wraps.
    struct Pos { int k, r, t, sx, sy, b; };   // r = (local + k) mod nloc
    const int n_rounds = (tw.end - tw.base + tw.stride - 1) / tw.stride;
    auto pos_first = [&]() -> Pos {
        Pos p{0, tw.local, tw.base + tw.local, 0, 0, 0};
        p.sx = p.t % st_x;                      // the only divisions of the launch
        const int q = p.t / st_x;
        p.sy = q % st_y;
        p.b = q / st_y;
        return p;
    };
    auto advance = [&](Pos p) -> Pos {
        ++p.k;
        int delta = tw.stride + 1;
        if (++p.r == tw.stride) { p.r = 0; delta = 1; }
        p.t += delta;
        p.sx += delta;
        while (p.sx >= st_x) {
            p.sx -= st_x;
            if (++p.sy == st_y) { p.sy = 0; ++p.b; }
        }
        return p;
    };
    auto tile_of = [&](const Pos& p) -> WTile {
        WTile w{0, 0, 0, false, false};
        if (p.k < n_rounds && p.t < tw.end) {
            w.b = p.b;
            w.ty0 = p.sy * PSTH + pair * WTH;
            w.tx0 = p.sx * PSTW;
            w.valid = w.ty0 < H && w.tx0 < W;
            w.inner = w.ty0 >= halo && w.ty0 + WTH + halo <= H && w.tx0 >= halo && w.tx0 + WTW + halo <= W;
        }
        return w;
    };
    int tile_no = 0;
    // ---- MS: the step a wave is at, the gate and the publication ---------------------------------------------------------------
    // What a wave needs only at a step boundary (the walk's first position) waits in LDS, on the dead W1 / W2 images above the four
    // carries (valid once the consumers hold the weights in registers: the second barrier).  The step itself is two 32-bit scalars
    // per wave: `step`, the step of the launch, and `ring_in`, the ring index of its input slot, (ms_t0 + step) mod ms_ring, advanced
    // by compare-and-reset at a step boundary.  The pointers of the step -- cond_grow_fwd_impl's step_args -- are formed from these two
    // and the launch's own arguments at the point of use, on the scalar ALU, and the two are opaque there: a pointer carried across
    // the tile loop is a 64-bit value the compiler parks in VGPR lanes and reads back in the middle of a tile, a kernel argument is
    // re-loaded.  The consumer's tile loop reads no LDS word for it: a round trip there is exposed time.
    constexpr int kCarrySize = [] { if constexpr (CARRY) return FireCarry<CP>::SIZE; else return 0; }();
    [[maybe_unused]] int step = 0, gbase = 0;   // MS: step of the launch, and its first round's number (rounds count on across steps)
    [[maybe_unused]] int ring_in = 0;           // MS: ring slot the step reads
    if constexpr (MS) ring_in = a_launch.ms_t0 % a_launch.ms_ring;   // the launch's only division besides the walk's
    typedef __attribute__((address_space(1))) unsigned gu32;   // a counter is a global agent-scope access, never a flat or plain one
    constexpr int kMsList = 64, kMsWave = 8, kMsPair = 2 * kMsWave;   // unpublished tiles a consumer can hold (its lanes); words per wave, per pair
    static_assert(!MS || 4 * (kCarrySize + kMsPair) <= K::OFF_W3, "carries and the MS state fit on the W1 / W2 images");
    [[maybe_unused]] int* const WS_ = reinterpret_cast<int*>(smem) + 4 * kCarrySize + pair * kMsPair + (producer ? kMsWave : 0);   // this wave's words
    enum { MS_R = 0, MS_T, MS_SX, MS_SY, MS_B, MS_END };
    static_assert(MS_END <= kMsWave, "a wave's words");
    [[maybe_unused]] auto ms_get = [&](int i) -> int { return __builtin_amdgcn_readfirstlane(WS_[i]); };
    [[maybe_unused]] gu32* const done = reinterpret_cast<gu32*>((uintptr_t)a_launch.ms_done);
    [[maybe_unused]] const int tgh = H >> 2, tgw = W >> 4;     // the counters' grid (whole 4 x 16 tiles: FW)
    // the producer's view: what the tile's loads read (x_in, pre_in -- none at the grow's step 0 --, the step's fire words) and
    // where its pre mask bytes go
    [[maybe_unused]] auto view_in = [&]() {
        int s = step, ri = ring_in;
        asm volatile("" : "+s"(s), "+s"(ri));
        const size_t pslot = (size_t)a_launch.B * a_launch.H * a_launch.W, slot = pslot * (size_t)a_launch.C * 4u;
        const int ro = ri + 1 == a_launch.ms_ring ? 0 : ri + 1;
        a_step.x_in = reinterpret_cast<const float*>(a_launch.ms_states + (size_t)ri * slot);
        a_step.pre_in = a_launch.ms_t0 + s == 0 ? nullptr : a_launch.ms_pre + (size_t)ri * pslot;
        a_step.pre_out = a_launch.ms_pre + (size_t)ro * pslot;
        a_step.fire_words = a_launch.fire_words + (size_t)s * (pslot >> 6);
        // the channel counts the loads' predicates compare with: opaque too, or every comparison is hoisted out of the tile loop as a
        // 64-bit lane mask of its own, parked in VGPR lanes with the rest
        int gc = a_launch.goal_ch, ac = a_launch.alive_ch;
        asm volatile("" : "+s"(gc), "+s"(ac));
        a_step.goal_ch = gc;
        a_step.alive_ch = ac;
    };
    // the consumer's view: where the step's state goes
    [[maybe_unused]] auto view_out = [&]() {
        int ri = ring_in;
        asm volatile("" : "+s"(ri));
        const size_t slot = (size_t)a_launch.B * a_launch.H * a_launch.W * (size_t)a_launch.C * 4u;
        const int ro = ri + 1 == a_launch.ms_ring ? 0 : ri + 1;
        a_step.x_out = reinterpret_cast<float*>(a_launch.ms_states + (size_t)ro * slot);
    };
    // the next step of the launch
    [[maybe_unused]] auto next_step = [&]() {
        ++step;
        gbase += n_rounds;
        if (++ring_in == a_launch.ms_ring) ring_in = 0;
    };
    // Producer gate of tile t for a step with `need` earlier steps in the grow: lanes 0..8 read the counters of the 3 x 3 tile
    // neighbourhood (same batch item; the tile itself included), lane 9 (and a lane whose neighbour lies outside the image) the abort
    // word.  The wait that makes this step's reads correct also makes its writes safe: the tile's output overwrites the ring slot its
    // neighbours READ one step earlier (ring == 2; a longer ring only moves that slot further away), and they have published that
    // step -- every load of it long retired -- before the tile is even staged.
    // The first look is taken BEFORE the producer waits for its tile buffer (gate_look, ahead of await(1, ...)): one round trip beyond
    // the L2 off the path between "buffer free" and "loads issued".  Within a grow the counters only grow and the abort word is sticky
    // (only the grow's first fire-word launch zeroes them, before any step launch), so a look that finds the gate open is as good
    // later; a look that finds it closed falls into the poll loop.  The tile's loads stay behind the check either way.
    constexpr int kGateSpins = 1 << 17;   // x (one L2 round trip + s_sleep 16): some 0.2 s, against waits of at most a few steps
    struct GateLook { gu32* p; bool nb; unsigned v; };
    [[maybe_unused]] auto gate_look = [&](const WTile& t) -> GateLook {
        const int dy = (lane >= 3) + (lane >= 6) - 1, dx = lane - 3 * (dy + 1) - 1;
        const int ny = (t.ty0 >> 2) + dy, nx = (t.tx0 >> 4) + dx;
        const bool nb = lane < 9 && ny >= 0 && ny < tgh && nx >= 0 && nx < tgw;
        const unsigned ntile = (unsigned)(a_launch.B * tgh * tgw);
        GateLook g{done + (nb ? (unsigned)((t.b * tgh + ny) * tgw + nx) : ntile), nb, 0u};
        if (lane < 10) g.v = __hip_atomic_load(g.p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return g;
    };
    [[maybe_unused]] auto gate = [&](const GateLook& g, int step_no) {
        const unsigned need = (unsigned)(a_launch.ms_t0 + step_no);
        const unsigned ntile = (unsigned)(a_launch.B * tgh * tgw);
        gu32* const p = g.p;
        const bool nb = g.nb;
        const bool early = __builtin_amdgcn_ballot_w64(lane < 10 && !nb && g.v != 0u) != 0ull ||   // some gate gave up: drain, no polling
                           __builtin_amdgcn_ballot_w64(nb && g.v < need) == 0ull;
        if (!early) for (int spins = 0;;) {
            unsigned v = need;
            if (lane < 10) v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_ballot_w64(lane < 10 && !nb && v != 0u) != 0ull) break;   // some gate gave up: drain, no polling
            if (__builtin_amdgcn_ballot_w64(nb && v < need) == 0ull) break;
            if (++spins >= kGateSpins) {
                // a neighbour never got there (a workgroup that is not resident): recorded like an expired hand-off (await), and
                // told to every later gate of the launch through the abort word
                if (lane == 0) {
                    if (a_launch.err) __hip_atomic_fetch_or(a_launch.err, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(done + ntile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                break;
            }
            __builtin_amdgcn_s_sleep(16);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // no instruction: keeps the tile's loads behind the poll
    };
    // (A register-carried prefetch of the NEXT tile's loads was tried here and measured slower, 97 -> 102 us f32 and
    // 60 -> 64 us bf16: border tiles force waits inside the issue sequence, and the producer is off the critical path.)
    auto produce = [&](const WTile& t, int which) {
        if (!t.valid) return;
        if constexpr (MS) view_in();
        TileRegs<CP, ST> R;
        const TileLds L = lds_of(which);
        if (t.inner) {
            issue_loads<CP, true, true, 0, EXACT, ST, FW, AUX>(a, t, lane, R);
            stage_tile<CP, false, EXACT, ST, true, FC, FW, AUX>(a, t, L, lane, R, tile_no);
        } else {
            issue_loads<CP, true, true, 1, EXACT, ST, FW, AUX>(a, t, lane, R);
            stage_tile<CP, true, EXACT, ST, true, FC, FW, AUX>(a, t, L, lane, R, tile_no);
        }
        // MS: the tile's pre mask bytes are in memory before the hand-off, so that the consumer's publication covers them
        if constexpr (MS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    MlpRegs<CP> Wr;        // exact-f32 operands (f32 storage)
    MlpRegsBf<CP> Wb;      // bf16 operands (bf16 storage)
    MlpRegsSplit<CP> Ws;   // bf16 hi/lo operand pairs (fp32 storage, ncahip_cond_precision(1))
    // CARRY: number of parked cells (wave-uniform) and the consumer's carry, on the W1 / W2 images (nothing without CARRY)
    [[maybe_unused]] int carry_n = 0;
    [[maybe_unused]] float* const CR = smem + pair * kCarrySize;
    // MS, consumer: the counters of the pair's unpublished tiles of the current step wait in ONE register, a ring over the lanes:
    // entry i (oldest first) in lane (head + i) mod 64, npend entries, of which the first `ready` are publishable -- every cell of
    // theirs is stored or on its way.  They are published one tile late, behind that tile's full groups (publish in consume): the
    // wave issues no loads, so the vmcnt(0) in front of the counter stores waits there for stores issued a tile's chain ago, i.e.
    // for nothing.
    [[maybe_unused]] int pend = 0, head = 0, npend = 0, ready = 0;
    [[maybe_unused]] unsigned pub_val = 0u;   // the counter value of the current step: steps of the grow completed with it
    [[maybe_unused]] auto publish = [&]() {
        if (ready == 0) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every store of this wave so far has completed (write-through)
        if (((lane - head) & 63) < ready) __hip_atomic_store(done + (unsigned)pend, pub_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        head = (head + ready) & 63;
        npend -= ready;
        ready = 0;
    };
    // FC: ng full groups of 16 listed cells of tile L, two per pass and one for an odd last one.  Without the carry ng counts the
    // partial last group too: its padding entries (kFirePad) compute on a real cell and write XR's padding column.
    auto fire_groups = [&]([[maybe_unused]] const TileLds& L, [[maybe_unused]] int ng) {
        if constexpr (FC) {
            const int* const FL = reinterpret_cast<const int*>(L.MK);
            auto cells = [&](auto nt, int gi) {
                constexpr int NTC = decltype(nt)::value;
                int zc[NTC], xc[NTC];
#pragma unroll
                for (int n = 0; n < NTC; ++n) {
                    const int e = FL[16 * (gi + n) + (lane & 15)];
                    zc[n] = e & 0xFFFF;
                    xc[n] = e >> 16;
                }
                float P[NTC][K::K1S];
                if (gi == 0) NCA_STAMP(4);
                perceive_cells_pipe<CP, NTC>(smem, L.Z, lane, zc, P);
                if (gi == 0) NCA_STAMP(5);
                mlp_cells_regs<CP, NTC>(Wr, smem, L.XR, lane, xc, P);
                if (gi == 0) NCA_STAMP(6);
            };
            int gi = 0;
#pragma unroll 1
            for (; gi + 2 <= ng; gi += 2) cells(std::integral_constant<int, 2>{}, gi);
            if (gi < ng) cells(std::integral_constant<int, 1>{}, gi);
        }
    };
    // flush (CARRY only): after the pair's last round -- no tile, one padded group on what the carry still holds
    auto consume = [&](const WTile& t, int which, [[maybe_unused]] bool flush) {
        if (!flush && !t.valid) return;
        const TileLds L = lds_of(which);
        if constexpr (CARRY) {
            using KC = FireCarry<CP>;
            const int* const FL = reinterpret_cast<const int*>(L.MK);
            int q = 0, rem = 0;
            if (!flush) {
                const int nf = __builtin_amdgcn_readfirstlane(*L.NF);
                q = nf >> 4;
                rem = nf & 15;
                fire_groups(L, q);   // the full groups, as without the carry
                if constexpr (MS) publish();
            }
            // the lane's own places in the carry: derived here, from an opaque lane id, so that nothing of it is kept in
            // registers through the full groups above
            int lane_c = lane;
            asm volatile("" : "+v"(lane_c));
            float* const CP_ = CR + KC::OFF_P + lane_c;
            float* const CX = CR + KC::OFF_X;
            int* const CPIX = reinterpret_cast<int*>(CR + KC::OFF_PIX) + lane_c;
            int* const CBAT = reinterpret_cast<int*>(CR + KC::OFF_BAT) + lane_c;
            const int g = (lane_c >> 4) & 3, col = lane_c & 15;
            float P1[1][K::K1S];
            bool has = false, run = flush;   // has: this lane's column took a remainder cell of this tile; run: a carry group is due
            int xcell = 0, pix = 0;
            // lane (g, col) moves channel rows 4g..4g+3 of its cell between the tile's XR and its slot of the carry
            auto park_x = [&]() {
#pragma unroll
                for (int k = 0; k < 4; ++k) CX[(4 * g + k) * KC::XCS + col] = L.XR[(4 * g + k) * XRS + xcell];
                *CPIX = pix;
                *CBAT = t.b;
            };
            if (!flush) {
                if (rem > 0) {
                    // remainder entry e -> MFMA column (carry_n + e) mod 16: behind the parked cells, wrapping to column 0
                    const int e = (col - carry_n) & 15;
                    has = e < rem;
                    const int ent = has ? FL[16 * q + e] : kFirePad;
                    const int zc[1] = {ent & 0xFFFF};
                    xcell = ent >> 16;
                    pix = __mul24(t.ty0 + (xcell >> 4), W) + t.tx0 + (xcell & 15);
                    perceive_cells_pipe<CP, 1>(smem, L.Z, lane, zc, P1);
                    if (carry_n + rem >= 16) {
                        run = true;
                    } else {
                        if (has) {
#pragma unroll
                            for (int s_ = 0; s_ < K::K1S; ++s_) CP_[s_ * 64] = P1[0][s_];
                            park_x();
                        }
                        carry_n += rem;
                    }
                }
            } else {
#pragma unroll
                for (int s_ = 0; s_ < K::K1S; ++s_) P1[0][s_] = 0.0f;
            }
            if (run) {
                // columns < carry_n hold parked cells; the others took this tile's remainder cells (flush: nothing, they compute
                // on zeros and are not stored).  A remainder cell that wrapped into a parked column swaps its P in and waits.
                const bool old = col < carry_n;
                if (old) {
#pragma unroll
                    for (int s_ = 0; s_ < K::K1S; ++s_) {
                        const float parked = CP_[s_ * 64];
                        if (has) CP_[s_ * 64] = P1[0][s_];
                        P1[0][s_] = parked;
                    }
                } else if (has) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) CX[(4 * g + k) * KC::XCS + col] = L.XR[(4 * g + k) * XRS + xcell];
                }
                const int xc1[1] = {col};
                mlp_cells_regs<CP, 1, KC::XCS>(Wr, smem, CX, lane, xc1, P1);
                // this tile's cells go back into its XR (store_tile below writes them); the parked ones go to x_out from here,
                // after the tile stores of the rounds they came from (those wrote their state before the update) have completed
                if (!old && has) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) L.XR[(4 * g + k) * XRS + xcell] = CX[(4 * g + k) * KC::XCS + col];
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if constexpr (MS) view_out();
                store_carry<CP, EXACT, kNtStore>(a, CX, lane, old, *CPIX, *CBAT);
                if (old && has) park_x();
                carry_n = flush ? 0 : carry_n + rem - 16;
                if constexpr (MS) ready = npend;   // what is parked now came from this tile: every listed tile (all older, or with the flush all) is complete
            }
            if (flush) return;
        } else if constexpr (FC) {
            fire_groups(L, (__builtin_amdgcn_readfirstlane(*L.NF) + 15) >> 4);
        } else {
            constexpr int NT = 2;
#pragma unroll 1
            for (int pass = 0; pass < WTH / NT; ++pass) {
                float P[NT][K::K1S];
                if (pass == 0) NCA_STAMP(4);
#ifdef NCA_STAMPS
                // diagnostic knobs (stamps build only): 0xD1A8 = no perception, 0xD1A9 = no MLP
                if (a.seed == 0xD1A8ull || a.seed == 0xD1AAull || a.seed == 0xD1ADull) {
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int s_ = 0; s_ < K::K1S; ++s_) P[n][s_] = L.Z[lane + n];
                } else
#endif
                perceive_tile_pipe<CP, NT>(smem, L.Z, lane, pass * NT, P);   // next channel group's LDS reads in flight
                if (pass == 0) NCA_STAMP(5);
#ifdef NCA_STAMPS
                if (a.seed == 0xD1A9ull || a.seed == 0xD1ABull || a.seed == 0xD1ADull) {
                    float acc_ = 0.0f;
#pragma unroll
                    for (int n = 0; n < NT; ++n)
#pragma unroll
                        for (int s_ = 0; s_ < K::K1S; ++s_) acc_ += P[n][s_];
                    L.XR[lane] = acc_;
                } else
#endif
                if constexpr (SPLIT) mlp_tile_split<CP, NT>(Ws, smem + K::OFF_B1, smem + K::OFF_B2, L.XR, L.MK, lane, pass * NT, P);
                else if constexpr (BF) mlp_tile_bf16<CP, NT>(Wb, smem + K::OFF_B1, smem + K::OFF_B2, L.XR, L.MK, lane, pass * NT, P);
                else mlp_tile_regs<CP, NT>(Wr, smem, L.XR, L.MK, lane, pass * NT, P);
                if (pass == 0) NCA_STAMP(6);
            }
        }
        NCA_STAMP(7);
#ifdef NCA_STAMPS
        if (a.seed == 0xD1ACull || a.seed == 0xD1ADull || a.seed == 0xD1AEull) return;   // diagnostic knob: no store (0xD1AE: nothing else changed)
#endif
        if constexpr (MS) view_out();
        if (t.inner) store_tile<CP, false, EXACT, kNtStore && !BF, ST>(a, t, L.XR, lane);   // bf16 rows are 32-byte segments: let the L2 merge them
        else store_tile<CP, true, EXACT, kNtStore && !BF, ST>(a, t, L.XR, lane);
        NCA_STAMP(8);
    };

    int which = 0;
    Pos pos = pos_first();
    WTile cur = tile_of(pos);
    // MS: a wave's boundary words (valid from the second barrier on), and the walk's first position back from them
    [[maybe_unused]] auto ms_save = [&]() {
        if (lane == 0) {
            WS_[MS_R] = pos.r, WS_[MS_T] = pos.t, WS_[MS_SX] = pos.sx, WS_[MS_SY] = pos.sy, WS_[MS_B] = pos.b;
        }
        wave_sync();
    };
    [[maybe_unused]] auto ms_pos0 = [&]() -> Pos { return Pos{0, ms_get(MS_R), ms_get(MS_T), ms_get(MS_SX), ms_get(MS_SY), ms_get(MS_B)}; };
    // Hand-off between the two waves of a pair: two monotonic round counters in LDS instead of a workgroup barrier per
    // tile.  A workgroup barrier keeps the four pairs of a CU in lock-step, so their perception phases (LDS-bandwidth-bound)
    // and their stores all collide; with pair-local hand-offs the pairs drift apart.  LDS operations of one wave execute in
    // order, so "data, then counter" on the writer side and "counter, then data" on the reader side is all the ordering
    // needed.  The polls are bounded (a broken hand-off never hangs the device; it sets the sticky error word, see await).
    int* const flags = reinterpret_cast<int*>(smem + PK::offs(pair, 0).scr + PK::SCR_FLAG);
    auto post = [&](int idx, int round) {
        wave_sync();
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this wave's LDS traffic for the round is done
        if (lane == 0) __hip_atomic_store(flags + idx, round, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto await = [&](int idx, int round) {
        int spins = 0;
        while (__hip_atomic_load(flags + idx, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < round && ++spins < (1 << 20))
            __builtin_amdgcn_s_sleep(1);
        // an expired poll means the partner wave never posted: the tile about to be used is stale.  The launch still drains (no
        // hung device), but the failure is RECORDED in the sticky host-visible error word, which the grow drivers and
        // ncahip_check_errors turn into a non-zero return code -- never silent wrong numbers.
        if (spins >= (1 << 20) && lane == 0 && a.err) __hip_atomic_fetch_or(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        wave_sync();
    };
    // The two roles run separate loops (all branches are wave-uniform): the consumer's 128 weight registers are then not
    // live in the producer's code and vice versa.
    if (producer) {
        if (lane == 0) { flags[0] = -1; flags[1] = -1; }
        // At equal priority the (older) consumer waves win every arbitration and the producer only issues in the gaps
        // of their MFMA stream; its instructions are few: let them go first.
        __builtin_amdgcn_s_setprio(3);
        produce(cur, 0);              // overlaps the weight-image fill of the consumer waves
        post(0, 0);
        NCA_KSTAMP(1);
        __syncthreads();              // weight image complete, counters initialised
        if constexpr (PK::WIDE || CARRY) __syncthreads();   // ... and moved into the consumers' registers: the second buffers (wide carve) / the carries may overwrite it
        NCA_KSTAMP(2);
        if constexpr (MS) ms_save();   // the first position is still in `pos`: the first tile was staged before the barriers
        for (;;) {
            Pos pn;
            if (pos.k + 1 < n_rounds) {
                pn = advance(pos);
            } else {
                if constexpr (!MS) {
                    break;
                } else {   // the first tile of the next step follows the last of this one
                    if (step + 1 >= a_launch.ms_steps) break;
                    tile_no = 0;   // stamps only: every step stamps its tiles, the last step's stay
                    next_step();
                    pn = ms_pos0();
                }
            }
            const WTile nxt = tile_of(pn);
            __builtin_amdgcn_s_setprio(0);
            NCA_STAMP(0);
            [[maybe_unused]] GateLook look{nullptr, false, 0u};
            if constexpr (MS) {
                if (step > 0 && nxt.valid) look = gate_look(nxt);   // the launch's first step reads what earlier launches wrote
            }
            await(1, gbase + pn.k - 2);       // the consumer is done with the round that used this buffer
            NCA_STAMP(1);
            if constexpr (MS) {
                if (step > 0 && nxt.valid) gate(look, step);
            }
            NCA_STAMP(2);
            __builtin_amdgcn_s_setprio(3);
            NCA_STAMP(3);
#ifdef NCA_STAMPS
            if (a.seed != 0xD1A6ull && (a.seed < 0xD1AAull || a.seed > 0xD1ADull))  // diagnostic knob (stamps build only): idle producers
#endif
            produce(nxt, which ^ 1);
            NCA_STAMP(14);
            post(0, gbase + pn.k);
            cur = nxt;
            pos = pn;
            which ^= 1;
            ++tile_no;
        }
        NCA_KSTAMP(3);
    } else {
        NCA_KSTAMP(1);
        __syncthreads();
        NCA_KSTAMP(2);
        if constexpr (SPLIT) load_weights_split_lds<CP>(smem, lane, Ws);
        else if constexpr (BF) load_weights_bf16_lds<CP>(smem, lane, Wb);   // same image, rounded to bf16 operand pairs
        else mlp_load_regs<CP>(smem, lane, Wr);
        if constexpr (PK::WIDE || CARRY) {
            static_assert(!PK::WIDE || !SPLIT, "wide carve: the exact-f32 and the bf16 consumer");
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the image reads have landed
            __syncthreads();
        }
        if constexpr (MS) {
            ms_save();
            pub_val = (unsigned)a_launch.ms_t0 + 1u;
        }
        for (;;) {
            while (pos.k < n_rounds) {
                const Pos pn = advance(pos);
                const WTile nxt = tile_of(pn);
                NCA_STAMP(0);
                await(0, gbase + pos.k);  // this round's tile has been staged
                NCA_STAMP(1);
                if (tile_no == 2) NCA_KSTAMP(4);            // light stamps around one steady-state tile
#ifdef NCA_STAMPS
                if (a.seed != 0xD1A7ull)  // diagnostic knob: idle consumers
#endif
                consume(cur, which, false);
                if (tile_no == 2) NCA_KSTAMP(5);
                post(1, gbase + pos.k);
                if constexpr (MS) {
                    if (cur.valid) {
                        if (lane == ((head + npend) & 63)) pend = (cur.b * tgh + (cur.ty0 >> 2)) * tgw + (cur.tx0 >> 4);
                        ++npend;
                        if (carry_n == 0) ready = npend;   // nothing parked: every tile so far is complete
                        // every lane holds a tile and cells are still parked (no carry group for 64 tiles: hardly any cell fires): run the padded
                        // group now, as at the end of a step -- the same bits for every cell -- and publish
                        if (npend == kMsList && ready < npend) {
                            consume(cur, which, true);
                            publish();
                        }
                    }
                }
                NCA_STAMP(14);
                if (tile_no == 2) NCA_KSTAMP(6);
                if (tile_no == 3) NCA_KSTAMP(7);
                cur = nxt;
                pos = pn;
                which ^= 1;
                ++tile_no;
            }
            if constexpr (CARRY) {
                if (carry_n > 0) consume(cur, which, true);
            }
            if constexpr (!MS) {
                break;
            } else {
                // the step is complete for this pair: publish what is left NOW (the gates of the next step's first tiles, this pair's
                // own producer's among them, may be waiting for exactly these), then walk the same tiles again
                ready = npend;
                publish();
                if (step + 1 >= a_launch.ms_steps) break;
                ++pub_val;
                tile_no = 0;   // stamps only
                next_step();
                pos = ms_pos0();
                cur = tile_of(pos);
            }
        }
        NCA_KSTAMP(3);
    }
}

template <int CP, bool EXACT, typename ST = StF32, bool SPLIT = false, bool FC = false, bool CARRY = false, bool FW = false, bool MS = false>
hipError_t launch_cond_pc(const NcaCondArgs& a, hipStream_t st) {
    using PK = PCfg<CP>;
    auto kern = cond_step_fwd_pc_kernel<CP, EXACT, ST, SPLIT, FC, CARRY, FW, MS>;
    const size_t lds = (size_t)PK::LDS_FLOATS * sizeof(float);
    static NcaLdsAttr attr;   // per instantiation; keyed by device inside
    if (hipError_t e = attr.ensure(reinterpret_cast<const void*>(kern), lds); e != hipSuccess) return e;
    const int cus = nca_cu_count();
    const int nst = a.B * ((a.W + 15) / 16) * ((a.H + 15) / 16);
    int nwg = nst < cus ? nst : cus;
    if (const int cap = nca_modes().pc_wg_cap; cap > 0 && nwg > cap) nwg = cap;   // test hook
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(kThreadsW), lds, st, a);
    return hipGetLastError();
}

// the default kernels of the exact-f32, fp32-storage step (neither test hook set: pc_dense, pc_nocarry) have a twin that reads a.fire_words
bool pc_fire_words_kernels() { return !nca_modes().pc_dense && !nca_modes().pc_nocarry; }
// the exact-f32, fp32-storage step: firing-cell lists (narrow carve: with the carry) unless a test hook asks otherwise
template <int CP, bool EXACT>
hipError_t launch_cond_pc_f32(const NcaCondArgs& a, hipStream_t st) {
    if (nca_modes().pc_dense) return launch_cond_pc<CP, EXACT, StF32, false, false>(a, st);
    const bool fw = a.fire_words != nullptr && nca_cond_pc_fire_words_ok(a);
    if constexpr (CP <= 16) {
        if (fw) return launch_cond_pc<CP, EXACT, StF32, false, true, true, true>(a, st);
        if (!nca_modes().pc_nocarry) return launch_cond_pc<CP, EXACT, StF32, false, true, true>(a, st);
    } else {
        if (fw) return launch_cond_pc<CP, EXACT, StF32, false, true, false, true>(a, st);
    }
    return launch_cond_pc<CP, EXACT, StF32, false, true>(a, st);
}

}  // namespace

// W % 4 == 0 and 16-byte aligned x_in / goal: caller (nca_cond_generic.hip dispatch) guarantees it.
extern "C" void nca_debug_set_stamp_buffer_pc(void* p);
static unsigned long long* g_stamp_pc = nullptr;
extern "C" void nca_debug_set_stamp_buffer_pc(void* p) { g_stamp_pc = (unsigned long long*)p; }
#if defined(NCA_STAMPS)
unsigned long long* nca_debug_stamp_ptr() { return g_stamp_pc; }
#endif
// the firing-cell-list kernels as they run by default; the words' grid needs whole, aligned tiles and 8-byte aligned words
bool nca_cond_pc_fire_words_ok(const NcaCondArgs& a) {
    return pc_fire_words_kernels() && nca_modes().cond_precision == 0 && a.u == nullptr && a.C <= 20 && a.W % 16 == 0 && a.H % 4 == 0 &&
           ((uintptr_t)a.fire_words & 7) == 0;
}
hipError_t nca_launch_cond_step_fwd_pc(const NcaCondArgs& a_in, hipStream_t st) {
    NcaCondArgs a = a_in;
    a.dbg = g_stamp_pc;
    a.err = nca_error_word_device();
    const bool h64 = a.hidden == 64;
    if (nca_modes().cond_precision == 1 && h64) {   // opt-in bf16x3 emulation of the fp32 products (exact shapes only)
        if (a.C == 12) return launch_cond_pc<12, true, StF32, true>(a, st);
        if (a.C == 16) return launch_cond_pc<16, true, StF32, true>(a, st);
    }
    if (a.C == 12 && h64) return launch_cond_pc_f32<12, true>(a, st);
    if (a.C == 16 && h64) return launch_cond_pc_f32<16, true>(a, st);
    if (a.C <= 12) return launch_cond_pc_f32<12, false>(a, st);
    if (a.C <= 16) return launch_cond_pc_f32<16, false>(a, st);
    // the reference's default model, C = 3 + 1 + 16 = 20 (nca.py:62-94)
    if (a.C == 20 && h64) return launch_cond_pc_f32<20, true>(a, st);
    if (a.C <= 20) return launch_cond_pc_f32<20, false>(a, st);
    return hipErrorInvalidValue;
}

// Several steps of a grow in one launch (a.ms_steps >= 1 and the ms_* fields set, a.fire_words the words of the launch's first step):
// the MS twins of the narrow-carve kernels that read fire words.  The caller asks nca_cond_pc_fused_steps_ok first.
bool nca_cond_pc_fused_steps_ok(const NcaCondArgs& a) {
    if (nca_modes().pc_no_fused_steps || a.C > 16 || a.fire_words == nullptr || !nca_cond_pc_fire_words_ok(a)) return false;
    // At least two rounds per workgroup, as launch_cond_pc sizes the grid: with one, a pair's next tile is its own last one and
    // nothing overlaps the gate.  And at most kFusedMaxRounds: the fused launch saves about half of a step's fixed cost and pays
    // 8 - 10 % more per round (profiles/r9a_fixed_cost_fit.txt, B x 16 x 256^2 on 256 CUs: F 17.4 -> 9.2 us, v 7.18 -> 7.76 us per
    // round), which is -7 % per step at 4 rounds, -5 % at 8, even at 16 and +4.5 % at 32; the line through those crosses at 15.
    // With the step view formed per tile and the gate's first look ahead of the hand-off wait (profiles/r10a_fixed_cost_fit.txt) F is
    // 8.2 -> 7.3 us and v unchanged, 7.96 -> 7.94 us against 7.35 us: the per-round cost did not move, the cap stays.
    // A set fire-word chunk cap (test hook) waives the upper bound, as it waives the minimum grow length.
    constexpr long kFusedMaxRounds = 12;
    const long nst = (long)a.B * ((a.W + 15) / 16) * ((a.H + 15) / 16);
    long nwg = nst < nca_cu_count() ? nst : nca_cu_count();
    if (const int cap = nca_modes().pc_wg_cap; cap > 0 && nwg > cap) nwg = cap;
    const long rounds = (nst + nwg - 1) / nwg;
    return rounds >= 2 && (rounds <= kFusedMaxRounds || nca_modes().fire_words_cap > 0);
}
hipError_t nca_launch_cond_steps_fwd_pc(const NcaCondArgs& a_in, hipStream_t st) {
    if (a_in.ms_steps < 1 || a_in.ms_ring < 2 || !a_in.ms_states || !a_in.ms_pre || !a_in.ms_done || !nca_cond_pc_fused_steps_ok(a_in))
        return hipErrorInvalidValue;
    NcaCondArgs a = a_in;
    a.dbg = g_stamp_pc;
    a.err = nca_error_word_device();
    const bool h64 = a.hidden == 64;
    if (a.C == 12 && h64) return launch_cond_pc<12, true, StF32, false, true, true, true, true>(a, st);
    if (a.C == 16 && h64) return launch_cond_pc<16, true, StF32, false, true, true, true, true>(a, st);
    if (a.C <= 12) return launch_cond_pc<12, false, StF32, false, true, true, true, true>(a, st);
    return launch_cond_pc<16, false, StF32, false, true, true, true, true>(a, st);
}

// bf16 state / goal behind the float-typed pointers of NcaCondArgs.  Caller (nca_capi.hip) guarantees W % 4 == 0, 8-byte
// aligned x_in / x_out / goal, C <= 20, hidden <= 64, H*W < 2^24.
hipError_t nca_launch_cond_step_fwd_bf16(const NcaCondArgs& a_in, hipStream_t st) {
    NcaCondArgs a = a_in;
    a.dbg = g_stamp_pc;
    a.err = nca_error_word_device();
    const bool h64 = a.hidden == 64;
    if (a.C == 12 && h64) return launch_cond_pc<12, true, StBF16>(a, st);
    if (a.C == 16 && h64) return launch_cond_pc<16, true, StBF16>(a, st);
    if (a.C <= 12) return launch_cond_pc<12, false, StBF16>(a, st);
    if (a.C <= 16) return launch_cond_pc<16, false, StBF16>(a, st);
    if (a.C == 20 && h64) return launch_cond_pc<20, true, StBF16>(a, st);
    if (a.C <= 20) return launch_cond_pc<20, false, StBF16>(a, st);
    return hipErrorInvalidValue;
}

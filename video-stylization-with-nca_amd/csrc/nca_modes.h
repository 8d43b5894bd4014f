// nca_modes.h -- every process-wide setting of the library, in one place (definitions: nca_modes.hip).
//
// A setting is written by one host thread (an entry point of include/ncahip.h) and read by launchers on any other, so each is a
// relaxed atomic: no torn or cached value, and no ordering promised between a setter and a call racing it on another thread.
// The fields of NcaModes are read PER LAUNCH, where the launcher decides: a grow whose mode changes half-way changes kernels half-way.
// The DyNCA precision and the direction field are read ONCE PER CALL instead (every step of a call runs the same arithmetic).
//
// A new mode is a field here, its bit in ncahip_debug_force_generic (nca_modes.hip) or an entry point of its own, a term in nca_cond_fwd_default()
// if it routes the ConditionedNCA forward away from its default kernels, and a line in ops.reset_modes().
#pragma once
#include <atomic>

template <typename T>
struct NcaMode {
    std::atomic<T> v{T()};
    operator T() const { return v.load(std::memory_order_relaxed); }
    void operator=(T x) { v.store(x, std::memory_order_relaxed); }
};

struct NcaModes {
    // ConditionedNCA forward (nca_cond_generic.hip, nca_cond_pc.hip, cond_grow_fwd_impl in nca_capi.hip)
    NcaMode<bool> force_generic;   // the generic any-shape kernels                                   NCAHIP_FORCE_GENERIC at load / hook bit 0
    NcaMode<int> cond_variant;     // 0 = producer/consumer (default), 1 = symmetric wave-private     NCAHIP_COND_VARIANT at load / hook bit 1
    NcaMode<bool> pc_dense;        // the fp32 producer/consumer step runs every cell (no firing-cell lists)                      hook bit 5
    NcaMode<bool> pc_nocarry;      // firing-cell lists pad every tile's last group (no carry across a pair's tiles)              hook bit 6
    NcaMode<bool> no_fire_words;   // a grow's steps draw their fire masks themselves                                             hook bit 7
    NcaMode<int> pc_wg_cap;        // at most this many workgroups per producer/consumer step launch (0: no cap)                  hook bits 8-15
    NcaMode<int> fire_words_cap;   // at most this many steps per fire-word launch; set, it also waives the minimum grow length   hook bits 16-23
    NcaMode<bool> pc_no_fused_steps;   // a grow's steps go out one launch each, also where a fused-steps launch exists               hook bit 24
    NcaMode<int> fused_steps_cap;  // at most this many steps per fused-steps launch (0: a fire-word chunk's steps in one launch)     hook bits 25-27
    NcaMode<int> cond_precision;   // 0 = exact-f32 MFMA (default), 1 = bf16x3 emulation in the producer/consumer kernel          ncahip_cond_precision
    // ConditionedNCA backward (nca_cond_bwd.hip, nca_cond_bwd_fm.hip)
    NcaMode<bool> bwd_bf16_exact;  // bf16-history backward with exact-f32 products instead of bf16 MFMA   NCAHIP_BWD_BF16_EXACT at load / hook bit 2
    NcaMode<int> bwd_variant;      // kernel A: 0 = the faster form per mode (bf16 MFMA: front + matrix kernels; fp32 products: one launch), 1 = one
                                   // launch always, 2 = front + matrix always, 3 = the slower form per mode   NCAHIP_BWD_VARIANT at load / hook bit 3 (3 or 0)
    NcaMode<bool> fm_nosplit;      // the matrix kernel walks whole super-tiles on small grids too (its summation order then equals the
                                   // one-launch form's)                                                                          hook bit 4
    // persistent DyNCA steps (nca_dynca_persist.hip)
    NcaMode<int> persist_drop_tiles;   // the launch leaves out its last n tiles (their neighbours' polls expire)   ncahip_debug_persist_drop_tiles
    // the last ncahip_debug_force_generic argument was not 0: some test hook is set, a backward one included
    NcaMode<bool> hooked;
};
NcaModes& nca_modes();   // what launchers read, and what the entry points that set a mode write

// The ConditionedNCA forward runs its default exact-f32 producer/consumer family: what the persistent grow is the twin of.  It is the
// production path, so it also stays away from a process in which any test hook is set (`hooked`); the environment's two backward
// settings do not concern it.
inline bool nca_cond_fwd_default() {
    const NcaModes& m = nca_modes();
    return !m.hooked && !m.force_generic && m.cond_variant == 0 && m.cond_precision == 0;
}

// ---- one snapshot per call ------------------------------------------------------------------------------------------------------
// DyNCA precision (ncahip_dynca_precision): 0 = exact fp32 (default), 1 = both 1x1 products of the forward step on bf16 MFMA; read at
// enqueue time by the fp32 forward entry points only (never by a backward one)
int nca_dynca_precision();
int nca_dynca_precision_exchange(int mode);   // returns the previous mode
// The range of mode 1 (ncahip_dynca_bf16_range): 0 = narrow (C <= 16, fc <= 128; default), 1 = wide (C <= 32, fc <= 256: single-scale
// unsteered per-step kernels beyond the narrow range).  It lives in ONE word with the precision, so the snapshot a call takes is a
// pair some setter left behind, never half of one change and half of another.
struct NcaDyncaPrec {
    int precision, range;
};
NcaDyncaPrec nca_dynca_prec_snapshot();
int nca_dynca_bf16_range_exchange(int range);   // returns the previous range

// Steered perception (ncahip_dynca_direction): the per-cell direction field [Bd,2,H,W] (plane 0 = s, plane 1 = c) the DyNCA forward
// rotates every Sobel pair by; p == nullptr: none attached
struct NcaDyncaDir {
    const float* p;
    int Bd, H, W;
};
NcaDyncaDir nca_dynca_dir_snapshot();
void nca_dynca_dir_set(const NcaDyncaDir& d);

// nca_modes.hip -- the one definition site of the library's process-wide modes (nca_modes.h): their storage, the four environment
// variables that give initial values, and the test hook that decodes one integer into them.  No kernels.
#include "nca_modes.h"

#include <cstdlib>
#include <mutex>

#include "../../include/ncahip.h"

namespace {

// The environment gives the initial values, read once when the library is loaded; the first ncahip_debug_force_generic overwrites them.
struct ModesFromEnv : NcaModes {
    ModesFromEnv() {
        force_generic = getenv("NCAHIP_FORCE_GENERIC") != nullptr;
        if (const char* e = getenv("NCAHIP_COND_VARIANT")) cond_variant = atoi(e);
        bwd_bf16_exact = getenv("NCAHIP_BWD_BF16_EXACT") != nullptr;
        if (const char* e = getenv("NCAHIP_BWD_VARIANT")) bwd_variant = atoi(e);
    }
} g_modes;

std::atomic<int> g_dynca_prec{0};   // precision | range << 8: one word, so that a call's snapshot is one consistent pair
std::mutex g_dynca_dir_mu;
NcaDyncaDir g_dynca_dir{nullptr, 0, 0, 0};

}  // namespace

NcaModes& nca_modes() { return g_modes; }

int nca_dynca_precision() { return g_dynca_prec.load(std::memory_order_relaxed) & 255; }
int nca_dynca_precision_exchange(int mode) {
    int cur = g_dynca_prec.load(std::memory_order_relaxed);
    while (!g_dynca_prec.compare_exchange_weak(cur, (cur & ~255) | mode, std::memory_order_relaxed)) {}
    return cur & 255;
}
NcaDyncaPrec nca_dynca_prec_snapshot() {
    const int v = g_dynca_prec.load(std::memory_order_relaxed);
    return NcaDyncaPrec{v & 255, (v >> 8) & 255};
}
int nca_dynca_bf16_range_exchange(int range) {
    int cur = g_dynca_prec.load(std::memory_order_relaxed);
    while (!g_dynca_prec.compare_exchange_weak(cur, (cur & 255) | (range << 8), std::memory_order_relaxed)) {}
    return (cur >> 8) & 255;
}

NcaDyncaDir nca_dynca_dir_snapshot() {
    std::lock_guard<std::mutex> lk(g_dynca_dir_mu);
    return g_dynca_dir;
}
void nca_dynca_dir_set(const NcaDyncaDir& d) {
    std::lock_guard<std::mutex> lk(g_dynca_dir_mu);
    g_dynca_dir = d;
}

// The bit layout of the test hook, written once: every call overwrites every field its bits cover (0 puts all of them at their defaults).
extern "C" int ncahip_debug_force_generic(int on) {
    NcaModes& m = g_modes;
    m.hooked = on != 0;
    m.force_generic = (on & 1) != 0;        // bit 0: generic any-shape kernels
    m.cond_variant = (on >> 1) & 1;         // bit 1: symmetric wave-private ConditionedNCA kernel instead of producer/consumer
    m.bwd_bf16_exact = (on & 4) != 0;       // bit 2: bf16-history backward with exact-f32 products instead of bf16 MFMA
    m.bwd_variant = (on & 8) ? 3 : 0;       // bit 3: ConditionedNCA backward kernel A in the form that is NOT the mode's default (one launch <-> front + matrix)
    m.fm_nosplit = (on & 16) != 0;          // bit 4: the matrix kernel walks whole super-tiles on small grids too
    m.pc_dense = (on & 32) != 0;            // bit 5: the fp32 producer/consumer step runs every cell (no firing-cell lists)
    m.pc_nocarry = (on & 64) != 0;          // bit 6: firing-cell lists pad every tile's last group (no carry across a pair's tiles)
    m.no_fire_words = (on & 128) != 0;      // bit 7: ncahip_cond_grow_fwd_f32's steps draw their fire masks themselves
    m.pc_wg_cap = (on >> 8) & 255;          // bits 8-15: at most this many workgroups per producer/consumer step launch (0: no cap)
    m.fire_words_cap = (on >> 16) & 255;    // bits 16-23: at most this many steps per fire-word launch (0: no cap); waives the minimum grow length
    m.pc_no_fused_steps = (on & (1 << 24)) != 0;   // bit 24: one launch per step, also where ncahip_cond_grow_fwd_f32 would fuse a chunk's steps
    m.fused_steps_cap = (on >> 25) & 7;     // bits 25-27: at most this many steps per fused-steps launch (0: no cap)
    return 0;
}

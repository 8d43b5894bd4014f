// nca_capi.hip -- extern "C" entry points of libncahip.so (declared in include/ncahip.h).
// Validates arguments on the host (shapes the kernels and their grids assume), then enqueues.
#include "../../include/ncahip.h"

#include <cstdarg>
#include <cstdio>

#include "nca_kernels.h"

namespace {

constexpr int kMaxC = 16, kMaxCCondFwd = 32, kMaxCCondFwdBf16 = 20, kMaxCDynca = 32, kMaxFc = 128, kMaxFcFwd = 1024, kMaxHidden = 64, kMaxCond = 4;   // DyNCA forward: C <= 32 (configs[4]), fc in 128-wide slices

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_result(hipError_t e, const char* what, const char* part = "") {
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s%s: %s", what, part, hipGetErrorString(e));
    return (int)e;
}

// `u` holds bit-packed fire masks instead of uniforms (include/ncahip.h: NCAHIP_SEED_U_IS_BITS)
bool u_is_bits(const void* u, uint64_t seed) { return u != nullptr && seed == NCAHIP_SEED_U_IS_BITS; }
// u of step t: floats are [T][B*H*W]; bits are [T][ceil(B*H*W / 32)] words
const float* u_at(const float* u, bool bits, int t, size_t cells) {
    if (!u) return nullptr;
    return bits ? reinterpret_cast<const float*>(reinterpret_cast<const uint32_t*>(u) + (size_t)t * ((cells + 31) / 32)) : u + (size_t)t * cells;
}
int check_bits(bool bits, int B, int H, int W, float rate, bool dynca) {
    if (!bits) return 0;
    if ((size_t)B * H * W >= (((size_t)1 << 32) - 64)) return fail(NCAHIP_ERANGE, "bit-packed fire masks: B*H*W must stay below 2^32");
    if (dynca && !(rate >= 0.0f && rate < 1.0f)) return fail(NCAHIP_ERANGE, "bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)");
    return 0;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// n floats of zeros for an accumulator that a driver's kernels add to: hipMemsetAsync -- except on a capturing stream, where a kernel
// writes them.  A replayed graph does not keep a memset node ahead of the kernel nodes behind it (measured on the backward rows of
// tests/test_gpu_graph_replay.py: the accumulators were zeroed under the first step's flush, every replay gave other gradients); a
// kernel node it does keep in its place.  Outside a capture nothing changes.
hipError_t nca_zero_async(float* p, size_t n, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipError_t e = hipStreamIsCapturing(st, &cs); e != hipSuccess) return e;
    if (cs == hipStreamCaptureStatusNone) return hipMemsetAsync(p, 0, n * sizeof(float), st);
    return nca_launch_zero_words(reinterpret_cast<uint32_t*>(p), n, st);
}

bool dims_ok(int B, int C, int H, int W) {
    return B > 0 && C > 0 && H > 0 && W > 0 && (size_t)B * C * H * W < ((size_t)1 << 40);
}

int check_dynca(const void* x_in, const void* x_out, const void* cond, const void* w1, const void* b1, const void* w2,
                const void* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode, int max_fc = kMaxFc) {
    if (!x_in || !x_out || !w1 || !b1 || !w2 || !b2) return fail(NCAHIP_EINVAL, "dynca step: null pointer");
    if (!dims_ok(B, C, H, W) || fc <= 0 || c_cond < 0) return fail(NCAHIP_EINVAL, "dynca step: bad size");
    if ((c_cond > 0) != (cond != nullptr)) return fail(NCAHIP_EINVAL, "dynca step: cond pointer / c_cond mismatch");
    if (pad_mode < 0 || pad_mode > 3) return fail(NCAHIP_EINVAL, "dynca step: bad pad_mode %d", pad_mode);
    if (pad_mode == NCAHIP_PAD_REFLECT && (H < 2 || W < 2)) return fail(NCAHIP_EINVAL, "reflect pad needs H,W >= 2");
    if (C > kMaxCDynca || fc > max_fc || c_cond > kMaxCond)
        return fail(NCAHIP_ERANGE, "dynca step: C=%d fc=%d c_cond=%d exceeds (%d,%d,%d)", C, fc, c_cond, kMaxCDynca, max_fc,
                    kMaxCond);
    if (x_in == x_out) return fail(NCAHIP_EINVAL, "dynca step: x_in and x_out must not alias (halo reads)");
    return 0;
}

// two-scale perception: the fixed filters also run on the H/2 x W/2 grid with the pad mode resolved there, and F.pad(mode="reflect")
// needs the pad (1) to be smaller than the dimension (the reference raises on a 1-wide coarse grid; nca_pad_index would clamp)
int check_ms_reflect(int H, int W, int pad_mode) {
    if (pad_mode == NCAHIP_PAD_REFLECT && (H < 4 || W < 4))
        return fail(NCAHIP_EINVAL, "dynca two-scale step: reflect pad needs a coarse grid of at least 2 x 2 (H, W >= 4); H=%d W=%d gives %d x %d", H, W, H / 2, W / 2);
    return 0;
}

int check_cond(const void* x_in, const void* x_out, const void* pre_out, const void* goal, const void* wp,
               const void* w1, const void* b1, const void* w2, const void* b2, const void* w3, int B, int C, int H,
               int W, int hidden, int goal_ch, int alive_ch, int max_c = kMaxC) {
    if (!x_in || !x_out || !pre_out || !wp || !w1 || !b1 || !w2 || !b2 || !w3)
        return fail(NCAHIP_EINVAL, "cond step: null pointer");
    if (!dims_ok(B, C, H, W) || hidden <= 0 || goal_ch < 0) return fail(NCAHIP_EINVAL, "cond step: bad size");
    if ((goal_ch > 0) != (goal != nullptr)) return fail(NCAHIP_EINVAL, "cond step: goal pointer / goal_ch mismatch");
    if (goal_ch > C || alive_ch >= C) return fail(NCAHIP_EINVAL, "cond step: goal_ch/alive_ch outside C=%d", C);
    if (C > max_c || hidden > kMaxHidden)
        return fail(NCAHIP_ERANGE, "cond step: C=%d hidden=%d exceeds (%d,%d)", C, hidden, max_c, kMaxHidden);
    if (x_in == x_out) return fail(NCAHIP_EINVAL, "cond step: x_in and x_out must not alias (halo reads)");
    return 0;
}

int check_ms(int C, int H, int W, int fc, int pad_mode, const void* pc) {
    if (!pc) return fail(NCAHIP_EINVAL, "dynca two-scale step: pc_scratch required");
    if (int rc = check_ms_reflect(H, W, pad_mode)) return rc;
    if ((H | W) & 1) return fail(NCAHIP_ERANGE, "dynca two-scale step: H and W must be even (the x2 resampling is then the exact 2x2 mean / (0.25, 0.75) blend)");
    if (C > kMaxC || fc > kMaxFc) return fail(NCAHIP_ERANGE, "dynca two-scale step: C=%d fc=%d exceeds (%d,%d)", C, fc, kMaxC, kMaxFc);
    return 0;
}

}  // namespace

// ---- sticky device error word: one host-mapped word per device, written by kernels (system-scope atomic OR), read by the host
// without synchronising -------------------------------------------------------------------------------------------------
namespace {
struct ErrWord {
    std::atomic<int> state{0};   // 0 = not allocated, 1 = ready, 2 = allocation failed
    unsigned* host = nullptr;
    unsigned* dev = nullptr;
};
ErrWord g_errw[kNcaMaxDevices];
ErrWord& errw() {
    ErrWord& w = g_errw[nca_device_index()];
    if (w.state.load(std::memory_order_acquire) == 0) {
        static std::atomic_flag lock = ATOMIC_FLAG_INIT;
        while (lock.test_and_set(std::memory_order_acquire)) {}
        if (w.state.load(std::memory_order_relaxed) == 0) {
            void *h = nullptr, *d = nullptr;
            int st = 2;
            if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
                *(volatile unsigned*)h = 0u;
                w.host = (unsigned*)h;
                w.dev = (unsigned*)d;
                st = 1;
            }
            w.state.store(st, std::memory_order_release);
        }
        lock.clear(std::memory_order_release);
    }
    return w;
}
}  // namespace
unsigned* nca_error_word_device() { return errw().dev; }
unsigned nca_error_word_read(bool clear) {
    ErrWord& w = errw();
    if (!w.host) return 0u;
    const unsigned v = *(volatile unsigned*)w.host;
    if (clear && v) *(volatile unsigned*)w.host = 0u;
    return v;
}
// positive return code of a recorded device-side failure (distinct from every hipError_t in use)
static int device_error_rc(const char* where) {
    const unsigned v = nca_error_word_read(false);
    if (!v) return 0;
    return fail(NCAHIP_EDEVICE, "%s: a device-side failure was recorded earlier on this device (error word 0x%x: bit 0 = "
                "producer/consumer hand-off poll expired, bit 1 = neighbour poll of a persistent DyNCA / ConditionedNCA kernel expired, bit 2 = tile "
                "gate of a fused-steps ConditionedNCA launch expired); results since "
                "the last ncahip_check_errors are not valid", where, v);
}

extern "C" {

int ncahip_check_errors(ncahip_stream_t stream, int clear) {
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return hip_result(e, "check_errors sync");
    const unsigned v = nca_error_word_read(clear != 0);
    if (!v) return 0;
    return fail(NCAHIP_EDEVICE, "device error word 0x%x (bit 0: a producer/consumer hand-off poll expired -- the affected launch "
                "produced stale tiles; bit 1: a neighbour poll of a persistent DyNCA / ConditionedNCA kernel expired -- that launch stopped early; "
                "bit 2: a tile gate of a fused-steps ConditionedNCA launch expired -- its later steps read tiles that were not ready)", v);
}

int ncahip_debug_inject_error(unsigned bits) {   // test hook: what a kernel does when a poll expires
    unsigned* h = errw().host;
    if (!h) return fail(NCAHIP_EINVAL, "no error word on this device");
    *(volatile unsigned*)h |= bits;
    return 0;
}

int ncahip_debug_persist_drop_tiles(int n) {   // test hook: see NcaModes::persist_drop_tiles
    nca_modes().persist_drop_tiles = n < 0 ? 0 : n;
    return 0;
}

int ncahip_version(void) { return NCAHIP_VERSION; }
const char* ncahip_last_error(void) { return g_err; }

int ncahip_cond_precision(int mode) {
    if (mode != 0 && mode != 1) return fail(NCAHIP_EINVAL, "cond precision: 0 (exact fp32) or 1 (bf16x3)");
    nca_modes().cond_precision = mode;
    return 0;
}

int ncahip_dynca_precision(int mode) {
    if (mode != 0 && mode != 1) return fail(NCAHIP_EINVAL, "dynca precision: 0 (exact fp32) or 1 (bf16 MFMA)");
    return nca_dynca_precision_exchange(mode);
}
static bool dynca_bf16_mfma(int C, int fc) { return nca_dynca_precision() == 1 && nca_dynca_bf16_shape_ok(C, fc); }
int ncahip_dynca_bf16_range(int range) {
    if (range != 0 && range != 1) return fail(NCAHIP_EINVAL, "dynca bf16 range: 0 (narrow: C <= 16, fc <= 128) or 1 (wide: C <= 32, fc <= 256)");
    return nca_dynca_bf16_range_exchange(range);
}

// Steered perception: the direction field (nca_modes.h) is process-wide like the precision; the eight fp32 forward entry points that
// honour the precision take ONE snapshot per call at enqueue time (the clip drivers hand theirs to the steps they enqueue).  Every
// other DyNCA step entry point refuses to run while a field is attached: a silently unsteered result or gradient is the failure to exclude.
namespace {
// an honouring entry point: the attached field must fit the call
int dynca_dir_check(const NcaDyncaDir& d, const char* who, int B, int H, int W) {
    if (!d.p) return 0;
    if (H != d.H || W != d.W)
        return fail(NCAHIP_EINVAL, "%s: the attached direction field (ncahip_dynca_direction) is %d x %d, the call is %d x %d", who, d.H, d.W, H, W);
    if (d.Bd != 1 && d.Bd != B)
        return fail(NCAHIP_EINVAL, "%s: the attached direction field (ncahip_dynca_direction) has Bd = %d, the call B = %d (Bd must be 1 or B)", who, d.Bd, B);
    return 0;
}
// an entry point that does not steer (backward, bf16 storage)
int dynca_dir_refuse(const char* who) {
    if (!nca_dynca_dir_snapshot().p) return 0;
    return fail(NCAHIP_EINVAL, "%s: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first", who);
}
}  // namespace
int ncahip_dynca_direction(const float* dirs, int Bd, int H, int W) {
    if (dirs && (Bd < 1 || H < 1 || W < 1)) return fail(NCAHIP_EINVAL, "dynca direction field: Bd=%d H=%d W=%d must all be positive", Bd, H, W);
    nca_dynca_dir_set(dirs ? NcaDyncaDir{dirs, Bd, H, W} : NcaDyncaDir{nullptr, 0, 0, 0});
    return 0;
}

int ncahip_limits(int* max_c, int* max_fc, int* max_hidden) {
    if (max_c) *max_c = kMaxC;
    if (max_fc) *max_fc = kMaxFc;
    if (max_hidden) *max_hidden = kMaxHidden;
    return 0;
}

int ncahip_selftest(void* scratch, ncahip_stream_t stream) {
    if (!scratch) return fail(NCAHIP_EINVAL, "selftest: null scratch");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(scratch, 0, 64, st);
    if (e != hipSuccess) return hip_result(e, "selftest memset");
    e = nca_launch_selftest((int*)scratch, st);
    if (e != hipSuccess) return hip_result(e, "selftest launch");
    int host = 0;
    e = hipMemcpyAsync(&host, scratch, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_result(e, "selftest sync");
    return host == 1 ? 0 : fail(NCAHIP_ERANGE, "selftest: MFMA 16x16x4 f32 lane map differs from the one assumed");
}

int ncahip_dynca_perceive_f32(const float* x, float* y, int B, int C, int H, int W, int pad_mode,
                              ncahip_stream_t stream) {
    if (!x || !y || x == y) return fail(NCAHIP_EINVAL, "dynca_perceive: null or aliased pointer");
    if (!dims_ok(B, C, H, W) || pad_mode < 0 || pad_mode > 3) return fail(NCAHIP_EINVAL, "dynca_perceive: bad argument");
    if (pad_mode == NCAHIP_PAD_REFLECT && (H < 2 || W < 2)) return fail(NCAHIP_EINVAL, "reflect pad needs H,W >= 2");
    return hip_result(nca_launch_dynca_perceive(x, y, B, C, H, W, pad_mode, (hipStream_t)stream), "dynca_perceive");
}

int ncahip_cond_perceive_f32(const float* z, const float* wp, float* y, int B, int C, int H, int W,
                             ncahip_stream_t stream) {
    if (!z || !wp || !y || z == y) return fail(NCAHIP_EINVAL, "cond_perceive: null or aliased pointer");
    if (!dims_ok(B, C, H, W)) return fail(NCAHIP_EINVAL, "cond_perceive: bad size");
    return hip_result(nca_launch_cond_perceive(z, wp, y, B, C, H, W, (hipStream_t)stream), "cond_perceive");
}

// ---- the DyNCA forward: one body for single step / T steps x fp32 / two-scale fp32 / bf16 storage ------------------------------
// fp32: C <= 32, fc in 128-wide slices.  Two-scale (perception_scales = [0, 1]): a coarse pass into pc_scratch, then the fused step
// with on-the-fly bilinear up-sampling.  bf16: storage format only (same kernel, exact f32 compute, RNE on store).
enum DyncaFwdKind { kDyncaFwdF32, kDyncaFwdMs, kDyncaFwdBf16 };
// single: the one step x_in -> x_out.  Otherwise x_in is a ring of `ring` state slots and step t goes from slot t % ring to slot
// (t + 1) % ring.  Nothing is enqueued before all checks have passed.
static int dynca_fwd_impl(DyncaFwdKind kind, const char* what, bool single, const void* x_in, void* x_out, int ring, int T, const float* cond, const float* u,
                          const float* w1, const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond,
                          int pad_mode, float update_rate, uint64_t seed, uint64_t step0, float* pc_scratch, ncahip_stream_t stream,
                          const NcaDyncaDir* dir_of_caller = nullptr) {
    const bool ms = kind == kDyncaFwdMs, bf16 = kind == kDyncaFwdBf16;
    if (bf16) {
        if (int rc = dynca_dir_refuse(what)) return rc;
    }
    const NcaDyncaDir dir = bf16 ? NcaDyncaDir{nullptr, 0, 0, 0} : dir_of_caller ? *dir_of_caller : nca_dynca_dir_snapshot();   // one read per call
    char* const states = (char*)const_cast<void*>(x_in);
    if (!single && (ring < 2 || T < 0)) return fail(NCAHIP_EINVAL, "dynca nsteps: ring >= 2 and T >= 0 required");
    if (int rc = check_dynca(x_in, single ? x_out : states + 1, cond, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode,
                             kind == kDyncaFwdF32 ? kMaxFcFwd : kMaxFc))
        return rc;
    if (ms) {
        if (int rc = check_ms(C, H, W, fc, pad_mode, pc_scratch)) return rc;
    }
    if (int rc = dynca_dir_check(dir, what, B, H, W)) return rc;
    const bool ubits = u_is_bits(u, seed);
    if (int rc = check_bits(ubits, B, H, W, update_rate, true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t slot = (size_t)B * C * H * W * (bf16 ? sizeof(uint16_t) : sizeof(float)), uslot = (size_t)B * H * W;
    // one read per call: every step of it runs the same arithmetic.  Mode 1 covers the narrow range in every form; in the wide range
    // (ncahip_dynca_bf16_range 1) also the single-scale unsteered step up to C = 32 / fc = 256.  Everything else runs exactly.
    const NcaDyncaPrec prec = bf16 ? NcaDyncaPrec{0, 0} : nca_dynca_prec_snapshot();
    const bool bfw = prec.precision == 1 && prec.range == 1 && !ms && !dir.p && !nca_dynca_bf16_shape_ok(C, fc) && nca_dynca_bf16_wide_shape_ok(C, fc);
    const bool bf = prec.precision == 1 && (nca_dynca_bf16_shape_ok(C, fc) || bfw);
    for (int t = 0; t < T; ++t) {
        const float* const xi = reinterpret_cast<const float*>(single ? x_in : states + (size_t)(t % ring) * slot);
        float* const xo = reinterpret_cast<float*>(single ? x_out : states + (size_t)((t + 1) % ring) * slot);
        if (ms) {
            if (int rc = hip_result(nca_launch_dynca_coarse_perceive(xi, pc_scratch, B, C, H, W, pad_mode, st), "dynca coarse perceive")) return rc;
        }
        NcaDyncaArgs a{xi, xo, cond, u_at(u, ubits, t, uslot), w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0 + (uint64_t)t};
        a.pc = ms ? pc_scratch : nullptr;
        a.u_bits = ubits;
        a.dirs = dir.p;
        a.dirs_bstride = dir.Bd == 1 ? 0 : (size_t)2 * H * W;
        if (int rc = hip_result(bf16 ? nca_launch_dynca_step_fwd_bf16(a, st) : nca_launch_dynca_step_fwd(a, st, bf, bfw), what)) return rc;
    }
    return 0;
}

int ncahip_dynca_step_fwd_f32(const float* x_in, float* x_out, const float* cond, const float* u, const float* w1,
                              const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc,
                              int c_cond, int pad_mode, float update_rate, uint64_t seed, uint64_t step,
                              ncahip_stream_t stream) {
    return dynca_fwd_impl(kDyncaFwdF32, "dynca_step_fwd", true, x_in, x_out, 0, 1, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate,
                          seed, step, nullptr, stream);
}
int ncahip_dynca_nsteps_fwd_f32(float* states, int ring, int T, const float* cond, const float* u, const float* w1,
                                const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc,
                                int c_cond, int pad_mode, float update_rate, uint64_t seed, uint64_t step0,
                                ncahip_stream_t stream) {
    return dynca_fwd_impl(kDyncaFwdF32, "dynca_nsteps_fwd", false, states, nullptr, ring, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode,
                          update_rate, seed, step0, nullptr, stream);
}
int ncahip_dynca_step_fwd_ms_f32(const float* x_in, float* x_out, const float* cond, const float* u, const float* w1,
                                 const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc,
                                 int c_cond, int pad_mode, float update_rate, uint64_t seed, uint64_t step, float* pc_scratch,
                                 ncahip_stream_t stream) {
    return dynca_fwd_impl(kDyncaFwdMs, "dynca_step_fwd_ms", true, x_in, x_out, 0, 1, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate,
                          seed, step, pc_scratch, stream);
}
int ncahip_dynca_nsteps_fwd_ms_f32(float* states, int ring, int T, const float* cond, const float* u, const float* w1,
                                   const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc,
                                   int c_cond, int pad_mode, float update_rate, uint64_t seed, uint64_t step0, float* pc_scratch,
                                   ncahip_stream_t stream) {
    return dynca_fwd_impl(kDyncaFwdMs, "dynca_nsteps_fwd_ms", false, states, nullptr, ring, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode,
                          update_rate, seed, step0, pc_scratch, stream);
}
int ncahip_dynca_step_fwd_bf16(const uint16_t* x_in, uint16_t* x_out, const float* cond, const float* u, const float* w1,
                               const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc,
                               int c_cond, int pad_mode, float update_rate, uint64_t seed, uint64_t step,
                               ncahip_stream_t stream) {
    return dynca_fwd_impl(kDyncaFwdBf16, "dynca_step_fwd_bf16", true, x_in, x_out, 0, 1, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate,
                          seed, step, nullptr, stream);
}
int ncahip_dynca_nsteps_fwd_bf16(uint16_t* states, int ring, int T, const float* cond, const float* u, const float* w1,
                                 const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc,
                                 int c_cond, int pad_mode, float update_rate, uint64_t seed, uint64_t step0,
                                 ncahip_stream_t stream) {
    return dynca_fwd_impl(kDyncaFwdBf16, "dynca_nsteps_fwd_bf16", false, states, nullptr, ring, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond,
                          pad_mode, update_rate, seed, step0, nullptr, stream);
}

// ---- T steps in ONE launch for small grids (B = 1 video inference), nca_dynca_persist.hip -------------------------------------
size_t ncahip_dynca_nsteps_persist_workspace(int B, int C, int H, int W, int fc, int c_cond) {
    if (!dims_ok(B, C, H, W) || !nca_dynca_persist_shape_ok(B, C, H, W, fc, c_cond)) return 0;
    // abort word + the exchange: 2 parities x tiles x C x (fine ring cells + coarse means) (value, tag) pairs: sized for the two-scale exchange
    return 256 + align256((size_t)2 * nca_dynca_persist_xch_pairs(B, C, H, W, true) * sizeof(unsigned long long));
}

// The persistent launches take their epoch as a kernel argument: captured into a graph, every replay would run with the captured epoch
// and meet the previous replay's equally tagged pairs.  On a capturing stream the entry points refuse with the code their callers
// already answer with the per-step kernels; the query enqueues nothing.
static int persist_refuse_capture(const char* who, ncahip_stream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (int rc = hip_result(hipStreamIsCapturing((hipStream_t)stream, &cs), "persist (capture status)")) return rc;
    if (cs == hipStreamCaptureStatusNone) return 0;
    return fail(NCAHIP_ERANGE, "%s: the stream is capturing a graph and a persistent launch cannot be captured (its epoch is a kernel argument, "
                "a replay would repeat it); use the per-step entry point", who);
}

static int dynca_persist_impl(bool two_scale, const float* x_in, float* x_out, int T, const float* cond, const float* u, const float* w1,
                                        const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond,
                                        int pad_mode, float update_rate, uint64_t seed, uint64_t step0, void* workspace,
                                        size_t workspace_bytes, unsigned epoch, ncahip_stream_t stream, const NcaDyncaDir* dir_of_caller = nullptr) {
    const NcaDyncaDir dir = dir_of_caller ? *dir_of_caller : nca_dynca_dir_snapshot();   // one read per call
    if (T < 1 || !workspace) return fail(NCAHIP_EINVAL, "dynca nsteps persist: T >= 1 and a workspace required");
    if (epoch < 1 || epoch >= (1u << 20)) return fail(NCAHIP_EINVAL, "dynca nsteps persist: epoch must be in [1, 2^20) (zero the workspace and restart at 1 when it runs out)");
    if (int rc = check_dynca(x_in, x_out, cond, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode)) return rc;   // (refuses x_in == x_out)
    if (two_scale) {
        if (int rc = check_ms_reflect(H, W, pad_mode)) return rc;
    }
    if (int rc = dynca_dir_check(dir, "dynca nsteps persist", B, H, W)) return rc;
    const size_t need = ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, c_cond);
    if (need == 0 || T >= 4096)
        return fail(NCAHIP_ERANGE, "dynca nsteps persist: shape not covered (C <= 16, fc <= 128, H %% 16 == 0, W %% 16 == 0, T < 4096); use ncahip_dynca_nsteps_fwd_f32");
    if (workspace_bytes < need) return fail(NCAHIP_EINVAL, "dynca nsteps persist: workspace too small");
    if ((((uintptr_t)x_in | (uintptr_t)x_out) & 15) != 0) return fail(NCAHIP_ERANGE, "dynca nsteps persist: 16-byte aligned states required");
    if (((uintptr_t)workspace & 255) != 0) return fail(NCAHIP_ERANGE, "dynca nsteps persist: 256-byte aligned workspace required");
    const bool ubits = u_is_bits(u, seed);
    if (int rc = check_bits(ubits, B, H, W, update_rate, true)) return rc;
    if (int rc = device_error_rc("dynca nsteps persist")) return rc;
    if (int rc = persist_refuse_capture("dynca nsteps persist", stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    NcaDyncaPersistArgs a{x_in, x_out, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0,
                          (int*)workspace, epoch, (unsigned long long*)((char*)workspace + 256),
                          nca_dynca_persist_xch_pairs(B, C, H, W, two_scale), nullptr, ubits ? 1 : 0};
    a.dirs = dir.p;
    a.dirs_bstride = dir.Bd == 1 ? 0 : (size_t)2 * H * W;
    bool fits = false;
    const bool bf = dynca_bf16_mfma(C, fc);   // the variant's own instantiation: its own LDS size and co-residency test
    auto launch = [&](const NcaDyncaPersistArgs& pa, hipStream_t ps, bool query_only, bool* f) {
        return two_scale ? nca_launch_dynca_persist_ms(pa, ps, query_only, f, bf) : nca_launch_dynca_persist(pa, ps, query_only, f, bf);
    };
    if (int rc = hip_result(launch(a, st, true, &fits), "dynca nsteps persist (occupancy)")) return rc;
    if (!fits) return fail(NCAHIP_ERANGE, "dynca nsteps persist: %d tiles cannot all be resident on this device; use ncahip_dynca_nsteps_fwd_f32",
                           nca_dynca_persist_tiles(B, H, W));
    return hip_result(launch(a, st, false, &fits), "dynca_nsteps_fwd_persist");     // ONE launch: no copy, no memset
}

int ncahip_dynca_nsteps_fwd_persist_f32(const float* x_in, float* x_out, int T, const float* cond, const float* u, const float* w1,
                                        const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond,
                                        int pad_mode, float update_rate, uint64_t seed, uint64_t step0, void* workspace,
                                        size_t workspace_bytes, unsigned epoch, ncahip_stream_t stream) {
    return dynca_persist_impl(false, x_in, x_out, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0,
                              workspace, workspace_bytes, epoch, stream);
}
int ncahip_dynca_nsteps_fwd_persist_ms_f32(const float* x_in, float* x_out, int T, const float* cond, const float* u, const float* w1,
                                           const float* b1, const float* w2, const float* b2, int B, int C, int H, int W, int fc,
                                           int c_cond, int pad_mode, float update_rate, uint64_t seed, uint64_t step0, void* workspace,
                                           size_t workspace_bytes, unsigned epoch, ncahip_stream_t stream) {
    return dynca_persist_impl(true, x_in, x_out, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0,
                              workspace, workspace_bytes, epoch, stream);
}

// ---- a whole ConditionedNCA grow in ONE launch for small grids, nca_cond_persist.hip -------------------------------------------
size_t ncahip_cond_grow_persist_workspace(int B, int C, int H, int W, int hidden, int goal_ch) {
    if (!dims_ok(B, C, H, W) || !nca_cond_persist_shape_ok(B, C, H, W, hidden, goal_ch)) return 0;
    // abort word + the exchange: 2 parities x tiles x (C state channels + the pre mask) x 156 band cells (value, tag) pairs
    return 256 + align256((size_t)2 * nca_cond_persist_xch_pairs(B, C, H, W) * sizeof(unsigned long long));
}

int ncahip_cond_grow_fwd_persist_f32(float* states, uint8_t* pre, int ring, int T, float* x_final, const float* goal, int goal_ch,
                                     const float* u, const float* wp, const float* w1, const float* b1, const float* w2,
                                     const float* b2, const float* w3, int B, int C, int H, int W, int hidden, int alive_ch,
                                     float alive_thr, float fire_rate, float clamp_lo, float clamp_hi, uint64_t seed, uint64_t step0,
                                     void* workspace, size_t workspace_bytes, unsigned epoch, ncahip_stream_t stream) {
    // host-side checks first: nothing below touches the device before the sticky-word refusal
    if (T < 1 || (ring != 2 && ring != T + 1)) return fail(NCAHIP_EINVAL, "cond grow persist: T >= 1 and ring 2 or T + 1 required");
    if (!states || !x_final || !workspace || (ring == T + 1 && !pre)) return fail(NCAHIP_EINVAL, "cond grow persist: null pointer");
    if (int rc = check_cond(states, x_final, ring == T + 1 ? (const void*)pre : (const void*)x_final, goal, wp, w1, b1, w2, b2, w3, B, C, H,
                            W, hidden, goal_ch, alive_ch, kMaxCCondFwd))
        return rc;
    if (epoch < 1 || epoch >= (1u << 20)) return fail(NCAHIP_EINVAL, "cond grow persist: epoch must be in [1, 2^20) (zero the workspace and restart at 1 when it runs out)");
    const size_t need = ncahip_cond_grow_persist_workspace(B, C, H, W, hidden, goal_ch);
    if (need == 0 || T >= 4096)
        return fail(NCAHIP_ERANGE, "cond grow persist: shape not covered (C <= 20, hidden 64, H %% 16 == 0, W %% 16 == 0, T < 4096); use ncahip_cond_grow_fwd_f32");
    if (workspace_bytes < need) return fail(NCAHIP_EINVAL, "cond grow persist: workspace too small");
    if (((uintptr_t)workspace & 255) != 0) return fail(NCAHIP_ERANGE, "cond grow persist: 256-byte aligned workspace required");
    // the per-step driver runs the producer/consumer family only on 16-byte aligned tensors: anything else is not this path's twin
    if ((((uintptr_t)states | (uintptr_t)x_final | (uintptr_t)goal) & 15) != 0)
        return fail(NCAHIP_ERANGE, "cond grow persist: 16-byte aligned states / x_final / goal required");
    const bool ubits = u_is_bits(u, seed);
    if (u && !ubits) return fail(NCAHIP_ERANGE, "cond grow persist: explicit float uniforms not covered (bit-packed masks or Philox); use ncahip_cond_grow_fwd_f32");
    if (int rc = check_bits(ubits, B, H, W, fire_rate, false)) return rc;
    if (!nca_cond_fwd_default())
        return fail(NCAHIP_ERANGE, "cond grow persist: only the default exact-f32 producer/consumer family has a persistent twin; use ncahip_cond_grow_fwd_f32");
    if (int rc = device_error_rc("cond grow")) return rc;
    if (int rc = persist_refuse_capture("cond grow persist", stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    NcaCondPersistArgs a{states, states, pre, ring == T + 1 ? 1 : 0, x_final, goal, ubits ? u : nullptr, wp, w1, b1, w2, b2, w3,
                         B, C, H, W, goal_ch, alive_ch, T, alive_thr, fire_rate, clamp_lo, clamp_hi, seed, step0, (int*)workspace, epoch,
                         (unsigned long long*)((char*)workspace + 256), nca_cond_persist_xch_pairs(B, C, H, W), nullptr, ubits ? 1 : 0, 0,
                         nullptr};
    bool fits = false;
    if (int rc = hip_result(nca_launch_cond_persist(a, st, true, &fits), "cond grow persist (residency)")) return rc;
    if (!fits) return fail(NCAHIP_ERANGE, "cond grow persist: %d tiles need a CU each on this device; use ncahip_cond_grow_fwd_f32",
                           nca_cond_persist_tiles(B, H, W));
    return hip_result(nca_launch_cond_persist(a, st, false, &fits), "cond_grow_fwd_persist");     // ONE launch: no copy, no memset
}

// ---- conditioning front ends (fixed-filter part of the encoders) ---------------------------------------------------------
int ncahip_image_encoder_front_f32(const float* img, const float* k3, const float* k5, float* feat, int B, int ch, int H, int W,
                                   ncahip_stream_t stream) {
    if (!img || !k3 || !k5 || !feat || img == feat) return fail(NCAHIP_EINVAL, "image_encoder_front: null or aliased pointer");
    if (!dims_ok(B, ch, H, W)) return fail(NCAHIP_EINVAL, "image_encoder_front: bad size");
    if (ch > 8) return fail(NCAHIP_ERANGE, "image_encoder_front: %d image channels (at most 8)", ch);
    return hip_result(nca_launch_image_encoder_front(img, k3, k5, feat, B, ch, H, W, (hipStream_t)stream), "image_encoder_front");
}

int ncahip_edge_extractor_f32(const float* img, const float* k3, float* out, int B, int H, int W, int apply_tanh, ncahip_stream_t stream) {
    if (!img || !k3 || !out || img == out) return fail(NCAHIP_EINVAL, "edge_extractor: null or aliased pointer");
    if (!dims_ok(B, 1, H, W)) return fail(NCAHIP_EINVAL, "edge_extractor: bad size");
    return hip_result(nca_launch_edge_extractor(img, k3, out, B, H, W, apply_tanh != 0, (hipStream_t)stream), "edge_extractor");
}

// ---- a whole clip per call (video_utils.py:50-83): conditioning of every frame, the existing step entry points, image output ----
static bool clip_fmt_ok(int fmt) { return fmt == NCAHIP_CLIP_F32_NCHW || fmt == NCAHIP_CLIP_U8_NHWC; }
static size_t clip_fmt_bytes(int fmt) { return fmt == NCAHIP_CLIP_U8_NHWC ? 1 : sizeof(float); }
static bool clip_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bn && pb < pa + an;
}
// images (never frames) may also leave as planar YUV 4:2:0: the record nca_img_out makes of an image format (nca_kernels.h)
// bytes of one image of B samples: [B,c,H,W] float32, [B,H,W,c] uint8 or [B,3H/2,W] uint8 (c == 3, H and W even: checked before)
static size_t clip_img_bytes(const NcaImgOut& io, int B, int c, int H, int W) {
    return io.planar() ? (size_t)B * H * W / 2 * 3 : (size_t)B * c * H * W * (io.kind == kImgU8 ? 1 : sizeof(float));
}
// what a planar image format adds to an emit's checks: three channels (NCAHIP_EINVAL) and even sides (NCAHIP_ERANGE)
static int check_clip_planar(const char* who, const NcaImgOut& io, int c_out, int H, int W) {
    if (!io.planar()) return 0;
    if (c_out != 3) return fail(NCAHIP_EINVAL, "%s: a planar YUV image is made of 3 channels, got c_out=%d", who, c_out);
    if ((H | W) & 1) return fail(NCAHIP_ERANGE, "%s: 4:2:0 images have even sides, got %d x %d", who, H, W);
    return 0;
}

size_t ncahip_clip_cond_workspace(int F, int B, int H, int W) {
    if (F <= 0 || !dims_ok(B, 3, H, W)) return 0;
    return (size_t)F * B * 3 * H * W * sizeof(float);
}

int ncahip_clip_cond(const void* frames, int frame_fmt, const float* k3, float gray_r, float gray_g, float gray_b, int apply_tanh, float* cond,
                     int F, int B, int H, int W, ncahip_stream_t stream) {
    if (!frames || !k3 || !cond) return fail(NCAHIP_EINVAL, "clip_cond: null pointer");
    if (!clip_fmt_ok(frame_fmt)) return fail(NCAHIP_EINVAL, "clip_cond: unknown frame format %d", frame_fmt);
    if (F <= 0 || !dims_ok(B, 3, H, W) || (size_t)F * B > 0x7fffffffu) return fail(NCAHIP_EINVAL, "clip_cond: bad size");
    const size_t px = (size_t)F * B * 3 * H * W;
    if (clip_overlap(frames, px * clip_fmt_bytes(frame_fmt), cond, px * sizeof(float)) || clip_overlap(k3, 27 * sizeof(float), cond, px * sizeof(float)))
        return fail(NCAHIP_EINVAL, "clip_cond: cond overlaps an input");
    if (frame_fmt == NCAHIP_CLIP_F32_NCHW && ((uintptr_t)frames & 3) != 0) return fail(NCAHIP_EINVAL, "clip_cond: float32 frames must be 4-byte aligned");
    return hip_result(nca_launch_clip_cond(frames, frame_fmt == NCAHIP_CLIP_U8_NHWC, k3, gray_r, gray_g, gray_b, apply_tanh != 0, cond, F * B, H, W,
                                           (hipStream_t)stream), "clip_cond");
}

// the checks of an image out of state[:, :c_out]; *io: the record of img_fmt, for the launcher
static int check_clip_emit(const void* state, const void* img, int img_fmt, NcaImgOut* io, int B, int C, int c_out, int H, int W, bool need_img = true) {
    if (!state || (need_img && !img)) return fail(NCAHIP_EINVAL, "clip emit: null pointer");
    if (!nca_img_out(img_fmt, io)) return fail(NCAHIP_EINVAL, "clip emit: unknown image format %d", img_fmt);
    if (!dims_ok(B, C, H, W)) return fail(NCAHIP_EINVAL, "clip emit: bad size");
    if (c_out < 1 || c_out > 4 || c_out > C) return fail(NCAHIP_EINVAL, "clip emit: c_out=%d must be in 1..4 and at most C=%d", c_out, C);
    if (int rc = check_clip_planar("clip emit", *io, c_out, H, W)) return rc;
    if (io->kind == kImgF32 && ((uintptr_t)img & 3) != 0) return fail(NCAHIP_EINVAL, "clip emit: float32 images must be 4-byte aligned");
    return 0;
}

int ncahip_clip_emit(const float* state, void* img, int img_fmt, int B, int C, int c_out, int H, int W, ncahip_stream_t stream) {
    NcaImgOut io;
    if (int rc = check_clip_emit(state, img, img_fmt, &io, B, C, c_out, H, W)) return rc;
    if (clip_overlap(state, (size_t)B * C * H * W * sizeof(float), img, clip_img_bytes(io, B, c_out, H, W)))
        return fail(NCAHIP_EINVAL, "clip emit: the image overlaps the state");
    // without a grey plane the launcher only reads the state
    return hip_result(nca_launch_clip_emit({const_cast<float*>(state), false, img, io, false, nullptr, B, C, c_out, H, W}, (hipStream_t)stream), "clip_emit");
}

int ncahip_clip_gray(const void* frames, int frame_fmt, float gray_r, float gray_g, float gray_b, float* gray, int F, int B, int H, int W,
                     ncahip_stream_t stream) {
    if (!frames || !gray) return fail(NCAHIP_EINVAL, "clip_gray: null pointer");
    if (!clip_fmt_ok(frame_fmt)) return fail(NCAHIP_EINVAL, "clip_gray: unknown frame format %d", frame_fmt);
    if (F <= 0 || !dims_ok(B, 3, H, W) || (size_t)F * B > 0x7fffffffu) return fail(NCAHIP_EINVAL, "clip_gray: bad size");
    const size_t px = (size_t)F * B * H * W;
    if (clip_overlap(frames, 3 * px * clip_fmt_bytes(frame_fmt), gray, px * sizeof(float))) return fail(NCAHIP_EINVAL, "clip_gray: gray overlaps the frames");
    if (frame_fmt == NCAHIP_CLIP_F32_NCHW && ((uintptr_t)frames & 3) != 0) return fail(NCAHIP_EINVAL, "clip_gray: float32 frames must be 4-byte aligned");
    return hip_result(nca_launch_clip_gray(frames, frame_fmt == NCAHIP_CLIP_U8_NHWC, gray_r, gray_g, gray_b, gray, F * B, H, W, (hipStream_t)stream),
                      "clip_gray");
}

// c_out of a model whose last state channel is the conditioning image: the image never reads that channel
static int check_extra_channel(const char* who, int C, int c_out) {
    if (c_out > C - 1) return fail(NCAHIP_EINVAL, "%s: c_out=%d reaches the extra channel (channel C-1 = %d holds the grey frame: c_out <= C-1)", who, c_out, C - 1);
    return 0;
}

int ncahip_clip_emit_inject(float* state, void* img, int img_fmt, const float* gray, int B, int C, int c_out, int H, int W, ncahip_stream_t stream) {
    if (!img && !gray) return fail(NCAHIP_EINVAL, "clip emit_inject: neither an image nor a grey plane (null pointer for both halves)");
    NcaImgOut io;
    if (int rc = check_clip_emit(state, img, img_fmt, &io, B, C, c_out, H, W, false)) return rc;
    if (int rc = check_extra_channel("clip emit_inject", C, c_out)) return rc;
    const size_t sbytes = (size_t)B * C * H * W * sizeof(float), gbytes = (size_t)B * H * W * sizeof(float);
    const size_t ibytes = clip_img_bytes(io, B, c_out, H, W);
    if ((img && clip_overlap(state, sbytes, img, ibytes)) || (gray && clip_overlap(state, sbytes, gray, gbytes)) ||
        (img && gray && clip_overlap(img, ibytes, gray, gbytes)))
        return fail(NCAHIP_EINVAL, "clip emit_inject: state, image and grey plane must not overlap");
    return hip_result(nca_launch_clip_emit({state, false, img, io, false, gray, B, C, c_out, H, W}, (hipStream_t)stream), "clip_emit_inject");
}

// What every clip driver checks of its counts: F * steps_per_frame calls (*calls) of step_n steps each ...
static int check_clip_counts(const char* who, int F, int steps_per_frame, int step_n, uint64_t* calls) {
    if (F <= 0 || steps_per_frame <= 0 || step_n <= 0) return fail(NCAHIP_EINVAL, "%s: F, steps_per_frame and step_n must be positive", who);
    *calls = (uint64_t)F * (uint64_t)steps_per_frame;
    if (*calls > 0x7fffffffu || *calls * (uint64_t)step_n > 0x7fffffffu) return fail(NCAHIP_EINVAL, "%s: F * steps_per_frame * step_n must stay below 2^31", who);
    return 0;
}
// ... and, behind its overlap test, of the epochs that a persistent workspace hands to those calls
static int check_clip_epochs(const char* who, const void* persist_ws, unsigned epoch0, uint64_t calls) {
    if (persist_ws && (epoch0 < 1 || (uint64_t)epoch0 + calls >= (1u << 20)))
        return fail(NCAHIP_EINVAL, "%s: epochs epoch0 .. epoch0 + F * steps_per_frame must lie in [1, 2^20) (zero the workspace and restart at 1 when they run out)", who);
    return 0;
}

// The body of the two clip drivers.  gray == NULL: ncahip_dynca_clip_f32 (cond [F] maps, one per frame).  gray != NULL:
// ncahip_dynca_clip_xc_f32 (one cond map or none for all frames; gray[f] replaces state channel C-1 before every call).
static int dynca_clip_impl(const char* who, float* states, const float* gray, const float* cond, int c_cond, bool cond_per_frame, void* images,
                           int img_fmt, int F, int steps_per_frame, int step_n, const float* u, const float* w1, const float* b1, const float* w2,
                           const float* b2, int B, int C, int c_out, int H, int W, int fc, int pad_mode, int two_scale, float update_rate,
                           uint64_t seed, uint64_t step0, float* pc_scratch, void* persist_ws, size_t persist_bytes, unsigned epoch0,
                           ncahip_stream_t stream) {
    // host-side checks: nothing is enqueued before all of them have passed
    NcaImgOut io;   // the image record of this call: built once, handed to every emit
    if (int rc = check_clip_emit(states, images, img_fmt, &io, B, C, c_out, H, W)) return rc;
    if (gray) {
        if (int rc = check_extra_channel(who, C, c_out)) return rc;
    }
    uint64_t calls = 0;
    if (int rc = check_clip_counts(who, F, steps_per_frame, step_n, &calls)) return rc;
    const size_t slot = (size_t)B * C * H * W, uslot = (size_t)B * H * W, cslot = (size_t)B * c_cond * H * W;
    const size_t ibytes = clip_img_bytes(io, B, c_out, H, W);
    const size_t sbytes = 2 * slot * sizeof(float), cbytes = (cond_per_frame ? (size_t)F : 1) * cslot * sizeof(float);
    const size_t gbytes = (size_t)F * uslot * sizeof(float);
    if ((cond && clip_overlap(states, sbytes, cond, cbytes)) || clip_overlap(states, sbytes, images, (size_t)calls * ibytes) ||
        (cond && clip_overlap(cond, cbytes, images, (size_t)calls * ibytes)) ||
        (gray && (clip_overlap(states, sbytes, gray, gbytes) || clip_overlap(gray, gbytes, images, (size_t)calls * ibytes) ||
                  (cond && clip_overlap(gray, gbytes, cond, cbytes)))))
        return fail(NCAHIP_EINVAL, "%s: states, %scond and images must not overlap", who, gray ? "gray, " : "");
    if (int rc = check_clip_epochs(who, persist_ws, epoch0, calls)) return rc;
    // the direction field of this call: read once, handed to every step the clip enqueues
    const NcaDyncaDir dir = nca_dynca_dir_snapshot();
    const DyncaFwdKind kind = two_scale ? kDyncaFwdMs : kDyncaFwdF32;
    // the per-step entry point's body with this call's field: (x_in, x_out) a single step, x_out == NULL the ring `states` of 2 slots
    auto steps = [&](const float* x_in, float* x_out, int T, const float* cf, const float* uf, uint64_t s0) {
        return dynca_fwd_impl(kind, who, x_out != nullptr, x_in, x_out, 2, x_out ? 1 : T, cf, uf, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode,
                              update_rate, seed, s0, pc_scratch, stream, &dir);
    };
    // what the per-step entry point refuses for this shape, the clip refuses with its code (T = 0: every check, no launch)
    if (int rc = steps(states, nullptr, 0, cond, u, step0)) return rc;
    if (persist_ws) {
        const size_t need = ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, c_cond);
        if (need != 0 && persist_bytes < need) return fail(NCAHIP_EINVAL, "%s: persistent workspace too small", who);
    }
    if (int rc = device_error_rc(who)) return rc;

    const bool ubits = u_is_bits(u, seed);
    hipStream_t st = (hipStream_t)stream;
    bool persist = persist_ws != nullptr;
    int cur = 0;   // the slot that holds the state
    if (gray) {    // the first frame's grey; every later one goes in with the image of the call before it
        if (int rc = hip_result(nca_launch_clip_emit({states, false, nullptr, io, false, gray, B, C, c_out, H, W}, st), "dynca clip (inject)")) return rc;
    }
    for (int n = 0; n < (int)calls; ++n) {
        const float* const cf = cond_per_frame ? cond + (size_t)(n / steps_per_frame) * cslot : cond;
        const int t0 = n * step_n;                                  // first step of this call within `u`
        const uint64_t s0 = step0 + (uint64_t)t0;
        bool done = false;
        if (persist) {
            const int rc = dynca_persist_impl(two_scale != 0, states + (size_t)cur * slot, states + (size_t)(cur ^ 1) * slot, step_n, cf,
                                              u_at(u, ubits, t0, uslot), w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, s0,
                                              persist_ws, persist_bytes, epoch0 + (unsigned)n, stream, &dir);
            if (rc == 0) {
                cur ^= 1;
                done = true;
            } else if (rc == NCAHIP_ERANGE) {
                persist = false;   // not covered (shape, alignment, residency): this call and the rest run on the per-step kernels
            } else {
                return rc;
            }
        }
        if (!done) {
            int T = step_n, t = t0;
            if (cur == 1) {   // the ring of the n-step entry point starts at slot 0: one single step brings the state there
                if (int rc = steps(states + slot, states, 1, cf, u_at(u, ubits, t, uslot), step0 + (uint64_t)t)) return rc;
                --T, ++t;
            }
            if (int rc = steps(states, nullptr, T, cf, u_at(u, ubits, t, uslot), step0 + (uint64_t)t)) return rc;
            cur = T & 1;
        }
        // image n and, in the same launch, the grey of the call that follows (the repeats j > 0 of a frame included: the channel has
        // evolved); after the last call the channel stays as the steps left it
        const float* const gnext = gray && n + 1 < (int)calls ? gray + (size_t)((n + 1) / steps_per_frame) * uslot : nullptr;
        const NcaClipEmitArgs e{states + (size_t)cur * slot, false, (char*)images + (size_t)n * ibytes, io, false, gnext, B, C, c_out, H, W};
        if (int rc = hip_result(nca_launch_clip_emit(e, st), "dynca clip (emit)")) return rc;
    }
    if (cur == 1)   // the state returns in slot 0
        return hip_result(hipMemcpyAsync(states, states + slot, slot * sizeof(float), hipMemcpyDeviceToDevice, st), "dynca clip (state copy)");
    return 0;
}

int ncahip_dynca_clip_f32(float* states, const float* cond, void* images, int img_fmt, int F, int steps_per_frame, int step_n, const float* u,
                          const float* w1, const float* b1, const float* w2, const float* b2, int B, int C, int c_out, int H, int W, int fc,
                          int pad_mode, int two_scale, float update_rate, uint64_t seed, uint64_t step0, float* pc_scratch, void* persist_ws,
                          size_t persist_bytes, unsigned epoch0, ncahip_stream_t stream) {
    if (!cond) return fail(NCAHIP_EINVAL, "dynca clip: null pointer");
    return dynca_clip_impl("dynca clip", states, nullptr, cond, 3, true, images, img_fmt, F, steps_per_frame, step_n, u, w1, b1, w2, b2, B, C, c_out, H, W,
                           fc, pad_mode, two_scale, update_rate, seed, step0, pc_scratch, persist_ws, persist_bytes, epoch0, stream);
}

int ncahip_dynca_clip_xc_f32(float* states, const float* gray, const float* cond, int c_cond, void* images, int img_fmt, int F, int steps_per_frame,
                             int step_n, const float* u, const float* w1, const float* b1, const float* w2, const float* b2, int B, int C, int c_out,
                             int H, int W, int fc, int pad_mode, int two_scale, float update_rate, uint64_t seed, uint64_t step0, float* pc_scratch,
                             void* persist_ws, size_t persist_bytes, unsigned epoch0, ncahip_stream_t stream) {
    if (!gray) return fail(NCAHIP_EINVAL, "dynca clip xc: null pointer");
    if (c_cond != 0 && c_cond != 2) return fail(NCAHIP_EINVAL, "dynca clip xc: c_cond=%d must be 0 (no cond map) or 2 (CPE)", c_cond);
    if ((c_cond == 2) != (cond != nullptr)) return fail(NCAHIP_EINVAL, "dynca clip xc: cond pointer / c_cond mismatch");
    return dynca_clip_impl("dynca clip xc", states, gray, cond, c_cond, false, images, img_fmt, F, steps_per_frame, step_n, u, w1, b1, w2, b2, B, C, c_out,
                           H, W, fc, pad_mode, two_scale, update_rate, seed, step0, pc_scratch, persist_ws, persist_bytes, epoch0, stream);
}

// ---- the ConditionedNCA forward: shared bodies for fp32 and bf16 state storage (nca_cond_bf16.hip: bf16 state and goal, bf16 MFMA) ----
static int check_bf16_shape(const void* x_in, const void* x_out, const void* goal, int H, int W) {
    if (W % 4 != 0 || (((uintptr_t)x_in | (uintptr_t)x_out | (uintptr_t)goal) & 7) != 0)
        return fail(NCAHIP_ERANGE, "bf16 cond step: needs W %% 4 == 0 and 8-byte aligned state / goal tensors");
    if ((size_t)H * W >= ((size_t)1 << 24)) return fail(NCAHIP_ERANGE, "bf16 cond step: H*W must be below 2^24");
    return 0;
}

static int cond_step_fwd_impl(bool bf16, const void* x_in, const uint8_t* pre_in, void* x_out, uint8_t* pre_out, const void* goal, int goal_ch,
                              const float* u, const float* wp, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                              int B, int C, int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                              float clamp_hi, uint64_t seed, uint64_t step, ncahip_stream_t stream) {
    if (int rc = check_cond(x_in, x_out, pre_out, goal, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, goal_ch, alive_ch,
                            bf16 ? kMaxCCondFwdBf16 : kMaxCCondFwd))
        return rc;
    if (bf16) {
        if (int rc = check_bf16_shape(x_in, x_out, goal, H, W)) return rc;
    }
    if (pre_in && pre_in == pre_out) return fail(NCAHIP_EINVAL, "cond step: pre_in and pre_out must not alias");
    NcaCondArgs a{reinterpret_cast<const float*>(x_in), pre_in, reinterpret_cast<float*>(x_out), pre_out,
                  reinterpret_cast<const float*>(goal), u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, goal_ch,
                  alive_ch, alive_thr, fire_rate, clamp_lo, clamp_hi, seed, step};
    if (int rc = check_bits(u_is_bits(u, seed), B, H, W, fire_rate, false)) return rc;
    a.u_bits = u_is_bits(u, seed);
    return bf16 ? hip_result(nca_launch_cond_step_fwd_bf16(a, (hipStream_t)stream), "cond_step_fwd_bf16")
                : hip_result(nca_launch_cond_step_fwd(a, (hipStream_t)stream), "cond_step_fwd");
}

static int cond_finalize_impl(bool bf16, const void* x_pend, const uint8_t* pre, void* x_out, int B, int C, int H, int W, int alive_ch,
                              float alive_thr, float clamp_lo, float clamp_hi, ncahip_stream_t stream) {
    if (!x_pend || !x_out || (alive_ch >= 0 && !pre)) return fail(NCAHIP_EINVAL, "cond_finalize: null pointer");
    if (!dims_ok(B, C, H, W) || alive_ch >= C) return fail(NCAHIP_EINVAL, "cond_finalize: bad size");
    if (alive_ch >= 0 && x_pend == x_out) return fail(NCAHIP_EINVAL, "cond_finalize: in-place needs alive_ch < 0");
    hipStream_t st = (hipStream_t)stream;
    return bf16 ? hip_result(nca_launch_cond_finalize_bf16((const uint16_t*)x_pend, pre, (uint16_t*)x_out, B, C, H, W, alive_ch, alive_thr, clamp_lo,
                                                           clamp_hi, st), "cond_finalize_bf16")
                : hip_result(nca_launch_cond_finalize((const float*)x_pend, pre, (float*)x_out, B, C, H, W, alive_ch, alive_thr, clamp_lo, clamp_hi, st),
                             "cond_finalize");
}

// ---- fire words: a grow's fire masks drawn before its steps (nca_cond_fire.hip) ---------------------------------------------------
int ncahip_cond_fire_words(uint64_t* words, int Tc, int B, int H, int W, float fire_rate, uint64_t seed, uint64_t step0,
                           ncahip_stream_t stream) {
    if (!words) return fail(NCAHIP_EINVAL, "cond_fire_words: null pointer");
    if (Tc < 1 || !dims_ok(B, 1, H, W)) return fail(NCAHIP_EINVAL, "cond_fire_words: Tc=%d B=%d H=%d W=%d must all be positive", Tc, B, H, W);
    if (W % 16 != 0 || H % 4 != 0) return fail(NCAHIP_ERANGE, "cond_fire_words: one word per 4 x 16 tile needs H %% 4 == 0 and W %% 16 == 0 (H=%d W=%d)", H, W);
    if (Tc > 65535) return fail(NCAHIP_ERANGE, "cond_fire_words: at most 65535 steps per call (Tc=%d)", Tc);
    if ((size_t)B * (H / 4) * (W / 16) > ((size_t)1 << 31)) return fail(NCAHIP_ERANGE, "cond_fire_words: more than 2^31 tiles per step");
    if (((uintptr_t)words & 7) != 0) return fail(NCAHIP_ERANGE, "cond_fire_words: 8-byte aligned words required");
    return hip_result(nca_launch_cond_fire_words(reinterpret_cast<unsigned long long*>(words), Tc, B, H, W, fire_rate, seed, step0, (hipStream_t)stream), "cond_fire_words");
}

// fire-word launches of the last ncahip_cond_grow_fwd_f32 that enqueued all its steps (0: its steps drew their masks themselves)
static std::atomic<int> g_fire_word_launches{0};
int ncahip_debug_fire_word_launches(void) { return g_fire_word_launches.load(std::memory_order_relaxed); }
// fused-steps launches (several steps per launch, nca_cond_pc.hip MS) of the last ncahip_cond_grow_fwd_f32 that enqueued all its steps
static std::atomic<int> g_fused_step_launches{0};
int ncahip_debug_fused_step_launches(void) { return g_fused_step_launches.load(std::memory_order_relaxed); }
// Shortest grow that draws its masks beforehand.  One fire-word launch has to be bought back by the steps it serves, and what a step
// saves grows with the tiles a wave pair stages in it: rounds = super-tiles per workgroup of the step launch.  Measured with the grow
// timed both ways over a ladder of T (tools/fire_words_cost.py, profiles/r8a_fire_words_cost.jsonl: launch cost / saving per step,
// the line through the ladder) at B x 16 x 256^2 on 256 CUs, where rounds = B:
//   rounds 8: 3.34 us / 0.709 us -> break-even  4.7 steps = 38 step-rounds        rounds 2: 5.23 / 0.196 -> 26.7 steps = 53
//   rounds 4: 4.55 us / 0.416 us -> break-even 10.9 steps = 44 step-rounds        rounds 1: 4.87 / 0.047 -> 104 steps: no gain to speak of
// (rounds 8: the step kernel's 1.3 us, r8a_kernel_stats.txt against r8a_base_kernel_stats.txt, less the 0.32 us per step the fire-word
// kernel runs for).  With one round per workgroup nothing is saved, and 8 x 20 x 64^2 and 1 x 20 x 256^2 lost 2 - 3 % over T = 64
// (tools/bench_paths.py cond_small_persist on the first build, which drew beforehand from T = 10 on at every size: the scalar load
// sits in the cold first tile).  So: at least two rounds, and T x rounds at least twice the largest break-even measured there, 2 x 53.
// A chunk cap (ncahip_debug_force_generic bits 16-23) waives both: the tests reach the path on small grids and at small T that way.
constexpr int kFireWordsMinRounds = 2, kFireWordsMinStepRounds = 106;
static bool fire_words_pay(int T, int B, int H, int W) {
    const long nst = (long)B * ((W + 15) / 16) * ((H + 15) / 16), cus = nca_cu_count();
    const long nwg = nst < cus ? nst : cus, rounds = (nst + nwg - 1) / nwg;   // as launch_cond_pc walks them (nca_cond_pc.hip)
    return rounds >= kFireWordsMinRounds && (long)T * rounds >= kFireWordsMinStepRounds;
}
// x_final can serve as the fire-word scratch: its bytes touch nothing a step reads or writes
static bool fire_scratch_free(const void* x_final, size_t bytes, const void* states, size_t sbytes, const void* pre, size_t pbytes, const void* goal,
                              size_t gbytes, const float* wp, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                              int C, int hidden) {
    const size_t f = sizeof(float);
    return !clip_overlap(x_final, bytes, states, sbytes) && !clip_overlap(x_final, bytes, pre, pbytes) &&
           !(goal && clip_overlap(x_final, bytes, goal, gbytes)) && !clip_overlap(x_final, bytes, wp, (size_t)3 * C * 9 * f) &&
           !clip_overlap(x_final, bytes, w1, (size_t)hidden * 3 * C * f) && !clip_overlap(x_final, bytes, b1, hidden * f) &&
           !clip_overlap(x_final, bytes, w2, (size_t)hidden * hidden * f) && !clip_overlap(x_final, bytes, b2, hidden * f) &&
           !clip_overlap(x_final, bytes, w3, (size_t)C * hidden * f);
}

// Where the fused-steps path keeps its per-tile step counters: x_final holds the fire words of a chunk of steps, [chunk][B*H*W/64] 64-bit
// words, and behind them B * H/4 * W/16 counters + the abort word (nca_cond_ms_done_bytes).  chunk = as many steps as fit beside the
// counters, at most 32 C (what the words alone allow) and at most chunk_cap (0: no cap).  Host only.
int ncahip_cond_fused_steps_layout(int B, int C, int H, int W, int chunk_cap, int* chunk, uint64_t* done_offset, uint64_t* done_bytes) {
    if (!chunk || !done_offset || !done_bytes) return fail(NCAHIP_EINVAL, "cond_fused_steps_layout: null pointer");
    if (!dims_ok(B, C, H, W) || chunk_cap < 0)
        return fail(NCAHIP_EINVAL, "cond_fused_steps_layout: B=%d C=%d H=%d W=%d must all be positive, chunk_cap=%d not negative", B, C, H, W, chunk_cap);
    if (W % 16 != 0 || H % 4 != 0) return fail(NCAHIP_ERANGE, "cond_fused_steps_layout: one counter per 4 x 16 tile needs H %% 4 == 0 and W %% 16 == 0 (H=%d W=%d)", H, W);
    if ((size_t)B * (H / 4) * (W / 16) > ((size_t)1 << 31)) return fail(NCAHIP_ERANGE, "cond_fused_steps_layout: more than 2^31 tiles per step");
    const size_t pslot = (size_t)B * H * W, slot = pslot * C * sizeof(float), words_bytes = pslot / 8, db = nca_cond_ms_done_bytes(B, H, W);
    if (slot < db + words_bytes) return fail(NCAHIP_ERANGE, "cond_fused_steps_layout: x_final has no room for one step's words and the counters");
    size_t n = (slot - db) / words_bytes;
    if (n > (size_t)32 * C) n = (size_t)32 * C;
    if (chunk_cap > 0 && n > (size_t)chunk_cap) n = (size_t)chunk_cap;
    *chunk = (int)n;
    *done_offset = n * words_bytes;
    *done_bytes = db;
    return 0;
}

// img (bf16 only; the clip driver): the grow's last launch also writes the unit image *io of x_final (checked by the caller)
static int cond_grow_fwd_impl(bool bf16, void* states_v, uint8_t* pre, int ring, int T, void* x_final, const void* goal, int goal_ch, const float* u,
                              const float* wp, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, int B, int C,
                              int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo, float clamp_hi,
                              uint64_t seed, uint64_t step0, ncahip_stream_t stream, void* img = nullptr, const NcaImgOut* io = nullptr) {
    char* const states = (char*)states_v;
    if (ring < 2 || T < 1 || !pre || !x_final) return fail(NCAHIP_EINVAL, "cond grow: ring >= 2, T >= 1, buffers required");
    if (int rc = check_cond(states, states + 1, pre, goal, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, goal_ch, alive_ch,
                            bf16 ? kMaxCCondFwdBf16 : kMaxCCondFwd))
        return rc;
    if (bf16) {
        if (int rc = check_bf16_shape(states, states, goal, H, W)) return rc;
    }
    if (int rc = device_error_rc(bf16 ? "cond grow (bf16)" : "cond grow")) return rc;
    const bool ubits = u_is_bits(u, seed);
    if (int rc = check_bits(ubits, B, H, W, fire_rate, false)) return rc;
    const size_t slot = (size_t)B * C * H * W * (bf16 ? sizeof(uint16_t) : sizeof(float)), pslot = (size_t)B * H * W;   // slot: bytes
    if (bf16 && slot % 8 != 0) return fail(NCAHIP_ERANGE, "bf16 cond grow: state slots must stay 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int sl = T % ring;
    if (x_final == states + (size_t)sl * slot && alive_ch >= 0)
        return fail(NCAHIP_EINVAL, "cond grow: x_final must not alias the last state slot");
    auto step_args = [&](int t) {
        const int si = t % ring, so = (t + 1) % ring;
        NcaCondArgs a{reinterpret_cast<const float*>(states + (size_t)si * slot), t == 0 ? nullptr : pre + (size_t)si * pslot,
                      reinterpret_cast<float*>(states + (size_t)so * slot), pre + (size_t)so * pslot,
                      reinterpret_cast<const float*>(goal), u_at(u, ubits, t, pslot), wp, w1, b1, w2, b2, w3, B, C, H,
                      W, hidden, goal_ch, alive_ch, alive_thr, fire_rate, clamp_lo, clamp_hi, seed, step0 + (uint64_t)t};
        a.u_bits = ubits;
        return a;
    };
    // Fire words (fp32, in-kernel Philox, the default producer/consumer kernels, whole 4 x 16 tiles): the masks of a chunk of steps
    // are drawn by one launch of nca_cond_fire.hip into x_final, which is dead until the finalize below writes it, and each step
    // reads its words instead of drawing.  Same stream, same predicate: the same bits as the steps would draw.
    unsigned long long* const fw_scratch = reinterpret_cast<unsigned long long*>(x_final);
    const size_t fw_step = pslot / 64;   // words per step
    int fw_chunk = 0;                    // steps per fire-word launch; 0: the steps draw their masks themselves
    const int fw_cap = nca_modes().fire_words_cap;   // test hook: steps per fire-word launch; set, it also waives fire_words_pay
    if (!bf16 && !u && !nca_modes().no_fire_words && (fw_cap > 0 || fire_words_pay(T, B, H, W))) {
        NcaCondArgs a0 = step_args(0);
        a0.fire_words = fw_scratch;
        // every slot is aligned as slots 0 and 1 are (W % 16 == 0 makes the slot size a multiple of 64 bytes)
        if (nca_cond_fire_words_ok(a0) &&
            fire_scratch_free(x_final, slot, states, (size_t)ring * slot, pre, (size_t)ring * pslot, goal, (size_t)B * goal_ch * H * W * sizeof(float), wp,
                              w1, b1, w2, b2, w3, C, hidden)) {
            fw_chunk = 32 * C;   // slot bytes / (B*H*W / 8 bytes of words per step)
            if (fw_cap > 0 && fw_chunk > fw_cap) fw_chunk = fw_cap;
        }
    }
    // Fused steps (nca_cond_pc.hip, the MS kernels): where the steps read fire words AND the narrow-carve producer/consumer kernel walks at
    // least two rounds per workgroup, a chunk's steps go out as ONE launch; tiles of step t + 1 wait for their 3 x 3 tile neighbourhood of
    // step t through one counter per 4 x 16 tile.  The counters (and the abort word) live in x_final behind the chunk's words, so the
    // chunk shrinks until both fit the slot; the grow's first fire-word launch zeroes them, later chunks count on.  Everything that keeps
    // a grow off the fire words keeps it off this path; hook bit 24 switches it off, bits 25-27 cap the steps per launch.
    unsigned* ms_done = nullptr;
    if (fw_chunk > 0) {
        NcaCondArgs a0 = step_args(0);
        a0.fire_words = fw_scratch;
        int chunk = 0;
        uint64_t done_off = 0, done_bytes = 0;
        if (nca_cond_pc_fused_steps_ok(a0) && ncahip_cond_fused_steps_layout(B, C, H, W, fw_chunk, &chunk, &done_off, &done_bytes) == 0) {
            fw_chunk = chunk;
            ms_done = reinterpret_cast<unsigned*>(static_cast<char*>(x_final) + done_off);
        }
    }
    const int ms_cap = nca_modes().fused_steps_cap;   // test hook: steps per fused launch
    int fw_launches = 0, fw_left = 0, ms_launches = 0;
    const unsigned long long* fw = nullptr;
    for (int t = 0; t < T; ++t) {
        NcaCondArgs a = step_args(t);
        if (fw_chunk > 0) {
            if (fw_left == 0) {
                fw_left = T - t < fw_chunk ? T - t : fw_chunk;
                if (int rc = hip_result(nca_launch_cond_fire_words(fw_scratch, fw_left, B, H, W, fire_rate, seed, step0 + (uint64_t)t, st,
                                                                   t == 0 ? ms_done : nullptr), "cond_grow fire words"))
                    return rc;
                fw = fw_scratch;
                ++fw_launches;
            }
            a.fire_words = fw;
            if (ms_done) {
                const int n = ms_cap > 0 && fw_left > ms_cap ? ms_cap : fw_left;
                a.ms_steps = n;
                a.ms_t0 = t;
                a.ms_ring = ring;
                a.ms_states = states;
                a.ms_pre = pre;
                a.ms_done = ms_done;
                if (int rc = hip_result(nca_launch_cond_steps_fwd_pc(a, st), "cond_grow_fwd (fused steps)")) return rc;
                fw += (size_t)n * fw_step;
                fw_left -= n;
                t += n - 1;
                ++ms_launches;
                continue;
            }
            fw += fw_step;
            --fw_left;
        }
        if (int rc = bf16 ? hip_result(nca_launch_cond_step_fwd_bf16(a, st), "cond_grow_fwd_bf16") : hip_result(nca_launch_cond_step_fwd(a, st), "cond_grow_fwd"))
            return rc;
    }
    if (!bf16) {
        g_fire_word_launches.store(fw_launches, std::memory_order_relaxed);
        g_fused_step_launches.store(ms_launches, std::memory_order_relaxed);
    }
    const uint8_t* const pre_last = pre + (size_t)sl * pslot;
    if (bf16 && img)
        return hip_result(nca_launch_cond_finalize_emit_bf16((const uint16_t*)(states + (size_t)sl * slot), pre_last, (uint16_t*)x_final, img, *io, B, C, H, W,
                                                             alive_ch, alive_thr, clamp_lo, clamp_hi, st), "cond_grow finalize + image (bf16)");
    return bf16 ? hip_result(nca_launch_cond_finalize_bf16((const uint16_t*)(states + (size_t)sl * slot), pre_last, (uint16_t*)x_final, B, C, H, W, alive_ch,
                                                           alive_thr, clamp_lo, clamp_hi, st), "cond_grow finalize (bf16)")
                : hip_result(nca_launch_cond_finalize((const float*)(states + (size_t)sl * slot), pre_last, (float*)x_final, B, C, H, W, alive_ch, alive_thr,
                                                      clamp_lo, clamp_hi, st), "cond_grow finalize");
}

int ncahip_cond_step_fwd_f32(const float* x_in, const uint8_t* pre_in, float* x_out, uint8_t* pre_out,
                             const float* goal, int goal_ch, const float* u, const float* wp, const float* w1,
                             const float* b1, const float* w2, const float* b2, const float* w3, int B, int C, int H,
                             int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                             float clamp_hi, uint64_t seed, uint64_t step, ncahip_stream_t stream) {
    return cond_step_fwd_impl(false, x_in, pre_in, x_out, pre_out, goal, goal_ch, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, alive_ch, alive_thr,
                              fire_rate, clamp_lo, clamp_hi, seed, step, stream);
}
int ncahip_cond_step_fwd_bf16(const uint16_t* x_in, const uint8_t* pre_in, uint16_t* x_out, uint8_t* pre_out,
                              const uint16_t* goal, int goal_ch, const float* u, const float* wp, const float* w1,
                              const float* b1, const float* w2, const float* b2, const float* w3, int B, int C, int H,
                              int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                              float clamp_hi, uint64_t seed, uint64_t step, ncahip_stream_t stream) {
    return cond_step_fwd_impl(true, x_in, pre_in, x_out, pre_out, goal, goal_ch, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, alive_ch, alive_thr,
                              fire_rate, clamp_lo, clamp_hi, seed, step, stream);
}
int ncahip_cond_finalize_f32(const float* x_pend, const uint8_t* pre, float* x_out, int B, int C, int H, int W,
                             int alive_ch, float alive_thr, float clamp_lo, float clamp_hi, ncahip_stream_t stream) {
    return cond_finalize_impl(false, x_pend, pre, x_out, B, C, H, W, alive_ch, alive_thr, clamp_lo, clamp_hi, stream);
}
int ncahip_cond_finalize_bf16(const uint16_t* x_pend, const uint8_t* pre, uint16_t* x_out, int B, int C, int H, int W,
                              int alive_ch, float alive_thr, float clamp_lo, float clamp_hi, ncahip_stream_t stream) {
    return cond_finalize_impl(true, x_pend, pre, x_out, B, C, H, W, alive_ch, alive_thr, clamp_lo, clamp_hi, stream);
}
int ncahip_cond_grow_fwd_f32(float* states, uint8_t* pre, int ring, int T, float* x_final, const float* goal,
                             int goal_ch, const float* u, const float* wp, const float* w1, const float* b1,
                             const float* w2, const float* b2, const float* w3, int B, int C, int H, int W, int hidden,
                             int alive_ch, float alive_thr, float fire_rate, float clamp_lo, float clamp_hi,
                             uint64_t seed, uint64_t step0, ncahip_stream_t stream) {
    return cond_grow_fwd_impl(false, states, pre, ring, T, x_final, goal, goal_ch, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, alive_ch, alive_thr,
                              fire_rate, clamp_lo, clamp_hi, seed, step0, stream);
}
int ncahip_cond_grow_fwd_bf16(uint16_t* states, uint8_t* pre, int ring, int T, uint16_t* x_final, const uint16_t* goal,
                              int goal_ch, const float* u, const float* wp, const float* w1, const float* b1,
                              const float* w2, const float* b2, const float* w3, int B, int C, int H, int W, int hidden,
                              int alive_ch, float alive_thr, float fire_rate, float clamp_lo, float clamp_hi,
                              uint64_t seed, uint64_t step0, ncahip_stream_t stream) {
    return cond_grow_fwd_impl(true, states, pre, ring, T, x_final, goal, goal_ch, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, alive_ch, alive_thr,
                              fire_rate, clamp_lo, clamp_hi, seed, step0, stream);
}

int ncahip_cond_alive_u8(const float* x, uint8_t* out, int B, int C, int H, int W, int alive_ch, float alive_thr,
                         ncahip_stream_t stream) {
    if (!x || !out) return fail(NCAHIP_EINVAL, "cond_alive: null pointer");
    if (!dims_ok(B, C, H, W) || alive_ch >= C) return fail(NCAHIP_EINVAL, "cond_alive: bad size");
    return hip_result(nca_launch_cond_alive(x, out, B, C, H, W, alive_ch, alive_thr, (hipStream_t)stream), "cond_alive");
}

// ---- a whole clip per call, ConditionedNCA (EncoderConditioning/visualisation.ipynb: the goal switched while the state runs) ----------
size_t ncahip_clip_encode_workspace(int F, int B, int E, int H, int W) {
    if (F <= 0 || !dims_ok(B, E, H, W)) return 0;
    return (size_t)F * B * E * H * W * sizeof(float);
}

// the two goal types share every check; a bf16 goal has half the bytes and is 2-byte aligned
static int clip_encode_impl(bool bf16, const void* frames, int frame_fmt, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2,
                            void* goal, int F, int B, int ch, int E, int H, int W, ncahip_stream_t stream) {
    if (!frames || !k3 || !k5 || !w1 || !b1 || !w2 || !goal) return fail(NCAHIP_EINVAL, "clip_encode: null pointer");
    if (!clip_fmt_ok(frame_fmt)) return fail(NCAHIP_EINVAL, "clip_encode: unknown frame format %d", frame_fmt);
    if (F <= 0 || ch <= 0 || E <= 0 || !dims_ok(B, 1, H, W) || (size_t)F * B > 0x7fffffffu) return fail(NCAHIP_EINVAL, "clip_encode: bad size");
    if (ch > 4 || E > 32) return fail(NCAHIP_ERANGE, "clip_encode: ch=%d E=%d exceeds (4, 32)", ch, E);
    if (frame_fmt == NCAHIP_CLIP_U8_NHWC && ch != 3) return fail(NCAHIP_ERANGE, "clip_encode: uint8 frames have 3 channels, got ch=%d", ch);
    const size_t px = (size_t)F * B * H * W;
    if ((size_t)F * B * ((H + 15) / 16) * ((W + 15) / 16) > 0x7fffffffu) return fail(NCAHIP_ERANGE, "clip_encode: more than 2^31 tiles of 16 x 16 in one launch");
    const size_t gbytes = px * E * (bf16 ? sizeof(uint16_t) : sizeof(float)), fbytes = px * ch * clip_fmt_bytes(frame_fmt);
    const size_t k1 = (size_t)(3 + ch);
    if (clip_overlap(frames, fbytes, goal, gbytes) || clip_overlap(k3, 27 * sizeof(float), goal, gbytes) || clip_overlap(k5, 25 * sizeof(float), goal, gbytes) ||
        clip_overlap(w1, E * k1 * 9 * sizeof(float), goal, gbytes) || clip_overlap(b1, E * sizeof(float), goal, gbytes) ||
        clip_overlap(w2, (size_t)E * E * 9 * sizeof(float), goal, gbytes))
        return fail(NCAHIP_EINVAL, "clip_encode: goal overlaps an input");
    if (frame_fmt == NCAHIP_CLIP_F32_NCHW && ((uintptr_t)frames & 3) != 0) return fail(NCAHIP_EINVAL, "clip_encode: float32 frames must be 4-byte aligned");
    if (bf16 && ((uintptr_t)goal & 1) != 0) return fail(NCAHIP_EINVAL, "clip_encode: a bf16 goal must be 2-byte aligned");
    const bool u8 = frame_fmt == NCAHIP_CLIP_U8_NHWC;
    return bf16 ? hip_result(nca_launch_clip_encode_bf16(frames, u8, k3, k5, w1, b1, w2, (uint16_t*)goal, F * B, ch, E, H, W, (hipStream_t)stream), "clip_encode_bf16")
                : hip_result(nca_launch_clip_encode(frames, u8, k3, k5, w1, b1, w2, (float*)goal, F * B, ch, E, H, W, (hipStream_t)stream), "clip_encode");
}

int ncahip_clip_encode(const void* frames, int frame_fmt, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2,
                       float* goal, int F, int B, int ch, int E, int H, int W, ncahip_stream_t stream) {
    return clip_encode_impl(false, frames, frame_fmt, k3, k5, w1, b1, w2, goal, F, B, ch, E, H, W, stream);
}
int ncahip_clip_encode_bf16(const void* frames, int frame_fmt, const float* k3, const float* k5, const float* w1, const float* b1, const float* w2,
                            uint16_t* goal, int F, int B, int ch, int E, int H, int W, ncahip_stream_t stream) {
    return clip_encode_impl(true, frames, frame_fmt, k3, k5, w1, b1, w2, goal, F, B, ch, E, H, W, stream);
}

static int check_clip_emit_unit(const void* state, const void* img, int img_fmt, NcaImgOut* io, int B, int C, int H, int W) {
    if (!state || !img) return fail(NCAHIP_EINVAL, "clip emit_unit: null pointer");
    if (!nca_img_out(img_fmt, io)) return fail(NCAHIP_EINVAL, "clip emit_unit: unknown image format %d", img_fmt);
    if (!dims_ok(B, C, H, W)) return fail(NCAHIP_EINVAL, "clip emit_unit: bad size");
    if (C < 3) return fail(NCAHIP_EINVAL, "clip emit_unit: the image is state[:, :3], C=%d has fewer than 3 channels", C);
    if (int rc = check_clip_planar("clip emit_unit", *io, 3, H, W)) return rc;
    if (io->kind == kImgF32 && ((uintptr_t)img & 3) != 0) return fail(NCAHIP_EINVAL, "clip emit_unit: float32 images must be 4-byte aligned");
    return 0;
}

// the two state types share every check; a state stored as bf16 has half the bytes and is 2-byte aligned
static int clip_emit_unit_impl(bool bf16, const void* state, void* img, int img_fmt, int B, int C, int H, int W, ncahip_stream_t stream) {
    NcaImgOut io;
    if (int rc = check_clip_emit_unit(state, img, img_fmt, &io, B, C, H, W)) return rc;
    if (bf16 && ((uintptr_t)state & 1) != 0) return fail(NCAHIP_EINVAL, "clip emit_unit: a bf16 state must be 2-byte aligned");
    if (clip_overlap(state, (size_t)B * C * H * W * (bf16 ? sizeof(uint16_t) : sizeof(float)), img, clip_img_bytes(io, B, 3, H, W)))
        return fail(NCAHIP_EINVAL, "clip emit_unit: the image overlaps the state");
    return hip_result(nca_launch_clip_emit({const_cast<void*>(state), bf16, img, io, true, nullptr, B, C, 3, H, W}, (hipStream_t)stream),
                      bf16 ? "clip_emit_unit_bf16" : "clip_emit_unit");
}

int ncahip_clip_emit_unit(const float* state, void* img, int img_fmt, int B, int C, int H, int W, ncahip_stream_t stream) {
    return clip_emit_unit_impl(false, state, img, img_fmt, B, C, H, W, stream);
}
int ncahip_clip_emit_unit_bf16(const uint16_t* state, void* img, int img_fmt, int B, int C, int H, int W, ncahip_stream_t stream) {
    return clip_emit_unit_impl(true, state, img, img_fmt, B, C, H, W, stream);
}

int ncahip_cond_finalize_emit_bf16(const uint16_t* x_pend, const uint8_t* pre, uint16_t* x_out, void* img, int img_fmt, int B, int C, int H, int W,
                                   int alive_ch, float alive_thr, float clamp_lo, float clamp_hi, ncahip_stream_t stream) {
    const char* const who = "cond_finalize_emit";
    NcaImgOut io;
    if (!x_pend || !x_out || !img || (alive_ch >= 0 && !pre)) return fail(NCAHIP_EINVAL, "%s: null pointer", who);
    if (int rc = check_clip_emit_unit(x_pend, img, img_fmt, &io, B, C, H, W)) return rc;
    if (alive_ch >= C) return fail(NCAHIP_EINVAL, "%s: bad size (alive_ch=%d outside C=%d)", who, alive_ch, C);
    if (alive_ch >= 0 && x_pend == x_out) return fail(NCAHIP_EINVAL, "%s: in-place needs alive_ch < 0", who);
    if ((((uintptr_t)x_pend | (uintptr_t)x_out) & 1) != 0) return fail(NCAHIP_EINVAL, "%s: bf16 states must be 2-byte aligned", who);
    const size_t sbytes = (size_t)B * C * H * W * sizeof(uint16_t), ibytes = clip_img_bytes(io, B, 3, H, W);
    if (clip_overlap(img, ibytes, x_pend, sbytes) || clip_overlap(img, ibytes, x_out, sbytes) || (pre && clip_overlap(img, ibytes, pre, (size_t)B * H * W)) ||
        (pre && clip_overlap(x_out, sbytes, pre, (size_t)B * H * W)))
        return fail(NCAHIP_EINVAL, "%s: the image must not overlap x_pend, x_out or pre, and x_out must not overlap pre", who);
    return hip_result(nca_launch_cond_finalize_emit_bf16(x_pend, pre, x_out, img, io, B, C, H, W, alive_ch, alive_thr, clamp_lo, clamp_hi, (hipStream_t)stream),
                      "cond_finalize_emit_bf16");
}

// The body of the two drivers; bf16: states and goal hold bf16, and there is no persistent grow (persist_ws == NULL).
// The driver keeps the state in slot 0 or slot 2 of `states` (cur).  A persistent call reads slot cur and writes slot cur ^ 2.  A per-step call
// runs the ring {cur, cur + 1}: after step_n steps the pending state lies in slot cur + (step_n & 1); the finalize writes the resolved state
// to slot cur when step_n is odd (the input is dead by then) and to slot cur ^ 2 when it is even (x_final must not be the pending slot).
// Each call's steps are enqueued by cond_grow_fwd_impl as ncahip_cond_grow_fwd_f32 / _bf16 enqueue them; fp32: an emit launch follows,
// bf16: the grow's last launch is the fused finalize + image.
static int cond_clip_impl(bool bf16, void* states_v, uint8_t* pre, const void* goal_v, int goal_ch, void* images, int img_fmt, int F, int steps_per_frame,
                          int step_n, const float* u, const float* wp, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, int B, int C, int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                          float clamp_hi, uint64_t seed, uint64_t step0, void* persist_ws, size_t persist_bytes, unsigned epoch0,
                          ncahip_stream_t stream) {
    const char* const who = bf16 ? "cond clip (bf16)" : "cond clip";
    char* const states = (char*)states_v;
    const char* const goal = (const char*)goal_v;
    // host-side checks: nothing is enqueued before all of them have passed
    if (!pre || !goal) return fail(NCAHIP_EINVAL, "%s: null pointer", who);
    NcaImgOut io;   // the image record of this call: built once, handed to every emit
    if (int rc = check_clip_emit_unit(states, images, img_fmt, &io, B, C, H, W)) return rc;
    uint64_t calls = 0;
    if (int rc = check_clip_counts(who, F, steps_per_frame, step_n, &calls)) return rc;
    // the checks of the grow drivers (they take no T = 0, so they are shared as functions): their codes
    if (int rc = check_cond(states, states + 1, pre, goal, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, goal_ch, alive_ch,
                            bf16 ? kMaxCCondFwdBf16 : kMaxCCondFwd))
        return rc;
    if (bf16) {   // W % 4 == 0: every state slot and every frame's goal is 8-byte aligned as slot 0 and goal[0] are
        if (int rc = check_bf16_shape(states, states, goal, H, W)) return rc;
    }
    const bool ubits = u_is_bits(u, seed);
    if (int rc = check_bits(ubits, B, H, W, fire_rate, false)) return rc;
    const size_t esize = bf16 ? sizeof(uint16_t) : sizeof(float), pslot = (size_t)B * H * W;
    const size_t slot = pslot * C * esize, gslot = pslot * goal_ch * esize;   // bytes
    const size_t ibytes = clip_img_bytes(io, B, 3, H, W);
    const size_t sbytes = 4 * slot, pbytes = 2 * pslot, gbytes = (size_t)F * gslot, abytes = (size_t)calls * ibytes;
    if (clip_overlap(states, sbytes, goal, gbytes) || clip_overlap(states, sbytes, images, abytes) || clip_overlap(states, sbytes, pre, pbytes) ||
        clip_overlap(goal, gbytes, images, abytes) || clip_overlap(goal, gbytes, pre, pbytes) || clip_overlap(images, abytes, pre, pbytes))
        return fail(NCAHIP_EINVAL, "%s: states, pre, goal and images must not overlap", who);
    if (int rc = check_clip_epochs(who, persist_ws, epoch0, calls)) return rc;
    if (persist_ws) {
        const size_t need = ncahip_cond_grow_persist_workspace(B, C, H, W, hidden, goal_ch);
        if (need != 0 && persist_bytes < need) return fail(NCAHIP_EINVAL, "%s: persistent workspace too small", who);
    }
    if (int rc = device_error_rc(who)) return rc;

    hipStream_t st = (hipStream_t)stream;
    bool persist = persist_ws != nullptr;
    int cur = 0;   // the slot that holds the state: 0 or 2
    for (int n = 0; n < (int)calls; ++n) {
        const char* const gf = goal + (size_t)(n / steps_per_frame) * gslot;
        const int t0 = n * step_n;                                  // first step of this call within `u`
        const uint64_t s0 = step0 + (uint64_t)t0;
        char* const in = states + (size_t)cur * slot;
        void* const img = (char*)images + (size_t)n * ibytes;
        bool done = false;
        if (persist) {
            const int rc = ncahip_cond_grow_fwd_persist_f32((float*)in, nullptr, 2, step_n, (float*)(states + (size_t)(cur ^ 2) * slot), (const float*)gf, goal_ch,
                                                            u_at(u, ubits, t0, pslot), wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, alive_ch, alive_thr, fire_rate,
                                                            clamp_lo, clamp_hi, seed, s0, persist_ws, persist_bytes, epoch0 + (unsigned)n, stream);
            if (rc == 0) {
                cur ^= 2;
                done = true;
            } else if (rc == NCAHIP_ERANGE) {
                persist = false;   // not covered (shape, masks, alignment, residency): this call and the rest run on the per-step kernels
            } else {
                return rc;
            }
        }
        if (!done) {
            const int out = (step_n & 1) ? cur : cur ^ 2;
            if (int rc = cond_grow_fwd_impl(bf16, in, pre, 2, step_n, states + (size_t)out * slot, gf, goal_ch, u_at(u, ubits, t0, pslot), wp, w1, b1, w2, b2, w3,
                                            B, C, H, W, hidden, alive_ch, alive_thr, fire_rate, clamp_lo, clamp_hi, seed, s0, stream, bf16 ? img : nullptr, &io))
                return rc;
            cur = out;
        }
        if (!bf16) {
            if (int rc = hip_result(nca_launch_clip_emit({states + (size_t)cur * slot, false, img, io, true, nullptr, B, C, 3, H, W}, st), "cond clip (emit)"))
                return rc;
        }
    }
    if (cur != 0)   // the state returns in slot 0: the one copy of a call
        return hip_result(hipMemcpyAsync(states, states + (size_t)cur * slot, slot, hipMemcpyDeviceToDevice, st),
                          bf16 ? "cond clip (bf16 state copy)" : "cond clip (state copy)");
    return 0;
}

int ncahip_cond_clip_f32(float* states, uint8_t* pre, const float* goal, int goal_ch, void* images, int img_fmt, int F, int steps_per_frame,
                         int step_n, const float* u, const float* wp, const float* w1, const float* b1, const float* w2, const float* b2,
                         const float* w3, int B, int C, int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                         float clamp_hi, uint64_t seed, uint64_t step0, void* persist_ws, size_t persist_bytes, unsigned epoch0,
                         ncahip_stream_t stream) {
    return cond_clip_impl(false, states, pre, goal, goal_ch, images, img_fmt, F, steps_per_frame, step_n, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden,
                          alive_ch, alive_thr, fire_rate, clamp_lo, clamp_hi, seed, step0, persist_ws, persist_bytes, epoch0, stream);
}
int ncahip_cond_clip_bf16(uint16_t* states, uint8_t* pre, const uint16_t* goal, int goal_ch, void* images, int img_fmt, int F, int steps_per_frame,
                          int step_n, const float* u, const float* wp, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, int B, int C, int H, int W, int hidden, int alive_ch, float alive_thr, float fire_rate, float clamp_lo,
                          float clamp_hi, uint64_t seed, uint64_t step0, ncahip_stream_t stream) {
    return cond_clip_impl(true, states, pre, goal, goal_ch, images, img_fmt, F, steps_per_frame, step_n, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden,
                          alive_ch, alive_thr, fire_rate, clamp_lo, clamp_hi, seed, step0, nullptr, 0, 0, stream);
}

// ---- decoder-sized uint8 frames: crop + Pillow-exact resize before the clip front ends (nca_resize.hip) ----------------------------
static bool resize_filter_ok(int filter) { return filter == NCAHIP_RESIZE_BICUBIC || filter == NCAHIP_RESIZE_LANCZOS; }
constexpr int kResizeMaxDim = 16384, kResizeMaxKsize = 2048;

int ncahip_resize_ksize(int in, int out, int filter) {
    if (in <= 0 || out <= 0) return fail(NCAHIP_EINVAL, "resize_ksize: bad size in=%d out=%d", in, out);
    if (!resize_filter_ok(filter)) return fail(NCAHIP_EINVAL, "resize_ksize: unknown filter %d", filter);
    const int ks = nca_resize_ksize(in, out, filter);
    if (ks < 0) return fail(NCAHIP_ERANGE, "resize_ksize: the table row of in=%d out=%d does not fit an int", in, out);
    return ks;
}

int ncahip_resize_tables(int in, int out, int filter, int32_t* k, int32_t* bounds, int ksize) {
    if (!k || !bounds) return fail(NCAHIP_EINVAL, "resize_tables: null pointer");
    const int ks = ncahip_resize_ksize(in, out, filter);
    if (ks < 0) return ks;
    if (ksize != ks) return fail(NCAHIP_EINVAL, "resize_tables: ksize=%d, but ncahip_resize_ksize(%d, %d, %d) = %d", ksize, in, out, filter, ks);
    if (const int row = nca_resize_build_tables(in, out, filter, k, bounds, ksize))
        return fail(NCAHIP_ERANGE, "resize_tables: row %d of in=%d out=%d breaks the int32 bound of a pass (255 * sum|k| + 2^21 < 2^31, |k| < 2^23)",
                    row - 1, in, out);
    return 0;
}

size_t ncahip_clip_resize_workspace(int N, int crop_h, int out_w) {
    if (N <= 0 || crop_h <= 0 || out_w <= 0) return 0;
    return (size_t)N * crop_h * out_w * 3;
}

// the checks of the resize entry points; frame_bytes: H * W * 3 (RGB24) or H * W * 3 / 2 (planar 4:2:0); planar_dst: dst is
// [N, 3 out_h / 2, out_w], half the bytes
static int clip_resize_check(const char* who, const uint8_t* src, size_t frame_bytes, int N, int H, int W, int x0, int y0, int crop_w, int crop_h,
                             const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, uint8_t* dst,
                             int out_h, int out_w, void* workspace, size_t workspace_bytes, bool planar_dst = false) {
    if (!src || !dst) return fail(NCAHIP_EINVAL, "%s: null pointer", who);
    if (N <= 0 || H <= 0 || W <= 0 || crop_w <= 0 || crop_h <= 0 || out_h <= 0 || out_w <= 0 || ksize_x <= 0 || ksize_y <= 0)
        return fail(NCAHIP_EINVAL, "%s: bad size", who);
    if (H > kResizeMaxDim || W > kResizeMaxDim || out_h > kResizeMaxDim || out_w > kResizeMaxDim)
        return fail(NCAHIP_ERANGE, "%s: H=%d W=%d out_h=%d out_w=%d exceeds %d", who, H, W, out_h, out_w, kResizeMaxDim);
    if (ksize_x > kResizeMaxKsize || ksize_y > kResizeMaxKsize)
        return fail(NCAHIP_ERANGE, "%s: table width ksize_x=%d ksize_y=%d exceeds %d", who, ksize_x, ksize_y, kResizeMaxKsize);
    if (x0 < 0 || y0 < 0 || crop_w > W - x0 || crop_h > H - y0)
        return fail(NCAHIP_ERANGE, "%s: crop (x0=%d, y0=%d, w=%d, h=%d) lies outside the %d x %d frame", who, x0, y0, crop_w, crop_h, H, W);
    if (!kx || !bx || !ky || !by || (((uintptr_t)kx | (uintptr_t)bx | (uintptr_t)ky | (uintptr_t)by) & 3) != 0)
        return fail(NCAHIP_ERANGE, "%s: null or misaligned table (int32, 4-byte aligned)", who);
    if (!workspace || ((uintptr_t)workspace & 3) != 0) return fail(NCAHIP_ERANGE, "%s: null or misaligned workspace (4-byte aligned)", who);
    const size_t need = ncahip_clip_resize_workspace(N, crop_h, out_w);
    if (workspace_bytes < need) return fail(NCAHIP_EINVAL, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    const size_t sbytes = (size_t)N * frame_bytes, dbytes = (size_t)N * out_h * out_w * 3 / (planar_dst ? 2 : 1);
    if (clip_overlap(src, sbytes, dst, dbytes) || clip_overlap(src, sbytes, workspace, need) || clip_overlap(dst, dbytes, workspace, need))
        return fail(NCAHIP_EINVAL, "%s: frames, output and workspace must not overlap", who);
    return 0;
}

int ncahip_clip_resize_u8(const uint8_t* src, int N, int H, int W, int x0, int y0, int crop_w, int crop_h, const int32_t* kx, const int32_t* bx,
                          int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, uint8_t* dst, int out_h, int out_w, void* workspace,
                          size_t workspace_bytes, ncahip_stream_t stream) {
    if (int rc = clip_resize_check("clip_resize", src, (size_t)H * W * 3, N, H, W, x0, y0, crop_w, crop_h, kx, bx, ksize_x, ky, by, ksize_y, dst, out_h,
                                   out_w, workspace, workspace_bytes))
        return rc;
    return hip_result(nca_launch_clip_resize(src, N, H, W, x0, y0, crop_w, crop_h, kx, bx, ksize_x, ky, by, ksize_y, dst, out_h, out_w,
                                             (unsigned char*)workspace, (hipStream_t)stream), "clip_resize");
}

// ---- planar YUV 4:2:0 clip frames (nca_yuv.hip; the fused loader in nca_resize.hip) ------------------------------------------------
static bool yuv_layout_ok(int layout) { return layout == NCAHIP_YUV_I420 || layout == NCAHIP_YUV_NV12; }

int ncahip_yuv_coeffs(int matrix, int range, int32_t k[6]) {
    if (!k) return fail(NCAHIP_EINVAL, "yuv_coeffs: null pointer");
    if (matrix != NCAHIP_YUV_BT601 && matrix != NCAHIP_YUV_BT709) return fail(NCAHIP_EINVAL, "yuv_coeffs: unknown matrix %d", matrix);
    if (range != NCAHIP_YUV_LIMITED && range != NCAHIP_YUV_FULL) return fail(NCAHIP_EINVAL, "yuv_coeffs: unknown range %d", range);
    nca_yuv_build_coeffs(matrix, range, k);
    return 0;
}

int ncahip_clip_yuv420_to_rgb_u8(const uint8_t* src, int layout, int N, int H, int W, int x0, int y0, int crop_w, int crop_h, const int32_t* k,
                                 uint8_t* dst, ncahip_stream_t stream) {
    if (!src || !dst || !k) return fail(NCAHIP_EINVAL, "clip_yuv420_to_rgb: null pointer");
    if (!yuv_layout_ok(layout)) return fail(NCAHIP_EINVAL, "clip_yuv420_to_rgb: unknown layout %d", layout);
    if (N <= 0 || H <= 0 || W <= 0 || crop_w <= 0 || crop_h <= 0) return fail(NCAHIP_EINVAL, "clip_yuv420_to_rgb: bad size");
    if (H > kResizeMaxDim || W > kResizeMaxDim) return fail(NCAHIP_ERANGE, "clip_yuv420_to_rgb: H=%d W=%d exceeds %d", H, W, kResizeMaxDim);
    if ((H | W) & 1) return fail(NCAHIP_ERANGE, "clip_yuv420_to_rgb: 4:2:0 frames have even sides, got %d x %d", H, W);
    if (x0 < 0 || y0 < 0 || crop_w > W - x0 || crop_h > H - y0)
        return fail(NCAHIP_ERANGE, "clip_yuv420_to_rgb: crop (x0=%d, y0=%d, w=%d, h=%d) lies outside the %d x %d frame", x0, y0, crop_w, crop_h, H, W);
    if (clip_overlap(src, (size_t)N * H * W / 2 * 3, dst, (size_t)N * crop_h * crop_w * 3))
        return fail(NCAHIP_EINVAL, "clip_yuv420_to_rgb: frames and output must not overlap");
    return hip_result(nca_launch_clip_yuv420_to_rgb(src, layout == NCAHIP_YUV_NV12, N, H, W, x0, y0, crop_w, crop_h, k, dst, (hipStream_t)stream),
                      "clip_yuv420_to_rgb");
}

int ncahip_rgb_yuv_coeffs(int matrix, int range, int32_t k[10]) {
    if (!k) return fail(NCAHIP_EINVAL, "rgb_yuv_coeffs: null pointer");
    if (matrix != NCAHIP_YUV_BT601 && matrix != NCAHIP_YUV_BT709) return fail(NCAHIP_EINVAL, "rgb_yuv_coeffs: unknown matrix %d", matrix);
    if (range != NCAHIP_YUV_LIMITED && range != NCAHIP_YUV_FULL) return fail(NCAHIP_EINVAL, "rgb_yuv_coeffs: unknown range %d", range);
    nca_rgb_yuv_build_coeffs(matrix, range, k);
    return 0;
}

int ncahip_clip_rgb_to_yuv420_u8(const uint8_t* src, int layout, int N, int H, int W, const int32_t* k, uint8_t* dst, ncahip_stream_t stream) {
    if (!src || !dst || !k) return fail(NCAHIP_EINVAL, "clip_rgb_to_yuv420: null pointer");
    if (!yuv_layout_ok(layout)) return fail(NCAHIP_EINVAL, "clip_rgb_to_yuv420: unknown layout %d", layout);
    if (N <= 0 || H <= 0 || W <= 0) return fail(NCAHIP_EINVAL, "clip_rgb_to_yuv420: bad size");
    if (H > kResizeMaxDim || W > kResizeMaxDim) return fail(NCAHIP_ERANGE, "clip_rgb_to_yuv420: H=%d W=%d exceeds %d", H, W, kResizeMaxDim);
    if ((H | W) & 1) return fail(NCAHIP_ERANGE, "clip_rgb_to_yuv420: 4:2:0 images have even sides, got %d x %d", H, W);
    if (clip_overlap(src, (size_t)N * H * W * 3, dst, (size_t)N * H * W / 2 * 3))
        return fail(NCAHIP_EINVAL, "clip_rgb_to_yuv420: images and output must not overlap");
    return hip_result(nca_launch_clip_rgb_to_yuv420(src, layout == NCAHIP_YUV_NV12, N, H, W, k, dst, (hipStream_t)stream), "clip_rgb_to_yuv420");
}

int ncahip_clip_resize_yuv420_u8(const uint8_t* src, int layout, const int32_t* k, int N, int H, int W, int x0, int y0, int crop_w, int crop_h,
                                 const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, uint8_t* dst,
                                 int out_h, int out_w, void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    if (!k) return fail(NCAHIP_EINVAL, "clip_resize_yuv420: null pointer");
    if (!yuv_layout_ok(layout)) return fail(NCAHIP_EINVAL, "clip_resize_yuv420: unknown layout %d", layout);
    if (int rc = clip_resize_check("clip_resize_yuv420", src, (size_t)H * W / 2 * 3, N, H, W, x0, y0, crop_w, crop_h, kx, bx, ksize_x, ky, by, ksize_y,
                                   dst, out_h, out_w, workspace, workspace_bytes))
        return rc;
    if ((H | W) & 1) return fail(NCAHIP_ERANGE, "clip_resize_yuv420: 4:2:0 frames have even sides, got %d x %d", H, W);
    return hip_result(nca_launch_clip_resize_yuv420(src, layout == NCAHIP_YUV_NV12, k, N, H, W, x0, y0, crop_w, crop_h, kx, bx, ksize_x, ky, by, ksize_y,
                                                    dst, out_h, out_w, (unsigned char*)workspace, (hipStream_t)stream), "clip_resize_yuv420");
}

int ncahip_clip_resize_u8_yuv420(const uint8_t* src, int N, int H, int W, int x0, int y0, int crop_w, int crop_h, const int32_t* kx, const int32_t* bx,
                                 int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, int layout, const int32_t* k, uint8_t* dst, int out_h,
                                 int out_w, void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    if (!k) return fail(NCAHIP_EINVAL, "clip_resize_u8_yuv420: null pointer");
    if (!yuv_layout_ok(layout)) return fail(NCAHIP_EINVAL, "clip_resize_u8_yuv420: unknown layout %d", layout);
    if (int rc = clip_resize_check("clip_resize_u8_yuv420", src, (size_t)H * W * 3, N, H, W, x0, y0, crop_w, crop_h, kx, bx, ksize_x, ky, by, ksize_y,
                                   dst, out_h, out_w, workspace, workspace_bytes, true))
        return rc;
    if ((out_h | out_w) & 1) return fail(NCAHIP_ERANGE, "clip_resize_u8_yuv420: 4:2:0 images have even sides, got %d x %d", out_h, out_w);
    return hip_result(nca_launch_clip_resize_u8_yuv420(src, N, H, W, x0, y0, crop_w, crop_h, kx, bx, ksize_x, ky, by, ksize_y, layout == NCAHIP_YUV_NV12,
                                                       k, dst, out_h, out_w, (unsigned char*)workspace, (hipStream_t)stream), "clip_resize_u8_yuv420");
}

// ---- the DyNCA backward: an entry point names its variant with a constant record and makes one forwarding call; every check is
// written once ----------------------------------------------------------------------------------------------------------------
namespace {
// mma: the fp32 kernels, or the bf16-MFMA training mode in its narrow range (C <= 16, fc <= 128) or its wide one (C <= 32, fc <= 256,
// single-scale).  The range is what an entry point refuses by; which kernels run inside it the shape alone tells (dynca_bwd_mlp_bf16
// below, nca_launch_gram_rows_bf16_wide): the wide entry points send narrow shapes to the narrow path.
enum DyncaBwdMma { kBwdExact, kBwdBfNarrow, kBwdBfWide };
struct DyncaBwdVariant { bool two_scale; int state_bytes; DyncaBwdMma mma; };   // a driver; state_bytes: 4 = fp32 history, 2 = bf16 (storage format only)
constexpr DyncaBwdVariant kBwdF32{false, 4, kBwdExact}, kBwdMs{true, 4, kBwdExact}, kBwdBf16{false, 2, kBwdExact},
                          kBwdBfmma{false, 4, kBwdBfNarrow}, kBwdMsBfmma{true, 4, kBwdBfNarrow}, kBwdBfmmaWide{false, 4, kBwdBfWide};
// a single-step stage entry: its name in a refusal and in a launch error, its mode, the widest layer check_dynca lets through, the mode's range
struct DyncaStepBwd { const char *who, *label; DyncaBwdMma mma; int max_fc; const char* range; };
constexpr DyncaStepBwd kStepBwdF32{"dynca step bwd", "dynca_step_bwd", kBwdExact, kMaxFc, ""},
                       kStepBwdW2{"dynca step bwd_w2", "dynca_step_bwd_w2", kBwdExact, kMaxFc, ""},
                       kStepBwdBfmma{"dynca step bwd_bfmma", "dynca_step_bwd_bfmma", kBwdBfNarrow, kMaxFc, "(C <= 16, fc <= 128)"},
                       kStepBwdBfmmaWide{"dynca step bwd_bfmma_wide", "dynca_step_bwd_bfmma_wide", kBwdBfWide, 256, "(C <= 32, fc <= 256)"};

// "Is this shape in range": a workspace query and its entry point ask the same function (always true for the fp32 kernels: check_dynca is their range).  The MLP stage: (C, fc)
bool dynca_bwd_mlp_range_ok(DyncaBwdMma mma, int C, int fc) {
    return mma == kBwdExact || (mma == kBwdBfNarrow ? nca_dynca_bf16_shape_ok(C, fc) : nca_dynca_bf16_wide_shape_ok(C, fc));
}
// a driver: also the 4C + c_cond columns of its layer-1 weight-gradient product (what a query adds; past check_dynca, c_cond <= 4 fits both)
bool dynca_bwd_range_ok(DyncaBwdMma mma, int C, int fc, int c_cond) {
    return dynca_bwd_mlp_range_ok(mma, C, fc) && (mma == kBwdExact || 4 * C + c_cond <= (mma == kBwdBfNarrow ? kNcaGramBf : kNcaGramBfWide).nb);
}
// the MLP launch of the bf16-MFMA backward: the two launchers share the wide range out between them by shape (each refuses the other's)
hipError_t dynca_bwd_mlp_bf16(const NcaDyncaArgs& a, hipStream_t st) {
    return nca_dynca_bf16_shape_ok(a.C, a.fc) ? nca_launch_dynca_step_bwd_mlp_bf16(a, st) : nca_launch_dynca_step_bwd_mlp_bf16_wide(a, st);
}
// the backward kernels store [rows, H, W] planes of one batch item (rows = the hidden units of a launch, or 4C) through 32-bit offsets
int check_store_offsets(const char* who, const char* rows_name, int rows, int C, int H, int W) {
    if ((size_t)(rows > 4 * C ? rows : 4 * C) * H * W * sizeof(float) < ((size_t)1 << 32)) return 0;
    return fail(NCAHIP_ERANGE, "%s: %s*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)", who, rows_name);
}
// What every single-step stage entry checks first, in this order.  a: the step as the entry will launch it; null_ptr: one of the entry's
// own pointers is null.  The wide entry's check_dynca is its range refusal (NCAHIP_ERANGE beyond C = 32 / fc = 256): the one below it is unreachable there, as for the exact entries
int dynca_step_bwd_checks(const DyncaStepBwd& v, bool null_ptr, const NcaDyncaArgs& a) {
    if (int rc = dynca_dir_refuse(v.who)) return rc;
    if (null_ptr) return fail(NCAHIP_EINVAL, "%s: null pointer", v.who);
    if (int rc = check_dynca(a.x_in, a.g_out, a.cond, a.w1, a.b1, a.w2, a.b2, a.B, a.C, a.H, a.W, a.fc, a.c_cond, a.pad_mode, v.max_fc)) return rc;
    if (!dynca_bwd_mlp_range_ok(v.mma, a.C, a.fc)) return fail(NCAHIP_ERANGE, "%s: C=%d fc=%d outside the bf16-MFMA range %s", v.who, a.C, a.fc, v.range);
    if (a.g_next == a.g_out) return fail(NCAHIP_EINVAL, "%s: g_next and g_x must not alias", v.who);
    return check_store_offsets(v.who, "fc", a.fc, a.C, a.H, a.W);
}
}  // namespace

int ncahip_dynca_step_bwd_f32(const float* x_t, const float* cond, const float* u, const float* w1, const float* b1,
                              const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                              float update_rate, uint64_t seed, uint64_t step, const float* g_next, float* g_x, float* h_out,
                              float* dh_out, float* dy_scratch, ncahip_stream_t stream) {
    NcaDyncaArgs a{x_t, nullptr, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step, g_next, h_out, dh_out, dy_scratch, g_x};
    a.u_bits = u_is_bits(u, seed);
    if (int rc = dynca_step_bwd_checks(kStepBwdF32, !g_next || !g_x || !h_out || !dh_out || !dy_scratch, a)) return rc;
    if (int rc = check_bits(a.u_bits, B, H, W, update_rate, true)) return rc;
    return hip_result(nca_launch_dynca_step_bwd(a, (hipStream_t)stream), kStepBwdF32.label);
}

// ---- backward of one DyNCA step with the layer-2 weight gradient fused in (no h buffer) ---------------------------------
size_t ncahip_dynca_step_bwd_w2_workspace(int B, int C, int H, int W, int fc) {
    if (!dims_ok(B, C, H, W) || fc <= 0 || !dynca_bwd_mlp_range_ok(kStepBwdW2.mma, C, fc)) return 0;
    return (size_t)nca_dynca_bwd_grid(B, H, W) * ((size_t)C * fc + C) * sizeof(float);
}

int ncahip_dynca_step_bwd_w2_f32(const float* x_t, const float* cond, const float* u, const float* w1, const float* b1,
                                 const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                 float update_rate, uint64_t seed, uint64_t step, const float* g_next, float* g_x,
                                 float* dh_out, float* dy_scratch, float* gw2_out, int accumulate, void* workspace,
                                 size_t workspace_bytes, ncahip_stream_t stream) {
    const DyncaStepBwd& v = kStepBwdW2;
    NcaDyncaArgs a{x_t, nullptr, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step, g_next, nullptr, dh_out, dy_scratch, g_x};
    a.gw2_ws = (float*)workspace;
    a.u_bits = u_is_bits(u, seed);
    if (int rc = dynca_step_bwd_checks(v, !g_next || !g_x || !dh_out || !dy_scratch || !gw2_out || !workspace, a)) return rc;
    if (workspace_bytes < ncahip_dynca_step_bwd_w2_workspace(B, C, H, W, fc)) return fail(NCAHIP_EINVAL, "%s: workspace too small", v.who);
    if (int rc = check_bits(a.u_bits, B, H, W, update_rate, true)) return rc;
    if (int rc = hip_result(nca_launch_dynca_step_bwd(a, (hipStream_t)stream), v.label)) return rc;
    return hip_result(nca_launch_reduce_rows((const float*)workspace, gw2_out, nca_dynca_bwd_grid_c(B, C, H, W), C * fc + C,
                                             (hipStream_t)stream, accumulate != 0), v.label, " reduce");
}

// ---- backward of ncahip_dynca_nsteps_fwd_f32: the whole T-step loop on the stream, caller-owned workspace ----------------
namespace {
struct DyncaBwdPlan {
    int nsl, fs, fc;             // hidden-layer slices of at most 128 units (fs = width of the full slices, fc = the whole layer)
    size_t n, off_g[2], off_y, off_dy, off_dh, off_ws2, off_wsg, off_acc1, off_acc2, off_pc, off_dpc, off_dxc, off_x32, total;
    int grid2, gridg, K1;
    struct Slice { int h0, fs; };   // slice sl: its first hidden unit and its width (a single slice is the whole layer)
    Slice slice(int sl) const { return {sl * 128, nsl == 1 ? fc : (fc - sl * 128 < 128 ? fc - sl * 128 : 128)}; }
};
// The bf16-MFMA training mode: y and dh are bf16 (half the floats), the gram partials are nca_gram_bf16_grid slabs; its buffers
// hold the whole hidden layer (narrow range: fc <= 128 anyway; wide range: the step launcher slices, dh, the slabs and the accumulators
// have the full layout and the layer-1 weight gradient is ONE product per step)
DyncaBwdPlan dynca_bwd_plan(const DyncaBwdVariant& v, int B, int C, int H, int W, int fc, int c_cond) {
    const bool bfmma = v.mma != kBwdExact;
    DyncaBwdPlan p{};
    p.fc = fc;
    p.nsl = bfmma ? 1 : (fc + 127) / 128;
    p.fs = (bfmma || fc < 128) ? fc : 128;
    p.K1 = 4 * C + c_cond;
    p.n = (size_t)B * C * H * W;
    p.grid2 = v.two_scale ? nca_dynca_bwd_ms_grid(B, H, W) : nca_dynca_bwd_grid_c(B, C, H, W);
    p.gridg = bfmma ? nca_gram_bf16_grid(B, H * W) : nca_gram_grid(B, H * W);
    size_t o = 0;
    auto take = [&](size_t floats) { size_t at = o; o += (floats * sizeof(float) + 255) & ~(size_t)255; return at; };
    p.off_g[0] = take(p.n);
    p.off_g[1] = take(p.n);
    p.off_y = take(bfmma ? 2 * p.n : 4 * p.n);
    p.off_dy = take(4 * p.n);
    p.off_dh = take(bfmma ? ((size_t)B * p.fs * H * W + 1) / 2 : (size_t)B * p.fs * H * W);
    p.off_ws2 = take((size_t)p.grid2 * ((size_t)C * p.fs + C));
    p.off_wsg = take((size_t)p.gridg * ((size_t)p.fs * p.K1 + p.fs));
    p.off_acc1 = take((size_t)p.nsl * ((size_t)p.fs * p.K1 + p.fs));
    p.off_acc2 = take((size_t)p.nsl * ((size_t)C * p.fs + C));
    if (v.two_scale) {   // coarse-level perception, its gradient, and dL/dx of the coarse level
        p.off_pc = take(p.n);      // 4C * (H/2) * (W/2) = C*H*W floats
        p.off_dpc = take(p.n);
        p.off_dxc = take(p.n / 4);
    }
    if (v.state_bytes == 2) p.off_x32 = take(p.n);   // x_t widened to fp32
    p.total = o;
    return p;
}

size_t dynca_nsteps_bwd_query(const DyncaBwdVariant& v, int B, int C, int H, int W, int fc, int c_cond) {
    if (!dims_ok(B, C, H, W) || fc <= 0 || c_cond < 0 || !dynca_bwd_range_ok(v.mma, C, fc, c_cond)) return 0;
    return dynca_bwd_plan(v, B, C, H, W, fc, c_cond).total;
}

int dynca_nsteps_bwd_impl(const DyncaBwdVariant& v, const void* states_v, int T, const float* cond, const float* u, const float* w1, const float* b1,
                          const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                          float update_rate, uint64_t seed, uint64_t step0, const float* g_final, const float* g_states,
                          float* g_x0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                          size_t workspace_bytes, ncahip_stream_t stream) {
    const char* const states = (const char*)states_v;
    const bool two_scale = v.two_scale, bf16 = v.state_bytes == 2, bfmma = v.mma != kBwdExact;
    if (int rc = dynca_dir_refuse("dynca nsteps bwd")) return rc;
    if (T < 1 || !states || !g_final || !g_x0 || !g_w1 || !g_b1 || !g_w2 || !g_b2 || !workspace)
        return fail(NCAHIP_EINVAL, "dynca nsteps bwd: null pointer or T < 1");
    if (int rc = check_dynca(states, g_x0, cond, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, kMaxFcFwd)) return rc;
    if (bf16 && ((((size_t)B * C * H * W) & 3) != 0 || ((uintptr_t)states & 7) != 0))
        return fail(NCAHIP_ERANGE, "dynca nsteps bwd (bf16): B*C*H*W %% 4 == 0 and 8-byte aligned states required");
    if (int rc = check_store_offsets("dynca nsteps bwd", "4C", 128, C, H, W)) return rc;
    if (v.mma == kBwdBfNarrow && !dynca_bwd_range_ok(v.mma, C, fc, c_cond))   // bf16-MFMA training mode: the history is a mode-1 one, the backward its own kernels
        return fail(NCAHIP_ERANGE, "dynca nsteps bwd (bf16 MFMA): C=%d fc=%d outside the mode's range (C <= 16, fc <= 128)", C, fc);
    if (v.mma == kBwdBfWide && !dynca_bwd_range_ok(v.mma, C, fc, c_cond))     // (a narrow shape is in the wide range too: it runs the narrow path)
        return fail(NCAHIP_ERANGE, "dynca nsteps bwd (bf16 MFMA, wide): C=%d fc=%d outside the mode's wide range (C <= 32, fc <= 256, single-scale)", C, fc);
    if (two_scale) {
        if (int rc = check_ms(C, H, W, fc, pad_mode, workspace)) return rc;
    }
    const bool ubits = u_is_bits(u, seed);
    if (int rc = check_bits(ubits, B, H, W, update_rate, true)) return rc;
    const DyncaBwdPlan p = dynca_bwd_plan(v, B, C, H, W, fc, c_cond);
    if (workspace_bytes < p.total) return fail(NCAHIP_EINVAL, "dynca nsteps bwd: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(NCAHIP_ERANGE, "dynca nsteps bwd: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* const ws = (char*)workspace;
    float* const gbuf[2] = {(float*)(ws + p.off_g[0]), (float*)(ws + p.off_g[1])};
    float* const y = (float*)(ws + p.off_y);
    float* const dy = (float*)(ws + p.off_dy);
    float* const dh = (float*)(ws + p.off_dh);
    float* const ws2 = (float*)(ws + p.off_ws2);
    float* const wsg = (float*)(ws + p.off_wsg);
    float* const acc1 = (float*)(ws + p.off_acc1);
    float* const acc2 = (float*)(ws + p.off_acc2);
    float* const pcb = two_scale ? (float*)(ws + p.off_pc) : nullptr;
    float* const dpc = two_scale ? (float*)(ws + p.off_dpc) : nullptr;
    float* const dxc = two_scale ? (float*)(ws + p.off_dxc) : nullptr;
    const size_t a1n = (size_t)p.fs * p.K1 + p.fs, a2n = (size_t)C * p.fs + C;
    hipError_t e = nca_zero_async(acc1, (size_t)p.nsl * a1n, st);
    if (e == hipSuccess) e = nca_zero_async(acc2, (size_t)p.nsl * a2n, st);
    if (e != hipSuccess) return hip_result(e, "dynca nsteps bwd memset");
    const size_t slot = p.n, uslot = (size_t)B * H * W;
    const float* gcur = g_final;
    for (int t = T - 1; t >= 0; --t) {
        const float* x_t = reinterpret_cast<const float*>(states + (size_t)t * slot * v.state_bytes);
        if (bf16) {   // bf16 history (storage format only: the DyNCA step computes in fp32 on the widened state)
            float* const x32 = (float*)(ws + p.off_x32);
            if (int rc = hip_result(nca_launch_widen_bf16(reinterpret_cast<const uint16_t*>(x_t), x32, slot, st), "dynca nsteps bwd widen")) return rc;
            x_t = x32;
        }
        float* const g_out = t == 0 ? g_x0 : gbuf[t & 1];
        // y (the B rows of the layer-1 weight-gradient product) is written by the first slice's step kernel, which recomputes it anyway
        if (two_scale) {   // coarse level of the two-scale perception: input of the step kernel
            if (int rc = hip_result(nca_launch_dynca_coarse_perceive(x_t, pcb, B, C, H, W, pad_mode, st), "dynca nsteps bwd coarse perceive")) return rc;
        }
        for (int sl = 0; sl < p.nsl; ++sl) {
            const auto [h0, fs] = p.slice(sl);
            NcaDyncaArgs a{x_t, nullptr, cond, u_at(u, ubits, t, uslot), w1 + (size_t)h0 * p.K1, b1 + h0, w2 + h0, b2, B, C, H, W,
                           fs, c_cond, pad_mode, update_rate, seed, step0 + (uint64_t)t, gcur, nullptr, dh, dy, g_out};
            a.w2_ld = fc;
            a.u_bits = ubits;
            a.gw2_ws = ws2;
            a.pc = pcb;
            a.ybuf = sl == 0 ? y : nullptr;
            if (bfmma) {   // the whole layer (wide range: sliced inside the step launcher); y and dh are bf16 buffers in the same workspace regions
                if (int rc = hip_result(dynca_bwd_mlp_bf16(a, st), "dynca nsteps bwd step (bf16 MFMA)")) return rc;
                if (int rc = hip_result(nca_launch_reduce_rows(ws2, acc2, p.grid2, C * fs + C, st, true), "dynca nsteps bwd reduce")) return rc;
                if (int rc = hip_result(nca_launch_gram_rows_bf16_wide(reinterpret_cast<const uint16_t*>(dh), fs, reinterpret_cast<const uint16_t*>(y), 4 * C,
                                                                       cond, c_cond, B, H * W, acc1, wsg, st, true), "dynca nsteps bwd gram (bf16 MFMA)")) return rc;
                continue;
            }
            if (int rc = hip_result(nca_launch_dynca_step_bwd_mlp(a, st, sl > 0), "dynca nsteps bwd step")) return rc;
            // slabs hold [C x fs | C] of THIS slice (compact); slices narrower than p.fs use the front of their accumulator
            if (int rc = hip_result(nca_launch_reduce_rows(ws2, acc2 + (size_t)sl * a2n, p.grid2, C * fs + C, st, true), "dynca nsteps bwd reduce")) return rc;
            if (int rc = hip_result(nca_launch_gram_rows(dh, fs, y, 4 * C, cond, c_cond, B, H * W, acc1 + (size_t)sl * a1n, wsg, st, true),
                                    "dynca nsteps bwd gram")) return rc;
        }
        NcaDyncaArgs s{x_t, nullptr, cond, nullptr, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0 + (uint64_t)t,
                       gcur, nullptr, dh, dy, g_out};
        s.g_extra = g_states ? g_states + (size_t)t * slot : nullptr;
        if (two_scale) {
            // dL/dy splits evenly over the two levels: coarse level = up2^T, then the coarse grid's stencil adjoint (pad mode
            // resolved there), then the adjoint of the 2x2 mean inside the fine-level kernel
            if (int rc = hip_result(nca_launch_dynca_ms_upT(dy, dpc, B, C, H, W, st), "dynca nsteps bwd upT")) return rc;
            NcaDyncaArgs cs{nullptr, nullptr, nullptr, nullptr, w1, b1, w2, b2, B, C, H / 2, W / 2, fc, c_cond, pad_mode, update_rate, seed, 0,
                            nullptr, nullptr, nullptr, dpc, dxc};
            if (int rc = hip_result(nca_launch_dynca_step_bwd_stencil(cs, st), "dynca nsteps bwd coarse stencil")) return rc;
            s.coarse_add = dxc;
            s.dy_half = 1;
        }
        if (int rc = hip_result(nca_launch_dynca_step_bwd_stencil(s, st), "dynca nsteps bwd stencil")) return rc;
        gcur = g_out;
    }
    // accumulators -> gradients in the reference layouts: w1 [fc, K1] rows of a slice are contiguous, w2 [C, fc] columns are not
    for (int sl = 0; sl < p.nsl && e == hipSuccess; ++sl) {
        const auto [h0, fs] = p.slice(sl);
        const float* const s1 = acc1 + (size_t)sl * a1n;
        const float* const s2 = acc2 + (size_t)sl * a2n;
        e = hipMemcpyAsync(g_w1 + (size_t)h0 * p.K1, s1, (size_t)fs * p.K1 * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(g_b1 + h0, s1 + (size_t)fs * p.K1, fs * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(g_w2 + h0, (size_t)fc * sizeof(float), s2, (size_t)fs * sizeof(float), (size_t)fs * sizeof(float), C,
                                 hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && sl == 0) e = hipMemcpyAsync(g_b2, s2 + (size_t)C * fs, C * sizeof(float), hipMemcpyDeviceToDevice, st);
    }
    return hip_result(e, "dynca nsteps bwd copy");
}
}  // namespace

size_t ncahip_dynca_nsteps_bwd_workspace(int B, int C, int H, int W, int fc, int c_cond) { return dynca_nsteps_bwd_query(kBwdF32, B, C, H, W, fc, c_cond); }
size_t ncahip_dynca_nsteps_bwd_ms_workspace(int B, int C, int H, int W, int fc, int c_cond) { return dynca_nsteps_bwd_query(kBwdMs, B, C, H, W, fc, c_cond); }
size_t ncahip_dynca_nsteps_bwd_bf16_workspace(int B, int C, int H, int W, int fc, int c_cond) { return dynca_nsteps_bwd_query(kBwdBf16, B, C, H, W, fc, c_cond); }

int ncahip_dynca_nsteps_bwd_f32(const float* states, int T, const float* cond, const float* u, const float* w1, const float* b1,
                                const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                float update_rate, uint64_t seed, uint64_t step0, const float* g_final, const float* g_states,
                                float* g_x0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                                size_t workspace_bytes, ncahip_stream_t stream) {
    return dynca_nsteps_bwd_impl(kBwdF32, states, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0, g_final,
                                 g_states, g_x0, g_w1, g_b1, g_w2, g_b2, workspace, workspace_bytes, stream);
}
int ncahip_dynca_nsteps_bwd_ms_f32(const float* states, int T, const float* cond, const float* u, const float* w1, const float* b1,
                                   const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                   float update_rate, uint64_t seed, uint64_t step0, const float* g_final, const float* g_states,
                                   float* g_x0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                                   size_t workspace_bytes, ncahip_stream_t stream) {
    return dynca_nsteps_bwd_impl(kBwdMs, states, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0, g_final,
                                 g_states, g_x0, g_w1, g_b1, g_w2, g_b2, workspace, workspace_bytes, stream);
}
int ncahip_dynca_nsteps_bwd_bf16(const uint16_t* states, int T, const float* cond, const float* u, const float* w1, const float* b1,
                                 const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                 float update_rate, uint64_t seed, uint64_t step0, const float* g_final, const float* g_states,
                                 float* g_x0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                                 size_t workspace_bytes, ncahip_stream_t stream) {
    return dynca_nsteps_bwd_impl(kBwdBf16, states, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0, g_final,
                                 g_states, g_x0, g_w1, g_b1, g_w2, g_b2, workspace, workspace_bytes, stream);
}

// ---- weight-gradient products of the DyNCA backward (cell axis as K) -------------------------------------------------
size_t ncahip_gram_rows_workspace(int ma, int nb, int B, int HW) {
    if (ma <= 0 || nb <= 0 || B <= 0 || HW <= 0) return 0;
    return (size_t)nca_gram_grid(B, HW) * ((size_t)ma * nb + ma) * sizeof(float);
}

int ncahip_gram_rows_f32(const float* a, int ma, const float* b1, int nb1, const float* b2, int nb2, int B, int HW,
                         float* out, int accumulate, void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    if (!a || !b1 || !out || !workspace || (nb2 > 0) != (b2 != nullptr)) return fail(NCAHIP_EINVAL, "gram_rows: null pointer");
    if (ma <= 0 || nb1 <= 0 || nb2 < 0 || B <= 0 || HW <= 0) return fail(NCAHIP_EINVAL, "gram_rows: bad size");
    const int nb = nb1 + nb2;
    if (!((ma <= 32 && nb <= 128) || (ma <= 128 && nb <= 144)))
        return fail(NCAHIP_ERANGE, "gram_rows: ma=%d nb=%d outside (<=32 x <=128) / (<=128 x <=144)", ma, nb);
    if (workspace_bytes < ncahip_gram_rows_workspace(ma, nb, B, HW)) return fail(NCAHIP_EINVAL, "gram_rows: workspace too small");
    return hip_result(nca_launch_gram_rows(a, ma, b1, nb1, b2, nb2, B, HW, out, (float*)workspace, (hipStream_t)stream,
                                           accumulate != 0), "gram_rows");
}

// ---- the bf16-MFMA training mode of DyNCA: stage entry points (the drivers are ncahip_dynca_nsteps_bwd_bfmma_f32 / _ms_ / _wide_) ----
namespace {
size_t gram_rows_bf16_query(const NcaGramBfRange& r, int ma, int nb, int B, int HW) {
    if (ma <= 0 || nb <= 0 || B <= 0 || HW <= 0 || !nca_gram_bf16_fits(r, ma, nb)) return 0;
    return (size_t)nca_gram_bf16_grid(B, HW) * ((size_t)ma * nb + ma) * sizeof(float);
}

int gram_rows_bf16_impl(const char* who, const NcaGramBfRange& r, const uint16_t* a, int ma, const uint16_t* b1, int nb1, const float* b2, int nb2, int B,
                        int HW, float* out, int accumulate, void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    if (!a || !b1 || !out || !workspace || (nb2 > 0) != (b2 != nullptr)) return fail(NCAHIP_EINVAL, "%s: null pointer", who);
    if (ma <= 0 || nb1 <= 0 || nb2 < 0 || B <= 0 || HW <= 0) return fail(NCAHIP_EINVAL, "%s: bad size", who);
    const int nb = nb1 + nb2;
    if (!nca_gram_bf16_fits(r, ma, nb)) return fail(NCAHIP_ERANGE, "%s: ma=%d nb=%d outside (<=%d x <=%d)", who, ma, nb, r.ma, r.nb);
    if ((((uintptr_t)a | (uintptr_t)b1) & 1) != 0 || (((uintptr_t)b2 | (uintptr_t)out | (uintptr_t)workspace) & 3) != 0)
        return fail(NCAHIP_ERANGE, "%s: misaligned pointer (bf16: 2 bytes; fp32 and workspace: 4 bytes)", who);
    if (workspace_bytes < gram_rows_bf16_query(r, ma, nb, B, HW)) return fail(NCAHIP_EINVAL, "%s: workspace too small", who);
    // one launcher for both ranges: inside the narrow one it IS nca_launch_gram_rows_bf16
    return hip_result(nca_launch_gram_rows_bf16_wide(a, ma, b1, nb1, b2, nb2, B, HW, out, (float*)workspace, (hipStream_t)stream, accumulate != 0), who);
}

size_t dynca_step_bwd_bfmma_query(const DyncaStepBwd& v, int B, int C, int H, int W, int fc) {
    if (!dims_ok(B, C, H, W) || fc <= 0 || !dynca_bwd_mlp_range_ok(v.mma, C, fc)) return 0;
    return (size_t)nca_dynca_bwd_grid_c(B, C, H, W) * ((size_t)C * fc + C) * sizeof(float);
}

int dynca_step_bwd_bfmma_impl(const DyncaStepBwd& v, const float* x_t, const float* cond, const float* u, const float* w1, const float* b1,
                              const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                              float update_rate, uint64_t seed, uint64_t step, const float* g_next, float* g_x,
                              uint16_t* y_out, uint16_t* dh_out, float* dy_scratch, float* gw2_out, int accumulate,
                              void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    NcaDyncaArgs a{x_t, nullptr, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step,
                   g_next, nullptr, reinterpret_cast<float*>(dh_out), dy_scratch, g_x};
    a.gw2_ws = (float*)workspace;
    a.ybuf = reinterpret_cast<float*>(y_out);
    a.u_bits = u_is_bits(u, seed);
    if (int rc = dynca_step_bwd_checks(v, !g_next || !g_x || !y_out || !dh_out || !dy_scratch || !gw2_out || !workspace, a)) return rc;
    if (workspace_bytes < dynca_step_bwd_bfmma_query(v, B, C, H, W, fc)) return fail(NCAHIP_EINVAL, "%s: workspace too small", v.who);
    if (((uintptr_t)workspace & 3) != 0 || (((uintptr_t)y_out | (uintptr_t)dh_out) & 1) != 0)
        return fail(NCAHIP_ERANGE, "%s: misaligned workspace (4 bytes) or bf16 output (2 bytes)", v.who);
    if (int rc = check_bits(a.u_bits, B, H, W, update_rate, true)) return rc;
    if (int rc = hip_result(dynca_bwd_mlp_bf16(a, (hipStream_t)stream), v.label)) return rc;
    if (int rc = hip_result(nca_launch_dynca_step_bwd_stencil(a, (hipStream_t)stream), v.label, " stencil")) return rc;
    return hip_result(nca_launch_reduce_rows((const float*)workspace, gw2_out, nca_dynca_bwd_grid_c(B, C, H, W), C * fc + C,
                                             (hipStream_t)stream, accumulate != 0), v.label, " reduce");
}
}  // namespace

size_t ncahip_gram_rows_bf16_workspace(int ma, int nb, int B, int HW) { return gram_rows_bf16_query(kNcaGramBf, ma, nb, B, HW); }
int ncahip_gram_rows_bf16(const uint16_t* a, int ma, const uint16_t* b1, int nb1, const float* b2, int nb2, int B, int HW,
                          float* out, int accumulate, void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    return gram_rows_bf16_impl("gram_rows_bf16", kNcaGramBf, a, ma, b1, nb1, b2, nb2, B, HW, out, accumulate, workspace, workspace_bytes, stream);
}

size_t ncahip_dynca_step_bwd_bfmma_workspace(int B, int C, int H, int W, int fc) { return dynca_step_bwd_bfmma_query(kStepBwdBfmma, B, C, H, W, fc); }
int ncahip_dynca_step_bwd_bfmma_f32(const float* x_t, const float* cond, const float* u, const float* w1, const float* b1,
                                    const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                    float update_rate, uint64_t seed, uint64_t step, const float* g_next, float* g_x,
                                    uint16_t* y_out, uint16_t* dh_out, float* dy_scratch, float* gw2_out, int accumulate,
                                    void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    return dynca_step_bwd_bfmma_impl(kStepBwdBfmma, x_t, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step, g_next, g_x,
                                     y_out, dh_out, dy_scratch, gw2_out, accumulate, workspace, workspace_bytes, stream);
}

size_t ncahip_dynca_nsteps_bwd_bfmma_workspace(int B, int C, int H, int W, int fc, int c_cond) { return dynca_nsteps_bwd_query(kBwdBfmma, B, C, H, W, fc, c_cond); }
size_t ncahip_dynca_nsteps_bwd_ms_bfmma_workspace(int B, int C, int H, int W, int fc, int c_cond) { return dynca_nsteps_bwd_query(kBwdMsBfmma, B, C, H, W, fc, c_cond); }
int ncahip_dynca_nsteps_bwd_bfmma_f32(const float* states, int T, const float* cond, const float* u, const float* w1, const float* b1,
                                      const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                      float update_rate, uint64_t seed, uint64_t step0, const float* g_final, const float* g_states,
                                      float* g_x0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                                      size_t workspace_bytes, ncahip_stream_t stream) {
    return dynca_nsteps_bwd_impl(kBwdBfmma, states, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0, g_final,
                                 g_states, g_x0, g_w1, g_b1, g_w2, g_b2, workspace, workspace_bytes, stream);
}
int ncahip_dynca_nsteps_bwd_ms_bfmma_f32(const float* states, int T, const float* cond, const float* u, const float* w1, const float* b1,
                                         const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                         float update_rate, uint64_t seed, uint64_t step0, const float* g_final, const float* g_states,
                                         float* g_x0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                                         size_t workspace_bytes, ncahip_stream_t stream) {
    return dynca_nsteps_bwd_impl(kBwdMsBfmma, states, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0, g_final,
                                 g_states, g_x0, g_w1, g_b1, g_w2, g_b2, workspace, workspace_bytes, stream);
}

// ---- the wide range of the bf16-MFMA training mode (C <= 32, fc <= 256, single-scale): a narrow shape runs the narrow path -----------
size_t ncahip_gram_rows_bf16_wide_workspace(int ma, int nb, int B, int HW) { return gram_rows_bf16_query(kNcaGramBfWide, ma, nb, B, HW); }
int ncahip_gram_rows_bf16_wide(const uint16_t* a, int ma, const uint16_t* b1, int nb1, const float* b2, int nb2, int B, int HW,
                               float* out, int accumulate, void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    return gram_rows_bf16_impl("gram_rows_bf16_wide", kNcaGramBfWide, a, ma, b1, nb1, b2, nb2, B, HW, out, accumulate, workspace, workspace_bytes, stream);
}

size_t ncahip_dynca_step_bwd_bfmma_wide_workspace(int B, int C, int H, int W, int fc) { return dynca_step_bwd_bfmma_query(kStepBwdBfmmaWide, B, C, H, W, fc); }
int ncahip_dynca_step_bwd_bfmma_wide_f32(const float* x_t, const float* cond, const float* u, const float* w1, const float* b1,
                                         const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                         float update_rate, uint64_t seed, uint64_t step, const float* g_next, float* g_x,
                                         uint16_t* y_out, uint16_t* dh_out, float* dy_scratch, float* gw2_out, int accumulate,
                                         void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    const DyncaStepBwd& v = nca_dynca_bf16_shape_ok(C, fc) ? kStepBwdBfmma : kStepBwdBfmmaWide;   // the narrow range: the narrow entry point, its kernels and its refusals
    return dynca_step_bwd_bfmma_impl(v, x_t, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step, g_next, g_x,
                                     y_out, dh_out, dy_scratch, gw2_out, accumulate, workspace, workspace_bytes, stream);
}

// a narrow shape is inside the wide range and runs the narrow kernels: then exactly ncahip_dynca_nsteps_bwd_bfmma_f32
size_t ncahip_dynca_nsteps_bwd_bfmma_wide_workspace(int B, int C, int H, int W, int fc, int c_cond) { return dynca_nsteps_bwd_query(kBwdBfmmaWide, B, C, H, W, fc, c_cond); }
int ncahip_dynca_nsteps_bwd_bfmma_wide_f32(const float* states, int T, const float* cond, const float* u, const float* w1, const float* b1,
                                           const float* w2, const float* b2, int B, int C, int H, int W, int fc, int c_cond, int pad_mode,
                                           float update_rate, uint64_t seed, uint64_t step0, const float* g_final, const float* g_states,
                                           float* g_x0, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                                           size_t workspace_bytes, ncahip_stream_t stream) {
    return dynca_nsteps_bwd_impl(kBwdBfmmaWide, states, T, cond, u, w1, b1, w2, b2, B, C, H, W, fc, c_cond, pad_mode, update_rate, seed, step0, g_final,
                                 g_states, g_x0, g_w1, g_b1, g_w2, g_b2, workspace, workspace_bytes, stream);
}

// ---- relaxed-EMD part of the OT appearance loss (nca_ot.hip) ---------------------------------------------------------
namespace {
constexpr int kOtMaxC = 512, kOtMaxN = 1024, kOtMaxB = 65535;
int check_ot(const char* what, int B, int N, int c) {
    if (B <= 0) return fail(NCAHIP_EINVAL, "%s: bad size B=%d", what, B);
    if (c <= 0 || (c & 3) != 0 || c > kOtMaxC) return fail(NCAHIP_ERANGE, "%s: c=%d must be a multiple of 4 in [4, %d]", what, c, kOtMaxC);
    if (N < 1 || N > kOtMaxN) return fail(NCAHIP_ERANGE, "%s: N=%d outside [1, %d]", what, N, kOtMaxN);
    if (B > kOtMaxB) return fail(NCAHIP_ERANGE, "%s: B=%d exceeds %d", what, B, kOtMaxB);
    return 0;
}
bool ot_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }
}  // namespace

size_t ncahip_ot_workspace(int B, int N, int c) {
    if (B <= 0 || B > kOtMaxB || N < 1 || N > kOtMaxN || c <= 0 || (c & 3) != 0 || c > kOtMaxC) return 0;
    return (size_t)nca_ot_bands(N) * B * N * (sizeof(float) + sizeof(int32_t));
}

int ncahip_ot_gather_f32(const float* t, const float* g, const int32_t* idx, float* x, float* y, float* xn, float* yn, int B, int c,
                         int HW, int N, ncahip_stream_t stream) {
    if (!t || !g || !x || !y || !xn || !yn) return fail(NCAHIP_EINVAL, "ot_gather: null pointer");
    if (int rc = check_ot("ot_gather", B, N, c)) return rc;
    if (HW < N || (size_t)B * c * HW >= ((size_t)1 << 40)) return fail(NCAHIP_EINVAL, "ot_gather: bad size HW=%d (N=%d positions)", HW, N);
    if (!idx && N != HW) return fail(NCAHIP_EINVAL, "ot_gather: idx == NULL means every position (N == HW), got N=%d HW=%d", N, HW);
    if (x == y || (const float*)x == t || (const float*)x == g || (const float*)y == t || (const float*)y == g || xn == yn)
        return fail(NCAHIP_EINVAL, "ot_gather: outputs must not alias each other or the inputs");
    return hip_result(nca_launch_ot_gather(t, g, idx, x, y, xn, yn, B, c, HW, N, (hipStream_t)stream), "ot_gather");
}

int ncahip_ot_gather_bwd_f32(const float* dy, const int32_t* idx, float* dg, int B, int c, int HW, int N, ncahip_stream_t stream) {
    if (!dy || !dg) return fail(NCAHIP_EINVAL, "ot_gather_bwd: null pointer");
    if (int rc = check_ot("ot_gather_bwd", B, N, c)) return rc;
    if (HW < N || (size_t)B * c * HW >= ((size_t)1 << 40)) return fail(NCAHIP_EINVAL, "ot_gather_bwd: bad size HW=%d (N=%d positions)", HW, N);
    if (!idx && N != HW) return fail(NCAHIP_EINVAL, "ot_gather_bwd: idx == NULL means every position (N == HW), got N=%d HW=%d", N, HW);
    if (dy == dg) return fail(NCAHIP_EINVAL, "ot_gather_bwd: dy and dg must not alias");
    return hip_result(nca_launch_ot_scatter(dy, idx, dg, B, c, HW, N, (hipStream_t)stream), "ot_gather_bwd");
}

int ncahip_ot_remd_fwd_f32(const float* x, const float* y, const float* xn, const float* yn, float* rmin, int32_t* rarg, float* cmin,
                           int32_t* carg, float* remd, int32_t* branch, int B, int N, int c, void* workspace, size_t workspace_bytes,
                           ncahip_stream_t stream) {
    if (!x || !y || !xn || !yn || !rmin || !rarg || !cmin || !carg || !remd || !branch || !workspace)
        return fail(NCAHIP_EINVAL, "ot_remd_fwd: null pointer");
    if (int rc = check_ot("ot_remd_fwd", B, N, c)) return rc;
    if (rmin == cmin || rarg == carg || (const float*)rmin == xn || (const float*)rmin == yn || (const float*)cmin == xn || (const float*)cmin == yn)
        return fail(NCAHIP_EINVAL, "ot_remd_fwd: outputs must not alias each other or the norms");
    if (!ot_aligned(x) || !ot_aligned(y) || !ot_aligned(workspace)) return fail(NCAHIP_ERANGE, "ot_remd_fwd: x, y and workspace must be 16-byte aligned");
    if (workspace_bytes < ncahip_ot_workspace(B, N, c)) return fail(NCAHIP_EINVAL, "ot_remd_fwd: workspace too small");
    return hip_result(nca_launch_ot_remd_fwd(x, y, xn, yn, rmin, rarg, cmin, carg, remd, branch, B, N, c, workspace, (hipStream_t)stream), "ot_remd_fwd");
}

int ncahip_ot_remd_bwd_f32(const float* x, const float* y, const float* xn, const float* yn, const int32_t* rarg, const int32_t* carg,
                           const int32_t* branch, const float* g_remd, float* dy, int B, int N, int c, ncahip_stream_t stream) {
    if (!x || !y || !xn || !yn || !rarg || !carg || !branch || !g_remd || !dy) return fail(NCAHIP_EINVAL, "ot_remd_bwd: null pointer");
    if (int rc = check_ot("ot_remd_bwd", B, N, c)) return rc;
    if ((const float*)dy == x || (const float*)dy == y) return fail(NCAHIP_EINVAL, "ot_remd_bwd: dy must not alias x or y");
    if (!ot_aligned(x) || !ot_aligned(y) || !ot_aligned(dy)) return fail(NCAHIP_ERANGE, "ot_remd_bwd: x, y and dy must be 16-byte aligned");
    return hip_result(nca_launch_ot_remd_bwd(x, y, xn, yn, rarg, carg, branch, g_remd, dy, B, N, c, (hipStream_t)stream), "ot_remd_bwd");
}

// ---- moment-matching part of the OT appearance loss (nca_ot_moment.hip) ------------------------------------------------
namespace {
int check_ot_moment(const char* what, int B, int N, int c) {
    if (int rc = check_ot(what, B, N, c)) return rc;
    if (N < 2) return fail(NCAHIP_ERANGE, "%s: N=%d outside [2, %d] (the unbiased covariance divides by N - 1)", what, N, kOtMaxN);
    return 0;
}
}  // namespace

size_t ncahip_ot_moment_workspace(int B, int N, int c) {
    if (B <= 0 || B > kOtMaxB || N < 2 || N > kOtMaxN || c <= 0 || (c & 3) != 0 || c > kOtMaxC) return 0;
    const int nt = nca_ot_moment_tiles(c);
    return (size_t)B * (c + nt + nt * (nt + 1) / 2) * sizeof(float);
}

int ncahip_ot_moment_fwd_f32(const float* x, const float* y, float* mom, float* my, float* sgn, int8_t* S, int B, int N, int c,
                             void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    if (!x || !y || !mom || !my || !sgn || !S || !workspace) return fail(NCAHIP_EINVAL, "ot_moment_fwd: null pointer");
    if (int rc = check_ot_moment("ot_moment_fwd", B, N, c)) return rc;
    const void* const in[2] = {x, y};
    const void* const out[5] = {mom, my, sgn, S, workspace};
    for (int a = 0; a < 5; ++a) {
        for (int k = 0; k < 2; ++k)
            if (out[a] == in[k]) return fail(NCAHIP_EINVAL, "ot_moment_fwd: outputs must not alias the inputs");
        for (int k = a + 1; k < 5; ++k)
            if (out[a] == out[k]) return fail(NCAHIP_EINVAL, "ot_moment_fwd: outputs must not alias each other");
    }
    if (!ot_aligned(x) || !ot_aligned(y) || !ot_aligned(my) || !ot_aligned(sgn) || !ot_aligned(S) || !ot_aligned(workspace))
        return fail(NCAHIP_ERANGE, "ot_moment_fwd: x, y, my, sgn, S and workspace must be 16-byte aligned");
    if (workspace_bytes < ncahip_ot_moment_workspace(B, N, c)) return fail(NCAHIP_EINVAL, "ot_moment_fwd: workspace too small");
    return hip_result(nca_launch_ot_moment_fwd(x, y, mom, my, sgn, (signed char*)S, B, N, c, workspace, (hipStream_t)stream), "ot_moment_fwd");
}

int ncahip_ot_moment_bwd_f32(const float* y, const float* my, const float* sgn, const int8_t* S, const float* g_mom, float* dy, int B, int N,
                             int c, ncahip_stream_t stream) {
    if (!y || !my || !sgn || !S || !g_mom || !dy) return fail(NCAHIP_EINVAL, "ot_moment_bwd: null pointer");
    if (int rc = check_ot_moment("ot_moment_bwd", B, N, c)) return rc;
    if ((const float*)dy == y || (const float*)dy == my || (const float*)dy == sgn || (const void*)dy == (const void*)S || (const float*)dy == g_mom)
        return fail(NCAHIP_EINVAL, "ot_moment_bwd: dy must not alias an input");
    if (!ot_aligned(y) || !ot_aligned(my) || !ot_aligned(S) || !ot_aligned(dy))
        return fail(NCAHIP_ERANGE, "ot_moment_bwd: y, my, S and dy must be 16-byte aligned");
    return hip_result(nca_launch_ot_moment_bwd(y, my, sgn, (const signed char*)S, g_mom, dy, B, N, c, (hipStream_t)stream), "ot_moment_bwd");
}

// ---- position sampler of the OT appearance loss (nca_ot_sample.hip) ------------------------------------------------------
int ncahip_ot_sample_idx(int32_t* idx, int rows, int HW, int n, uint64_t seed, uint64_t row0, int key_bits, ncahip_stream_t stream) {
    constexpr int kSmpMaxHW = 1 << 20;
    if (!idx) return fail(NCAHIP_EINVAL, "ot_sample_idx: null pointer");
    if (rows <= 0 || HW <= 0 || n <= 0) return fail(NCAHIP_EINVAL, "ot_sample_idx: bad size rows=%d HW=%d n=%d", rows, HW, n);
    if (n > HW) return fail(NCAHIP_EINVAL, "ot_sample_idx: n=%d exceeds HW=%d (positions are drawn without replacement)", n, HW);
    if (key_bits < 1 || key_bits > 32) return fail(NCAHIP_EINVAL, "ot_sample_idx: key_bits=%d outside [1, 32]", key_bits);
    if (n > kOtMaxN) return fail(NCAHIP_ERANGE, "ot_sample_idx: n=%d outside [1, %d]", n, kOtMaxN);
    if (HW > kSmpMaxHW) return fail(NCAHIP_ERANGE, "ot_sample_idx: HW=%d exceeds %d", HW, kSmpMaxHW);
    if (rows > kOtMaxB) return fail(NCAHIP_ERANGE, "ot_sample_idx: rows=%d exceeds %d", rows, kOtMaxB);
    if (int rc = device_error_rc("ot_sample_idx")) return rc;
    return hip_result(nca_launch_ot_sample(idx, rows, HW, n, seed, row0, key_bits, (hipStream_t)stream), "ot_sample_idx");
}

// ---- sliced-Wasserstein style loss (nca_slw.hip) -------------------------------------------------------------------------
namespace {
constexpr int kSlwMaxC = 512, kSlwMaxLen = 65536, kSlwMaxB = 1024, kSlwMaxRows = 65535, kSlwDirs = 32;
bool slw_c_ok(int c) { return c == 3 || (c >= 4 && (c & 3) == 0 && c <= kSlwMaxC); }
int check_slw(const char* what, int B, int c, int n, int m) {
    if (B <= 0) return fail(NCAHIP_EINVAL, "%s: bad size B=%d", what, B);
    if (B > kSlwMaxB) return fail(NCAHIP_ERANGE, "%s: B=%d exceeds %d", what, B, kSlwMaxB);
    if (!slw_c_ok(c)) return fail(NCAHIP_ERANGE, "%s: c=%d must be 3 or a multiple of 4 in [4, %d]", what, c, kSlwMaxC);
    if (n < 1 || n > kSlwMaxLen) return fail(NCAHIP_ERANGE, "%s: n=%d outside [1, %d]", what, n, kSlwMaxLen);
    if (m < 1 || m > kSlwMaxLen) return fail(NCAHIP_ERANGE, "%s: m=%d outside [1, %d]", what, m, kSlwMaxLen);
    return 0;
}
}  // namespace

size_t ncahip_slw_workspace(int B, int c, int n, int m) {
    if (B <= 0 || B > kSlwMaxB || !slw_c_ok(c) || n < 1 || n > kSlwMaxLen || m < 1 || m > kSlwMaxLen) return 0;
    const size_t dk = (size_t)B * kSlwDirs * n, part = (size_t)B * kSlwDirs * nca_slw_blocks(n) + B;   // the backward's dk; the forward's partials
    return (dk > part ? dk : part) * sizeof(float);
}

int ncahip_slw_project_f32(const float* source, const float* target, const float* proj, float* ks, float* kt, int B, int c, int n, int m,
                           ncahip_stream_t stream) {
    if (!source || !target || !proj || !ks || !kt) return fail(NCAHIP_EINVAL, "slw_project: null pointer");
    if (int rc = check_slw("slw_project", B, c, n, m)) return rc;
    if (ks == kt || (const float*)ks == source || (const float*)ks == target || (const float*)ks == proj || (const float*)kt == source ||
        (const float*)kt == target || (const float*)kt == proj)
        return fail(NCAHIP_EINVAL, "slw_project: outputs must not alias each other or the inputs");
    if (!ot_aligned(source) || !ot_aligned(target) || !ot_aligned(proj))
        return fail(NCAHIP_ERANGE, "slw_project: source, target and proj must be 16-byte aligned");
    return hip_result(nca_launch_slw_project(source, target, proj, ks, kt, B, c, n, m, (hipStream_t)stream), "slw_project");
}

int ncahip_slw_sort_f32(float* keys, int32_t* perm, int rows, int n, ncahip_stream_t stream) {
    if (!keys || !perm) return fail(NCAHIP_EINVAL, "slw_sort: null pointer");
    if (rows <= 0) return fail(NCAHIP_EINVAL, "slw_sort: bad size rows=%d", rows);
    if (rows > kSlwMaxRows) return fail(NCAHIP_ERANGE, "slw_sort: rows=%d exceeds %d", rows, kSlwMaxRows);
    if (n < 1 || n > kSlwMaxLen) return fail(NCAHIP_ERANGE, "slw_sort: n=%d outside [1, %d]", n, kSlwMaxLen);
    if ((void*)keys == (void*)perm) return fail(NCAHIP_EINVAL, "slw_sort: keys and perm must not alias");
    return hip_result(nca_launch_slw_sort(keys, perm, rows, n, (hipStream_t)stream), "slw_sort");
}

int ncahip_slw_loss_fwd_f32(const float* s, const float* t, const int32_t* jmap, float* loss, int B, int n, int m, void* workspace,
                            size_t workspace_bytes, ncahip_stream_t stream) {
    if (!s || !t || !jmap || !loss || !workspace) return fail(NCAHIP_EINVAL, "slw_loss_fwd: null pointer");
    if (int rc = check_slw("slw_loss_fwd", B, 4, n, m)) return rc;
    if ((void*)loss == (void*)s || (void*)loss == (void*)t || (void*)loss == (void*)jmap || workspace == (void*)s || workspace == (void*)t ||
        workspace == (void*)jmap || workspace == (void*)loss)
        return fail(NCAHIP_EINVAL, "slw_loss_fwd: loss and workspace must not alias each other or the inputs");
    if (((uintptr_t)workspace & 3u) != 0) return fail(NCAHIP_ERANGE, "slw_loss_fwd: workspace must be 4-byte aligned");
    if (workspace_bytes < ncahip_slw_workspace(B, 4, n, m)) return fail(NCAHIP_EINVAL, "slw_loss_fwd: workspace too small");
    return hip_result(nca_launch_slw_loss_fwd(s, t, jmap, loss, B, n, m, workspace, (hipStream_t)stream), "slw_loss_fwd");
}

int ncahip_slw_bwd_f32(const float* s, const float* t, const int32_t* jmap, const int32_t* perm, const float* proj, const float* g_loss,
                       float* dsource, int B, int c, int n, int m, void* workspace, size_t workspace_bytes, ncahip_stream_t stream) {
    if (!s || !t || !jmap || !perm || !proj || !g_loss || !dsource || !workspace) return fail(NCAHIP_EINVAL, "slw_bwd: null pointer");
    if (int rc = check_slw("slw_bwd", B, c, n, m)) return rc;
    const void* const in[6] = {s, t, jmap, perm, proj, g_loss};
    for (int k = 0; k < 6; ++k)
        if (in[k] == (const void*)dsource || in[k] == (const void*)workspace)
            return fail(NCAHIP_EINVAL, "slw_bwd: dsource and workspace must not alias an input");
    if ((void*)dsource == workspace) return fail(NCAHIP_EINVAL, "slw_bwd: dsource and workspace must not alias each other");
    if (((uintptr_t)workspace & 3u) != 0) return fail(NCAHIP_ERANGE, "slw_bwd: workspace must be 4-byte aligned");
    if (workspace_bytes < ncahip_slw_workspace(B, c, n, m)) return fail(NCAHIP_EINVAL, "slw_bwd: workspace too small");
    return hip_result(nca_launch_slw_bwd(s, t, jmap, perm, proj, g_loss, dsource, B, c, n, m, workspace, (hipStream_t)stream), "slw_bwd");
}

size_t ncahip_cond_grow_bwd_workspace(int B, int C, int H, int W, int hidden) {
    if (!dims_ok(B, C, H, W) || hidden <= 0) return 0;
    const size_t n = (size_t)B * C * H * W * sizeof(float);
    return 4 * align256(n) + align256(3 * n) +
           align256((size_t)(nca_cond_bwd_nslab() + 1) * nca_cond_bwd_slab_floats(C, hidden) * sizeof(float)) +
           align256((size_t)nca_cond_bwd_nblk(B, C, H, W) * 27 * sizeof(float)) +
           align256(nca_cond_bwd_fm_pscr_bytes(B, C, H, W)) + align256(nca_cond_bwd_fm_doscr_bytes(B, C, H, W)) + align256(kNcaCondBwdOpimgBytes);
}

// states / goal: fp32 or bf16 (sb = bytes per element); everything else fp32
static int cond_grow_bwd_impl(const void* states_v, int sb, const uint8_t* pre, int T, const void* goal_v, int goal_ch,
                              const float* u, const float* wp, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* w3, int B, int C, int H, int W, int hidden, int alive_ch,
                              float alive_thr, float fire_rate, float clamp_lo, float clamp_hi, uint64_t seed,
                              uint64_t step0, const float* g_final, float* g_x0, float* g_goal, float* g_wp, float* g_w1,
                              float* g_b1, float* g_w2, float* g_b2, float* g_w3, void* workspace, size_t workspace_bytes,
                              ncahip_stream_t stream) {
    const char* const states = (const char*)states_v;
    const bool bf16 = sb == 2;
    if (T < 1 || !states || !pre || !g_final || !g_x0 || !g_wp || !g_w1 || !g_b1 || !g_w2 || !g_b2 || !g_w3 || !workspace)
        return fail(NCAHIP_EINVAL, "cond grow bwd: null pointer or T < 1");
    // fp32 history: C <= 32 (16 < C <= 32 on the front + matrix kernels); bf16 history: C <= 20 (as the bf16 forward)
    if (int rc = check_cond(states, g_x0, pre, goal_v, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, goal_ch, alive_ch, bf16 ? kMaxCCondFwdBf16 : kMaxCCondFwd)) return rc;
    if (goal_ch > 0 && !g_goal) return fail(NCAHIP_EINVAL, "cond grow bwd: g_goal required when goal_ch > 0");
    const uintptr_t amask = bf16 ? 7 : 15;   // state-type tensors: 4-cell groups (16 bytes fp32, 8 bytes bf16)
    if (W % 4 != 0 || (((uintptr_t)states | (uintptr_t)goal_v) & amask) != 0 ||
        ((uintptr_t)g_final | (uintptr_t)g_x0 | (uintptr_t)workspace) % 16 != 0)
        return fail(NCAHIP_ERANGE, "cond grow bwd: needs W %% 4 == 0 and 16-byte aligned buffers (8-byte for bf16 states / goal)");
    if ((size_t)H * W >= ((size_t)1 << 24) || (size_t)(C > 16 ? C : 16) * H * W * 4 >= ((size_t)1 << 32))
        return fail(NCAHIP_ERANGE, "cond grow bwd: grid too large for the tile kernels' 32-bit addressing (H*W < 2^24)");
    if (workspace_bytes < ncahip_cond_grow_bwd_workspace(B, C, H, W, hidden))
        return fail(NCAHIP_EINVAL, "cond grow bwd: workspace too small");
    const bool ubits = u_is_bits(u, seed);
    if (int rc = check_bits(ubits, B, H, W, fire_rate, false)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t slot = (size_t)B * C * H * W, pslot = (size_t)B * H * W, nb = slot * sizeof(float);
    if (bf16 && (slot * 2) % 8 != 0) return fail(NCAHIP_ERANGE, "cond grow bwd (bf16): state slots must stay 8-byte aligned");
    char* p = (char*)workspace;
    float* gbuf[2] = {(float*)p, (float*)(p + align256(nb))};
    p += 2 * align256(nb);
    float* gx = (float*)p; p += align256(nb);
    float* zbuf = (float*)p; p += align256(nb);
    float* dP = (float*)p; p += align256(3 * nb);
    const int nslab = nca_cond_bwd_nslab(), sf = nca_cond_bwd_slab_floats(C, hidden), nblk = nca_cond_bwd_nblk(B, C, H, W);
    float* slabs = (float*)p;
    float* red = slabs + (size_t)nslab * sf;  // one extra slab: the reduced gradients
    p += align256((size_t)(nslab + 1) * sf * sizeof(float));
    float* wpp = (float*)p; p += align256((size_t)nblk * 27 * sizeof(float));
    void* pscr = p; p += align256(nca_cond_bwd_fm_pscr_bytes(B, C, H, W));   // front kernel -> matrix kernel scratch (operand order)
    void* doscr = p; p += align256(nca_cond_bwd_fm_doscr_bytes(B, C, H, W));
    float* opimg = (float*)p;   // the matrix kernel's operand image, built once per call (the weights do not change between the steps)
    hipError_t e = nca_zero_async(slabs, (size_t)nslab * sf, st);
    if (e == hipSuccess) e = nca_zero_async(wpp, (size_t)nblk * 27, st);
    if (e == hipSuccess && goal_ch > 0) e = nca_zero_async(g_goal, (size_t)B * goal_ch * H * W, st);
    if (e != hipSuccess) return hip_result(e, "cond grow bwd memset");
    const float* gcur = g_final;
    auto step_args = [&](int t, const float* g_in) {
        NcaCondBwdArgs ba{};
        ba.f = NcaCondArgs{reinterpret_cast<const float*>(states + (size_t)t * slot * sb), t == 0 ? nullptr : pre + (size_t)t * pslot,
                           nullptr, nullptr, reinterpret_cast<const float*>(goal_v),
                           u_at(u, ubits, t, pslot), wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, goal_ch,
                           alive_ch, alive_thr, fire_rate, clamp_lo, clamp_hi, seed, step0 + (uint64_t)t, nullptr};
        ba.f.u_bits = ubits;
        ba.x_next = reinterpret_cast<const float*>(states + (size_t)(t + 1) * slot * sb);
        ba.pre_t = pre + (size_t)(t + 1) * pslot;
        ba.g_next = g_in;
        ba.g_out = t == 0 ? g_x0 : gbuf[t & 1];
        ba.gx = gx; ba.dP = dP; ba.zbuf = zbuf; ba.dgoal = g_goal; ba.slabs = slabs; ba.wp_partials = wpp;
        ba.nslab = nslab; ba.nblk = nblk;
        ba.pscr = pscr; ba.doscr = doscr;
        ba.opimg = opimg;
        return ba;
    };
    // The weights do not change between the steps: in the front + matrix form ONE workgroup builds the matrix kernel's operand image
    // (opmode 1, no tile work) and the T step launches copy it (opmode 2) instead of gathering it again each (~6 us per launch).
    int opmode = 0;
    if (T >= 2) {
        NcaCondBwdArgs pa = step_args(T - 1, gcur);
        if (nca_cond_bwd_is_fm(pa, bf16)) {
            pa.opmode = 1;
            if (int rc = hip_result(nca_launch_cond_step_bwd(pa, st, bf16), "cond_grow_bwd operand image")) return rc;
            opmode = 2;
        }
    }
    for (int t = T - 1; t >= 0; --t) {
        NcaCondBwdArgs ba = step_args(t, gcur);
        ba.opmode = opmode;
        if (int rc = hip_result(nca_launch_cond_step_bwd(ba, st, bf16), "cond_grow_bwd step")) return rc;
        gcur = ba.g_out;
    }
    // slabs -> one summed slab (tile-major) -> gradients in the reference layouts
    if (int rc = hip_result(nca_launch_reduce_rows(slabs, red, nslab, sf, st), "cond_grow_bwd reduce")) return rc;
    if (int rc = hip_result(nca_launch_cond_bwd_unpermute(red, C, hidden, bf16, g_w1, g_w2, g_w3, g_b1, g_b2, st), "cond_grow_bwd unpermute")) return rc;
    return hip_result(nca_launch_reduce_wp(wpp, g_wp, B, C, H, W, st), "cond_grow_bwd reduce wp");
}

int ncahip_cond_grow_bwd_f32(const float* states, const uint8_t* pre, int T, const float* goal, int goal_ch,
                             const float* u, const float* wp, const float* w1, const float* b1, const float* w2,
                             const float* b2, const float* w3, int B, int C, int H, int W, int hidden, int alive_ch,
                             float alive_thr, float fire_rate, float clamp_lo, float clamp_hi, uint64_t seed,
                             uint64_t step0, const float* g_final, float* g_x0, float* g_goal, float* g_wp, float* g_w1,
                             float* g_b1, float* g_w2, float* g_b2, float* g_w3, void* workspace, size_t workspace_bytes,
                             ncahip_stream_t stream) {
    return cond_grow_bwd_impl(states, 4, pre, T, goal, goal_ch, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, alive_ch, alive_thr,
                              fire_rate, clamp_lo, clamp_hi, seed, step0, g_final, g_x0, g_goal, g_wp, g_w1, g_b1, g_w2, g_b2,
                              g_w3, workspace, workspace_bytes, stream);
}

int ncahip_cond_grow_bwd_bf16(const uint16_t* states, const uint8_t* pre, int T, const uint16_t* goal, int goal_ch,
                              const float* u, const float* wp, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* w3, int B, int C, int H, int W, int hidden, int alive_ch,
                              float alive_thr, float fire_rate, float clamp_lo, float clamp_hi, uint64_t seed,
                              uint64_t step0, const float* g_final, float* g_x0, float* g_goal, float* g_wp, float* g_w1,
                              float* g_b1, float* g_w2, float* g_b2, float* g_w3, void* workspace, size_t workspace_bytes,
                              ncahip_stream_t stream) {
    return cond_grow_bwd_impl(states, 2, pre, T, goal, goal_ch, u, wp, w1, b1, w2, b2, w3, B, C, H, W, hidden, alive_ch, alive_thr,
                              fire_rate, clamp_lo, clamp_hi, seed, step0, g_final, g_x0, g_goal, g_wp, g_w1, g_b1, g_w2, g_b2,
                              g_w3, workspace, workspace_bytes, stream);
}

int ncahip_pack_fire_mask_u32(const float* u, uint32_t* bits, int T, int B, int H, int W, float rate, int mode, ncahip_stream_t stream) {
    if (!u || !bits || T <= 0 || B <= 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1)) return fail(NCAHIP_EINVAL, "pack_fire_mask: bad argument");
    if (int rc = check_bits(true, B, H, W, rate, mode == 1)) return rc;
    return hip_result(nca_launch_pack_fire_mask(u, bits, T, (size_t)B * H * W, rate, mode, (hipStream_t)stream), "pack_fire_mask");
}

int ncahip_philox_uniform_f32(float* u, int B, int H, int W, uint64_t seed, uint64_t step, ncahip_stream_t stream) {
    if (!u || B <= 0 || H <= 0 || W <= 0) return fail(NCAHIP_EINVAL, "philox_uniform: bad argument");
    return hip_result(nca_launch_philox_uniform(u, B, H, W, seed, step, (hipStream_t)stream), "philox_uniform");
}

}  // extern "C"

// nca_dynca_fwd.hip -- the forward launchers of the fused DyNCA step; instantiates the forward variants of dynca_step_fwd_kernel
// (nca_dynca_step.h) and no other.
// Built only through nca_step.hip, which includes this file: never list it in the Makefile's SRCS beside that unit (duplicate symbols).
#include "nca_dynca_step.h"

hipError_t nca_launch_dynca_step_fwd(const NcaDyncaArgs& a, hipStream_t st, bool bf16_mfma) {
    const bool bf = bf16_mfma && nca_dynca_bf16_shape_ok(a.C, a.fc);   // ncahip_dynca_precision mode 1; shapes outside its range run exactly
    if (a.pc) {   // two-scale perception
        if ((a.H | a.W) & 1) return hipErrorInvalidValue;
        return bf ? dispatch_dynca<DyncaFwdMsBf, kDynca12x96, kDynca16x128>(a, st) : dispatch_dynca<DyncaFwdMs, kDynca12x96, kDynca16x128>(a, st);
    }
    if (bf) return dispatch_dynca<DyncaFwdBf, kDynca12x96, kDynca16x128>(a, st);
    if (a.fc <= 128) return dispatch_dynca<DyncaFwd, kDynca12x96, kDynca32x128>(a, st);
    if (a.C > 32) return hipErrorInvalidValue;
    // fc > 128: the A-operand image of w1 no longer fits the LDS beside the tile.  w2 relu(w1 y + b1) is a sum over hidden
    // units, so the step runs as one launch per 128-wide slice: the first writes x + mask*(slice + b2), the others add
    // their slice to x_out (same mask: same explicit uniforms / Philox key).  Each launch recomputes the perception.
    const int K1 = 4 * a.C + a.c_cond;
    for (int h0 = 0; h0 < a.fc; h0 += 128) {
        NcaDyncaArgs s = a;
        s.w1 = a.w1 + (size_t)h0 * K1;
        s.b1 = a.b1 + h0;
        s.w2 = a.w2 + h0;
        s.fc = a.fc - h0 < 128 ? a.fc - h0 : 128;
        s.w2_ld = a.fc;
        const hipError_t e = h0 == 0 ? dispatch_dynca<DyncaFwd, kDynca16x128, kDynca32x128>(s, st)
                                     : dispatch_dynca<DyncaFwdAcc, kDynca16x128, kDynca32x128>(s, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// bf16 state storage: x_in / x_out point at bf16 data (cond, uniforms, weights stay f32); same kernel, exact f32 compute,
// round-to-nearest-even on store.  The 8-byte vector path needs W % 4 == 0 and 8-byte aligned planes.
hipError_t nca_launch_dynca_step_fwd_bf16(const NcaDyncaArgs& a, hipStream_t st) {
    return dispatch_dynca<DyncaFwdB16, kDynca12x96, kDynca32x128>(a, st);
}

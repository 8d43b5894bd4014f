// nca_dynca_fwd.hip -- the forward launchers of the fused DyNCA step; instantiates the forward variants of dynca_step_fwd_kernel
// (nca_dynca_step.h) and no other.
// Built only through nca_step.hip, which includes this file: never list it in the Makefile's SRCS beside that unit (duplicate symbols).
#include "nca_dynca_step.h"

hipError_t nca_launch_dynca_step_fwd(const NcaDyncaArgs& a, hipStream_t st, bool bf16_mfma, bool bf16_wide) {
    if (a.dirs) return nca_launch_dynca_step_fwd_steered(a, st, bf16_mfma);   // a direction field attached: nca_dynca_steer.hip
    // ncahip_dynca_bf16_range 1: single-scale shapes beyond the narrow range, up to C = 32 / fc = 256 (nca_dynca_bf16_wide.hip)
    if (bf16_mfma && bf16_wide && !a.pc && !nca_dynca_bf16_shape_ok(a.C, a.fc) && nca_dynca_bf16_wide_shape_ok(a.C, a.fc))
        return nca_launch_dynca_step_fwd_bf16_wide(a, st);
    return launch_dynca_fwd_ladder<false>(a, st, bf16_mfma);
}

// bf16 state storage: x_in / x_out point at bf16 data (cond, uniforms, weights stay f32); same kernel, exact f32 compute,
// round-to-nearest-even on store.  The 8-byte vector path needs W % 4 == 0 and 8-byte aligned planes.
hipError_t nca_launch_dynca_step_fwd_bf16(const NcaDyncaArgs& a, hipStream_t st) {
    return dispatch_dynca<DyncaFwdB16, kDynca12x96, kDynca32x128>(a, st);
}

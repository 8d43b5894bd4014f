// nca_dynca_steer.hip -- the steered forward variants of the fused DyNCA step: DyncaSteered<V> of DyncaFwd, DyncaFwdBf, DyncaFwdMs,
// DyncaFwdMsBf and DyncaFwdAcc (nca_dynca_step.h), i.e. the kernels a launch with a direction field attached runs
// (ncahip_dynca_direction).  A unit of its own: it compiles beside nca_step.hip, whose kernels are what they were without it.
#include "nca_dynca_step.h"

hipError_t nca_launch_dynca_step_fwd_steered(const NcaDyncaArgs& a, hipStream_t st, bool bf16_mfma) {
    if (!a.dirs) return hipErrorInvalidValue;
    return launch_dynca_fwd_ladder<true>(a, st, bf16_mfma);
}

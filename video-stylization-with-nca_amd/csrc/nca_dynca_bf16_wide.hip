// nca_dynca_bf16_wide.hip -- the bf16-MFMA DyNCA forward step in its wide range (ncahip_dynca_bf16_range 1, include/ncahip.h): the
// variant DyncaFwdBf of dynca_step_fwd_kernel (nca_dynca_step.h) at the shape classes <32, 128>, <16, 256> and <32, 256>, with and
// without conditioning, vector and any-shape form.  Two output tiles and up to sixteen hidden tiles in ONE launch per step, one
// perception pass (NcaDyncaBf16::mlp_wide, nca_dynca_bf16.h).  A unit of its own, as the steered and the bf16-MFMA backward kernels
// are: it compiles beside nca_step.hip, whose kernels are what they were without it.  The ladder lives here and not in the header: a
// plain function there would instantiate these kernels in every unit that includes it.
#include "nca_dynca_step.h"

// Three classes beyond <16, 128>, smallest first; the whole hidden layer in one launch.  Only single-scale unsteered shapes outside
// the narrow range come here (nca_launch_dynca_step_fwd's test): C > 16 or fc > 128.
hipError_t nca_launch_dynca_step_fwd_bf16_wide(const NcaDyncaArgs& a, hipStream_t st) {
    if (!nca_dynca_bf16_wide_shape_ok(a.C, a.fc) || nca_dynca_bf16_shape_ok(a.C, a.fc) || a.pc || a.dirs || a.w2_ld) return hipErrorInvalidValue;
    if (a.fc <= 128) return launch_dynca_class<32, 128, DyncaFwdBf>(a, st);
    if (a.C <= 16) return launch_dynca_class<16, 256, DyncaFwdBf>(a, st);
    return launch_dynca_class<32, 256, DyncaFwdBf>(a, st);
}

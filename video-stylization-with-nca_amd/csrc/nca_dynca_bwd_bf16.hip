// nca_dynca_bwd_bf16.hip -- the MLP part of the DyNCA backward step in the "bf16-MFMA training" mode (include/ncahip.h): the variants
// DyncaBwdBf and DyncaBwdBfMs of dynca_step_fwd_kernel (nca_dynca_step.h) at the shape classes <12, 96> and <16, 128>, with and without
// conditioning, vector and any-shape form.  A unit of its own, as the steered kernels are: it compiles beside nca_step.hip, whose
// kernels are what they were without it.  The stencil adjoint, the two-scale adjoints and the reductions are the fp32 backward's.
#include "nca_dynca_step.h"

// Writes yb [B,4C,H,W] (a.ybuf) and dhb [B,fc,H,W] (a.dhbuf) as bf16, dL/dy (a.dybuf) as fp32 and the per-workgroup dW2 | db2 partials
// (a.gw2_ws: nca_dynca_bwd_grid_c / nca_dynca_bwd_ms_grid slabs).  C <= 16 and fc <= 128 only.
hipError_t nca_launch_dynca_step_bwd_mlp_bf16(const NcaDyncaArgs& a, hipStream_t st) {
    if (!nca_dynca_bf16_shape_ok(a.C, a.fc) || !a.gw2_ws || !a.ybuf || !a.dhbuf || !a.dybuf || !a.g_next) return hipErrorInvalidValue;
    if (a.pc) {
        if ((a.H | a.W) & 1) return hipErrorInvalidValue;
        return dispatch_dynca<DyncaBwdBfMs, kDynca12x96, kDynca16x128>(a, st);
    }
    return dispatch_dynca<DyncaBwdBf, kDynca12x96, kDynca16x128>(a, st);
}

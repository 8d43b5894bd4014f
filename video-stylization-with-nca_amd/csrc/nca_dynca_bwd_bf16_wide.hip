// nca_dynca_bwd_bf16_wide.hip -- the MLP part of the DyNCA backward step in the WIDE range of the "bf16-MFMA training" mode
// (include/ncahip.h: 1 <= C <= 32, 1 <= fc <= 256, single-scale): the variants DyncaBwdBfSl / DyncaBwdBfSlAcc of dynca_step_fwd_kernel
// (nca_dynca_step.h), with and without conditioning, vector and any-shape form.  A unit of its own, as nca_dynca_bwd_bf16.hip is: the
// kernels of the other units are what they were without it.
//
// One launch per 128-wide slice of the hidden layer, dL/dy accumulated from the second slice on ("DyNCA training
// on bf16 MFMA, the wide range": the W1, W1^T and W2^T images of a whole <32, 256> layer do not fit the LDS beside the state tile).
// The gate must be the forward's bit for bit, so every slice forms a1 with pack_y / layer1 of the channel class the FORWARD picked
// (nca_dynca_bf16_wide.hip); the hidden tiles of a class are independent and K1S, K1Q and the chunk order depend on CP alone:
//     forward <32, 128> (fc <= 128)            -> one slice  at <32, 128>
//     forward <16, 256> (C <= 16, fc > 128)    -> two slices at <16, 128>      (NOT <32, 128>: another K1Q)
//     forward <32, 256>                        -> two slices at <32, 128>
#include "nca_dynca_step.h"

// Writes yb [B,4C,H,W] (a.ybuf, first slice) and dhb [B,fc,H,W] (a.dhbuf) as bf16, dL/dy (a.dybuf) as fp32 and the per-workgroup
// dW2 | db2 partials in the layout of the whole layer (a.gw2_ws: nca_dynca_bwd_grid_c slabs of C*fc + C floats; every element of a slab is
// written by exactly one slice).  Shapes inside the wide and outside the narrow range only.
hipError_t nca_launch_dynca_step_bwd_mlp_bf16_wide(const NcaDyncaArgs& a, hipStream_t st) {
    if (!nca_dynca_bf16_wide_shape_ok(a.C, a.fc) || nca_dynca_bf16_shape_ok(a.C, a.fc) || a.pc || a.dirs) return hipErrorInvalidValue;
    if (!a.gw2_ws || !a.ybuf || !a.dhbuf || !a.dybuf || !a.g_next) return hipErrorInvalidValue;
    const int K1 = 4 * a.C + a.c_cond;
    const size_t plane = (size_t)a.H * a.W;
    for (int h0 = 0; h0 < a.fc; h0 += 128) {
        NcaDyncaArgs s = a;
        s.w1 = a.w1 + (size_t)h0 * K1;
        s.b1 = a.b1 + h0;
        s.w2 = a.w2 + h0;
        s.fc = a.fc - h0 < 128 ? a.fc - h0 : 128;
        s.w2_ld = a.fc;
        s.dhbuf = reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(a.dhbuf) + (size_t)h0 * plane);
        s.gw2_ws = a.gw2_ws + h0;
        hipError_t e;
        if (a.C <= 16) e = h0 == 0 ? launch_dynca_class<16, 128, DyncaBwdBfSl>(s, st) : launch_dynca_class<16, 128, DyncaBwdBfSlAcc>(s, st);
        else e = h0 == 0 ? launch_dynca_class<32, 128, DyncaBwdBfSl>(s, st) : launch_dynca_class<32, 128, DyncaBwdBfSlAcc>(s, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

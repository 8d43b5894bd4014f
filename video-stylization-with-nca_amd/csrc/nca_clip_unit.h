// nca_clip_unit.h -- ConditionedNCA's image value, shared by the emit kernels of nca_clip.hip and the fused finalize + image kernel of
// nca_cond_bf16.hip: one definition, so the two produce the same bits.
#pragma once
#include <hip/hip_runtime.h>

// img = clamp(x, 0, 1) as torch.clamp evaluates it on the device (EncoderConditioning/trainer.py:36-39): NaN passes through, then
// min(max(x, 0), 1)
__device__ __forceinline__ float clip_unit_value(float x) { return x != x ? x : fminf(fmaxf(x, 0.0f), 1.0f); }

// The head trunks' activation in the training kernels (head_sparse.hip, gram_heads.hip): InPlaceABN's leaky_relu(0.01) or, with
// MODEL.INPLACE_ABN False, ReLU.  The kernels take it as the slope below zero (wave-uniform), so that neither branches on `act`
// (train_kernels.hip bn_bwd's form: 1 above the threshold, `slope` below).
#pragma once
#include "common.h"

namespace mfx {

// 0.01 (ACT_LEAKY), 0 (ACT_RELU); the entry points refuse every other activation before they ask
inline float head_act_slope(int act) { return act == ACT_RELU ? 0.f : 0.01f; }

// slope 0.01: today's expression, bit for bit.  Slope 0: +0 for every z <= 0 (0 * z would be -0, and NaN for z = -inf), as torch's ReLU gives.
__device__ __forceinline__ float head_act(float z, float slope) { return z > 0.f ? z : (slope != 0.f ? slope * z : 0.f); }

// d act / d z: 1 for z > 0, `slope` otherwise (ReLU: 0 at z == 0, torch's threshold_backward)
__device__ __forceinline__ float head_act_grad(float z, float slope) { return z > 0.f ? 1.f : slope; }

}  // namespace mfx

// fleet_amd/csrc/descent_math.h -- the arithmetic of descentNative's model step
// (SURVEY.md §8 f1), shared by k_descent (kernels.hip) and the resident model's
// step (rmodel_kernels.hip): sgd::increment_w (commonLib/cppNN/solver.h:88-94,
// w -= lr*(dW + 0*w)) and update_bias (layer.h:241-243, b -= db*lr), each op one
// fp32 rounding as in the reference's SSE build (no contraction).
#pragma once
#include <hip/hip_runtime.h>

#include "codec_math.h"

namespace fleet {

// NaN results as the reference's x86 SSE build produces them (the GPU's own
// canonical NaN is 0x7FC00000): a NaN operand propagates quieted, the
// instruction's first operand winning; an invalid operation gives 0xFFC00000.
__device__ __forceinline__ float x86_nan(float a, float b, float r) {
  if (r == r) return r;
  if (a != a) return u2f(f2u(a) | 0x00400000u);
  if (b != b) return u2f(f2u(b) | 0x00400000u);
  return u2f(0xFFC00000u);
}

__device__ __forceinline__ float descent_weight(float x, float g, float lr) {
  const float t = x86_nan(0.0f, x, 0.0f * x);  // w_decay * w
  const float u = x86_nan(t, g, t + g);        // dW + t (the product is the x86 first operand)
  const float v = x86_nan(lr, u, lr * u);
  return x86_nan(x, v, x - v);
}

__device__ __forceinline__ float descent_bias(float b, float g, float lr) {
  const float v = x86_nan(g, lr, g * lr);
  return x86_nan(b, v, b - v);
}

}  // namespace fleet

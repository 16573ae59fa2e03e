// fleet_amd/csrc/solver_math.h -- the arithmetic of the reference's three other
// solvers (commonLib/cppNN/solver.h:97-195: adagrad, rmsprop, adam), host+device
// in one source so that tests/native/check_solver.cpp checks on the CPU, against
// libm and the reference's recorded bits, the code the kernels run.
//
// The reference is built -O0 for x86-64 SSE: every operation is one IEEE rounding
// in the type its source shows, no contraction. adam's denominator is binary64
// (`g2[s]/(1.-b2_t)` promotes, std::sqrt(double)), cast to float before `+ eps`.
//
// adam's b1_t and b2_t: 0.9f and 0.999f in a fresh solver, multiplied by b1 and b2 at
// every reset() (solver.h:167-172). The server's only reset is the one in
// fetchParamsNative's start_epoch (network.h:1442, epoch_count stays 0; it runs before
// the model is read, so it clears no state), so a session's values are 0.9f*0.9f and
// 0.999f*0.999f from the first descent to the last: no decay per step. They are
// arguments here (adam_bias_terms); the models pass the session's.
//
// NaN: as in descent_math.h / teacher_math.h, the device applies the x86 rule per
// operation with the operands in source order (a NaN operand propagates quieted,
// the first winning; an invalid operation gives 0xFFC00000, in binary64
// 0xFFF8000000000000; the float <-> double conversions quiet a NaN and keep its
// sign and upper payload). On the host the hardware has done it already.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define FLEET_SV __host__ __device__ __forceinline__
#else
#define FLEET_SV static inline __attribute__((always_inline))
#endif

namespace fleet {

FLEET_SV uint32_t sv_f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
FLEET_SV float sv_u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
FLEET_SV uint64_t sv_d2u(double x) { return __builtin_bit_cast(uint64_t, x); }
FLEET_SV double sv_u2d(uint64_t u) { return __builtin_bit_cast(double, u); }

FLEET_SV float sv_nan(float a, float b, float r) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (r == r) return r;
  if (a != a) return sv_u2f(sv_f2u(a) | 0x00400000u);
  if (b != b) return sv_u2f(sv_f2u(b) | 0x00400000u);
  return sv_u2f(0xFFC00000u);
#else
  (void)a, (void)b;
  return r;
#endif
}
FLEET_SV double sv_nan64(double a, double b, double r) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (r == r) return r;
  if (a != a) return sv_u2d(sv_d2u(a) | 0x0008000000000000ull);
  if (b != b) return sv_u2d(sv_d2u(b) | 0x0008000000000000ull);
  return sv_u2d(0xFFF8000000000000ull);
#else
  (void)a, (void)b;
  return r;
#endif
}

FLEET_SV float sv_add(float a, float b) { return sv_nan(a, b, a + b); }
FLEET_SV float sv_sub(float a, float b) { return sv_nan(a, b, a - b); }
FLEET_SV float sv_mul(float a, float b) { return sv_nan(a, b, a * b); }
FLEET_SV float sv_div(float a, float b) { return sv_nan(a, b, a / b); }
FLEET_SV float sv_sqrt(float a) { return sv_nan(a, a, __builtin_sqrtf(a)); }
FLEET_SV double sv_div64(double a, double b) { return sv_nan64(a, b, a / b); }
FLEET_SV double sv_sqrt64(double a) { return sv_nan64(a, a, __builtin_sqrt(a)); }
// cvtss2sd / cvtsd2ss
FLEET_SV double sv_widen(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (a != a) {
    const uint32_t u = sv_f2u(a) | 0x00400000u;
    return sv_u2d(((uint64_t)(u & 0x80000000u) << 32) | 0x7FF0000000000000ull | ((uint64_t)(u & 0x007fffffu) << 29));
  }
#endif
  return (double)a;
}
FLEET_SV float sv_narrow(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (a != a) {
    const uint64_t u = sv_d2u(a);
    return sv_u2f((uint32_t)(u >> 32 & 0x80000000u) | 0x7FC00000u | (uint32_t)(u >> 29 & 0x003fffffu));
  }
#endif
  return (float)a;
}

constexpr float kSvEps = 1.e-8f;
constexpr float kRmsMu = 0.999f;
constexpr float kAdamB1 = 0.9f, kAdamB2 = 0.999f;    // b1, b2

// b1_t, b2_t after `resets` calls of adam::reset (b1_t *= b1; b2_t *= b2, in float)
FLEET_SV void adam_bias_terms(int resets, float* b1_t, float* b2_t) {
  float t1 = kAdamB1, t2 = kAdamB2;
  for (int i = 0; i < resets; ++i) {
    t1 *= kAdamB1;
    t2 *= kAdamB2;
  }
  *b1_t = t1;
  *b2_t = t2;
}
constexpr int kServerResets = 1;  // fetchParamsNative's start_epoch

struct SolverStep {
  float w, g1, g2;
};

// adagrad::increment_w (solver.h:111-126): lr = custom_factor * learning_rate
FLEET_SV SolverStep adagrad_step(float w, float d, float g1, float L) {
  const float lr = sv_mul(1.0f, L);
  g1 = sv_add(g1, sv_mul(d, d));
  const float den = sv_add(sv_sqrt(g1), kSvEps);
  return SolverStep{sv_sub(w, sv_div(sv_mul(lr, d), den)), g1, 0.0f};
}

// rmsprop::increment_w (solver.h:139-151): lr = 0.01f * custom_factor * learning_rate
FLEET_SV SolverStep rmsprop_step(float w, float d, float g1, float L) {
  const float lr = sv_mul(0.01f * 1.0f, L);
  g1 = sv_add(sv_mul(kRmsMu, g1), sv_mul(sv_mul(1.0f - kRmsMu, d), d));
  const float den = sv_add(sv_sqrt(g1), kSvEps);
  return SolverStep{sv_sub(w, sv_div(sv_mul(lr, d), den)), g1, 0.0f};
}

// (float)std::sqrt(g2 / (1. - b2_t)) + eps
FLEET_SV float adam_den(float g2, float b2_t) {
  return sv_add(sv_narrow(sv_sqrt64(sv_div64(sv_widen(g2), 1.0 - (double)b2_t))), kSvEps);
}
// g1 / (1.f - b1_t)
FLEET_SV float adam_num(float g1, float b1_t) { return sv_div(g1, 1.0f - b1_t); }

// adam::increment_w (solver.h:180-193): lr = 0.1f * custom_factor * learning_rate
FLEET_SV SolverStep adam_step(float w, float d, float g1, float g2, float L, float b1_t, float b2_t) {
  const float lr = sv_mul(0.1f * 1.0f, L);
  g1 = sv_add(sv_mul(kAdamB1, g1), sv_mul(1.0f - kAdamB1, d));
  g2 = sv_add(sv_mul(kAdamB2, g2), sv_mul(sv_mul(1.0f - kAdamB2, d), d));
  return SolverStep{sv_sub(w, sv_div(sv_mul(lr, adam_num(g1, b1_t)), adam_den(g2, b2_t))), g1, g2};
}

// solver numbers of the C-ABI (FLEET_SOLVER_*)
constexpr int kSolverSgd = 0, kSolverAdagrad = 1, kSolverRmsprop = 2, kSolverAdam = 3;

template <int S>
FLEET_SV SolverStep solver_step(float w, float d, float g1, float g2, float L, float b1_t, float b2_t) {
  if (S == kSolverAdagrad) return adagrad_step(w, d, g1, L);
  if (S == kSolverRmsprop) return rmsprop_step(w, d, g1, L);
  return adam_step(w, d, g1, g2, L, b1_t, b2_t);
}

}  // namespace fleet

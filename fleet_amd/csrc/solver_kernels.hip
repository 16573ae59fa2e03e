// fleet_amd/csrc/solver_kernels.hip -- descentNative's model step under the
// reference's other solvers (solver_math.h: adagrad, rmsprop, adam), stateless
// form, and the self-test digests of their device arithmetic. A unit of its own,
// and siblings of k_descent / k_digest rather than flags of them, so that
// kernels.hip compiles to what it compiled to before (profiles/solvers/README.md).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "descent_math.h"
#include "kernels.h"
#include "solver_math.h"

namespace fleet {
namespace {

// k_descent's grid (block row = segment): the solver body in the weight segments,
// whose state rows are indexed like the weights; update_bias (descent_math.h, the
// plain learning rate) in the fully-connected bias segments.
template <int S>
__global__ void __launch_bounds__(256) k_descent_solver(float* __restrict__ weights, float* __restrict__ g1,
                                                        float* __restrict__ g2, float* __restrict__ fc_bias,
                                                        const float* __restrict__ grad, DescentSegs segs, float lr,
                                                        float b1_t, float b2_t) {
  const int sg = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= segs.len[sg]) return;
  const float g = grad[segs.grad_off[sg] + i];
  const int64_t e = segs.model_off[sg] + i;
  if (segs.kind[sg] == 0) {
    const SolverStep y = solver_step<S>(weights[e], g, g1[e], S == kSolverAdam ? g2[e] : 0.0f, lr, b1_t, b2_t);
    weights[e] = y.w;
    g1[e] = y.g1;
    if (S == kSolverAdam) g2[e] = y.g2;
  } else {
    fc_bias[e] = descent_bias(fc_bias[e], g, lr);
  }
}

__device__ __forceinline__ uint64_t sv_splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the edge grid of fn 28: every pair of these as (dividend, divisor)
__device__ const uint32_t kDivEdges[11] = {0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x3f800000u,
                                           0x7f7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u};

// fn 25..27, 29, 30: k_digest's sum of splitmix64(u << 32 | f(u)) over all 2^32 patterns u
// (26, 27: adam's denominator and numerator with a fresh solver's b2_t, b1_t; 29, 30: with
// the server session's, one reset on).
// fn 28: sum of splitmix64(splitmix64(a << 32 | b) + bits(a / b)) over the pairs
// (a, b) = (low, high word of splitmix64(i)), i < 2^32, and over the edge grid.
__global__ void __launch_bounds__(256) k_digest_solver(int fn, float b1_t, float b2_t,
                                                       unsigned long long* __restrict__ out) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint64_t sum = 0;
  for (uint64_t i = tid; i < (1ull << 32); i += nthreads) {
    const uint32_t u = (uint32_t)i;
    if (fn == 28) {
      const uint64_t p = sv_splitmix64(i);
      const uint32_t a = (uint32_t)p, b = (uint32_t)(p >> 32);
      sum += sv_splitmix64(sv_splitmix64(((uint64_t)a << 32) | b) + sv_f2u(sv_div(sv_u2f(a), sv_u2f(b))));
      continue;
    }
    uint32_t o;
    switch (fn) {
      case 25: o = sv_f2u(sv_sqrt(sv_u2f(u))); break;
      case 26: case 29: o = sv_f2u(adam_den(sv_u2f(u), b2_t)); break;
      default: o = sv_f2u(adam_num(sv_u2f(u), b1_t)); break;
    }
    sum += sv_splitmix64(((uint64_t)u << 32) | o);
  }
  if (fn == 28 && tid < 121) {
    const uint32_t a = kDivEdges[tid / 11], b = kDivEdges[tid % 11];
    sum += sv_splitmix64(sv_splitmix64(((uint64_t)a << 32) | b) + sv_f2u(sv_div(sv_u2f(a), sv_u2f(b))));
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)sum);
}

}  // namespace

hipError_t launch_descent_solver(int solver, float* weights, float* g1, float* g2, float* fc_bias, const float* grad,
                                 const DescentSegs& segs, float lr, float b1_t, float b2_t, hipStream_t s) {
  int64_t mx = 0;
  for (int k = 0; k < segs.n; ++k) mx = std::max(mx, segs.len[k]);
  if (segs.n == 0 || mx == 0) return hipSuccess;
  const dim3 grid((unsigned)((mx + 255) / 256), (unsigned)segs.n);
  switch (solver) {
    case kSolverAdagrad:
      hipLaunchKernelGGL(k_descent_solver<kSolverAdagrad>, grid, dim3(256), 0, s, weights, g1, g2, fc_bias, grad, segs, lr,
                         b1_t, b2_t);
      break;
    case kSolverRmsprop:
      hipLaunchKernelGGL(k_descent_solver<kSolverRmsprop>, grid, dim3(256), 0, s, weights, g1, g2, fc_bias, grad, segs, lr,
                         b1_t, b2_t);
      break;
    case kSolverAdam:
      hipLaunchKernelGGL(k_descent_solver<kSolverAdam>, grid, dim3(256), 0, s, weights, g1, g2, fc_bias, grad, segs, lr,
                         b1_t, b2_t);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_digest_solver(int fn, unsigned long long* out, hipStream_t s) {
  float b1_t, b2_t;
  adam_bias_terms(fn >= 29 ? kServerResets : 0, &b1_t, &b2_t);
  hipLaunchKernelGGL(k_digest_solver, dim3(256 * 16), dim3(256), 0, s, fn, b1_t, b2_t, out);
  return hipGetLastError();
}

}  // namespace fleet

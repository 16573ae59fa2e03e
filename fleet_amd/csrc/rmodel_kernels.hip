// fleet_amd/csrc/rmodel_kernels.hip -- the resident model's step on gfx950:
// descentNative (Server/src/main/c++/cppNN_backend.cpp:329-383) on a model that
// lives in HBM. The header checks fleet_model_descent makes on the host run
// here in k_rm_check before any weight is written; k_rm_step applies
// descent_math.h's two update bodies and, in DISTILLATION_MODE=0, leaves the
// model copy's `%g` / strtof round trip of every value in the new version's row.
// k_rm_step_solver<S> is the same step under adagrad, rmsprop or adam (solver_math.h),
// with the solver's state rows beside cnn.
#include <hip/hip_runtime.h>

#include "decimal6.h"
#include "descent_math.h"
#include "rmodel_kernels.h"
#include "solver_math.h"

namespace fleet {
namespace {

// strtof of the `%g` text: ±inf kept, NaN to the default quiet NaN with its sign
__device__ __forceinline__ float rt_text(float x) {
  const uint32_t u = f2u(x);
  if ((u & 0x7f800000u) != 0x7f800000u) return g6_roundtrip(x);
  if ((u & 0x007fffffu) == 0) return x;
  return u2f((u & 0x80000000u) | 0x7fc00000u);
}

// take(): the next header slot as an int (fleet_model_descent's lambda)
__device__ __forceinline__ bool rm_take(const float* g, int64_t n, int64_t& idx, int32_t* v, bool* whole) {
  if (idx >= n) return false;
  const float f = g[idx++];
  if (!(__builtin_fabsf(f) < 2147483648.0f)) return false;
  *v = (int32_t)f;
  if ((float)*v != f) *whole = false;  // fleet_descent's grad[idx] == (float)size
  return true;
}

__global__ void k_rm_check(const float* __restrict__ g, int64_t n, RmLayout L, int* __restrict__ err) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t idx = 0, wo = 0, bo = 0;
  int nws = 0, nbs = 0;
  int32_t cnt = 0, sz = 0;
  bool whole = true;
  if (!rm_take(g, n, idx, &cnt, &whole) || cnt != L.n_edges) {
    *err = kRmErrLayout;
    return;
  }
  for (int i = 0; i < L.n_edges; ++i) {
    if (!rm_take(g, n, idx, &sz, &whole) || sz < 0 || idx + sz > n) {
      *err = kRmErrLayout;
      return;
    }
    if (L.w_present[i]) {
      // a block that would run past the model's weights can only end in a size error:
      // nothing more is recorded, so no table entry ever points outside the model
      if (sz > 0 && wo + sz <= L.n_w) {
        L.w_start[nws] = wo;
        L.w_grad[nws] = idx;
        ++nws;
      }
      wo += sz;
    }
    idx += sz;
  }
  if (!rm_take(g, n, idx, &cnt, &whole) || cnt != L.n_layers) {
    *err = kRmErrLayout;
    return;
  }
  for (int k = 0; k < L.n_layers; ++k) {
    if (!rm_take(g, n, idx, &sz, &whole) || sz < 0 || idx + sz > n) {
      *err = kRmErrLayout;
      return;
    }
    if (L.fc_layer[k]) {
      if (sz > 0 && bo + sz <= L.n_fc) {
        L.b_start[nbs] = bo;
        L.b_grad[nbs] = idx;
        ++nbs;
      }
      bo += sz;
    }
    idx += sz;
  }
  if (idx != n || wo != L.n_w || bo != L.n_fc) {
    *err = kRmErrSizes;
    return;
  }
  if (!whole) {
    *err = kRmErrLayout;
    return;
  }
  L.w_start[nws] = L.n_w;
  L.b_start[nbs] = L.n_fc;
  L.counts[0] = nws;
  L.counts[1] = nbs;
}

// the segment of a sorted start table that holds e: start[k] <= e < start[k + 1]
__device__ __forceinline__ int seg_of(const int64_t* __restrict__ start, int n, int64_t e) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// One thread per weight, then per fc bias (compact index), then per use_bias() bias
// (the row's copy of the biases no segment covers).
__global__ void __launch_bounds__(256) k_rm_step(float* __restrict__ cnn_w, float* __restrict__ cnn_b,
                                                 const float* __restrict__ g, RmLayout L, float lr,
                                                 float* __restrict__ row_w, float* __restrict__ row_b,
                                                 const int* __restrict__ err) {
  if (*err) return;
  int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < L.n_w) {
    const int k = seg_of(L.w_start, L.counts[0], e);
    const float y = descent_weight(cnn_w[e], g[L.w_grad[k] + (e - L.w_start[k])], lr);
    cnn_w[e] = y;
    if (row_w) row_w[e] = rt_text(y);
    return;
  }
  e -= L.n_w;
  if (e < L.n_fc) {
    const int k = seg_of(L.b_start, L.counts[1], e);
    const int j = seg_of(L.fcl_start, L.n_fcl, e);
    const int64_t q = L.fcl_boff[j] + (e - L.fcl_start[j]);
    const float y = descent_bias(cnn_b[q], g[L.b_grad[k] + (e - L.b_start[k])], lr);
    cnn_b[q] = y;
    if (row_b) row_b[q] = rt_text(y);
    return;
  }
  e -= L.n_fc;
  if (e < L.n_b && row_b) {
    for (int j = 0; j < L.n_fcl; ++j)  // an fc layer's bias: written above
      if (e >= L.fcl_boff[j] && e < L.fcl_boff[j] + (L.fcl_start[j + 1] - L.fcl_start[j])) return;
    row_b[e] = rt_text(cnn_b[e]);
  }
}

// k_rm_step under adagrad, rmsprop or adam (solver_math.h): the solver body and its state
// rows (indexed like the weights, read and written in place) in the weight leg only; the
// bias legs, the header check's word and the mode-0 version row are k_rm_step's.
template <int S>
__global__ void __launch_bounds__(256) k_rm_step_solver(float* __restrict__ cnn_w, float* __restrict__ cnn_b,
                                                        float* __restrict__ g1, float* __restrict__ g2,
                                                        const float* __restrict__ g, RmLayout L, float lr,
                                                        float b1_t, float b2_t, float* __restrict__ row_w,
                                                        float* __restrict__ row_b, const int* __restrict__ err) {
  if (*err) return;
  int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < L.n_w) {
    const int k = seg_of(L.w_start, L.counts[0], e);
    const SolverStep y = solver_step<S>(cnn_w[e], g[L.w_grad[k] + (e - L.w_start[k])], g1[e],
                                        S == kSolverAdam ? g2[e] : 0.0f, lr, b1_t, b2_t);
    cnn_w[e] = y.w;
    g1[e] = y.g1;
    if (S == kSolverAdam) g2[e] = y.g2;
    if (row_w) row_w[e] = rt_text(y.w);
    return;
  }
  e -= L.n_w;
  if (e < L.n_fc) {
    const int k = seg_of(L.b_start, L.counts[1], e);
    const int j = seg_of(L.fcl_start, L.n_fcl, e);
    const int64_t q = L.fcl_boff[j] + (e - L.fcl_start[j]);
    const float y = descent_bias(cnn_b[q], g[L.b_grad[k] + (e - L.b_start[k])], lr);
    cnn_b[q] = y;
    if (row_b) row_b[q] = rt_text(y);
    return;
  }
  e -= L.n_fc;
  if (e < L.n_b && row_b) {
    for (int j = 0; j < L.n_fcl; ++j)  // an fc layer's bias: written above
      if (e >= L.fcl_boff[j] && e < L.fcl_boff[j] + (L.fcl_start[j + 1] - L.fcl_start[j])) return;
    row_b[e] = rt_text(cnn_b[e]);
  }
}

__global__ void __launch_bounds__(256) k_rm_roundtrip(const float* __restrict__ in, float* __restrict__ out,
                                                      int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = rt_text(in[i]);
}

}  // namespace

hipError_t launch_rm_check(const float* d_grad, int64_t n_values, const RmLayout& L, int* d_err, hipStream_t s) {
  hipLaunchKernelGGL(k_rm_check, dim3(1), dim3(1), 0, s, d_grad, n_values, L, d_err);
  return hipGetLastError();
}

hipError_t launch_rm_step(float* cnn_w, float* cnn_b, const float* d_grad, const RmLayout& L, float lr, float* row_w,
                          float* row_b, const int* d_err, hipStream_t s) {
  const int64_t n = L.n_w + L.n_fc + L.n_b;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cnn_w, cnn_b, d_grad, L, lr,
                     row_w, row_b, d_err);
  return hipGetLastError();
}

hipError_t launch_rm_step_solver(int solver, float* cnn_w, float* cnn_b, float* g1, float* g2, const float* d_grad,
                                 const RmLayout& L, float lr, float b1_t, float b2_t, float* row_w, float* row_b,
                                 const int* d_err, hipStream_t s) {
  const int64_t n = L.n_w + L.n_fc + L.n_b;
  if (n == 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  switch (solver) {
    case kSolverAdagrad:
      hipLaunchKernelGGL(k_rm_step_solver<kSolverAdagrad>, grid, dim3(256), 0, s, cnn_w, cnn_b, g1, g2, d_grad, L, lr,
                         b1_t, b2_t, row_w, row_b, d_err);
      break;
    case kSolverRmsprop:
      hipLaunchKernelGGL(k_rm_step_solver<kSolverRmsprop>, grid, dim3(256), 0, s, cnn_w, cnn_b, g1, g2, d_grad, L, lr,
                         b1_t, b2_t, row_w, row_b, d_err);
      break;
    case kSolverAdam:
      hipLaunchKernelGGL(k_rm_step_solver<kSolverAdam>, grid, dim3(256), 0, s, cnn_w, cnn_b, g1, g2, d_grad, L, lr,
                         b1_t, b2_t, row_w, row_b, d_err);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_rm_roundtrip(const float* in, float* out, int64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rm_roundtrip, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
  return hipGetLastError();
}

}  // namespace fleet

// fleet_amd/csrc/rmodel_kernels.h -- launchers of the resident model's step
// (rmodel_kernels.hip <-> rmodel_state.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fleet {

// error word of the step (what k_rm_check found in the merged gradient's header
// slots; fleet_model_descent's checks in its order)
constexpr int kRmErrLayout = 1;  // a count or a block size the walk refuses, or a slot that is no integer
constexpr int kRmErrSizes = 2;   // the blocks do not add up to the model's weights / fc biases / n_values

// What the model knows (uploaded once at load) and what the check derives from
// the gradient (device tables the step reads): segment k of the weights covers
// model weights [w_start[k], w_start[k+1]) from gradient position w_grad[k];
// likewise the fully-connected bias blocks over the compact fc-bias index.
struct RmLayout {
  int n_edges, n_layers, n_fcl;
  int64_t n_w, n_fc, n_b;
  const uint8_t* w_present;   // [n_edges]
  const uint8_t* fc_layer;    // [n_layers]
  const int64_t* fcl_start;   // [n_fcl + 1] compact fc-bias offset of each fc layer's block
  const int64_t* fcl_boff;    // [n_fcl]     its offset in the use_bias() bias vector
  int64_t* w_start;           // [n_edges + 1]
  int64_t* w_grad;            // [n_edges]
  int64_t* b_start;           // [n_layers + 1]
  int64_t* b_grad;            // [n_layers]
  int* counts;                // {weight segments, bias segments}
};

// The header walk of network::descent(vector) over d_grad[n_values] on the device (one
// thread: a few dozen dependent loads); sets *d_err and fills the tables.
hipError_t launch_rm_check(const float* d_grad, int64_t n_values, const RmLayout& L, int* d_err, hipStream_t s);
// The step over every weight and fc bias (descent_math.h), skipped when *d_err != 0.
// row_w / row_b (both or neither): the new version's row takes the `%g` / strtof
// round trip of every value (DISTILLATION_MODE=0's model copy), the biases no
// segment covers included.
hipError_t launch_rm_step(float* cnn_w, float* cnn_b, const float* d_grad, const RmLayout& L, float lr, float* row_w,
                          float* row_b, const int* d_err, hipStream_t s);
// The same step under FLEET_SOLVER_ADAGRAD / _RMSPROP / _ADAM (solver_math.h): g1, g2 = the
// model's state rows of n_w floats (g2: adam only), advanced in place in the weight leg; b1_t, b2_t = adam's bias-correction terms.
hipError_t launch_rm_step_solver(int solver, float* cnn_w, float* cnn_b, float* g1, float* g2, const float* d_grad,
                                 const RmLayout& L, float lr, float b1_t, float b2_t, float* row_w, float* row_b,
                                 const int* d_err, hipStream_t s);
// out[i] = strtof(sprintf("%g", in[i])): finite values through g6_roundtrip, inf kept,
// NaN to the default quiet NaN with its sign (what strtof gives for "nan" / "-nan")
hipError_t launch_rm_roundtrip(const float* in, float* out, int64_t n, hipStream_t s);

}  // namespace fleet

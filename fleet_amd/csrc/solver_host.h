// fleet_amd/csrc/solver_host.h -- the host model's way into the stateless solver step
// (fleet_codec.cpp <-> model_state.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/fleet_codec.h"

namespace fleet {

// fleet_descent_solver with adam's b1_t, b2_t as `adam_resets` calls of adam::reset leave
// them (solver_math.h adam_bias_terms): 0 = a fresh solver, fleet_descent_solver's;
// kServerResets = a server session's, the models'.
int descent_solver_host(fleet_ctx* ctx, int solver, int adam_resets, float* weights, size_t n_weights, float* g1,
                        float* g2, float* fc_bias, size_t n_fc_bias, const float* grad, size_t n_grad,
                        const int32_t* w_sizes, const uint8_t* w_present, int n_w, const int32_t* b_sizes,
                        const uint8_t* fc_layer, int n_b, float lr);

}  // namespace fleet

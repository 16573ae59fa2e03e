// fleet_amd/csrc/model_state.h -- the host model's state (model_state.cpp), shared
// with the resident model (rmodel_state.cpp), which loads its text through
// fleet_model_load and keeps the parsed layout as its host mirror.
#pragma once
#include <cstdint>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fleet_codec.h"

namespace fleet {

struct Layer {
  std::string name, type, act;  // act: the config's activation word ("elu", "softmax", ...), if any
  std::vector<long> args;
  bool use_bias = false, fc = false;
  int cols = 1, rows = 1, chans = 1;  // node dims after the graph is connected
  int kernels_per_map = 0;
  size_t bias_size = 0;
};

struct Version {
  std::vector<float> w;  // non-null W concatenated in W order
  std::vector<float> b;  // biases of the use_bias() layers, layer order
};

}  // namespace fleet

struct fleet_model;
namespace fleet {
// FLEET_OK when m is the Driver's MNIST network (Driver/src/main/c++/cppNN_backend.cpp:109-115),
// the only one the evaluation kernels run; otherwise *why names the first layer that differs
int eval_check_mnist(const fleet_model* m, std::string* why);
// FLEET_OK when m is the reference's CIFAR network (Driver/src/main/c++/cppNN_backend.cpp:128-138:
// type, arguments and activation word of every layer, and the chain), *classes then FC2's size,
// 10 or 100; otherwise *why names the first layer that differs
int cifar_check(const fleet_model* m, int* classes, std::string* why);
}  // namespace fleet

struct fleet_model {
  fleet_ctx* ctx = nullptr;
  int mode = 1;  // DISTILLATION_MODE
  std::mutex mu;
  std::string header;  // "mojo01" .. graph .. "0\n", re-emitted verbatim by getParams
  std::vector<fleet::Layer> layers;
  std::vector<int32_t> edge_w_size;  // per layer-graph edge: W size, 0 for a null W
  std::vector<int32_t> dims;         // per non-null W: cols, rows, chans
  std::vector<uint8_t> fc;           // per layer: fully_connected (update_bias applies)
  fleet::Version cnn;                // `cnn`
  std::deque<fleet::Version> models; // `models`
  int64_t pushed = 0;                // versions ever pushed: models[v]'s id is pushed - models.size() + v
  std::vector<double> lrates;        // `lrates_vec`
  float lr = 0.0f;                   // cnn's learning rate (set_learning_rate(double) -> float)
  int epoch = 0, priority = 0;
  int solver = 0;                    // FLEET_SOLVER_*: what `cnn` was constructed with
  bool stepped = false;              // a descent has run: the solver can no longer be set
  std::vector<float> g1, g2;         // the solver's state (G1, G2), laid out like cnn.w
  std::string err;
};

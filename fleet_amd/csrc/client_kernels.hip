// fleet_amd/csrc/client_kernels.hip -- the client's gradient computation on the device
// (SURVEY.md row 3b): for C clients of B samples each, the float vector cnn.gradients()
// returns after B train_class calls (Client/app/src/main/cpp/cppNN-lib.cpp:101-113, 218-234;
// commonLib/cppNN/network.h:1806-2008, 1551-1611, 1289-1331, 1038-1056). The arithmetic and
// its order are client_backward.h's, documented at its head; this unit only places it:
//
//   k_client_sample  one 256-thread block per (client, sample): the sample's layers (nodes,
//                    p_maps, deltas, the two padded convolution deltas: clientnet::Sample,
//                    104 KB) live in LDS, the stages run one after the other with a barrier
//                    between them, every element computed by one lane, serially, in the
//                    reference's order. The sample's own dW and dbias go to its row of the
//                    workspace in the gradients() layout (22961 floats).
//   k_client_sum     one lane per (client, element): the rows added in sample order in
//                    binary32, header values passed through, into the caller's fp32 rows.
// No atomics on values, no cross-lane reductions, no MFMA, no contraction (the unit builds
// with -ffp-contract=off -fno-slp-vectorize); the two kernels are separate launches on the
// caller's stream, and clients are walked in chunks whose workspace fits a cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "client_backward.h"
#include "fleet_codec.h"
#include "kernels.h"

namespace fleet {

namespace {

struct BlockPar {
  template <class F>
  __device__ __forceinline__ void operator()(int n, F f) const {
    for (int o = threadIdx.x; o < n; o += blockDim.x) f(o);
    __syncthreads();
  }
};

}  // namespace

// block = (client c0 + blockIdx.x / B, sample blockIdx.x % B); rows: the chunk's workspace,
// row blockIdx.x. An index outside the images or the model rows sets FLEET_ERRBIT_ARG and the
// block computes on image / model 0 (its output is not to be used); E NaN sets FLEET_ERRBIT_NAN.
__global__ void __launch_bounds__(256) k_client_sample(const float* __restrict__ models, int64_t model_pitch, int n_models,
                                                       const int32_t* __restrict__ model_of_client,
                                                       const float* __restrict__ images, int64_t n_images, int F,
                                                       const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ idx,
                                                       const int32_t* __restrict__ shift, int c0, int B,
                                                       float temperature, float* __restrict__ rows,
                                                       int* __restrict__ err) {
  using namespace clientnet;
  __shared__ Sample S;
  const int c = c0 + (int)(blockIdx.x / (unsigned)B), k = (int)(blockIdx.x % (unsigned)B);
  const int64_t slot = (int64_t)c * B + k;
  int64_t img = idx ? (int64_t)idx[slot] : slot;
  int model = model_of_client ? model_of_client[c] : 0;
  int dx = shift ? shift[2 * slot] : 0, dy = shift ? shift[2 * slot + 1] : 0;
  bool bad = false;  // block-uniform
  if (img < 0 || img >= n_images) bad = true, img = 0;
  if (model < 0 || model >= n_models) bad = true, model = 0;
  if (dx < -1 || dx > 1 || dy < -1 || dy > 1) bad = true, dx = dy = 0;
  if (bad && threadIdx.x == 0) atomicOr(err, FLEET_ERRBIT_ARG);
  const float* w = models + (int64_t)model * model_pitch;
  const bool finite = sample_stages(BlockPar{}, S, w, w + kWTotal, images + img * F, labels[img], dx, dy,
                                    temperature, rows + (int64_t)blockIdx.x * kGradLen);
  if (!finite && threadIdx.x == 0) atomicOr(err, FLEET_ERRBIT_NAN);
}

__global__ void __launch_bounds__(256) k_client_sum(const float* __restrict__ rows, int B, int clients,
                                                    float* __restrict__ grads, int64_t grad_pitch) {
  using namespace clientnet;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)clients * kGradLen) return;
  const int c = (int)(i / kGradLen), e = (int)(i % kGradLen);
  grads[(int64_t)c * grad_pitch + e] = grad_element(rows + (int64_t)c * B * kGradLen, kGradLen, B, e);
}

namespace {
std::atomic<int> g_client_chunk{0};
constexpr size_t kClientWorkspaceCap = (size_t)256 << 20;  // bytes of per-sample rows in flight
}  // namespace

int64_t client_grad_len() { return clientnet::kGradLen; }

int client_grad_set_chunk(int max_clients) { return g_client_chunk.exchange(max_clients > 0 ? max_clients : 0); }

// clients per chunk for B samples each: the override, else what fits the cap (at least one)
int client_grad_chunk(int C, int B) {
  const int forced = g_client_chunk.load();
  size_t n = forced > 0 ? (size_t)forced : kClientWorkspaceCap / ((size_t)B * clientnet::kGradLen * sizeof(float));
  if (n < 1) n = 1;
  return n > (size_t)C ? C : (int)n;
}

size_t client_grad_workspace_bytes(int chunk, int B) {
  return (size_t)chunk * (size_t)B * clientnet::kGradLen * sizeof(float);
}

// grads: C rows of grad_pitch floats. workspace: client_grad_workspace_bytes(chunk, B).
hipError_t launch_client_grads(const float* models, int64_t model_pitch, int n_models, const int32_t* model_of_client,
                               const float* images, int64_t n_images, int F, const int32_t* labels, const int32_t* idx,
                               const int32_t* shift, int C, int B, int chunk, float temperature, float* workspace,
                               float* grads, int64_t grad_pitch, int* err, hipStream_t s) {
  if (C <= 0 || B <= 0 || chunk <= 0 || F < clientnet::kPix || grad_pitch < clientnet::kGradLen ||
      (int64_t)chunk * B > INT32_MAX)
    return hipErrorInvalidValue;
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int n = C - c0 < chunk ? C - c0 : chunk;
    hipLaunchKernelGGL(k_client_sample, dim3((unsigned)(n * B)), dim3(256), 0, s, models, model_pitch, n_models,
                       model_of_client, images, n_images, F, labels, idx, shift, c0, B, temperature, workspace, err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t elems = (int64_t)n * clientnet::kGradLen;
    hipLaunchKernelGGL(k_client_sum, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, workspace, B, n,
                       grads + (int64_t)c0 * grad_pitch, grad_pitch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace fleet

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
// With the distillation cost (cppNN-lib.cpp:251-252) k_client_sample_distill runs the same
// stages with the other output delta. With sigma > 0 for some client (cnn.DPgradients,
// network.h:1092-1181) two more kernels take k_client_sum's place:
//   k_client_clip    one block per (client, sample >= 1) of the clients with sigma > 0:
//                    scale_gradients' sqsum over the sample's stored row. The lanes read a
//                    tile of the row in the reference's walk order (coalesced inside a block of
//                    the layout) and square it into LDS; the products are independent. Lane 0
//                    then adds the tile, in order, in binary32, while every lane's loads of
//                    the next tile are in flight (two LDS tiles, one barrier per tile). The
//                    block writes scale[client][sample]; slot 0's scale is 1.
//   k_client_sum_dp  k_client_sum with the bias blocks of samples >= 1 multiplied by their
//                    scale as they are added and the draw z[e] * (clip * sigma) added in
//                    binary64; z is the resident table of 22961 standard-normal draws made on
//                    the host. A client with sigma = 0 gets k_client_sum's row.
// No atomics on values, no cross-lane reductions, no MFMA, no contraction (the unit builds
// with -ffp-contract=off -fno-slp-vectorize); the kernels are separate launches on the
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
// (one body for both costs, as text: the cross-entropy kernel is then the kernel it was)
#define FLEET_CLIENT_SAMPLE_KERNEL(NAME, COST)                                                                      \
  __global__ void __launch_bounds__(256)                                                                            \
      NAME(const float* __restrict__ models, int64_t model_pitch, int n_models,                                     \
           const int32_t* __restrict__ model_of_client, const float* __restrict__ images, int64_t n_images, int F,  \
           const int32_t* __restrict__ labels, const int32_t* __restrict__ idx, const int32_t* __restrict__ shift,  \
           int c0, int B, float temperature, float* __restrict__ rows, int* __restrict__ err) {                     \
    using namespace clientnet;                                                                                      \
    __shared__ Sample S;                                                                                            \
    const int c = c0 + (int)(blockIdx.x / (unsigned)B), k = (int)(blockIdx.x % (unsigned)B);                        \
    const int64_t slot = (int64_t)c * B + k;                                                                        \
    int64_t img = idx ? (int64_t)idx[slot] : slot;                                                                  \
    int model = model_of_client ? model_of_client[c] : 0;                                                           \
    int dx = shift ? shift[2 * slot] : 0, dy = shift ? shift[2 * slot + 1] : 0;                                     \
    bool bad = false; /* block-uniform */                                                                           \
    if (img < 0 || img >= n_images) bad = true, img = 0;                                                            \
    if (model < 0 || model >= n_models) bad = true, model = 0;                                                      \
    if (dx < -1 || dx > 1 || dy < -1 || dy > 1) bad = true, dx = dy = 0;                                            \
    if (bad && threadIdx.x == 0) atomicOr(err, FLEET_ERRBIT_ARG);                                                   \
    const float* w = models + (int64_t)model * model_pitch;                                                         \
    const bool finite = sample_stages<COST>(BlockPar{}, S, w, w + kWTotal, images + img * F, labels[img], dx, dy,   \
                                            temperature, rows + (int64_t)blockIdx.x * kGradLen);                    \
    if (!finite && threadIdx.x == 0) atomicOr(err, FLEET_ERRBIT_NAN);                                               \
  }

FLEET_CLIENT_SAMPLE_KERNEL(k_client_sample, kCostCrossEntropy)
FLEET_CLIENT_SAMPLE_KERNEL(k_client_sample_distill, kCostDistillation)

__global__ void __launch_bounds__(256) k_client_sum(const float* __restrict__ rows, int B, int clients,
                                                    float* __restrict__ grads, int64_t grad_pitch) {
  using namespace clientnet;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)clients * kGradLen) return;
  const int c = (int)(i / kGradLen), e = (int)(i % kGradLen);
  grads[(int64_t)c * grad_pitch + e] = grad_element(rows + (int64_t)c * B * kGradLen, kGradLen, B, e);
}

// scale_gradients (network.h:1092-1112) for block = (client c0 + blockIdx.x / (B-1), sample
// 1 + blockIdx.x % (B-1)); B >= 2. rows: the chunk's workspace; scale: [chunk clients][B].
// clip, sigma: [C] of the whole call. A client with sigma = 0 is not clipped: its blocks leave.
constexpr int kClipTile = 2048;  // squares per LDS tile: 8 per lane
__global__ void __launch_bounds__(256) k_client_clip(const float* __restrict__ rows, int c0, int B,
                                                     const float* __restrict__ clip, const float* __restrict__ sigma,
                                                     float* __restrict__ scale) {
  using namespace clientnet;
  constexpr int kPer = kClipTile / 256;
  __shared__ __attribute__((aligned(16))) float sq[2][kClipTile];
  const int lc = (int)(blockIdx.x / (unsigned)(B - 1)), k = 1 + (int)(blockIdx.x % (unsigned)(B - 1));
  if (!(sigma[c0 + lc] > 0.0f)) return;  // block-uniform
  const float* row = rows + ((int64_t)lc * B + k) * kGradLen;
  float v[kPer];
  // the walk's positions base + threadIdx.x + 256*j of a tile: consecutive lanes, consecutive
  // elements inside a block of the layout; a position past the walk's end squares to +0 and is
  // never added
  auto load = [&](int base) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int p = base + (int)threadIdx.x + 256 * j;
      v[j] = p < kClipLen ? row[clip_element(p)] : 0.0f;
    }
  };
  load(0);
  float sqsum = 0.0f;
  for (int base = 0, t = 0; base < kClipLen; base += kClipTile, ++t) {
    float* tile = sq[t & 1];
#pragma unroll
    for (int j = 0; j < kPer; ++j) tile[threadIdx.x + 256 * j] = v[j] * v[j];
    // lane 0 left this tile's other buffer before it arrived here, so the next iteration's
    // writes to that buffer need no second barrier
    __syncthreads();
    if (base + kClipTile < kClipLen) load(base + kClipTile);
    if (threadIdx.x == 0) {
      const int n = kClipLen - base < kClipTile ? kClipLen - base : kClipTile;
      int i = 0;
      for (; i + 4 <= n; i += 4) {
        const float4 q = *reinterpret_cast<const float4*>(tile + i);
        sqsum = sqsum + q.x;
        sqsum = sqsum + q.y;
        sqsum = sqsum + q.z;
        sqsum = sqsum + q.w;
      }
      for (; i < n; ++i) sqsum = sqsum + tile[i];
    }
  }
  if (threadIdx.x == 0) {
    scale[(int64_t)lc * B + k] = clip_scale(sqsum, clip[c0 + lc]);
    if (k == 1) scale[(int64_t)lc * B] = 1.0f;
  }
}

// clip, sigma: [C] of the whole call, client c0 + c of it is client c of this chunk; scale:
// [clients][B] as k_client_clip wrote it (not read for a client with sigma = 0, nor where B = 1)
__global__ void __launch_bounds__(256) k_client_sum_dp(const float* __restrict__ rows, int B, int clients, int c0,
                                                       const float* __restrict__ clip, const float* __restrict__ sigma,
                                                       const float* __restrict__ scale, const double* __restrict__ z,
                                                       float* __restrict__ grads, int64_t grad_pitch) {
  using namespace clientnet;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)clients * kGradLen) return;
  const int c = (int)(i / kGradLen), e = (int)(i % kGradLen);
  const float* r = rows + (int64_t)c * B * kGradLen;
  const float sg = sigma[c0 + c];
  grads[(int64_t)c * grad_pitch + e] =
      sg > 0.0f ? dp_grad_element(r, kGradLen, B, scale + (int64_t)c * B, e, z[e], (double)(clip[c0 + c] * sg))
                : grad_element(r, kGradLen, B, e);
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

// the scales of a chunk live beside its rows: [chunk][B] floats behind the workspace
size_t client_grad_scale_bytes(int chunk, int B) { return (size_t)chunk * (size_t)B * sizeof(float); }

#if !defined(__HIP_DEVICE_COMPILE__)  // host code: the device pass never sees the generator
void client_dp_noise(double* out, size_t n) { clientnet::dp_noise_draws(out, n); }
#endif

// grads: C rows of grad_pitch floats. workspace: client_grad_workspace_bytes(chunk, B).
hipError_t launch_client_grads(const float* models, int64_t model_pitch, int n_models, const int32_t* model_of_client,
                               const float* images, int64_t n_images, int F, const int32_t* labels, const int32_t* idx,
                               const int32_t* shift, int C, int B, int chunk, float temperature, float* workspace,
                               float* grads, int64_t grad_pitch, int* err, hipStream_t s) {
  return launch_client_grads_ex(models, model_pitch, n_models, model_of_client, images, n_images, F, labels, idx, shift, C,
                                B, chunk, temperature, clientnet::kCostCrossEntropy, nullptr, nullptr, nullptr, nullptr,
                                nullptr, workspace, grads, grad_pitch, err, s);
}

// cost: 0 cross_entropy, 1 distillation. DP where d_clip is given: d_clip, d_sigma [C] on the
// device, dp_of_client [C] on the host (non-zero: sigma > 0, for the launch decisions alone), d_z
// the 22961 draws, scale: client_grad_scale_bytes(chunk, B) on the device.
hipError_t launch_client_grads_ex(const float* models, int64_t model_pitch, int n_models,
                                  const int32_t* model_of_client, const float* images, int64_t n_images, int F,
                                  const int32_t* labels, const int32_t* idx, const int32_t* shift, int C, int B,
                                  int chunk, float temperature, int cost, const float* d_clip, const float* d_sigma,
                                  const uint8_t* dp_of_client, const double* d_z, float* scale, float* workspace,
                                  float* grads, int64_t grad_pitch, int* err, hipStream_t s) {
  if (C <= 0 || B <= 0 || chunk <= 0 || F < clientnet::kPix || grad_pitch < clientnet::kGradLen ||
      (int64_t)chunk * B > INT32_MAX || (cost != clientnet::kCostCrossEntropy && cost != clientnet::kCostDistillation) ||
      (d_clip && (!d_sigma || !dp_of_client || !d_z || !scale)))
    return hipErrorInvalidValue;
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int n = C - c0 < chunk ? C - c0 : chunk;
    hipLaunchKernelGGL(cost == clientnet::kCostDistillation ? k_client_sample_distill : k_client_sample,
                       dim3((unsigned)(n * B)), dim3(256), 0, s, models, model_pitch, n_models, model_of_client, images,
                       n_images, F, labels, idx, shift, c0, B, temperature, workspace, err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t elems = (int64_t)n * clientnet::kGradLen;
    bool dp = false;  // a client of this chunk with sigma > 0
    for (int c = c0; d_clip && c < c0 + n; ++c) dp |= dp_of_client[c] != 0;
    if (!dp) {
      hipLaunchKernelGGL(k_client_sum, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, workspace, B, n,
                         grads + (int64_t)c0 * grad_pitch, grad_pitch);
    } else {
      if (B > 1) {
        hipLaunchKernelGGL(k_client_clip, dim3((unsigned)(n * (B - 1))), dim3(256), 0, s, workspace, c0, B, d_clip,
                           d_sigma, scale);
        if ((e = hipGetLastError()) != hipSuccess) return e;
      }
      hipLaunchKernelGGL(k_client_sum_dp, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, workspace, B, n, c0,
                         d_clip, d_sigma, scale, d_z, grads + (int64_t)c0 * grad_pitch, grad_pitch);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace fleet

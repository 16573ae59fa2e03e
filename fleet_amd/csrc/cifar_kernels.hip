// fleet_amd/csrc/cifar_kernels.hip -- the Driver's test() on the reference's CIFAR network
// (Driver/src/main/c++/cppNN_backend.cpp:53-75 on the network of :128-138) on the device: the
// inference forward per image with arg_max and the Driver's cost (k_cifar_forward), then
// eval_kernels.hip's k_eval_reduce as it is (the ordered binary32 sum, the count and the
// two closing lines do not depend on the network). The arithmetic is cifar_forward.h's,
// host + device: every output element is computed by one lane in the reference's order.
//
// One launch, no workspace between stages. A 384-thread block takes kCifarImages images
// at a time and walks such groups grid-stride:
//   * C1's and C2's weights and biases (38.9 KB) are loaded to LDS once per block and
//     serve every image the block ever takes;
//   * the convolutions run one image at a time, all lanes on it: a lane takes one output
//     place for four maps (cifar_forward.h's conv_place: the 3x3 patch of an input channel
//     is read once for the four sums), C1 into LDS (16 x 900 floats; the reference's four
//     padding floats per map do not exist here, see cifar_forward.h), P1, C2 into the
//     same LDS region, P2 into the image's row of the group's P2 block;
//   * the fully connected layers then run for the whole group: a lane owns one neuron
//     and keeps one sum per image, so local4's 885 KB and local5's 295 KB are read once
//     per group, not once per image. Rows 576 (384) floats apart would not coalesce, so a
//     tile of 32 columns of every row goes through LDS transposed (pitch = rows + 1: the
//     lanes of a wave read neighbouring banks); the tile lies where C1 was;
//   * FC2 (N x 192, at most 77 KB) is read from memory row by row, then the softmax /
//     arg_max / cost tail of image g runs in lane g, in place on the nodes in LDS.
// LDS: 139,808 bytes per block, one block per CU; 134 VGPRs, no scratch (the fc tile loops
// are unrolled by four: unrolled whole, their 256 LDS reads per tile were hoisted and spilled).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "cifar_forward.h"
#include "fleet_codec.h"
#include "kernels.h"

namespace fleet {

// eval_kernels.hip's, launched with 256 threads
__global__ void k_eval_reduce(const float* __restrict__ cost, const int32_t* __restrict__ pred,
                              const int32_t* __restrict__ labels, const int32_t* __restrict__ idx, int64_t n_images,
                              int B, float* __restrict__ result);
constexpr int kEvalReduceThreads = 256;

constexpr int kCifarImages = 8;  // images a block takes at a time (fleet_cifar_block_images)
constexpr int kCifarThreads = 384;
constexpr int kFcTile = 32;      // columns of a fully connected layer staged at a time

// tile[col * (rows + 1) + row] = w[row * cols + c0 + col] for the kFcTile columns from c0
__device__ __forceinline__ void cifar_load_tile(float* tile, const float* __restrict__ w, int rows, int cols, int c0) {
  for (int e = threadIdx.x; e < rows * kFcTile; e += kCifarThreads) {
    const int row = e / kFcTile, col = e % kFcTile;
    tile[col * (rows + 1) + row] = w[(int64_t)row * cols + c0 + col];
  }
}

__global__ void __launch_bounds__(kCifarThreads)
    k_cifar_forward(int classes, const float* __restrict__ w, const float* __restrict__ b,
                    const float* __restrict__ images, int64_t n_images, int F, const int32_t* __restrict__ labels,
                    const int32_t* __restrict__ idx, int B, int32_t* __restrict__ pred, float* __restrict__ prob,
                    float* __restrict__ cost, float* __restrict__ probsN, int* __restrict__ err) {
  using namespace cifarnet;
  constexpr int G = kCifarImages;
  static_assert(kCifarThreads == kFc4 && kCifarThreads == 2 * kFc5 && G % 2 == 0, "a lane per neuron");
  static_assert(G * kFc4 <= kP1Out && G * (kFc5 + kMaxClasses) <= kPix, "the fc nodes lie where P1 and the image were");
  static_assert(kFcTile * (kFc4 + 1) <= kC1Out && kFcIn % kFcTile == 0 && kFc4 % kFcTile == 0, "the tile lies where C1 was");
  __shared__ float s_img[kPix];     // the fc phase: local5's nodes [G][192], then FC2's [G][classes]
  __shared__ float s_w1[kW2 - kW1];
  __shared__ float s_w2[kW4 - kW2];
  __shared__ float s_b[kB4];        // C1's and C2's biases
  __shared__ float s_c1[kC1Out];    // [16][900]; C2's outputs [64][144] once P1 is made; the fc phase: the weight tile
  __shared__ float s_p1[kP1Out];    // the fc phase: local4's nodes [G][384]
  __shared__ float s_p2[G][kFcIn];
  __shared__ int32_t s_label[G];
  float* const s_c2 = s_c1;
  float* const s_tile = s_c1;
  float* const s_h4 = s_p1;
  float* const s_h5 = s_img;
  float* const s_fc = s_img + G * kFc5;
  const int t = threadIdx.x;

  for (int i = t; i < kW2 - kW1; i += kCifarThreads) s_w1[i] = w[kW1 + i];
  for (int i = t; i < kW4 - kW2; i += kCifarThreads) s_w2[i] = w[kW2 + i];
  for (int i = t; i < kB4; i += kCifarThreads) s_b[i] = b[i];

  const int n_groups = (B + G - 1) / G;
  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    // the convolutions and the pools, one image at a time (block-uniform control flow)
    for (int g = 0; g < G; ++g) {
      const int k = grp * G + g;
      if (k >= B) {  // a slot past B: its fc sums run on zeros and nothing of it is written
        for (int i = t; i < kFcIn; i += kCifarThreads) s_p2[g][i] = 0.0f;
        if (t == 0) s_label[g] = 0;
        continue;
      }
      int64_t row = idx ? (int64_t)idx[k] : (int64_t)k;
      if (row < 0 || row >= n_images) {
        if (t == 0) atomicOr(err, FLEET_ERRBIT_ARG);
        row = 0;
      }
      for (int i = t; i < kPix; i += kCifarThreads) s_img[i] = images[row * F + i];
      if (t == 0) s_label[g] = labels[row];
      __syncthreads();  // the image (and, the first time, the weights)
      for (int it = t; it < kC1Items; it += kCifarThreads) c1_item(s_img, s_w1, s_b + kB1, it, s_c1);
      __syncthreads();
      for (int o = t; o < kP1Out; o += kCifarThreads) s_p1[o] = p1_out(s_c1, o);
      __syncthreads();  // C1 is done with: C2 overwrites it
      for (int it = t; it < kC2Items; it += kCifarThreads) c2_item(s_p1, s_w2, s_b + kB2, it, s_c2);
      __syncthreads();
      for (int o = t; o < kFcIn; o += kCifarThreads) s_p2[g][o] = p2_out(s_c2, o);
      __syncthreads();  // the next image overwrites s_img, s_c1 and s_p1
    }
    __syncthreads();  // (a group of skipped slots only: their zeros)

    // local4: lane t owns neuron t, one sum per image of the group
    {
      float acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = 0.0f;
      for (int c0 = 0; c0 < kFcIn; c0 += kFcTile) {
        __syncthreads();  // the tile before is consumed
        cifar_load_tile(s_tile, w + kW4, kFc4, kFcIn, c0);
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < kFcTile; ++i) {
          const float wv = s_tile[i * (kFc4 + 1) + t];
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g] = acc[g] + s_p2[g][c0 + i] * wv;
        }
      }
      const float bias = b[kB4 + t];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float a = acc[g];
        if (a != a) a = fc_x86(s_p2[g], w + kW4 + t * kFcIn, kFcIn);
        s_h4[g * kFc4 + t] = fc_relu(a, bias);
      }
    }

    // local5: lane t owns neuron t % 192 for half of the group's images
    {
      constexpr int H = G / 2;
      const int j = t % kFc5, g0 = (t / kFc5) * H;
      float acc[H];
#pragma unroll
      for (int g = 0; g < H; ++g) acc[g] = 0.0f;
      for (int c0 = 0; c0 < kFc4; c0 += kFcTile) {
        __syncthreads();  // the tile before is consumed (the first time: local4's nodes are written)
        cifar_load_tile(s_tile, w + kW5, kFc5, kFc4, c0);
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < kFcTile; ++i) {
          const float wv = s_tile[i * (kFc5 + 1) + j];
#pragma unroll
          for (int g = 0; g < H; ++g) acc[g] = acc[g] + s_h4[(g0 + g) * kFc4 + c0 + i] * wv;
        }
      }
      const float bias = b[kB5 + j];
#pragma unroll
      for (int g = 0; g < H; ++g) {
        float a = acc[g];
        if (a != a) a = fc_x86(s_h4 + (g0 + g) * kFc4, w + kW5 + j * kFc4, kFc4);
        s_h5[(g0 + g) * kFc5 + j] = fc_relu(a, bias);  // (the image in s_img is done with)
      }
    }
    __syncthreads();

    // FC2: node o = g*classes + j, its row read from memory
    for (int o = t; o < G * classes; o += kCifarThreads) {
      const int g = o / classes, j = o % classes;
      s_fc[o] = mojo_add(0.0f, fc_dot(s_h5 + g * kFc5, w + kWfc + j * kFc5, kFc5));
    }
    __syncthreads();

    // the tail of image g in lane g, in place on its nodes
    {
      const int k = grp * G + t;
      if (t < G && k < B) {
        const evalnet::Verdict v = tail(s_fc + t * classes, classes, s_label[t], probsN ? probsN + (int64_t)k * classes : nullptr);
        if (pred) pred[k] = v.pred;
        if (prob) prob[k] = v.p;
        cost[k] = v.cost;
      }
    }
    __syncthreads();  // the next group overwrites everything
  }
}

namespace {
std::atomic<int> g_cifar_grid{0};  // fleet_cifar_set_grid: tests walk several grid-stride passes at a small B
}

int cifar_block_images() { return kCifarImages; }
int cifar_set_grid(int max_blocks) { return g_cifar_grid.exchange(max_blocks < 0 ? 0 : max_blocks); }

hipError_t launch_cifar_test(int classes, const float* w, const float* b, const float* images, int64_t n_images, int F,
                             const int32_t* labels, const int32_t* idx, int B, int32_t* pred, float* prob, float* cost,
                             float* probsN, float* result, int* err, hipStream_t s) {
  if (!cifarnet::classes_ok(classes) || B <= 0 || F < cifarnet::kPix || !pred || !cost || !result)
    return hipErrorInvalidValue;
  const int n_groups = (B + kCifarImages - 1) / kCifarImages;
  int grid = g_cifar_grid.load();
  if (grid <= 0) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    grid = std::max(cus, 1);  // one block fits a CU's LDS
  }
  grid = std::min(grid, n_groups);
  hipLaunchKernelGGL(k_cifar_forward, dim3((unsigned)grid), dim3(kCifarThreads), 0, s, classes, w, b, images, n_images,
                     F, labels, idx, B, pred, prob, cost, probsN, err);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_eval_reduce, dim3(1), dim3(kEvalReduceThreads), 0, s, cost, pred, labels, idx, n_images, B, result);
  return hipGetLastError();
}

}  // namespace fleet

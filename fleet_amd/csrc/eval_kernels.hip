// fleet_amd/csrc/eval_kernels.hip -- the Driver's test() on the device
// (Driver/src/main/c++/cppNN_backend.cpp:53-75; evaluateNative :201-205): the
// inference forward of the MNIST network per image with arg_max and the Driver's
// cost (k_eval_forward), then the ordered binary32 sum, the count and the two
// closing lines (k_eval_reduce). The arithmetic is eval_forward.h's, host + device.
//
// k_eval_forward is shaped for thousands of images where k_teacher_forward
// (teacher.hip) is shaped for a mini-batch. A 256-thread block takes kEvalImages
// images at a time and walks such groups grid-stride:
//   * C1's, C2i's and FC2's weights and every bias (9.4 KB) are loaded to LDS once
//     per block and serve every image the block ever takes;
//   * C1 and P1 are one stage: a lane makes a pooled value from the 7x7 input patch
//     in registers, so the 18 KB of C1 outputs per image never exist;
//   * C2 and P2 are one stage, image g in the g-th 256 / kEvalImages lanes (one
//     image per wave at kEvalImages = 4): a lane keeps one P2 window's four sums
//     for three of the 48 maps in registers and advances them one input channel at
//     a time, from the window's 6x6 patch read once per channel; the channel's
//     48x25 weights (4.8 KB of C2's 77 KB) are staged through a double-buffered LDS
//     slice, one barrier per channel, and serve every image of the group;
//   * FC2 and the softmax / arg_max / cost tail of image g run in the same lanes.
// The per-output order of operations is teacher.hip's; only the assignment of
// outputs to lanes differs. The image shares its LDS with the C2i outputs that
// replace it: 46.8 KB per block at kEvalImages = 4, three blocks per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "eval_forward.h"
#include "fleet_codec.h"
#include "kernels.h"

namespace fleet {

constexpr int kEvalImages = 4;     // images a block takes at a time (fleet_evaluate_block_images)
constexpr int kEvalThreads = 256;
constexpr int kFcPitch = evalnet::kFcIn + 1;  // FC2 rows 193 floats apart in LDS: ten rows, ten banks
constexpr int kReduceChunk = 1024;

template <int G>
__global__ void __launch_bounds__(kEvalThreads)
    k_eval_forward(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ images,
                   int64_t n_images, int F, const int32_t* __restrict__ labels, const int32_t* __restrict__ idx, int B,
                   int32_t* __restrict__ pred, float* __restrict__ prob, float* __restrict__ cost,
                   float* __restrict__ probs10, int* __restrict__ err) {
  using namespace evalnet;
  static_assert(G >= 1 && G <= 16 && kEvalThreads % G == 0, "a slot of lanes per image");
  constexpr int kSlot = kEvalThreads / G;
  __shared__ float s_w1[kMaps1 * 25];
  __shared__ float s_w2i[kMaps2i * kMaps1];
  __shared__ float s_wfc[kClasses * kFcPitch];
  __shared__ float s_b[kBTotal];
  __shared__ float s_w2[2][kC2Slice];
  __shared__ float s_c2i[G][kC2iOut];  // its head is the image first: C1 + P1 is done with it before C2i writes
  __shared__ float s_p1[G][kP1Out];
  __shared__ float s_p2[G][kFcIn];
  __shared__ float s_fc[G][kClasses];
  __shared__ int32_t s_label[G];
  float(*s_in)[kC2iOut] = s_c2i;
  const int t = threadIdx.x;

  for (int i = t; i < kMaps1 * 25; i += kEvalThreads) s_w1[i] = w[kW1 + i];
  for (int i = t; i < kMaps2i * kMaps1; i += kEvalThreads) s_w2i[i] = w[kW2i + i];
  for (int i = t; i < kClasses * kFcIn; i += kEvalThreads) s_wfc[(i / kFcIn) * kFcPitch + i % kFcIn] = w[kWfc + i];
  for (int i = t; i < kBTotal; i += kEvalThreads) s_b[i] = b[i];

  const int n_groups = (B + G - 1) / G;
  for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    // the group's images (a slot past B computes on zeros and writes nothing)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k = grp * G + g;
      if (k < B) {
        int64_t row = idx ? (int64_t)idx[k] : (int64_t)k;
        if (row < 0 || row >= n_images) {  // block-uniform
          if (t == 0) atomicOr(err, FLEET_ERRBIT_ARG);
          row = 0;
        }
        for (int i = t; i < kPix; i += kEvalThreads) s_in[g][i] = images[row * F + i];
        if (t == 0) s_label[g] = labels[row];
      } else {
        for (int i = t; i < kPix; i += kEvalThreads) s_in[g][i] = 0.0f;
        if (t == 0) s_label[g] = 0;
      }
    }
    for (int i = t; i < kC2Slice; i += kEvalThreads) s_w2[0][i] = w[kW2 + i];
    __syncthreads();

    // C1 + P1
    for (int o = t; o < G * kP1Out; o += kEvalThreads) {
      const int g = o / kP1Out, oo = o % kP1Out;
      s_p1[g][oo] = c1p1(s_in[g], s_w1, s_b + kB1, oo);
    }
    __syncthreads();

    // C2i
    for (int o = t; o < G * kC2iOut; o += kEvalThreads) {
      const int g = o / kC2iOut, oo = o % kC2iOut;
      s_c2i[g][oo] = c2i(s_p1[g], s_w2i, s_b + kB2i, oo);
    }
    __syncthreads();

    // C2 + P2: image g in the g-th slot of lanes; a lane takes one window of kMaps2 / (kSlot / 4)
    // maps, so the window's 6x6 patch serves them all; channel slices through LDS
    {
      constexpr int kLaneMaps = kSlot / 4;             // maps a slot covers at a time
      constexpr int kPer = kMaps2 / kLaneMaps;         // maps per lane
      static_assert(kSlot % 4 == 0 && kMaps2 % kLaneMaps == 0, "a slot covers C2's maps evenly");
      const int g = t / kSlot, l = t % kSlot, map0 = l / 4, wy = (l % 4) / 2, wx = l % 2;
      float acc[kPer][4];
#pragma unroll
      for (int j = 0; j < kPer; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
      for (int k = 0; k < kMaps2i; ++k) {
        if (k + 1 < kMaps2i)
          for (int i = t; i < kC2Slice; i += kEvalThreads) s_w2[(k + 1) & 1][i] = w[kW2 + (k + 1) * kC2Slice + i];
        float patch[36];
        c2_patch(patch, s_c2i[g] + k * kP1 * kP1, wy, wx);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          float wk[25];
#pragma unroll
          for (int i = 0; i < 25; ++i) wk[i] = s_w2[k & 1][(map0 + j * kLaneMaps) * 25 + i];
          c2_taps(acc[j], patch, wk);
        }
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int map = map0 + j * kLaneMaps;
        s_p2[g][map * 4 + l % 4] = c2p2_finish(acc[j], s_c2i[g], w + kW2, s_b[kB2 + map], map, wy, wx);
      }
    }
    __syncthreads();

    // FC2 and the tail: image g in the g-th slot of lanes
    {
      const int g = t / kSlot, j = t % kSlot;
      if (j < kClasses) s_fc[g][j] = fc(s_p2[g], s_wfc + j * kFcPitch);
      __syncthreads();
      const int k = grp * G + g;
      if (j == 0 && k < B) {
        float in[kClasses];
#pragma unroll
        for (int q = 0; q < kClasses; ++q) in[q] = s_fc[g][q];
        const Verdict v = tail(in, s_label[g], probs10 ? probs10 + (int64_t)k * kClasses : nullptr);
        if (pred) pred[k] = v.pred;
        if (prob) prob[k] = v.p;
        cost[k] = v.cost;
      }
    }
    __syncthreads();  // the next group overwrites s_in .. s_fc
  }
}

// One block: the count (integer, any order), the costs added in image order in
// binary32 by one lane from LDS chunks the block loads a chunk ahead, then test()'s
// two closing lines. result: float error, float accuracy, int32 correct.
__global__ void __launch_bounds__(kEvalThreads)
    k_eval_reduce(const float* __restrict__ cost, const int32_t* __restrict__ pred, const int32_t* __restrict__ labels,
                  const int32_t* __restrict__ idx, int64_t n_images, int B, float* __restrict__ result) {
  __shared__ __attribute__((aligned(16))) float s_cost[2][kReduceChunk];
  __shared__ int s_correct;
  const int t = threadIdx.x;
  if (t == 0) s_correct = 0;
  int c = 0;
  for (int k = t; k < B; k += kEvalThreads) {
    int64_t row = idx ? (int64_t)idx[k] : (int64_t)k;
    if (row < 0 || row >= n_images) row = 0;  // k_eval_forward has set the error bit
    c += pred[k] == labels[row];
  }
  for (int i = t; i < kReduceChunk && i < B; i += kEvalThreads) s_cost[0][i] = cost[i];
  __syncthreads();
  atomicAdd(&s_correct, c);
  const int n_chunks = (B + kReduceChunk - 1) / kReduceChunk;
  float sum = 0.0f;
  for (int ch = 0; ch < n_chunks; ++ch) {
    if (ch + 1 < n_chunks) {
      const int base = (ch + 1) * kReduceChunk;
      for (int i = t; i < kReduceChunk && base + i < B; i += kEvalThreads) s_cost[(ch + 1) & 1][i] = cost[base + i];
    }
    if (t == 0) {
      // 32 costs at a time, the next 32 on their way from LDS while these are added
      const int n = min(kReduceChunk, B - ch * kReduceChunk), n32 = n / 32;
      const float* s = s_cost[ch & 1];
      const float4* s4 = (const float4*)s;
      float4 cur[8], nxt[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) cur[q] = nxt[q] = s4[q];  // (a chunk shorter than 32 reads its buffer, adds nothing)
      for (int blk = 0; blk < n32; ++blk) {
        if (blk + 1 < n32) {
#pragma unroll
          for (int q = 0; q < 8; ++q) nxt[q] = s4[(blk + 1) * 8 + q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          sum = sum + cur[q].x;
          sum = sum + cur[q].y;
          sum = sum + cur[q].z;
          sum = sum + cur[q].w;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) cur[q] = nxt[q];
      }
      for (int i = n32 * 32; i < n; ++i) sum = sum + s[i];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (sum != sum) sum = evalnet::sum_x86(cost, B);
    float error, accuracy;
    evalnet::finish(sum, s_correct, B, &error, &accuracy);
    result[0] = error;
    result[1] = accuracy;
    ((int32_t*)result)[2] = s_correct;
  }
}

namespace {
std::atomic<int> g_eval_grid{0};  // fleet_evaluate_set_grid: tests walk a grid-stride pass at a small B
}

int eval_block_images() { return kEvalImages; }
int eval_set_grid(int max_blocks) { return g_eval_grid.exchange(max_blocks < 0 ? 0 : max_blocks); }

hipError_t launch_eval(const float* w, const float* b, const float* images, int64_t n_images, int F,
                       const int32_t* labels, const int32_t* idx, int B, int32_t* pred, float* prob, float* cost,
                       float* probs10, float* result, int* err, hipStream_t s) {
  if (B <= 0 || F < evalnet::kPix || !pred || !cost || !result) return hipErrorInvalidValue;
  const int n_groups = (B + kEvalImages - 1) / kEvalImages;
  int grid = g_eval_grid.load();
  if (grid <= 0) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    grid = 3 * std::max(cus, 1);  // three blocks fit a CU's LDS
  }
  grid = std::min(grid, n_groups);
  hipLaunchKernelGGL(k_eval_forward<kEvalImages>, dim3((unsigned)grid), dim3(kEvalThreads), 0, s, w, b, images,
                     n_images, F, labels, idx, B, pred, prob, cost, probs10, err);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_eval_reduce, dim3(1), dim3(kEvalThreads), 0, s, cost, pred, labels, idx, n_images, B, result);
  return hipGetLastError();
}

}  // namespace fleet

// fleet_amd/csrc/cifar_client_kernels.hip -- the client's gradient computation on the CIFAR
// network on the device: for C clients of B samples each, the float vector cnn.gradients()
// returns after B train_class calls (commonLib/cppNN/network.h:1806-2008, 1551-1611, 1289-1331,
// 1038-1056). The arithmetic and its order are cifar_backward.h's, documented at its head; this
// unit only places it.
//
//   k_rgb_sample  one 512-thread block per (client, sample). The sample's layers live in LDS
//                 (rgbnet::Sample, 158,436 of the CU's 163,840 bytes), the stages run one after
//                 the other with a barrier between them, every element computed by one lane,
//                 serially, in the reference's order. The block writes the sample's RECORD
//                 (18,160 + N floats): C1's and C2's dW, the six dbias blocks and the nodes of
//                 P2, local4 and local5. The three fully connected dW blocks, 96 % of the
//                 vector, are never stored per sample.
//   k_rgb_sum     one lane per (client, element) of the records' summed part and of the header
//                 slots: the records added in sample order in binary32.
//   k_rgb_fc_sum  the fully connected dW blocks as an ordered rank-B sum. A 256-thread block
//                 owns a tile of 32 rows (delta) x 64 columns (node) of one block of one client:
//                 lane (wave v, lane l) keeps eight sums, rows 8v .. 8v+7 at column l, in
//                 registers. The node and delta slices of kSampleTile samples at a time are
//                 staged in LDS (6 KB), a sample's node read once per lane (consecutive banks)
//                 and its eight deltas as broadcasts; sample 0 leaves the bare product, every
//                 later one adds its rounded product, in sample order. The tile is written
//                 once, a wave's 64 columns of a row together.
// DPgradients(C, sigma), for the chunks that hold a client with sigma > 0:
//   k_rgb_clip      one lane per clipped sample, 64 samples' chains side by side in a wave: the
//                   scale of every (client, sample >= 1) from the records, the fully connected
//                   squares recomputed from node[t] * delta[b]; no per-sample row is written
//   k_rgb_sum_dp    k_rgb_sum with the dbias elements of samples >= 1 times their scale, the
//                   noise added in binary64 and the sizes in the header slots
//   k_rgb_fc_sum_dp k_rgb_fc_sum's body with the noise added as the tile is written
//
// What lives where in k_rgb_sample (floats; 40,960 fit a CU):
//   img   3,072  shift .. C1's dW        c1 14,400  node, then its own delta (df in place)
//   w1      432  forward and reversed    c2  9,216  node, then its own delta (df in place)
//   p1    3,136  node, until C2's dW     d_p1 3,136 forward: the fc weight tile; then P1's delta
//   pm1   3,136  P1's picks              p2, pm2, d_p2 576 each; h4, d4 384; h5, d5 192; fc, d_fc 100
// Not stored: the padded deltas of C2 and C1 (65 KB and 74 KB: bounds checks read the padding's
// zeros instead), I1's delta (written straight into the record) and C2's weights (36 KB): they
// are read from memory, forward and reversed, every lane of a wave nearly always the same
// address. No per-block scratch row in HBM is needed.
// No atomics on values, no cross-lane sums, no MFMA (an MFMA accumulation is not the
// reference's sequence of rounded adds), no contraction (the unit builds with
// -ffp-contract=off -fno-slp-vectorize and without packed fp32 operations).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "cifar_backward.h"
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

constexpr int kSampleThreads = 512;
constexpr int kSumThreads = 256;
constexpr int kSampleTile = 16;               // samples staged at a time in k_rgb_fc_sum
constexpr int kTileCols = 64, kTileRows = 32;  // a tile: a wave per 8 rows, a lane per column
constexpr int kLaneRows = 8;

__host__ __device__ inline int fc_tiles(const rgbnet::FcBlock& f) {
  return ((f.rows + kTileRows - 1) / kTileRows) * (f.cols / kTileCols);
}

}  // namespace

// block = (client c0 + blockIdx.x / B, sample blockIdx.x % B); recs: the chunk's workspace,
// record blockIdx.x. An index outside the images or the model rows or a shift outside
// {-1, 0, 1} sets FLEET_ERRBIT_ARG and the block computes on image / model 0 unshifted (its
// output is not to be used); E NaN sets FLEET_ERRBIT_NAN.
__global__ void __launch_bounds__(kSampleThreads)
    k_rgb_sample(int classes, const float* __restrict__ models, int64_t model_pitch, int n_models,
                 const int32_t* __restrict__ model_of_client, const float* __restrict__ images, int64_t n_images, int F,
                 const int32_t* __restrict__ labels, const int32_t* __restrict__ idx, const int32_t* __restrict__ shift,
                 int c0, int B, float temperature, float* __restrict__ recs, int* __restrict__ err) {
  using namespace rgbnet;
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
  const bool finite = sample_stages(BlockPar{}, S, classes, w, w + weight_count(classes), images + img * F, labels[img],
                                    dx, dy, temperature, recs + (int64_t)blockIdx.x * record_len(classes));
  if (!finite && threadIdx.x == 0) atomicOr(err, FLEET_ERRBIT_NAN);
}

// lane = (client, q): q below summed_len the element of the records' summed part, the next
// kHeaders the header slots
__global__ void __launch_bounds__(kSumThreads)
    k_rgb_sum(int classes, const float* __restrict__ recs, int B, int clients, float* __restrict__ grads,
              int64_t grad_pitch) {
  using namespace rgbnet;
  const int per = summed_len(classes) + kHeaders;
  const int64_t i = (int64_t)blockIdx.x * kSumThreads + threadIdx.x;
  if (i >= (int64_t)clients * per) return;
  const int c = (int)(i / per), q = (int)(i % per);
  float* row = grads + (int64_t)c * grad_pitch;
  if (q >= summed_len(classes)) {
    const Header h = header(q - summed_len(classes), classes);
    row[h.pos] = h.value;
    return;
  }
  const int64_t pitch = record_len(classes);
  row[summed_pos(q, classes)] = sum_element(recs + (int64_t)c * B * pitch, pitch, B, q);
}

// block = (client blockIdx.x / tiles, tile blockIdx.x % tiles), tiles counted through the
// three blocks, a block's tiles row-major. Rows past the block's last (FC2's N is no multiple
// of 32) stage delta 0 and are not written.
// One body for the plain and the DP kernel, as text (a shared __forceinline__ template gave the
// plain kernel 8 more bytes of code): VALUE is what lane (row, t0 + lane) stores, the rest of the
// arguments are appended to the kernel's.
#define FLEET_RGB_FC_SUM_KERNEL(NAME, VALUE, ...)                                                                     \
  __global__ void __launch_bounds__(256)                                                                              \
      NAME(int classes, const float* __restrict__ recs, int B, int tiles, float* __restrict__ grads,                  \
           int64_t grad_pitch __VA_ARGS__) {                                                                          \
    using namespace rgbnet;                                                                                           \
    __shared__ float s_node[kSampleTile][kTileCols];                                                                  \
    __shared__ float s_delta[kSampleTile][kTileRows];                                                                 \
    const int c = (int)(blockIdx.x / (unsigned)tiles);                                                                \
    int tile = (int)(blockIdx.x % (unsigned)tiles), blk = 0;                                                          \
    FcBlock f = fc_block(0, classes);                                                                                 \
    while (tile >= fc_tiles(f)) tile -= fc_tiles(f), f = fc_block(++blk, classes); /* block-uniform */                \
    const int col_tiles = f.cols / kTileCols;                                                                         \
    const int r0 = (tile / col_tiles) * kTileRows, t0 = (tile % col_tiles) * kTileCols;                               \
    const int64_t pitch = record_len(classes);                                                                        \
    const float* rec = recs + (int64_t)c * B * pitch;                                                                 \
    const int lane = threadIdx.x % kTileCols, wave = threadIdx.x / kTileCols;                                         \
    float acc[kLaneRows];                                                                                             \
    _Pragma("unroll") for (int r = 0; r < kLaneRows; ++r) acc[r] = 0.0f;                                              \
    for (int s0 = 0; s0 < B; s0 += kSampleTile) {                                                                     \
      const int n = B - s0 < kSampleTile ? B - s0 : kSampleTile;                                                      \
      __syncthreads(); /* the slices before are consumed */                                                           \
      for (int e = threadIdx.x; e < n * kTileCols; e += 256)                                                          \
        s_node[e / kTileCols][e % kTileCols] =                                                                        \
            rec[(int64_t)(s0 + e / kTileCols) * pitch + f.node + t0 + e % kTileCols];                                 \
      for (int e = threadIdx.x; e < n * kTileRows; e += 256) {                                                        \
        const int r = r0 + e % kTileRows;                                                                             \
        s_delta[e / kTileRows][e % kTileRows] =                                                                       \
            r < f.rows ? rec[(int64_t)(s0 + e / kTileRows) * pitch + f.delta + r] : 0.0f;                             \
      }                                                                                                               \
      __syncthreads();                                                                                                \
      for (int s = 0; s < n; ++s) {                                                                                   \
        const float node = s_node[s][lane];                                                                           \
        const bool first = s0 + s == 0;                                                                               \
        _Pragma("unroll") for (int r = 0; r < kLaneRows; ++r) acc[r] =                                                \
            fc_step(acc[r], first, node, s_delta[s][wave * kLaneRows + r]);                                           \
      }                                                                                                               \
    }                                                                                                                 \
    float* out = grads + (int64_t)c * grad_pitch + f.pos;                                                             \
    _Pragma("unroll") for (int r = 0; r < kLaneRows; ++r) {                                                           \
      const int row = r0 + wave * kLaneRows + r;                                                                      \
      if (row < f.rows) out[(int64_t)row * f.cols + t0 + lane] = VALUE;                                               \
    }                                                                                                                 \
  }

// the DP kernel's arguments: the chunk's first client, clip and sigma [C] of the whole call, the draws
struct RgbDp {
  int c0;
  const float *clip, *sigma;
  const double* z;
};

// client c0 + c with sigma > 0 adds addGaussian's draw of the element's slot, z[slot] * s in
// binary64, as the tile is written
__device__ __forceinline__ float rgb_fc_noisy(const RgbDp& dp, int c, float sum, int64_t slot) {
  const float sg = dp.sigma[dp.c0 + c];  // block-uniform
  return sg > 0.0f ? clientnet::noisy(sum, dp.z[slot], (double)(dp.clip[dp.c0 + c] * sg)) : sum;
}

FLEET_RGB_FC_SUM_KERNEL(k_rgb_fc_sum, acc[r])
FLEET_RGB_FC_SUM_KERNEL(k_rgb_fc_sum_dp, rgb_fc_noisy(dp, c, acc[r], f.pos + (int64_t)row * f.cols + t0 + lane), , RgbDp dp)

// scale_gradients (network.h:1092-1112) with one lane per sample: block = one wave, lane l the
// clipped sample (client lc, slot k >= 1) number 64 * blockIdx.x + l of the chunk, lc-major; B >= 2.
// A lane carries its sample's whole chain, 313,850 dependent binary32 adds in the walk's order
// (cifar_backward.h: FLEET_RGB_CLIP_ORDER), so every multiply and add of the wave is 64 chains
// wide. The values come through one LDS tile laid out [t][lane] (pitch 65: the transposed
// staging writes and the walk's reads both touch 64 different banks): lane l copies value t0 + l
// of record r, for r = 0 .. 63, a coalesced 256-byte read each. A fully connected dW block is
// walked row b outer, t inner, so its WHOLE node vector (up to 576 values of 64 samples, 150 KB)
// is staged once and read rows times, delta[b] in a register and the next row's on its way; a
// slice of t would have to be staged again for every row. The record's own blocks go through the
// same tile 576 values at a time.
// Lanes past the chunk's last sample or of a client with sigma = 0 are masked: their chains run
// and nothing of them is written. A wave without a live lane leaves at once. scale:
// [clients][B]; clip, sigma: [C] of the whole call.
constexpr int kClipLanes = 64;
constexpr int kClipRows = rgbnet::kFcIn;     // values per sample the tile holds
constexpr int kClipPitch = kClipLanes + 1;  // floats between two values of a sample
static_assert(rgbnet::kFcIn % 16 == 0 && rgbnet::kFc4 % 16 == 0 && rgbnet::kFc5 % 16 == 0 &&
                  rgbnet::kFc4 <= kClipRows && rgbnet::kFc5 <= kClipRows,
              "a fully connected layer's input fits the tile in whole groups of 16");

__global__ void __launch_bounds__(kClipLanes)
    k_rgb_clip(int classes, const float* __restrict__ recs, int c0, int B, int clients, const float* __restrict__ clip,
               const float* __restrict__ sigma, float* __restrict__ scale) {
  using namespace rgbnet;
  __shared__ float tile[kClipRows * kClipPitch];
  __shared__ int s_rec[kClipLanes];  // the record of lane r's sample
  const int lane = threadIdx.x;
  const int64_t slot = (int64_t)blockIdx.x * kClipLanes + lane;
  const bool in = slot < (int64_t)clients * (B - 1);
  const int lc = in ? (int)(slot / (B - 1)) : 0, k = in ? 1 + (int)(slot % (B - 1)) : 0;
  const bool live = in && sigma[c0 + lc] > 0.0f;
  if (__ballot(live) == 0) return;  // wave-uniform: the block is one wave
  // a masked lane stands for a record of the chunk all the same (the client's first, or the
  // chunk's): the staging loop then has no branch, and nothing of that lane is used
  const int mine = lc * B + k;
  s_rec[lane] = mine;
  const int64_t pitch = record_len(classes);
  // n <= kClipRows values at `off` of every lane's record into tile[t][lane]
  auto stage = [&](int off, int n) {
    __syncthreads();  // the tile before is consumed (and s_rec written)
#pragma unroll 8
    for (int r = 0; r < kClipLanes; ++r) {
      const float* src = recs + (int64_t)__builtin_amdgcn_readfirstlane(s_rec[r]) * pitch + off;
      for (int t = lane; t < n; t += kClipLanes) tile[t * kClipPitch + r] = src[t];
    }
    __syncthreads();
  };
  const float* x = tile + lane;
  float sqsum = 0.0f;
#pragma unroll 1
  for (int i = 0; i < kClipSegments; ++i) {
    const ClipSegment sg = clip_segment(i, classes);  // wave-uniform
    if (sg.fc < 0) {
      for (int base = 0; base < sg.len; base += kClipRows) {
        const int n = sg.len - base < kClipRows ? sg.len - base : kClipRows;
        stage(sg.rec + base, n);
        for (int t = 0; t < n; ++t) sqsum = clip_add(sqsum, x[t * kClipPitch]);
      }
      continue;
    }
    const FcBlock f = fc_block(sg.fc, classes);
    stage(f.node, f.cols);
    const float* delta = recs + (int64_t)mine * pitch + f.delta;
    float d = delta[0];
#pragma unroll 1
    for (int b = 0; b < f.rows; ++b) {
      const float next = delta[b + 1 < f.rows ? b + 1 : b];  // in flight while row b is walked
      for (int t = 0; t < f.cols; t += 16) {
#pragma unroll
        for (int u = 0; u < 16; ++u) sqsum = clip_add(sqsum, x[(t + u) * kClipPitch] * d);
      }
      d = next;
    }
  }
  if (live) {
    scale[mine] = clientnet::clip_scale(sqsum, clip[c0 + lc]);
    if (k == 1) scale[(int64_t)lc * B] = 1.0f;
  }
}

// k_rgb_sum for a chunk with a DP client: a client with sigma = 0 gets k_rgb_sum's value; for
// the others the dbias elements of samples >= 1 are added times their scale (no dW is scaled),
// the slot's draw is added in binary64, and the header slots give the sizes. scale: [clients][B]
// as k_rgb_clip wrote it (not read where B = 1)
__global__ void __launch_bounds__(kSumThreads)
    k_rgb_sum_dp(int classes, const float* __restrict__ recs, int B, int clients, int c0, const float* __restrict__ clip,
                 const float* __restrict__ sigma, const float* __restrict__ scale, const double* __restrict__ z,
                 float* __restrict__ grads, int64_t grad_pitch) {
  using namespace rgbnet;
  const int per = summed_len(classes) + kHeaders;
  const int64_t i = (int64_t)blockIdx.x * kSumThreads + threadIdx.x;
  if (i >= (int64_t)clients * per) return;
  const int c = (int)(i / per), q = (int)(i % per);
  float* row = grads + (int64_t)c * grad_pitch;
  if (q >= summed_len(classes)) {
    const Header h = header(q - summed_len(classes), classes);
    row[h.pos] = h.value;
    return;
  }
  const int64_t pitch = record_len(classes);
  const float* rec = recs + (int64_t)c * B * pitch;
  const float sg = sigma[c0 + c];
  const int pos = summed_pos(q, classes);
  row[pos] = sg > 0.0f ? clientnet::noisy(dp_sum_element(rec, pitch, B, q, scale + (int64_t)c * B), z[pos],
                                          (double)(clip[c0 + c] * sg))
                       : sum_element(rec, pitch, B, q);
}

namespace {
std::atomic<int> g_rgb_chunk{0};
constexpr size_t kRgbWorkspaceCap = (size_t)256 << 20;  // bytes of records in flight
}  // namespace

int64_t rgbnet_grad_len(int classes) { return rgbnet::grad_len(classes); }
int rgbnet_sample_tile() { return kSampleTile; }
int rgbnet_set_chunk(int max_clients) { return g_rgb_chunk.exchange(max_clients > 0 ? max_clients : 0); }

// clients per chunk for B samples each: the override, else what fits the cap (at least one)
int rgbnet_chunk(int classes, int C, int B) {
  const int forced = g_rgb_chunk.load();
  size_t n = forced > 0 ? (size_t)forced : kRgbWorkspaceCap / rgbnet_workspace_bytes(classes, 1, B);
  if (n < 1) n = 1;
  return n > (size_t)C ? C : (int)n;
}

size_t rgbnet_workspace_bytes(int classes, int chunk, int B) {
  return (size_t)chunk * (size_t)B * (size_t)rgbnet::record_len(classes) * sizeof(float);
}

// the scales of a chunk live behind its records: [chunk][B] floats
size_t rgbnet_scale_bytes(int chunk, int B) { return (size_t)chunk * (size_t)B * sizeof(float); }

hipError_t launch_rgbnet_grads(int classes, const float* models, int64_t model_pitch, int n_models,
                               const int32_t* model_of_client, const float* images, int64_t n_images, int F,
                               const int32_t* labels, const int32_t* idx, const int32_t* shift, int C, int B, int chunk,
                               float temperature, float* workspace, float* grads, int64_t grad_pitch, int* err,
                               hipStream_t s) {
  return launch_rgbnet_grads_dp(classes, models, model_pitch, n_models, model_of_client, images, n_images, F, labels, idx,
                                shift, C, B, chunk, temperature, nullptr, nullptr, nullptr, nullptr, nullptr, workspace,
                                grads, grad_pitch, err, s);
}

// DP where d_clip is given: d_clip, d_sigma [C] on the device, dp_of_client [C] on the host
// (non-zero: sigma > 0, for the launch decisions alone), d_z the grad_len(classes) draws, scale:
// rgbnet_scale_bytes(chunk, B) on the device. A chunk without a DP client launches the plain kernels.
hipError_t launch_rgbnet_grads_dp(int classes, const float* models, int64_t model_pitch, int n_models,
                                  const int32_t* model_of_client, const float* images, int64_t n_images, int F,
                                  const int32_t* labels, const int32_t* idx, const int32_t* shift, int C, int B,
                                  int chunk, float temperature, const float* d_clip, const float* d_sigma,
                                  const uint8_t* dp_of_client, const double* d_z, float* scale, float* workspace,
                                  float* grads, int64_t grad_pitch, int* err, hipStream_t s) {
  using namespace rgbnet;
  if (!classes_ok(classes) || C <= 0 || B <= 0 || chunk <= 0 || F < kPix || grad_pitch < grad_len(classes) ||
      model_pitch < weight_count(classes) + bias_count(classes) || (int64_t)chunk * B > INT32_MAX ||
      (d_clip && (!d_sigma || !dp_of_client || !d_z || !scale)))
    return hipErrorInvalidValue;
  int tiles = 0;
  for (int i = 0; i < kFcBlocks; ++i) tiles += fc_tiles(fc_block(i, classes));
  if ((int64_t)chunk * tiles > INT32_MAX) return hipErrorInvalidValue;
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int n = C - c0 < chunk ? C - c0 : chunk;
    float* rows = grads + (int64_t)c0 * grad_pitch;
    hipLaunchKernelGGL(k_rgb_sample, dim3((unsigned)(n * B)), dim3(kSampleThreads), 0, s, classes, models, model_pitch,
                       n_models, model_of_client, images, n_images, F, labels, idx, shift, c0, B, temperature, workspace,
                       err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t elems = (int64_t)n * (summed_len(classes) + kHeaders);
    const dim3 sum_grid((unsigned)((elems + kSumThreads - 1) / kSumThreads));
    bool dp = false;  // a client of this chunk with sigma > 0
    for (int c = c0; d_clip && c < c0 + n; ++c) dp |= dp_of_client[c] != 0;
    if (!dp) {
      hipLaunchKernelGGL(k_rgb_sum, sum_grid, dim3(kSumThreads), 0, s, classes, workspace, B, n, rows, grad_pitch);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      hipLaunchKernelGGL(k_rgb_fc_sum, dim3((unsigned)(n * tiles)), dim3(256), 0, s, classes, workspace, B, tiles, rows,
                         grad_pitch);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      continue;
    }
    if (B > 1) {
      const int64_t waves = ((int64_t)n * (B - 1) + kClipLanes - 1) / kClipLanes;
      hipLaunchKernelGGL(k_rgb_clip, dim3((unsigned)waves), dim3(kClipLanes), 0, s, classes, workspace, c0, B, n, d_clip,
                         d_sigma, scale);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_rgb_sum_dp, sum_grid, dim3(kSumThreads), 0, s, classes, workspace, B, n, c0, d_clip, d_sigma,
                       scale, d_z, rows, grad_pitch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_rgb_fc_sum_dp, dim3((unsigned)(n * tiles)), dim3(256), 0, s, classes, workspace, B, tiles, rows,
                       grad_pitch, RgbDp{c0, d_clip, d_sigma, d_z});
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace fleet

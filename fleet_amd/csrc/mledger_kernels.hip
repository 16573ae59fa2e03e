// fleet_amd/csrc/mledger_kernels.hip -- the Kardam model ledger's kernels (fleet_mledger_*):
// a model version made resident as one fp32 row (k_mrow_stage), and the norms
// Kardam.setModel asks for, for every ordered pair of rows of an update in one launch
// (k_mrow_pair_norms, k_mrow_reduce).
//
// kardam.setModel(pickedId, pickedModel) (CppNNUpdater.java:472-476, Kardam.java:114-125)
// takes T_v = getModelParametersNative(v) (cppNN_backend.cpp:227-242: Base64::encode of
// getModelParams, the biases repeated once per layer-graph edge, then the weights) and
// computes getNorm(subtractNative(T_v, models[w])) (cppNN_backend.cpp:779-795, 848-892).
// Per element, with Q = decodeFloat o encode on one float (codec_math.h q):
//   a = Q(P_v[i])   b = Q(P_u[i])   D = Q(a - b)   norm = sqrt(sum (double)(D * D))
// A resident row holds a, what decoding the text gives: Q applied ONCE (Q is not
// idempotent, so a row is never re-quantised), and no Base64 text is ever built.
// The subtraction is not symmetric (Q(-1) != -Q(1)): pairs are ordered (cur, prev).
//
// A lane owns 4 consecutive values (16 bytes of a row; rows are padded with zeros to
// whole quads) and every Q is q_stage_d16x: the table stage, with the general codec per
// lane for values outside its domain (non-finite and huge parameters), wave-uniform
// behind a ballot. A block copies the tables into LDS once and strides over the row, at
// most kMlMaxTiles blocks per row or pair. The norms follow the ledger's rule: a lane
// sums its own values in order, the wave folds by DPP lane moves (group_sum_f64), lane 0
// adds the block's four waves in order, and k_mrow_reduce adds the blocks' partials in a
// fixed order. No floating-point atomics: the same inputs give the same bits.
//
// This unit takes the stage helpers of kernels.hip and none of its kernels.
#define FLEET_STREAM_TU
#define FLEET_ACC_TU
#include "kernels.hip"

namespace fleet {

namespace {

constexpr int kMlNT = 256;
static_assert(kMlMaxTiles <= 64, "k_mrow_reduce adds a row's or pair's partials in one wave");

typedef float f4 __attribute__((ext_vector_type(4)));

struct MlShared {
  B64Tables tab;  // (its digit-count rows: the compare of q_stage_d16x)
  D16Table dtab;
  double red[kMlNT / 64];
};

__device__ __forceinline__ void ml_block_open(MlShared& sh) {
  b64_tables_init<kMlNT>(&sh.tab);
  d16_table_init<kMlNT>(&sh.dtab);
  __syncthreads();
}

// The block's sum of every lane's s into *out: wave by wave, then the waves in order.
// Every lane of the block calls it.
__device__ __forceinline__ void ml_block_sum(MlShared& sh, double s, double* out) {
  s = group_sum_f64<64>(s);  // valid in lane 63
  if ((threadIdx.x & 63) == 63) sh.red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < kMlNT / 64; ++i) t += sh.red[i];
    *out = t;
  }
}

}  // namespace

// row[i] = Q(param(i)), i < n = n_b * reps + n_w, in getModelParams' order (network.h:708-723,
// as k_encode_model_params reads it): param(i) = biases[i % n_b] for i < n_b * reps, else
// weights[i - n_b * reps]; row[n .. 4 quads) = 0. partials[blockIdx.x] = the block's part of
// sum (double)(row[i] * row[i]), getNorm of the version's own text (Kardam.java:116).
__global__ void __launch_bounds__(kMlNT) k_mrow_stage(const float* __restrict__ weights,
                                                      const float* __restrict__ biases, uint32_t n_b, uint32_t nbr,
                                                      uint32_t n, float* __restrict__ row, uint32_t quads,
                                                      double* __restrict__ partials) {
  __shared__ MlShared sh;
  ml_block_open(sh);
  double s = 0.0;
  for (uint32_t base = blockIdx.x * kMlNT; base < quads; base += gridDim.x * kMlNT) {  // block-uniform trip count
    const uint32_t g = base + threadIdx.x;
    const bool live = g < quads;
    float x[4], a[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t v = 4 * g + e;
      x[e] = 0.0f;
      if (live && v < n) x[e] = v < nbr ? biases[v % n_b] : weights[v - nbr];
    }
    q_stage_d16x<4>(a, x, &sh.dtab, sh.tab.var);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!live || 4 * g + e >= n) a[e] = 0.0f;
      s += (double)(a[e] * a[e]);
    }
    if (live) *reinterpret_cast<f4*>(row + 4 * (size_t)g) = f4{a[0], a[1], a[2], a[3]};
  }
  ml_block_sum(sh, s, partials + blockIdx.x);
}

// The pairs of one launch by value, so the rows' addresses stay scalar.
struct MlPairs {
  int32_t cur[kAccBurst];
  int32_t prev[kAccBurst];
};

// Pair p = blockIdx.y: D = Q(cur[i] - prev[i]) over the two rows, partials[p * gridDim.x +
// blockIdx.x] = the block's part of sum (double)(D * D). The rows' padding is 0 in both, and
// Q(0 - 0) = 0.
__global__ void __launch_bounds__(kMlNT) k_mrow_pair_norms(const float* __restrict__ slab, size_t vpitch, MlPairs pairs,
                                                           uint32_t quads, double* __restrict__ partials) {
  __shared__ MlShared sh;
  ml_block_open(sh);
  const int p = blockIdx.y;
  const float* cur = slab + (size_t)pairs.cur[p] * vpitch;
  const float* prev = slab + (size_t)pairs.prev[p] * vpitch;
  double s = 0.0;
  for (uint32_t base = blockIdx.x * kMlNT; base < quads; base += gridDim.x * kMlNT) {
    const uint32_t g = base + threadIdx.x;
    f4 a = f4{0.f, 0.f, 0.f, 0.f}, b = a;
    if (g < quads) {
      a = *reinterpret_cast<const f4*>(cur + 4 * (size_t)g);
      b = *reinterpret_cast<const f4*>(prev + 4 * (size_t)g);
    }
    const float dv[4] = {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
    float D[4];
    q_stage_d16x<4>(D, dv, &sh.dtab, sh.tab.var);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)(D[e] * D[e]);
  }
  ml_block_sum(sh, s, partials + (size_t)p * gridDim.x + blockIdx.x);
}

// sums[blockIdx.x] = partials[blockIdx.x * tiles + 0 .. tiles), tiles <= 64: a lane each,
// folded by DPP lane moves in a fixed order.
__global__ void __launch_bounds__(64) k_mrow_reduce(const double* __restrict__ partials, int tiles,
                                                    double* __restrict__ sums) {
  const int lane = threadIdx.x;
  double v = lane < tiles ? partials[(size_t)blockIdx.x * tiles + lane] : 0.0;
  v = group_sum_f64<64>(v);
  if (lane == 63) sums[blockIdx.x] = v;
}

int mrow_block_values() { return 4 * kMlNT; }

int mrow_tiles(int64_t n) {
  const int64_t quads = (n + 3) / 4;
  return (int)std::max<int64_t>(1, std::min<int64_t>((quads + kMlNT - 1) / kMlNT, kMlMaxTiles));
}

hipError_t launch_mrow_stage(const float* weights, int64_t n_w, const float* biases, int64_t n_b, int64_t reps,
                             float* row, double* partials, double* norm_sq, hipStream_t s) {
  const int64_t nbr = n_b * reps, n = nbr + n_w;
  if (n <= 0 || n >= kMlMaxValues || !row || !partials || !norm_sq || (n_w && !weights) || (nbr && !biases))
    return hipErrorInvalidValue;
  const int tiles = mrow_tiles(n);
  k_mrow_stage<<<dim3((unsigned)tiles), dim3(kMlNT), 0, s>>>(weights, biases, (uint32_t)n_b, (uint32_t)nbr, (uint32_t)n,
                                                              row, (uint32_t)((n + 3) / 4), partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_mrow_reduce<<<dim3(1), dim3(64), 0, s>>>(partials, tiles, norm_sq);
  return hipGetLastError();
}

hipError_t launch_mrow_pair_norms(const float* slab, size_t vpitch, int rows, int64_t n, const int32_t* cur,
                                  const int32_t* prev, int P, double* partials, double* sums, hipStream_t s) {
  if (P <= 0 || P > kAccBurst || n <= 0 || n >= kMlMaxValues || !slab || !partials || !sums) return hipErrorInvalidValue;
  const int64_t quads = (n + 3) / 4;
  if (vpitch < (size_t)(4 * quads)) return hipErrorInvalidValue;
  MlPairs pr;
  for (int i = 0; i < kAccBurst; ++i) {
    pr.cur[i] = i < P ? cur[i] : 0, pr.prev[i] = i < P ? prev[i] : 0;
    // a row outside the slab never reaches the kernel
    if (pr.cur[i] < 0 || pr.cur[i] >= rows || pr.prev[i] < 0 || pr.prev[i] >= rows) return hipErrorInvalidValue;
  }
  const int tiles = mrow_tiles(n);
  k_mrow_pair_norms<<<dim3((unsigned)tiles, (unsigned)P), dim3(kMlNT), 0, s>>>(slab, vpitch, pr, (uint32_t)quads, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_mrow_reduce<<<dim3((unsigned)P), dim3(64), 0, s>>>(partials, tiles, sums);
  return hipGetLastError();
}

}  // namespace fleet

// fleet_amd/csrc/model_codec.hip -- the DISTILLATION_MODE=1 model codec on gfx950
// (SURVEY.md §8 rows a15-a19): per-matrix min-max quantisation, the
// first-occurrence dictionary and the selected-index set that getParams
// prints, and the read-back of that text.
//
// Reference semantics (all restated bit-exactly):
//   quantization_weight_model  commonLib/cppNN/network.h:1683-1774 (non-bucketing path)
//   matrix::min_max             commonLib/cppNN/core_math.h:881-899
//   matrix::round_matrix        core_math.h:901-912 (s = rows*cols: the shadowed parameter)
//   operator+(float), *(float)  core_math.h:1045-1056
//   float_vector_find           network.h:594-608 (first entry with fabsf(x - e) < 1e-8f)
//   getParams mode-1 section    network.h:641-692
//   network::read mode-1 branch network.h:958-997
//
// Layout: the W matrices of a model concatenated in W order (n floats), each
// cols*rows*chans (chan_aligned = 0, no padding), matrix j at offset off[j].
//
// The dictionary is built without the reference's O(n*U) scans: values are
// radix-sorted (stable, so equal values keep index order); a "cluster" is a
// maximal run of sorted neighbours closer than the tolerance. Two values in
// different clusters never match (their float difference is at least the
// gap at the cluster boundary: rounding is monotone), so every cluster is
// resolved alone: a cluster of equal values is one entry created by its
// first occurrence; a cluster of distinct near-equal values (a tolerance
// chain, where non-transitivity matters) replays the reference's sequential
// rule over its members in index order. Entry creators ranked by index give
// the dictionary order; NaN/inf match nothing (fabsf(NaN) < tol is false),
// each creates an entry and prints index -1 (the reference's pass 2).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "model_codec.h"
#include "dev_mem.h"
#include "decimal6.h"

namespace fleet {

// Device-wide sums and the key sort on rocPRIM, AMD's own primitives library (its
// wave-level scans and LDS radix passes are tuned for CDNA; no CUB-compatible layer).
// Each call with tmp == nullptr only sizes the temporary storage, as in rocPRIM.
template <class T>
static hipError_t inclusive_sum(void* tmp, size_t& bytes, const T* in, T* out, size_t n, hipStream_t s) {
  return rocprim::inclusive_scan(tmp, bytes, in, out, n, rocprim::plus<T>(), s);
}
template <class T>
static hipError_t exclusive_sum(void* tmp, size_t& bytes, const T* in, T* out, size_t n, hipStream_t s) {
  return rocprim::exclusive_scan(tmp, bytes, in, out, T(0), n, rocprim::plus<T>(), s);
}
static hipError_t sort_pairs(void* tmp, size_t& bytes, const uint32_t* keys, uint32_t* keys_out, const int32_t* vals,
                             int32_t* vals_out, size_t n, hipStream_t s) {
  return rocprim::radix_sort_pairs(tmp, bytes, keys, keys_out, vals, vals_out, n, 0u, 32u, s);
}
namespace {

constexpr float kTol = 0.00000001f;

struct MatParams {
  float alpha, beta, nbeta, ialpha, fs, one_over_s;
};

__device__ __forceinline__ bool finite_f(float x) { return __builtin_isfinite(x); }

// matrix::min_max: mini/maxi start at 0 and move on a strict < / > -- the
// first index of the extreme value, NaN never selected unless x[0] is NaN.
__global__ void __launch_bounds__(256) k_mm_minmax(const float* __restrict__ w, const int64_t* __restrict__ off,
                                                   const int32_t* __restrict__ dims, MatParams* __restrict__ prm) {
  const int j = blockIdx.x;
  const int64_t o = off[j], n = off[j + 1] - off[j];
  const int s = dims[3 * j] * dims[3 * j + 1];
  __shared__ float smin[256], smax[256];
  __shared__ int64_t simin[256], simax[256];
  float bmin = 0.f, bmax = 0.f;
  int64_t imin = -1, imax = -1;  // -1: nothing seen yet
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const float x = w[o + i];
    if (x != x) continue;
    if (imin < 0 || x < bmin) bmin = x, imin = i;
    if (imax < 0 || x > bmax) bmax = x, imax = i;
  }
  smin[threadIdx.x] = bmin;
  smax[threadIdx.x] = bmax;
  simin[threadIdx.x] = imin;
  simax[threadIdx.x] = imax;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      const int t = threadIdx.x, u = t + st;
      if (simin[u] >= 0 &&
          (simin[t] < 0 || smin[u] < smin[t] || (smin[u] == smin[t] && simin[u] < simin[t])))
        smin[t] = smin[u], simin[t] = simin[u];
      if (simax[u] >= 0 &&
          (simax[t] < 0 || smax[u] > smax[t] || (smax[u] == smax[t] && simax[u] < simax[t])))
        smax[t] = smax[u], simax[t] = simax[u];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float mn, mx;
    if (n == 0) {
      mn = mx = 0.f;
    } else if (w[o] != w[o]) {  // x[0] NaN: no comparison ever moves mini/maxi off 0
      mn = mx = w[o];
    } else {
      mn = smin[0];
      mx = smax[0];
    }
    MatParams p;
    p.alpha = mx - mn;
    p.beta = mn;
    p.nbeta = (float)(-1.0 * (double)mn);
    p.ialpha = (float)(1.0 / (double)p.alpha);
    p.fs = (float)s;
    p.one_over_s = (float)(1 / s);
    prm[j] = p;
  }
}

__device__ __forceinline__ int mat_of(const int64_t* __restrict__ off, int n_mats, int64_t i) {
  int lo = 0, hi = n_mats;  // off[lo] <= i < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// x + (-beta); * (1/alpha); round_matrix(s); * alpha; + beta -- one rounding per step.
__global__ void __launch_bounds__(256) k_mm_quantize(const float* __restrict__ w, int64_t n,
                                                     const int64_t* __restrict__ off, int n_mats,
                                                     const MatParams* __restrict__ prm, float* __restrict__ wq) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const MatParams p = prm[mat_of(off, n_mats, i)];
  float x = w[i] + p.nbeta;
  x = x * p.ialpha;
  if (x - floorf(x) > 0.5f)
    x = floorf(x * p.fs) / p.fs + p.one_over_s;
  else
    x = floorf(x * p.fs) / p.fs;
  x = x * p.alpha;
  wq[i] = x + p.beta;
}

// order-preserving key; NaN/inf last (they never match, their order is by index)
__global__ void __launch_bounds__(256) k_dict_keys(const float* __restrict__ w, int64_t n, uint32_t* __restrict__ key,
                                                   int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = w[i];
  uint32_t u = __float_as_uint(x);
  if (!finite_f(x))
    u = 0xFFFFFFFFu;
  else if (u == 0x80000000u)
    u = 0x80000000u;  // -0 sorts with +0 (fabsf(-0 - 0) = 0 < tol)
  else
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  key[i] = u;
  idx[i] = (int32_t)i;
}

// start[k] = 1 where a new cluster begins in sorted order
__global__ void __launch_bounds__(256) k_dict_starts(const float* __restrict__ w, const int32_t* __restrict__ sidx,
                                                     int64_t n, int32_t* __restrict__ start) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  int32_t st = 1;
  if (k > 0) {
    const float a = w[sidx[k - 1]], b = w[sidx[k]];
    if (finite_f(a) && finite_f(b) && fabsf(b - a) < kTol) st = 0;
  }
  start[k] = st;
}

// cluster c spans sorted positions [cbeg[c], cbeg[c+1])
__global__ void __launch_bounds__(256) k_dict_cbeg(const int32_t* __restrict__ start,
                                                   const int32_t* __restrict__ cid_incl, int64_t n,
                                                   int32_t* __restrict__ cbeg) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  if (start[k]) cbeg[cid_incl[k] - 1] = (int32_t)k;
}

// One thread per cluster: creator (original index of the element that created
// the member's dictionary entry) for every member; is_creator flags.
__global__ void __launch_bounds__(256) k_dict_resolve(const float* __restrict__ w, const int32_t* __restrict__ sidx,
                                                      const int32_t* __restrict__ cbeg, int32_t n_clusters,
                                                      int32_t* __restrict__ creator_of_sorted,
                                                      uint8_t* __restrict__ is_creator,
                                                      int32_t* __restrict__ scratch /* n: entry list */) {
  const int32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_clusters) return;
  const int32_t a = cbeg[c], b = cbeg[c + 1];
  const float va = w[sidx[a]], vb = w[sidx[b - 1]];
  if (!finite_f(va)) {  // NaN / inf: singleton, creates an entry, prints -1
    creator_of_sorted[a] = sidx[a];
    is_creator[sidx[a]] = 1;
    return;
  }
  if (va == vb) {  // all equal (sorted): one entry, created by the first occurrence
    const int32_t cr = sidx[a];  // stable sort: smallest index first
    is_creator[cr] = 1;
    for (int32_t k = a; k < b; ++k) creator_of_sorted[k] = cr;
    return;
  }
  // tolerance chain: the reference's sequential rule over members in index
  // order. Entries (sorted positions) kept in scratch[a..). Members are
  // visited by increasing original index (selection over the run).
  int32_t n_ent = 0;
  int32_t last = -1;
  for (int32_t done = 0; done < b - a; ++done) {
    int32_t kk = -1, best = 0x7FFFFFFF;
    for (int32_t k = a; k < b; ++k) {
      const int32_t id = sidx[k];
      if (id > last && id < best) best = id, kk = k;
    }
    last = best;
    const float x = w[best];
    int32_t cr = -1;
    for (int32_t e = 0; e < n_ent; ++e) {
      const int32_t ek = scratch[a + e];
      if (fabsf(x - w[sidx[ek]]) < kTol) {
        cr = sidx[ek];
        break;
      }
    }
    if (cr < 0) {
      scratch[a + n_ent++] = kk;
      cr = best;
      is_creator[best] = 1;
    }
    creator_of_sorted[kk] = cr;
  }
}

__global__ void __launch_bounds__(256) k_dict_u8_to_i32(const uint8_t* __restrict__ f, int64_t n,
                                                        int32_t* __restrict__ o) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) o[i] = f[i];
}

// dictionary value at each creator's rank; index of every element
__global__ void __launch_bounds__(256) k_dict_emit(const float* __restrict__ w, const int32_t* __restrict__ sidx,
                                                   const int32_t* __restrict__ creator_of_sorted,
                                                   const uint8_t* __restrict__ is_creator,
                                                   const int32_t* __restrict__ rank, int64_t n,
                                                   float* __restrict__ dict, int32_t* __restrict__ index) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int32_t i = sidx[k];
  if (is_creator[i]) dict[rank[i]] = w[i];
  if (index) index[i] = finite_f(w[i]) ? rank[creator_of_sorted[k]] : -1;
}

// ------------------------------------------------------------ text (a17)

__device__ __forceinline__ int dec_len(int32_t v) {
  uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  int d = 1;
  while (a >= 10u) a /= 10u, ++d;
  return d + (v < 0);
}

// bytes of element i in the index section: digits + ' ' (+ '\n' after a matrix's last)
__global__ void __launch_bounds__(256) k_text_len(const int32_t* __restrict__ index, int64_t n,
                                                  const int64_t* __restrict__ off, int n_mats,
                                                  int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = mat_of(off, n_mats, i);
  len[i] = dec_len(index[i]) + 1 + (i + 1 == off[j + 1] ? 1 : 0);
}

__global__ void __launch_bounds__(256) k_text_write(const int32_t* __restrict__ index, int64_t n,
                                                    const int64_t* __restrict__ off, int n_mats,
                                                    const int64_t* __restrict__ pos, char* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = mat_of(off, n_mats, i);
  int32_t v = index[i];
  char* p = out + pos[i];
  const int l = dec_len(v);
  uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  if (v < 0) p[0] = '-';
  for (int q = l - 1; q >= (v < 0); --q) {
    p[q] = (char)('0' + a % 10u);
    a /= 10u;
  }
  p[l] = ' ';
  if (i + 1 == off[j + 1]) p[l + 1] = '\n';
}

// ------------------------------------------------------------ value text
// `ostream << float` (decimal6.h g6_text) for a run of n values, in the shape of
// k_text_len / k_text_write. The exact digits cost a few hundred integer
// operations, so they are derived once: k_vtext_len leaves each value's bytes
// in a 16-byte cell (bytes 0..11 text, byte 12 its length) and k_vtext_write
// only copies them to the scanned position.
//   lines (n_blocks > 0): "value " per value, '\n' after a block's last value;
//     a block of size 0 still prints its lone '\n' -- those of the blocks before
//     the first value ride with value 0, the others with the value before them.
//   pairs (n_blocks == 0): "i\nvalue\n", the mode-1 dictionary section.
struct VCell {
  char t[12];
  uint8_t len, lead, trail, pad;  // '\n's before (value 0 only) and after this value's "text "
};
static_assert(sizeof(VCell) == 16, "one 16-byte cell per value");

__global__ void __launch_bounds__(256) k_vtext_len(const float* __restrict__ v, int64_t n,
                                                   const int64_t* __restrict__ off, int n_blocks,
                                                   VCell* __restrict__ cell, int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  VCell c;
#pragma unroll
  for (int k = 0; k < 12; ++k) c.t[k] = 0;
  c.len = (uint8_t)g6_text(v[i], c.t);
  c.lead = c.trail = c.pad = 0;
  int64_t l = c.len + 1;
  if (n_blocks > 0) {
    const int j = mat_of(off, n_blocks, i);  // off[j] <= i < off[j + 1]: never an empty block
    int lead = 0, trail = 0;
    if (i == 0) lead = j;  // every block before value 0's is empty
    if (i + 1 == off[j + 1])
      for (int k = j + 1; k <= n_blocks && off[k] == i + 1; ++k) ++trail;
    // more than 254 empty blocks in a row do not fit the cell's counters: the host refuses them
    c.lead = (uint8_t)lead;
    c.trail = (uint8_t)trail;
    l += lead + trail;
  } else {
    l += dec_len((int32_t)i) + 1;
  }
  cell[i] = c;
  len[i] = l;
}

__global__ void __launch_bounds__(256) k_vtext_write(const VCell* __restrict__ cell, int64_t n, int n_blocks,
                                                     const int64_t* __restrict__ pos, char* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const VCell c = cell[i];
  char* p = out + pos[i];
  if (n_blocks > 0) {
    for (int k = 0; k < c.lead; ++k) *p++ = '\n';
  } else {
    const int l = dec_len((int32_t)i);
    uint32_t a = (uint32_t)i;
    for (int q = l - 1; q >= 0; --q) {
      p[q] = (char)('0' + a % 10u);
      a /= 10u;
    }
    p += l;
    *p++ = '\n';
  }
  for (int k = 0; k < c.len; ++k) *p++ = c.t[k];
  if (n_blocks > 0) {
    *p++ = ' ';
    for (int k = 0; k < c.trail; ++k) *p++ = '\n';
  } else {
    *p++ = '\n';
  }
}

// ------------------------------------------------------------ read (a19)

__device__ __forceinline__ bool is_ws(uint8_t c) { return c == ' ' || c == '\n' || c == '\t' || c == '\r'; }
__device__ __forceinline__ bool tok_char(uint8_t c) { return c == '-' || c == '+' || (c >= '0' && c <= '9'); }

__global__ void __launch_bounds__(256) k_read_starts(const uint8_t* __restrict__ t, int64_t len,
                                                     int32_t* __restrict__ st) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= len) return;
  st[p] = tok_char(t[p]) && (p == 0 || is_ws(t[p - 1])) ? 1 : 0;
}

// token number t (from the inclusive scan) -> weight t = value of its key
__global__ void __launch_bounds__(256) k_read_tokens(const uint8_t* __restrict__ t, int64_t len,
                                                     const int32_t* __restrict__ st,
                                                     const int32_t* __restrict__ tok_incl, int64_t n_w,
                                                     const int32_t* __restrict__ keys,
                                                     const float* __restrict__ vals, int32_t n_keys,
                                                     float* __restrict__ w, int* __restrict__ bad) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= len || !st[p]) return;
  const int64_t tk = tok_incl[p] - 1;
  // `ifs >> int`: optional sign, digits; the reference's own texts only
  int64_t q = p;
  bool neg = false;
  if (t[q] == '-' || t[q] == '+') neg = t[q++] == '-';
  int64_t v = 0;
  int nd = 0;
  while (q < len && t[q] >= '0' && t[q] <= '9' && nd < 12) v = v * 10 + (t[q++] - '0'), ++nd;
  if (nd == 0 || nd >= 12 || (q < len && !is_ws(t[q]))) {
    atomicOr(bad, 1);
    return;
  }
  if (neg) v = -v;
  if (tk >= n_w) {
    atomicOr(bad, 2);
    return;
  }
  // std::map<int,float> operator[]: the value of the key, 0.0f when absent
  int32_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  w[tk] = (lo < n_keys && keys[lo] == v) ? vals[lo] : 0.0f;
}

inline unsigned nb(int64_t n) { return (unsigned)((n + 255) / 256); }

// n elements, at least one
template <typename T>
hipError_t alloc1(DevBuf<T>& b, size_t n) { return b.alloc(n ? n : 1); }

// *p: a caller-owned workspace's buffer when there is one, else an allocation of n (at least
// one) that `owned` keeps until the function returns
template <typename T>
hipError_t ws_or_alloc(T* from_ws, size_t n, std::vector<DevBuf<void>>& owned, T** p) {
  *p = from_ws;
  if (from_ws) return hipSuccess;
  owned.emplace_back();
  const hipError_t e = owned.back().alloc(sizeof(T) * (n ? n : 1));
  *p = (T*)owned.back().get();
  return e;
}

#define MC_TRY(x)                      \
  do {                                 \
    hipError_t e_ = (x);               \
    if (e_ != hipSuccess) return e_;   \
  } while (0)

}  // namespace

hipError_t model_quantize_index(const float* d_w, const int32_t* h_dims, int n_mats, float* d_wq, float* d_dict,
                                int32_t* d_index, int32_t* h_U, hipStream_t s, bool quantize, const DictWs* ws) {
  std::vector<int64_t> off(n_mats + 1, 0);
  for (int j = 0; j < n_mats; ++j) off[j + 1] = off[j] + (int64_t)h_dims[3 * j] * h_dims[3 * j + 1] * h_dims[3 * j + 2];
  const int64_t n = off[n_mats];
  *h_U = 0;
  if (n == 0) return hipSuccess;
  std::vector<DevBuf<void>> owned;  // what the workspace does not bring
  int64_t* d_off;
  int32_t* d_dims;
  MatParams* d_prm;
  MC_TRY(ws_or_alloc(ws ? ws->off : nullptr, n_mats + 1, owned, &d_off));
  MC_TRY(ws_or_alloc(ws ? ws->dims : nullptr, 3 * n_mats, owned, &d_dims));
  MC_TRY(ws_or_alloc(ws ? (MatParams*)ws->prm : nullptr, n_mats, owned, &d_prm));
  MC_TRY(hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * (n_mats + 1), hipMemcpyHostToDevice, s));
  MC_TRY(hipMemcpyAsync(d_dims, h_dims, sizeof(int32_t) * 3 * n_mats, hipMemcpyHostToDevice, s));
  if (quantize) {
    hipLaunchKernelGGL(k_mm_minmax, dim3(n_mats), dim3(256), 0, s, d_w, d_off, d_dims, d_prm);
    hipLaunchKernelGGL(k_mm_quantize, dim3(nb(n)), dim3(256), 0, s, d_w, n, d_off, n_mats, d_prm, d_wq);
    MC_TRY(hipGetLastError());
  } else {  // the dictionary of the weights as they are (descentNative's model copy)
    d_wq = const_cast<float*>(d_w);
  }

  // dictionary over the quantised weights
  uint32_t *key, *key2;
  int32_t *idx, *sidx, *start, *cid, *cbeg, *creator, *scratch, *rank, *flag32;
  uint8_t* is_creator;
  MC_TRY(ws_or_alloc(ws ? ws->key : nullptr, n, owned, &key));
  MC_TRY(ws_or_alloc(ws ? ws->key2 : nullptr, n, owned, &key2));
  MC_TRY(ws_or_alloc(ws ? ws->idx : nullptr, n, owned, &idx));
  MC_TRY(ws_or_alloc(ws ? ws->sidx : nullptr, n, owned, &sidx));
  MC_TRY(ws_or_alloc(ws ? ws->start : nullptr, n, owned, &start));
  MC_TRY(ws_or_alloc(ws ? ws->cid : nullptr, n, owned, &cid));
  MC_TRY(ws_or_alloc(ws ? ws->cbeg : nullptr, n + 1, owned, &cbeg));
  MC_TRY(ws_or_alloc(ws ? ws->creator : nullptr, n, owned, &creator));
  MC_TRY(ws_or_alloc(ws ? ws->scratch : nullptr, n, owned, &scratch));
  MC_TRY(ws_or_alloc(ws ? ws->rank : nullptr, n, owned, &rank));
  MC_TRY(ws_or_alloc(ws ? ws->flag32 : nullptr, n, owned, &flag32));
  MC_TRY(ws_or_alloc(ws ? ws->is_creator : nullptr, n, owned, &is_creator));
  hipLaunchKernelGGL(k_dict_keys, dim3(nb(n)), dim3(256), 0, s, d_wq, n, key, idx);
  size_t tmp_bytes = 0, t2 = 0, t3 = 0;
  MC_TRY(sort_pairs(nullptr, tmp_bytes, key, key2, idx, sidx, n, s));
  MC_TRY(inclusive_sum(nullptr, t2, start, cid, n, s));
  MC_TRY(exclusive_sum(nullptr, t3, flag32, rank, n, s));
  tmp_bytes = std::max(tmp_bytes, std::max(t2, t3));
  uint8_t* tmp;
  if (ws && ws->tmp_bytes < tmp_bytes) return hipErrorInvalidValue;  // (sized by model_dict_ws_carve for this n)
  MC_TRY(ws_or_alloc(ws ? (uint8_t*)ws->tmp : nullptr, tmp_bytes, owned, &tmp));
  MC_TRY(sort_pairs(tmp, tmp_bytes, key, key2, idx, sidx, n, s));
  hipLaunchKernelGGL(k_dict_starts, dim3(nb(n)), dim3(256), 0, s, d_wq, sidx, n, start);
  size_t tb = tmp_bytes;
  MC_TRY(inclusive_sum(tmp, tb, start, cid, n, s));
  int32_t n_clusters = 0;
  MC_TRY(hipMemcpyAsync(&n_clusters, cid + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MC_TRY(hipStreamSynchronize(s));
  hipLaunchKernelGGL(k_dict_cbeg, dim3(nb(n)), dim3(256), 0, s, start, cid, n, cbeg);
  const int32_t nn = (int32_t)n;
  MC_TRY(hipMemcpyAsync(cbeg + n_clusters, &nn, sizeof(int32_t), hipMemcpyHostToDevice, s));
  MC_TRY(hipMemsetAsync(is_creator, 0, n, s));
  hipLaunchKernelGGL(k_dict_resolve, dim3(nb(n_clusters)), dim3(256), 0, s, d_wq, sidx, cbeg, n_clusters,
                     creator, is_creator, scratch);
  hipLaunchKernelGGL(k_dict_u8_to_i32, dim3(nb(n)), dim3(256), 0, s, is_creator, n, flag32);
  tb = tmp_bytes;
  MC_TRY(exclusive_sum(tmp, tb, flag32, rank, n, s));
  int32_t last_rank = 0, last_flag = 0;
  MC_TRY(hipMemcpyAsync(&last_rank, rank + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MC_TRY(hipMemcpyAsync(&last_flag, flag32 + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  hipLaunchKernelGGL(k_dict_emit, dim3(nb(n)), dim3(256), 0, s, d_wq, sidx, creator, is_creator, rank, n,
                     d_dict, d_index);
  MC_TRY(hipGetLastError());
  MC_TRY(hipStreamSynchronize(s));
  *h_U = last_rank + last_flag;
  return hipSuccess;
}

// w[i] = vals[index[i]] (index -1, a non-finite weight: 0.0f, std::map::operator[])
__global__ void __launch_bounds__(256) k_dict_gather(const int32_t* __restrict__ index, int64_t n,
                                                     const float* __restrict__ vals, float* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t k = index[i];
  w[i] = k >= 0 ? vals[k] : 0.0f;
}

__global__ void __launch_bounds__(256) k_g6_inplace(float* __restrict__ v, int64_t n, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = v[i];
  if ((f2u(x) & 0x7f800000u) == 0x7f800000u) {  // inf / NaN: the reference's text read fails
    atomicOr(bad, 1);
    return;
  }
  v[i] = g6_roundtrip(x);
}

hipError_t model_g6_inplace(float* d_v, int64_t n, int* d_bad, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_g6_inplace, dim3(nb(n)), dim3(256), 0, s, d_v, n, d_bad);
  return hipGetLastError();
}

hipError_t model_dict_gather(const int32_t* d_index, int64_t n, const float* d_vals, float* d_w, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dict_gather, dim3(nb(n)), dim3(256), 0, s, d_index, n, d_vals, d_w);
  return hipGetLastError();
}

hipError_t model_index_text(const int32_t* d_index, const int32_t* h_dims, int n_mats, std::vector<char>* out,
                            hipStream_t s) {
  std::vector<int64_t> off(n_mats + 1, 0);
  for (int j = 0; j < n_mats; ++j) off[j + 1] = off[j] + (int64_t)h_dims[3 * j] * h_dims[3 * j + 1] * h_dims[3 * j + 2];
  const int64_t n = off[n_mats];
  // matrices of size 0 still print their '\n' (the reference loops W[j] non-null)
  out->clear();
  if (n == 0) {
    out->assign((size_t)n_mats, '\n');
    return hipSuccess;
  }
  DevBuf<int64_t> d_off, len, pos;
  DevBuf<char> txt;
  MC_TRY(alloc1(d_off, n_mats + 1));
  MC_TRY(alloc1(len, n));
  MC_TRY(alloc1(pos, n));
  MC_TRY(hipMemcpyAsync(d_off.get(), off.data(), sizeof(int64_t) * (n_mats + 1), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_text_len, dim3(nb(n)), dim3(256), 0, s, d_index, n, d_off.get(), n_mats, len.get());
  size_t tb = 0;
  MC_TRY(exclusive_sum(nullptr, tb, len.get(), pos.get(), n, s));
  DevBuf<uint8_t> tmp;
  MC_TRY(alloc1(tmp, tb));
  MC_TRY(exclusive_sum(tmp.get(), tb, len.get(), pos.get(), n, s));
  int64_t last_pos = 0, last_len = 0;
  MC_TRY(hipMemcpyAsync(&last_pos, pos.get() + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, s));
  MC_TRY(hipMemcpyAsync(&last_len, len.get() + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, s));
  MC_TRY(hipStreamSynchronize(s));
  const int64_t total = last_pos + last_len;
  MC_TRY(alloc1(txt, total));
  hipLaunchKernelGGL(k_text_write, dim3(nb(n)), dim3(256), 0, s, d_index, n, d_off.get(), n_mats, pos.get(), txt.get());
  MC_TRY(hipGetLastError());
  // empty matrices print a lone '\n' in their place: stitch them in on the host
  std::vector<char> body((size_t)total);
  MC_TRY(hipMemcpyAsync(body.data(), txt.get(), (size_t)total, hipMemcpyDeviceToHost, s));
  MC_TRY(hipStreamSynchronize(s));
  bool any_empty = false;
  for (int j = 0; j < n_mats; ++j) any_empty |= off[j + 1] == off[j];
  if (!any_empty) {
    out->swap(body);
    return hipSuccess;
  }
  // positions of each matrix's text: recompute from the line breaks
  size_t p = 0;
  for (int j = 0; j < n_mats; ++j) {
    if (off[j + 1] == off[j]) {
      out->push_back('\n');
      continue;
    }
    const size_t q = (size_t)(std::find(body.begin() + p, body.end(), '\n') - body.begin()) + 1;
    out->insert(out->end(), body.begin() + p, body.begin() + q);
    p = q;
  }
  return hipSuccess;
}

hipError_t model_values_text(const float* d_v, int64_t n, const int64_t* h_off, int n_blocks, std::vector<char>* out,
                             hipStream_t s) {
  out->clear();
  if (n == 0) {  // nothing but the empty blocks' '\n's
    out->assign((size_t)std::max(0, n_blocks), '\n');
    return hipSuccess;
  }
  if (n_blocks > 0) {
    if (h_off[0] != 0 || h_off[n_blocks] != n) return hipErrorInvalidValue;
    int run = 0;
    for (int j = 0; j < n_blocks; ++j) {
      if (h_off[j + 1] < h_off[j]) return hipErrorInvalidValue;
      run = h_off[j + 1] == h_off[j] ? run + 1 : 0;
      // VCell's 8-bit counters: `trail` holds a block's own '\n' and those of the empty
      // blocks after it, `lead` those before value 0
      if (run > 254) return hipErrorInvalidValue;
    }
  } else if (n > 0x7fffffff) {
    return hipErrorInvalidValue;  // the pairs' keys are ints
  }
  DevBuf<int64_t> d_off;
  DevBuf<uint8_t> wsmem;
  MC_TRY(alloc1(d_off, (size_t)n_blocks + 1));
  TextWs ws;
  const size_t ws_bytes = model_text_ws_carve(nullptr, n, &ws);
  if (!ws_bytes) return hipErrorUnknown;
  MC_TRY(alloc1(wsmem, ws_bytes));
  model_text_ws_carve(wsmem.get(), n, &ws);
  if (n_blocks > 0)
    MC_TRY(hipMemcpyAsync(d_off.get(), h_off, sizeof(int64_t) * ((size_t)n_blocks + 1), hipMemcpyHostToDevice, s));
  // 12 bytes and a separator per value, an int key and its newline (pairs) or the blocks' newlines
  const int64_t cap = n_blocks > 0 ? 13 * n + n_blocks : 24 * n;
  DevBuf<char> txt;
  MC_TRY(alloc1(txt, (size_t)cap));
  int64_t total = 0;
  MC_TRY(model_values_text_ws(d_v, n, d_off.get(), n_blocks, ws, txt.get(), cap, &total, s));
  out->resize((size_t)total);
  MC_TRY(hipMemcpyAsync(out->data(), txt.get(), (size_t)total, hipMemcpyDeviceToHost, s));
  return hipStreamSynchronize(s);
}

size_t model_text_ws_carve(void* base, int64_t n, TextWs* ws) {
  Carver c{(uint8_t*)base};
  ws->len = c.take<int64_t>((size_t)n);
  ws->pos = c.take<int64_t>((size_t)n);
  ws->cell = c.take<VCell>((size_t)n);
  size_t tb = 0;
  if (n > 0 && exclusive_sum<int64_t>(nullptr, tb, nullptr, nullptr, (size_t)n, nullptr) != hipSuccess) return 0;
  ws->tmp_bytes = tb;
  ws->tmp = c.take<uint8_t>(tb);
  return c.at;
}

size_t model_dict_ws_carve(void* base, int64_t n, int n_mats, DictWs* ws) {
  Carver c{(uint8_t*)base};
  const size_t m = (size_t)n;
  ws->off = c.take<int64_t>((size_t)n_mats + 1);
  ws->dims = c.take<int32_t>(3 * (size_t)n_mats);
  ws->prm = c.take<MatParams>((size_t)n_mats);
  ws->key = c.take<uint32_t>(m);
  ws->key2 = c.take<uint32_t>(m);
  ws->idx = c.take<int32_t>(m);
  ws->sidx = c.take<int32_t>(m);
  ws->start = c.take<int32_t>(m);
  ws->cid = c.take<int32_t>(m);
  ws->cbeg = c.take<int32_t>(m + 1);
  ws->creator = c.take<int32_t>(m);
  ws->scratch = c.take<int32_t>(m);
  ws->rank = c.take<int32_t>(m);
  ws->flag32 = c.take<int32_t>(m);
  ws->is_creator = c.take<uint8_t>(m);
  size_t t1 = 0, t2 = 0, t3 = 0;
  if (n > 0 && (sort_pairs(nullptr, t1, nullptr, nullptr, nullptr, nullptr, m, nullptr) != hipSuccess ||
                inclusive_sum<int32_t>(nullptr, t2, nullptr, nullptr, m, nullptr) != hipSuccess ||
                exclusive_sum<int32_t>(nullptr, t3, nullptr, nullptr, m, nullptr) != hipSuccess))
    return 0;
  ws->tmp_bytes = std::max(t1, std::max(t2, t3));
  ws->tmp = c.take<uint8_t>(ws->tmp_bytes);
  return c.at;
}

// scan the lengths, read the total back, refuse a text the buffer cannot hold
static hipError_t text_positions(int64_t n, const TextWs& ws, int64_t cap, int64_t* h_total, hipStream_t s) {
  size_t tb = ws.tmp_bytes;
  MC_TRY(exclusive_sum(ws.tmp, tb, ws.len, ws.pos, (size_t)n, s));
  int64_t last_pos = 0, last_len = 0;
  MC_TRY(hipMemcpyAsync(&last_pos, ws.pos + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, s));
  MC_TRY(hipMemcpyAsync(&last_len, ws.len + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, s));
  MC_TRY(hipStreamSynchronize(s));
  *h_total = last_pos + last_len;
  return *h_total > cap ? hipErrorOutOfMemory : hipSuccess;
}

hipError_t model_values_text_ws(const float* d_v, int64_t n, const int64_t* d_off, int n_blocks, const TextWs& ws,
                                char* d_out, int64_t cap, int64_t* h_total, hipStream_t s) {
  *h_total = 0;
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vtext_len, dim3(nb(n)), dim3(256), 0, s, d_v, n, d_off, n_blocks, (VCell*)ws.cell, ws.len);
  MC_TRY(hipGetLastError());
  MC_TRY(text_positions(n, ws, cap, h_total, s));
  hipLaunchKernelGGL(k_vtext_write, dim3(nb(n)), dim3(256), 0, s, (const VCell*)ws.cell, n, n_blocks, ws.pos, d_out);
  return hipGetLastError();
}

hipError_t model_index_text_ws(const int32_t* d_index, int64_t n, const int64_t* d_off, int n_mats, const TextWs& ws,
                               char* d_out, int64_t cap, int64_t* h_total, hipStream_t s) {
  *h_total = 0;
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_text_len, dim3(nb(n)), dim3(256), 0, s, d_index, n, d_off, n_mats, ws.len);
  MC_TRY(hipGetLastError());
  MC_TRY(text_positions(n, ws, cap, h_total, s));
  hipLaunchKernelGGL(k_text_write, dim3(nb(n)), dim3(256), 0, s, d_index, n, d_off, n_mats, ws.pos, d_out);
  return hipGetLastError();
}

hipError_t model_read_index(const uint8_t* d_text, int64_t len, int64_t n_w, const int32_t* d_keys,
                            const float* d_vals, int32_t n_keys, float* d_w, int* h_status, hipStream_t s) {
  *h_status = 0;
  if (len == 0) {
    *h_status = n_w ? 2 : 0;
    return hipSuccess;
  }
  DevBuf<int32_t> st, tok;
  DevBuf<int> bad;
  MC_TRY(alloc1(st, len));
  MC_TRY(alloc1(tok, len));
  MC_TRY(alloc1(bad, 1));
  MC_TRY(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
  hipLaunchKernelGGL(k_read_starts, dim3(nb(len)), dim3(256), 0, s, d_text, len, st.get());
  size_t tb = 0;
  MC_TRY(inclusive_sum(nullptr, tb, st.get(), tok.get(), (size_t)len, s));
  DevBuf<uint8_t> tmp;
  MC_TRY(alloc1(tmp, tb));
  MC_TRY(inclusive_sum(tmp.get(), tb, st.get(), tok.get(), (size_t)len, s));
  hipLaunchKernelGGL(k_read_tokens, dim3(nb(len)), dim3(256), 0, s, d_text, len, st.get(), tok.get(), n_w, d_keys, d_vals,
                     n_keys, d_w, bad.get());
  MC_TRY(hipGetLastError());
  int32_t n_tok = 0;
  int hbad = 0;
  MC_TRY(hipMemcpyAsync(&n_tok, tok.get() + (len - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MC_TRY(hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  MC_TRY(hipStreamSynchronize(s));
  *h_status = hbad ? hbad : (n_tok != n_w ? 2 : 0);
  return hipSuccess;
}

}  // namespace fleet

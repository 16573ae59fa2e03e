// fleet_amd/csrc/acc_kernels.hip -- streaming aggregation: one upload folded into a
// resident sum per launch (k_acc_push), the merged gradient from the sum (k_acc_finish),
// a burst of uploads per launch (k_acc_push_many), the upload pool's fold over picked
// resident rows (k_pool_fold), and that fold with Kardam's side outputs of the picks
// (k_pool_fold_kd, k_pool_kd_reduce: the Kardam ledger), and the arrival gate's pass over
// resident rows that folds nothing (k_pool_vet, k_pool_vet_reduce).
//
// CppNNUpdater.update is entered once per upload and only buffers it until M have
// arrived (CppNNUpdater.java:383-391); the chain it then runs over the picked uploads
// (:420-421, :463-464, :490-508) is serial over clients and independent per element,
// so one client's step can run when its upload arrives:
//   y = Q(dec(code))   p = Q((float)((double)y * d))   A = first ? p : Q(A + p)
// The state A is one fp32 per upload position of the accumulator's group window, read
// from one buffer and written to the other, so a rejected upload leaves no trace.
//
// The batch kernels recompute a lane's whole chain from all M uploads when a value
// leaves the table stages' domain (chain_general); a fold step no longer has the
// earlier uploads, so here every stage falls back to the general codec within the step
// (q_stage_d16x: wave-uniform behind a ballot, never taken by gradient-like data).
//
// One copy of each piece: the block prologue (acc_block_open), the per-group prologue
// (acc_group_open), the per-upload step (acc_lane_step) and the finish epilogue
// (acc_lane_finish); the kernels are loops around them, k_acc_push the step at K = 1.
// One exception: k_pool_fold spells the per-group prologue out on locals of its own.
// Calling acc_group_open there changed the kernel's schedule and cost 1-2 % per launch
// (profiles/stream_shared/), so that piece of sharing stops at the other two kernels.
//
// This unit takes the stage helpers of kernels.hip and none of its kernels.
#define FLEET_STREAM_TU
#define FLEET_ACC_TU
#include "kernels.hip"

namespace fleet {

namespace {

constexpr int kAccNT = 256;
// header positions a block keeps in LDS for the per-group search (more: from global memory)
constexpr int kAccLdsHdr = 1024;

typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));

// first index i with hdr[i] >= p0 (hdr sorted)
__device__ __forceinline__ int acc_lower_bound(const int32_t* hdr, int n_hdr, int64_t p0) {
  int lo = 0, hi = n_hdr;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (hdr[mid] < p0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct AccShared {
  B64Tables tab;
  D16Table dtab;
  int32_t hdr[kAccLdsHdr];
};

// hdr_block = {0, count, walk_end, 0, positions} as a block reads it
struct AccHdr {
  int n_hdr;
  int64_t walk_end;
  const int32_t* hdr;
};

// Every kernel's block prologue: hdr_block unpacked, the tables and (when they fit) the
// header positions copied into LDS.
__device__ __forceinline__ AccHdr acc_block_open(AccShared& sh, const int32_t* __restrict__ hdr_block) {
  const AccHdr H{hdr_block[1], hdr_block[2], hdr_block + 4};
  b64_tables_init<kAccNT>(&sh.tab);
  d16_table_init<kAccNT>(&sh.dtab);
  if (H.n_hdr <= kAccLdsHdr)
    for (int i = threadIdx.x; i < H.n_hdr; i += kAccNT) sh.hdr[i] = H.hdr[i];
  __syncthreads();
  return H;
}

// bit e = slot p0 + e is a header slot; *first = the index of the group's first header
__device__ __forceinline__ uint32_t acc_bits_in(const int32_t* hdr, int n_hdr, int64_t p0, int* first) {
  const int lo = acc_lower_bound(hdr, n_hdr, p0);
  *first = lo;
  uint32_t bits = 0;
  for (int i = lo; i < n_hdr && hdr[i] < p0 + 3; ++i) bits |= 1u << (hdr[i] - p0);
  return bits;
}
__device__ __forceinline__ uint32_t acc_header_bits(const AccShared& sh, const int32_t* __restrict__ hdr, int n_hdr,
                                                    int64_t p0, int* first) {
  return n_hdr <= kAccLdsHdr ? acc_bits_in(sh.hdr, n_hdr, p0, first) : acc_bits_in(hdr, n_hdr, p0, first);
}

// A lane's group for the kernels that step: what does not change from one upload to the
// next, and the two values the steps carry (href, A).
struct AccGroup {
  bool live;              // inside the window; a dead lane loads nothing, runs the chain on code 0 and stores nothing
  int64_t gs, g;          // the group's index in the window (dead lanes: 0) and in the whole upload
  uint32_t need;          // the Base64 characters the group's values need
  uint32_t hbits, kbits;  // bit i: slot 3 g + i is a header slot / carries no chain (header, or at or past the walk's end)
  int h0;                 // index of the group's first header in hfirst[]
  bool wave_keep;         // some lane of the wave has kbits: few waves hold a header, so the header work hides behind this
  int32_t href[3];        // the batch's first upload's codes in the group's header slots
  float A[3];             // the running value
};

// The per-group prologue. `first`: the launch's first upload is the batch's first, so
// the state is not read and href comes from that upload (acc_lane_step); otherwise A is
// the lane's 12 bytes of `st` and href is loaded from hfirst[].
__device__ __forceinline__ AccGroup acc_group_open(const AccShared& sh, const AccHdr& H, int64_t gl, int64_t ng,
                                                   int64_t g_begin, int64_t n_up, bool first, const float* st,
                                                   const int32_t* hfirst) {
  AccGroup G;
  G.live = gl < ng;
  G.gs = G.live ? gl : 0;
  G.g = g_begin + G.gs;
  G.A[0] = G.A[1] = G.A[2] = 0.f;
  if (!first && G.live) {
    const f3u a = *reinterpret_cast<const f3u*>(st + 3 * G.gs);
    G.A[0] = a.x, G.A[1] = a.y, G.A[2] = a.z;
  }
  G.need = needed_chars_mask((int)min<int64_t>(3, max<int64_t>(0, n_up - 3 * G.g)));
  G.hbits = acc_header_bits(sh, H.hdr, H.n_hdr, 3 * G.g, &G.h0);
  G.kbits = keep_bits<3>(G.hbits, true, 3 * G.g, H.walk_end);
  G.wave_keep = __ballot(G.kbits != 0) != 0;
  G.href[0] = G.href[1] = G.href[2] = 0;
  if (G.wave_keep && !first) {
    int hi = G.h0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if ((G.hbits >> i) & 1u) G.href[i] = hfirst[hi++];
  }
  return G;
}

// One upload's step on a lane's group: A = is_first ? p : Q(A + p) with p the upload's
// dampened value (the file's header), every Q q_stage_d16x. `src` is the lane's 16 bytes
// of the upload's row. Slots with a kbit carry no chain: their code is taken as 0, so
// their state stays Q(0) = 0. `is_first` (uniform): the batch's first upload -- its header
// codes go to href and hfirst[]; a later upload's are compared with href, as the batch
// kernels compare with client 0. FINISH keeps the upload's own codes in keepc for the
// epilogue. bad / layout_bad collect the Base64 check's and the header comparison's
// failures of live lanes. The group's values come one by one (AccGroup's fields, or
// k_pool_fold's locals).
template <bool FINISH>
__device__ __forceinline__ void acc_lane_step(const AccShared& sh, const uint8_t* src, bool live, uint32_t need,
                                              bool wave_keep, uint32_t hbits, uint32_t kbits, int h0, bool is_first,
                                              double d, int32_t* hfirst, int32_t (&href)[3], int32_t (&keepc)[3],
                                              float (&A)[3], uint32_t& bad, uint32_t& layout_bad) {
  uint4 w = uint4{0u, 0u, 0u, 0u};
  if (live) w = *reinterpret_cast<const uint4*>(src);
  int32_t codes[3];
  if (need == 0xffffu) bad |= live ? b64_decode_group_full(w, &sh.tab, codes) : 0u;
  else bad |= live ? (b64_decode_group(w, &sh.tab, codes) & need) : 0u;
  if (!live) codes[0] = codes[1] = codes[2] = 0;
  if (wave_keep) {
    int hi = h0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if ((hbits >> i) & 1u) {
        if (is_first) {
          href[i] = codes[i];
          if (live) hfirst[hi] = codes[i];
        } else if (live) {
          layout_bad |= (uint32_t)(codes[i] != href[i]);
        }
        ++hi;
      }
      if (FINISH) keepc[i] = codes[i];
      if ((kbits >> i) & 1u) codes[i] = 0;
    }
  }
  float y0[3], y[3], p[3];
  dec_stage_d16<3>(y0, codes, &sh.dtab);
  q_stage_d16x<3>(y, y0, &sh.dtab, sh.tab.var);
  dampen_stage<3>(y, d);
  q_stage_d16x<3>(p, y, &sh.dtab, sh.tab.var);
  if (is_first) {
    A[0] = p[0], A[1] = p[1], A[2] = p[2];
  } else {
    const float sm[3] = {A[0] + p[0], A[1] + p[1], A[2] + p[2]};
    q_stage_d16x<3>(A, sm, &sh.dtab, sh.tab.var);
  }
}

// The step in two pieces for k_pool_fold_kd, which takes p between them: the upload's
// dampened value p (acc_lane_value: acc_lane_step up to its last stage, line for line) and
// its add into the running value (acc_lane_add). A copy, not a split of acc_lane_step:
// building that from the two pieces changed k_pool_fold's register allocation and added
// 29 instructions to it, and the sharing there already stops where it costs (the file's
// header).
template <bool FINISH>
__device__ __forceinline__ void acc_lane_value(const AccShared& sh, const uint8_t* src, bool live, uint32_t need,
                                               bool wave_keep, uint32_t hbits, uint32_t kbits, int h0, bool is_first,
                                               double d, int32_t* hfirst, int32_t (&href)[3], int32_t (&keepc)[3],
                                               float (&p)[3], uint32_t& bad, uint32_t& layout_bad) {
  uint4 w = uint4{0u, 0u, 0u, 0u};
  if (live) w = *reinterpret_cast<const uint4*>(src);
  int32_t codes[3];
  if (need == 0xffffu) bad |= live ? b64_decode_group_full(w, &sh.tab, codes) : 0u;
  else bad |= live ? (b64_decode_group(w, &sh.tab, codes) & need) : 0u;
  if (!live) codes[0] = codes[1] = codes[2] = 0;
  if (wave_keep) {
    int hi = h0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if ((hbits >> i) & 1u) {
        if (is_first) {
          href[i] = codes[i];
          if (live) hfirst[hi] = codes[i];
        } else if (live) {
          layout_bad |= (uint32_t)(codes[i] != href[i]);
        }
        ++hi;
      }
      if (FINISH) keepc[i] = codes[i];
      if ((kbits >> i) & 1u) codes[i] = 0;
    }
  }
  float y0[3], y[3];
  dec_stage_d16<3>(y0, codes, &sh.dtab);
  q_stage_d16x<3>(y, y0, &sh.dtab, sh.tab.var);
  dampen_stage<3>(y, d);
  q_stage_d16x<3>(p, y, &sh.dtab, sh.tab.var);
}
__device__ __forceinline__ void acc_lane_add(const AccShared& sh, bool is_first, const float (&p)[3], float (&A)[3]) {
  if (is_first) {
    A[0] = p[0], A[1] = p[1], A[2] = p[2];
  } else {
    const float sm[3] = {A[0] + p[0], A[1] + p[1], A[2] + p[2]};
    q_stage_d16x<3>(A, sm, &sh.dtab, sh.tab.var);
  }
}

// The finish epilogue on a live lane's group g: merged_code = Q(f32(f64(A) * inv))
// encoded, slots with a kbit the last accepted upload's own codes (keepc; mergeFlatGradient,
// CppNNUpdater.java:507-508). `merged` and `merged_f32` are addressed by the whole
// upload's group index: Base64 at byte 16 g, fp32 at value 3 g.
__device__ __forceinline__ void acc_lane_finish(const AccShared& sh, const float (&A)[3], const int32_t (&keepc)[3],
                                                uint32_t kbits, double inv, int64_t n_up, int64_t g, uint8_t* merged,
                                                float* merged_f32) {
  const int r = (int)min<int64_t>(3, n_up - 3 * g);
  int32_t out[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = i < r ? merged_code(A[i], inv, keepc[i], (kbits >> i) & 1u, &sh.tab) : 0;
  *reinterpret_cast<uint4*>(merged + 16 * g) = pad_group(b64_encode_group(out, &sh.tab), r);
  if (merged_f32) {
    float* mf = merged_f32 + 3 * g;
    if (r == 3) {
      *reinterpret_cast<f3u*>(mf) = f3u{dec_mt(out[0], sh.tab.mt), dec_mt(out[1], sh.tab.mt), dec_mt(out[2], sh.tab.mt)};
    } else {
      for (int e = 0; e < r; ++e) mf[e] = dec_mt(out[e], sh.tab.mt);
    }
  }
}

}  // namespace

// a launch's factors and the pool's picked slots, by value in the kernel arguments
struct AccDampen {
  double d[kAccBurst];
};
struct PoolPicks {
  int32_t slot[kAccBurst];
};

// All four kernels work on the groups [g_begin, g_end), a lane per group: rows and state
// hold that window alone (group g at byte 16 (g - g_begin), value 3 (g - g_begin)), one
// 16-byte row load per upload and at most one 12-byte state load and store per lane.

// One upload's step: state st_in -> st_out (st_in is not read when `first`).
__global__ void __launch_bounds__(kAccNT) k_acc_push(const uint8_t* __restrict__ row, const float* __restrict__ st_in,
                                                     float* __restrict__ st_out, int first, double dampen,
                                                     int64_t n_up, int64_t g_begin, int64_t g_end,
                                                     const int32_t* __restrict__ hdr_block,
                                                     int32_t* __restrict__ hfirst, int* __restrict__ err) {
  __shared__ AccShared sh;
  const AccHdr H = acc_block_open(sh, hdr_block);
  const int64_t ng = g_end - g_begin;
  uint32_t bad = 0, layout_bad = 0;
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    AccGroup G = acc_group_open(sh, H, base + threadIdx.x, ng, g_begin, n_up, first, st_in, hfirst);
    int32_t keepc[3];
    acc_lane_step<false>(sh, row + 16 * G.gs, G.live, G.need, G.wave_keep, G.hbits, G.kbits, G.h0, first, dampen, hfirst,
                         G.href, keepc, G.A, bad, layout_bad);
    if (G.live) *reinterpret_cast<f3u*>(st_out + 3 * G.gs) = f3u{G.A[0], G.A[1], G.A[2]};
  }
  if (bad) atomicOr(err, FLEET_ERRBIT_BASE64);
  if (layout_bad) atomicOr(err, FLEET_ERRBIT_LAYOUT);
}

// The merged gradient from the state `st` and the accumulator's copy of the last accepted
// upload's row (both in window coordinates).
__global__ void __launch_bounds__(kAccNT) k_acc_finish(const uint8_t* __restrict__ last_row,
                                                       const float* __restrict__ st, double inv, int64_t n_up,
                                                       int64_t g_begin, int64_t g_end,
                                                       const int32_t* __restrict__ hdr_block,
                                                       uint8_t* __restrict__ merged, float* __restrict__ merged_f32) {
  __shared__ AccShared sh;
  const AccHdr H = acc_block_open(sh, hdr_block);
  const int64_t ng = g_end - g_begin;
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    const int64_t gl = base + threadIdx.x;
    if (gl >= ng) break;
    const int64_t g = g_begin + gl;
    const uint4 w = *reinterpret_cast<const uint4*>(last_row + 16 * gl);
    const f3u a = *reinterpret_cast<const f3u*>(st + 3 * gl);
    const float A[3] = {a.x, a.y, a.z};
    int32_t codes[3];
    (void)b64_decode_group(w, &sh.tab, codes);  // checked when the row was pushed
    int h0;
    const uint32_t kbits = keep_bits<3>(acc_header_bits(sh, H.hdr, H.n_hdr, 3 * g, &h0), true, 3 * g, H.walk_end);
    acc_lane_finish(sh, A, codes, kbits, inv, n_up, g, merged, merged_f32);
  }
}

// A burst: the steps of K <= kAccBurst uploads in one launch, the running value in
// registers across them, so the state is read and written once per lane instead of once
// per upload. Rows 0..K-2 are rows + k * pitch, row K-1 is `last_row` (the accumulator's
// spare row when the burst ends there, so the finish finds "the last accepted upload"; a
// chunk of a longer burst passes rows + (K-1) * pitch). `first`: row 0 is the batch's
// first upload. The factors travel by value: the index is wave-uniform, so dampen_stage's
// test stays scalar. st_in and st_out may be the same buffer (the later chunks of a long
// burst): a lane reads its 12 bytes before it writes them.
//
// FINISH: the epilogue after the last upload, inv = 1 / (count + K), in place of the
// state store. `merged` may be `last_row` shifted back by the window's start and
// merged_f32 likewise `st_in` (the host form borrows the spare buffers): a lane reads its
// group before it writes it.
template <bool FINISH>
__global__ void __launch_bounds__(kAccNT) k_acc_push_many(const uint8_t* rows, size_t pitch, const uint8_t* last_row,
                                                          const float* st_in, float* st_out, int first, int K,
                                                          AccDampen dampen, double inv, int64_t n_up, int64_t g_begin,
                                                          int64_t g_end, const int32_t* __restrict__ hdr_block,
                                                          int32_t* hfirst, int* __restrict__ err, uint8_t* merged,
                                                          float* merged_f32) {
  __shared__ AccShared sh;
  const AccHdr H = acc_block_open(sh, hdr_block);
  const int64_t ng = g_end - g_begin;
  uint32_t bad = 0, layout_bad = 0;
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    AccGroup G = acc_group_open(sh, H, base + threadIdx.x, ng, g_begin, n_up, first, st_in, hfirst);
    int32_t keepc[3] = {0, 0, 0};  // row K-1's are the ones left after the loop
    for (int k = 0; k < K; ++k) {
      const uint8_t* src = (k == K - 1 ? last_row : rows + (size_t)k * pitch) + 16 * G.gs;
      acc_lane_step<FINISH>(sh, src, G.live, G.need, G.wave_keep, G.hbits, G.kbits, G.h0, first && k == 0, dampen.d[k],
                            hfirst, G.href, keepc, G.A, bad, layout_bad);
    }
    if (!FINISH) {
      if (G.live) *reinterpret_cast<f3u*>(st_out + 3 * G.gs) = f3u{G.A[0], G.A[1], G.A[2]};
    } else if (G.live) {
      acc_lane_finish(sh, G.A, keepc, G.kbits, inv, n_up, G.g, merged, merged_f32);
    }
  }
  if (bad) atomicOr(err, FLEET_ERRBIT_BASE64);
  if (layout_bad) atomicOr(err, FLEET_ERRBIT_LAYOUT);
}

// The upload pool's fold: the steps of K <= kAccBurst picked rows of a pool of resident
// uploads in one launch (the reference's `acc` with staleSize > 0, CppNNUpdater.java:
// 394-407: the server picks, at update time, which buffered uploads to aggregate). Pick
// k's row is pool + slot[k] * pitch; the slots travel by value beside the factors, so the
// row address stays scalar too. A longer pick list runs as consecutive launches over the
// one state buffer `st`: every launch but the first (`first`) reads the lane's 12 bytes,
// every launch but the last (FINISH) writes them; K <= kAccBurst picks move no state.
// FINISH: inv = 1 / picks of the whole update; merged_f32 may be `st` shifted back by the
// window's start (a lane reads its 12 bytes before it writes them).
// Errors are attributed per pick: a lane remembers in two 64-bit masks which picks failed
// the Base64 check or differed from the first pick's header codes and after all its
// groups ORs FLEET_ERRBIT_* into status[slot[k]]; clean data pays no atomics.
template <bool FINISH>
__global__ void __launch_bounds__(kAccNT) k_pool_fold(const uint8_t* pool, size_t pitch, PoolPicks picks, float* st,
                                                      int first, int K, AccDampen dampen, double inv, int64_t n_up,
                                                      int64_t g_begin, int64_t g_end,
                                                      const int32_t* __restrict__ hdr_block, int32_t* hfirst,
                                                      int* __restrict__ status, uint8_t* merged, float* merged_f32) {
  __shared__ AccShared sh;
  const AccHdr H = acc_block_open(sh, hdr_block);
  const int64_t ng = g_end - g_begin;
  uint64_t bad_picks = 0, layout_picks = 0;
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    const int64_t gl = base + threadIdx.x;
    const bool live = gl < ng;
    const int64_t gs = live ? gl : 0, g = g_begin + gs;  // acc_group_open, spelled out (the file's header)
    float A[3] = {0.f, 0.f, 0.f};
    if (!first && live) {
      const f3u a = *reinterpret_cast<const f3u*>(st + 3 * gs);
      A[0] = a.x, A[1] = a.y, A[2] = a.z;
    }
    const uint32_t need = needed_chars_mask((int)min<int64_t>(3, max<int64_t>(0, n_up - 3 * g)));
    int h0;
    const uint32_t hbits = acc_header_bits(sh, H.hdr, H.n_hdr, 3 * g, &h0);
    const uint32_t kbits = keep_bits<3>(hbits, true, 3 * g, H.walk_end);
    const bool wave_keep = __ballot(kbits != 0) != 0;
    int32_t href[3] = {0, 0, 0}, keepc[3] = {0, 0, 0};
    if (wave_keep && !first) {
      int hi = h0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if ((hbits >> i) & 1u) href[i] = hfirst[hi++];
    }
    for (int k = 0; k < K; ++k) {
      const uint8_t* src = pool + (size_t)picks.slot[k] * pitch + 16 * gs;
      uint32_t bad = 0, layout_bad = 0;
      acc_lane_step<FINISH>(sh, src, live, need, wave_keep, hbits, kbits, h0, first && k == 0, dampen.d[k], hfirst, href,
                            keepc, A, bad, layout_bad);
      bad_picks |= (uint64_t)(bad != 0) << k;
      layout_picks |= (uint64_t)(layout_bad != 0) << k;
    }
    if (!FINISH) {
      if (live) *reinterpret_cast<f3u*>(st + 3 * gs) = f3u{A[0], A[1], A[2]};
    } else if (live) {
      acc_lane_finish(sh, A, keepc, kbits, inv, n_up, g, merged, merged_f32);
    }
  }
  if (bad_picks | layout_picks) {
    for (int k = 0; k < K; ++k) {
      const int e = (((bad_picks >> k) & 1) ? FLEET_ERRBIT_BASE64 : 0) | (((layout_picks >> k) & 1) ? FLEET_ERRBIT_LAYOUT : 0);
      if (e) atomicOr(status + picks.slot[k], e);
    }
  }
}

// Kardam's side outputs of the pool's fold (the ledger, fleet_kledger_update*): pick k's
// previous row and output row in the slab of fp32 rows (-1: none) and its mode, by value
// beside the slots and the factors, so every test on them stays scalar.
constexpr int kKdNorm = 1, kKdDiff = 2, kKdStore = 4;
struct PoolKdRows {
  int32_t prev[kAccBurst];
  int32_t out[kAccBurst];
};
struct PoolKdModes {
  uint8_t m[kAccBurst];
};

// k_pool_fold with, per pick k, what kardam_lane_step does in the batch stream kernel
// (CppNNUpdater.java:478, Kardam.java:56-71), on the pick's p between the dampen stage
// and the add: G = Q(f32(f64(p) * lr)), sg = sum (double)(G * G) over the flat slots
// (neither header slots nor at or past the walk's end, where G is 0), with a previous row
// D = Q(G - prev) and sd = sum (double)(D * D), and for a storing pick G as the lane's 12
// bytes of its output row (upload coordinates; a row holds whole groups, so a ragged last
// group is stored whole, its tail 0). A pick's previous row may be the output row of an
// earlier pick of the launch (a worker picked twice): the same lane stored those 12 bytes,
// and the load follows the store in program order, so `slab` is not __restrict__ and the
// previous row is loaded inside its own pick's step, not a pick ahead.
// The norms: per pick the wave's sg / sd are reduced over the wave two picks at a time
// (quad_sum_f64, a last even pick by pair_sum_f64<64>) and added into the wave's own LDS
// slots kdp[wave][pick][2] across the grid-stride iterations; after them the wave stores
// its 2 K sums once, partials[(k * waves + w) * 2 + {0, 1}], w = 4 blockIdx.x + wave, and
// k_pool_kd_reduce adds the waves in a fixed order. No floating-point atomics: the same
// bits for the same inputs and grid. The ledger's pool covers the whole upload (g_begin =
// 0), so the lane's slots are 3 g .. 3 g + 2 in the row.
// merged, merged_f32, the state and status[] are k_pool_fold's: the loop below is that
// kernel's with the step in its two pieces.
template <bool FINISH>
__global__ void __launch_bounds__(kAccNT) k_pool_fold_kd(const uint8_t* pool, size_t pitch, PoolPicks picks, float* st,
                                                         int first, int K, AccDampen dampen, double inv, int64_t n_up,
                                                         int64_t g_begin, int64_t g_end,
                                                         const int32_t* __restrict__ hdr_block, int32_t* hfirst,
                                                         int* __restrict__ status, uint8_t* merged, float* merged_f32,
                                                         PoolKdRows rows, PoolKdModes modes, double lr, float* slab,
                                                         size_t vpitch, double* __restrict__ partials) {
  __shared__ AccShared sh;
  __shared__ double kdp[kAccNT / 64][kAccBurst][2];
  for (int i = threadIdx.x; i < (kAccNT / 64) * kAccBurst * 2; i += kAccNT) (&kdp[0][0][0])[i] = 0.0;
  const AccHdr H = acc_block_open(sh, hdr_block);  // (its barrier covers the zeroes)
  const int64_t ng = g_end - g_begin;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t bad_picks = 0, layout_picks = 0;
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    const int64_t gl = base + threadIdx.x;
    const bool live = gl < ng;
    const int64_t gs = live ? gl : 0, g = g_begin + gs;
    float A[3] = {0.f, 0.f, 0.f};
    if (!first && live) {
      const f3u a = *reinterpret_cast<const f3u*>(st + 3 * gs);
      A[0] = a.x, A[1] = a.y, A[2] = a.z;
    }
    const uint32_t need = needed_chars_mask((int)min<int64_t>(3, max<int64_t>(0, n_up - 3 * g)));
    int h0;
    const uint32_t hbits = acc_header_bits(sh, H.hdr, H.n_hdr, 3 * g, &h0);
    const uint32_t kbits = keep_bits<3>(hbits, true, 3 * g, H.walk_end);
    const bool wave_keep = __ballot(kbits != 0) != 0;
    const uint32_t flat = live ? ~kbits & 7u : 0u;
    int32_t href[3] = {0, 0, 0}, keepc[3] = {0, 0, 0};
    if (wave_keep && !first) {
      int hi = h0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if ((hbits >> i) & 1u) href[i] = hfirst[hi++];
    }
    double sg0 = 0.0, sd0 = 0.0;  // an even pick's sums, held for the pair
    int mode0 = 0;
    for (int k = 0; k < K; ++k) {
      const int mode = modes.m[k];
      float pv[3] = {0.f, 0.f, 0.f};
      if ((mode & kKdDiff) && live) {
        const f3u t = *reinterpret_cast<const f3u*>(slab + (size_t)rows.prev[k] * vpitch + 3 * gs);
        pv[0] = t.x, pv[1] = t.y, pv[2] = t.z;
      }
      const uint8_t* src = pool + (size_t)picks.slot[k] * pitch + 16 * gs;
      uint32_t bad = 0, layout_bad = 0;
      float p[3];
      acc_lane_value<FINISH>(sh, src, live, need, wave_keep, hbits, kbits, h0, first && k == 0, dampen.d[k], hfirst, href,
                             keepc, p, bad, layout_bad);
      bad_picks |= (uint64_t)(bad != 0) << k;
      layout_picks |= (uint64_t)(layout_bad != 0) << k;
      double sg = 0.0, sd = 0.0;
      if (mode & kKdNorm) {
        float rg[3] = {p[0], p[1], p[2]}, G[3];
        dampen_stage<3>(rg, lr);
        q_stage_d16x<3>(G, rg, &sh.dtab, sh.tab.var);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          G[i] = ((flat >> i) & 1u) ? G[i] : 0.0f;
          sg += (double)(G[i] * G[i]);
        }
        if (mode & kKdDiff) {
          float dv[3], D[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) dv[i] = ((flat >> i) & 1u) ? G[i] - pv[i] : 0.0f;
          q_stage_d16x<3>(D, dv, &sh.dtab, sh.tab.var);
#pragma unroll
          for (int i = 0; i < 3; ++i) sd += (double)(D[i] * D[i]);
        }
        if ((mode & kKdStore) && live)
          *reinterpret_cast<f3u*>(slab + (size_t)rows.out[k] * vpitch + 3 * gs) = f3u{G[0], G[1], G[2]};
      }
      acc_lane_add(sh, first && k == 0, p, A);
      if (k & 1) {
        if ((mode | mode0) & kKdNorm) {
          const double s = quad_sum_f64(sg0, sd0, sg, sd);
          if ((lane & 15) == 15)  // rows 0..3: (k - 1, g), (k, g), (k - 1, d), (k, d)
            kdp[wave][k - 1 + ((lane >> 4) & 1)][lane >> 5] += s;
        }
      } else if (k + 1 == K) {
        if (mode & kKdNorm) {
          const double s = pair_sum_f64<64>(sg, sd);
          if ((lane & 31) == 31) kdp[wave][k][lane >> 5] += s;
        }
      } else {
        sg0 = sg, sd0 = sd, mode0 = mode;
      }
    }
    if (!FINISH) {
      if (live) *reinterpret_cast<f3u*>(st + 3 * gs) = f3u{A[0], A[1], A[2]};
    } else if (live) {
      acc_lane_finish(sh, A, keepc, kbits, inv, n_up, g, merged, merged_f32);
    }
  }
  if (bad_picks | layout_picks) {
    for (int k = 0; k < K; ++k) {
      const int e = (((bad_picks >> k) & 1) ? FLEET_ERRBIT_BASE64 : 0) | (((layout_picks >> k) & 1) ? FLEET_ERRBIT_LAYOUT : 0);
      if (e) atomicOr(status + picks.slot[k], e);
    }
  }
  __syncthreads();  // the wave's slots were written by four (or two) of its lanes
  if (lane < K) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const size_t w = (size_t)blockIdx.x * (kAccNT / 64) + wave, waves = (size_t)gridDim.x * (kAccNT / 64);
    reinterpret_cast<d2*>(partials)[(size_t)lane * waves + w] = d2{kdp[wave][lane][0], kdp[wave][lane][1]};
  }
}

// Pick k's 2 sums from the waves' partials of one k_pool_fold_kd launch, in a fixed
// order: a lane adds every 256th wave's pair in turn, the wave folds by DPP lane moves
// (group_sum_f64), lane 0 adds the block's four waves in order. sums[2 k + {0, 1}].
__global__ void __launch_bounds__(kAccNT) k_pool_kd_reduce(const double* __restrict__ partials, int64_t waves,
                                                           double* __restrict__ sums) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  __shared__ double red[2][kAccNT / 64];
  const int k = blockIdx.x;
  const d2* p = reinterpret_cast<const d2*>(partials) + (size_t)k * waves;
  d2 v = d2{0.0, 0.0};
  for (int64_t w = threadIdx.x; w < waves; w += kAccNT) v += p[w];
  const double a = group_sum_f64<64>(v.x), b = group_sum_f64<64>(v.y);  // valid in lane 63
  if ((threadIdx.x & 63) == 63) {
    red[0][threadIdx.x / 64] = a;
    red[1][threadIdx.x / 64] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0.0, sb = 0.0;
    for (int i = 0; i < kAccNT / 64; ++i) {
      sa += red[0][i];
      sb += red[1][i];
    }
    sums[2 * k] = sa;
    sums[2 * k + 1] = sb;
  }
}

// The average as the next update's lastGrad reads it (CppNNUpdater.java:507, 510): avg =
// scalarMultiply(1 / avgSize) of the running value, decoded -- Q(f32(f64(A) * inv)) per
// slot. Not decodeFloat(merged): the merge decodes and encodes that value once more
// (merged_code), and Q is not idempotent on every value. Every lane of the wave calls
// (the stage's fallback is behind a ballot); a live lane stores its 12 bytes.
__device__ __forceinline__ void acc_lane_avg(const AccShared& sh, const float (&A)[3], double inv, bool live, float* out) {
  float r[3] = {A[0], A[1], A[2]}, q[3];
  dampen_stage<3>(r, inv);
  q_stage_d16x<3>(q, r, &sh.dtab, sh.tab.var);
  if (live) *reinterpret_cast<f3u*>(out) = f3u{q[0], q[1], q[2]};
}

// The filter form of k_pool_fold_kd (fleet_kfilter_update*): beside everything that kernel
// does, per pick k what Kardam.checkByz's checkNorm reads of the pick (Kardam.java:136-185,
// CppNNUpdater.java:488 without its `true ||`): sp = sum (double)(p * p) over the flat slots,
// p the pick's dampened value before the learning rate, and, with a previous average
// `lastg` (one fp32 row in upload coordinates, the avg of the last update that had one as
// acc_lane_avg leaves it; nullptr: none), E = Q(p - L) and se = sum (double)(E * E). A lane loads
// its 12 bytes of L once per group, before the pick loop. sp does not depend on the pick's
// mode: the filter's norm is taken of every pick, a worker[k] < 0 one included. The finish
// form also leaves this update's avg in `avg_out` (another row than `lastg`).
// The wave's slots are kfp[wave][pick][4] = {sg, sd, sp, se}: sg / sd go through
// k_pool_fold_kd's reduction line for line (the same bits as the ledger form gives), and
// sp / se through a second one of the same shape. partials[(k * waves + w) * 4 + 0..3];
// k_pool_kf_reduce adds the waves in k_pool_kd_reduce's order. A sibling, not a flag of
// k_pool_fold_kd: that kernel's instantiations stay what they were.
// Occupancy: the ledger form's finish instantiation takes 91 VGPRs, five waves a SIMD.
// Left to itself this kernel takes 99, one wave fewer; asked for five waves it fits 89
// without scratch. Its 26432 bytes of LDS (AccShared + 8 KiB of slots) allow six blocks a
// CU, so the registers stay the bound, as they are for the ledger form (22336 bytes, seven).
template <bool FINISH>
__global__ void __launch_bounds__(kAccNT) __attribute__((amdgpu_waves_per_eu(5))) k_pool_fold_kf(const uint8_t* pool, size_t pitch, PoolPicks picks, float* st,
                                                         int first, int K, AccDampen dampen, double inv, int64_t n_up,
                                                         int64_t g_begin, int64_t g_end,
                                                         const int32_t* __restrict__ hdr_block, int32_t* hfirst,
                                                         int* __restrict__ status, uint8_t* merged, float* merged_f32,
                                                         PoolKdRows rows, PoolKdModes modes, double lr, float* slab,
                                                         size_t vpitch, double* __restrict__ partials,
                                                         const float* __restrict__ lastg, float* __restrict__ avg_out) {
  __shared__ AccShared sh;
  __shared__ double kfp[kAccNT / 64][kAccBurst][4];
  for (int i = threadIdx.x; i < (kAccNT / 64) * kAccBurst * 4; i += kAccNT) (&kfp[0][0][0])[i] = 0.0;
  const AccHdr H = acc_block_open(sh, hdr_block);  // (its barrier covers the zeroes)
  const int64_t ng = g_end - g_begin;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool has_last = lastg != nullptr;
  uint64_t bad_picks = 0, layout_picks = 0;
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    const int64_t gl = base + threadIdx.x;
    const bool live = gl < ng;
    const int64_t gs = live ? gl : 0, g = g_begin + gs;
    float A[3] = {0.f, 0.f, 0.f};
    if (!first && live) {
      const f3u a = *reinterpret_cast<const f3u*>(st + 3 * gs);
      A[0] = a.x, A[1] = a.y, A[2] = a.z;
    }
    float Lv[3] = {0.f, 0.f, 0.f};
    if (has_last && live) {
      const f3u t = *reinterpret_cast<const f3u*>(lastg + 3 * gs);
      Lv[0] = t.x, Lv[1] = t.y, Lv[2] = t.z;
    }
    const uint32_t need = needed_chars_mask((int)min<int64_t>(3, max<int64_t>(0, n_up - 3 * g)));
    int h0;
    const uint32_t hbits = acc_header_bits(sh, H.hdr, H.n_hdr, 3 * g, &h0);
    const uint32_t kbits = keep_bits<3>(hbits, true, 3 * g, H.walk_end);
    const bool wave_keep = __ballot(kbits != 0) != 0;
    const uint32_t flat = live ? ~kbits & 7u : 0u;
    int32_t href[3] = {0, 0, 0}, keepc[3] = {0, 0, 0};
    if (wave_keep && !first) {
      int hi = h0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if ((hbits >> i) & 1u) href[i] = hfirst[hi++];
    }
    double sg0 = 0.0, sd0 = 0.0, sp0 = 0.0, se0 = 0.0;  // an even pick's sums, held for the pair
    int mode0 = 0;
    for (int k = 0; k < K; ++k) {
      const int mode = modes.m[k];
      float pv[3] = {0.f, 0.f, 0.f};
      if ((mode & kKdDiff) && live) {
        const f3u t = *reinterpret_cast<const f3u*>(slab + (size_t)rows.prev[k] * vpitch + 3 * gs);
        pv[0] = t.x, pv[1] = t.y, pv[2] = t.z;
      }
      const uint8_t* src = pool + (size_t)picks.slot[k] * pitch + 16 * gs;
      uint32_t bad = 0, layout_bad = 0;
      float p[3];
      acc_lane_value<FINISH>(sh, src, live, need, wave_keep, hbits, kbits, h0, first && k == 0, dampen.d[k], hfirst, href,
                             keepc, p, bad, layout_bad);
      bad_picks |= (uint64_t)(bad != 0) << k;
      layout_picks |= (uint64_t)(layout_bad != 0) << k;
      double sg = 0.0, sd = 0.0, sp = 0.0, se = 0.0;
      float pf[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        pf[i] = ((flat >> i) & 1u) ? p[i] : 0.0f;
        sp += (double)(pf[i] * pf[i]);
      }
      if (has_last) {
        float ev[3], E[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) ev[i] = ((flat >> i) & 1u) ? pf[i] - Lv[i] : 0.0f;
        q_stage_d16x<3>(E, ev, &sh.dtab, sh.tab.var);
#pragma unroll
        for (int i = 0; i < 3; ++i) se += (double)(E[i] * E[i]);
      }
      if (mode & kKdNorm) {
        float rg[3] = {p[0], p[1], p[2]}, G[3];
        dampen_stage<3>(rg, lr);
        q_stage_d16x<3>(G, rg, &sh.dtab, sh.tab.var);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          G[i] = ((flat >> i) & 1u) ? G[i] : 0.0f;
          sg += (double)(G[i] * G[i]);
        }
        if (mode & kKdDiff) {
          float dv[3], D[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) dv[i] = ((flat >> i) & 1u) ? G[i] - pv[i] : 0.0f;
          q_stage_d16x<3>(D, dv, &sh.dtab, sh.tab.var);
#pragma unroll
          for (int i = 0; i < 3; ++i) sd += (double)(D[i] * D[i]);
        }
        if ((mode & kKdStore) && live)
          *reinterpret_cast<f3u*>(slab + (size_t)rows.out[k] * vpitch + 3 * gs) = f3u{G[0], G[1], G[2]};
      }
      acc_lane_add(sh, first && k == 0, p, A);
      if (k & 1) {
        if ((mode | mode0) & kKdNorm) {
          const double s = quad_sum_f64(sg0, sd0, sg, sd);
          if ((lane & 15) == 15)  // rows 0..3: (k - 1, g), (k, g), (k - 1, d), (k, d)
            kfp[wave][k - 1 + ((lane >> 4) & 1)][lane >> 5] += s;
        }
        const double t = quad_sum_f64(sp0, se0, sp, se);
        if ((lane & 15) == 15) kfp[wave][k - 1 + ((lane >> 4) & 1)][2 + (lane >> 5)] += t;
      } else if (k + 1 == K) {
        if (mode & kKdNorm) {
          const double s = pair_sum_f64<64>(sg, sd);
          if ((lane & 31) == 31) kfp[wave][k][lane >> 5] += s;
        }
        const double t = pair_sum_f64<64>(sp, se);
        if ((lane & 31) == 31) kfp[wave][k][2 + (lane >> 5)] += t;
      } else {
        sg0 = sg, sd0 = sd, sp0 = sp, se0 = se, mode0 = mode;
      }
    }
    if (!FINISH) {
      if (live) *reinterpret_cast<f3u*>(st + 3 * gs) = f3u{A[0], A[1], A[2]};
    } else {
      if (live) acc_lane_finish(sh, A, keepc, kbits, inv, n_up, g, merged, merged_f32);
      acc_lane_avg(sh, A, inv, live, avg_out + 3 * gs);
    }
  }
  if (bad_picks | layout_picks) {
    for (int k = 0; k < K; ++k) {
      const int e = (((bad_picks >> k) & 1) ? FLEET_ERRBIT_BASE64 : 0) | (((layout_picks >> k) & 1) ? FLEET_ERRBIT_LAYOUT : 0);
      if (e) atomicOr(status + picks.slot[k], e);
    }
  }
  __syncthreads();  // the wave's slots were written by four (or two) of its lanes
  if (lane < K) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const size_t w = (size_t)blockIdx.x * (kAccNT / 64) + wave, waves = (size_t)gridDim.x * (kAccNT / 64);
    d2* out = reinterpret_cast<d2*>(partials) + ((size_t)lane * waves + w) * 2;
    out[0] = d2{kfp[wave][lane][0], kfp[wave][lane][1]};
    out[1] = d2{kfp[wave][lane][2], kfp[wave][lane][3]};
  }
}

// k_pool_kd_reduce over four sums per pick: the same lanes add the same waves in the same
// order per component. sums[4 k + 0..3].
__global__ void __launch_bounds__(kAccNT) k_pool_kf_reduce(const double* __restrict__ partials, int64_t waves,
                                                           double* __restrict__ sums) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  __shared__ double red[4][kAccNT / 64];
  const int k = blockIdx.x;
  const d2* p = reinterpret_cast<const d2*>(partials) + (size_t)k * waves * 2;
  d2 v = d2{0.0, 0.0}, u = d2{0.0, 0.0};
  for (int64_t w = threadIdx.x; w < waves; w += kAccNT) {
    v += p[2 * w];
    u += p[2 * w + 1];
  }
  const double a = group_sum_f64<64>(v.x), b = group_sum_f64<64>(v.y);  // valid in lane 63
  const double c = group_sum_f64<64>(u.x), d = group_sum_f64<64>(u.y);
  if ((threadIdx.x & 63) == 63) {
    red[0][threadIdx.x / 64] = a;
    red[1][threadIdx.x / 64] = b;
    red[2][threadIdx.x / 64] = c;
    red[3][threadIdx.x / 64] = d;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double s = 0.0;
    for (int i = 0; i < kAccNT / 64; ++i) s += red[threadIdx.x][i];
    sums[4 * k + threadIdx.x] = s;
  }
}

// acc_lane_avg over a state: the avg row of a fold that ran without its finish (the
// filter's refold, whose finish is k_acc_finish).
__global__ void __launch_bounds__(kAccNT) k_acc_avg_row(const float* __restrict__ st, double inv, int64_t ng,
                                                        const int32_t* __restrict__ hdr_block,
                                                        float* __restrict__ avg_out) {
  __shared__ AccShared sh;
  (void)acc_block_open(sh, hdr_block);
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    const int64_t gl = base + threadIdx.x;
    const bool live = gl < ng;
    const int64_t gs = live ? gl : 0;
    float A[3] = {0.f, 0.f, 0.f};
    if (live) {
      const f3u a = *reinterpret_cast<const f3u*>(st + 3 * gs);
      A[0] = a.x, A[1] = a.y, A[2] = a.z;
    }
    acc_lane_avg(sh, A, inv, live, avg_out + 3 * gs);
  }
}

// The largest of v >= 0 over the wave, valid in lane 63: group_sum_f64<64>'s DPP lane moves
// with a maximum for the add (a row the move leaves out reads 0, which no maximum of
// magnitudes notices). Every lane of the wave active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_max_f32(float v) {
  v = fmaxf(v, dpp_move_f32<0x141, 0xf>(v));  // row_half_mirror
  v = fmaxf(v, dpp_move_f32<0x4e, 0xf>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_move_f32<0xb1, 0xf>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_move_f32<0x140, 0xf>(v));  // row_mirror
  v = fmaxf(v, dpp_move_f32<0x142, 0xa>(v));  // row_bcast15 into rows 1, 3
  v = fmaxf(v, dpp_move_f32<0x143, 0x8>(v));  // row_bcast31 into row 3
  return v;
}

// The arrival gate's pass over K <= kAccBurst resident rows of a pool (fleet_gate_vet*): per
// slot what an update would find wrong with the upload, and what the reference can say of
// it on arrival -- new ByteVec(getFlatGradient(g)).getNorm() (cppNN_backend.cpp:701-720,
// 779-795) -- without folding anything. Per slot k and group, in k_pool_fold's order: the
// lane's 16 bytes of the row, the Base64 check under acc_lane_step's `need` mask (so the
// verdict is the fold's, character for character), with `expected` (n_hdr codes, indexed
// by the header's index in the whole upload; nullptr: no header check) every header slot's
// code against expected[h0 + i], the code of every slot with a kbit taken as 0, y =
// Q(dec(code)) by the fold's first two stages, and over the flat slots of live lanes
// ss += (double)(y * y) -- getNorm's fp32 product, widened -- and m = max(m, |y|).
// The wave's ss and m of a slot are reduced over the wave (group_sum_f64<64>,
// wave_max_f32) and folded into the wave's own LDS cells across the grid-stride
// iterations; after them the wave stores {ss, m} once per slot, partials[(k * waves + w)
// * 2 + {0, 1}], and k_pool_vet_reduce adds the waves in a fixed order. No floating-point
// atomics, and nothing of slot k's path reads another slot's values or its position in
// the launch: the same bits for a slot vetted alone or in any burst.
// Errors per slot as k_pool_fold attributes them, ORed into status[k] -- the gate's own
// words, one per slot of the launch, not the pool's per-slot status. The kernel reads the
// rows and the header block and writes status[] and partials[] alone.
__global__ void __launch_bounds__(kAccNT) k_pool_vet(const uint8_t* __restrict__ pool, size_t pitch, PoolPicks picks,
                                                     int K, int64_t n_up, int64_t g_begin, int64_t g_end,
                                                     const int32_t* __restrict__ hdr_block,
                                                     const int32_t* __restrict__ expected, int* __restrict__ status,
                                                     double* __restrict__ partials) {
  __shared__ AccShared sh;
  __shared__ double vss[kAccNT / 64][kAccBurst];
  __shared__ float vmx[kAccNT / 64][kAccBurst];
  for (int i = threadIdx.x; i < (kAccNT / 64) * kAccBurst; i += kAccNT) {
    (&vss[0][0])[i] = 0.0;
    (&vmx[0][0])[i] = 0.0f;
  }
  const AccHdr H = acc_block_open(sh, hdr_block);  // (its barrier covers the zeroes)
  const int64_t ng = g_end - g_begin;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool check = expected != nullptr;
  uint64_t bad_picks = 0, layout_picks = 0;
  for (int64_t base = (int64_t)blockIdx.x * kAccNT; base < ng; base += (int64_t)gridDim.x * kAccNT) {
    const int64_t gl = base + threadIdx.x;
    const bool live = gl < ng;
    const int64_t gs = live ? gl : 0, g = g_begin + gs;
    const uint32_t need = needed_chars_mask((int)min<int64_t>(3, max<int64_t>(0, n_up - 3 * g)));
    int h0;
    const uint32_t hbits = acc_header_bits(sh, H.hdr, H.n_hdr, 3 * g, &h0);
    const uint32_t kbits = keep_bits<3>(hbits, true, 3 * g, H.walk_end);
    const bool wave_keep = __ballot(kbits != 0) != 0;
    const uint32_t flat = live ? ~kbits & 7u : 0u;
    int32_t want[3] = {0, 0, 0};
    if (wave_keep && check) {
      int hi = h0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if ((hbits >> i) & 1u) want[i] = expected[hi++];
    }
    for (int k = 0; k < K; ++k) {
      const uint8_t* src = pool + (size_t)picks.slot[k] * pitch + 16 * gs;
      uint4 w = uint4{0u, 0u, 0u, 0u};
      if (live) w = *reinterpret_cast<const uint4*>(src);
      int32_t codes[3];
      uint32_t bad = 0, layout_bad = 0;
      if (need == 0xffffu) bad = live ? b64_decode_group_full(w, &sh.tab, codes) : 0u;
      else bad = live ? (b64_decode_group(w, &sh.tab, codes) & need) : 0u;
      if (!live) codes[0] = codes[1] = codes[2] = 0;
      if (wave_keep) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (((hbits >> i) & 1u) && check && live) layout_bad |= (uint32_t)(codes[i] != want[i]);
          if ((kbits >> i) & 1u) codes[i] = 0;
        }
      }
      bad_picks |= (uint64_t)(bad != 0) << k;
      layout_picks |= (uint64_t)(layout_bad != 0) << k;
      float y0[3], y[3];
      dec_stage_d16<3>(y0, codes, &sh.dtab);
      q_stage_d16x<3>(y, y0, &sh.dtab, sh.tab.var);
      double ss = 0.0;
      float m = 0.0f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float yf = ((flat >> i) & 1u) ? y[i] : 0.0f;
        ss += (double)(yf * yf);
        m = fmaxf(m, fabsf(yf));
      }
      const double s = group_sum_f64<64>(ss);
      const float mm = wave_max_f32(m);
      if (lane == 63) {
        vss[wave][k] += s;
        vmx[wave][k] = fmaxf(vmx[wave][k], mm);
      }
    }
  }
  if (bad_picks | layout_picks) {
    for (int k = 0; k < K; ++k) {
      const int e = (((bad_picks >> k) & 1) ? FLEET_ERRBIT_BASE64 : 0) | (((layout_picks >> k) & 1) ? FLEET_ERRBIT_LAYOUT : 0);
      if (e) atomicOr(status + k, e);
    }
  }
  __syncthreads();  // the wave's cells were written by its last lane
  if (lane < K) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const size_t w = (size_t)blockIdx.x * (kAccNT / 64) + wave, waves = (size_t)gridDim.x * (kAccNT / 64);
    reinterpret_cast<d2*>(partials)[(size_t)lane * waves + w] = d2{vss[wave][lane], (double)vmx[wave][lane]};
  }
}

// Slot k's results from the waves' partials of one k_pool_vet launch: a lane adds every
// 256th wave's ss in turn and keeps the largest m, the wave folds by DPP lane moves, lane 0
// adds the block's four waves in order. The slot's status word travels with them, so the
// three outputs of a launch land in the caller's arrays (device or the gate's own) at k.
// waves = 0 (an empty window, nothing launched before): 0, 0 and the cleared status.
__global__ void __launch_bounds__(kAccNT) k_pool_vet_reduce(const double* __restrict__ partials, int64_t waves,
                                                            const int* __restrict__ status,
                                                            int32_t* __restrict__ out_status,
                                                            double* __restrict__ out_sumsq,
                                                            float* __restrict__ out_max) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  __shared__ double red[kAccNT / 64];
  __shared__ float redm[kAccNT / 64];
  const int k = blockIdx.x;
  const d2* p = reinterpret_cast<const d2*>(partials) + (size_t)k * waves;
  double v = 0.0;
  float m = 0.0f;
  for (int64_t w = threadIdx.x; w < waves; w += kAccNT) {
    const d2 t = p[w];
    v += t.x;
    m = fmaxf(m, (float)t.y);
  }
  const double a = group_sum_f64<64>(v);  // valid in lane 63
  const float b = wave_max_f32(m);
  if ((threadIdx.x & 63) == 63) {
    red[threadIdx.x / 64] = a;
    redm[threadIdx.x / 64] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0.0;
    float sm = 0.0f;
    for (int i = 0; i < kAccNT / 64; ++i) {
      sa += red[i];
      sm = fmaxf(sm, redm[i]);
    }
    out_status[k] = status[k];
    out_sumsq[k] = sa;
    out_max[k] = sm;
  }
}

// Element-wise kernels: a grid of whole blocks per CU (8 x 256 lanes fill a CU's wave
// slots), striding over the groups, so the tables are copied into LDS once per block.
static unsigned acc_grid(int64_t groups) {
  static std::atomic<int> cus_of[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    dev = 0;
  }
  const bool cached = dev >= 0 && dev < 64;
  int cus = cached ? cus_of[dev].load(std::memory_order_relaxed) : 0;
  if (!cus) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
      (void)hipGetLastError();
      cus = 256;
    }
    if (cached) cus_of[dev].store(cus, std::memory_order_relaxed);
  }
  const int64_t need = (groups + kAccNT - 1) / kAccNT;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(need, 8LL * cus));
}

// One launch over the window's groups; an empty window launches nothing.
template <typename... P, typename... A>
static hipError_t acc_launch(void (*kern)(P...), const AccWindow& w, hipStream_t s, A... args) {
  if (w.g_end <= w.g_begin) return hipSuccess;
  kern<<<dim3(acc_grid(w.g_end - w.g_begin)), dim3(kAccNT), 0, s>>>(args...);
  return hipGetLastError();
}

// the K factors of a launch by value
static AccDampen acc_dampen(const double* dampen, int K) {
  AccDampen d;
  for (int k = 0; k < kAccBurst; ++k) d.d[k] = k < K ? dampen[k] : 1.0;
  return d;
}

hipError_t launch_acc_push(const uint8_t* row, const float* st_in, float* st_out, int first, double dampen,
                           const AccWindow& w, int* d_err, hipStream_t s) {
  return acc_launch(k_acc_push, w, s, row, st_in, st_out, first, dampen, w.n_up, w.g_begin, w.g_end, w.d_hdr_block,
                    w.d_hfirst, d_err);
}

hipError_t launch_acc_finish(const uint8_t* last_row, const float* st, double inv, const AccWindow& w, uint8_t* merged,
                             float* merged_f32, hipStream_t s) {
  return acc_launch(k_acc_finish, w, s, last_row, st, inv, w.n_up, w.g_begin, w.g_end, w.d_hdr_block, merged,
                    merged_f32);
}

hipError_t launch_acc_push_many(const uint8_t* rows, size_t pitch, const uint8_t* last_row, const float* st_in,
                                float* st_out, int first, int K, const double* dampen, bool finish, double inv,
                                const AccWindow& w, int* d_err, uint8_t* merged, float* merged_f32, hipStream_t s) {
  if (K <= 0 || K > kAccBurst) return hipErrorInvalidValue;
  return acc_launch(finish ? k_acc_push_many<true> : k_acc_push_many<false>, w, s, rows, pitch, last_row, st_in, st_out,
                    first, K, acc_dampen(dampen, K), inv, w.n_up, w.g_begin, w.g_end, w.d_hdr_block, w.d_hfirst, d_err,
                    merged, merged_f32);
}

hipError_t launch_pool_fold(const uint8_t* pool, size_t pitch, const int32_t* slots, float* st, int first, int K,
                            const double* dampen, bool finish, double inv, const AccWindow& w, int* d_status,
                            uint8_t* merged, float* merged_f32, hipStream_t s) {
  if (K <= 0 || K > kAccBurst) return hipErrorInvalidValue;
  PoolPicks p;
  for (int k = 0; k < kAccBurst; ++k) p.slot[k] = k < K ? slots[k] : 0;
  return acc_launch(finish ? k_pool_fold<true> : k_pool_fold<false>, w, s, pool, pitch, p, st, first, K,
                    acc_dampen(dampen, K), inv, w.n_up, w.g_begin, w.g_end, w.d_hdr_block, w.d_hfirst, d_status, merged,
                    merged_f32);
}

int64_t pool_kd_partial_doubles(const AccWindow& w) {
  return (int64_t)acc_grid(std::max<int64_t>(1, w.g_end - w.g_begin)) * (kAccNT / 64) * kAccBurst * 2;
}
int64_t pool_kf_partial_doubles(const AccWindow& w) { return 2 * pool_kd_partial_doubles(w); }

// the picks, rows and modes of a launch by value; false for a mode that names no row, or
// a row outside the slab: such a launch never reaches the kernel
static bool pool_kd_args(const int32_t* slots, int K, const PoolKd& kd, PoolPicks* p, PoolKdRows* r, PoolKdModes* m) {
  for (int k = 0; k < kAccBurst; ++k) {
    p->slot[k] = k < K ? slots[k] : 0;
    m->m[k] = k < K ? kd.mode[k] : 0;
    r->prev[k] = k < K && (m->m[k] & kKdDiff) ? kd.prev[k] : -1;
    r->out[k] = k < K && (m->m[k] & kKdStore) ? kd.out[k] : -1;
    if ((m->m[k] & (kKdDiff | kKdStore)) && !(m->m[k] & kKdNorm)) return false;
    if ((m->m[k] & kKdDiff) && (r->prev[k] < 0 || r->prev[k] >= kd.rows)) return false;
    if ((m->m[k] & kKdStore) && (r->out[k] < 0 || r->out[k] >= kd.rows)) return false;
  }
  return true;
}

hipError_t launch_pool_fold_kf(const uint8_t* pool, size_t pitch, const int32_t* slots, float* st, int first, int K,
                               const double* dampen, bool finish, double inv, const AccWindow& w, int* d_status,
                               uint8_t* merged, float* merged_f32, const PoolKd& kd, const float* lastg,
                               float* avg_out, hipStream_t s) {
  if (K <= 0 || K > kAccBurst || w.g_begin != 0 || w.g_end <= 0 || (finish && !avg_out) || avg_out == lastg)
    return hipErrorInvalidValue;
  if (!kd.slab || !kd.partials || !kd.sums || kd.vpitch < (size_t)(3 * w.g_end)) return hipErrorInvalidValue;
  PoolPicks p;
  PoolKdRows r;
  PoolKdModes m;
  if (!pool_kd_args(slots, K, kd, &p, &r, &m)) return hipErrorInvalidValue;
  const unsigned grid = acc_grid(w.g_end - w.g_begin);
  hipError_t e = acc_launch(finish ? k_pool_fold_kf<true> : k_pool_fold_kf<false>, w, s, pool, pitch, p, st, first, K,
                            acc_dampen(dampen, K), inv, w.n_up, w.g_begin, w.g_end, w.d_hdr_block, w.d_hfirst,
                            d_status, merged, merged_f32, r, m, kd.lr, kd.slab, kd.vpitch, kd.partials, lastg, avg_out);
  if (e != hipSuccess) return e;
  k_pool_kf_reduce<<<dim3((unsigned)K), dim3(kAccNT), 0, s>>>(kd.partials, (int64_t)grid * (kAccNT / 64), kd.sums);
  return hipGetLastError();
}

int64_t pool_vet_partial_doubles(const AccWindow& w) { return pool_kd_partial_doubles(w); }

hipError_t launch_pool_vet(const uint8_t* pool, size_t pitch, const int32_t* slots, int K, const AccWindow& w,
                           const int32_t* d_expected, int* d_work_status, double* partials, int32_t* out_status,
                           double* out_sumsq, float* out_max, hipStream_t s) {
  if (K <= 0 || K > kAccBurst || !pool || !slots || !d_work_status || !partials || !out_status || !out_sumsq || !out_max)
    return hipErrorInvalidValue;
  PoolPicks p;
  for (int k = 0; k < kAccBurst; ++k) p.slot[k] = k < K ? slots[k] : 0;
  hipError_t e = hipMemsetAsync(d_work_status, 0, sizeof(int) * (size_t)K, s);
  if (e != hipSuccess) return e;
  const bool empty = w.g_end <= w.g_begin;
  const unsigned grid = acc_grid(std::max<int64_t>(1, w.g_end - w.g_begin));
  e = acc_launch(k_pool_vet, w, s, pool, pitch, p, K, w.n_up, w.g_begin, w.g_end, w.d_hdr_block, d_expected,
                 d_work_status, partials);
  if (e != hipSuccess) return e;
  k_pool_vet_reduce<<<dim3((unsigned)K), dim3(kAccNT), 0, s>>>(partials, empty ? 0 : (int64_t)grid * (kAccNT / 64),
                                                               d_work_status, out_status, out_sumsq, out_max);
  return hipGetLastError();
}

hipError_t launch_acc_avg_row(const float* st, double inv, const AccWindow& w, float* avg_out, hipStream_t s) {
  if (!st || !avg_out) return hipErrorInvalidValue;
  return acc_launch(k_acc_avg_row, w, s, st, inv, w.g_end - w.g_begin, w.d_hdr_block, avg_out);
}

hipError_t launch_pool_fold_kd(const uint8_t* pool, size_t pitch, const int32_t* slots, float* st, int first, int K,
                               const double* dampen, bool finish, double inv, const AccWindow& w, int* d_status,
                               uint8_t* merged, float* merged_f32, const PoolKd& kd, hipStream_t s) {
  if (K <= 0 || K > kAccBurst || w.g_begin != 0 || w.g_end <= 0) return hipErrorInvalidValue;
  if (!kd.slab || !kd.partials || !kd.sums || kd.vpitch < (size_t)(3 * w.g_end)) return hipErrorInvalidValue;
  PoolPicks p;
  PoolKdRows r;
  PoolKdModes m;
  for (int k = 0; k < kAccBurst; ++k) {
    p.slot[k] = k < K ? slots[k] : 0;
    m.m[k] = k < K ? kd.mode[k] : 0;
    r.prev[k] = k < K && (m.m[k] & kKdDiff) ? kd.prev[k] : -1;
    r.out[k] = k < K && (m.m[k] & kKdStore) ? kd.out[k] : -1;
    // a mode that names no row, or a row outside the slab, never reaches the kernel
    if ((m.m[k] & (kKdDiff | kKdStore)) && !(m.m[k] & kKdNorm)) return hipErrorInvalidValue;
    if ((m.m[k] & kKdDiff) && (r.prev[k] < 0 || r.prev[k] >= kd.rows)) return hipErrorInvalidValue;
    if ((m.m[k] & kKdStore) && (r.out[k] < 0 || r.out[k] >= kd.rows)) return hipErrorInvalidValue;
  }
  const unsigned grid = acc_grid(w.g_end - w.g_begin);
  hipError_t e = acc_launch(finish ? k_pool_fold_kd<true> : k_pool_fold_kd<false>, w, s, pool, pitch, p, st, first, K,
                            acc_dampen(dampen, K), inv, w.n_up, w.g_begin, w.g_end, w.d_hdr_block, w.d_hfirst,
                            d_status, merged, merged_f32, r, m, kd.lr, kd.slab, kd.vpitch, kd.partials);
  if (e != hipSuccess) return e;
  k_pool_kd_reduce<<<dim3((unsigned)K), dim3(kAccNT), 0, s>>>(kd.partials, (int64_t)grid * (kAccNT / 64), kd.sums);
  return hipGetLastError();
}

}  // namespace fleet

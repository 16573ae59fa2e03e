// fleet_amd/csrc/kardam_state.cpp -- Kardam's state behind the C-ABI: the gradient ledger
// (fleet_kledger) and the Byzantine filter (fleet_kfilter) beside an upload pool, whose
// members they read and write (pool_state.h), and the model ledger (fleet_mledger).
#include <cmath>
#include <cstring>

#include "pool_state.h"
#include "mledger_table.h"

using namespace fleet::host;

// --------------------------------------------------------------- Kardam ledger

// Kardam.java's `grads` map (worker -> (g, epoch), Kardam.java:40, 56-71) with every g
// one fp32 row of a slab in HBM (upload coordinates, header slots 0). An update's picks
// are resolved against the tables on the host, in pick order, into (mode, prev row, out
// row) per pick; G always goes to a free row, and the tables change after the slot
// status came back clean, so a rejected update leaves no trace.
struct fleet_kledger {
  fleet_pool* p = nullptr;
  int workers = 0, max_store = 0, rows = 0;
  size_t vpitch = 0;           // floats per row: 12 G bytes rounded up to 16
  DevBuf<float> d_slab;
  DevBuf<double> d_part;       // one launch's per-wave partials
  DevBuf<double> d_sums;       // 2 sums per pick of an update (picks are distinct slots)
  PinBuf<double> h_sums;
  std::vector<int32_t> row_of, epoch_of, free_rows;
  // one update's resolution
  std::vector<int32_t> t_row, t_epoch, t_free, t_release, k_prev, k_out;
  std::vector<uint8_t> k_mode, k_set;
};

namespace {

static int kledger_worker_arg(const fleet_kledger* l, int worker, const char* what) {
  if (worker < 0 || worker >= l->workers)
    return fail(l->p->c, FLEET_ERR_ARG, "%s: worker %d outside [0, %d)", what, worker, l->workers);
  if (l->row_of[worker] < 0) return fail(l->p->c, FLEET_ERR_ARG, "%s: worker %d is not in the ledger", what, worker);
  return FLEET_OK;
}

// Kardam.setGrad's decisions (Kardam.java:56-71) for the picks in order, on copies of the
// tables; FLEET_ERR_ARG before anything is launched.
static int kledger_resolve(fleet_kledger* l, int K, const int32_t* worker, const int32_t* epoch, const char* what) {
  fleet_ctx* c = l->p->c;
  for (int k = 0; k < K; ++k)
    if (worker[k] >= l->workers) return fail(c, FLEET_ERR_ARG, "%s: pick %d names worker %d of %d", what, k, worker[k], l->workers);
  l->t_row = l->row_of, l->t_epoch = l->epoch_of, l->t_free = l->free_rows;
  l->t_release.clear();
  l->k_mode.assign((size_t)K, 0), l->k_set.assign((size_t)K, 0);
  l->k_prev.assign((size_t)K, -1), l->k_out.assign((size_t)K, -1);
  int stores = 0;
  for (int k = 0; k < K; ++k) {
    const int w = worker[k];
    if (w < 0) continue;  // Kardam does not run for this pick (CppNNUpdater.java:472-474)
    const int32_t cur = l->t_row[w];
    if (cur >= 0 && l->t_epoch[w] == epoch[k]) {  // the push is ignored (Kardam.java:59-62)
      l->k_mode[k] = 1;
      continue;
    }
    if (++stores > l->max_store || l->t_free.empty())
      return fail(c, FLEET_ERR_ARG, "%s: more than %d picks store a row", what, l->max_store);
    const int32_t out = l->t_free.back();
    l->t_free.pop_back();
    l->k_out[k] = out;
    l->k_mode[k] = 1 | 4;
    if (cur >= 0) {  // Kardam.java:63-65
      l->k_mode[k] |= 2;
      l->k_prev[k] = cur;
      l->k_set[k] = 1;
      l->t_release.push_back(cur);
    }
    l->t_row[w] = out, l->t_epoch[w] = epoch[k];
  }
  return FLEET_OK;
}

// pool_fold with the side outputs: every launch's sums land in d_sums[2 k0 ..)
static int kledger_fold(fleet_kledger* l, const int32_t* picks, int K, const double* dampen, double lr, hipStream_t s,
                        uint8_t* d_merged, float* d_f32) {
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  constexpr int B = fleet::kAccBurst;
  HIP_TRY(c, hipMemsetAsync(p->d_status, 0, sizeof(int) * (size_t)p->slots, s));
  for (int k0 = 0; k0 < K; k0 += B) {
    const int kc = std::min(B, K - k0);
    const fleet::PoolKd kd{lr, l->k_mode.data() + k0, l->k_prev.data() + k0, l->k_out.data() + k0, l->d_slab, l->vpitch,
                           l->rows, l->d_part, l->d_sums + 2 * (size_t)k0};
    HIP_TRY(c, fleet::launch_pool_fold_kd(p->d_rows, p->pitch, picks + k0, p->d_state, k0 == 0, kc, dampen + k0,
                                          k0 + kc == K, (double)1 / K, p->w.launch(), p->d_status, d_merged, d_f32, kd, s));
  }
  HIP_TRY(c, hipMemcpyAsync(p->h_status, p->d_status, sizeof(int) * (size_t)p->slots, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(l->h_sums, l->d_sums, sizeof(double) * 2 * (size_t)K, hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// after the stream was synchronised: the verdict, and on a clean one the commit and the outputs
static int kledger_commit(fleet_kledger* l, const int32_t* picks, int K, double* norm_g, double* norm_diff, uint8_t* set) {
  const int rc = pool_verdict(l->p, picks, K);
  if (rc) return rc;  // the tables, the free list and every row a worker names are as before
  l->row_of.swap(l->t_row), l->epoch_of.swap(l->t_epoch), l->free_rows.swap(l->t_free);
  l->free_rows.insert(l->free_rows.end(), l->t_release.begin(), l->t_release.end());
  for (int k = 0; k < K; ++k) {
    norm_g[k] = (l->k_mode[k] & 1) ? std::sqrt(l->h_sums[2 * k]) : std::nan("");
    norm_diff[k] = (l->k_mode[k] & 2) ? std::sqrt(l->h_sums[2 * k + 1]) : std::nan("");
    set[k] = l->k_set[k];
  }
  return FLEET_OK;
}

}  // namespace

int fleet_kledger_create(fleet_pool* p, int workers, int max_store, fleet_kledger** out) {
  if (!p || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (workers < 1 || max_store < 1) return FLEET_ERR_ARG;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (p->w.gb != 0 || p->w.ng != groups_of(p->w.n) || p->w.ng == 0)
    return fail(c, FLEET_ERR_ARG, "fleet_kledger_create: the pool holds the groups [%zu, %zu) of %zu (the norms are sums over the whole upload)",
                p->w.gb, p->w.ge, groups_of(p->w.n));
  if ((size_t)workers + (size_t)max_store > (size_t)1 << 24)
    return fail(c, FLEET_ERR_ARG, "fleet_kledger_create: %d workers + %d rows", workers, max_store);
  fleet_kledger* l = new fleet_kledger();
  l->p = p;
  l->workers = workers, l->max_store = max_store, l->rows = workers + max_store;
  l->vpitch = (12 * p->w.ng + 15) / 16 * 4;
  l->row_of.assign((size_t)workers, -1);
  l->epoch_of.assign((size_t)workers, 0);
  for (int r = l->rows - 1; r >= 0; --r) l->free_rows.push_back(r);
  const bool ok = l->d_slab.alloc_zero(l->vpitch * (size_t)l->rows) == hipSuccess &&
                  l->d_part.alloc((size_t)fleet::pool_kd_partial_doubles(p->w.launch())) == hipSuccess &&
                  l->d_sums.alloc(2 * (size_t)p->slots) == hipSuccess &&
                  l->h_sums.alloc(2 * (size_t)p->slots) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete l;
    return fail(c, FLEET_ERR_NOMEM, "fleet_kledger_create: allocating %d rows of %zu groups failed", workers + max_store, p->w.ng);
  }
  *out = l;
  return FLEET_OK;
}

void fleet_kledger_destroy(fleet_kledger* l) {
  if (!l) return;
  fleet_ctx* c = l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete l;
}

int fleet_kledger_workers(const fleet_kledger* l) { return l ? l->workers : FLEET_ERR_ARG; }

int fleet_kledger_has(const fleet_kledger* l, int worker) {
  if (!l || worker < 0 || worker >= l->workers) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->p->c->mu);
  return l->row_of[worker] >= 0 ? 1 : 0;
}

int fleet_kledger_epoch(const fleet_kledger* l, int worker, int* epoch) {
  if (!l || !epoch) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->p->c->mu);
  const int rc = kledger_worker_arg(l, worker, "fleet_kledger_epoch");
  if (rc) return rc;
  *epoch = l->epoch_of[worker];
  return FLEET_OK;
}

int fleet_kledger_forget(fleet_kledger* l, int worker) {
  if (!l) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->p->c->mu);
  const int rc = kledger_worker_arg(l, worker, "fleet_kledger_forget");
  if (rc) return rc;
  l->free_rows.push_back(l->row_of[worker]);  // every update synchronised: nothing in flight reads the row
  l->row_of[worker] = -1;
  return FLEET_OK;
}

int fleet_kledger_read(fleet_kledger* l, int worker, float* g, size_t cap) {
  if (!l || !g) return FLEET_ERR_ARG;
  fleet_ctx* c = l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const int rc = kledger_worker_arg(l, worker, "fleet_kledger_read");
  if (rc) return rc;
  const size_t n = l->p->w.n;
  if (cap < n) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu values", cap, n);
  HIP_TRY(c, hipMemcpyAsync(g, l->d_slab + (size_t)l->row_of[worker] * l->vpitch, sizeof(float) * n, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLEET_OK;
}

int fleet_kledger_update(fleet_kledger* l, const int32_t* picks, int K, const double* dampen, const int32_t* worker,
                         const int32_t* epoch, double lr, char* merged, size_t cap, size_t* out_len, float* merged_f32,
                         double* norm_g, double* norm_diff, uint8_t* set) {
  if (!l || !picks || !dampen || !merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set)
    return FLEET_ERR_ARG;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kledger_update: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kledger_update");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kledger_update"))) return rc;
  if (out_len) *out_len = p->w.len;
  if (cap < p->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, p->w.len);
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  uint8_t* d_out = p->d_rows + (size_t)p->slots * p->pitch;  // as fleet_pool_update
  if ((rc = kledger_fold(l, picks, K, dampen, lr, c->stream, d_out, merged_f32 ? p->d_state : nullptr))) return rc;
  if ((rc = window_read_back(c, p->w, d_out, p->d_state, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return kledger_commit(l, picks, K, norm_g, norm_diff, set);
}

int fleet_kledger_update_device(fleet_kledger* l, const int32_t* picks, int K, const double* dampen,
                                const int32_t* worker, const int32_t* epoch, double lr, void* d_merged,
                                void* d_merged_f32, double* norm_g, double* norm_diff, uint8_t* set, void* stream) {
  if (!l || !picks || !dampen || !d_merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set)
    return FLEET_ERR_ARG;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kledger_update_device: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kledger_update_device");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kledger_update_device"))) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if ((rc = kledger_fold(l, picks, K, dampen, lr, s, (uint8_t*)d_merged, (float*)d_merged_f32))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  p->fly.done();
  return kledger_commit(l, picks, K, norm_g, norm_diff, set);
}

// ------------------------------------------------------ Kardam Byzantine filter

// What Kardam.checkByz reads of an update's picks (Kardam.java:136-185; CppNNUpdater.java:
// 488 without its `true ||`), beside a ledger: lastGrad as two fp32 rows in upload
// coordinates (d_lg[lg] is read by the update's kernel, d_lg[lg ^ 1] receives the avg of
// the update's result as lastGrad decodes it, Q(f32(f64(A) / accepted)); the two swap when
// a resolve ends with an average), currModel / lastModel as two rows of a slab (d_m, rows mc and mc ^ 1), and the
// optimistic result of the pending update (d_out, d_f32).
struct FLEET_MEM_LOCAL fleet_kfilter {
  fleet_kledger* l = nullptr;
  size_t n_w = 0, n_b = 0, n_m = 0, mpitch = 0;
  int edges = 0;
  DevBuf<float> d_lg[2];
  int lg = 0;
  bool has_last = false;
  DevBuf<uint8_t> d_out;        // the merged bytes of the pending update
  DevBuf<float> d_f32;          // and their decodeFloat
  DevBuf<double> d_part;        // one launch's per-wave partials (four sums a pick)
  DevBuf<double> d_sums;        // 4 sums per pick of an update
  PinBuf<double> h_sums;
  DevBuf<float> d_m;            // two model rows
  int mc = 0;
  bool has_model = false, has_last_model = false;  // row mc was staged since the last resolve / row mc ^ 1 holds lastModel
  DevBuf<float> d_w, d_b;       // the host form's staging of a model
  DevBuf<double> d_mpart;       // kAccBurst * kMlMaxTiles partials
  DevBuf<double> d_msq;         // {row norm, pair norm}
  PinBuf<double> h_msq;
  // the pending update
  bool pending = false;
  std::vector<int32_t> picks;
  std::vector<double> dampen;
};

namespace {

// kledger_fold through the filter form: the merged bytes and their fp32 go to the filter's
// own rows, the avg to the lastGrad row that is not read, the four sums of every pick to
// d_sums[4 k ..)
static int kfilter_fold(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen, double lr, hipStream_t s) {
  fleet_kledger* l = f->l;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  constexpr int B = fleet::kAccBurst;
  HIP_TRY(c, hipMemsetAsync(p->d_status, 0, sizeof(int) * (size_t)p->slots, s));
  for (int k0 = 0; k0 < K; k0 += B) {
    const int kc = std::min(B, K - k0);
    const fleet::PoolKd kd{lr, l->k_mode.data() + k0, l->k_prev.data() + k0, l->k_out.data() + k0, l->d_slab, l->vpitch,
                           l->rows, f->d_part, f->d_sums + 4 * (size_t)k0};
    HIP_TRY(c, fleet::launch_pool_fold_kf(p->d_rows, p->pitch, picks + k0, p->d_state, k0 == 0, kc, dampen + k0,
                                          k0 + kc == K, (double)1 / K, p->w.launch(), p->d_status, f->d_out, f->d_f32,
                                          kd, f->has_last ? f->d_lg[f->lg] : nullptr, f->d_lg[f->lg ^ 1], s));
  }
  HIP_TRY(c, hipMemcpyAsync(p->h_status, p->d_status, sizeof(int) * (size_t)p->slots, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(f->h_sums, f->d_sums, sizeof(double) * 4 * (size_t)K, hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// after the stream was synchronised: kledger_commit on the first two sums of every pick,
// and on a clean verdict the filter's norms and the pending update
static int kfilter_commit(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen, double* norm_g,
                          double* norm_diff, uint8_t* set, double* norm_p, double* norm_pdiff) {
  fleet_kledger* l = f->l;
  for (int k = 0; k < K; ++k) l->h_sums[2 * k] = f->h_sums[4 * k], l->h_sums[2 * k + 1] = f->h_sums[4 * k + 1];
  const int rc = kledger_commit(l, picks, K, norm_g, norm_diff, set);
  if (rc) return rc;
  for (int k = 0; k < K; ++k) {
    norm_p[k] = std::sqrt(f->h_sums[4 * k + 2]);
    norm_pdiff[k] = f->has_last ? std::sqrt(f->h_sums[4 * k + 3]) : std::nan("");
  }
  f->picks.assign(picks, picks + K);
  f->dampen.assign(dampen, dampen + K);
  f->pending = true;
  return FLEET_OK;
}

// the device outputs of an update or a resolve from the filter's rows, on s
static int kfilter_copy_out(fleet_kfilter* f, void* d_merged, void* d_merged_f32, hipStream_t s) {
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  HIP_TRY(c, hipMemcpyAsync(d_merged, f->d_out, 16 * p->w.ng, hipMemcpyDeviceToDevice, s));
  if (d_merged_f32)
    HIP_TRY(c, hipMemcpyAsync(d_merged_f32, f->d_f32, sizeof(float) * p->w.n, hipMemcpyDeviceToDevice, s));
  return FLEET_OK;
}

// A resolve's checks (FLEET_ERR_ARG with everything untouched) and the count of accepted picks.
static int kfilter_resolve_args(fleet_kfilter* f, const uint8_t* accept, int K, const char* what, int* accepted) {
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  if (!f->pending) return fail(c, FLEET_ERR_ARG, "%s: no update is pending", what);
  if (K != (int)f->picks.size())
    return fail(c, FLEET_ERR_ARG, "%s: %d decisions for the pending update's %zu picks", what, K, f->picks.size());
  for (int k = 0; k < K; ++k)
    if (!p->occupied[f->picks[k]])
      return fail(c, FLEET_ERR_ARG, "%s: pick %d's slot %d holds no upload any more", what, k, f->picks[k]);
  int n = 0;
  for (int k = 0; k < K; ++k) n += accept[k] ? 1 : 0;
  *accepted = n;
  return FLEET_OK;
}

// The refold of a proper subset (CppNNUpdater.java:490-508 over the accepted picks): the
// pool's fold without its finish over the accepted slots in pick order, then the finish
// with the last of all K picks' row, so the header and the unwalked slots are that pick's
// whether it was accepted or not (:508, pickedG). Overwrites the filter's output rows.
static int kfilter_refold(fleet_kfilter* f, const uint8_t* accept, int accepted, hipStream_t s) {
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  constexpr int B = fleet::kAccBurst;
  const int K = (int)f->picks.size();
  std::vector<int32_t> slots;
  std::vector<double> d;
  for (int k = 0; k < K; ++k)
    if (accept[k]) slots.push_back(f->picks[k]), d.push_back(f->dampen[k]);
  HIP_TRY(c, hipMemsetAsync(p->d_status, 0, sizeof(int) * (size_t)p->slots, s));
  for (int k0 = 0; k0 < accepted; k0 += B) {
    const int kc = std::min(B, accepted - k0);
    HIP_TRY(c, fleet::launch_pool_fold(p->d_rows, p->pitch, slots.data() + k0, p->d_state, k0 == 0, kc, d.data() + k0, false,
                                       (double)1 / accepted, p->w.launch(), p->d_status, nullptr, nullptr, s));
  }
  HIP_TRY(c, fleet::launch_acc_finish(p->d_rows + (size_t)f->picks[K - 1] * p->pitch, p->d_state, (double)1 / accepted,
                                      p->w.launch(), f->d_out, f->d_f32, s));
  HIP_TRY(c, fleet::launch_acc_avg_row(p->d_state, (double)1 / accepted, p->w.launch(), f->d_lg[f->lg ^ 1], s));
  HIP_TRY(c, hipMemcpyAsync(p->h_status, p->d_status, sizeof(int) * (size_t)p->slots, hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// a resolve that ended with an average: lastGrad and lastModel advance (CppNNUpdater.java:510-511)
static void kfilter_advance(fleet_kfilter* f) {
  f->lg ^= 1;
  f->has_last = true;
  if (f->has_model) {
    f->mc ^= 1;
    f->has_last_model = true;
  }
}

// currModel from device vectors on s, its norm and the norm of its difference to lastModel
static int kfilter_model_on(fleet_kfilter* f, const float* d_w, const float* d_b, hipStream_t s, double* norm_model,
                            double* norm_model_diff) {
  fleet_ctx* c = f->l->p->c;
  HIP_TRY(c, fleet::launch_mrow_stage(d_w, (int64_t)f->n_w, d_b, (int64_t)f->n_b, f->n_b ? (int64_t)f->edges : 0,
                                      f->d_m + (size_t)f->mc * f->mpitch, f->d_mpart, f->d_msq, s));
  if (f->has_last_model) {
    const int32_t cur = f->mc, prev = f->mc ^ 1;
    HIP_TRY(c, fleet::launch_mrow_pair_norms(f->d_m, f->mpitch, 2, (int64_t)f->n_m, &cur, &prev, 1, f->d_mpart, f->d_msq + 1, s));
  }
  HIP_TRY(c, hipMemcpyAsync(f->h_msq, f->d_msq, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  f->has_model = true;
  *norm_model = std::sqrt(f->h_msq[0]);
  *norm_model_diff = f->has_last_model ? std::sqrt(f->h_msq[1]) : std::nan("");
  return FLEET_OK;
}

}  // namespace

int fleet_kfilter_create(fleet_kledger* l, size_t n_weights, size_t n_biases, int graph_edges, fleet_kfilter** out) {
  if (!l || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (graph_edges < 0) return FLEET_ERR_ARG;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (n_weights >= (size_t)fleet::kMlMaxValues || n_biases >= (size_t)fleet::kMlMaxValues)
    return fail(c, FLEET_ERR_ARG, "fleet_kfilter_create: %zu weights, %zu biases", n_weights, n_biases);
  const size_t n = n_biases * (size_t)graph_edges + n_weights;
  if (n == 0 || n >= (size_t)fleet::kMlMaxValues) return fail(c, FLEET_ERR_ARG, "fleet_kfilter_create: a model of %zu values", n);
  fleet_kfilter* f = new fleet_kfilter();
  f->l = l;
  f->n_w = n_weights, f->n_b = n_biases, f->edges = graph_edges, f->n_m = n;
  f->mpitch = (n + 3) / 4 * 4;
  const size_t lg = 3 * p->w.ng;  // the floats of a state row (Window::state_bytes: and 64 bytes)
  const bool ok =
      f->d_lg[0].alloc_zero(lg, 64) == hipSuccess && f->d_lg[1].alloc_zero(lg, 64) == hipSuccess &&
      f->d_out.alloc_zero(p->w.row_bytes()) == hipSuccess && f->d_f32.alloc_zero(lg, 64) == hipSuccess &&
      f->d_part.alloc((size_t)fleet::pool_kf_partial_doubles(p->w.launch())) == hipSuccess &&
      f->d_sums.alloc(4 * (size_t)p->slots) == hipSuccess && f->h_sums.alloc(4 * (size_t)p->slots) == hipSuccess &&
      f->d_m.alloc_zero(2 * f->mpitch) == hipSuccess && f->d_w.alloc(std::max<size_t>(1, n_weights)) == hipSuccess &&
      f->d_b.alloc(std::max<size_t>(1, n_biases)) == hipSuccess &&
      f->d_mpart.alloc((size_t)fleet::kAccBurst * fleet::kMlMaxTiles) == hipSuccess &&
      f->d_msq.alloc(2) == hipSuccess && f->h_msq.alloc(2) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete f;
    return fail(c, FLEET_ERR_NOMEM, "fleet_kfilter_create: allocating the rows of %zu groups and %zu model values failed", p->w.ng, n);
  }
  *out = f;
  return FLEET_OK;
}

void fleet_kfilter_destroy(fleet_kfilter* f) {
  if (!f) return;
  fleet_ctx* c = f->l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete f;
}

int fleet_kfilter_has_last(const fleet_kfilter* f) {
  if (!f) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(f->l->p->c->mu);
  return f->has_last ? 1 : 0;
}

int fleet_kfilter_set_model(fleet_kfilter* f, const float* weights, const float* biases, double* norm_model,
                            double* norm_model_diff) {
  if (!f || (f->n_w && !weights) || (f->n_b && !biases) || !norm_model || !norm_model_diff) return FLEET_ERR_ARG;
  fleet_ctx* c = f->l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (f->n_w) HIP_TRY(c, hipMemcpyAsync(f->d_w, weights, sizeof(float) * f->n_w, hipMemcpyHostToDevice, c->stream));
  if (f->n_b) HIP_TRY(c, hipMemcpyAsync(f->d_b, biases, sizeof(float) * f->n_b, hipMemcpyHostToDevice, c->stream));
  return kfilter_model_on(f, f->d_w, f->d_b, c->stream, norm_model, norm_model_diff);
}

int fleet_kfilter_set_model_device(fleet_kfilter* f, const float* d_weights, const float* d_biases, double* norm_model,
                                   double* norm_model_diff, void* stream) {
  if (!f || (f->n_w && !d_weights) || (f->n_b && !d_biases) || !norm_model || !norm_model_diff) return FLEET_ERR_ARG;
  fleet_ctx* c = f->l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  return kfilter_model_on(f, d_weights, d_biases, pick(c, stream), norm_model, norm_model_diff);
}

int fleet_kfilter_update(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen, const int32_t* worker,
                         const int32_t* epoch, double lr, char* merged, size_t cap, size_t* out_len, float* merged_f32,
                         double* norm_g, double* norm_diff, uint8_t* set, double* norm_p, double* norm_pdiff) {
  if (!f || !picks || !dampen || !merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set || !norm_p ||
      !norm_pdiff)
    return FLEET_ERR_ARG;
  fleet_kledger* l = f->l;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  f->pending = false;
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kfilter_update: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kfilter_update");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kfilter_update"))) return rc;
  if (out_len) *out_len = p->w.len;
  if (cap < p->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, p->w.len);
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  if ((rc = kfilter_fold(f, picks, K, dampen, lr, c->stream))) return rc;
  if ((rc = window_read_back(c, p->w, f->d_out, f->d_f32, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return kfilter_commit(f, picks, K, dampen, norm_g, norm_diff, set, norm_p, norm_pdiff);
}

int fleet_kfilter_update_device(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen,
                                const int32_t* worker, const int32_t* epoch, double lr, void* d_merged,
                                void* d_merged_f32, double* norm_g, double* norm_diff, uint8_t* set, double* norm_p,
                                double* norm_pdiff, void* stream) {
  if (!f || !picks || !dampen || !d_merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set || !norm_p ||
      !norm_pdiff)
    return FLEET_ERR_ARG;
  fleet_kledger* l = f->l;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  f->pending = false;
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kfilter_update_device: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kfilter_update_device");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kfilter_update_device"))) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if ((rc = kfilter_fold(f, picks, K, dampen, lr, s))) return rc;
  if ((rc = kfilter_copy_out(f, d_merged, d_merged_f32, s))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  p->fly.done();
  return kfilter_commit(f, picks, K, dampen, norm_g, norm_diff, set, norm_p, norm_pdiff);
}

int fleet_kfilter_resolve(fleet_kfilter* f, const uint8_t* accept, int K, char* merged, size_t cap, size_t* out_len,
                          float* merged_f32) {
  if (!f || !accept || !merged || !out_len || K <= 0) return FLEET_ERR_ARG;
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int accepted = 0;
  int rc = kfilter_resolve_args(f, accept, K, "fleet_kfilter_resolve", &accepted);
  if (rc) return rc;
  if (accepted && cap < p->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, p->w.len);
  f->pending = false;
  *out_len = 0;
  if (!accepted) return FLEET_OK;  // no average: lastGrad and lastModel stay (CppNNUpdater.java:506)
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  if (accepted < K && (rc = kfilter_refold(f, accept, accepted, c->stream))) return rc;
  if ((rc = window_read_back(c, p->w, f->d_out, f->d_f32, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (accepted < K && (rc = pool_verdict(p, f->picks.data(), K))) return rc;
  *out_len = p->w.len;
  kfilter_advance(f);
  return FLEET_OK;
}

int fleet_kfilter_resolve_device(fleet_kfilter* f, const uint8_t* accept, int K, void* d_merged, void* d_merged_f32,
                                 size_t* out_len, void* stream) {
  if (!f || !accept || !d_merged || !out_len || K <= 0) return FLEET_ERR_ARG;
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int accepted = 0;
  int rc = kfilter_resolve_args(f, accept, K, "fleet_kfilter_resolve_device", &accepted);
  if (rc) return rc;
  f->pending = false;
  *out_len = 0;
  if (!accepted) return FLEET_OK;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if (accepted < K && (rc = kfilter_refold(f, accept, accepted, s))) return rc;
  if ((rc = kfilter_copy_out(f, d_merged, d_merged_f32, s))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  p->fly.done();
  if (accepted < K && (rc = pool_verdict(p, f->picks.data(), K))) return rc;
  *out_len = p->w.len;
  kfilter_advance(f);
  return FLEET_OK;
}

// --------------------------------------------------------- Kardam model ledger

// Kardam.java's `models` map (worker -> model, Kardam.java:114-125) over a slab of fp32
// rows that belong to model versions (mledger_table.h keeps the tables and resolves an
// update into row pairs; mledger_kernels.hip fills rows and computes the pairs' norms).
struct FLEET_MEM_LOCAL fleet_mledger {
  fleet_ctx* c = nullptr;
  size_t n_w = 0, n_b = 0, n = 0;
  int edges = 0;
  size_t vpitch = 0;            // floats per row: n rounded up to 4
  std::unique_ptr<fleet::MledgerTable> t;
  DevBuf<float> d_slab;
  DevBuf<float> d_w, d_b;          // the host form's staging of one version
  DevBuf<double> d_stage_part;     // kMlMaxTiles partials per row: stages on different streams do not meet
  DevBuf<double> d_row_sq;         // per row: sum (double)(a * a)
  DevBuf<double> d_pair_part;      // one launch of pairs
  DevBuf<double> d_pair_sq;        // an update's pairs; freed on growth
  PinBuf<double> h_sq;             // rows row sums, then the pairs'; freed on growth
  hipEvent_t staged = nullptr;     // orders the context's stream after a stage on a caller's stream
  std::vector<double> pair_norm;
  ~fleet_mledger() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

namespace {

static int mledger_worker_arg(const fleet_mledger* l, int worker, const char* what) {
  if (worker < 0 || worker >= l->t->workers())
    return fail(l->c, FLEET_ERR_ARG, "%s: worker %d outside [0, %d)", what, worker, l->t->workers());
  if (l->t->row_of_worker(worker) < 0) return fail(l->c, FLEET_ERR_ARG, "%s: worker %d holds no model", what, worker);
  return FLEET_OK;
}

// room for an update's P pairs in HBM and pinned memory
static int mledger_pair_room(fleet_mledger* l, size_t P) {
  fleet_ctx* c = l->c;
  const size_t rows = (size_t)l->t->rows();
  if (P > l->d_pair_sq.cap())
    HIP_TRY(c, l->d_pair_sq.grow_exact(std::max<size_t>(2 * P, 4 * (size_t)fleet::kAccBurst)));
  HIP_TRY(c, l->h_sq.grow_exact(rows + l->d_pair_sq.cap()));
  return FLEET_OK;
}

// version `id` from device vectors on stream s; the caller holds the context's mutex
static int mledger_stage_on(fleet_mledger* l, int64_t id, const float* d_w, const float* d_b, hipStream_t s) {
  fleet_ctx* c = l->c;
  bool fresh = false;
  const int row = l->t->stage(id, &fresh);
  if (!fresh) return FLEET_OK;
  const hipError_t e = fleet::launch_mrow_stage(d_w, (int64_t)l->n_w, d_b, (int64_t)l->n_b, l->n_b ? (int64_t)l->edges : 0,
                                                l->d_slab + (size_t)row * l->vpitch,
                                                l->d_stage_part + (size_t)row * fleet::kMlMaxTiles, l->d_row_sq + row, s);
  if (e != hipSuccess) {
    l->t->unstage(id);
    return fail(c, FLEET_ERR_HIP, "launch_mrow_stage: %s", hipGetErrorString(e));
  }
  return FLEET_OK;
}

static int mledger_read_row(fleet_mledger* l, int row, float* params, size_t cap) {
  fleet_ctx* c = l->c;
  if (cap < l->n) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu values", cap, l->n);
  HIP_TRY(c, hipMemcpyAsync(params, l->d_slab + (size_t)row * l->vpitch, sizeof(float) * l->n, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLEET_OK;
}

}  // namespace

int fleet_mledger_create(fleet_ctx* c, size_t n_weights, size_t n_biases, int graph_edges, int workers,
                         int max_versions, fleet_mledger** out) {
  if (!c || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (workers < 1 || max_versions < 1 || graph_edges < 0) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (n_weights >= (size_t)fleet::kMlMaxValues || n_biases >= (size_t)fleet::kMlMaxValues ||
      (size_t)workers + (size_t)max_versions > (size_t)1 << 24)
    return fail(c, FLEET_ERR_ARG, "fleet_mledger_create: %zu weights, %zu biases, %d workers + %d versions", n_weights,
                n_biases, workers, max_versions);
  const size_t n = n_biases * (size_t)graph_edges + n_weights;
  if (n == 0 || n >= (size_t)fleet::kMlMaxValues)
    return fail(c, FLEET_ERR_ARG, "fleet_mledger_create: a model of %zu values", n);
  fleet_mledger* l = new fleet_mledger();
  l->c = c;
  l->n_w = n_weights, l->n_b = n_biases, l->edges = graph_edges, l->n = n;
  l->vpitch = (n + 3) / 4 * 4;
  l->t.reset(new fleet::MledgerTable(workers, max_versions));
  const size_t rows = (size_t)l->t->rows();
  const bool ok =
      l->d_slab.alloc_zero(l->vpitch * rows) == hipSuccess && l->d_w.alloc(std::max<size_t>(1, n_weights)) == hipSuccess &&
      l->d_b.alloc(std::max<size_t>(1, n_biases)) == hipSuccess &&
      l->d_stage_part.alloc(rows * fleet::kMlMaxTiles) == hipSuccess && l->d_row_sq.alloc_zero(rows) == hipSuccess &&
      l->d_pair_part.alloc((size_t)fleet::kAccBurst * fleet::kMlMaxTiles) == hipSuccess &&
      hipEventCreateWithFlags(&l->staged, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete l;
    return fail(c, FLEET_ERR_NOMEM, "fleet_mledger_create: allocating %zu rows of %zu values failed", rows, n);
  }
  *out = l;
  return FLEET_OK;
}

void fleet_mledger_destroy(fleet_mledger* l) {
  if (!l) return;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete l;
}

fleet_ctx* fleet_ctx_of_mledger(const fleet_mledger* l) { return l ? l->c : nullptr; }

int fleet_mledger_shape(const fleet_mledger* l, size_t* n_weights, size_t* n_biases, int* graph_edges, int* workers,
                        int* max_versions) {
  if (!l) return FLEET_ERR_ARG;
  if (n_weights) *n_weights = l->n_w;
  if (n_biases) *n_biases = l->n_b;
  if (graph_edges) *graph_edges = l->edges;
  if (workers) *workers = l->t->workers();
  if (max_versions) *max_versions = l->t->max_versions();
  return FLEET_OK;
}

int fleet_mledger_launch_shape(int* wave, int* block_values, int* max_blocks) {
  if (wave) *wave = 64;
  if (block_values) *block_values = fleet::mrow_block_values();
  if (max_blocks) *max_blocks = fleet::kMlMaxTiles;
  return FLEET_OK;
}

int fleet_mledger_stage(fleet_mledger* l, int64_t id, const float* weights, const float* biases) {
  if (!l || (l->n_w && !weights) || (l->n_b && !biases)) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (l->t->row_of_id(id) >= 0) {  // resident: only its age changes
    bool fresh;
    (void)l->t->stage(id, &fresh);
    return FLEET_OK;
  }
  if (l->n_w) HIP_TRY(c, hipMemcpyAsync(l->d_w, weights, sizeof(float) * l->n_w, hipMemcpyHostToDevice, c->stream));
  if (l->n_b) HIP_TRY(c, hipMemcpyAsync(l->d_b, biases, sizeof(float) * l->n_b, hipMemcpyHostToDevice, c->stream));
  const int rc = mledger_stage_on(l, id, l->d_w, l->d_b, c->stream);
  if (rc) return rc;
  const hipError_t e = hipStreamSynchronize(c->stream);  // the caller's vectors and d_w / d_b are free again
  if (e != hipSuccess) {
    l->t->unstage(id);
    return fail(c, FLEET_ERR_HIP, "fleet_mledger_stage: %s", hipGetErrorString(e));
  }
  return FLEET_OK;
}

int fleet_mledger_stage_device(fleet_mledger* l, int64_t id, const float* d_weights, const float* d_biases,
                               void* stream) {
  if (!l || (l->n_w && !d_weights) || (l->n_b && !d_biases)) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  hipStream_t s = pick(c, stream);
  const bool was = l->t->row_of_id(id) >= 0;
  const int rc = mledger_stage_on(l, id, d_weights, d_biases, s);
  if (rc || was || s == c->stream) return rc;
  HIP_TRY(c, hipEventRecord(l->staged, s));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, l->staged, 0));
  return FLEET_OK;
}

int fleet_mledger_resident(const fleet_mledger* l, int64_t id) {
  if (!l) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  return l->t->row_of_id(id) >= 0 ? 1 : 0;
}

int fleet_mledger_has(const fleet_mledger* l, int worker) {
  if (!l || worker < 0 || worker >= l->t->workers()) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  return l->t->row_of_worker(worker) >= 0 ? 1 : 0;
}

int fleet_mledger_version(const fleet_mledger* l, int worker, int64_t* id) {
  if (!l || !id) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  const int rc = mledger_worker_arg(l, worker, "fleet_mledger_version");
  if (rc) return rc;
  *id = l->t->id_of_row(l->t->row_of_worker(worker));
  return FLEET_OK;
}

int fleet_mledger_forget(fleet_mledger* l, int worker) {
  if (!l) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  const int rc = mledger_worker_arg(l, worker, "fleet_mledger_forget");
  if (rc) return rc;
  (void)l->t->forget(worker);
  return FLEET_OK;
}

int fleet_mledger_read(fleet_mledger* l, int worker, float* params, size_t cap) {
  if (!l || !params) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const int rc = mledger_worker_arg(l, worker, "fleet_mledger_read");
  if (rc) return rc;
  return mledger_read_row(l, l->t->row_of_worker(worker), params, cap);
}

int fleet_mledger_read_version(fleet_mledger* l, int64_t id, float* params, size_t cap) {
  if (!l || !params) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const int row = l->t->row_of_id(id);
  if (row < 0) return fail(c, FLEET_ERR_ARG, "fleet_mledger_read_version: version %lld is not resident", (long long)id);
  return mledger_read_row(l, row, params, cap);
}

int fleet_mledger_update(fleet_mledger* l, const int64_t* id, const int32_t* worker, int K, double* norm_model,
                         double* norm_diff, uint8_t* status) {
  if (!l || K < 0 || !id || !worker || !norm_model || !norm_diff || !status) return FLEET_ERR_ARG;
  if (K == 0) return FLEET_OK;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  fleet::MledgerTable& t = *l->t;
  std::string why;
  if (!t.resolve(id, worker, K, &why)) return fail(c, FLEET_ERR_ARG, "fleet_mledger_update: %s", why.c_str());
  const size_t rows = (size_t)t.rows(), P = t.pair_cur().size();
  if (t.active()) {  // (none: every pick is skipped and nothing is launched or copied)
    int rc = mledger_pair_room(l, P);
    if (rc) return rc;
    constexpr int B = fleet::kAccBurst;
    for (size_t p0 = 0; p0 < P; p0 += B) {
      const int pc = (int)std::min<size_t>(B, P - p0);
      HIP_TRY(c, fleet::launch_mrow_pair_norms(l->d_slab, l->vpitch, (int)rows, (int64_t)l->n, t.pair_cur().data() + p0,
                                               t.pair_prev().data() + p0, pc, l->d_pair_part, l->d_pair_sq + p0,
                                               c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(l->h_sq, l->d_row_sq, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
    if (P)
      HIP_TRY(c, hipMemcpyAsync(l->h_sq + rows, l->d_pair_sq, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  l->pair_norm.resize(P);
  for (size_t i = 0; i < P; ++i) l->pair_norm[i] = std::sqrt(l->h_sq[rows + i]);
  t.replay(l->pair_norm.data(), norm_diff, status);  // Kardam.java:114-125 in pick order; the tables change here
  for (int k = 0; k < K; ++k)
    norm_model[k] = t.pick_row(k) >= 0 ? std::sqrt(l->h_sq[(size_t)t.pick_row(k)]) : std::nan("");
  return FLEET_OK;
}

// fleet_amd/csrc/kernels.h -- internal launchers (fleet_codec.cpp <-> kernels.hip). What an
// update launcher launches is decided in launch_plan.h / launch_plan.cpp (host code only:
// the plan's overrides, plan_update and its two siblings, the kernel names).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "launch_plan.h"

// device error bits (atomicOr into the context's error word, read back by fleet_check)
#define FLEET_ERRBIT_BASE64 1
#define FLEET_ERRBIT_LAYOUT 2
#define FLEET_ERRBIT_ARG 4
#define FLEET_ERRBIT_SYNC 8  // a cross-block hand-off timed out (Kardam reduce blocks)
#define FLEET_ERRBIT_NAN 16  // a client sample's E is NaN (train_class's bail, network.h:1984)

namespace fleet {

// FLEET_MAX_HEADERS of fleet_codec.h (checked there): header positions a kernel may
// hold in LDS
constexpr int kMaxHeaderSlots = 4096;
// segments of descentNative's model step (k_descent): kind 0 = weight block,
// 1 = fully-connected bias block; offsets in floats
constexpr int kMaxDescentSegs = 64;
struct DescentSegs {
  int n;
  int kind[kMaxDescentSegs];
  int64_t grad_off[kMaxDescentSegs], model_off[kMaxDescentSegs], len[kMaxDescentSegs];
};
hipError_t launch_descent(float* weights, float* fc_bias, const float* grad, const DescentSegs& segs, float lr,
                          hipStream_t s);
// the same segments under FLEET_SOLVER_ADAGRAD / _RMSPROP / _ADAM (solver_kernels.hip,
// k_descent_solver<S>): g1, g2 = state rows indexed like the weights (g2: adam only);
// b1_t, b2_t = adam's bias-correction terms (solver_math.h adam_bias_terms)
hipError_t launch_descent_solver(int solver, float* weights, float* g1, float* g2, float* fc_bias, const float* grad,
                                 const DescentSegs& segs, float lr, float b1_t, float b2_t, hipStream_t s);
// self-test digests fn 25..30 of the solvers' arithmetic (solver_kernels.hip)
hipError_t launch_digest_solver(int fn, unsigned long long* out, hipStream_t s);
hipError_t launch_update(const uint8_t* uploads, size_t pitch, int M, const double* d_dampen, double inv_avg,
                         int64_t n_up, int64_t g_begin, int64_t g_end, const int32_t* d_hdr_block,
                         uint8_t* merged, float* merged_f32, int* d_err, hipStream_t s);
// Kardam's side outputs of the fused update (k_update_mixed<256, true>, the tiles, the
// pipelined tiles): per client c and flat value (upload positions that are neither header slots nor past the walk)
//   G = Q(f32(f64(p) lr))            the decoded Kardam.setGrad text (p = stage B)
//   D = Q(G - prev[c])               the decoded g.subtract(prev) text (has_prev[c])
// partials[(c * n_waves + w) * 2 + {0, 1}] = per-wave (or per-tile) sums of (double)(G*G),
// (double)(D*D); g_out (nullable) = G in upload
// coordinates (M rows of vpitch floats; may be prev itself).
// launch_update_kardam: *n_waves = partial slots per client (sizing call: partials
// NULL), norms = M x *norm_parts pairs of sums, added in order on the host;
// *flag_slots = the u32 tile flags the pipelined form needs (kd_flags: zeroed once at
// allocation, kd_epoch: a value new to them, per launch). The plan
// overrides are the caller's one snapshot, passed to the sizing call and the launch
// alike, so a concurrent fleet_set_plan cannot change the grid between the two.
struct KardamOut {
  double lr;
  const float* prev;
  const uint8_t* has_prev;
  size_t vpitch;
  float* g_out;
  double* partials;
};
hipError_t launch_update_kardam(const uint8_t* uploads, size_t pitch, int M, const double* d_dampen, double inv_avg,
                                int64_t n_up, int64_t g_begin, int64_t g_end, const int32_t* d_hdr_block,
                                uint8_t* merged, float* merged_f32, int* d_err, const KardamOut& kd, int* n_waves,
                                double* norms, int* norm_parts, int* flag_slots, uint32_t* kd_flags,
                                uint32_t kd_epoch, const PlanOverrides& o, hipStream_t s,
                                uint32_t kd_wait_skew = 0);
// names of the kernels launch_update / launch_update_encode pick for `groups` groups
std::string update_kernel_name(int64_t groups);
void update_plan_grid(int64_t groups, int* kind, int64_t* blocks, int64_t* n_a, int64_t* n_w, int64_t* n_n);
std::string update_encode_kernel_name(int64_t groups);
hipError_t launch_update_encode(const uint8_t* uploads, size_t pitch, int M, const double* d_dampen, double inv_avg,
                                int64_t n_up, const int32_t* d_hdr_block, uint8_t* merged, float* merged_f32,
                                int* d_err, const float* values, size_t vpitch, uint8_t* enc_out, hipStream_t s);
hipError_t launch_encode_f32(const float* values, int64_t n, size_t vpitch, int rows, uint8_t* out, size_t pitch,
                             hipStream_t s);
// Streaming aggregation (acc_kernels.hip). Every launcher works on a window of an
// upload's groups: rows and state hold the groups [g_begin, g_end) alone (group g at byte
// 16 (g - g_begin), value 3 (g - g_begin)), while merged / merged_f32 are addressed by
// the whole upload's group index, as launch_update's. d_hfirst (n_headers codes) is
// written by a batch's first step and compared by the later ones.
struct AccWindow {
  int64_t n_up, g_begin, g_end;
  const int32_t* d_hdr_block;
  int32_t* d_hfirst;
};
// One upload's step of the chain (st_in is not read when `first`), and the merged
// gradient from the state and the last accepted row.
hipError_t launch_acc_push(const uint8_t* row, const float* st_in, float* st_out, int first, double dampen,
                           const AccWindow& w, int* d_err, hipStream_t s);
hipError_t launch_acc_finish(const uint8_t* last_row, const float* st, double inv, const AccWindow& w, uint8_t* merged,
                             float* merged_f32, hipStream_t s);
// A burst of K <= kAccBurst uploads folded by one launch (k_acc_push_many): rows 0..K-2
// at rows + k * pitch, row K-1 at last_row; dampen holds K factors (host memory: they
// travel in the kernel arguments). `first`: row 0 is the batch's first upload (st_in
// unread, hfirst[] written). st_in may equal st_out. With `finish` the launch ends in
// the finish epilogue (inv = 1 / uploads of the batch) and stores no state.
constexpr int kAccBurst = 64;
hipError_t launch_acc_push_many(const uint8_t* rows, size_t pitch, const uint8_t* last_row, const float* st_in,
                                float* st_out, int first, int K, const double* dampen, bool finish, double inv,
                                const AccWindow& w, int* d_err, uint8_t* merged, float* merged_f32, hipStream_t s);
// The upload pool's fold (k_pool_fold): K <= kAccBurst picked rows of a pool of resident
// uploads, pick k at pool + slots[k] * pitch (pitch a multiple of 16); slots and dampen
// are host arrays of K entries. `first`: pick 0 is the update's first (st unread,
// hfirst[] written); without `finish` the launch stores the running value in st, with it
// the launch ends in the finish epilogue (inv = 1 / picks of the whole update) and
// stores no state. d_status: one error word per slot of the pool.
hipError_t launch_pool_fold(const uint8_t* pool, size_t pitch, const int32_t* slots, float* st, int first, int K,
                            const double* dampen, bool finish, double inv, const AccWindow& w, int* d_status,
                            uint8_t* merged, float* merged_f32, hipStream_t s);
// launch_pool_fold with Kardam's side outputs of the picks (k_pool_fold_kd, then
// k_pool_kd_reduce on the same stream): mode[k] = 1 (G and its squared norm) | 2 (prev[k]:
// D = Q(G - prev) and its squared norm) | 4 (G stored in row out[k]), 0 = the plain step;
// prev / out are rows of `slab` (`rows` rows of vpitch >= 3 groups floats, 16-byte
// aligned), prev[k] possibly the out[j] of an earlier pick. sums[2 k + {0, 1}] receive
// pick k's two sums (0 where the mode computes none); partials holds
// pool_kd_partial_doubles(w) doubles. The window must begin at group 0 (hipErrorInvalidValue
// otherwise, as for a mode or a row that does not fit). All arrays are host arrays of K.
struct PoolKd {
  double lr;
  const uint8_t* mode;
  const int32_t* prev;
  const int32_t* out;
  float* slab;
  size_t vpitch;
  int rows;
  double* partials;
  double* sums;
};
int64_t pool_kd_partial_doubles(const AccWindow& w);
hipError_t launch_pool_fold_kd(const uint8_t* pool, size_t pitch, const int32_t* slots, float* st, int first, int K,
                               const double* dampen, bool finish, double inv, const AccWindow& w, int* d_status,
                               uint8_t* merged, float* merged_f32, const PoolKd& kd, hipStream_t s);
// launch_pool_fold_kd's filter form (k_pool_fold_kf, then k_pool_kf_reduce): beside the
// ledger's sums, per pick the squared norm of its dampened value p over the flat slots and,
// with `lastg` (one fp32 row of >= 3 groups floats in upload coordinates; nullptr: none),
// that of Q(p - lastg), whatever the pick's mode. With `finish` the launch also leaves the
// update's avg, Q(f32(f64(A) * inv)) per slot -- what the next update's lastGrad decodes to,
// which decodeFloat(merged) is not where Q is not idempotent --, in avg_out (another row).
// launch_acc_avg_row gives the same row from a state that a fold without finish left. sums[4 k + {0, 1, 2, 3}] = pick k's sg,
// sd, sp, se, the first two bit for bit launch_pool_fold_kd's; partials holds
// pool_kf_partial_doubles(w) doubles.
int64_t pool_kf_partial_doubles(const AccWindow& w);
hipError_t launch_pool_fold_kf(const uint8_t* pool, size_t pitch, const int32_t* slots, float* st, int first, int K,
                               const double* dampen, bool finish, double inv, const AccWindow& w, int* d_status,
                               uint8_t* merged, float* merged_f32, const PoolKd& kd, const float* lastg,
                               float* avg_out, hipStream_t s);
hipError_t launch_acc_avg_row(const float* st, double inv, const AccWindow& w, float* avg_out, hipStream_t s);
// The arrival gate's pass (k_pool_vet, then k_pool_vet_reduce on the same stream) over K <=
// kAccBurst rows of a pool (slots: a host array of K), folding nothing: per slot k
// out_status[k] = FLEET_ERRBIT_BASE64 where the row is not Base64::encode output (the
// fold's verdict) | FLEET_ERRBIT_LAYOUT where a header slot's code differs from d_expected
// (the window's n_headers codes by header index; nullptr: not checked), out_sumsq[k] = sum
// (double)(y * y) and out_max[k] = max |y| over the window's flat slots, y = Q(dec(code)).
// d_work_status (kAccBurst words) and partials (pool_vet_partial_doubles(w) doubles) are
// the launch's own; the three outputs are device arrays of K. The pool's rows, state,
// hfirst[] and status are not written.
int64_t pool_vet_partial_doubles(const AccWindow& w);
hipError_t launch_pool_vet(const uint8_t* pool, size_t pitch, const int32_t* slots, int K, const AccWindow& w,
                           const int32_t* d_expected, int* d_work_status, double* partials, int32_t* out_status,
                           double* out_sumsq, float* out_max, hipStream_t s);
// The Kardam model ledger (mledger_kernels.hip). A model version is one fp32 row of
// 4 * ceil(n / 4) floats, n = n_b * reps + n_w < kMlMaxValues values in getModelParams'
// order, row[i] = Q(param(i)), the padding 0. A row or a pair runs on mrow_tiles(n) <=
// kMlMaxTiles blocks of mrow_block_values() values a pass, and `partials` holds one double
// per block: mrow_tiles(n) for a stage, kAccBurst * kMlMaxTiles for a launch of pairs.
// launch_mrow_stage: the row, and *norm_sq = sum (double)(row[i]^2) (k_mrow_stage, then
// k_mrow_reduce on the same stream). launch_mrow_pair_norms: P <= kAccBurst ordered pairs
// of rows of `slab` (`rows` rows of vpitch floats, 16-byte aligned; cur / prev are host
// arrays), sums[p] = sum (double)(D^2), D = Q(cur[i] - prev[i]) (k_mrow_pair_norms, then
// k_mrow_reduce). hipErrorInvalidValue for a row outside the slab or a size that does not fit.
constexpr int kMlMaxTiles = 64;
constexpr int64_t kMlMaxValues = ((int64_t)1 << 31) - 4096;
int mrow_block_values();
int mrow_tiles(int64_t n);
hipError_t launch_mrow_stage(const float* weights, int64_t n_w, const float* biases, int64_t n_b, int64_t reps,
                             float* row, double* partials, double* norm_sq, hipStream_t s);
hipError_t launch_mrow_pair_norms(const float* slab, size_t vpitch, int rows, int64_t n, const int32_t* cur,
                                  const int32_t* prev, int P, double* partials, double* sums, hipStream_t s);
hipError_t launch_encode_minibatch(const float* images, int64_t n_images, int F, const int32_t* labels,
                                   const int32_t* idx, int B, const float* teacher, int NL, const float header[7],
                                   uint8_t* out, int* err, hipStream_t s);
// the sampler's mode-1 teacher forward (teacher.hip): probs[b*10 + j] for sample
// idx[b] (idx == nullptr: sample b) of the n_images x F rows
hipError_t launch_teacher_forward(const float* w, const float* b, const float* images, int64_t n_images, int F,
                                  const int32_t* idx, int B, float temperature, float* probs, int* err,
                                  hipStream_t s);
int64_t teacher_weight_count();
int64_t teacher_bias_count();
// the Driver's test() (eval_kernels.hip): k_eval_forward over images idx[0..B) (idx == nullptr:
// images 0..B-1) of the n_images x F rows, then k_eval_reduce. pred[B], cost[B] and
// result (float error, float accuracy, int32 correct) are written; prob[B] and
// probs10[B][10] when not nullptr. hipErrorInvalidValue for B <= 0, F < 784 or a missing
// pred / cost / result.
hipError_t launch_eval(const float* w, const float* b, const float* images, int64_t n_images, int F,
                       const int32_t* labels, const int32_t* idx, int B, int32_t* pred, float* prob, float* cost,
                       float* probs10, float* result, int* err, hipStream_t s);
int eval_block_images();
int eval_set_grid(int max_blocks);  // 0: three blocks per CU; returns the previous value
// the Driver's test() on the reference's CIFAR network (cifar_kernels.hip), classes 10 or 100:
// k_cifar_forward over images idx[0..B) (idx == nullptr: images 0..B-1) of the n_images x F rows,
// then k_eval_reduce. pred[B], cost[B] and result (float error, float accuracy, int32 correct)
// are written; prob[B] and probsN[B][classes] when not nullptr. hipErrorInvalidValue for other
// classes, B <= 0, F < 3072 or a missing pred / cost / result.
hipError_t launch_cifar_test(int classes, const float* w, const float* b, const float* images, int64_t n_images, int F,
                             const int32_t* labels, const int32_t* idx, int B, int32_t* pred, float* prob, float* cost,
                             float* probsN, float* result, int* err, hipStream_t s);
int cifar_block_images();
int cifar_set_grid(int max_blocks);  // 0: one block per CU; returns the previous value
// the client's getGradients (client_kernels.hip): per client c of C its gradients() vector over
// samples idx[c*B + k] (idx == nullptr: images c*B + k) under shift[c*B + k] = {dx, dy} (nullptr:
// none) on model row model_of_client[c] (nullptr: row 0) of models (rows of model_pitch floats,
// w then b), into grads (rows of grad_pitch floats), `chunk` clients at a time. workspace:
// client_grad_workspace_bytes(chunk, B).
hipError_t launch_client_grads(const float* models, int64_t model_pitch, int n_models, const int32_t* model_of_client,
                               const float* images, int64_t n_images, int F, const int32_t* labels, const int32_t* idx,
                               const int32_t* shift, int C, int B, int chunk, float temperature, float* workspace,
                               float* grads, int64_t grad_pitch, int* err, hipStream_t s);
// the same with a cost (0 cross_entropy, 1 distillation) and, where d_clip is given, DPgradients
// for the clients with sigma > 0: d_clip, d_sigma [C] on the device, dp_of_client [C] on the host
// (non-zero: sigma > 0), d_z the 22961 draws of client_dp_noise, scale:
// client_grad_scale_bytes(chunk, B) on the device
hipError_t launch_client_grads_ex(const float* models, int64_t model_pitch, int n_models,
                                  const int32_t* model_of_client, const float* images, int64_t n_images, int F,
                                  const int32_t* labels, const int32_t* idx, const int32_t* shift, int C, int B,
                                  int chunk, float temperature, int cost, const float* d_clip, const float* d_sigma,
                                  const uint8_t* dp_of_client, const double* d_z, float* scale, float* workspace,
                                  float* grads, int64_t grad_pitch, int* err, hipStream_t s);
size_t client_grad_scale_bytes(int chunk, int B);
void client_dp_noise(double* out, size_t n);  // host: the standard-normal draws of addGaussian
int64_t client_grad_len();  // 22961
size_t client_grad_workspace_bytes(int chunk, int B);
int client_grad_chunk(int C, int B);
int client_grad_set_chunk(int max_clients);  // 0: what fits the workspace cap; returns the previous value
hipError_t launch_encode_model_params(const float* weights, int64_t n_w, const float* biases, int64_t n_b, int64_t reps,
                                      uint8_t* out, hipStream_t s);
hipError_t launch_encode_i32(const int32_t* codes, int64_t n, uint8_t* out, hipStream_t s);
hipError_t launch_decode(const uint8_t* text, int64_t n, size_t pitch, int rows, void* out, size_t vpitch,
                         int as_codes, int* d_err, hipStream_t s);
hipError_t launch_elementwise(const uint8_t* a, const uint8_t* b, int op, double scale, int64_t n, uint8_t* out,
                              int* d_err, hipStream_t s);
hipError_t launch_norm_partials(const uint8_t* a, int64_t n, double* partials, int* nblocks, int* d_err,
                                hipStream_t s);
hipError_t launch_kardam_grads(const uint8_t* uploads, size_t pitch, int M, const int32_t* d_hdr, int n_hdr,
                               int64_t n_flat, const double* d_dampen, double lr, const uint8_t* prev,
                               size_t prev_pitch, const uint8_t* d_has_prev, uint8_t* g_out, size_t g_pitch,
                               double* partials, int* nblocks, int* d_err, hipStream_t s);
hipError_t launch_flat(const uint8_t* up, const int32_t* d_hdr, int n_hdr, int64_t n_flat, uint8_t* out,
                       int* d_err, hipStream_t s);
hipError_t launch_merge(const uint8_t* up, const uint8_t* flat, const int32_t* d_hdr, int n_hdr, int64_t walk_end,
                        int64_t n_up, uint8_t* out, int* d_err, hipStream_t s);
hipError_t launch_layout_parse(const uint8_t* up, int64_t n, int cap, int32_t* out, hipStream_t s);
hipError_t launch_synth(uint64_t seed, int client0, int64_t elem0, int rows, int64_t n_up, float* out, size_t vpitch,
                        const int32_t* d_hpos, const float* d_hval, int n_hdr, hipStream_t s);
hipError_t launch_digest(int fn, unsigned long long* out, hipStream_t s);
#ifdef FLEET_TRACE
hipError_t set_trace_buffer(void* p);  // dev builds: the tile kernels' phase trace (FLEET_WTRACE)
#endif
}  // namespace fleet

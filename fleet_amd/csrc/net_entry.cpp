// fleet_amd/csrc/net_entry.cpp -- the model and network entry points of the C-ABI: the mode-1
// model codec and values text, model parameters, minibatch, teacher, evaluation and client
// gradients (both networks), the descent and solver epilogues, fleet_model_version.
#include <cmath>
#include <cstring>

#include "host_ctx.h"
#include "cifar_forward.h"
#include "kernels.h"
#include "model_codec.h"
#include "solver_host.h"
#include "solver_math.h"

using namespace fleet::host;

// ------------------------------------------------- mode-1 model codec

namespace {

static int model_total(fleet_ctx* c, const int32_t* dims, int n_mats, size_t* n) {
  if (n_mats < 0 || (n_mats && !dims)) return fail(c, FLEET_ERR_ARG, "bad dims");
  size_t t = 0;
  for (int j = 0; j < n_mats; ++j) {
    if (dims[3 * j] < 0 || dims[3 * j + 1] < 0 || dims[3 * j + 2] < 0) return fail(c, FLEET_ERR_ARG, "negative dim");
    t += (size_t)dims[3 * j] * dims[3 * j + 1] * dims[3 * j + 2];
  }
  if (t > (size_t)INT32_MAX) return fail(c, FLEET_ERR_ARG, "model too large for int32 indices");
  *n = t;
  return FLEET_OK;
}

// quantize + dictionary on the device; leaves d_index and the dictionary on the host
static int model_run(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats, size_t n, float* quantized,
              std::vector<float>* dict_host, int32_t* U, DevBuf<int32_t>* d_index_keep) {
  DevBuf<float> dw, dq, dd;
  if (n) {
    HIP_TRY(c, dw.alloc(n));
    HIP_TRY(c, dq.alloc(n));
    HIP_TRY(c, dd.alloc(n));
    HIP_TRY(c, d_index_keep->alloc(n));
    HIP_TRY(c, hipMemcpyAsync(dw, weights, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, fleet::model_quantize_index(dw, dims, n_mats, dq, dd, *d_index_keep, U, c->stream));
  if (quantized && n) HIP_TRY(c, hipMemcpyAsync(quantized, dq, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  dict_host->resize((size_t)*U);
  if (*U) HIP_TRY(c, hipMemcpyAsync(dict_host->data(), dd, (size_t)*U * sizeof(float), hipMemcpyDeviceToHost,
                                    c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLEET_OK;
}

}  // namespace

int fleet_model_quantize_index(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats,
                               float* quantized, float* dict, int* n_dict, int32_t* index) {
  if (!c) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && !weights) return FLEET_ERR_ARG;
  std::vector<float> dh;
  int32_t U = 0;
  DevBuf<int32_t> di;
  if ((rc = model_run(c, weights, dims, n_mats, n, quantized, &dh, &U, &di))) return rc;
  if (dict && U) std::memcpy(dict, dh.data(), sizeof(float) * (size_t)U);
  if (n_dict) *n_dict = U;
  if (index && n) {
    HIP_TRY(c, hipMemcpy(index, di, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return FLEET_OK;
}

int fleet_model_weights_text(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats, char* out,
                             size_t cap, size_t* out_len) {
  if (!c) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && !weights) return FLEET_ERR_ARG;
  std::vector<float> dh;
  int32_t U = 0;
  DevBuf<int32_t> di;
  if ((rc = model_run(c, weights, dims, n_mats, n, nullptr, &dh, &U, &di))) return rc;
  // header and dictionary lines: `ostream << int` / `ostream << float` (precision 6 == %g),
  // U lines of host formatting; the n index tokens are formatted on the device
  std::string head;
  char buf[64];
  snprintf(buf, sizeof buf, "%zu\n%d\n", n, U);
  head += buf;
  for (int32_t k = 0; k < U; ++k) {
    snprintf(buf, sizeof buf, "%d\n%g\n", k, (double)dh[(size_t)k]);
    head += buf;
  }
  std::vector<char> body;
  HIP_TRY(c, fleet::model_index_text(di, dims, n_mats, &body, c->stream));
  const size_t total = head.size() + body.size();
  if (out_len) *out_len = total;
  if (cap < total) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, total);
  std::memcpy(out, head.data(), head.size());
  if (!body.empty()) std::memcpy(out + head.size(), body.data(), body.size());
  return FLEET_OK;
}

namespace {

// the block offsets of fleet_values_text's sizes; empty for the pairs form
static int values_offsets(fleet_ctx* c, size_t n, const int64_t* block_sizes, int n_blocks, std::vector<int64_t>* off) {
  if (n_blocks < 0 || (n_blocks && !block_sizes)) return fail(c, FLEET_ERR_ARG, "values text: bad blocks");
  if (n > (size_t)INT32_MAX) return fail(c, FLEET_ERR_ARG, "values text: %zu values (the limit is 2^31 - 1)", n);
  off->assign((size_t)n_blocks + 1, 0);
  for (int j = 0; j < n_blocks; ++j) {
    if (block_sizes[j] < 0) return fail(c, FLEET_ERR_ARG, "values text: negative block size");
    (*off)[(size_t)j + 1] = (*off)[(size_t)j] + block_sizes[j];
  }
  if (n_blocks && (size_t)off->back() != n)
    return fail(c, FLEET_ERR_ARG, "values text: the blocks hold %lld values, not %zu", (long long)off->back(), n);
  return FLEET_OK;
}

static int values_text_out(fleet_ctx* c, const float* d_values, size_t n, const std::vector<int64_t>& off,
                           int n_blocks, char* out, size_t cap, size_t* out_len, hipStream_t s) {
  std::vector<char> text;
  const hipError_t e = fleet::model_values_text(d_values, (int64_t)n, off.data(), n_blocks, &text, s);
  if (e == hipErrorInvalidValue)
    return fail(c, FLEET_ERR_ARG, "values text: more than 254 empty blocks in a row");
  HIP_TRY(c, e);
  if (out_len) *out_len = text.size();
  if (!out || cap < text.size()) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, text.size());
  if (!text.empty()) std::memcpy(out, text.data(), text.size());
  return FLEET_OK;
}

}  // namespace

int fleet_values_text_device(fleet_ctx* c, const void* d_values, size_t n, const int64_t* block_sizes, int n_blocks,
                             char* out, size_t cap, size_t* out_len, void* stream) {
  if (!c || (n && !d_values)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<int64_t> off;
  int rc = values_offsets(c, n, block_sizes, n_blocks, &off);
  if (rc) return rc;
  DEVICE_SCOPE(c);
  return values_text_out(c, (const float*)d_values, n, off, n_blocks, out, cap, out_len, pick(c, stream));
}

int fleet_values_text(fleet_ctx* c, const float* values, size_t n, const int64_t* block_sizes, int n_blocks, char* out,
                      size_t cap, size_t* out_len) {
  if (!c || (n && !values)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<int64_t> off;
  int rc = values_offsets(c, n, block_sizes, n_blocks, &off);
  if (rc) return rc;
  DEVICE_SCOPE(c);
  DevBuf<float> dv;
  if (n) {
    HIP_TRY(c, dv.alloc(n));
    HIP_TRY(c, hipMemcpyAsync(dv, values, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  return values_text_out(c, dv, n, off, n_blocks, out, cap, out_len, c->stream);
}

int fleet_model_read_weights(fleet_ctx* c, const char* text, size_t len, const int32_t* dims, int n_mats,
                             float* weights_out) {
  if (!c || (!text && len)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && !weights_out) return FLEET_ERR_ARG;
  // header: loop_counter and U lines (getcleanline + atoi), then U pairs read
  // with `>>` (int, float = strtof); the std::map keeps the first value of a key
  std::string t(text, len);
  const char* p = t.c_str();
  char* e = nullptr;
  (void)strtol(p, &e, 10);
  if (e == p) return fail(c, FLEET_ERR_ARG, "weights section: no loop counter");
  p = e;
  const long U = strtol(p, &e, 10);
  if (e == p || U < 0) return fail(c, FLEET_ERR_ARG, "weights section: no dictionary size");
  p = e;
  std::vector<std::pair<int32_t, float>> kv;
  kv.reserve((size_t)U);
  for (long k = 0; k < U; ++k) {
    const long key = strtol(p, &e, 10);
    if (e == p) return fail(c, FLEET_ERR_ARG, "weights section: bad dictionary index %ld", k);
    p = e;
    const float v = strtof(p, &e);
    if (e == p) return fail(c, FLEET_ERR_ARG, "weights section: bad dictionary value %ld", k);
    p = e;
    kv.emplace_back((int32_t)key, v);
  }
  std::stable_sort(kv.begin(), kv.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  std::vector<int32_t> keys;
  std::vector<float> vals;
  for (size_t k = 0; k < kv.size(); ++k)
    if (k == 0 || kv[k].first != kv[k - 1].first) keys.push_back(kv[k].first), vals.push_back(kv[k].second);
  const size_t body = (size_t)(p - t.c_str());
  const size_t blen = len - body;
  DevBuf<uint8_t> dt;
  DevBuf<int32_t> dk;
  DevBuf<float> dv, dw;
  if (blen) HIP_TRY(c, dt.alloc(blen));
  HIP_TRY(c, dk.alloc(keys.size() + 1));
  HIP_TRY(c, dv.alloc(vals.size() + 1));
  if (n) HIP_TRY(c, dw.alloc(n));
  if (blen) HIP_TRY(c, hipMemcpyAsync(dt, text + body, blen, hipMemcpyHostToDevice, c->stream));
  if (!keys.empty()) {
    HIP_TRY(c, hipMemcpyAsync(dk, keys.data(), sizeof(int32_t) * keys.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dv, vals.data(), sizeof(float) * vals.size(), hipMemcpyHostToDevice, c->stream));
  }
  int status = 0;
  HIP_TRY(c, fleet::model_read_index(dt, (int64_t)blen, (int64_t)n, dk, dv, (int32_t)keys.size(), dw, &status,
                                     c->stream));
  if (status == 1) return fail(c, FLEET_ERR_ARG, "weights section: malformed index token");
  if (status == 2) return fail(c, FLEET_ERR_LAYOUT, "weights section: index count differs from the model size");
  if (n) HIP_TRY(c, hipMemcpy(weights_out, dw, sizeof(float) * n, hipMemcpyDeviceToHost));
  return FLEET_OK;
}

// ------------------------------------------ model parameters (getModelParametersNative)

int fleet_model_params_device(fleet_ctx* c, const float* d_weights, size_t n_weights, const float* d_biases,
                              size_t n_biases, int graph_edges, void* d_out, void* stream) {
  if (!c || !d_out || graph_edges < 0 || (n_weights && !d_weights) || (n_biases && graph_edges && !d_biases))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  HIP_TRY(c, fleet::launch_encode_model_params(d_weights, (int64_t)n_weights, d_biases, (int64_t)n_biases,
                                               n_biases ? (int64_t)graph_edges : 0, (uint8_t*)d_out,
                                               pick(c, stream)));
  return FLEET_OK;
}

size_t fleet_minibatch_len(int F, int B, int num_labels, int with_teacher) {
  if (F < 0 || B < 0 || num_labels < 0) return 0;
  const size_t n = 7 + (size_t)B * ((size_t)F + (with_teacher ? (size_t)num_labels : 0) + 1) + (with_teacher ? 1 : 0);
  return fleet_b64_len(n);
}

int fleet_minibatch_device(fleet_ctx* c, const void* d_images, size_t n_images, int F, const void* d_labels,
                           const void* d_idx, int B, const void* d_teacher, int num_labels, const float header[7],
                           void* d_out, void* stream) {
  if (!c || !d_out || !header || F < 0 || B < 0 || num_labels < 0 || (B && (!d_idx || !d_labels || !d_images)) ||
      (d_teacher && num_labels == 0))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  HIP_TRY(c, fleet::launch_encode_minibatch((const float*)d_images, (int64_t)n_images, F, (const int32_t*)d_labels,
                                            (const int32_t*)d_idx, B, (const float*)d_teacher, num_labels, header,
                                            (uint8_t*)d_out, c->d_dev_err, pick(c, stream)));
  return FLEET_OK;
}

int fleet_minibatch(fleet_ctx* c, const float* images, size_t n_images, int F, const int32_t* labels,
                    const int32_t* idx, int B, const float* teacher, int num_labels, const float header[7],
                    char* out, size_t cap, size_t* out_len) {
  if (!c || !header || F < 0 || B < 0 || num_labels < 0 || (B && (!idx || !labels || !images)) ||
      (teacher && num_labels == 0))
    return FLEET_ERR_ARG;
  const size_t len = fleet_minibatch_len(F, B, num_labels, teacher != nullptr);
  if (out_len) *out_len = len;
  if (cap < len || !out) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, len);
  for (int b = 0; b < B; ++b)
    if (idx[b] < 0 || (size_t)idx[b] >= n_images)
      return fail(c, FLEET_ERR_ARG, "sample %d: index %d outside the %zu images", b, idx[b], n_images);
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  // staging: [B x F features | B labels | 0..B-1 | B x NL teacher]; the device gathers nothing
  const size_t nl = teacher ? (size_t)num_labels : 0;
  const size_t o_lab = round16(sizeof(float) * (size_t)B * (size_t)F), o_idx = o_lab + round16(4 * (size_t)B);
  const size_t o_tea = o_idx + round16(4 * (size_t)B), o_out = o_tea + round16(sizeof(float) * (size_t)B * nl);
  const size_t o_end = o_out + round16(len) + 16;
  int rc;
  if ((rc = grow_pinned(c, o_end))) return rc;
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // staging buffer reuse
  uint8_t* h = c->h_stage;
  for (int b = 0; b < B; ++b) {
    std::memcpy(h + sizeof(float) * (size_t)b * F, images + (size_t)idx[b] * F, sizeof(float) * (size_t)F);
    reinterpret_cast<int32_t*>(h + o_lab)[b] = labels[idx[b]];
    reinterpret_cast<int32_t*>(h + o_idx)[b] = b;
  }
  if (teacher) std::memcpy(h + o_tea, teacher, sizeof(float) * (size_t)B * nl);
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fleet::launch_encode_minibatch((const float*)d, (int64_t)B, F, (const int32_t*)(d + o_lab),
                                            (const int32_t*)(d + o_idx), B, teacher ? (const float*)(d + o_tea) : nullptr,
                                            num_labels, header, d + o_out, c->d_err, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + o_out, d + o_out, len, hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  std::memcpy(out, h + o_out, len);
  return FLEET_OK;
}

size_t fleet_teacher_weight_count(void) { return (size_t)fleet::teacher_weight_count(); }
size_t fleet_teacher_bias_count(void) { return (size_t)fleet::teacher_bias_count(); }

namespace {
// a host form's model arrays against the network's counts; `who`: the entry point's message prefix
int check_model_counts(fleet_ctx* c, const char* who, size_t n_w, size_t n_b, size_t want_w, size_t want_b) {
  if (n_w == want_w && n_b == want_b) return FLEET_OK;
  return fail(c, FLEET_ERR_ARG, "%s: %zu weights and %zu biases, expected %zu and %zu", who, n_w, n_b, want_w, want_b);
}
}  // namespace

int fleet_teacher_forward_device(fleet_ctx* c, const void* d_w, const void* d_b, const void* d_images, size_t n_images,
                                 int F, const void* d_idx, int B, float temperature, void* d_probs, void* stream) {
  if (!c || B < 0 || (B && (!d_w || !d_b || !d_images || !d_probs)) || F < 28 * 28) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  HIP_TRY(c, fleet::launch_teacher_forward((const float*)d_w, (const float*)d_b, (const float*)d_images,
                                           (int64_t)n_images, F, (const int32_t*)d_idx, B, temperature,
                                           (float*)d_probs, c->d_dev_err, pick(c, stream)));
  return FLEET_OK;
}

int fleet_teacher_forward(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                          size_t n_images, int F, const int32_t* idx, int B, float temperature, float* probs) {
  if (!c || B < 0 || F < 28 * 28 || (B && (!w || !b || !images || !idx || !probs))) return FLEET_ERR_ARG;
  int rc = check_model_counts(c, "teacher", n_w, n_b, fleet_teacher_weight_count(), fleet_teacher_bias_count());
  if (rc) return rc;
  for (int i = 0; i < B; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return fail(c, FLEET_ERR_ARG, "sample %d: index %d outside the %zu images", i, idx[i], n_images);
  if (B == 0) return FLEET_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  // staging: [w | b | B gathered rows | B x 10 probs]
  const size_t o_b = round16(sizeof(float) * n_w), o_x = o_b + round16(sizeof(float) * n_b);
  const size_t o_p = o_x + round16(sizeof(float) * (size_t)B * (size_t)F);
  const size_t o_end = o_p + round16(sizeof(float) * (size_t)B * 10);
  if ((rc = grow_pinned(c, o_end))) return rc;
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // staging buffer reuse
  uint8_t* h = c->h_stage;
  std::memcpy(h, w, sizeof(float) * n_w);
  std::memcpy(h + o_b, b, sizeof(float) * n_b);
  for (int i = 0; i < B; ++i)
    std::memcpy(h + o_x + sizeof(float) * (size_t)i * F, images + (size_t)idx[i] * F, sizeof(float) * (size_t)F);
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, h, o_p, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fleet::launch_teacher_forward((const float*)d, (const float*)(d + o_b), (const float*)(d + o_x), B, F,
                                           nullptr, B, temperature, (float*)(d + o_p), c->d_err, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + o_p, d + o_p, sizeof(float) * (size_t)B * 10, hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  std::memcpy(probs, h + o_p, sizeof(float) * (size_t)B * 10);
  return FLEET_OK;
}

size_t fleet_evaluate_block_images(void) { return (size_t)fleet::eval_block_images(); }
int fleet_evaluate_set_grid(int max_blocks) { return fleet::eval_set_grid(max_blocks); }

namespace {

// Both _device evaluations: where the costs and predictions go that the caller does not take,
// [B floats | B int32] of the context's d_eval (its rule is at the member).
int eval_untaken(fleet_ctx* c, int B, void* d_cost, void* d_pred, float** cost, int32_t** pred) {
  if (!d_cost || !d_pred) {
    const hipError_t e = c->d_eval.grow_exact(8 * (size_t)B, 64, &c->retired);
    if (e != hipSuccess) return nomem(c, "hipMalloc", 8 * (size_t)B, e);
  }
  *cost = d_cost ? (float*)d_cost : (float*)c->d_eval.get();
  *pred = d_pred ? (int32_t*)d_pred : (int32_t*)(c->d_eval + c->d_eval.cap() / 2);  // behind the costs
  return FLEET_OK;
}

// what evaluate_host hands the network's launch: the workspace's device pointers
struct EvalArgs {
  const float *w, *b, *images;
  int64_t rows;
  const int32_t *labels, *idx;
  int32_t* pred;
  float *prob, *cost, *probsN, *result;
};

// fleet_evaluate and fleet_cifar_test behind their own early checks: the count, pick and index
// checks under `who`'s prefix, the workspace, the copies in, the network's launch on the
// context's stream (launch(EvalArgs), returning a FLEET code) and the copies out.
// n_probs: probsN's floats per image.
template <typename Launch>
int evaluate_host(fleet_ctx* c, const char* who, const float* w, size_t n_w, size_t want_w, const float* b, size_t n_b,
                  size_t want_b, const float* images, size_t n_images, int F, const int32_t* labels, const int32_t* idx,
                  int B, float* error, float* accuracy, int32_t* correct, int32_t* pred, float* prob, float* cost,
                  float* probsN, size_t n_probs, Launch launch) {
  int rc = check_model_counts(c, who, n_w, n_b, want_w, want_b);
  if (rc) return rc;
  if (!idx && (size_t)B > n_images) return fail(c, FLEET_ERR_ARG, "%s: %d images asked of %zu", who, B, n_images);
  for (int i = 0; idx && i < B; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return fail(c, FLEET_ERR_ARG, "image %d: index %d outside the %zu images", i, idx[i], n_images);
  // the images the evaluation reads: all of them with idx, the first B without
  const size_t rows = idx ? n_images : (size_t)B, nB = (size_t)B;
  const size_t o_b = round16(sizeof(float) * n_w), o_x = o_b + round16(sizeof(float) * n_b);
  const size_t o_l = o_x + round16(sizeof(float) * rows * (size_t)F), o_i = o_l + round16(4 * rows);
  const size_t o_pred = o_i + round16(4 * nB), o_prob = o_pred + round16(4 * nB), o_cost = o_prob + round16(4 * nB);
  const size_t o_pn = o_cost + round16(4 * nB), o_res = o_pn + (probsN ? round16(4 * nB * n_probs) : 0);
  const size_t o_end = o_res + 16;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, w, sizeof(float) * n_w, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_b, b, sizeof(float) * n_b, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_x, images, sizeof(float) * rows * (size_t)F, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_l, labels, 4 * rows, hipMemcpyHostToDevice, c->stream));
  if (idx) HIP_TRY(c, hipMemcpyAsync(d + o_i, idx, 4 * nB, hipMemcpyHostToDevice, c->stream));
  if ((rc = launch(EvalArgs{(const float*)d, (const float*)(d + o_b), (const float*)(d + o_x), (int64_t)rows,
                            (const int32_t*)(d + o_l), idx ? (const int32_t*)(d + o_i) : nullptr,
                            (int32_t*)(d + o_pred), (float*)(d + o_prob), (float*)(d + o_cost),
                            probsN ? (float*)(d + o_pn) : nullptr, (float*)(d + o_res)})))
    return rc;
  float res[4] = {0, 0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(res, d + o_res, 12, hipMemcpyDeviceToHost, c->stream));
  if (pred) HIP_TRY(c, hipMemcpyAsync(pred, d + o_pred, 4 * nB, hipMemcpyDeviceToHost, c->stream));
  if (prob) HIP_TRY(c, hipMemcpyAsync(prob, d + o_prob, 4 * nB, hipMemcpyDeviceToHost, c->stream));
  if (cost) HIP_TRY(c, hipMemcpyAsync(cost, d + o_cost, 4 * nB, hipMemcpyDeviceToHost, c->stream));
  if (probsN) HIP_TRY(c, hipMemcpyAsync(probsN, d + o_pn, 4 * nB * n_probs, hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  if (error) *error = res[0];
  if (accuracy) *accuracy = res[1];
  if (correct) std::memcpy(correct, &res[2], 4);
  return FLEET_OK;
}

}  // namespace

int fleet_evaluate_device(fleet_ctx* c, const void* d_w, const void* d_b, const void* d_images, size_t n_images, int F,
                          const void* d_labels, const void* d_idx, int B, void* d_pred, void* d_prob, void* d_cost,
                          void* d_probs10, void* d_result, void* stream) {
  if (!c || !d_w || !d_b || !d_images || !d_labels || !d_result || B <= 0 || F < 28 * 28 || n_images == 0 ||
      (!d_idx && (size_t)B > n_images))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  float* cost;
  int32_t* pred;
  const int rc = eval_untaken(c, B, d_cost, d_pred, &cost, &pred);
  if (rc) return rc;
  HIP_TRY(c, fleet::launch_eval((const float*)d_w, (const float*)d_b, (const float*)d_images, (int64_t)n_images, F,
                                (const int32_t*)d_labels, (const int32_t*)d_idx, B, pred, (float*)d_prob, cost,
                                (float*)d_probs10, (float*)d_result, c->d_dev_err, pick(c, stream)));
  return FLEET_OK;
}

int fleet_evaluate(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                   size_t n_images, int F, const int32_t* labels, const int32_t* idx, int B, float* error,
                   float* accuracy, int32_t* correct, int32_t* pred, float* prob) {
  if (!c || !w || !b || !images || !labels || B <= 0 || F < 28 * 28 || n_images == 0) return FLEET_ERR_ARG;
  return evaluate_host(c, "evaluate", w, n_w, fleet_teacher_weight_count(), b, n_b, fleet_teacher_bias_count(), images,
                       n_images, F, labels, idx, B, error, accuracy, correct, pred, prob, nullptr, nullptr, 0,
                       [=](const EvalArgs& a) {
                         HIP_TRY(c, fleet::launch_eval(a.w, a.b, a.images, a.rows, F, a.labels, a.idx, B, a.pred, a.prob,
                                                       a.cost, nullptr, a.result, c->d_err, c->stream));
                         return FLEET_OK;
                       });
}

// ------------------------------------------ test() on the CIFAR network (cifar_kernels.hip)

size_t fleet_cifar_weight_count(int classes) { return (size_t)fleet::cifarnet::weight_count(classes); }
size_t fleet_cifar_bias_count(int classes) { return (size_t)fleet::cifarnet::bias_count(classes); }
size_t fleet_cifar_block_images(void) { return (size_t)fleet::cifar_block_images(); }
int fleet_cifar_set_grid(int max_blocks) { return fleet::cifar_set_grid(max_blocks); }

int fleet_cifar_test_device(fleet_ctx* c, int classes, const void* d_w, const void* d_b, const void* d_images,
                            size_t n_images, int F, const void* d_labels, const void* d_idx, int B, void* d_pred,
                            void* d_prob, void* d_cost, void* d_probsN, void* d_result, void* stream) {
  if (!c || !fleet::cifarnet::classes_ok(classes) || !d_w || !d_b || !d_images || !d_labels || !d_result || B <= 0 ||
      F < fleet::cifarnet::kPix || n_images == 0 || (!d_idx && (size_t)B > n_images))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  float* cost;
  int32_t* pred;
  const int rc = eval_untaken(c, B, d_cost, d_pred, &cost, &pred);
  if (rc) return rc;
  HIP_TRY(c, fleet::launch_cifar_test(classes, (const float*)d_w, (const float*)d_b, (const float*)d_images,
                                      (int64_t)n_images, F, (const int32_t*)d_labels, (const int32_t*)d_idx, B, pred,
                                      (float*)d_prob, cost, (float*)d_probsN, (float*)d_result, c->d_dev_err,
                                      pick(c, stream)));
  return FLEET_OK;
}

int fleet_cifar_test(fleet_ctx* c, int classes, const float* w, size_t n_w, const float* b, size_t n_b,
                     const float* images, size_t n_images, int F, const int32_t* labels, const int32_t* idx, int B,
                     float* error, float* accuracy, int32_t* correct, int32_t* pred, float* prob, float* cost,
                     float* probsN) {
  if (!c || !w || !b || !images || !labels || B <= 0 || F < fleet::cifarnet::kPix || n_images == 0) return FLEET_ERR_ARG;
  if (!fleet::cifarnet::classes_ok(classes)) return fail(c, FLEET_ERR_ARG, "cifar test: %d classes, the network has 10 or 100", classes);
  return evaluate_host(c, "cifar test", w, n_w, fleet_cifar_weight_count(classes), b, n_b, fleet_cifar_bias_count(classes),
                       images, n_images, F, labels, idx, B, error, accuracy, correct, pred, prob, cost, probsN,
                       (size_t)classes, [=](const EvalArgs& a) {
                         HIP_TRY(c, fleet::launch_cifar_test(classes, a.w, a.b, a.images, a.rows, F, a.labels, a.idx, B,
                                                             a.pred, a.prob, a.cost, a.probsN, a.result, c->d_err,
                                                             c->stream));
                         return FLEET_OK;
                       });
}

// ------------------------------------------ the client's getGradients (client_kernels.hip)

size_t fleet_client_grad_len(void) { return (size_t)fleet::client_grad_len(); }
int fleet_client_grad_set_chunk(int max_clients) { return fleet::client_grad_set_chunk(max_clients); }

// Client/app/src/main/cpp/cppNN-lib.cpp:101-113, 218-234; commonLib/cppNN/network.h:1806-2008,
// 1551-1611, 1289-1331, 1038-1056
namespace {

// the cost and the DP parameters of the _ex_ forms, before anything else is looked at
bool client_ex_args_ok(int cost, const float* clip, const float* sigma, int C) {
  if (cost != FLEET_COST_CROSS_ENTROPY && cost != FLEET_COST_DISTILLATION) return false;
  if (!clip != !sigma) return false;
  for (int c = 0; clip && c < C; ++c) {
    if (!(sigma[c] >= 0.0f) || std::isinf(sigma[c])) return false;
    if (sigma[c] > 0.0f && (!(clip[c] > 0.0f) || std::isinf(clip[c]))) return false;
  }
  return true;
}

// every form, the lock held and the device set: the workspace, the launches per chunk of
// clients, the encode of the rows; err: the error word the kernels report to. clip, sigma: host
// [C] or both NULL (checked by client_ex_args_ok).
int client_grads_locked(fleet_ctx* c, const void* d_models, size_t model_pitch, int n_models,
                        const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                        const void* d_labels, const void* d_idx, const void* d_shift, int C, int B, float temperature,
                        int cost, const float* clip, const float* sigma, void* d_grads, size_t grad_pitch,
                        void* d_uploads, size_t upload_pitch, hipStream_t s) {
  const size_t n_up = fleet_client_grad_len();
  const int chunk = fleet::client_grad_chunk(C, B);
  const size_t rows_bytes = fleet::client_grad_workspace_bytes(chunk, B);
  std::vector<uint8_t> dp_of_client;
  bool dp = false;
  if (sigma) {
    dp_of_client.resize((size_t)C);
    for (int i = 0; i < C; ++i) dp |= (dp_of_client[(size_t)i] = sigma[i] > 0.0f) != 0;
  }
  // the scales lie behind the rows, with or without DP, so a DP call grows nothing a plain one made
  const size_t need = rows_bytes + fleet::client_grad_scale_bytes(chunk, B);
  const hipError_t ew = c->d_client_ws.grow_exact(need, 64, &c->retired);
  if (ew != hipSuccess) return nomem(c, "hipMalloc", need, ew);
  if (dp) {
    if (!c->d_dp_z) {  // once per context
      // the host table is made once per process and kept: every context uploads the same draws
      static const std::vector<double> z = [n_up] {
        std::vector<double> t(n_up);
        fleet::client_dp_noise(t.data(), t.size());
        return t;
      }();
      const hipError_t e = c->d_dp_z.alloc(n_up);
      if (e != hipSuccess) return nomem(c, "hipMalloc", sizeof(double) * n_up, e);
      const hipError_t e2 = hipMemcpy(c->d_dp_z, z.data(), sizeof(double) * n_up, hipMemcpyHostToDevice);
      if (e2 != hipSuccess) {
        c->d_dp_z.reset();
        return fail(c, FLEET_ERR_HIP, "the DP noise table: %s", hipGetErrorString(e2));
      }
    }
    const hipError_t ed = c->d_client_dp.grow_exact(2 * (size_t)C, 0, &c->retired);
    if (ed != hipSuccess) return nomem(c, "hipMalloc", 8 * (size_t)C, ed);
    // pageable sources: the copies have left clip and sigma when the call returns
    HIP_TRY(c, hipMemcpyAsync(c->d_client_dp, clip, sizeof(float) * (size_t)C, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_client_dp + C, sigma, sizeof(float) * (size_t)C, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(c, fleet::launch_client_grads_ex((const float*)d_models, (int64_t)model_pitch, n_models,
                                           (const int32_t*)d_model_of_client, (const float*)d_images,
                                           (int64_t)n_images, F, (const int32_t*)d_labels, (const int32_t*)d_idx,
                                           (const int32_t*)d_shift, C, B, chunk, temperature, cost,
                                           dp ? c->d_client_dp : nullptr, dp ? c->d_client_dp + C : nullptr,
                                           dp ? dp_of_client.data() : nullptr, dp ? c->d_dp_z : nullptr,
                                           dp ? (float*)(c->d_client_ws + rows_bytes) : nullptr,
                                           (float*)c->d_client_ws.get(), (float*)d_grads, (int64_t)grad_pitch, c->d_dev_err, s));
  if (d_uploads)
    HIP_TRY(c, fleet::launch_encode_f32((const float*)d_grads, (int64_t)n_up, grad_pitch, C, (uint8_t*)d_uploads,
                                        upload_pitch, s));
  return FLEET_OK;
}

}  // namespace

int fleet_client_dp_noise(double* out, size_t n) {
  if (!out || n > fleet_client_grad_len()) return FLEET_ERR_ARG;
  fleet::client_dp_noise(out, n);
  return FLEET_OK;
}

int fleet_client_ex_grads_device(fleet_ctx* c, const void* d_models, size_t model_pitch, int n_models,
                                 const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                                 const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                                 float temperature, int cost, const float* clip, const float* sigma, void* d_grads,
                                 size_t grad_pitch, void* d_uploads, size_t upload_pitch, void* stream) {
  const size_t n_up = fleet_client_grad_len();
  if (!c || !d_models || !d_images || !d_labels || !d_grads || C <= 0 || B <= 0 || F < 28 * 28 || n_models <= 0 ||
      n_images == 0 || model_pitch < fleet_teacher_weight_count() + fleet_teacher_bias_count() || grad_pitch < n_up ||
      (size_t)C * (size_t)B > (size_t)INT32_MAX || (!d_idx && (size_t)C * (size_t)B > n_images))
    return FLEET_ERR_ARG;
  if (!client_ex_args_ok(cost, clip, sigma, C))
    return fail(c, FLEET_ERR_ARG, "client gradients: cost 0 or 1; clip and sigma both or neither, sigma >= 0 and "
                                  "finite, clip > 0 and finite where sigma > 0");
  if (d_uploads && (upload_pitch % 16 != 0 || upload_pitch < 16 * groups_of(n_up)))
    return fail(c, FLEET_ERR_ARG, "bad upload pitch");
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  return client_grads_locked(c, d_models, model_pitch, n_models, d_model_of_client, d_images, n_images, F, d_labels, d_idx,
                             d_shift, C, B, temperature, cost, clip, sigma, d_grads, grad_pitch, d_uploads, upload_pitch,
                             pick(c, stream));
}

int fleet_client_grads_device(fleet_ctx* c, const void* d_models, size_t model_pitch, int n_models,
                              const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                              const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                              float temperature, void* d_grads, size_t grad_pitch, void* d_uploads,
                              size_t upload_pitch, void* stream) {
  return fleet_client_ex_grads_device(c, d_models, model_pitch, n_models, d_model_of_client, d_images, n_images, F,
                                      d_labels, d_idx, d_shift, C, B, temperature, FLEET_COST_CROSS_ENTROPY, nullptr,
                                      nullptr, d_grads, grad_pitch, d_uploads, upload_pitch, stream);
}

namespace {

// what client_grads_host hands the network's locked launcher: the workspace's device pointers
struct GradArgs {
  const void* models;
  size_t model_pitch;
  const void* images;
  size_t rows;
  const void *labels, *idx, *shift;
  void *grads, *uploads;
  size_t upload_pitch;
};

// fleet_client_ex_grads and fleet_rgbnet_grads behind their own early checks: the count, pick,
// index, shift and pitch checks, the workspace, the copies in, the network's locked launcher on
// the context's stream (locked(GradArgs), returning a FLEET code), the copies out and the error
// word. n_up: the network's gradient length.
template <typename Locked>
int client_grads_host(fleet_ctx* c, const float* w, size_t n_w, size_t want_w, const float* b, size_t n_b, size_t want_b,
                      const float* images, size_t n_images, int F, const int32_t* labels, const int32_t* idx,
                      const int32_t* shifts, int C, int B, size_t n_up, float* grads, char* uploads, size_t upload_pitch,
                      Locked locked) {
  int rc = check_model_counts(c, "client gradients", n_w, n_b, want_w, want_b);
  if (rc) return rc;
  const size_t n = (size_t)C * (size_t)B;
  if (n > (size_t)INT32_MAX) return fail(c, FLEET_ERR_ARG, "client gradients: %d clients of %d samples", C, B);
  if (!idx && n > n_images) return fail(c, FLEET_ERR_ARG, "client gradients: %zu images asked of %zu", n, n_images);
  for (size_t i = 0; idx && i < n; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return fail(c, FLEET_ERR_ARG, "sample %zu: index %d outside the %zu images", i, idx[i], n_images);
  for (size_t i = 0; shifts && i < 2 * n; ++i)
    if (shifts[i] < -1 || shifts[i] > 1)
      return fail(c, FLEET_ERR_ARG, "sample %zu: shift %d outside {-1, 0, 1}", i / 2, shifts[i]);
  const size_t up_len = fleet_b64_len(n_up), groups_bytes = 16 * groups_of(n_up);
  if (uploads && upload_pitch < up_len) return fail(c, FLEET_ERR_CAPACITY, "upload pitch %zu < %zu", upload_pitch, up_len);
  const size_t rows = idx ? n_images : n;  // the images the call reads
  const size_t o_x = round16(sizeof(float) * (n_w + n_b)), o_l = o_x + round16(sizeof(float) * rows * (size_t)F);
  const size_t o_i = o_l + round16(4 * rows), o_s = o_i + round16(4 * n), o_g = o_s + round16(8 * n);
  const size_t o_u = o_g + round16(sizeof(float) * (size_t)C * n_up), o_end = o_u + (uploads ? (size_t)C * groups_bytes : 0);
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, w, sizeof(float) * n_w, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + sizeof(float) * n_w, b, sizeof(float) * n_b, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_x, images, sizeof(float) * rows * (size_t)F, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_l, labels, 4 * rows, hipMemcpyHostToDevice, c->stream));
  if (idx) HIP_TRY(c, hipMemcpyAsync(d + o_i, idx, 4 * n, hipMemcpyHostToDevice, c->stream));
  if (shifts) HIP_TRY(c, hipMemcpyAsync(d + o_s, shifts, 8 * n, hipMemcpyHostToDevice, c->stream));
  if ((rc = locked(GradArgs{d, n_w + n_b, d + o_x, rows, d + o_l, idx ? d + o_i : nullptr, shifts ? d + o_s : nullptr,
                            d + o_g, uploads ? d + o_u : nullptr, groups_bytes})))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(grads, d + o_g, sizeof(float) * (size_t)C * n_up, hipMemcpyDeviceToHost, c->stream));
  if (uploads)
    HIP_TRY(c, hipMemcpy2DAsync(uploads, upload_pitch, d + o_u, groups_bytes, up_len, (size_t)C, hipMemcpyDeviceToHost,
                                c->stream));
  return read_err(c, c->stream, c->d_dev_err);
}

}  // namespace

int fleet_client_ex_grads(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                          size_t n_images, int F, const int32_t* labels, const int32_t* idx, const int32_t* shifts,
                          int C, int B, float temperature, int cost, const float* clip, const float* sigma,
                          float* grads, char* uploads, size_t upload_pitch) {
  if (!c || !w || !b || !images || !labels || !grads || C <= 0 || B <= 0 || F < 28 * 28 || n_images == 0)
    return FLEET_ERR_ARG;
  if (!client_ex_args_ok(cost, clip, sigma, C))
    return fail(c, FLEET_ERR_ARG, "client gradients: cost 0 or 1; clip and sigma both or neither, sigma >= 0 and "
                                  "finite, clip > 0 and finite where sigma > 0");
  return client_grads_host(
      c, w, n_w, fleet_teacher_weight_count(), b, n_b, fleet_teacher_bias_count(), images, n_images, F, labels, idx, shifts,
      C, B, fleet_client_grad_len(), grads, uploads, upload_pitch, [=](const GradArgs& a) {
        return client_grads_locked(c, a.models, a.model_pitch, 1, nullptr, a.images, a.rows, F, a.labels, a.idx, a.shift, C,
                                   B, temperature, cost, clip, sigma, a.grads, fleet_client_grad_len(), a.uploads,
                                   a.upload_pitch, c->stream);
      });
}

int fleet_client_grads(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                       size_t n_images, int F, const int32_t* labels, const int32_t* idx, const int32_t* shifts, int C,
                       int B, float temperature, float* grads, char* uploads, size_t upload_pitch) {
  return fleet_client_ex_grads(c, w, n_w, b, n_b, images, n_images, F, labels, idx, shifts, C, B, temperature,
                               FLEET_COST_CROSS_ENTROPY, nullptr, nullptr, grads, uploads, upload_pitch);
}

// ------------------------------------------ getGradients on the CIFAR network (cifar_client_kernels.hip)

size_t fleet_rgbnet_grad_len(int classes) { return (size_t)fleet::rgbnet_grad_len(classes); }
size_t fleet_rgbnet_sample_tile(void) { return (size_t)fleet::rgbnet_sample_tile(); }
int fleet_rgbnet_set_chunk(int max_clients) { return fleet::rgbnet_set_chunk(max_clients); }

namespace {

// the draws of a DP vector on this network: fleet_client_dp_noise's table continued to the
// CIFAR-100 vector's length by the same host code, made once per process and kept
const std::vector<double>& rgb_dp_table() {
  static const std::vector<double> z = [] {
    std::vector<double> t(fleet_rgbnet_grad_len(100));
    fleet::client_dp_noise(t.data(), t.size());
    return t;
  }();
  return z;
}

// every form, the lock held and the device set: the records' workspace (the one of
// fleet_client_grads_device, under its rule), the launches per chunk of clients, the encode.
// clip, sigma: host [C] or both NULL (checked by client_ex_args_ok).
int rgbnet_grads_locked(fleet_ctx* c, int classes, const void* d_models, size_t model_pitch, int n_models,
                        const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                        const void* d_labels, const void* d_idx, const void* d_shift, int C, int B, float temperature,
                        const float* clip, const float* sigma, void* d_grads, size_t grad_pitch, void* d_uploads,
                        size_t upload_pitch, hipStream_t s) {
  const int chunk = fleet::rgbnet_chunk(classes, C, B);
  const size_t recs_bytes = fleet::rgbnet_workspace_bytes(classes, chunk, B);
  std::vector<uint8_t> dp_of_client;
  bool dp = false;
  if (sigma) {
    dp_of_client.resize((size_t)C);
    for (int i = 0; i < C; ++i) dp |= (dp_of_client[(size_t)i] = sigma[i] > 0.0f) != 0;
  }
  // the scales lie behind the records, with or without DP, so a DP call grows nothing a plain one made
  const size_t need = recs_bytes + fleet::rgbnet_scale_bytes(chunk, B);
  const hipError_t ew = c->d_client_ws.grow_exact(need, 64, &c->retired);
  if (ew != hipSuccess) return nomem(c, "hipMalloc", need, ew);
  if (dp) {
    if (!c->d_rgb_z) {  // once per context
      const std::vector<double>& z = rgb_dp_table();
      const hipError_t e = c->d_rgb_z.alloc(z.size());
      if (e != hipSuccess) return nomem(c, "hipMalloc", sizeof(double) * z.size(), e);
      const hipError_t e2 = hipMemcpy(c->d_rgb_z, z.data(), sizeof(double) * z.size(), hipMemcpyHostToDevice);
      if (e2 != hipSuccess) {
        c->d_rgb_z.reset();
        return fail(c, FLEET_ERR_HIP, "the DP noise table: %s", hipGetErrorString(e2));
      }
    }
    const hipError_t ed = c->d_client_dp.grow_exact(2 * (size_t)C, 0, &c->retired);
    if (ed != hipSuccess) return nomem(c, "hipMalloc", 8 * (size_t)C, ed);
    // pageable sources: the copies have left clip and sigma when the call returns
    HIP_TRY(c, hipMemcpyAsync(c->d_client_dp, clip, sizeof(float) * (size_t)C, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_client_dp + C, sigma, sizeof(float) * (size_t)C, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(c, fleet::launch_rgbnet_grads_dp(classes, (const float*)d_models, (int64_t)model_pitch, n_models,
                                           (const int32_t*)d_model_of_client, (const float*)d_images,
                                           (int64_t)n_images, F, (const int32_t*)d_labels, (const int32_t*)d_idx,
                                           (const int32_t*)d_shift, C, B, chunk, temperature,
                                           dp ? c->d_client_dp : nullptr, dp ? c->d_client_dp + C : nullptr,
                                           dp ? dp_of_client.data() : nullptr, dp ? c->d_rgb_z : nullptr,
                                           dp ? (float*)(c->d_client_ws + recs_bytes) : nullptr,
                                           (float*)c->d_client_ws.get(), (float*)d_grads, (int64_t)grad_pitch,
                                           c->d_dev_err, s));
  if (d_uploads)
    HIP_TRY(c, fleet::launch_encode_f32((const float*)d_grads, (int64_t)fleet_rgbnet_grad_len(classes), grad_pitch, C,
                                        (uint8_t*)d_uploads, upload_pitch, s));
  return FLEET_OK;
}

}  // namespace

int fleet_rgb_dp_noise(double* out, size_t n) {
  if (!out || n > fleet_rgbnet_grad_len(100)) return FLEET_ERR_ARG;
  std::memcpy(out, rgb_dp_table().data(), sizeof(double) * n);
  return FLEET_OK;
}

int fleet_rgb_dp_grads_device(fleet_ctx* c, int classes, const void* d_models, size_t model_pitch, int n_models,
                              const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                              const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                              float temperature, const float* clip, const float* sigma, void* d_grads,
                              size_t grad_pitch, void* d_uploads, size_t upload_pitch, void* stream) {
  const size_t n_up = fleet_rgbnet_grad_len(classes);
  if (!c || !n_up || !d_models || !d_images || !d_labels || !d_grads || C <= 0 || B <= 0 || F < fleet::cifarnet::kPix ||
      n_models <= 0 || n_images == 0 || model_pitch < fleet_cifar_weight_count(classes) + fleet_cifar_bias_count(classes) ||
      grad_pitch < n_up || (size_t)C * (size_t)B > (size_t)INT32_MAX || (!d_idx && (size_t)C * (size_t)B > n_images))
    return FLEET_ERR_ARG;
  if (!client_ex_args_ok(FLEET_COST_CROSS_ENTROPY, clip, sigma, C))
    return fail(c, FLEET_ERR_ARG, "client gradients: clip and sigma both or neither, sigma >= 0 and finite, clip > 0 "
                                  "and finite where sigma > 0");
  if (d_uploads && (upload_pitch % 16 != 0 || upload_pitch < 16 * groups_of(n_up)))
    return fail(c, FLEET_ERR_ARG, "bad upload pitch");
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  return rgbnet_grads_locked(c, classes, d_models, model_pitch, n_models, d_model_of_client, d_images, n_images, F,
                             d_labels, d_idx, d_shift, C, B, temperature, clip, sigma, d_grads, grad_pitch, d_uploads,
                             upload_pitch, pick(c, stream));
}

int fleet_rgbnet_grads_device(fleet_ctx* c, int classes, const void* d_models, size_t model_pitch, int n_models,
                              const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                              const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                              float temperature, void* d_grads, size_t grad_pitch, void* d_uploads,
                              size_t upload_pitch, void* stream) {
  return fleet_rgb_dp_grads_device(c, classes, d_models, model_pitch, n_models, d_model_of_client, d_images, n_images, F,
                                   d_labels, d_idx, d_shift, C, B, temperature, nullptr, nullptr, d_grads, grad_pitch,
                                   d_uploads, upload_pitch, stream);
}

int fleet_rgb_dp_grads(fleet_ctx* c, int classes, const float* w, size_t n_w, const float* b, size_t n_b,
                       const float* images, size_t n_images, int F, const int32_t* labels, const int32_t* idx,
                       const int32_t* shifts, int C, int B, float temperature, const float* clip, const float* sigma,
                       float* grads, char* uploads, size_t upload_pitch) {
  if (!c || !w || !b || !images || !labels || !grads || C <= 0 || B <= 0 || F < fleet::cifarnet::kPix || n_images == 0)
    return FLEET_ERR_ARG;
  if (!fleet::cifarnet::classes_ok(classes))
    return fail(c, FLEET_ERR_ARG, "client gradients: %d classes, the network has 10 or 100", classes);
  if (!client_ex_args_ok(FLEET_COST_CROSS_ENTROPY, clip, sigma, C))
    return fail(c, FLEET_ERR_ARG, "client gradients: clip and sigma both or neither, sigma >= 0 and finite, clip > 0 "
                                  "and finite where sigma > 0");
  return client_grads_host(
      c, w, n_w, fleet_cifar_weight_count(classes), b, n_b, fleet_cifar_bias_count(classes), images, n_images, F, labels,
      idx, shifts, C, B, fleet_rgbnet_grad_len(classes), grads, uploads, upload_pitch, [=](const GradArgs& a) {
        return rgbnet_grads_locked(c, classes, a.models, a.model_pitch, 1, nullptr, a.images, a.rows, F, a.labels, a.idx,
                                   a.shift, C, B, temperature, clip, sigma, a.grads, fleet_rgbnet_grad_len(classes),
                                   a.uploads, a.upload_pitch, c->stream);
      });
}

int fleet_rgbnet_grads(fleet_ctx* c, int classes, const float* w, size_t n_w, const float* b, size_t n_b,
                       const float* images, size_t n_images, int F, const int32_t* labels, const int32_t* idx,
                       const int32_t* shifts, int C, int B, float temperature, float* grads, char* uploads,
                       size_t upload_pitch) {
  return fleet_rgb_dp_grads(c, classes, w, n_w, b, n_b, images, n_images, F, labels, idx, shifts, C, B, temperature,
                            nullptr, nullptr, grads, uploads, upload_pitch);
}

int fleet_model_params(fleet_ctx* c, const float* weights, size_t n_weights, const float* biases, size_t n_biases,
                       int graph_edges, char* out, size_t cap, size_t* out_len) {
  if (!c || graph_edges < 0 || (n_weights && !weights) || (n_biases && !biases)) return FLEET_ERR_ARG;
  const size_t n = n_biases * (size_t)graph_edges + n_weights;
  const size_t len = fleet_b64_len(n);
  if (out_len) *out_len = len;
  if (cap < len || !out) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, len);
  DevBuf<float> dw, db;  // declared out here: freed after the lock and the device scope end
  DevBuf<uint8_t> dt;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DEVICE_SCOPE(c);
    if (n_weights) HIP_TRY(c, dw.alloc(n_weights));
    if (n_biases) HIP_TRY(c, db.alloc(n_biases));
    HIP_TRY(c, dt.alloc(16 * groups_of(n) + 16));
    if (n_weights) HIP_TRY(c, hipMemcpyAsync(dw, weights, n_weights * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (n_biases) HIP_TRY(c, hipMemcpyAsync(db, biases, n_biases * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, fleet::launch_encode_model_params(dw, (int64_t)n_weights, db, (int64_t)n_biases,
                                                 n_biases ? (int64_t)graph_edges : 0, dt, c->stream));
    if (len) HIP_TRY(c, hipMemcpyAsync(out, dt, len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FLEET_OK;
}

// ------------------------------------------ SGD epilogue (descentNative)

namespace {

// Segments of network::descent(vector)'s walk over the gradients() layout
// (network.h:1185-1202): weight blocks of non-null W, bias blocks of the
// fully-connected layers. Also the layout's total length and the model sizes.
// Segments of the model step; with [vb, ve) only the parts whose gradient
// positions fall in that window of upload values (an element shard), with
// gradient offsets relative to vb.
static int descent_segments(fleet_ctx* c, const int32_t* w_sizes, const uint8_t* w_present, int n_w,
                     const int32_t* b_sizes, const uint8_t* fc_layer, int n_b, size_t* n_up, size_t* n_weights,
                     size_t* n_fc, std::vector<fleet::DescentSegs>* segs, size_t vb = 0, size_t ve = SIZE_MAX) {
  if (n_w < 0 || n_b < 0 || (n_w && (!w_sizes || !w_present)) || (n_b && (!b_sizes || !fc_layer)))
    return fail(c, FLEET_ERR_ARG, "bad descent layout arguments");
  segs->clear();
  auto add = [&](int kind, size_t g, size_t m, size_t len) {
    const size_t lo = std::max(g, vb), hi = std::min(g + len, ve);
    if (lo >= hi) return;
    m += lo - g;
    len = hi - lo;
    g = lo - vb;
    if (segs->empty() || segs->back().n == fleet::kMaxDescentSegs) {
      segs->emplace_back();
      segs->back().n = 0;
    }
    fleet::DescentSegs& d = segs->back();
    d.kind[d.n] = kind;
    d.grad_off[d.n] = (int64_t)g;
    d.model_off[d.n] = (int64_t)m;
    d.len[d.n] = (int64_t)len;
    ++d.n;
  };
  size_t idx = 1, wo = 0, bo = 0;
  for (int i = 0; i < n_w; ++i) {
    if (w_sizes[i] < 0) return fail(c, FLEET_ERR_ARG, "negative weight block size");
    ++idx;
    if (w_present[i] && w_sizes[i] > 0) add(0, idx, wo, (size_t)w_sizes[i]);
    if (w_present[i]) wo += (size_t)w_sizes[i];
    idx += (size_t)w_sizes[i];
  }
  ++idx;
  for (int k = 0; k < n_b; ++k) {
    if (b_sizes[k] < 0) return fail(c, FLEET_ERR_ARG, "negative bias block size");
    ++idx;
    if (fc_layer[k] && b_sizes[k] > 0) add(1, idx, bo, (size_t)b_sizes[k]);
    if (fc_layer[k]) bo += (size_t)b_sizes[k];
    idx += (size_t)b_sizes[k];
  }
  *n_up = idx;
  *n_weights = wo;
  *n_fc = bo;
  return FLEET_OK;
}

}  // namespace

int fleet_descent_device(fleet_ctx* c, float* d_weights, float* d_fc_bias, const float* d_grad,
                         const int32_t* w_sizes, const uint8_t* w_present, int n_w, const int32_t* b_sizes,
                         const uint8_t* fc_layer, int n_b, float lr, void* stream) {
  if (!c || !d_grad) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  if (rc) return rc;
  if ((nw && !d_weights) || (nf && !d_fc_bias)) return FLEET_ERR_ARG;
  for (const auto& sg : segs)
    HIP_TRY(c, fleet::launch_descent(d_weights, d_fc_bias, d_grad, sg, lr, pick(c, stream)));
  return FLEET_OK;
}

int fleet_descent_window_device(fleet_ctx* c, float* d_weights, float* d_fc_bias, const float* d_grad_window,
                                size_t value_begin, size_t value_end, const int32_t* w_sizes,
                                const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer,
                                int n_b, float lr, void* stream) {
  if (!c || !d_grad_window || value_end < value_begin) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs, value_begin,
                            value_end);
  if (rc) return rc;
  if ((nw && !d_weights) || (nf && !d_fc_bias)) return FLEET_ERR_ARG;
  for (const auto& sg : segs)
    HIP_TRY(c, fleet::launch_descent(d_weights, d_fc_bias, d_grad_window, sg, lr, pick(c, stream)));
  return FLEET_OK;
}

int fleet_descent(fleet_ctx* c, float* weights, size_t n_weights, float* fc_bias, size_t n_fc_bias,
                  const float* grad, size_t n_grad, const int32_t* w_sizes, const uint8_t* w_present, int n_w,
                  const int32_t* b_sizes, const uint8_t* fc_layer, int n_b, float lr) {
  if (!c || !grad) return FLEET_ERR_ARG;
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  }
  if (rc) return rc;
  if (n_grad != n_up || n_weights != nw || n_fc_bias != nf || (nw && !weights) || (nf && !fc_bias))
    return fail(c, FLEET_ERR_ARG, "descent: sizes do not match the layout (grad %zu/%zu, weights %zu/%zu, bias %zu/%zu)",
                n_grad, n_up, n_weights, nw, n_fc_bias, nf);
  // the header floats network::descent(vector) reads its block sizes from
  size_t idx = 0;
  bool ok = grad[idx++] == (float)n_w;
  for (int i = 0; i < n_w && ok; ++i) {
    ok = grad[idx++] == (float)w_sizes[i];
    idx += (size_t)w_sizes[i];
  }
  ok = ok && grad[idx++] == (float)n_b;
  for (int k = 0; k < n_b && ok; ++k) {
    ok = grad[idx++] == (float)b_sizes[k];
    idx += (size_t)b_sizes[k];
  }
  if (!ok) return fail(c, FLEET_ERR_LAYOUT, "descent: gradient header does not match the model layout");
  DevBuf<float> dw, db, dg;  // freed after the lock and the device scope end
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DEVICE_SCOPE(c);
    if (nw) HIP_TRY(c, dw.alloc(nw));
    if (nf) HIP_TRY(c, db.alloc(nf));
    HIP_TRY(c, dg.alloc(n_grad));
    if (nw) HIP_TRY(c, hipMemcpyAsync(dw, weights, nw * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(db, fc_bias, nf * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dg, grad, n_grad * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (const auto& sg : segs) HIP_TRY(c, fleet::launch_descent(dw, db, dg, sg, lr, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(weights, dw, nw * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(fc_bias, db, nf * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FLEET_OK;
}

// The same step under the reference's other solvers (solver_kernels.hip, solver_math.h)

int fleet_solver_from_name(const char* name) {
  if (!name) return -1;
  static const char* const names[] = {"sgd", "adagrad", "rmsprop", "adam"};  // new_solver (solver.h:198-208)
  for (int i = 0; i < 4; ++i)
    if (!std::strcmp(name, names[i])) return i;
  return -1;
}

namespace {
static int solver_args(fleet_ctx* c, int solver, const void* g1, const void* g2, size_t nw) {
  if (solver < FLEET_SOLVER_SGD || solver > FLEET_SOLVER_ADAM) return fail(c, FLEET_ERR_ARG, "no solver %d", solver);
  if (nw && ((solver != FLEET_SOLVER_SGD && !g1) || (solver == FLEET_SOLVER_ADAM && !g2)))
    return fail(c, FLEET_ERR_ARG, "descent: solver %d needs its state row%s", solver,
                solver == FLEET_SOLVER_ADAM ? "s g1 and g2" : " g1");
  return FLEET_OK;
}
}  // namespace

int fleet_descent_solver_device(fleet_ctx* c, int solver, float* d_weights, float* d_g1, float* d_g2,
                                float* d_fc_bias, const float* d_grad, const int32_t* w_sizes,
                                const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer,
                                int n_b, float lr, void* stream) {
  if (!c || !d_grad) return FLEET_ERR_ARG;
  if (solver == FLEET_SOLVER_SGD)
    return fleet_descent_device(c, d_weights, d_fc_bias, d_grad, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, lr,
                                stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  if (rc) return rc;
  if ((nw && !d_weights) || (nf && !d_fc_bias)) return FLEET_ERR_ARG;
  if ((rc = solver_args(c, solver, d_g1, d_g2, nw))) return rc;
  float b1_t, b2_t;  // a fresh solver's
  fleet::adam_bias_terms(0, &b1_t, &b2_t);
  for (const auto& sg : segs)
    HIP_TRY(c, fleet::launch_descent_solver(solver, d_weights, d_g1, d_g2, d_fc_bias, d_grad, sg, lr, b1_t, b2_t,
                                            pick(c, stream)));
  return FLEET_OK;
}

int fleet_descent_solver(fleet_ctx* c, int solver, float* weights, size_t n_weights, float* g1, float* g2,
                         float* fc_bias, size_t n_fc_bias, const float* grad, size_t n_grad, const int32_t* w_sizes,
                         const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer, int n_b,
                         float lr) {
  return fleet::descent_solver_host(c, solver, 0, weights, n_weights, g1, g2, fc_bias, n_fc_bias, grad, n_grad, w_sizes,
                                    w_present, n_w, b_sizes, fc_layer, n_b, lr);
}

// fleet_descent_solver with adam's b1_t, b2_t after `adam_resets` resets (solver_host.h)
int fleet::descent_solver_host(fleet_ctx* c, int solver, int adam_resets, float* weights, size_t n_weights, float* g1,
                               float* g2, float* fc_bias, size_t n_fc_bias, const float* grad, size_t n_grad,
                               const int32_t* w_sizes, const uint8_t* w_present, int n_w, const int32_t* b_sizes,
                               const uint8_t* fc_layer, int n_b, float lr) {
  if (!c || !grad) return FLEET_ERR_ARG;
  if (solver == FLEET_SOLVER_SGD)
    return fleet_descent(c, weights, n_weights, fc_bias, n_fc_bias, grad, n_grad, w_sizes, w_present, n_w, b_sizes,
                         fc_layer, n_b, lr);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  }
  if (rc) return rc;
  if (n_grad != n_up || n_weights != nw || n_fc_bias != nf || (nw && !weights) || (nf && !fc_bias))
    return fail(c, FLEET_ERR_ARG, "descent: sizes do not match the layout (grad %zu/%zu, weights %zu/%zu, bias %zu/%zu)",
                n_grad, n_up, n_weights, nw, n_fc_bias, nf);
  if ((rc = solver_args(c, solver, g1, g2, nw))) return rc;
  size_t idx = 0;  // fleet_descent's header check
  bool ok = grad[idx++] == (float)n_w;
  for (int i = 0; i < n_w && ok; ++i) {
    ok = grad[idx++] == (float)w_sizes[i];
    idx += (size_t)w_sizes[i];
  }
  ok = ok && grad[idx++] == (float)n_b;
  for (int k = 0; k < n_b && ok; ++k) {
    ok = grad[idx++] == (float)b_sizes[k];
    idx += (size_t)b_sizes[k];
  }
  if (!ok) return fail(c, FLEET_ERR_LAYOUT, "descent: gradient header does not match the model layout");
  const bool two = solver == FLEET_SOLVER_ADAM;
  float b1_t, b2_t;
  fleet::adam_bias_terms(adam_resets, &b1_t, &b2_t);
  DevBuf<float> dw, d1, d2, db, dg;  // freed after the lock and the device scope end
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DEVICE_SCOPE(c);
    const size_t wb = nw * sizeof(float);
    if (nw) HIP_TRY(c, dw.alloc(nw));
    if (nw) HIP_TRY(c, d1.alloc(nw));
    if (nw && two) HIP_TRY(c, d2.alloc(nw));
    if (nf) HIP_TRY(c, db.alloc(nf));
    HIP_TRY(c, dg.alloc(n_grad));
    if (nw) HIP_TRY(c, hipMemcpyAsync(dw, weights, wb, hipMemcpyHostToDevice, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(d1, g1, wb, hipMemcpyHostToDevice, c->stream));
    if (nw && two) HIP_TRY(c, hipMemcpyAsync(d2, g2, wb, hipMemcpyHostToDevice, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(db, fc_bias, nf * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dg, grad, n_grad * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (const auto& sg : segs)
      HIP_TRY(c, fleet::launch_descent_solver(solver, dw, d1, d2, db, dg, sg, lr, b1_t, b2_t, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(weights, dw, wb, hipMemcpyDeviceToHost, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(g1, d1, wb, hipMemcpyDeviceToHost, c->stream));
    if (nw && two) HIP_TRY(c, hipMemcpyAsync(g2, d2, wb, hipMemcpyDeviceToHost, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(fc_bias, db, nf * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FLEET_OK;
}

// descentNative's model copy in DISTILLATION_MODE=1 (cppNN_backend.cpp:355-372):
// cnnNew->read(cnn.getParams()) of the unquantised model. getParams prints the
// biases and the first-occurrence dictionary values with `ostream << float`
// (precision 6 = %g) and read() parses them back (strtof); every weight takes
// its dictionary entry's value. All on the device: the dictionary (sort-based,
// no O(n*U) scans), the %g / strtof round trip of the U values and the biases
// (decimal6.h: exact integer arithmetic, checked against libc on every finite
// binary32, digest fn 22) and the gather; no host round trip of the values.
int fleet_model_version(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats, const float* biases,
                        size_t n_biases, float* weights_out, float* biases_out) {
  if (!c || (n_biases && (!biases || !biases_out))) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && (!weights || !weights_out)) return FLEET_ERR_ARG;
  DevBuf<float> dw, dd, db;
  DevBuf<int32_t> di;
  // the biases' text round trip on the device as well (getParams prints them with `<<` too)
  if (n_biases) {
    HIP_TRY(c, db.alloc(n_biases));
    HIP_TRY(c, hipMemcpyAsync(db, biases, n_biases * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
    HIP_TRY(c, fleet::model_g6_inplace(db, (int64_t)n_biases, c->d_err, c->stream));
    HIP_TRY(c, hipMemcpyAsync(biases_out, db, n_biases * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (*c->h_err) {
      HIP_TRY(c, hipMemset(c->d_err, 0, sizeof(int)));
      return fail(c, FLEET_ERR_ARG, "non-finite bias: the reference's text read fails");
    }
  }
  if (!n) return FLEET_OK;
  HIP_TRY(c, dw.alloc(n));
  HIP_TRY(c, dd.alloc(n + 1));
  HIP_TRY(c, di.alloc(n));
  HIP_TRY(c, hipMemcpyAsync(dw, weights, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  int32_t U = 0;
  HIP_TRY(c, fleet::model_quantize_index(dw, dims, n_mats, nullptr, dd, di, &U, c->stream, false));
  // the U dictionary values through `<<` / `>>` (decimal6.h), in place, then the gather
  HIP_TRY(c, hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
  HIP_TRY(c, fleet::model_g6_inplace(dd, (int64_t)U, c->d_err, c->stream));
  HIP_TRY(c, fleet::model_dict_gather(di, (int64_t)n, dd, dw, c->stream));
  HIP_TRY(c, hipMemcpyAsync(weights_out, dw, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*c->h_err) {
    HIP_TRY(c, hipMemset(c->d_err, 0, sizeof(int)));
    return fail(c, FLEET_ERR_ARG, "non-finite weight: the reference's text read fails");
  }
  return FLEET_OK;
}


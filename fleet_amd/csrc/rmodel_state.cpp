// fleet_amd/csrc/rmodel_state.cpp -- the server's model resident in HBM
// (fleet_rmodel): fleet_model's natives (model_state.cpp, same citations) on a
// model whose `cnn` and `models` live on the device.
//
//   fleet_rmodel_load            fetchParamsNative: fleet_model_load's parse, then the
//                                weights and biases go to the device once
//   fleet_rmodel_init_updater    initUpdater's model part
//   fleet_rmodel_descent(_device) descentNative: header checks, step and model copy on
//                                the device (rmodel_kernels.hip, model_codec.hip)
//   fleet_rmodel_get_params      getParametersNative: every value's text formatted on
//                                the device (decimal6.h g6_text) into one buffer
//   fleet_rmodel_get_model_params getModelParametersNative from the resident row
//
// HBM: row 0 of `state` is cnn, rows 1.. are the ring of max_versions + 1
// version rows (the push comes before the pop, as in fleet_model_descent); a
// row is [weights | use_bias() biases], `stride` floats apart. Everything the
// entry points need besides (tables, dictionary and text workspaces, the text
// and a20 buffers) is allocated at load; only the staging of a host gradient
// text grows, on its first use. Host mirrors: the parsed layout (a fleet_model
// that never holds weights), lrates, epoch, priority, the ring's order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fleet_codec.h"
#include "dev_mem.h"
#include "model_codec.h"
#include "model_state.h"
#include "rmodel_kernels.h"
#include "solver_math.h"

struct FLEET_MEM_LOCAL fleet_rmodel {
  fleet_ctx* ctx = nullptr;
  fleet_model* host = nullptr;  // layout, header, dims (its cnn is released after the upload)
  int device = 0, mode = 1, max_versions = 0;
  std::mutex mu;
  hipStream_t stream = nullptr;
  size_t nw = 0, nb = 0, nfc = 0, stride = 0;
  int n_mats = 0, n_bias_blocks = 0;
  // HBM; what grows is freed and allocated at the exact size (nothing here is retired: the
  // two that a caller's stream may still use wait for the device first)
  fleet::DevBuf<float> state;
  fleet::DevBuf<uint8_t> tab, work;
  fleet::DevBuf<char> text;
  fleet::DevBuf<uint8_t> a20;
  fleet::DevBuf<uint8_t> gtext;  // a host gradient text, staged (grown on first use)
  fleet::DevBuf<float> grad;
  fleet::DevBuf<float> sstate;  // the solver's state rows g1 | g2, nw floats each (fleet_rmodel_set_solver)
  int solver = 0;
  bool stepped = false;
  fleet::DevBuf<int32_t> d_client_rows;  // client gradients: the row of every client's version
  fleet::DevBuf<uint8_t> eval_ws;  // evaluation, either network's: [B costs | B predictions | B p | result | staged images, labels, indices]
  fleet::PinBuf<int> h_pin;  // [0] the error word's copy, [4..] the counts line
  // carved from tab / work
  fleet::RmLayout lay{};
  int* d_err = nullptr;
  int64_t *d_woff = nullptr, *d_boff = nullptr;
  char* d_header = nullptr;
  fleet::DictWs dws{};
  fleet::TextWs tws{};
  float *d_wq = nullptr, *d_dict = nullptr;
  int32_t* d_index = nullptr;
  size_t a20_len = 0;
  // ring
  std::deque<int> models;  // row numbers, oldest first
  std::vector<int> free_rows;
  int64_t pushed = 0;
  std::vector<double> lrates;
  float lr = 0.0f;
  int epoch = 0, priority = 0;
  size_t resident_bytes = 0, work_bytes = 0;
  int device_allocs = 0;
  std::string err;
};

namespace {

using fleet::Layer;

int rfail(fleet_rmodel* m, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int rfail(fleet_rmodel* m, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  m->err = buf;
  return code;
}

#define RM_HIP(m, expr)                                                                             \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return rfail((m), FLEET_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// every entry runs on the model's device and restores the caller's
struct DeviceScope {
  int prev = -1;
  bool ok = true;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define RM_SCOPE(m)                  \
  DeviceScope device_scope_((m)->device); \
  if (!device_scope_.ok) return rfail((m), FLEET_ERR_HIP, "hipSetDevice(%d) failed", (m)->device)

// exactly n elements (an empty request still gets a byte); what b held is freed first
template <typename T>
int dev_alloc(fleet_rmodel* m, fleet::DevBuf<T>& b, size_t n) {
  RM_HIP(m, b.alloc(n, n ? 0 : 1));
  m->device_allocs++;
  return FLEET_OK;
}

using fleet::Carver;

float* row_w(fleet_rmodel* m, int row) { return m->state + (size_t)row * m->stride; }
float* row_b(fleet_rmodel* m, int row) { return row_w(m, row) + m->nw; }

// The _device entry points run on the caller's stream as it is given, NULL being the null
// stream as everywhere in this C-ABI: they order with the work that wrote their inputs and
// the caller's next use of their outputs. The host-buffer entry points run on the model's
// own stream and end in a synchronise; so does every step, so nothing of the model is ever
// in flight between two entries.
hipStream_t caller_stream(void* stream) { return (hipStream_t)stream; }

// the error word after everything queued on s (one 4-byte read-back), cleared when set
int read_word(fleet_rmodel* m, hipStream_t s, int* word) {
  RM_HIP(m, hipMemcpyAsync(m->h_pin, m->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
  RM_HIP(m, hipStreamSynchronize(s));
  *word = m->h_pin[0];
  if (*word) {
    RM_HIP(m, hipMemsetAsync(m->d_err, 0, sizeof(int), s));
    RM_HIP(m, hipStreamSynchronize(s));
  }
  return FLEET_OK;
}

// the tables (sizes only with base == nullptr)
size_t carve_tables(fleet_rmodel* m, uint8_t* base) {
  const fleet_model* h = m->host;
  Carver c{base};
  const size_t ne = h->edge_w_size.size(), nl = h->layers.size();
  size_t nfl = 0;
  for (const Layer& L : h->layers) nfl += L.fc ? 1 : 0;
  m->lay.w_present = c.take<uint8_t>(ne);
  m->lay.fc_layer = c.take<uint8_t>(nl);
  m->lay.fcl_start = c.take<int64_t>(nfl + 1);
  m->lay.fcl_boff = c.take<int64_t>(nfl);
  m->lay.w_start = c.take<int64_t>(ne + 1);
  m->lay.w_grad = c.take<int64_t>(ne);
  m->lay.b_start = c.take<int64_t>(nl + 1);
  m->lay.b_grad = c.take<int64_t>(nl);
  m->lay.counts = c.take<int>(2);
  m->d_err = c.take<int>(1);
  m->d_woff = c.take<int64_t>((size_t)m->n_mats + 1);
  m->d_boff = c.take<int64_t>((size_t)m->n_bias_blocks + 1);
  m->d_header = c.take<char>(h->header.size());
  return c.at;
}

size_t carve_work(fleet_rmodel* m, uint8_t* base) {
  Carver c{base};
  const size_t nt = std::max(m->nw, m->nb);
  uint8_t* at = base;
  size_t used = fleet::model_text_ws_carve(at, (int64_t)nt, &m->tws);
  if (!used && nt) return 0;
  c.at = (used + 255) & ~(size_t)255;
  if (m->mode && m->nw) {
    m->d_wq = c.take<float>(m->nw);
    m->d_dict = c.take<float>(m->nw + 1);
    m->d_index = c.take<int32_t>(m->nw);
    used = fleet::model_dict_ws_carve(base ? base + c.at : nullptr, (int64_t)m->nw, m->n_mats, &m->dws);
    if (!used) return 0;
    c.at += used;
  }
  return c.at;
}

void release(fleet_rmodel* m) {
  if (!m) return;
  fleet_model* host = m->host;
  {
    DeviceScope sc(m->device);
    hipStream_t s = m->stream;
    if (s) (void)hipStreamSynchronize(s);
    delete m;  // the model's memory, inside the device scope
    if (s) (void)hipStreamDestroy(s);
  }
  if (host) fleet_model_destroy(host);
}

int set_up(fleet_rmodel* m) {
  fleet_model* h = m->host;
  RM_SCOPE(m);
  m->nw = h->cnn.w.size();
  m->nb = h->cnn.b.size();
  m->n_mats = (int)(h->dims.size() / 3);
  for (const Layer& L : h->layers) {
    m->n_bias_blocks += L.use_bias ? 1 : 0;
    m->nfc += L.fc ? L.bias_size : 0;
  }
  m->stride = (m->nw + m->nb + 63) / 64 * 64;
  if (m->stride == 0) m->stride = 64;
  const size_t rows = (size_t)m->max_versions + 2;
  RM_HIP(m, hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  RM_HIP(m, m->h_pin.alloc(64));
  m->device_allocs++;
  int rc;
  m->resident_bytes = sizeof(float) * m->stride * rows;
  if ((rc = dev_alloc(m, m->state, m->stride * rows))) return rc;
  RM_HIP(m, hipMemsetAsync(m->state, 0, m->resident_bytes, m->stream));
  const size_t tab_bytes = carve_tables(m, nullptr);
  if ((rc = dev_alloc(m, m->tab, tab_bytes))) return rc;
  carve_tables(m, m->tab);
  m->work_bytes = carve_work(m, nullptr);
  if (!m->work_bytes && std::max(m->nw, m->nb)) return rfail(m, FLEET_ERR_HIP, "rocPRIM would not size its storage");
  if ((rc = dev_alloc(m, m->work, m->work_bytes))) return rc;
  carve_work(m, m->work);
  // the longest getParams text: 12 bytes and a separator per value, a line break per
  // block; mode 1 adds the counts, an int key per dictionary entry and an index per weight
  const size_t text_cap = h->header.size() + 13 * m->nb + (size_t)m->n_bias_blocks + 64 +
                          (m->mode ? 24 * m->nw + 12 * m->nw + (size_t)m->n_mats : 13 * m->nw + (size_t)m->n_mats);
  if ((rc = dev_alloc(m, m->text, text_cap))) return rc;
  m->a20_len = fleet_b64_len(m->nb * h->edge_w_size.size() + m->nw);
  if ((rc = dev_alloc(m, m->a20, (m->a20_len + 15) / 16 * 16 + 64))) return rc;
  m->work_bytes += tab_bytes + text_cap + (m->a20_len + 15) / 16 * 16 + 64;

  // tables: what the model knows
  const size_t ne = h->edge_w_size.size(), nl = h->layers.size();
  std::vector<uint8_t> present(ne), fcl(nl);
  for (size_t i = 0; i < ne; ++i) present[i] = h->edge_w_size[i] > 0;
  std::vector<int64_t> fstart{0}, fboff, woff{0}, boff{0};
  size_t o = 0;
  for (size_t k = 0; k < nl; ++k) {
    const Layer& L = h->layers[k];
    fcl[k] = L.fc ? 1 : 0;
    if (L.fc) {
      fboff.push_back((int64_t)o);
      fstart.push_back(fstart.back() + (int64_t)L.bias_size);
    }
    if (L.use_bias) {
      boff.push_back(boff.back() + (int64_t)L.bias_size);
      o += L.bias_size;
    }
  }
  // the text emitters count the line breaks after a value in 8 bits (model_codec.hip VCell)
  for (size_t k = 1, run = 0; k < boff.size(); ++k) {
    run = boff[k] == boff[k - 1] ? run + 1 : 0;
    if (run > 254) return rfail(m, FLEET_ERR_ARG, "more than 254 use_bias() layers without biases in a row");
  }
  for (int j = 0; j < m->n_mats; ++j)
    woff.push_back(woff.back() + (int64_t)h->dims[3 * j] * h->dims[3 * j + 1] * h->dims[3 * j + 2]);
  m->lay.n_edges = (int)ne;
  m->lay.n_layers = (int)nl;
  m->lay.n_fcl = (int)fboff.size();
  m->lay.n_w = (int64_t)m->nw;
  m->lay.n_fc = (int64_t)m->nfc;
  m->lay.n_b = (int64_t)m->nb;
  auto up = [&](const void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpy((void*)dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
  RM_HIP(m, up(m->lay.w_present, present.data(), ne));
  RM_HIP(m, up(m->lay.fc_layer, fcl.data(), nl));
  RM_HIP(m, up(m->lay.fcl_start, fstart.data(), sizeof(int64_t) * fstart.size()));
  RM_HIP(m, up(m->lay.fcl_boff, fboff.data(), sizeof(int64_t) * fboff.size()));
  RM_HIP(m, up(m->d_woff, woff.data(), sizeof(int64_t) * woff.size()));
  RM_HIP(m, up(m->d_boff, boff.data(), sizeof(int64_t) * boff.size()));
  RM_HIP(m, up(m->d_header, h->header.data(), h->header.size()));
  RM_HIP(m, hipMemset(m->d_err, 0, sizeof(int)));
  // cnn: the one host to device trip the weights ever make
  RM_HIP(m, hipStreamSynchronize(m->stream));
  RM_HIP(m, up(row_w(m, 0), h->cnn.w.data(), sizeof(float) * m->nw));
  RM_HIP(m, up(row_b(m, 0), h->cnn.b.data(), sizeof(float) * m->nb));
  std::vector<float>().swap(h->cnn.w);
  std::vector<float>().swap(h->cnn.b);
  for (int r = (int)rows - 1; r >= 1; --r) m->free_rows.push_back(r);
  return FLEET_OK;
}

// descentNative's model copy of cnn into `row` (mode 1: the first-occurrence dictionary and
// the `%g` / strtof round trips of fleet_model_version, in its order and with its errors;
// mode 0: the round trip of every value)
int make_version(fleet_rmodel* m, int row, hipStream_t s) {
  if (!m->mode) {
    RM_HIP(m, fleet::launch_rm_roundtrip(row_w(m, 0), row_w(m, row), (int64_t)(m->nw + m->nb), s));
    RM_HIP(m, hipStreamSynchronize(s));
    return FLEET_OK;
  }
  int bad = 0, rc;
  if (m->nb) {
    RM_HIP(m, hipMemcpyAsync(row_b(m, row), row_b(m, 0), sizeof(float) * m->nb, hipMemcpyDeviceToDevice, s));
    RM_HIP(m, fleet::model_g6_inplace(row_b(m, row), (int64_t)m->nb, m->d_err, s));
    if ((rc = read_word(m, s, &bad))) return rc;
    if (bad) return rfail(m, FLEET_ERR_ARG, "model version copy: non-finite bias: the reference's text read fails");
  }
  if (!m->nw) return FLEET_OK;
  int32_t U = 0;
  RM_HIP(m, fleet::model_quantize_index(row_w(m, 0), m->host->dims.data(), m->n_mats, nullptr, m->d_dict, m->d_index,
                                        &U, s, false, &m->dws));
  RM_HIP(m, fleet::model_g6_inplace(m->d_dict, (int64_t)U, m->d_err, s));
  RM_HIP(m, fleet::model_dict_gather(m->d_index, (int64_t)m->nw, m->d_dict, row_w(m, row), s));
  if ((rc = read_word(m, s, &bad))) return rc;
  if (bad) return rfail(m, FLEET_ERR_ARG, "model version copy: non-finite weight: the reference's text read fails");
  return FLEET_OK;
}

void push_version(fleet_rmodel* m, int row, int stale_size) {
  m->free_rows.pop_back();
  m->models.push_back(row);
  m->pushed++;
  if ((int)m->models.size() > std::max(0, stale_size)) {
    m->free_rows.push_back(m->models.front());
    m->models.pop_front();
  }
}

// descentNative from a gradient on the device (both forms end here)
int step(fleet_rmodel* m, const float* d_grad, size_t n_values, int stale_size, hipStream_t s) {
  const int count = (int)m->models.size();
  const int after = count + 1 > std::max(0, stale_size) ? count : count + 1;
  if (after > m->max_versions)
    return rfail(m, FLEET_ERR_ARG, "descent: stale_size %d would keep %d versions, the model holds %d", stale_size, after,
                 m->max_versions);
  if (m->epoch < (int)m->lrates.size()) m->lr = (float)m->lrates[(size_t)m->epoch];
  const int row = m->free_rows.back();
  RM_HIP(m, fleet::launch_rm_check(d_grad, (int64_t)n_values, m->lay, m->d_err, s));
  float b1_t, b2_t;  // adam's, as fetchParamsNative's start_epoch leaves them
  fleet::adam_bias_terms(fleet::kServerResets, &b1_t, &b2_t);
  if (m->solver == FLEET_SOLVER_SGD)
    RM_HIP(m, fleet::launch_rm_step(row_w(m, 0), row_b(m, 0), d_grad, m->lay, m->lr, m->mode ? nullptr : row_w(m, row),
                                    m->mode ? nullptr : row_b(m, row), m->d_err, s));
  else
    RM_HIP(m, fleet::launch_rm_step_solver(m->solver, row_w(m, 0), row_b(m, 0), m->sstate,
                                           m->solver == FLEET_SOLVER_ADAM ? m->sstate + m->nw : nullptr, d_grad, m->lay,
                                           m->lr, b1_t, b2_t, m->mode ? nullptr : row_w(m, row), m->mode ? nullptr : row_b(m, row),
                                           m->d_err, s));
  int word = 0, rc;
  if ((rc = read_word(m, s, &word))) return rc;
  if (word == fleet::kRmErrSizes)
    return rfail(m, FLEET_ERR_ARG, "descent: the gradient's blocks do not match the model (%zu values, %zu weights, %zu fc biases)",
                 n_values, m->nw, m->nfc);
  if (word) return rfail(m, FLEET_ERR_LAYOUT, "descent: the gradient header does not match the model layout");
  m->epoch++;
  m->stepped = true;
  if (m->mode && (rc = make_version(m, row, s))) return rc;
  push_version(m, row, stale_size);
  return FLEET_OK;
}

int version_row(fleet_rmodel* m, int version, int* row) {
  if (version < 0 || (size_t)version >= m->models.size())
    return rfail(m, FLEET_ERR_ARG, "model version %d of %zu", version, m->models.size());
  *row = m->models[(size_t)version];
  return FLEET_OK;
}

// the evaluation workspace: allocated on first use, grown only for a larger need
int eval_workspace(fleet_rmodel* m, size_t bytes) {
  if (bytes <= m->eval_ws.cap()) return FLEET_OK;
  // (an evaluation on a caller's stream may still write the old one)
  if (m->eval_ws) RM_HIP(m, hipDeviceSynchronize());
  return dev_alloc(m, m->eval_ws, bytes);
}

inline size_t r256(size_t x) { return (x + 255) & ~(size_t)255; }

// both evaluate forms, the lock held: `staged` bytes follow the per-image part of the workspace
int evaluate_on(fleet_rmodel* m, int version, const void* d_images, size_t n_images, int F, const void* d_labels,
                const void* d_idx, int B, void* d_pred, void* d_prob, void* d_result, size_t staged, hipStream_t s) {
  std::string why;
  if (fleet::eval_check_mnist(m->host, &why)) return rfail(m, FLEET_ERR_ARG, "evaluate: %s", why.c_str());
  int row = 0, rc;
  if (version >= 0 && (rc = version_row(m, version, &row))) return rc;
  if ((rc = eval_workspace(m, 3 * r256(4 * (size_t)B) + 256 + staged))) return rc;
  uint8_t* ws = m->eval_ws;
  if ((rc = fleet_evaluate_device(m->ctx, row_w(m, row), row_b(m, row), d_images, n_images, F, d_labels, d_idx, B,
                                  d_pred ? d_pred : ws + r256(4 * (size_t)B), d_prob, ws, nullptr, d_result, (void*)s)))
    return rfail(m, rc, "evaluate: %s", rc == FLEET_ERR_ARG ? "images, labels and a result, B >= 1 (and <= n_images without indices), F >= 784"
                                                            : fleet_last_error(m->ctx));
  return FLEET_OK;
}

// both forms of test() on the CIFAR network, the lock held: evaluate_on with cifar_check and
// fleet_cifar_test_device in its places, on the same workspace
int cifar_test_on(fleet_rmodel* m, int version, const void* d_images, size_t n_images, int F, const void* d_labels,
                  const void* d_idx, int B, void* d_pred, void* d_prob, void* d_result, size_t staged, hipStream_t s) {
  std::string why;
  int classes = 0;
  if (fleet::cifar_check(m->host, &classes, &why)) return rfail(m, FLEET_ERR_ARG, "cifar test: %s", why.c_str());
  int row = 0, rc;
  if (version >= 0 && (rc = version_row(m, version, &row))) return rc;
  if ((rc = eval_workspace(m, 3 * r256(4 * (size_t)B) + 256 + staged))) return rc;
  uint8_t* ws = m->eval_ws;
  if ((rc = fleet_cifar_test_device(m->ctx, classes, row_w(m, row), row_b(m, row), d_images, n_images, F, d_labels, d_idx,
                                    B, d_pred ? d_pred : ws + r256(4 * (size_t)B), d_prob, ws, nullptr, d_result,
                                    (void*)s)))
    return rfail(m, rc, "cifar test: %s", rc == FLEET_ERR_ARG ? "images, labels and a result, B >= 1 (and <= n_images without indices), F >= 3072"
                                                              : fleet_last_error(m->ctx));
  return FLEET_OK;
}

// the host form of either network's test(), the lock held and the device set: every refusal
// first, then images, labels and indices staged behind the per-image part of the workspace,
// evaluate_on / cifar_test_on on the model's own stream, and the results copied out
int host_test(fleet_rmodel* m, bool cifar, int version, const float* images, size_t n_images, int F,
              const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy, int32_t* correct,
              int32_t* pred, float* prob) {
  const char* what = cifar ? "cifar test" : "evaluate";
  const int min_F = cifar ? 3 * 32 * 32 : 28 * 28;
  if (!images || !labels || B <= 0 || F < min_F || n_images == 0 || (!idx && (size_t)B > n_images))
    return rfail(m, FLEET_ERR_ARG, "%s: images and labels, B >= 1 (and <= n_images without indices), F >= %d", what, min_F);
  for (int i = 0; idx && i < B; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return rfail(m, FLEET_ERR_ARG, "image %d: index %d outside the %zu images", i, idx[i], n_images);
  std::string why;
  int classes = 0;
  if (cifar ? fleet::cifar_check(m->host, &classes, &why) : fleet::eval_check_mnist(m->host, &why))
    return rfail(m, FLEET_ERR_ARG, "%s: %s", what, why.c_str());
  int row = 0, rc;
  if (version >= 0 && (rc = version_row(m, version, &row))) return rc;
  const size_t rows = idx ? n_images : (size_t)B;  // the images the evaluation reads
  const size_t per = 3 * r256(4 * (size_t)B) + 256;
  const size_t o_x = per, o_l = o_x + r256(sizeof(float) * rows * (size_t)F), o_i = o_l + r256(4 * rows);
  const size_t staged = o_i + r256(4 * (size_t)B) - per;
  if ((rc = eval_workspace(m, per + staged))) return rc;
  uint8_t* ws = m->eval_ws;
  hipStream_t s = m->stream;
  RM_HIP(m, hipMemcpyAsync(ws + o_x, images, sizeof(float) * rows * (size_t)F, hipMemcpyHostToDevice, s));
  RM_HIP(m, hipMemcpyAsync(ws + o_l, labels, 4 * rows, hipMemcpyHostToDevice, s));
  if (idx) RM_HIP(m, hipMemcpyAsync(ws + o_i, idx, 4 * (size_t)B, hipMemcpyHostToDevice, s));
  uint8_t* d_pred = ws + r256(4 * (size_t)B);
  uint8_t* d_prob = ws + 2 * r256(4 * (size_t)B);
  uint8_t* d_res = ws + 3 * r256(4 * (size_t)B);
  if ((rc = (cifar ? cifar_test_on : evaluate_on)(m, version, ws + o_x, rows, F, ws + o_l, idx ? ws + o_i : nullptr, B,
                                                  d_pred, d_prob, d_res, staged, s)))
    return rc;
  float res[4] = {0, 0, 0, 0};
  RM_HIP(m, hipMemcpyAsync(res, d_res, 12, hipMemcpyDeviceToHost, s));
  if (pred) RM_HIP(m, hipMemcpyAsync(pred, d_pred, 4 * (size_t)B, hipMemcpyDeviceToHost, s));
  if (prob) RM_HIP(m, hipMemcpyAsync(prob, d_prob, 4 * (size_t)B, hipMemcpyDeviceToHost, s));
  if ((rc = fleet_check(m->ctx, (void*)s))) return rfail(m, rc, "%s: %s", what, fleet_last_error(m->ctx));
  if (error) *error = res[0];
  if (accuracy) *accuracy = res[1];
  if (correct) std::memcpy(correct, &res[2], 4);
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_rmodel_load(fleet_ctx* ctx, const char* text, size_t len, int distillation_mode, int max_versions,
                      fleet_rmodel** out) {
  if (!ctx || !out || (!text && len) || max_versions < 1) return FLEET_ERR_ARG;
  *out = nullptr;
  fleet_model* host = nullptr;
  const int rc = fleet_model_load(ctx, text, len, distillation_mode, &host);
  if (rc) return rc;
  fleet_rmodel* m = new fleet_rmodel();
  m->ctx = ctx;
  m->host = host;
  m->device = fleet_ctx_device(ctx);
  m->mode = host->mode;
  m->max_versions = max_versions;
  const int rc2 = set_up(m);
  if (rc2) {
    std::fprintf(stderr, "[fleet] fleet_rmodel_load: %s\n", m->err.c_str());
    release(m);
    return rc2;
  }
  *out = m;
  return FLEET_OK;
}

void fleet_rmodel_destroy(fleet_rmodel* m) { release(m); }

const char* fleet_rmodel_last_error(const fleet_rmodel* m) { return m ? m->err.c_str() : "no model"; }

int fleet_rmodel_init_updater(fleet_rmodel* m, const double* lrates, int n_lrates) {
  if (!m || n_lrates <= 0 || !lrates) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  if ((int)m->models.size() + 1 > m->max_versions)  // (initUpdater pushes and never pops)
    return rfail(m, FLEET_ERR_ARG, "initUpdater: the model already holds its %d versions", m->max_versions);
  m->lrates.assign(lrates, lrates + n_lrates);
  m->lr = (float)m->lrates[0];
  const int row = m->free_rows.back();
  const int rc = make_version(m, row, m->stream);
  if (rc) return rc;
  m->free_rows.pop_back();
  m->models.push_back(row);
  m->pushed++;
  m->priority = 0;
  m->epoch = 0;
  return FLEET_OK;
}

int fleet_rmodel_descent(fleet_rmodel* m, const char* merged, size_t len, int client_batch_size, int stale_size) {
  (void)client_batch_size;  // cnn.set_mini_batch_size: sizes dW storage only, no arithmetic effect
  if (!m || (!merged && len)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  if (len % 4 != 0) return rfail(m, FLEET_ERR_BASE64, "descent: Base64 length %zu is not a multiple of 4", len);
  const size_t n = fleet_b64_count(len), padded = (len + 15) / 16 * 16 + 16;
  int rc;
  // both grow on the first use (and for a longer text)
  if (padded > m->gtext.cap() && (rc = dev_alloc(m, m->gtext, padded))) return rc;
  if (n + 3 > m->grad.cap() && (rc = dev_alloc(m, m->grad, n + 3))) return rc;
  hipStream_t s = m->stream;
  RM_HIP(m, hipMemsetAsync(m->gtext + (len & ~(size_t)15), 0, padded - (len & ~(size_t)15), s));
  if (len) RM_HIP(m, hipMemcpyAsync(m->gtext, merged, len, hipMemcpyHostToDevice, s));
  if (len) {
    if ((rc = fleet_decode_device(m->ctx, m->gtext, len, padded, 1, m->grad, n + 3, s)))
      return rfail(m, rc, "descent: %s", fleet_last_error(m->ctx));
    if ((rc = fleet_check(m->ctx, s))) return rfail(m, rc, "descent: %s", fleet_last_error(m->ctx));
  }
  return step(m, m->grad, n, stale_size, s);
}

int fleet_rmodel_descent_device(fleet_rmodel* m, const void* d_merged_f32, size_t n_values, int stale_size,
                                void* stream) {
  if (!m || !d_merged_f32) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  // the shortest gradient of this model: both counts, a size per graph edge and per layer,
  // every weight and fc bias (the other layers' bias blocks are the gradient's own)
  const size_t least = 2 + m->host->edge_w_size.size() + m->host->layers.size() + m->nw + m->nfc;
  if (n_values < least || n_values > (size_t)INT64_MAX / 8)
    return rfail(m, FLEET_ERR_ARG, "descent: %zu values, a gradient of this model holds at least %zu", n_values, least);
  return step(m, (const float*)d_merged_f32, n_values, stale_size, caller_stream(stream));
}

int fleet_rmodel_set_solver(fleet_rmodel* m, const char* name) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  const int sv = fleet_solver_from_name(name);
  if (sv < 0) return rfail(m, FLEET_ERR_ARG, "set_solver: no solver \"%s\" (sgd, adagrad, rmsprop, adam)", name ? name : "(null)");
  if (m->stepped) return rfail(m, FLEET_ERR_ARG, "set_solver: the model has been stepped");
  const auto rows_of = [](int v) { return (size_t)(v == FLEET_SOLVER_SGD ? 0 : v == FLEET_SOLVER_ADAM ? 2 : 1); };
  // (a second call before the first step starts over: state rows are small beside the versions)
  m->sstate.reset();
  m->resident_bytes -= sizeof(float) * m->nw * rows_of(m->solver);
  m->solver = FLEET_SOLVER_SGD;
  const size_t bytes = sizeof(float) * m->nw * rows_of(sv);
  if (rows_of(sv)) {
    int rc;
    if ((rc = dev_alloc(m, m->sstate, m->nw * rows_of(sv)))) return rc;
    m->resident_bytes += bytes;
    RM_HIP(m, hipMemsetAsync(m->sstate, 0, bytes, m->stream));
    RM_HIP(m, hipStreamSynchronize(m->stream));
  }
  m->solver = sv;
  return FLEET_OK;
}

int fleet_rmodel_solver(fleet_rmodel* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return m->solver;
}

int fleet_rmodel_solver_state(fleet_rmodel* m, int which, float* out, size_t cap) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  if (which < 0 || which > 1 || m->solver == FLEET_SOLVER_SGD || (which == 1 && m->solver != FLEET_SOLVER_ADAM))
    return rfail(m, FLEET_ERR_ARG, "solver_state: solver %d keeps no state row %d", m->solver, which);
  if (cap < m->nw || (m->nw && !out)) return rfail(m, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, m->nw);
  if (m->nw) RM_HIP(m, hipMemcpy(out, m->sstate + (size_t)which * m->nw, sizeof(float) * m->nw, hipMemcpyDeviceToHost));
  return FLEET_OK;
}

int fleet_rmodel_count(fleet_rmodel* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return (int)m->models.size();
}

size_t fleet_rmodel_params_cap(const fleet_rmodel* m) { return m ? m->text.cap() : 0; }

int fleet_rmodel_get_params(fleet_rmodel* m, int version, char* out, size_t cap, size_t* out_len) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  int row = 0, rc;
  if ((rc = version_row(m, version, &row))) return rc;
  hipStream_t s = m->stream;
  const std::string& header = m->host->header;
  size_t at = header.size();
  int64_t got = 0;
  if (at) RM_HIP(m, hipMemcpyAsync(m->text, m->d_header, at, hipMemcpyDeviceToDevice, s));
  if (m->nb) {
    RM_HIP(m, fleet::model_values_text_ws(row_b(m, row), (int64_t)m->nb, m->d_boff, m->n_bias_blocks, m->tws,
                                          m->text + at, (int64_t)(m->text.cap() - at), &got, s));
    at += (size_t)got;
  } else if (m->n_bias_blocks) {  // every use_bias() layer still prints its line
    RM_HIP(m, hipMemsetAsync(m->text + at, '\n', (size_t)m->n_bias_blocks, s));
    at += (size_t)m->n_bias_blocks;
  }
  if (!m->mode) {
    if (m->nw) {
      RM_HIP(m, fleet::model_values_text_ws(row_w(m, row), (int64_t)m->nw, m->d_woff, m->n_mats, m->tws, m->text + at,
                                            (int64_t)(m->text.cap() - at), &got, s));
      at += (size_t)got;
    }
  } else {
    // save_model_weights, quantization_weight_model, getParams, load_model_weights: the
    // quantised weights' dictionary section; the version itself is not modified
    int32_t U = 0;
    if (m->nw)
      RM_HIP(m, fleet::model_quantize_index(row_w(m, row), m->host->dims.data(), m->n_mats, m->d_wq, m->d_dict,
                                            m->d_index, &U, s, true, &m->dws));
    char* counts = (char*)(m->h_pin + 4);  // (the stream is idle: every piece above ended in a sync)
    const int cl = snprintf(counts, 64, "%zu\n%d\n", m->nw, U);
    RM_HIP(m, hipMemcpyAsync(m->text + at, counts, (size_t)cl, hipMemcpyHostToDevice, s));
    at += (size_t)cl;
    if (U) {
      RM_HIP(m, fleet::model_values_text_ws(m->d_dict, (int64_t)U, nullptr, 0, m->tws, m->text + at,
                                            (int64_t)(m->text.cap() - at), &got, s));
      at += (size_t)got;
    }
    if (m->nw) {
      RM_HIP(m, fleet::model_index_text_ws(m->d_index, (int64_t)m->nw, m->d_woff, m->n_mats, m->tws, m->text + at,
                                           (int64_t)(m->text.cap() - at), &got, s));
      at += (size_t)got;
    }
  }
  if (out_len) *out_len = at;
  if (!out || cap < at) {
    RM_HIP(m, hipStreamSynchronize(s));
    return rfail(m, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, at);
  }
  RM_HIP(m, hipMemcpyAsync(out, m->text, at, hipMemcpyDeviceToHost, s));  // the one copy out
  RM_HIP(m, hipStreamSynchronize(s));
  return FLEET_OK;
}

int fleet_rmodel_get_model_params_device(fleet_rmodel* m, int version, void* d_out, void* stream) {
  if (!m || !d_out) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  int row = 0, rc;
  if ((rc = version_row(m, version, &row))) return rc;
  if ((rc = fleet_model_params_device(m->ctx, row_w(m, row), m->nw, row_b(m, row), m->nb,
                                      (int)m->host->edge_w_size.size(), d_out, stream)))
    return rfail(m, rc, "getModelParams: %s", fleet_last_error(m->ctx));
  return FLEET_OK;
}

int fleet_rmodel_get_model_params(fleet_rmodel* m, int version, char* out, size_t cap, size_t* out_len) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  int row = 0, rc;
  if ((rc = version_row(m, version, &row))) return rc;
  if (out_len) *out_len = m->a20_len;
  if (!out || cap < m->a20_len) return rfail(m, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, m->a20_len);
  if ((rc = fleet_model_params_device(m->ctx, row_w(m, row), m->nw, row_b(m, row), m->nb,
                                      (int)m->host->edge_w_size.size(), m->a20, (void*)m->stream)))
    return rfail(m, rc, "getModelParams: %s", fleet_last_error(m->ctx));
  if (m->a20_len) RM_HIP(m, hipMemcpyAsync(out, m->a20, m->a20_len, hipMemcpyDeviceToHost, m->stream));
  RM_HIP(m, hipStreamSynchronize(m->stream));
  return FLEET_OK;
}

int fleet_rmodel_get_epoch(fleet_rmodel* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return m->epoch;
}
void fleet_rmodel_set_epoch(fleet_rmodel* m, int epoch) {
  if (!m) return;
  std::lock_guard<std::mutex> lk(m->mu);
  m->epoch = epoch;
}
int fleet_rmodel_get_priority(fleet_rmodel* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return m->priority;
}
void fleet_rmodel_set_priority(fleet_rmodel* m, int p) {
  if (!m) return;
  std::lock_guard<std::mutex> lk(m->mu);
  m->priority = p;
}
double fleet_rmodel_get_lrate(fleet_rmodel* m) {
  if (!m) return 0.0;
  std::lock_guard<std::mutex> lk(m->mu);
  return (double)m->lr;
}

int fleet_rmodel_export(fleet_rmodel* m, int version, float* weights, size_t n_weights, float* biases,
                        size_t n_biases) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  int row = 0, rc;
  if (version >= 0 && (rc = version_row(m, version, &row))) return rc;
  if (n_weights != m->nw || n_biases != m->nb)
    return rfail(m, FLEET_ERR_ARG, "model holds %zu weights and %zu biases", m->nw, m->nb);
  if (n_weights) RM_HIP(m, hipMemcpy(weights, row_w(m, row), sizeof(float) * n_weights, hipMemcpyDeviceToHost));
  if (n_biases) RM_HIP(m, hipMemcpy(biases, row_b(m, row), sizeof(float) * n_biases, hipMemcpyDeviceToHost));
  return FLEET_OK;
}

int fleet_rmodel_shape(fleet_rmodel* m, size_t* n_weights_out, size_t* n_biases_out, int* graph_edges, int* n_layers) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (n_weights_out) *n_weights_out = m->nw;
  if (n_biases_out) *n_biases_out = m->nb;
  if (graph_edges) *graph_edges = (int)m->host->edge_w_size.size();
  if (n_layers) *n_layers = (int)m->host->layers.size();
  return FLEET_OK;
}

int fleet_rmodel_version_id(fleet_rmodel* m, int version, int64_t* id) {
  if (!m || !id) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  int row = 0, rc;
  if ((rc = version_row(m, version, &row))) return rc;
  *id = m->pushed - (int64_t)m->models.size() + version;
  return FLEET_OK;
}

int fleet_rmodel_version_device(fleet_rmodel* m, int version, const float** d_weights, const float** d_biases) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  int row = 0, rc;
  if (version >= 0 && (rc = version_row(m, version, &row))) return rc;
  if (d_weights) *d_weights = row_w(m, row);
  if (d_biases) *d_biases = row_b(m, row);
  return FLEET_OK;
}

int fleet_rmodel_stage_mledger(fleet_mledger* ledger, fleet_rmodel* m, int version, int64_t* id) {
  if (!ledger || !m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  int row = 0, rc;
  if ((rc = version_row(m, version, &row))) return rc;
  // the rows go device to device, and a failing stage leaves its text in the ledger's context
  if (fleet_ctx_of_mledger(ledger) != m->ctx)
    return rfail(m, FLEET_ERR_ARG, "stage: the ledger was made on another context than the model");
  size_t nw = 0, nb = 0;
  int edges = 0;
  if ((rc = fleet_mledger_shape(ledger, &nw, &nb, &edges, nullptr, nullptr))) return rc;
  if (nw != m->nw || nb != m->nb || edges != (int)m->host->edge_w_size.size())
    return rfail(m, FLEET_ERR_ARG, "the ledger holds %zu weights, %zu biases, %d edges; the model %zu, %zu, %zu", nw, nb,
                 edges, m->nw, m->nb, m->host->edge_w_size.size());
  const int64_t vid = m->pushed - (int64_t)m->models.size() + version;
  // device to device: the row is complete (every step ends in a sync), so any stream will do
  if ((rc = fleet_mledger_stage_device(ledger, vid, m->nw ? row_w(m, row) : nullptr, m->nb ? row_b(m, row) : nullptr,
                                       (void*)m->stream)))
    return rfail(m, rc, "stage: %s", fleet_last_error(m->ctx));
  RM_SCOPE(m);
  RM_HIP(m, hipStreamSynchronize(m->stream));
  if (id) *id = vid;
  return FLEET_OK;
}

int fleet_rmodel_evaluate_device(fleet_rmodel* m, int version, const void* d_images, size_t n_images, int F,
                                 const void* d_labels, const void* d_idx, int B, void* d_pred, void* d_prob,
                                 void* d_result, void* stream) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  if (!d_images || !d_labels || !d_result || B <= 0 || F < 28 * 28 || n_images == 0 || (!d_idx && (size_t)B > n_images))
    return rfail(m, FLEET_ERR_ARG, "evaluate: images, labels and a result, B >= 1 (and <= n_images without indices), F >= 784");
  return evaluate_on(m, version, d_images, n_images, F, d_labels, d_idx, B, d_pred, d_prob, d_result, 0,
                     caller_stream(stream));
}

int fleet_rmodel_evaluate(fleet_rmodel* m, int version, const float* images, size_t n_images, int F,
                          const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                          int32_t* correct, int32_t* pred, float* prob) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  return host_test(m, false, version, images, n_images, F, labels, idx, B, error, accuracy, correct, pred, prob);
}

int fleet_rmodel_cifar_test_device(fleet_rmodel* m, int version, const void* d_images, size_t n_images, int F,
                                   const void* d_labels, const void* d_idx, int B, void* d_pred, void* d_prob,
                                   void* d_result, void* stream) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  if (!d_images || !d_labels || !d_result || B <= 0 || F < 3 * 32 * 32 || n_images == 0 || (!d_idx && (size_t)B > n_images))
    return rfail(m, FLEET_ERR_ARG, "cifar test: images, labels and a result, B >= 1 (and <= n_images without indices), F >= 3072");
  return cifar_test_on(m, version, d_images, n_images, F, d_labels, d_idx, B, d_pred, d_prob, d_result, 0,
                       caller_stream(stream));
}

int fleet_rmodel_cifar_test(fleet_rmodel* m, int version, const float* images, size_t n_images, int F,
                            const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                            int32_t* correct, int32_t* pred, float* prob) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  return host_test(m, true, version, images, n_images, F, labels, idx, B, error, accuracy, correct, pred, prob);
}

int fleet_rmodel_client_ex_grads_device(fleet_rmodel* m, const int32_t* versions, const void* d_images, size_t n_images,
                                        int F, const void* d_labels, const void* d_idx, const void* d_shift, int C,
                                        int B, float temperature, int cost, const float* clip, const float* sigma,
                                        void* d_grads, size_t grad_pitch, void* d_uploads, size_t upload_pitch,
                                        void* stream) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  RM_SCOPE(m);
  if (!versions || !d_images || !d_labels || !d_grads || C <= 0 || B <= 0 || F < 28 * 28 || n_images == 0)
    return rfail(m, FLEET_ERR_ARG, "client gradients: versions, images, labels and rows, C >= 1, B >= 1, F >= 784");
  std::string why;
  if (fleet::eval_check_mnist(m->host, &why)) return rfail(m, FLEET_ERR_ARG, "client gradients: %s", why.c_str());
  std::vector<int32_t> rows((size_t)C, 0);
  int rc, n_rows = 1;
  for (int c = 0; c < C; ++c) {
    int row = 0;
    if (versions[c] >= 0 && (rc = version_row(m, versions[c], &row))) return rc;
    rows[(size_t)c] = row;
    n_rows = std::max(n_rows, row + 1);
  }
  hipStream_t s = caller_stream(stream);
  if ((size_t)C > m->d_client_rows.cap()) {
    // (a call on another stream may still read the old one)
    if (m->d_client_rows) RM_HIP(m, hipDeviceSynchronize());
    if ((rc = dev_alloc(m, m->d_client_rows, (size_t)C))) return rc;
  }
  // pageable source: the copy has left `rows` when the call returns
  RM_HIP(m, hipMemcpyAsync(m->d_client_rows, rows.data(), 4 * (size_t)C, hipMemcpyHostToDevice, s));
  if ((rc = fleet_client_ex_grads_device(m->ctx, m->state, m->stride, n_rows, m->d_client_rows, d_images, n_images, F,
                                         d_labels, d_idx, d_shift, C, B, temperature, cost, clip, sigma, d_grads,
                                         grad_pitch, d_uploads, upload_pitch, (void*)s)))
    return rfail(m, rc, "client gradients: %s", rc == FLEET_ERR_ARG ? "C*B images without indices, a row pitch >= 22961, an upload pitch of whole groups, a cost and DP parameters in range"
                                                                     : fleet_last_error(m->ctx));
  return FLEET_OK;
}

int fleet_rmodel_client_grads_device(fleet_rmodel* m, const int32_t* versions, const void* d_images, size_t n_images,
                                     int F, const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                                     float temperature, void* d_grads, size_t grad_pitch, void* d_uploads,
                                     size_t upload_pitch, void* stream) {
  return fleet_rmodel_client_ex_grads_device(m, versions, d_images, n_images, F, d_labels, d_idx, d_shift, C, B,
                                             temperature, FLEET_COST_CROSS_ENTROPY, nullptr, nullptr, d_grads,
                                             grad_pitch, d_uploads, upload_pitch, stream);
}

int fleet_rmodel_stats(fleet_rmodel* m, size_t* resident_bytes, int* device_allocs) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (resident_bytes) *resident_bytes = m->resident_bytes;
  if (device_allocs) *device_allocs = m->device_allocs;
  return FLEET_OK;
}

size_t fleet_rmodel_workspace_bytes(const fleet_rmodel* m) { return m ? m->work_bytes : 0; }

}  // extern "C"

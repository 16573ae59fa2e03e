// fleet_amd/csrc/model_state.cpp -- the server's resident model (fleet_model):
// the state the reference's updater natives keep in globals of libnative.so
// (Server/src/main/c++/cppNN_backend.cpp: `cnn`, `models`, `lrates_vec`,
// `currEpoch`, `priority`), on top of the public C-ABI (fleet_codec.h).
//
//   fleet_model_load        fetchParamsNative (:282-301): network::read of a
//                           getParams text (commonLib/cppNN/network.h:840-1010)
//   fleet_model_init_updater initUpdater's model part (:161-194)
//   fleet_model_descent     descentNative (:329-383)
//   fleet_model_get_params  getParametersNative (:244-280)
//   fleet_model_get_model_params getModelParametersNative (:227-242)
//
// The text is the mojo01 format of network::getParams (network.h:611-706):
// "mojo01", the layer count, per layer its name and config string, the layer
// graph, "0", one bias line per use_bias() layer, then the weights (mode 1:
// the first-occurrence dictionary and one index line per non-null W; mode 0:
// one value line per non-null W). The W shapes (needed by the mode-1
// quantisation, round_matrix's s = rows*cols) follow the layers' own
// new_connection rules (commonLib/cppNN/layer.h:148-160 base / fully
// connected, :343-358 pooling, :776-788 convolution); the layer types FLeet's
// cppNN models use are supported (input, convolution, max_pool,
// semi_stochastic_pool, fully_connected), others are rejected.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/fleet_codec.h"
#include "model_state.h"
#include "solver_host.h"
#include "solver_math.h"

using fleet::Layer;
using fleet::Version;

namespace {

int mfail(fleet_model* m, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int mfail(fleet_model* m, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  m->err = buf;
  return code;
}

// getline that drops a trailing '\r' (network.h getcleanline)
bool next_line(const std::string& t, size_t& pos, std::string& line) {
  if (pos >= t.size()) return false;
  size_t e = t.find('\n', pos);
  if (e == std::string::npos) e = t.size();
  line = t.substr(pos, e - pos);
  if (!line.empty() && line.back() == '\r') line.pop_back();
  pos = e + 1 > t.size() ? t.size() : e + 1;
  return true;
}

std::vector<std::string> tokens(const std::string& s) {
  std::istringstream ss(s);
  std::vector<std::string> out;
  for (std::string w; ss >> w;) out.push_back(w);
  return out;
}

bool to_long(const std::string& s, long* v) {
  char* e = nullptr;
  *v = strtol(s.c_str(), &e, 10);
  return e != s.c_str() && *e == 0;
}

// `ostream << float` (precision 6, %g) followed by the separator
void put_float(std::string& out, float v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%g", (double)v);
  out += buf;
}

int parse(fleet_model* m, const std::string& t, std::vector<float>* w, std::vector<float>* b) {
  size_t pos = 0;
  std::string line;
  if (!next_line(t, pos, line) || line != "mojo01") return mfail(m, FLEET_ERR_ARG, "model text: no mojo01 header");
  long n_layers = 0;
  if (!next_line(t, pos, line) || !to_long(line, &n_layers) || n_layers <= 0 || n_layers > 4096)
    return mfail(m, FLEET_ERR_ARG, "model text: bad layer count");
  for (long j = 0; j < n_layers; ++j) {
    Layer L;
    std::string cfg;
    if (!next_line(t, pos, L.name) || !next_line(t, pos, cfg)) return mfail(m, FLEET_ERR_ARG, "model text: truncated layers");
    const auto tk = tokens(cfg);
    if (tk.empty()) return mfail(m, FLEET_ERR_ARG, "model text: empty config of layer %s", L.name.c_str());
    L.type = tk[0];
    for (size_t i = 1; i < tk.size(); ++i) {
      long v;
      if (to_long(tk[i], &v)) L.args.push_back(v);
      else L.act = tk[i];
    }
    auto need = [&](size_t k) { return L.args.size() >= k; };
    if (L.type == "input") {
      if (!need(3)) return mfail(m, FLEET_ERR_ARG, "input layer %s: want cols rows chans", L.name.c_str());
      L.cols = (int)L.args[0], L.rows = (int)L.args[1], L.chans = (int)L.args[2];
    } else if (L.type == "convolution") {
      if (!need(3) || L.args[0] < 1 || L.args[1] < 1 || L.args[2] < 1)
        return mfail(m, FLEET_ERR_ARG, "convolution layer %s: want kernel maps stride", L.name.c_str());
      L.use_bias = true;
    } else if (L.type == "max_pool" || L.type == "semi_stochastic_pool") {
      if (!need(2) || L.args[0] < 1 || L.args[1] < 1)
        return mfail(m, FLEET_ERR_ARG, "pooling layer %s: want pool stride", L.name.c_str());
    } else if (L.type == "fully_connected") {
      if (!need(1) || L.args[0] < 1) return mfail(m, FLEET_ERR_ARG, "fully_connected layer %s: want size", L.name.c_str());
      L.use_bias = L.fc = true;
      L.cols = (int)L.args[0];
      L.bias_size = (size_t)L.args[0];
    } else {
      return mfail(m, FLEET_ERR_ARG, "layer %s: type '%s' is not supported", L.name.c_str(), L.type.c_str());
    }
    m->layers.push_back(L);
  }
  long n_edges = 0;
  if (!next_line(t, pos, line) || !to_long(line, &n_edges) || n_edges < 0 || n_edges > 65536)
    return mfail(m, FLEET_ERR_ARG, "model text: bad graph size");
  auto find = [&](const std::string& nm) {
    for (size_t k = 0; k < m->layers.size(); ++k)
      if (m->layers[k].name == nm) return (int)k;
    return -1;
  };
  for (long e = 0; e < n_edges; ++e) {
    std::string top, bottom;
    if (!next_line(t, pos, top) || !next_line(t, pos, bottom)) return mfail(m, FLEET_ERR_ARG, "model text: truncated graph");
    const int a = find(top), z = find(bottom);
    if (a < 0 || z < 0) return mfail(m, FLEET_ERR_ARG, "model text: graph edge %s -> %s names no layer", top.c_str(), bottom.c_str());
    const Layer& T = m->layers[(size_t)a];
    Layer& B = m->layers[(size_t)z];
    // bottom.new_connection(top): node shape and the W matrix of this edge
    if (B.type == "convolution") {
      const int k = (int)B.args[0], maps = (int)B.args[1], s = (int)B.args[2];
      B.kernels_per_map += T.chans;
      B.cols = std::max(1, (T.cols - k) / s + 1);
      B.rows = std::max(1, (T.rows - k) / s + 1);
      B.chans = maps;
      B.bias_size = (size_t)maps;  // bias = matrix(1, 1, maps)
      m->dims.insert(m->dims.end(), {k, k, maps * B.kernels_per_map});
      m->edge_w_size.push_back(k * k * maps * B.kernels_per_map);
    } else if (B.type == "max_pool" || B.type == "semi_stochastic_pool") {
      const int p = (int)B.args[0], s = (int)B.args[1];
      int w = T.cols / p, h = T.rows / p;
      if (s != p) w = 1 + (T.cols - p) / s, h = 1 + (T.rows - p) / s;
      B.cols = std::max(1, w), B.rows = std::max(1, h), B.chans = std::max(1, T.chans);
      m->edge_w_size.push_back(0);  // no weights: W[edge] == NULL
    } else if (B.type == "fully_connected") {
      const int in = T.cols * T.rows * T.chans, out = B.cols * B.rows * B.chans;
      m->dims.insert(m->dims.end(), {in, out, 1});
      m->edge_w_size.push_back(in * out);
    } else {
      return mfail(m, FLEET_ERR_ARG, "layer %s (%s) cannot be a graph edge's bottom", B.name.c_str(), B.type.c_str());
    }
  }
  if (!next_line(t, pos, line) || line != "0") return mfail(m, FLEET_ERR_ARG, "model text: no '0' line after the graph");
  m->header = t.substr(0, pos);
  for (const Layer& L : m->layers) m->fc.push_back(L.fc ? 1 : 0);
  // bias lines (read(): `ifs >> bias.x[k]`, i.e. strtof, bias.size() of them)
  for (const Layer& L : m->layers) {
    if (!L.use_bias) continue;
    if (!next_line(t, pos, line)) return mfail(m, FLEET_ERR_ARG, "model text: missing bias line of %s", L.name.c_str());
    const auto tk = tokens(line);
    if (tk.size() != L.bias_size)
      return mfail(m, FLEET_ERR_ARG, "model text: %zu biases for %s, expected %zu", tk.size(), L.name.c_str(), L.bias_size);
    for (const auto& s : tk) b->push_back(strtof(s.c_str(), nullptr));
  }
  size_t n_w = 0;
  for (int32_t s : m->edge_w_size) n_w += (size_t)s;
  w->assign(n_w, 0.0f);
  const std::string rest = t.substr(pos);
  if (m->mode) {
    const int rc = fleet_model_read_weights(m->ctx, rest.data(), rest.size(), m->dims.data(), (int)(m->dims.size() / 3),
                                            w->data());
    if (rc) return mfail(m, rc, "model text weights: %s", fleet_last_error(m->ctx));
  } else {
    size_t o = 0, p2 = 0;
    for (int32_t s : m->edge_w_size) {
      if (!s) continue;
      if (!next_line(rest, p2, line)) return mfail(m, FLEET_ERR_ARG, "model text: missing weight line");
      const auto tk = tokens(line);
      if (tk.size() != (size_t)s) return mfail(m, FLEET_ERR_ARG, "model text: %zu weights, expected %d", tk.size(), s);
      for (const auto& x : tk) (*w)[o++] = strtof(x.c_str(), nullptr);
    }
  }
  return FLEET_OK;
}

}  // namespace

int fleet::eval_check_mnist(const fleet_model* m, std::string* why) {
  struct Want {
    const char *name, *type, *act;
    long args[3];
    int n_args;
  };
  static const Want want[] = {{"I1", "input", "identity", {28, 28, 1}, 3},
                              {"C1", "convolution", "elu", {5, 8, 1}, 3},
                              {"P1", "semi_stochastic_pool", "", {3, 3, 0}, 2},
                              {"C2i", "convolution", "elu", {1, 16, 1}, 3},
                              {"C2", "convolution", "elu", {5, 48, 1}, 3},
                              {"P2", "semi_stochastic_pool", "", {2, 2, 0}, 2},
                              {"FC2", "fully_connected", "softmax", {10, 0, 0}, 1}};
  const size_t n = sizeof want / sizeof want[0];
  auto config = [](const std::string& type, const std::vector<long>& args, const std::string& act) {
    std::string s = type;
    for (long a : args) s += " " + std::to_string(a);
    return act.empty() ? s : s + " " + act;
  };
  for (size_t k = 0; k < n; ++k) {
    const Want& W = want[k];
    const std::string expect = config(W.type, std::vector<long>(W.args, W.args + W.n_args), W.act);
    if (k >= m->layers.size()) {
      *why = std::string("layer ") + std::to_string(k) + " (" + W.name + " " + expect + ") is missing";
      return FLEET_ERR_ARG;
    }
    const Layer& L = m->layers[k];
    // (an input layer's "identity" is what getParams prints for it; a text without the word reads the same)
    const bool act_ok = L.act == W.act || (k == 0 && L.act.empty());
    if (L.type != W.type || !act_ok || L.args != std::vector<long>(W.args, W.args + W.n_args)) {
      *why = "layer " + std::to_string(k) + " is " + L.name + " " + config(L.type, L.args, L.act) + ", the MNIST network has " +
             W.name + " " + expect;
      return FLEET_ERR_ARG;
    }
  }
  if (m->layers.size() != n) {
    *why = "layer " + std::to_string(n) + " (" + m->layers[n].name + ") follows FC2, the MNIST network ends there";
    return FLEET_ERR_ARG;
  }
  // a chain: every layer feeds the next and nothing else
  if (m->edge_w_size.size() != n - 1 || m->dims.size() != 12) {
    *why = "the layer graph is not the chain I1 - C1 - P1 - C2i - C2 - P2 - FC2";
    return FLEET_ERR_ARG;
  }
  static const int32_t dims[12] = {5, 5, 8, 1, 1, 128, 5, 5, 768, 192, 10, 1};
  for (int i = 0; i < 12; ++i)
    if (m->dims[(size_t)i] != dims[i]) {
      *why = "the layer graph is not the chain I1 - C1 - P1 - C2i - C2 - P2 - FC2";
      return FLEET_ERR_ARG;
    }
  return FLEET_OK;
}

int fleet::cifar_check(const fleet_model* m, int* classes, std::string* why) {
  struct Want {
    const char *name, *type, *act;
    long args[3];
    int n_args;
  };
  static const Want want[] = {{"I1", "input", "identity", {32, 32, 3}, 3},
                              {"C1", "convolution", "elu", {3, 16, 1}, 3},
                              {"P1", "max_pool", "", {3, 2, 0}, 2},
                              {"C2", "convolution", "elu", {3, 64, 1}, 3},
                              {"P2", "max_pool", "", {4, 4, 0}, 2},
                              {"local4", "fully_connected", "relu", {384, 0, 0}, 1},
                              {"local5", "fully_connected", "relu", {192, 0, 0}, 1},
                              {"FC2", "fully_connected", "softmax", {10, 0, 0}, 1}};
  const size_t n = sizeof want / sizeof want[0];
  auto config = [](const std::string& type, const std::vector<long>& args, const std::string& act) {
    std::string s = type;
    for (long a : args) s += " " + std::to_string(a);
    return act.empty() ? s : s + " " + act;
  };
  const char* chain = "the layer graph is not the chain I1 - C1 - P1 - C2 - P2 - local4 - local5 - FC2";
  int N = 0;
  for (size_t k = 0; k < n; ++k) {
    const Want& W = want[k];
    const bool head = k + 1 == n;  // FC2: 10 or 100 outputs
    const std::string expect = config(W.type, std::vector<long>(W.args, W.args + W.n_args), W.act) + (head ? " (or 100)" : "");
    if (k >= m->layers.size()) {
      *why = std::string("layer ") + std::to_string(k) + " (" + W.name + " " + expect + ") is missing";
      return FLEET_ERR_ARG;
    }
    const Layer& L = m->layers[k];
    const bool act_ok = L.act == W.act || (k == 0 && L.act.empty());
    bool args_ok = L.args == std::vector<long>(W.args, W.args + W.n_args);
    if (head && L.args.size() == 1 && L.args[0] == 100) args_ok = true;
    if (L.type != W.type || !act_ok || !args_ok) {
      *why = "layer " + std::to_string(k) + " is " + L.name + " " + config(L.type, L.args, L.act) + ", the CIFAR network has " +
             W.name + " " + expect;
      return FLEET_ERR_ARG;
    }
    if (head) N = (int)L.args[0];
  }
  if (m->layers.size() != n) {
    *why = "layer " + std::to_string(n) + " (" + m->layers[n].name + ") follows FC2, the CIFAR network ends there";
    return FLEET_ERR_ARG;
  }
  // a chain: every layer feeds the next and nothing else
  const int32_t dims[15] = {3, 3, 48, 3, 3, 1024, 576, 384, 1, 384, 192, 1, 192, N, 1};
  if (m->edge_w_size.size() != n - 1 || m->dims.size() != 15) {
    *why = chain;
    return FLEET_ERR_ARG;
  }
  for (int i = 0; i < 15; ++i)
    if (m->dims[(size_t)i] != dims[i]) {
      *why = chain;
      return FLEET_ERR_ARG;
    }
  *classes = N;
  return FLEET_OK;
}

namespace {

size_t n_weights(const fleet_model* m) {
  size_t n = 0;
  for (int32_t s : m->edge_w_size) n += (size_t)s;
  return n;
}

// descentNative's model copy: new network reading getParams() of `cnn`
// (mode 1: fleet_model_version's dictionary + %g/strtof; mode 0: %g/strtof of every value)
int version_of(fleet_model* m, const Version& v, Version* out) {
  out->w.assign(v.w.size(), 0.0f);
  out->b.assign(v.b.size(), 0.0f);
  if (m->mode) {
    const int rc = fleet_model_version(m->ctx, v.w.data(), m->dims.data(), (int)(m->dims.size() / 3), v.b.data(),
                                       v.b.size(), out->w.data(), out->b.data());
    if (rc) return mfail(m, rc, "model version copy: %s", fleet_last_error(m->ctx));
    return FLEET_OK;
  }
  auto rt = [](float x) {
    char buf[64];
    snprintf(buf, sizeof buf, "%g", (double)x);
    return strtof(buf, nullptr);
  };
  for (size_t i = 0; i < v.w.size(); ++i) out->w[i] = rt(v.w[i]);
  for (size_t i = 0; i < v.b.size(); ++i) out->b[i] = rt(v.b[i]);
  return FLEET_OK;
}

int copy_out(fleet_model* m, const std::string& s, char* out, size_t cap, size_t* out_len) {
  if (out_len) *out_len = s.size();
  if (!out || cap < s.size()) return mfail(m, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, s.size());
  std::memcpy(out, s.data(), s.size());
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_model_load(fleet_ctx* ctx, const char* text, size_t len, int distillation_mode, fleet_model** out) {
  if (!ctx || !out || (!text && len)) return FLEET_ERR_ARG;
  *out = nullptr;
  fleet_model* m = new fleet_model();
  m->ctx = ctx;
  m->mode = distillation_mode ? 1 : 0;
  const int rc = parse(m, std::string(text, len), &m->cnn.w, &m->cnn.b);
  if (rc) {
    std::fprintf(stderr, "[fleet] fleet_model_load: %s\n", m->err.c_str());
    delete m;
    return rc;
  }
  *out = m;
  return FLEET_OK;
}

void fleet_model_destroy(fleet_model* m) { delete m; }

const char* fleet_model_last_error(const fleet_model* m) { return m ? m->err.c_str() : "no model"; }

int fleet_model_init_updater(fleet_model* m, const double* lrates, int n_lrates) {
  if (!m || n_lrates <= 0 || !lrates) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  m->lrates.assign(lrates, lrates + n_lrates);
  m->lr = (float)m->lrates[0];
  Version v;
  const int rc = version_of(m, m->cnn, &v);
  if (rc) return rc;
  m->models.push_back(std::move(v));
  m->pushed++;
  m->priority = 0;
  m->epoch = 0;
  return FLEET_OK;
}

int fleet_model_descent(fleet_model* m, const char* merged, size_t len, int client_batch_size, int stale_size) {
  (void)client_batch_size;  // cnn.set_mini_batch_size: sizes dW storage only, no arithmetic effect
  if (!m || (!merged && len)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  std::vector<float> g(fleet_b64_count(len) + 1);
  size_t n = 0;
  int rc = fleet_decode_f32(m->ctx, merged, len, g.data(), g.size(), &n);
  if (rc) return mfail(m, rc, "descent: %s", fleet_last_error(m->ctx));
  if (m->epoch < (int)m->lrates.size()) m->lr = (float)m->lrates[(size_t)m->epoch];
  // the gradients() layout the merged vector carries (network::descent(vector) walks it)
  std::vector<int32_t> w_sizes, b_sizes;
  size_t idx = 0;
  auto take = [&](int32_t* v) {
    if (idx >= n) return false;
    const float f = g[idx++];
    if (!(std::fabs(f) < 2147483648.0f)) return false;
    *v = (int32_t)f;
    return true;
  };
  int32_t nw = 0, nb = 0, s = 0;
  if (!take(&nw) || nw != (int32_t)m->edge_w_size.size())
    return mfail(m, FLEET_ERR_LAYOUT, "descent: %d weight blocks for a model with %zu graph edges", nw,
                 m->edge_w_size.size());
  for (int32_t i = 0; i < nw; ++i) {
    if (!take(&s) || s < 0 || idx + (size_t)s > n) return mfail(m, FLEET_ERR_LAYOUT, "descent: bad weight block %d", i);
    w_sizes.push_back(s);
    idx += (size_t)s;
  }
  if (!take(&nb) || nb != (int32_t)m->layers.size())
    return mfail(m, FLEET_ERR_LAYOUT, "descent: %d bias blocks for a model with %zu layers", nb, m->layers.size());
  for (int32_t k = 0; k < nb; ++k) {
    if (!take(&s) || s < 0 || idx + (size_t)s > n) return mfail(m, FLEET_ERR_LAYOUT, "descent: bad bias block %d", k);
    b_sizes.push_back(s);
    idx += (size_t)s;
  }
  std::vector<uint8_t> w_present(m->edge_w_size.size());
  for (size_t i = 0; i < w_present.size(); ++i) w_present[i] = m->edge_w_size[i] > 0;
  // the fully-connected layers' biases (update_bias) out of the use_bias() block
  std::vector<float> fcb;
  size_t o = 0;
  for (const Layer& L : m->layers) {
    if (L.use_bias && L.fc) fcb.insert(fcb.end(), m->cnn.b.begin() + (long)o, m->cnn.b.begin() + (long)(o + L.bias_size));
    o += L.use_bias ? L.bias_size : 0;
  }
  if (m->solver == FLEET_SOLVER_SGD)
    rc = fleet_descent(m->ctx, m->cnn.w.data(), m->cnn.w.size(), fcb.data(), fcb.size(), g.data(), n, w_sizes.data(),
                       w_present.data(), nw, b_sizes.data(), m->fc.data(), nb, m->lr);
  else
    rc = fleet::descent_solver_host(m->ctx, m->solver, fleet::kServerResets, m->cnn.w.data(), m->cnn.w.size(), m->g1.data(), m->g2.data(),
                                    fcb.data(), fcb.size(), g.data(), n, w_sizes.data(), w_present.data(), nw,
                                    b_sizes.data(), m->fc.data(), nb, m->lr);
  if (rc) return mfail(m, rc, "descent: %s", fleet_last_error(m->ctx));
  m->stepped = true;
  o = 0;
  size_t f = 0;
  for (const Layer& L : m->layers) {
    if (L.use_bias && L.fc) {
      std::memcpy(m->cnn.b.data() + o, fcb.data() + f, sizeof(float) * L.bias_size);
      f += L.bias_size;
    }
    o += L.use_bias ? L.bias_size : 0;
  }
  m->epoch++;
  Version v;
  if ((rc = version_of(m, m->cnn, &v))) return rc;
  m->models.push_back(std::move(v));
  m->pushed++;
  if (m->models.size() > (size_t)std::max(0, stale_size)) m->models.pop_front();
  return FLEET_OK;
}

int fleet_model_set_solver(fleet_model* m, const char* name) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  const int sv = fleet_solver_from_name(name);
  if (sv < 0) return mfail(m, FLEET_ERR_ARG, "set_solver: no solver \"%s\" (sgd, adagrad, rmsprop, adam)", name ? name : "(null)");
  if (m->stepped) return mfail(m, FLEET_ERR_ARG, "set_solver: the model has been stepped");
  m->solver = sv;
  m->g1.assign(sv != FLEET_SOLVER_SGD ? m->cnn.w.size() : 0, 0.0f);
  m->g2.assign(sv == FLEET_SOLVER_ADAM ? m->cnn.w.size() : 0, 0.0f);
  return FLEET_OK;
}

int fleet_model_solver(fleet_model* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return m->solver;
}

int fleet_model_solver_state(fleet_model* m, int which, float* out, size_t cap) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (which < 0 || which > 1 || m->solver == FLEET_SOLVER_SGD || (which == 1 && m->solver != FLEET_SOLVER_ADAM))
    return mfail(m, FLEET_ERR_ARG, "solver_state: solver %d keeps no state row %d", m->solver, which);
  const std::vector<float>& g = which ? m->g2 : m->g1;
  if (cap < g.size() || (g.size() && !out)) return mfail(m, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, g.size());
  if (!g.empty()) std::memcpy(out, g.data(), sizeof(float) * g.size());
  return FLEET_OK;
}

int fleet_model_count(fleet_model* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return (int)m->models.size();
}

int fleet_model_get_params(fleet_model* m, int version, char* out, size_t cap, size_t* out_len) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (version < 0 || (size_t)version >= m->models.size())
    return mfail(m, FLEET_ERR_ARG, "model version %d of %zu", version, m->models.size());
  const Version& v = m->models[(size_t)version];
  std::string s = m->header;
  size_t o = 0;
  for (const Layer& L : m->layers) {
    if (!L.use_bias) continue;
    for (size_t k = 0; k < L.bias_size; ++k) {
      put_float(s, v.b[o + k]);
      s += ' ';
    }
    s += '\n';
    o += L.bias_size;
  }
  if (m->mode) {
    // save_model_weights, quantization_weight_model, getParams, load_model_weights:
    // the quantised weights' dictionary section; the version itself is not modified
    size_t need = 0;
    const int nm = (int)(m->dims.size() / 3);
    int rc = fleet_model_weights_text(m->ctx, v.w.data(), m->dims.data(), nm, nullptr, 0, &need);
    if (rc && rc != FLEET_ERR_CAPACITY) return mfail(m, rc, "getParams: %s", fleet_last_error(m->ctx));
    std::vector<char> buf(need + 1);
    rc = fleet_model_weights_text(m->ctx, v.w.data(), m->dims.data(), nm, buf.data(), buf.size(), &need);
    if (rc) return mfail(m, rc, "getParams: %s", fleet_last_error(m->ctx));
    s.append(buf.data(), need);
  } else {
    size_t w0 = 0;
    for (int32_t sz : m->edge_w_size) {
      if (!sz) continue;
      for (int32_t i = 0; i < sz; ++i) {
        put_float(s, v.w[w0 + (size_t)i]);
        s += ' ';
      }
      s += '\n';
      w0 += (size_t)sz;
    }
  }
  return copy_out(m, s, out, cap, out_len);
}

int fleet_model_get_model_params(fleet_model* m, int version, char* out, size_t cap, size_t* out_len) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (version < 0 || (size_t)version >= m->models.size())
    return mfail(m, FLEET_ERR_ARG, "model version %d of %zu", version, m->models.size());
  const Version& v = m->models[(size_t)version];
  const int rc = fleet_model_params(m->ctx, v.w.data(), v.w.size(), v.b.data(), v.b.size(),
                                    (int)m->edge_w_size.size(), out, cap, out_len);
  if (rc) return mfail(m, rc, "getModelParams: %s", fleet_last_error(m->ctx));
  return FLEET_OK;
}

int fleet_model_get_epoch(fleet_model* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return m->epoch;
}
void fleet_model_set_epoch(fleet_model* m, int epoch) {
  if (!m) return;
  std::lock_guard<std::mutex> lk(m->mu);
  m->epoch = epoch;
}
int fleet_model_get_priority(fleet_model* m) {
  if (!m) return 0;
  std::lock_guard<std::mutex> lk(m->mu);
  return m->priority;
}
void fleet_model_set_priority(fleet_model* m, int p) {
  if (!m) return;
  std::lock_guard<std::mutex> lk(m->mu);
  m->priority = p;
}
double fleet_model_get_lrate(fleet_model* m) {
  if (!m) return 0.0;
  std::lock_guard<std::mutex> lk(m->mu);
  return (double)m->lr;
}

int fleet_model_evaluate(fleet_model* m, int version, const float* images, size_t n_images, int F,
                         const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                         int32_t* correct, int32_t* pred, float* prob) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (!images || !labels || B <= 0 || F < 28 * 28 || n_images == 0)
    return mfail(m, FLEET_ERR_ARG, "evaluate: images and labels, B >= 1, F >= 784");
  std::string why;
  if (fleet::eval_check_mnist(m, &why)) return mfail(m, FLEET_ERR_ARG, "evaluate: %s", why.c_str());
  const Version* v = &m->cnn;
  if (version >= 0) {
    if ((size_t)version >= m->models.size()) return mfail(m, FLEET_ERR_ARG, "model version %d of %zu", version, m->models.size());
    v = &m->models[(size_t)version];
  }
  const int rc = fleet_evaluate(m->ctx, v->w.data(), v->w.size(), v->b.data(), v->b.size(), images, n_images, F, labels, idx,
                                B, error, accuracy, correct, pred, prob);
  if (rc) return mfail(m, rc, "evaluate: %s", m->ctx ? fleet_last_error(m->ctx) : "the model has no device context");
  return FLEET_OK;
}

int fleet_model_cifar_test(fleet_model* m, int version, const float* images, size_t n_images, int F,
                           const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                           int32_t* correct, int32_t* pred, float* prob) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (!images || !labels || B <= 0 || F < 3 * 32 * 32 || n_images == 0)
    return mfail(m, FLEET_ERR_ARG, "cifar test: images and labels, B >= 1, F >= 3072");
  std::string why;
  int classes = 0;
  if (fleet::cifar_check(m, &classes, &why)) return mfail(m, FLEET_ERR_ARG, "cifar test: %s", why.c_str());
  const Version* v = &m->cnn;
  if (version >= 0) {
    if ((size_t)version >= m->models.size()) return mfail(m, FLEET_ERR_ARG, "model version %d of %zu", version, m->models.size());
    v = &m->models[(size_t)version];
  }
  const int rc = fleet_cifar_test(m->ctx, classes, v->w.data(), v->w.size(), v->b.data(), v->b.size(), images, n_images, F,
                                  labels, idx, B, error, accuracy, correct, pred, prob, nullptr, nullptr);
  if (rc) return mfail(m, rc, "cifar test: %s", m->ctx ? fleet_last_error(m->ctx) : "the model has no device context");
  return FLEET_OK;
}

int fleet_model_export(fleet_model* m, int version, float* weights, size_t n_weights, float* biases, size_t n_biases) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  const Version* v = &m->cnn;
  if (version >= 0) {
    if ((size_t)version >= m->models.size()) return mfail(m, FLEET_ERR_ARG, "model version %d", version);
    v = &m->models[(size_t)version];
  }
  if (n_weights != v->w.size() || n_biases != v->b.size())
    return mfail(m, FLEET_ERR_ARG, "model holds %zu weights and %zu biases", v->w.size(), v->b.size());
  if (n_weights) std::memcpy(weights, v->w.data(), sizeof(float) * n_weights);
  if (n_biases) std::memcpy(biases, v->b.data(), sizeof(float) * n_biases);
  return FLEET_OK;
}

int fleet_model_shape(fleet_model* m, size_t* n_weights_out, size_t* n_biases_out, int* graph_edges, int* n_layers) {
  if (!m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (n_weights_out) *n_weights_out = n_weights(m);
  if (n_biases_out) *n_biases_out = m->cnn.b.size();
  if (graph_edges) *graph_edges = (int)m->edge_w_size.size();
  if (n_layers) *n_layers = (int)m->layers.size();
  return FLEET_OK;
}

int fleet_model_version_id(fleet_model* m, int version, int64_t* id) {
  if (!m || !id) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (version < 0 || (size_t)version >= m->models.size())
    return mfail(m, FLEET_ERR_ARG, "model version %d of %zu", version, m->models.size());
  *id = m->pushed - (int64_t)m->models.size() + version;
  return FLEET_OK;
}

int fleet_mledger_stage_model(fleet_mledger* ledger, fleet_model* m, int version, int64_t* id) {
  if (!ledger || !m) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(m->mu);
  if (version < 0 || (size_t)version >= m->models.size())
    return mfail(m, FLEET_ERR_ARG, "model version %d of %zu", version, m->models.size());
  size_t nw = 0, nb = 0;
  int edges = 0;
  int rc = fleet_mledger_shape(ledger, &nw, &nb, &edges, nullptr, nullptr);
  if (rc) return rc;
  const Version& v = m->models[(size_t)version];
  if (nw != v.w.size() || nb != v.b.size() || edges != (int)m->edge_w_size.size())
    return mfail(m, FLEET_ERR_ARG, "the ledger holds %zu weights, %zu biases, %d edges; the model %zu, %zu, %zu", nw, nb,
                 edges, v.w.size(), v.b.size(), m->edge_w_size.size());
  const int64_t vid = m->pushed - (int64_t)m->models.size() + version;
  if ((rc = fleet_mledger_stage(ledger, vid, v.w.data(), v.b.data())))
    return mfail(m, rc, "stage_model: %s", fleet_last_error(m->ctx));
  if (id) *id = vid;
  return FLEET_OK;
}

}  // extern "C"

// tests/native/check_cifar_forward.cpp -- the CIFAR evaluation's host mirror
// (fleet_amd/csrc/cifar_forward.h: cifar_forward_host, cifar_reduce_host, the functions
// k_cifar_forward runs per lane) against tests/golden/cifar_ref.npz, the Driver's test() on
// the CIFAR network recorded from the reference's own network class.
//
//   check_cifar_forward <cifar_ref.bin>
//
// reads the fixture as the flat file tests/cifar_ref.py write_flat() makes of it and, per
// case, compares pred, p, cost and the kept probabilities of every image, every layer's
// node of the images that have them, and error, accuracy and correct of every prefix length
// (and of the recorded permutation): bitwise for contract-1 cases; for contract-2 cases
// (NaN inputs) NaN at the same positions and every other value bitwise.
//
//   check_cifar_forward --mirror <jobs.bin> <out.bin>
//
// runs the host form over jobs (tests/cifar_ref.py mirror() writes them and reads the
// results), for the shapes the fixture does not hold. Stand-alone, so it also runs under
// the host sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fleet_amd/csrc/cifar_forward.h"

namespace {

using namespace fleet::cifarnet;
using fleet::evalnet::Verdict;

uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }

bool same(int contract, float got, float want) {
  if (contract == 1) return bits(got) == bits(want);
  return (got != got) == (want != want) && (want != want || bits(got) == bits(want));
}

constexpr int kLayerFloats = kC1Out + kP1Out + kC2Out + kFcIn + kFc4 + kFc5;  // and N for FC2

struct Case {
  std::string name;
  int contract = 1, N = 10, B = 0, n_probs = 0, has_perm = 0, n_layers = 0;
  std::vector<float> w, b, x, p, cost, probs, error, accuracy, layers;
  std::vector<int32_t> labels, pred, correct, perm;
  float perm_error = 0, perm_accuracy = 0;
  int32_t perm_correct = 0;
};

template <typename T>
bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

bool read_cases(const char* path, std::vector<Case>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n > 0 && n < 1000;
  for (int i = 0; ok && i < n; ++i) {
    Case c;
    int32_t len = 0, hdr[6];
    ok = std::fread(&len, 4, 1, f) == 1 && len > 0 && len < 256;
    if (!ok) break;
    c.name.resize(len);
    ok = std::fread(&c.name[0], 1, len, f) == (size_t)len && std::fread(hdr, 4, 6, f) == 6 && classes_ok(hdr[1]) &&
         hdr[2] > 0 && hdr[2] <= 100000 && hdr[3] >= 0 && hdr[3] <= hdr[2] && hdr[5] >= 0 && hdr[5] <= hdr[2];
    if (!ok) break;
    c.contract = hdr[0], c.N = hdr[1], c.B = hdr[2], c.n_probs = hdr[3], c.has_perm = hdr[4], c.n_layers = hdr[5];
    const size_t B = (size_t)c.B;
    ok = get(f, c.w, weight_count(c.N)) && get(f, c.b, bias_count(c.N)) && get(f, c.x, B * kPix) && get(f, c.labels, B) &&
         get(f, c.pred, B) && get(f, c.p, B) && get(f, c.cost, B) && get(f, c.probs, (size_t)c.n_probs * c.N) &&
         get(f, c.error, B) && get(f, c.accuracy, B) && get(f, c.correct, B) &&
         get(f, c.layers, (size_t)c.n_layers * (kLayerFloats + c.N));
    if (ok && c.has_perm)
      ok = get(f, c.perm, B) && std::fread(&c.perm_error, 4, 1, f) == 1 && std::fread(&c.perm_accuracy, 4, 1, f) == 1 &&
           std::fread(&c.perm_correct, 4, 1, f) == 1;
    for (int32_t v : c.perm) ok = ok && v >= 0 && v < c.B;
    out.push_back(std::move(c));
  }
  std::fclose(f);
  return ok;
}

int run_case(const Case& c) {
  int bad = 0;
  const size_t B = (size_t)c.B;
  std::vector<int32_t> pred(B);
  std::vector<float> p(B), cost(B), node((size_t)kLayerFloats + c.N);
  for (size_t k = 0; k < B; ++k) {
    float probs[kMaxClasses];
    Layers keep;
    const bool layers = (int)k < c.n_layers;
    if (layers) {
      float* q = node.data();
      keep.c1 = q, q += kC1Out;
      keep.p1 = q, q += kP1Out;
      keep.c2 = q, q += kC2Out;
      keep.p2 = q, q += kFcIn;
      keep.local4 = q, q += kFc4;
      keep.local5 = q, q += kFc5;
      keep.fc2 = q;
    }
    const Verdict v = cifar_forward_host(c.w.data(), c.b.data(), c.N, c.x.data() + k * kPix, c.labels[k], probs,
                                         layers ? &keep : nullptr);
    pred[k] = v.pred, p[k] = v.p, cost[k] = v.cost;
    bad += v.pred != c.pred[k];
    bad += !same(c.contract, v.p, c.p[k]);
    bad += !same(c.contract, v.cost, c.cost[k]);
    if ((int)k < c.n_probs)
      for (int j = 0; j < c.N; ++j) bad += !same(c.contract, probs[j], c.probs[k * c.N + j]);
    if (layers)
      for (size_t i = 0; i < node.size(); ++i) bad += !same(c.contract, node[i], c.layers[k * node.size() + i]);
  }
  for (int n = 1; n <= c.B; ++n) {  // every prefix: test(..., sample = n)
    float error, accuracy;
    int32_t correct;
    cifar_reduce_host(cost.data(), pred.data(), c.labels.data(), nullptr, n, &error, &accuracy, &correct);
    bad += !same(c.contract, error, c.error[n - 1]);
    bad += !same(c.contract, accuracy, c.accuracy[n - 1]);
    bad += correct != c.correct[n - 1];
  }
  if (c.has_perm) {
    std::vector<float> pc(B);
    std::vector<int32_t> pp(B);
    for (size_t k = 0; k < B; ++k) pc[k] = cost[c.perm[k]], pp[k] = pred[c.perm[k]];
    float error, accuracy;
    int32_t correct;
    cifar_reduce_host(pc.data(), pp.data(), c.labels.data(), c.perm.data(), c.B, &error, &accuracy, &correct);
    bad += !same(c.contract, error, c.perm_error);
    bad += !same(c.contract, accuracy, c.perm_accuracy);
    bad += correct != c.perm_correct;
  }
  return bad;
}

// jobs: int32 n, then per job int32 N, B, rows, has_idx; w, b, x[rows*3072], labels[rows], idx[B].
// out: per job pred[B], p[B], cost[B], probs[B*N], error, accuracy, correct
int run_mirror(const char* in_path, const char* out_path) {
  FILE* f = std::fopen(in_path, "rb");
  FILE* out = std::fopen(out_path, "wb");
  if (!f || !out) return 2;
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n > 0 && n < 10000;
  for (int i = 0; ok && i < n; ++i) {
    int32_t hdr[4];
    ok = std::fread(hdr, 4, 4, f) == 4 && classes_ok(hdr[0]) && hdr[1] > 0 && hdr[1] <= 1000000 && hdr[2] > 0 &&
         hdr[2] <= 1000000 && (hdr[3] || hdr[1] <= hdr[2]);
    if (!ok) break;
    const int N = hdr[0], B = hdr[1];
    const size_t rows = (size_t)hdr[2];
    std::vector<float> w, b, x;
    std::vector<int32_t> labels, idx;
    ok = get(f, w, weight_count(N)) && get(f, b, bias_count(N)) && get(f, x, rows * kPix) && get(f, labels, rows) &&
         (!hdr[3] || get(f, idx, (size_t)B));
    for (int32_t v : idx) ok = ok && v >= 0 && (size_t)v < rows;
    if (!ok) break;
    std::vector<int32_t> pred(B);
    std::vector<float> p(B), cost(B), probs((size_t)B * N);
    for (int k = 0; k < B; ++k) {
      const size_t row = hdr[3] ? (size_t)idx[k] : (size_t)k;
      const Verdict v = cifar_forward_host(w.data(), b.data(), N, x.data() + row * kPix, labels[row], &probs[(size_t)k * N]);
      pred[k] = v.pred, p[k] = v.p, cost[k] = v.cost;
    }
    float error, accuracy;
    int32_t correct;
    cifar_reduce_host(cost.data(), pred.data(), labels.data(), hdr[3] ? idx.data() : nullptr, B, &error, &accuracy, &correct);
    std::fwrite(pred.data(), 4, B, out);
    std::fwrite(p.data(), 4, B, out);
    std::fwrite(cost.data(), 4, B, out);
    std::fwrite(probs.data(), 4, probs.size(), out);
    std::fwrite(&error, 4, 1, out);
    std::fwrite(&accuracy, 4, 1, out);
    std::fwrite(&correct, 4, 1, out);
  }
  std::fclose(f);
  return std::fclose(out) == 0 && ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--mirror")) return run_mirror(argv[2], argv[3]);
  if (argc != 2) {
    std::fprintf(stderr, "usage: check_cifar_forward cifar_ref.bin | --mirror jobs.bin out.bin\n");
    return 2;
  }
  std::vector<Case> cases;
  if (!read_cases(argv[1], cases)) {
    std::fprintf(stderr, "cannot read the fixture\n");
    return 2;
  }
  int failures = 0;
  for (const Case& c : cases) {
    const int bad = run_case(c);
    std::printf("reproduce %-14s contract %d classes %d images %d: %s (%d values differ)\n", c.name.c_str(), c.contract,
                c.N, c.B, bad ? "MISMATCH" : "ok", bad);
    failures += bad != 0;
  }
  std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
  return failures ? 1 : 0;
}

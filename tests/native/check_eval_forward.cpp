// tests/native/check_eval_forward.cpp -- the evaluation's host mirror
// (fleet_amd/csrc/eval_forward.h: eval_forward_host, eval_reduce_host, the functions
// k_eval_forward and k_eval_reduce run per lane) against tests/golden/eval_ref.npz, the
// Driver's test() recorded from the reference's own network class.
//
//   check_eval_forward <eval_ref.bin>
//
// reads the fixture as the flat file tests/eval_ref.py write_flat() makes of it and, per
// case, compares pred, p, cost and the kept probabilities of every image, and error,
// accuracy and correct of every prefix length (and of the recorded permutation):
// bitwise for contract-1 cases; for contract-2 cases (NaN inputs) NaN at the same
// positions and every other value bitwise. Stand-alone, so it also runs under the
// host sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fleet_amd/csrc/eval_forward.h"

namespace {

using namespace fleet::evalnet;

uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }

bool same(int contract, float got, float want) {
  if (contract == 1) return bits(got) == bits(want);
  return (got != got) == (want != want) && (want != want || bits(got) == bits(want));
}

struct Case {
  std::string name;
  int contract = 1, B = 0, n_probs = 0, has_perm = 0;
  std::vector<float> w, b, x, p, cost, probs, error, accuracy;
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
    int32_t len = 0, hdr[4];
    ok = std::fread(&len, 4, 1, f) == 1 && len > 0 && len < 256;
    if (!ok) break;
    c.name.resize(len);
    ok = std::fread(&c.name[0], 1, len, f) == (size_t)len && std::fread(hdr, 4, 4, f) == 4 && hdr[1] > 0 &&
         hdr[1] <= 100000 && hdr[2] >= 0 && hdr[2] <= hdr[1];
    if (!ok) break;
    c.contract = hdr[0], c.B = hdr[1], c.n_probs = hdr[2], c.has_perm = hdr[3];
    const size_t B = (size_t)c.B;
    ok = get(f, c.w, kWTotal) && get(f, c.b, kBTotal) && get(f, c.x, B * kPix) && get(f, c.labels, B) && get(f, c.pred, B) &&
         get(f, c.p, B) && get(f, c.cost, B) && get(f, c.probs, (size_t)c.n_probs * kClasses) && get(f, c.error, B) &&
         get(f, c.accuracy, B) && get(f, c.correct, B);
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
  std::vector<float> p(B), cost(B);
  for (size_t k = 0; k < B; ++k) {
    float probs[kClasses];
    const Verdict v = eval_forward_host(c.w.data(), c.b.data(), c.x.data() + k * kPix, c.labels[k], probs);
    pred[k] = v.pred, p[k] = v.p, cost[k] = v.cost;
    bad += v.pred != c.pred[k];
    bad += !same(c.contract, v.p, c.p[k]);
    bad += !same(c.contract, v.cost, c.cost[k]);
    if ((int)k < c.n_probs)
      for (int j = 0; j < kClasses; ++j) bad += !same(c.contract, probs[j], c.probs[k * kClasses + j]);
  }
  for (int n = 1; n <= c.B; ++n) {  // every prefix: test(..., sample = n)
    float error, accuracy;
    int32_t correct;
    eval_reduce_host(cost.data(), pred.data(), c.labels.data(), nullptr, n, &error, &accuracy, &correct);
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
    eval_reduce_host(pc.data(), pp.data(), c.labels.data(), c.perm.data(), c.B, &error, &accuracy, &correct);
    bad += !same(c.contract, error, c.perm_error);
    bad += !same(c.contract, accuracy, c.perm_accuracy);
    bad += correct != c.perm_correct;
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: check_eval_forward eval_ref.bin\n");
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
    std::printf("reproduce %-14s contract %d images %d: %s (%d values differ)\n", c.name.c_str(), c.contract, c.B,
                bad ? "MISMATCH" : "ok", bad);
    failures += bad != 0;
  }
  std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
  return failures ? 1 : 0;
}

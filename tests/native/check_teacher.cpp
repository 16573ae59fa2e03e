// tests/native/check_teacher.cpp -- host census and mutants of the sampler's mode-1
// teacher forward (fleet_amd/csrc/teacher.hip k_teacher_forward). The forward below
// is the kernel's loop nest in plain C++ over the functions of teacher_math.h (host
// + device), so the arithmetic checked here is the code the GPU runs.
//
//   check_teacher <teacher_mnist.bin> <teacher_edges.bin>
//
// reads the two fixtures as the flat files tests/teacher_edges.py write_flat() makes
// of them. Built plain (MUTANT 0) it
//   * reproduces every recorded probability of the reference's network: bitwise for
//     contract-1 cases (no NaN among the inputs); for contract-2 cases (NaN inputs)
//     NaN at the same positions and every other value bitwise;
//   * prints a census of the data-dependent branches per pooling layer, of elu, expf
//     and the softmax, per fixture, and fails unless teacher_edges alone visits every
//     branch listed in `required` below;
//   * checks its own observer: the pick it predicts for each pooling window is the
//     value mojo_semi_pool returned.
// Built with -DMUTANT=k (1..11) the forward carries one deliberate error (the pooling
// ones in P1 only / P2 only with -DMUTANT_POOL=1 / 2); it runs
// teacher_edges only and reports the mutant KILLED when a recorded output bit or a
// NaN position changes, SURVIVED otherwise (exit status 1). For the comparison
// mutants it also counts the windows whose picked index / picked bits differ.
// Mutants are arithmetic restated here; none of them lives in fleet_amd/csrc.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fleet_amd/csrc/teacher_math.h"

#ifndef MUTANT
#define MUTANT 0
#endif
#ifndef MUTANT_POOL  // 0: the pooling mutants act on P1 and P2, 1: on P1 only, 2: on P2 only
#define MUTANT_POOL 0
#endif

[[maybe_unused]] static const char* const kMutantNames[] = {
    "none",
    "pool: denom == 0 test removed",
    "pool: always the largest",
    "pool: `mx < v` became `mx <= v`",
    "pool: `mx2 < v` became `mx2 <= v`",
    "pool: mx2 starts at -inf instead of v[0]",
    "pool: (int) as a saturating cast, NaN -> 0 (a bare device cast)",
    "elu: `v < 0` became `v <= 0`",
    "softmax: max scan without the reference's /T quirk",
    "subnormal results flushed to zero after every operation",
    "C2i: input channels in reverse order",
    "C2: tap loop outside the channel loop",
};

namespace {

constexpr int kIn = 28, kC1 = 24, kP1 = 8, kC2 = 4, kP2 = 2;
constexpr int kMaps1 = 8, kMaps2i = 16, kMaps2 = 48, kClasses = 10, kFcIn = 192;
constexpr int kW1 = 0, kW2i = 200, kW2 = 328, kWfc = 19528, kWTotal = 21448;
constexpr int kB1 = 0, kB2i = 8, kB2 = 24, kBTotal = 82;

uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// ---- census ---------------------------------------------------------------
#define POOL_FIELDS(X)                                                                                         \
  X(windows) X(second_pick) X(second_pick_other_slot) X(second_pick_other_bits) X(denom_zero)                   \
  X(denom_zero_other_bits) X(all_equal) X(largest_is_zero) X(nan_slot0) X(nan_other_slot) X(inf_any_slot)      \
  X(nonfinite_other_slot_only) X(cvtt_int_min) X(cvtt_positive_overflow) X(t1_is_8) X(t1_is_9) X(t1_is_10)     \
  X(tie_for_largest) X(negative_zero_value)
#define NET_FIELDS(X)                                                                                          \
  X(elu_calls) X(elu_negative) X(elu_plus_zero) X(elu_minus_zero) X(elu_nan) X(elu_saturated_to_minus_tenth)    \
  X(expf_calls) X(expf_minus_inf) X(expf_inf_or_nan) X(expf_overflow) X(expf_underflow) X(expf_may_underflow)  \
  X(expf_88_or_more_computed) X(subnormal_c1) X(subnormal_p1) X(subnormal_c2i) X(subnormal_c2) X(subnormal_p2) \
  X(subnormal_fc) X(subnormal_prob) X(softmax_rows) X(softmax_in0_is_max) X(softmax_max_replaced)              \
  X(softmax_inf_over_inf) X(softmax_zero_over_zero) X(softmax_row_finite_with_dropped_nonfinite) X(prob_nan) X(prob_zero) X(prob_one)

struct PoolCensus {
#define X(f) long f = 0;
  POOL_FIELDS(X)
#undef X
};
struct Census {
  PoolCensus pool[2];
#define X(f) long f = 0;
  NET_FIELDS(X)
#undef X
  long observer_errors = 0, mutant_index_differs = 0, mutant_bits_differ = 0, mutant_elu_differs = 0;
};

// ---- one pooling window, real or mutated -----------------------------------
struct PoolRule {
  bool no_denom_test = false, always_largest = false, le_first = false, le_second = false, mx2_from_minus_inf = false,
       saturating_cast = false, flush = false;
};

float flush_subnormal(float r) { return std::fpclassify(r) == FP_SUBNORMAL ? std::copysign(0.0f, r) : r; }

int32_t saturating_cast(float x) {  // what a bare `(int)x` gives on the device
  if (x != x) return 0;
  if (x >= 2147483648.0f) return INT32_MAX;
  if (x <= -2147483648.0f) return INT32_MIN;
  return (int32_t)x;
}

struct Scan {
  float mx, mx2, denom, t;
  int mi, mi2, pick;
  int32_t t1;
  bool denom_zero;
};

template <int N>
Scan scan_window(const float (&v)[N], const PoolRule& r) {
  Scan s{};
  s.mx = v[0];
  s.mx2 = r.mx2_from_minus_inf ? -INFINITY : v[0];
  for (int i = 0; i < N; ++i) {
    if (r.le_first ? s.mx <= v[i] : s.mx < v[i]) {
      s.mx2 = s.mx, s.mi2 = s.mi, s.mx = v[i], s.mi = i;
    } else if (r.le_second ? s.mx2 <= v[i] : s.mx2 < v[i]) {
      s.mx2 = v[i], s.mi2 = i;
    }
  }
  auto z = [&](float x) { return r.flush ? flush_subnormal(x) : x; };
  s.denom = z(s.mx + s.mx2);
  s.denom_zero = !r.no_denom_test && s.denom == 0.0f;
  if (s.denom_zero) {
    s.pick = s.mi;
    return s;
  }
  s.t = z(z(100.0f * s.mx) / z(s.mx + s.mx2));
  s.t1 = r.saturating_cast ? saturating_cast(s.t) : fleet::mojo_cvtt(s.t);
  s.pick = (9 <= s.t1 || r.always_largest) ? s.mi : s.mi2;
  return s;
}

[[maybe_unused]] PoolRule mutant_rule() {
  PoolRule r;
  r.no_denom_test = MUTANT == 1, r.always_largest = MUTANT == 2, r.le_first = MUTANT == 3, r.le_second = MUTANT == 4;
  r.mx2_from_minus_inf = MUTANT == 5, r.saturating_cast = MUTANT == 6, r.flush = MUTANT == 9;
  return r;
}

template <int P>
float pool(const float (&v)[P * P], PoolCensus& c, Census& all) {
  const Scan s = scan_window(v, PoolRule{});
#if MUTANT == 0
  const float out = fleet::mojo_semi_pool<P>(v, true);
  if (bits(out) != bits(v[s.pick])) all.observer_errors++;
#else
  const Scan m = scan_window(v, MUTANT_POOL == 0 || (MUTANT_POOL == 1) == (P == 3) ? mutant_rule() : PoolRule{});
  const float out = v[m.pick];
  all.mutant_index_differs += m.pick != s.pick;
  all.mutant_bits_differ += bits(v[m.pick]) != bits(v[s.pick]);
#endif
  c.windows++;
  bool all_eq = true, nan_other = false, inf_any = false, tie = false, neg_zero = false;
  for (int i = 0; i < P * P; ++i) {
    all_eq &= v[i] == v[0];
    nan_other |= i > 0 && v[i] != v[i];
    inf_any |= std::isinf(v[i]);
    tie |= i != s.mi && v[i] == s.mx;
    neg_zero |= bits(v[i]) == 0x80000000u;
  }
  bool nonfinite_other = false;
  for (int i = 1; i < P * P; ++i) nonfinite_other |= !std::isfinite(v[i]);
  c.all_equal += all_eq;
  c.largest_is_zero += s.mx == 0.0f;
  c.nan_slot0 += v[0] != v[0];
  c.nan_other_slot += nan_other;
  c.inf_any_slot += inf_any;
  c.nonfinite_other_slot_only += nonfinite_other && std::isfinite(v[0]);
  c.tie_for_largest += tie;
  c.negative_zero_value += neg_zero;
  if (s.denom_zero) {
    c.denom_zero++;
    c.denom_zero_other_bits += bits(v[s.mi]) != bits(v[s.mi2]);
  } else {
    c.cvtt_int_min += !(std::fabs(s.t) < 2147483648.0f);
    c.cvtt_positive_overflow += s.t >= 2147483648.0f;
    c.t1_is_8 += s.t1 == 8, c.t1_is_9 += s.t1 == 9, c.t1_is_10 += s.t1 == 10;
    if (s.t1 < 9) {
      c.second_pick++;
      c.second_pick_other_slot += s.mi2 != s.mi;
      c.second_pick_other_bits += bits(v[s.mi2]) != bits(v[s.mi]);
    }
  }
  return out;
}

// ---- the forward: k_teacher_forward's loop nest -----------------------------
float Z(float r) { return MUTANT == 9 ? flush_subnormal(r) : r; }
float ADD(float a, float b) { return Z(fleet::mojo_add(a, b)); }
float SUB(float a, float b) { return Z(fleet::mojo_sub(a, b)); }
float MUL(float a, float b) { return Z(fleet::mojo_mul(a, b)); }
float DIV(float a, float b) { return Z(fleet::mojo_div(a, b)); }
// one running sum, as the kernel writes it: sum(mac) runs the loop nest with the step `mac`
template <class Sum>
float SUM(Sum sum) {
#if MUTANT == 9
  return sum([](float acc, float a, float b) { return ADD(acc, MUL(a, b)); });
#else
  return fleet::mojo_sum(sum);
#endif
}

float expf_observed(float x, Census& c) {
  c.expf_calls++;
  const uint32_t ux = bits(x), abstop = (ux >> 20) & 0x7ffu;
  if (abstop >= 0x42bu) {  // the conditions of glibc_expf's early returns, in its order
    if (ux == 0xff800000u) c.expf_minus_inf++;
    else if (abstop >= 0x7f8u) c.expf_inf_or_nan++;
    else if (x > 0x1.62e42ep6f) c.expf_overflow++;
    else if (x < -0x1.9fe368p6f) c.expf_underflow++;
    else if (x < -0x1.9d1d9ep6f) c.expf_may_underflow++;
    else c.expf_88_or_more_computed++;
  }
  return Z(fleet::mojo_expf(x));
}

float elu(float x, float bias, Census& c) {
  const float v = ADD(x, bias);
  c.elu_calls++;
  c.elu_negative += v < 0.0f;
  c.elu_plus_zero += bits(v) == 0u;
  c.elu_minus_zero += bits(v) == 0x80000000u;
  c.elu_nan += v != v;
  float out;
#if MUTANT == 0
  if (v < 0.0f) expf_observed(v, c);
  out = fleet::mojo_elu(x, bias);
#else
  out = (MUTANT == 7 ? v <= 0.0f : v < 0.0f) ? MUL(0.1f, SUB(expf_observed(v, c), 1.0f)) : v;
  if (MUTANT == 7) c.mutant_elu_differs += bits(out) != bits(fleet::mojo_elu(x, bias));
#endif
  c.elu_saturated_to_minus_tenth += out == -0.1f;
  return out;
}

long count_subnormal(const float* a, int n) {
  long k = 0;
  for (int i = 0; i < n; ++i) k += std::fpclassify(a[i]) == FP_SUBNORMAL;
  return k;
}

void forward(const float* w, const float* b, const float* image, float temperature, float* probs, Census& c) {
  static float s_c1[kMaps1 * kC1 * kC1], s_p1[kMaps1 * kP1 * kP1], s_c2i[kMaps2i * kP1 * kP1], s_c2[kMaps2 * kC2 * kC2],
      s_p2[kFcIn], s_fc[kClasses];
  const float* s_in = image;
  // C1: 5x5 over the single input channel, then bias + elu
  for (int o = 0; o < kMaps1 * kC1 * kC1; ++o) {
    const int map = o / (kC1 * kC1), p = o % (kC1 * kC1), y = p / kC1, x = p % kC1;
    const float* wm = w + kW1 + map * 25;
    const float acc = SUM([&](auto mac) {
      float a = 0.0f;
      for (int i = 0; i < 25; ++i) a = mac(a, s_in[(y + i / 5) * kIn + x + i % 5], wm[i]);
      return a;
    });
    s_c1[o] = elu(acc, b[kB1 + map], c);
  }
  // P1: semi-stochastic 3x3 pool, stride 3
  for (int o = 0; o < kMaps1 * kP1 * kP1; ++o) {
    const int k = o / (kP1 * kP1), p = o % (kP1 * kP1), j = 3 * (p / kP1), i = 3 * (p % kP1);
    float v[9];
    for (int q = 0; q < 9; ++q) v[q] = s_c1[k * kC1 * kC1 + (j + q / 3) * kC1 + i + q % 3];
    s_p1[o] = pool<3>(v, c.pool[0], c);
  }
  // C2i: 1x1 over 8 input channels, then bias + elu
  for (int o = 0; o < kMaps2i * kP1 * kP1; ++o) {
    const int map = o / (kP1 * kP1), p = o % (kP1 * kP1);
    const float acc = SUM([&](auto mac) {
      float a = 0.0f;
      for (int kk = 0; kk < kMaps1; ++kk) {
        const int k = MUTANT == 10 ? kMaps1 - 1 - kk : kk;
        a = mac(a, s_p1[k * kP1 * kP1 + p], w[kW2i + map + k * kMaps2i]);
      }
      return a;
    });
    s_c2i[o] = elu(acc, b[kB2i + map], c);
  }
  // C2: 5x5 over 16 input channels (channel outer, tap inner), then bias + elu
  for (int o = 0; o < kMaps2 * kC2 * kC2; ++o) {
    const int map = o / (kC2 * kC2), p = o % (kC2 * kC2), y = p / kC2, x = p % kC2;
    const float acc = SUM([&](auto mac) {
      float a = 0.0f;
      for (int n = 0; n < kMaps2i * 25; ++n) {
        const int k = MUTANT == 11 ? n % kMaps2i : n / 25, i = MUTANT == 11 ? n / kMaps2i : n % 25;
        const float* wm = w + kW2 + (k * kMaps2 + map) * 25;
        const float* src = s_c2i + k * kP1 * kP1;
        a = mac(a, src[(y + i / 5) * kP1 + x + i % 5], wm[i]);
      }
      return a;
    });
    s_c2[o] = elu(acc, b[kB2 + map], c);
  }
  // P2: semi-stochastic 2x2 pool, stride 2
  for (int t = 0; t < kFcIn; ++t) {
    const int k = t / (kP2 * kP2), p = t % (kP2 * kP2), j = 2 * (p / kP2), i = 2 * (p % kP2);
    float v[4];
    for (int q = 0; q < 4; ++q) v[q] = s_c2[k * kC2 * kC2 + (j + q / 2) * kC2 + i + q % 2];
    s_p2[t] = pool<2>(v, c.pool[1], c);
  }
  // FC2: node[j] = 0 + dot(P2, W row j)
  for (int t = 0; t < kClasses; ++t) {
    const float* wr = w + kWfc + t * kFcIn;
    const float v = SUM([&](auto mac) {
      float a = 0.0f;
      for (int i = 0; i < kFcIn; ++i) a = mac(a, s_p2[i], wr[i]);
      return a;
    });
    s_fc[t] = ADD(0.0f, v);
  }
  // softmax with temperature, the reference's order
  const float* in = s_fc;
  float mx = MUTANT == 8 ? DIV(in[0], temperature) : in[0];
  bool replaced = false;
  for (int j = 1; j < kClasses; ++j)
    if (in[j] > mx) mx = MUTANT == 8 ? in[j] : DIV(in[j], temperature), replaced = true;
  float denom = 0.0f;
  for (int j = 0; j < kClasses; ++j) denom = ADD(denom, expf_observed(SUB(DIV(in[j], temperature), mx), c));
  bool inf_over_inf = false, zero_over_zero = false;
  for (int j = 0; j < kClasses; ++j) {
    const float num = expf_observed(SUB(DIV(in[j], temperature), mx), c);
    inf_over_inf |= std::isinf(num) && std::isinf(denom);
    zero_over_zero |= num == 0.0f && denom == 0.0f;
    probs[j] = DIV(num, denom);
  }
  c.subnormal_c1 += count_subnormal(s_c1, kMaps1 * kC1 * kC1), c.subnormal_p1 += count_subnormal(s_p1, kMaps1 * kP1 * kP1);
  c.subnormal_c2i += count_subnormal(s_c2i, kMaps2i * kP1 * kP1), c.subnormal_c2 += count_subnormal(s_c2, kMaps2 * kC2 * kC2);
  c.subnormal_p2 += count_subnormal(s_p2, kFcIn), c.subnormal_fc += count_subnormal(s_fc, kClasses);
  c.subnormal_prob += count_subnormal(probs, kClasses);
  c.softmax_rows++, c.softmax_in0_is_max += !replaced, c.softmax_max_replaced += replaced, c.softmax_inf_over_inf += inf_over_inf;
  c.softmax_zero_over_zero += zero_over_zero;
  for (int j = 0; j < kClasses; ++j) {
    c.prob_nan += probs[j] != probs[j], c.prob_zero += probs[j] == 0.0f, c.prob_one += probs[j] == 1.0f;
  }
}

// ---- fixtures ----------------------------------------------------------------
struct Case {
  std::string name;
  int contract = 1, rows = 0;
  std::vector<float> w, b, x, probs;
};

bool read_cases(const char* path, std::vector<Case>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n > 0 && n < 1000;
  for (int i = 0; ok && i < n; ++i) {
    Case c;
    int32_t len = 0, hdr[2];
    ok = std::fread(&len, 4, 1, f) == 1 && len > 0 && len < 256;
    if (!ok) break;
    c.name.resize(len);
    ok = std::fread(&c.name[0], 1, len, f) == (size_t)len && std::fread(hdr, 4, 2, f) == 2 && hdr[1] > 0 && hdr[1] <= 64;
    if (!ok) break;
    c.contract = hdr[0], c.rows = hdr[1];
    c.w.resize(kWTotal), c.b.resize(kBTotal), c.x.resize((size_t)c.rows * kIn * kIn), c.probs.resize((size_t)c.rows * kClasses);
    for (std::vector<float>* v : {&c.w, &c.b, &c.x, &c.probs}) ok = ok && std::fread(v->data(), 4, v->size(), f) == v->size();
    out.push_back(std::move(c));
  }
  std::fclose(f);
  return ok;
}

// values that differ from the recording under the case's contract
int run_case(const Case& k, Census& c, bool& finite_with_dropped) {
  int bad = 0;
  const PoolCensus before[2] = {c.pool[0], c.pool[1]};
  bool all_finite = true;
  for (int r = 0; r < k.rows; ++r) {
    float p[kClasses];
    forward(k.w.data(), k.b.data(), k.x.data() + (size_t)r * kIn * kIn, 2.0f, p, c);
    for (int j = 0; j < kClasses; ++j) {
      const float want = k.probs[(size_t)r * kClasses + j];
      all_finite &= std::isfinite(want);
      if (k.contract == 1) bad += bits(p[j]) != bits(want);
      else bad += (p[j] != p[j]) != (want != want) || (want == want && bits(p[j]) != bits(want));
    }
  }
  long dropped = 0;
  for (int l = 0; l < 2; ++l) dropped += c.pool[l].nonfinite_other_slot_only - before[l].nonfinite_other_slot_only;
  finite_with_dropped = all_finite && dropped > 0;
  return bad;
}

[[maybe_unused]] void print_census(const char* fixture, const Census& c) {
  for (int l = 0; l < 2; ++l) {
#define X(f) std::printf("census %-6s P%d %-34s %ld\n", fixture, l + 1, #f, c.pool[l].f);
    POOL_FIELDS(X)
#undef X
  }
#define X(f) std::printf("census %-6s net %-34s %ld\n", fixture, #f, c.f);
  NET_FIELDS(X)
#undef X
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: check_teacher teacher_mnist.bin teacher_edges.bin\n");
    return 2;
  }
  std::vector<Case> mnist, edges;
  if (!read_cases(argv[1], mnist) || !read_cases(argv[2], edges)) {
    std::fprintf(stderr, "cannot read the fixtures\n");
    return 2;
  }
  int failures = 0;
#if MUTANT == 0
  Census cm, ce;
  for (int which = 0; which < 2; ++which) {
    Census& c = which ? ce : cm;
    for (const Case& k : which ? edges : mnist) {
      bool fd = false;
      const int bad = run_case(k, c, fd);
      c.softmax_row_finite_with_dropped_nonfinite += fd;
      std::printf("reproduce %-6s %-18s contract %d rows %d: %s (%d values differ)\n", which ? "edges" : "mnist",
                  k.name.c_str(), k.contract, k.rows, bad ? "MISMATCH" : "ok", bad);
      failures += bad != 0;
    }
    print_census(which ? "edges" : "mnist", c);
    if (c.observer_errors) std::printf("OBSERVER ERRORS %ld\n", c.observer_errors), failures++;
  }
  // every branch the kernel has, from teacher_edges alone
  struct Req { std::string what; long n; };
  std::vector<Req> required;
  for (int l = 0; l < 2; ++l) {
    const PoolCensus& p = ce.pool[l];
    auto add = [&](const char* s, long n) { required.push_back({std::string(l ? "P2 " : "P1 ") + s, n}); };
    add("second_pick", p.second_pick), add("second_pick_other_slot", p.second_pick_other_slot);
    add("second_pick_other_bits", p.second_pick_other_bits), add("denom_zero", p.denom_zero);
    add("all_equal", p.all_equal), add("largest_is_zero", p.largest_is_zero), add("nan_slot0", p.nan_slot0);
    add("nan_other_slot", p.nan_other_slot), add("inf_any_slot", p.inf_any_slot), add("cvtt_int_min", p.cvtt_int_min);
  }
  for (int l = 0; l < 2; ++l) {
    required.push_back({std::string(l ? "P2 " : "P1 ") + "denom_zero_other_bits", ce.pool[l].denom_zero_other_bits});
    required.push_back({std::string(l ? "P2 " : "P1 ") + "cvtt_positive_overflow", ce.pool[l].cvtt_positive_overflow});
  }
  required.push_back({"P1 nonfinite_other_slot_only", ce.pool[0].nonfinite_other_slot_only});
  required.push_back({"finite output with a dropped NaN/inf", ce.softmax_row_finite_with_dropped_nonfinite});
  required.push_back({"elu_negative", ce.elu_negative}), required.push_back({"elu_plus_zero", ce.elu_plus_zero});
  required.push_back({"elu_nan", ce.elu_nan}), required.push_back({"elu_saturated", ce.elu_saturated_to_minus_tenth});
  required.push_back({"expf_minus_inf", ce.expf_minus_inf}), required.push_back({"expf_inf_or_nan", ce.expf_inf_or_nan});
  required.push_back({"expf_overflow", ce.expf_overflow}), required.push_back({"expf_underflow", ce.expf_underflow});
  required.push_back({"expf_may_underflow", ce.expf_may_underflow});
  required.push_back({"expf_88_or_more_computed", ce.expf_88_or_more_computed});
  required.push_back({"subnormal_c1", ce.subnormal_c1}), required.push_back({"subnormal_p1", ce.subnormal_p1});
  required.push_back({"subnormal_c2i", ce.subnormal_c2i}), required.push_back({"subnormal_c2", ce.subnormal_c2});
  required.push_back({"subnormal_fc", ce.subnormal_fc}), required.push_back({"subnormal_prob", ce.subnormal_prob});
  required.push_back({"softmax_in0_is_max", ce.softmax_in0_is_max});
  required.push_back({"softmax_max_replaced", ce.softmax_max_replaced});
  required.push_back({"softmax_inf_over_inf", ce.softmax_inf_over_inf});
  required.push_back({"softmax_zero_over_zero", ce.softmax_zero_over_zero});
  required.push_back({"prob_nan", ce.prob_nan}), required.push_back({"prob_zero", ce.prob_zero});
  required.push_back({"prob_one", ce.prob_one});
  for (const Req& r : required) {
    std::printf("required edges %-40s %ld%s\n", r.what.c_str(), r.n, r.n ? "" : "  MISSING");
    failures += r.n == 0;
  }
  // -0 cannot arise inside the network (sums start from +0, x + -x = +0, elu of a value below 0 is
  // at most -2^-28): the reason the `<=` and `v <= 0` mutants cannot be told from the original
  const long neg_zero = cm.elu_minus_zero + ce.elu_minus_zero + cm.pool[0].negative_zero_value + ce.pool[0].negative_zero_value +
                        cm.pool[1].negative_zero_value + ce.pool[1].negative_zero_value;
  std::printf("minus zero among pre-activations and pooled values: %ld%s\n", neg_zero, neg_zero ? "  UNEXPECTED" : "");
  failures += neg_zero != 0;
  std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
#else
  Census c;
  int killed_cases = 0, changed = 0;
  std::string first;
  for (const Case& k : edges) {
    bool fd = false;
    const int bad = run_case(k, c, fd);
    if (bad && !killed_cases++) first = k.name;
    changed += bad;
  }
  if (MUTANT_POOL) std::printf("pooling mutants act on P%d only\n", MUTANT_POOL);
  std::printf("mutant %d (%s): picked slot differs in %ld windows, picked bits differ in %ld windows, elu differs in %ld of %ld "
              "values (%ld at +0, %ld at -0)\n", MUTANT, kMutantNames[MUTANT], c.mutant_index_differs, c.mutant_bits_differ,
              c.mutant_elu_differs, c.elu_calls, c.elu_plus_zero, c.elu_minus_zero);
  if (changed)
    std::printf("mutant %d KILLED: %d recorded values change in %d cases, first %s\n", MUTANT, changed, killed_cases, first.c_str());
  else
    std::printf("mutant %d SURVIVED\n", MUTANT);
  failures = changed == 0;
#endif
  return failures ? 1 : 0;
}

// tests/native/check_solver.cpp -- the CPU side of the solvers' arithmetic
// (fleet_amd/csrc/solver_math.h, host build):
//   check_solver sample       solver_math.h against libm (sqrtf, sqrt called through
//                             pointers the compiler cannot see through) and against a plain
//                             spelling of the three update bodies with every intermediate
//                             forced to memory, on ~2^23 sampled bit patterns and pairs
//   check_solver exhaustive   the same on all 2^32 patterns (a few minutes)
//   check_solver digest [OUT] the digests fleet_selftest_digest fn 25..30 must equal
//                             (tests/golden/solver_digests.json when OUT is given)
//   check_solver fixture FILE the update bodies against the reference's recorded bits:
//                             the flat export of tests/golden/solver_ref.npz that
//                             tests/test_solver_math.py writes (i32 records; per record
//                             i32 solver, N, steps, adam resets, f32 L, w0[N], g1_0[N], g2_0[N],
//                             d[steps][N], then per step the expected w[N], g1[N], g2[N])
// Prints ALL OK and exits 0 when nothing differs. Build: clang++ -std=c++17 -O2
// -ffp-contract=off -pthread.
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "../../fleet_amd/csrc/solver_math.h"

using namespace fleet;

namespace {

// libm through pointers no optimiser follows
float (*volatile libm_sqrtf)(float) = ::sqrtf;
double (*volatile libm_sqrt)(double) = ::sqrt;

uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

const uint32_t kDivEdges[11] = {0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x3f800000u,
                                0x7f7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u};

// every comparison is bitwise, NaN payloads included
struct Tally {
  std::atomic<uint64_t> checked{0}, bad{0};
  void eq(uint32_t got, uint32_t want, const char* what, uint32_t a, uint32_t b) {
    checked.fetch_add(1, std::memory_order_relaxed);
    if (got == want) return;
    if (bad.fetch_add(1) < 20) std::printf("MISMATCH %s(%08x, %08x): %08x, plain spelling %08x\n", what, a, b, got, want);
  }
};

// the reference's statements, every intermediate a volatile float (one rounding each)
SolverStep plain_step(int solver, float w, float d, float g1, float g2, float L, float b1_t_, float b2_t_) {
  volatile float eps = 1.e-8f, one = 1.0f, t, u, lr, den;
  if (solver == kSolverAdagrad) {
    lr = one * L;
    t = d * d;
    g1 = g1 + t;
    den = libm_sqrtf(g1);
    den = den + eps;
    t = lr * d;
    t = t / den;
    return SolverStep{w - t, g1, 0.0f};
  }
  if (solver == kSolverRmsprop) {
    volatile float mu = 0.999f;
    lr = 0.01f * one;
    lr = lr * L;
    t = mu * g1;
    u = one - mu;
    u = u * d;
    u = u * d;
    g1 = t + u;
    den = libm_sqrtf(g1);
    den = den + eps;
    t = lr * d;
    t = t / den;
    return SolverStep{w - t, g1, 0.0f};
  }
  volatile float b1 = 0.9f, b2 = 0.999f, b1_t = b1_t_, b2_t = b2_t_;
  volatile double q;
  lr = 0.1f * one;
  lr = lr * L;
  t = b1 * g1;
  u = one - b1;
  u = u * d;
  g1 = t + u;
  t = b2 * g2;
  u = one - b2;
  u = u * d;
  u = u * d;
  g2 = t + u;
  q = 1. - (double)b2_t;
  q = (double)g2 / q;
  q = libm_sqrt(q);
  den = (float)q;
  den = den + eps;
  t = one - b1_t;
  t = g1 / t;
  t = lr * t;
  t = t / den;
  return SolverStep{w - t, g1, g2};
}

SolverStep math_step(int solver, float w, float d, float g1, float g2, float L, float b1_t, float b2_t) {
  if (solver == kSolverAdagrad) return adagrad_step(w, d, g1, L);
  if (solver == kSolverRmsprop) return rmsprop_step(w, d, g1, L);
  return adam_step(w, d, g1, g2, L, b1_t, b2_t);
}

void parallel(uint64_t n, const std::function<void(uint64_t, uint64_t, unsigned)>& body) {
  const unsigned nt = std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back([&, t] { body(n * t / nt, n * (t + 1) / nt, t); });
  for (auto& x : th) x.join();
}

int check(bool exhaustive) {
  Tally T;
  float bt[2][2];  // b1_t, b2_t of a fresh solver and of a server session
  adam_bias_terms(0, &bt[0][0], &bt[0][1]);
  adam_bias_terms(kServerResets, &bt[1][0], &bt[1][1]);
  const uint64_t n = exhaustive ? (1ull << 32) : (1ull << 23);
  parallel(n, [&](uint64_t lo, uint64_t hi, unsigned) {
    for (uint64_t i = lo; i < hi; ++i) {
      // sampled: every exponent and both signs (top 9 bits), mantissas from a hash
      const uint32_t u = exhaustive ? (uint32_t)i : ((uint32_t)(i & 511u) << 23) | ((uint32_t)splitmix64(i) & 0x007fffffu);
      const float x = sv_u2f(u);
      T.eq(sv_f2u(sv_sqrt(x)), sv_f2u(libm_sqrtf(x)), "sqrtf", u, 0);
      for (int k = 0; k < 2; ++k) {
        volatile double q = 1. - (double)bt[k][1];
        q = (double)x / q;
        q = libm_sqrt(q);
        volatile float r = (float)q;
        r = r + 1.e-8f;
        T.eq(sv_f2u(adam_den(x, bt[k][1])), sv_f2u(r), "adam_den", u, (uint32_t)k);
        volatile float t = 1.0f - bt[k][0];
        t = x / t;
        T.eq(sv_f2u(adam_num(x, bt[k][0])), sv_f2u(t), "adam_num", u, (uint32_t)k);
      }
      const uint64_t p = splitmix64(i ^ 0x5bd1e995u), p2 = splitmix64(p);
      const uint32_t ua = (uint32_t)p, ub = (uint32_t)(p >> 32);
      {
        volatile float a = sv_u2f(ua), b = sv_u2f(ub), r;
        r = a / b;
        T.eq(sv_f2u(sv_div(sv_u2f(ua), sv_u2f(ub))), sv_f2u(r), "div", ua, ub);
      }
      // the update bodies: x as the gradient, hashed weight, state and rate (state that
      // is no NaN unless x is: the payload of two NaN operands is the compiler's choice)
      if ((i & 7) == 0 || !exhaustive) {
        const float w = sv_u2f(ua), L = sv_u2f(0x3c000000u + ((uint32_t)p2 & 0x03ffffffu));
        float g1 = sv_u2f(ub), g2 = sv_u2f((uint32_t)(p2 >> 32) & 0x7fffffffu);
        if (g1 != g1 || g2 != g2 || w != w || x != x) continue;
        for (int s = kSolverAdagrad; s <= kSolverAdam; ++s) {
          const float s1 = s == kSolverAdam ? g1 : __builtin_fabsf(g1);
          const float* t = bt[i >> 3 & 1];
          const SolverStep a = math_step(s, w, x, s1, g2, L, t[0], t[1]), b = plain_step(s, w, x, s1, g2, L, t[0], t[1]);
          T.eq(sv_f2u(a.w), sv_f2u(b.w), s == 1 ? "adagrad.w" : s == 2 ? "rmsprop.w" : "adam.w", u, ua);
          T.eq(sv_f2u(a.g1), sv_f2u(b.g1), "step.g1", u, ub);
          T.eq(sv_f2u(a.g2), sv_f2u(b.g2), "step.g2", u, ub);
        }
      }
    }
  });
  for (uint32_t ua : kDivEdges)
    for (uint32_t ub : kDivEdges) {
      volatile float a = sv_u2f(ua), b = sv_u2f(ub), r;
      r = a / b;
      T.eq(sv_f2u(sv_div(sv_u2f(ua), sv_u2f(ub))), sv_f2u(r), "div", ua, ub);
    }
  std::printf("%s: %llu comparisons, %llu mismatches\n", exhaustive ? "exhaustive" : "sample",
              (unsigned long long)T.checked.load(), (unsigned long long)T.bad.load());
  if (T.bad.load()) return 1;
  std::printf("ALL OK\n");
  return 0;
}

uint64_t div_term(uint32_t a, uint32_t b) {
  return splitmix64(splitmix64(((uint64_t)a << 32) | b) + sv_f2u(sv_div(sv_u2f(a), sv_u2f(b))));
}

uint64_t digest(int fn) {
  std::vector<uint64_t> part(64, 0);
  float b1_t, b2_t;
  adam_bias_terms(fn >= 29 ? kServerResets : 0, &b1_t, &b2_t);
  parallel(1ull << 32, [&](uint64_t lo, uint64_t hi, unsigned t) {
    uint64_t sum = 0;
    for (uint64_t i = lo; i < hi; ++i) {
      const uint32_t u = (uint32_t)i;
      if (fn == 28) {
        const uint64_t p = splitmix64(i);
        sum += div_term((uint32_t)p, (uint32_t)(p >> 32));
        continue;
      }
      const float x = sv_u2f(u);
      const uint32_t o = sv_f2u(fn == 25 ? sv_sqrt(x) : fn == 26 || fn == 29 ? adam_den(x, b2_t) : adam_num(x, b1_t));
      sum += splitmix64(((uint64_t)u << 32) | o);
    }
    part[t] = sum;
  });
  uint64_t s = 0;
  for (uint64_t p : part) s += p;
  if (fn == 28)
    for (uint32_t a : kDivEdges)
      for (uint32_t b : kDivEdges) s += div_term(a, b);
  return s;
}

int digests(const char* path) {
  FILE* f = path ? std::fopen(path, "w") : nullptr;
  if (path && !f) return 2;
  if (f) std::fprintf(f, "{\n  \"generator\": \"tests/native/check_solver.cpp digest (solver_math.h, host build, libm)\",\n");
  for (int fn = 25; fn <= 30; ++fn) {
    const uint64_t d = digest(fn);
    std::printf("fn%d %016llx\n", fn, (unsigned long long)d);
    std::fflush(stdout);
    if (f) std::fprintf(f, "  \"fn%d\": \"%016llx\"%s\n", fn, (unsigned long long)d, fn < 30 ? "," : "");
  }
  if (f) {
    std::fprintf(f, "}\n");
    std::fclose(f);
  }
  return 0;
}

int fixture(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  int32_t records = 0;
  bool ok = std::fread(&records, 4, 1, f) == 1 && records > 0 && records < 1000;
  uint64_t checked = 0, bad = 0;
  for (int r = 0; ok && r < records; ++r) {
    int32_t hdr[4];
    float L = 0, b1_t, b2_t;
    ok = std::fread(hdr, 4, 4, f) == 4 && std::fread(&L, 4, 1, f) == 1 && hdr[3] >= 0 && hdr[3] < 100 && hdr[0] >= 1 && hdr[0] <= 3 && hdr[1] > 0 &&
         hdr[1] < (1 << 24) && hdr[2] > 0 && hdr[2] < 1000;
    if (!ok) break;
    const size_t N = (size_t)hdr[1], steps = (size_t)hdr[2];
    adam_bias_terms(hdr[3], &b1_t, &b2_t);
    std::vector<float> w(N), g1(N), g2(N), d(N * steps), want(3 * N * steps);
    for (std::vector<float>* v : {&w, &g1, &g2, &d, &want}) ok = ok && std::fread(v->data(), 4, v->size(), f) == v->size();
    if (!ok) break;
    for (size_t s = 0; s < steps; ++s)
      for (size_t i = 0; i < N; ++i) {
        const SolverStep y = math_step(hdr[0], w[i], d[s * N + i], g1[i], g2[i], L, b1_t, b2_t);
        w[i] = y.w, g1[i] = y.g1, g2[i] = y.g2;
        const float* e = want.data() + 3 * N * s;
        const uint32_t got[3] = {sv_f2u(y.w), sv_f2u(y.g1), sv_f2u(y.g2)};
        const uint32_t exp[3] = {sv_f2u(e[i]), sv_f2u(e[N + i]), sv_f2u(e[2 * N + i])};
        for (int k = 0; k < 3; ++k) {
          ++checked;
          if (got[k] != exp[k] && bad++ < 20)
            std::printf("MISMATCH record %d solver %d step %zu element %zu %s: %08x, recorded %08x\n", r, hdr[0], s, i,
                        k == 0 ? "w" : k == 1 ? "g1" : "g2", got[k], exp[k]);
        }
      }
  }
  std::fclose(f);
  if (!ok) {
    std::fprintf(stderr, "malformed fixture file\n");
    return 2;
  }
  std::printf("fixture: %d records, %llu values, %llu mismatches\n", records, (unsigned long long)checked,
              (unsigned long long)bad);
  if (bad) return 1;
  std::printf("ALL OK\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "sample")) return check(false);
  if (!std::strcmp(mode, "exhaustive")) return check(true);
  if (!std::strcmp(mode, "digest")) return digests(argc > 2 ? argv[2] : nullptr);
  if (!std::strcmp(mode, "fixture") && argc > 2) return fixture(argv[2]);
  std::fprintf(stderr, "usage: check_solver sample | exhaustive | digest [OUT.json] | fixture FILE\n");
  return 2;
}

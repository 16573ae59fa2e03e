// tests/native/check_g6text.cpp -- CPU check of g6_text (fleet_amd/csrc/decimal6.h),
// the `ostream << float` text the device emits for model parameters, against
// libc's snprintf("%g") byte for byte. Stand-alone: no oracle, no library.
//
//   check_g6text sample      every 4099th bit pattern and the edge list (CPU test suite)
//   check_g6text exhaustive  every binary32: the finite ones against snprintf, the
//                            non-finite ones against the six fixed strings; prints the
//                            order-independent digest of tests/golden/g6text_digest.json
//                            (digest fn 24 of the device self-test)
//   check_g6text edges       the edge list as "bits text" lines (tests/g6_edges.py holds
//                            the same list for the GPU test)
//
// Exit status 0 = all byte-identical.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../fleet_amd/csrc/decimal6.h"

using namespace fleet;

static std::atomic<long> g_bad{0};
static std::atomic<int> g_maxlen{0};

// the reference text of bit pattern u (no terminator counted)
static int ref_text(uint32_t u, char* buf /* 32 */) {
  const uint32_t a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) {
    const char* s = a == 0x7f800000u ? ((u >> 31) ? "-inf" : "inf") : ((u >> 31) ? "-nan" : "nan");
    std::strcpy(buf, s);
    return (int)std::strlen(s);
  }
  return snprintf(buf, 32, "%g", (double)u2f(u));
}

static uint64_t check_one(uint32_t u) {
  char ref[32], got[32];
  std::memset(got, 0x55, sizeof got);
  const int rl = ref_text(u, ref), gl = g6_text(u2f(u), got);
  bool ok = rl == gl && gl <= kG6TextMax && std::memcmp(ref, got, (size_t)rl) == 0;
  for (int i = gl < 0 ? 0 : gl; i < 32 && ok; ++i) ok = got[i] == 0x55;  // nothing written past the length
  if (!ok) {
    if (g_bad++ < 10) fprintf(stderr, "mismatch %08x: libc '%s' (%d), g6_text '%.*s' (%d)\n", u, ref, rl, gl, got, gl);
  }
  int m = g_maxlen.load();
  while (rl > m && !g_maxlen.compare_exchange_weak(m, rl)) {
  }
  return g6_text_term(u, ref, rl);
}

static const uint32_t kNanPayload = 0x7f800001u;

static std::vector<uint32_t> edges() {
  std::vector<uint32_t> e = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
                             kNanPayload, 0xffffffffu};
  const float vals[] = {
      // one output of every length from 1 to 12
      1.0f, -1.0f, 0.5f, 1.25f, -1.25f, 1e6f, 123456.0f, 1.5e10f, -1.5e10f, 1.25e-10f, 1.234e10f, 1.2345e10f,
      1.23456e10f, -1.23456e10f, 0.000123456f, -0.000123456f, -FLT_MIN,
      // the fixed / scientific switch below: 1e-5 | 1e-4, with the round-up carry 9.999995e-5
      1e-5f, 9.99999e-5f, 9.999995e-5f, 9.9999995e-5f, 1e-4f, 1.00001e-4f,
      // and above: 999999 | 1e+06, with the half-even ties at 999999.5, 999998.5, 999997.5
      999999.0f, 999999.5f, 999999.4375f, 999998.5f, 999997.5f, 1e6f, 1000001.0f, 100000.0f, 99999.95f,
      // the ends of the range, two-digit exponents of both signs
      FLT_TRUE_MIN, 2 * FLT_TRUE_MIN, FLT_MIN, FLT_MAX, -FLT_MAX, 1e10f, 1e-10f, 1e38f, 1e-38f, 1e-45f,
      // plain values, trailing zeros, a bare point
      0.1f, 0.001f, 100.0f, 1e5f, 12345.6f, 123456.7f, 1.5f, 0.3f, 16777216.0f, 3.14159274f, -2.5e-7f};
  for (float v : vals) e.push_back(f2u(v));
  return e;
}

template <typename F>
static uint64_t par_sum(uint64_t begin, uint64_t end, uint64_t stride, F f) {
  // at most 16 threads: a shared box reports many times the CPUs one command may use
  unsigned nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  std::vector<uint64_t> part(nt, 0);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([=, &part] {
      uint64_t s = 0;
      for (uint64_t i = begin + t * stride; i < end; i += (uint64_t)nt * stride) s += f((uint32_t)i);
      part[t] = s;
    });
  for (auto& x : th) x.join();
  uint64_t s = 0;
  for (uint64_t p : part) s += p;
  return s;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "sample";
  const auto t0 = std::chrono::steady_clock::now();
  if (mode == "edges") {
    for (uint32_t u : edges()) {
      char ref[32];
      ref_text(u, ref);
      printf("%08x %s\n", u, ref);
    }
    return 0;
  }
  if (mode == "exhaustive") {
    const uint64_t dg = par_sum(0, 1ull << 32, 1, check_one);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("g6_text (exhaustive)         %s (%ld mismatches of 4294967296, longest %d bytes, %.0f s)\n",
           g_bad ? "FAIL" : "ok", g_bad.load(), g_maxlen.load(), sec);
    printf("digest %016llx\n", (unsigned long long)dg);
    return g_bad || g_maxlen != kG6TextMax ? 1 : 0;
  }
  if (mode != "sample") {
    fprintf(stderr, "usage: check_g6text sample|exhaustive|edges\n");
    return 2;
  }
  par_sum(0, 1ull << 32, 4099, check_one);
  unsigned seen = 0;  // bit l: an edge prints l bytes
  for (uint32_t u : edges()) {
    check_one(u);
    char ref[32];
    seen |= 1u << ref_text(u, ref);
  }
  const bool all_lengths = seen == 0x1ffeu;  // 1..12, nothing else
  printf("g6_text (sampled + edges)    %s (%ld mismatches, longest %d bytes, edge lengths %s)\n",
         g_bad ? "FAIL" : "ok", g_bad.load(), g_maxlen.load(), all_lengths ? "1..12" : "INCOMPLETE");
  if (g_bad || !all_lengths || g_maxlen != kG6TextMax) return 1;
  printf("ALL OK\n");
  return 0;
}

// tests/native/check_div10.cpp -- CPU check of the one-fma-per-step /10 chains of
// fleet_amd/csrc/codec_math.h (div10_mt in its scaled form with the MulEntry /
// StepTables rows, and the fixed nine-step d9) against the chain the reference
// runs: k IEEE binary32 divisions by 10.0f (Base64.cpp:91-98).
//
//   check_div10 sample      every 13th mantissa (offset by the binade) and the 4096
//                           mantissas at either end of each binade; every 17th int32 code
//                           and the 2^16 codes at either end and around 0 (CPU test suite)
//   check_div10 exhaustive  every mantissa and every int32 code (dev check; ~2 min on 8 cores)
//
// Both modes cover every digit row d = 0..15 (k = 9 - d steps, none for d > 9), the
// binades 2^-3 .. 2^31 (every value a chain can start from: |code| <= 2^31, and
// nothing below 1 but 0), both signs and +-0, and int2float's own form -- (float)c
// with the row of c's last digit -- through dec_mt_r and dec_d16. -0.0 only ever
// enters a chain as the signed float of code 0 (q_fast, code_float_mt), where the
// reference divides (float)0 = +0.0: its expected result is that of +0.0.
//
// Exit status 0 = all bit-identical.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../fleet_amd/csrc/codec_math.h"

using namespace fleet;
static std::atomic<long> g_bad{0};
static std::atomic<long> g_cases{0};
static const StepTables g_st = make_step_tables();
static MulEntry g_mt[16];

template <typename F>
void par_for(uint64_t begin, uint64_t end, F f) {
  unsigned nt = std::max(1u, std::thread::hardware_concurrency());
  std::vector<std::thread> th;
  const uint64_t chunk = 1u << 16;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([=] {
      long bad = 0, cases = 0;
      for (uint64_t b = begin + t * chunk; b < end; b += (uint64_t)nt * chunk)
        for (uint64_t i = b; i < std::min(b + chunk, end); ++i) f(i, bad, cases);
      g_bad += bad;
      g_cases += cases;
    });
  for (auto& x : th) x.join();
}

static long report(const char* name, long bad_before, long cases_before) {
  long b = g_bad.load() - bad_before;
  printf("%-44s %s (%ld mismatches in %ld cases)\n", name, b ? "FAIL" : "ok", b, g_cases.load() - cases_before);
  return b;
}

static inline bool same(float a, float b) { return f2u(a) == f2u(b); }

// U[k] = t after k divisions, k = 0..9; -0.0 starts as +0.0 (see above)
static inline void ref_chain(float t, float U[10]) {
  U[0] = f2u(t) == 0x80000000u ? 0.0f : t;
  for (int k = 1; k <= 9; ++k) U[k] = U[k - 1] / 10.0f;
}

// every form of the chain on one start value
static inline void check_value(float t, long& bad, long& cases) {
  float U[10];
  ref_chain(t, U);
  for (uint32_t d = 0; d < 16; ++d) {
    const uint32_t k = d <= 9u ? 9u - d : 0u;
    bad += !same(div10_mt(t, g_mt[d]), U[k]);
  }
  bad += !same(d9(t), U[9]);
  cases += 17;
}

// int2float's form: (float)c with the row of c's own last digit
static inline void check_code(int32_t c, long& bad, long& cases) {
  const uint32_t a = c < 0 ? 0u - (uint32_t)c : (uint32_t)c;
  const uint32_t r = a % 10u;
  float U[10];
  ref_chain((float)c, U);
  bad += !same(dec_mt_r(c, r, g_mt), U[9 - r]);
  bad += !same(dec_d16(c, r << 4, &g_st), U[9 - r]);
  cases += 2;
  if (r == 0) {
    bad += !same(dec_fast(c), U[9]);
    cases += 1;
  }
}

constexpr uint32_t kBeLo = 124, kBeHi = 158;  // binades 2^-3 .. 2^31
constexpr uint32_t kBinades = kBeHi - kBeLo + 1;

static inline float value_at(uint32_t sign, uint32_t binade, uint32_t mant) {
  return u2f((sign << 31) | ((kBeLo + binade) << 23) | mant);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "sample";
  if (mode != "sample" && mode != "exhaustive") {
    fprintf(stderr, "usage: check_div10 sample|exhaustive\n");
    return 2;
  }
  const bool exhaustive = mode == "exhaustive";
  for (uint32_t d = 0; d < 16; ++d) g_mt[d] = mul_entry(d);

  // the table rows: multipliers and the descale
  long b = g_bad, n = g_cases;
  for (uint32_t d = 0; d < 16; ++d) {
    const uint32_t k = d <= 9u ? 9u - d : 0u;
    const float s = u2f((127u - 3u * k) << 23);
    const Steps st = steps_of(k);
    const bool g[4] = {d <= 9u && st.e, d <= 9u && st.b0, d <= 9u && st.b1, d <= 9u && st.b2};
    for (int i = 0; i < 4; ++i) {
      g_bad += !same(g_mt[d].h[i], g[i] ? 8.0f * kTenthHi : 1.0f);
      g_bad += !same(g_st.h[d][i], g_mt[d].h[i]);
    }
    g_bad += !same(g_mt[d].s, s);
    g_bad += g_st.d[d][0] != d || g_st.d[d][1] != f2u(s);
    g_cases += 11;
  }
  report("table rows (h, s)", b, n);

  b = g_bad, n = g_cases;
  {
    long bad = 0, cases = 0;
    check_value(0.0f, bad, cases);
    check_value(-0.0f, bad, cases);
    g_bad += bad;
    g_cases += cases;
  }
  report("+-0, rows 0..15 and d9", b, n);

  b = g_bad, n = g_cases;
  if (exhaustive) {
    par_for(0, (uint64_t)2 * kBinades << 23, [](uint64_t i, long& bad, long& cases) {
      const uint32_t mant = (uint32_t)i & 0x7fffffu, hi = (uint32_t)(i >> 23);
      check_value(value_at(hi / kBinades, hi % kBinades, mant), bad, cases);
    });
  } else {
    constexpr uint32_t stride = 13, per = ((1u << 23) + stride - 1) / stride, edge = 4096;
    par_for(0, (uint64_t)2 * kBinades * (per + 2 * edge), [](uint64_t i, long& bad, long& cases) {
      const uint32_t j = (uint32_t)(i % (per + 2 * edge)), hi = (uint32_t)(i / (per + 2 * edge));
      uint32_t mant;
      if (j < edge) mant = j;
      else if (j < 2 * edge) mant = 0x7fffffu - (j - edge);
      else mant = std::min((j - 2 * edge) * stride + hi % stride, 0x7fffffu);
      check_value(value_at(hi / kBinades, hi % kBinades, mant), bad, cases);
    });
  }
  report(exhaustive ? "div10_mt rows 0..15, d9 (every mantissa)" : "div10_mt rows 0..15, d9 (sampled)", b, n);

  b = g_bad, n = g_cases;
  if (exhaustive) {
    par_for(0, 1ull << 32, [](uint64_t i, long& bad, long& cases) { check_code((int32_t)(uint32_t)i, bad, cases); });
  } else {
    constexpr uint64_t stride = 17, per = ((1ull << 32) + stride - 1) / stride, edge = 1u << 16;
    par_for(0, per + 4 * edge, [](uint64_t i, long& bad, long& cases) {
      uint32_t u;
      if (i < 2 * edge) u = (uint32_t)i - (uint32_t)edge;                      // around 0
      else if (i < 4 * edge) u = 0x80000000u + (uint32_t)(i - 3 * edge);       // INT_MAX / INT_MIN ends
      else u = (uint32_t)std::min((i - 4 * edge) * stride, (uint64_t)0xffffffffu);
      check_code((int32_t)u, bad, cases);
    });
  }
  report(exhaustive ? "dec_mt_r, dec_d16, dec_fast (every int32)" : "dec_mt_r, dec_d16, dec_fast (sampled)", b, n);

  printf("%s\n", g_bad ? "MISMATCHES" : "ALL OK");
  return g_bad ? 1 : 0;
}

// tests/native/check_client_dp.cpp -- the host mirror of the client's DPgradients and of the
// distillation cost (fleet_amd/csrc/client_backward.h: client_grad_host_ex over sample_stages,
// sample_sqsum, clip_scale, dp_grad_element and dp_noise_draws, the functions k_client_sample,
// k_client_clip and k_client_sum_dp run) against tests/golden/client_dp_ref.npz, recorded from
// the reference's own network class.
//
//   check_client_dp <client_dp_ref.bin> <vectors.out>
//
// reads the fixture as the flat file tests/client_dp_ref.py write_flat() makes of it and, per
// case, compares bit for bit every recorded array: E, FC2's node and delta of every sample;
// sqsum, norm and scale of every batch slot scale_gradients walks (1 .. B-1) where sigma > 0;
// the I1 and FC2 bias blocks of the vector, and the whole vector where the fixture holds it. The
// vector computed for every case is written to <vectors.out> after the 22961 draws (doubles),
// so the caller can compare the digests the fixture holds. Stand-alone, so it also runs under
// the host sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fleet_amd/csrc/client_backward.h"

namespace {

using namespace fleet::clientnet;

uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }

int diff(const char* what, const float* got, const float* want, size_t n) {
  int bad = 0;
  for (size_t i = 0; i < n; ++i)
    if (bits(got[i]) != bits(want[i])) {
      if (!bad) std::printf("    %s[%zu]: got %a, recorded %a\n", what, i, got[i], want[i]);
      ++bad;
    }
  if (bad) std::printf("    %s: %d of %zu differ\n", what, bad, n);
  return bad;
}

template <typename T>
bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: check_client_dp client_dp_ref.bin vectors.out\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  FILE* vec = std::fopen(argv[2], "wb");
  if (!f || !vec) {
    std::fprintf(stderr, "cannot open the fixture or the output\n");
    return 2;
  }
  std::vector<double> z(kGradLen);
  dp_noise_draws(z.data(), z.size());
  std::fwrite(z.data(), 8, z.size(), vec);
  std::vector<float> w, b;
  int32_t n = 0;
  if (!get(f, w, kWTotal) || !get(f, b, kBTotal) || std::fread(&n, 4, 1, f) != 1 || n <= 0 || n > 1000) return 2;
  int failures = 0;
  for (int i = 0; i < n; ++i) {
    int32_t len = 0, hdr[3];
    float dp[2];
    std::string name;
    if (std::fread(&len, 4, 1, f) != 1 || len <= 0 || len > 255) return 2;
    name.resize(len);
    if (std::fread(&name[0], 1, len, f) != (size_t)len || std::fread(hdr, 4, 3, f) != 3 || std::fread(dp, 4, 2, f) != 2 ||
        hdr[0] <= 0 || hdr[0] > 64)
      return 2;
    const int B = hdr[0], cost = hdr[1], full = hdr[2];
    const float clip = dp[0], sigma = dp[1];
    std::vector<float> x, E, node, delta, sqsum, norm, scale, g_i1, g_fc2, grad;
    std::vector<int32_t> labels, shifts;
    bool ok = get(f, x, (size_t)B * kPix) && get(f, labels, B) && get(f, shifts, 2 * (size_t)B) && get(f, E, B) &&
              get(f, node, (size_t)B * kClasses) && get(f, delta, (size_t)B * kClasses) && get(f, sqsum, B) &&
              get(f, norm, B) && get(f, scale, B) && get(f, g_i1, kPix) && get(f, g_fc2, kClasses);
    if (ok && full) ok = get(f, grad, kGradLen);
    if (!ok) {
      std::fprintf(stderr, "truncated fixture at case %d\n", i);
      return 2;
    }
    std::vector<Sample> S(B);
    std::vector<float> rows((size_t)B * kGradLen), out(kGradLen), stats(3 * (size_t)B);
    int bad = client_grad_host_ex(w.data(), b.data(), x.data(), labels.data(), shifts.data(), B, 2.0f, cost, clip, sigma,
                                  z.data(), rows.data(), out.data(), S.data(), stats.data());
    for (int k = 0; k < B; ++k) {
      bad += diff("E", &S[k].E, &E[k], 1);
      bad += diff("node FC2", S[k].fc, node.data() + (size_t)k * kClasses, kClasses);
      bad += diff("delta FC2", S[k].d_fc, delta.data() + (size_t)k * kClasses, kClasses);
    }
    if (sigma > 0.0f && B > 1) {
      bad += diff("sqsum", stats.data() + 1, sqsum.data() + 1, B - 1);
      bad += diff("norm", stats.data() + B + 1, norm.data() + 1, B - 1);
      bad += diff("scale", stats.data() + 2 * B + 1, scale.data() + 1, B - 1);
    }
    bad += diff("gradients I1 bias", out.data() + kG_BI1, g_i1.data(), kPix);
    bad += diff("gradients FC2 bias", out.data() + kG_Bfc, g_fc2.data(), kClasses);
    if (full) bad += diff("gradients", out.data(), grad.data(), kGradLen);
    std::fwrite(out.data(), 4, kGradLen, vec);
    std::printf("reproduce %-4s B %d cost %d clip %g sigma %g: %s (%d values differ)\n", name.c_str(), B, cost, clip, sigma,
                bad ? "MISMATCH" : "ok", bad);
    failures += bad != 0;
  }
  std::fclose(f);
  std::fclose(vec);
  std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
  return failures ? 1 : 0;
}

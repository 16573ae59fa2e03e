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
//
//   check_client_dp --mirror <jobs.bin> <out.bin>
//
// the host mirror alone, for shapes the fixture does not hold (tests/client_dp_jobs.py writes the
// jobs and reads the output): int32 n, then per job int32 n_models, the model rows (w[21448]
// then b[82] each), int32 C, B, float temperature, int32 cost, model_of_client[C], clip[C],
// sigma[C], images[C*B][784] (gathered), labels[C*B], shifts[C*B][2]. Writes per job the C
// vectors and then the stats [C][3][B] (sqsum, norm, scale; zeros for a client with sigma = 0),
// and prints per client how many of its samples came out with E NaN.
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

int mirror(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  FILE* res = std::fopen(out, "wb");
  int32_t n = 0;
  if (!f || !res || std::fread(&n, 4, 1, f) != 1 || n <= 0 || n > 1000) return 2;
  std::vector<double> z(kGradLen);
  dp_noise_draws(z.data(), z.size());
  constexpr size_t kRow = (size_t)kWTotal + kBTotal;
  for (int i = 0; i < n; ++i) {
    std::vector<float> models, clip, sigma, x;
    std::vector<int32_t> model_of, labels, shifts;
    int32_t n_models = 0, cb[2], cost = 0;
    float temperature = 0;
    if (std::fread(&n_models, 4, 1, f) != 1 || n_models <= 0 || n_models > 16 || !get(f, models, n_models * kRow) ||
        std::fread(cb, 4, 2, f) != 2 || cb[0] <= 0 || cb[1] <= 0 || (int64_t)cb[0] * cb[1] > 100000 ||
        std::fread(&temperature, 4, 1, f) != 1 || std::fread(&cost, 4, 1, f) != 1 ||
        (cost != kCostCrossEntropy && cost != kCostDistillation))
      return 2;
    const size_t C = (size_t)cb[0], B = (size_t)cb[1];
    if (!get(f, model_of, C) || !get(f, clip, C) || !get(f, sigma, C) || !get(f, x, C * B * kPix) ||
        !get(f, labels, C * B) || !get(f, shifts, 2 * C * B))
      return 2;
    for (size_t c = 0; c < C; ++c)
      if (model_of[c] < 0 || model_of[c] >= n_models) return 2;
    std::vector<float> rows(B * kGradLen), outv(kGradLen), stats(C * 3 * B, 0.0f);
    for (size_t c = 0; c < C; ++c) {
      const float* w = models.data() + (size_t)model_of[c] * kRow;
      const int blown = client_grad_host_ex(w, w + kWTotal, x.data() + c * B * kPix, labels.data() + c * B,
                                            shifts.data() + 2 * c * B, (int)B, temperature, cost, clip[c], sigma[c],
                                            z.data(), rows.data(), outv.data(), nullptr, stats.data() + c * 3 * B);
      std::fwrite(outv.data(), 4, kGradLen, res);
      std::printf("job %d client %zu blown %d\n", i, c, blown);
    }
    std::fwrite(stats.data(), 4, stats.size(), res);
  }
  if (std::fgetc(f) != EOF) return 2;  // the writer and this reader disagree on the format
  std::fclose(f);
  return std::fclose(res) ? 2 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--mirror")) return mirror(argv[2], argv[3]);
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

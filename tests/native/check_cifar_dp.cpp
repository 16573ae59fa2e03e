// tests/native/check_cifar_dp.cpp -- the host form of DPgradients on the CIFAR network
// (fleet_amd/csrc/cifar_backward.h: record_sqsum, dp_sum_element, rgb_dp_host, the arithmetic
// k_rgb_clip, k_rgb_sum_dp and k_rgb_fc_sum_dp place on the device).
//
//   check_cifar_dp --mirror <jobs.bin> <out.bin>
//
// check_cifar_backward's jobs and output (tests/cifar_grad_ref.py mirror()), with every job's
// float clip and sigma in <jobs.bin>.dp. Stand-alone, so it also runs under the host sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fleet_amd/csrc/cifar_backward.h"

using namespace fleet::rgbnet;

template <typename T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4 || std::strcmp(argv[1], "--mirror")) return 2;
  FILE* f = std::fopen(argv[2], "rb");
  FILE* dp = std::fopen((std::string(argv[2]) + ".dp").c_str(), "rb");
  FILE* out = std::fopen(argv[3], "wb");
  if (!f || !dp || !out) return 2;
  std::vector<double> z(grad_len(100));
  fleet::clientnet::dp_noise_draws(z.data(), z.size());
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n > 0 && n < 10000;
  for (int i = 0; ok && i < n; ++i) {
    int32_t hdr[3];
    float temperature = 0.0f, cs[2];
    ok = std::fread(hdr, 4, 3, f) == 3 && std::fread(&temperature, 4, 1, f) == 1 && std::fread(cs, 4, 2, dp) == 2 &&
         classes_ok(hdr[0]) && hdr[1] > 0 && hdr[1] <= 100000 && cs[0] > 0.0f && cs[1] > 0.0f;
    if (!ok) break;
    const int N = hdr[0], B = hdr[1];
    std::vector<float> w, b, x;
    std::vector<int32_t> labels, shifts;
    ok = get(f, w, weight_count(N)) && get(f, b, bias_count(N)) && get(f, x, (size_t)B * kPix) && get(f, labels, B) &&
         (!hdr[2] || get(f, shifts, (size_t)B * 2));
    for (int32_t v : shifts) ok = ok && v >= -1 && v <= 1;
    if (!ok) break;
    std::vector<float> recs((size_t)B * record_len(N)), grads(grad_len(N)), scale(B);
    const int32_t blown = rgb_grads_host(N, w.data(), b.data(), x.data(), labels.data(), hdr[2] ? shifts.data() : nullptr,
                                         B, temperature, recs.data(), grads.data());
    rgb_dp_host(N, recs.data(), B, cs[0], cs[1], z.data(), scale.data(), grads.data());
    std::fwrite(grads.data(), 4, grads.size(), out);
    std::fwrite(&blown, 4, 1, out);
  }
  std::fclose(f);
  std::fclose(dp);
  return std::fclose(out) == 0 && ok ? 0 : 2;
}

// tests/native/check_cifar_backward.cpp -- the host mirror of the client's gradients on the
// CIFAR network (fleet_amd/csrc/cifar_backward.h: rgb_grads_host, the functions the kernels of
// cifar_client_kernels.hip run per lane).
//
//   check_cifar_backward --mirror <jobs.bin> <out.bin>
//
// runs the host form over jobs, one client each (tests/cifar_grad_ref.py mirror() writes them
// and reads the results). Stand-alone, so it also runs under the host sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fleet_amd/csrc/cifar_backward.h"

namespace {

using namespace fleet::rgbnet;

template <typename T>
bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

// jobs: int32 n, then per job int32 N, B, has_shifts and float temperature; w, b, x[B*3072],
// labels[B], shifts[B*2] = (dx, dy). out: per job the vector [grad_len(N)], then int32 the
// number of samples whose E is NaN
int run_mirror(const char* in_path, const char* out_path) {
  FILE* f = std::fopen(in_path, "rb");
  FILE* out = std::fopen(out_path, "wb");
  if (!f || !out) return 2;
  int32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1 && n > 0 && n < 10000;
  for (int i = 0; ok && i < n; ++i) {
    int32_t hdr[3];
    float temperature = 0.0f;
    ok = std::fread(hdr, 4, 3, f) == 3 && std::fread(&temperature, 4, 1, f) == 1 && classes_ok(hdr[0]) && hdr[1] > 0 &&
         hdr[1] <= 100000;
    if (!ok) break;
    const int N = hdr[0], B = hdr[1];
    std::vector<float> w, b, x;
    std::vector<int32_t> labels, shifts;
    ok = get(f, w, weight_count(N)) && get(f, b, bias_count(N)) && get(f, x, (size_t)B * kPix) && get(f, labels, B) &&
         (!hdr[2] || get(f, shifts, (size_t)B * 2));
    for (int32_t v : shifts) ok = ok && v >= -1 && v <= 1;
    if (!ok) break;
    std::vector<float> recs((size_t)B * record_len(N)), grads(grad_len(N));
    const int32_t blown = rgb_grads_host(N, w.data(), b.data(), x.data(), labels.data(), hdr[2] ? shifts.data() : nullptr,
                                         B, temperature, recs.data(), grads.data());
    std::fwrite(grads.data(), 4, grads.size(), out);
    std::fwrite(&blown, 4, 1, out);
  }
  std::fclose(f);
  return std::fclose(out) == 0 && ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--mirror")) return run_mirror(argv[2], argv[3]);
  std::fprintf(stderr, "usage: check_cifar_backward --mirror jobs.bin out.bin\n");
  return 2;
}

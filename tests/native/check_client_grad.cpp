// tests/native/check_client_grad.cpp -- the client gradient's host mirror
// (fleet_amd/csrc/client_backward.h: client_grad_host over sample_stages and grad_element, the
// functions k_client_sample and k_client_sum run) against tests/golden/client_grad_ref.npz,
// getGradients recorded from the reference's own network class.
//
//   check_client_grad <client_grad_ref.bin> <vectors.out>
//
// reads the fixture as the flat file tests/client_grad_ref.py write_flat() makes of it and,
// per case, compares bit for bit every recorded array: the shifted input layer and E of every
// sample; for the full cases every layer's node, both p_maps and every layer's delta after
// pass 1; the gradients() vector (for the eight shift cases its C1 weight block and I1 bias
// block, and FC2's node). The vector computed for every case is written to <vectors.out>, so
// the caller can compare the digests the fixture holds. Stand-alone, so it also runs under the
// host sanitizers.
//
//   check_client_grad --mirror <jobs.bin> <vectors.out>
//
// the host mirror alone, for the GPU tests: int32 n, then per job w[21448], b[82], int32 C, B,
// float temperature, images[C*B][784] (gathered), labels[C*B], shifts[C*B][2]; writes the C
// vectors of every job.
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

int diff_i(const char* what, const int32_t* got, const int32_t* want, size_t n) {
  int bad = 0;
  for (size_t i = 0; i < n; ++i) bad += got[i] != want[i];
  if (bad) std::printf("    %s: %d of %zu differ\n", what, bad, n);
  return bad;
}

template <typename T>
bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

constexpr int kNodes = kPix + kC1Out + kP1Out + kC2iOut + kC2Out + kFcIn + kClasses;  // 7898

// a padded delta [maps][n + 8][n + 8] without its padding
std::vector<float> unpad(const float* pad, int maps, int n) {
  std::vector<float> out((size_t)maps * n * n);
  for (int m = 0; m < maps; ++m)
    for (int y = 0; y < n; ++y)
      for (int x = 0; x < n; ++x) out[(m * n + y) * n + x] = pad[(m * (n + 8) + y + 4) * (n + 8) + x + 4];
  return out;
}

int mirror(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  FILE* vec = std::fopen(out, "wb");
  int32_t n = 0;
  if (!f || !vec || std::fread(&n, 4, 1, f) != 1 || n <= 0 || n > 1000) return 2;
  for (int i = 0; i < n; ++i) {
    std::vector<float> w, b, x;
    std::vector<int32_t> labels, shifts;
    int32_t cb[2];
    float temperature = 0;
    if (!get(f, w, kWTotal) || !get(f, b, kBTotal) || std::fread(cb, 4, 2, f) != 2 || cb[0] <= 0 || cb[1] <= 0 ||
        (int64_t)cb[0] * cb[1] > 100000 || std::fread(&temperature, 4, 1, f) != 1)
      return 2;
    const size_t C = (size_t)cb[0], B = (size_t)cb[1];
    if (!get(f, x, C * B * kPix) || !get(f, labels, C * B) || !get(f, shifts, 2 * C * B)) return 2;
    std::vector<float> rows(B * kGradLen), outv(kGradLen);
    for (size_t c = 0; c < C; ++c) {
      client_grad_host(w.data(), b.data(), x.data() + c * B * kPix, labels.data() + c * B, shifts.data() + 2 * c * B,
                       (int)B, temperature, rows.data(), outv.data(), nullptr);
      std::fwrite(outv.data(), 4, kGradLen, vec);
    }
  }
  std::fclose(f);
  std::fclose(vec);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--mirror")) return mirror(argv[2], argv[3]);
  if (argc != 3) {
    std::fprintf(stderr, "usage: check_client_grad client_grad_ref.bin vectors.out\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  FILE* vec = std::fopen(argv[2], "wb");
  if (!f || !vec) {
    std::fprintf(stderr, "cannot open the fixture or the output\n");
    return 2;
  }
  std::vector<float> w, b;
  int32_t n = 0;
  if (!get(f, w, kWTotal) || !get(f, b, kBTotal) || std::fread(&n, 4, 1, f) != 1 || n <= 0 || n > 1000) return 2;
  int failures = 0;
  for (int i = 0; i < n; ++i) {
    int32_t len = 0, hdr[2];
    float temperature = 0;
    std::string name;
    if (std::fread(&len, 4, 1, f) != 1 || len <= 0 || len > 255) return 2;
    name.resize(len);
    if (std::fread(&name[0], 1, len, f) != (size_t)len || std::fread(hdr, 4, 2, f) != 2 ||
        std::fread(&temperature, 4, 1, f) != 1 || hdr[0] <= 0 || hdr[0] > 64)
      return 2;
    const int B = hdr[0], kind = hdr[1];
    std::vector<float> x, input, E, node, delta, grad, fc_node, g_c1, g_i1;
    std::vector<int32_t> labels, shifts, pmap;
    bool ok = get(f, x, (size_t)B * kPix) && get(f, labels, B) && get(f, shifts, 2 * (size_t)B) &&
              get(f, input, (size_t)B * kPix) && get(f, E, B);
    if (ok && kind == 1) ok = B == 1 && get(f, node, kNodes) && get(f, pmap, kP1Out + kFcIn) && get(f, delta, kNodes);
    if (ok && kind == 2) ok = get(f, fc_node, kClasses) && get(f, g_c1, 200) && get(f, g_i1, kPix);
    if (ok && kind != 2) ok = get(f, grad, kGradLen);
    if (!ok) {
      std::fprintf(stderr, "truncated fixture at case %d\n", i);
      return 2;
    }
    std::vector<Sample> S(B);
    std::vector<float> rows((size_t)B * kGradLen), out(kGradLen);
    int bad = client_grad_host(w.data(), b.data(), x.data(), labels.data(), shifts.data(), B, temperature, rows.data(),
                               out.data(), S.data());
    for (int k = 0; k < B; ++k) {
      bad += diff("input", S[k].in, input.data() + (size_t)k * kPix, kPix);
      bad += diff("E", &S[k].E, &E[k], 1);
    }
    if (kind == 1) {
      const Sample& s = S[0];
      const float* nd = node.data();
      const float* dl = delta.data();
      const std::vector<float> d_c1 = unpad(s.d_c1, kMaps1, kC1), d_c2 = unpad(s.d_c2, kMaps2, kC2);
      const struct {
        const char* name;
        const float *node, *delta;
        int n;
      } layers[7] = {{"I1", s.in, s.d_in, kPix},         {"C1", s.c1, d_c1.data(), kC1Out}, {"P1", s.p1, s.d_p1, kP1Out},
                     {"C2i", s.c2i, s.d_c2i, kC2iOut},   {"C2", s.c2, d_c2.data(), kC2Out}, {"P2", s.p2, s.d_p2, kFcIn},
                     {"FC2", s.fc, s.d_fc, kClasses}};
      for (const auto& L : layers) {
        bad += diff((std::string("node ") + L.name).c_str(), L.node, nd, L.n);
        bad += diff((std::string("delta ") + L.name).c_str(), L.delta, dl, L.n);
        nd += L.n, dl += L.n;
      }
      bad += diff_i("p_map P1", s.pm1, pmap.data(), kP1Out);
      bad += diff_i("p_map P2", s.pm2, pmap.data() + kP1Out, kFcIn);
    }
    if (kind == 2) {
      bad += diff("node FC2", S[0].fc, fc_node.data(), kClasses);
      bad += diff("gradients C1", out.data() + kG_W1, g_c1.data(), 200);
      bad += diff("gradients I1", out.data() + kG_BI1, g_i1.data(), kPix);
    } else {
      bad += diff("gradients", out.data(), grad.data(), kGradLen);
    }
    std::fwrite(out.data(), 4, kGradLen, vec);
    std::printf("reproduce %-10s B %d temperature %g: %s (%d values differ)\n", name.c_str(), B, temperature,
                bad ? "MISMATCH" : "ok", bad);
    failures += bad != 0;
  }
  std::fclose(f);
  std::fclose(vec);
  std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
  return failures ? 1 : 0;
}

// tests/native/ref_client_dp_driver.cpp -- records tests/golden/client_dp_ref.npz from the
// reference's own network class (tests/golden/make_client_dp_golden.py compiles this into a
// temporary directory with the flags of the client-gradient recorder, -std=c++11 -O0
// -DDISTILLATION_MODE=1 -fno-access-control, against commonLib/cppNN). Nothing of it, and
// nothing compiled from it, is kept in the repository.
//
// The network is the client's (Client/app/src/main/cpp/cppNN-lib.cpp:250-257) under
// start_epoch("cross_entropy") or start_epoch("distillation"). One case is one getGradients
// call in the single-thread order: B train_class calls with the shifts given (sample k takes
// batch slot k), then cnn.DPgradients(C, sigma) where sigma > 0 and cnn.gradients() otherwise
// (cppNN-lib.cpp:218-221).
//
//   ref_client_dp_driver IN OUT
//     IN : w[21448], b[82], i32 n_cases, then per case
//          i32 B, i32 cost (0 cross_entropy, 1 distillation), f32 clip, f32 sigma,
//          images[B][784], i32 labels[B], i32 shift[B][2]
//   OUT: i32 n_draws = 22961, f64 draws[n_draws]: std::normal_distribution<double>(0.0, 1.0) on a
//        default-constructed std::default_random_engine, what addGaussian draws from on every
//        call, before scaling; then per case, per sample: f32 E, node[10] and delta[10] of FC2
//        after train_class; then per sample f32 sqsum, sqsum_layout, norm, scale: the walk of
//        scale_gradients restated over the reference's own dW_sets / dbias_sets before
//        DPgradients runs (sqsum_layout: the same squares added in the gradients() order; slot 0
//        is recorded too, though the reference never clips it); then the f32 vector [22961]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "mojo.h"

namespace {

std::vector<char> slurp(const char* path) {
  std::vector<char> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  char buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

struct Reader {
  const char* p;
  const char* end;
  template <typename T>
  bool get(T* out, size_t n = 1) {
    if ((size_t)(end - p) < sizeof(T) * n) return false;
    std::memcpy(out, p, sizeof(T) * n);
    p += sizeof(T) * n;
    return true;
  }
};

int run_case(Reader& in, const std::vector<float>& w, const std::vector<float>& b, FILE* out) {
  int32_t B = 0, cost = 0;
  float clip = 0, sigma = 0;
  if (!in.get(&B) || !in.get(&cost) || !in.get(&clip) || !in.get(&sigma) || B <= 0) return 2;
  std::vector<float> images((size_t)B * 784);
  std::vector<int32_t> labels(B), shift((size_t)B * 2);
  if (!in.get(images.data(), images.size()) || !in.get(labels.data(), B) || !in.get(shift.data(), shift.size()))
    return 2;
  mojo::network cnn("sgd");
  cnn.push_back("I1", "input 28 28 1");
  cnn.push_back("C1", "convolution 5 8 1 elu");
  cnn.push_back("P1", "semi_stochastic_pool 3 3");
  cnn.push_back("C2i", "convolution 1 16 1 elu");
  cnn.push_back("C2", "convolution 5 48 1 elu");
  cnn.push_back("P2", "semi_stochastic_pool 2 2");
  cnn.push_back("FC2", "softmax 10");
  cnn.connect_all();
  cnn.start_epoch(cost ? "distillation" : "cross_entropy");
  cnn.set_smart_training(false);
  cnn.set_mini_batch_size(B);
  cnn.set_random_augmentation(1, 1, 0, 0, mojo::edge);
  size_t ow = 0, ob = 0;
  for (auto* m : cnn.W)
    if (m) {
      if (ow + m->size() > w.size()) return 3;
      std::memcpy(m->x, w.data() + ow, sizeof(float) * m->size());
      ow += m->size();
    }
  auto& layers = cnn.layer_sets[mojo::network::MAIN_LAYER_SET];
  for (auto* l : layers)
    if (l->use_bias()) {
      if (ob + l->bias.size() > b.size()) return 3;
      std::memcpy(l->bias.x, b.data() + ob, sizeof(float) * l->bias.size());
      ob += l->bias.size();
    }
  if (ow != w.size() || ob != b.size() || layers.size() != 7) return 3;
  std::vector<float> teacher_prob(10, 0.1f);
  cnn.use_augmentation = 0;
  for (int k = 0; k < B; k++) {
    mojo::matrix m(28, 28, 1, images.data() + (size_t)k * 784);
    mojo::matrix shifted = m.shift(shift[2 * k], shift[2 * k + 1], mojo::edge);
    if (!cnn.train_class(shifted.x, labels[k], &teacher_prob, 0)) return 4;
    const mojo::matrix& node = layers[6]->node;
    float E = 0;
    for (int j = 0; j < 10; j++) {
      const float target = (labels[k] >= 0 && labels[k] < 10 && j == labels[k]) ? 1 : 0;
      float f = mojo::mse::cost(node.x[j], target, 0, 0);
      E += f;
    }
    E /= (float)10;
    std::fwrite(&E, 4, 1, out);
    std::fwrite(node.x, 4, 10, out);
    std::fwrite(layers[6]->delta.x, 4, 10, out);
  }
  for (int s = 0; s < B; s++) {
    float sqsum = 0, layout = 0;
    for (int k = (int)layers.size() - 1; k >= 0; k--) {
      for (auto& link : layers[k]->backward_linked_layers) {
        const mojo::matrix& dw = cnn.dW_sets[s][link.first];
        for (int j = 0; j < dw.size(); j++) sqsum += dw.x[j] * dw.x[j];
      }
      const mojo::matrix& db = cnn.dbias_sets[s][k];
      for (int j = 0; j < db.size(); j++) sqsum += db.x[j] * db.x[j];
    }
    for (size_t i = 0; i < cnn.dW_sets[s].size(); i++)
      for (int j = 0; j < cnn.dW_sets[s][i].size(); j++) layout += cnn.dW_sets[s][i].x[j] * cnn.dW_sets[s][i].x[j];
    for (size_t i = 0; i < cnn.dbias_sets[s].size(); i++)
      for (int j = 0; j < cnn.dbias_sets[s][i].size(); j++)
        layout += cnn.dbias_sets[s][i].x[j] * cnn.dbias_sets[s][i].x[j];
    float norm = sqrt(sqsum);
    float scale = 1 / std::max<float>(1.0, norm / clip);
    const float rec[4] = {sqsum, layout, norm, scale};
    std::fwrite(rec, 4, 4, out);
  }
  const std::vector<float> g = sigma > 0 ? cnn.DPgradients(clip, sigma) : cnn.gradients();
  if (g.size() != 22961) return 5;
  std::fwrite(g.data(), 4, g.size(), out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: ref_client_dp_driver IN OUT\n");
    return 2;
  }
  const std::vector<char> in = slurp(argv[1]);
  FILE* out = std::fopen(argv[2], "wb");
  if (in.empty() || !out) return 2;
  Reader r{in.data(), in.data() + in.size()};
  std::vector<float> w(21448), b(82);
  int32_t n = 0;
  if (!r.get(w.data(), w.size()) || !r.get(b.data(), b.size()) || !r.get(&n)) return 2;
  {
    const int32_t n_draws = 22961;
    std::default_random_engine generator;
    std::normal_distribution<double> dist(0.0, 1.0);
    std::vector<double> z(n_draws);
    for (auto& v : z) v = dist(generator);
    std::fwrite(&n_draws, 4, 1, out);
    std::fwrite(z.data(), 8, z.size(), out);
  }
  int rc = 0;
  for (int i = 0; i < n && !rc; i++) rc = run_case(r, w, b, out);
  std::fclose(out);
  return rc;
}

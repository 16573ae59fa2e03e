// tests/native/ref_client_grad_driver.cpp -- records tests/golden/client_grad_ref.npz from the
// reference's own network class (tests/golden/make_client_grad_golden.py compiles this into a
// temporary directory with the reference's flags, -std=c++11 -O0 -DDISTILLATION_MODE=1, against
// commonLib/cppNN, plus -fno-access-control). Nothing of it, and nothing compiled from it, is
// kept in the repository.
//
// The network is the client's (Client/app/src/main/cpp/cppNN-lib.cpp:250-257: the MNIST
// network of Driver/src/main/c++/cppNN_backend.cpp:109-115, start_epoch("cross_entropy"),
// set_mini_batch_size(B), set_random_augmentation(1, 1, 0, 0, mojo::edge)). One case is one
// getGradients call in the single-thread order: B train_class calls on layer set 0
// (cppNN-lib.cpp:110-115), sample k taking batch slot k, then cnn.gradients() (:221).
//
//   ref_client_grad_driver IN OUT
//     IN : w[21448], b[82], i32 n_cases, then per case
//          i32 B, i32 teacher (1: a non-NULL teacher_prob as the client passes, so the forward
//          runs at TEMPERATURE = 2; 0: NULL, temperature 1), i32 mode, i32 seed,
//          images[B][784], i32 labels[B], i32 shift[B][2]
//          mode 0: the shift is given: augmentation off, the sample is
//                  matrix(28, 28, 1, in).shift(dx, dy, mojo::edge), train_class's own call
//                  (network.h:1825, 1840) with the two draws replaced by the given values
//          mode 1: srand(seed), augmentation on: train_class draws the shifts itself
//   OUT: per case, per sample: f32 input[784] (layer I1's node after the forward), f32 E
//        (network.h:1974-1982 restated), node[7898] of all seven layers in order, i32 p_map of
//        P1 [512] and P2 [192], delta[7898] after backward_hidden; then f32 gradients()[22961]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// a layer's matrix, channel by channel (chan_stride may exceed cols*rows)
void put(FILE* out, const mojo::matrix& m) {
  for (int c = 0; c < m.chans; c++) std::fwrite(m.x + (size_t)c * m.chan_stride, 4, (size_t)m.cols * m.rows, out);
}

int run_case(Reader& in, const std::vector<float>& w, const std::vector<float>& b, FILE* out) {
  int32_t B = 0, teacher = 0, mode = 0, seed = 0;
  if (!in.get(&B) || !in.get(&teacher) || !in.get(&mode) || !in.get(&seed) || B <= 0) return 2;
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
  cnn.start_epoch("cross_entropy");
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
  if (mode == 1) srand((unsigned)seed);
  std::vector<float> teacher_prob(10, 0.1f);
  for (int k = 0; k < B; k++) {
    float* img = images.data() + (size_t)k * 784;
    mojo::matrix shifted;
    if (mode == 0) {
      cnn.use_augmentation = 0;
      mojo::matrix m(28, 28, 1, img);
      shifted = m.shift(shift[2 * k], shift[2 * k + 1], mojo::edge);
      img = shifted.x;
    }
    if (!cnn.train_class(img, labels[k], teacher ? &teacher_prob : NULL, 0)) return 4;
    put(out, layers[0]->node);
    const mojo::matrix& node = layers[6]->node;
    float E = 0;
    for (int j = 0; j < 10; j++) {
      const float target = (labels[k] >= 0 && labels[k] < 10 && j == labels[k]) ? 1 : 0;
      float f = mojo::mse::cost(node.x[j], target, 0, 0);
      E += f;
    }
    E /= (float)10;
    std::fwrite(&E, 4, 1, out);
    for (auto* l : layers) put(out, l->node);
    for (int p : {2, 5}) {
      auto* pool = dynamic_cast<mojo::max_pooling_layer*>(layers[p]);
      if (!pool) return 3;
      std::vector<int32_t> map(pool->_max_map.begin(), pool->_max_map.end());
      std::fwrite(map.data(), 4, map.size(), out);
    }
    for (auto* l : layers) put(out, l->delta);
  }
  const std::vector<float> g = cnn.gradients();
  if (g.size() != 22961) return 5;
  std::fwrite(g.data(), 4, g.size(), out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: ref_client_grad_driver IN OUT\n");
    return 2;
  }
  const std::vector<char> in = slurp(argv[1]);
  FILE* out = std::fopen(argv[2], "wb");
  if (in.empty() || !out) return 2;
  Reader r{in.data(), in.data() + in.size()};
  std::vector<float> w(21448), b(82);
  int32_t n = 0;
  if (!r.get(w.data(), w.size()) || !r.get(b.data(), b.size()) || !r.get(&n)) return 2;
  int rc = 0;
  for (int i = 0; i < n && !rc; i++) rc = run_case(r, w, b, out);
  std::fclose(out);
  return rc;
}

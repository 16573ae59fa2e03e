// tests/native/ref_cifar_driver.cpp -- records tests/golden/cifar_ref.npz from the reference's
// own network class (tests/golden/make_cifar_golden.py compiles this into a temporary
// directory with the reference's flags, -std=c++11 -O0 -DDISTILLATION_MODE=1, against
// commonLib/cppNN, plus -fno-access-control). Nothing of it, and nothing compiled from it,
// is kept in the repository.
//
// The network is the CIFAR one of Driver/src/main/c++/cppNN_backend.cpp:128-138, set up as
// initializeNative sets a network up (:87-93, push_back + connect_all), and evaluated by the
// loop of test() (:53-75), restated here with the per-image values kept, as
// ref_eval_driver.cpp does for the MNIST network.
//
//   ref_cifar_driver IN OUT
//     IN : i32 N (10 or 100), i32 B, i32 P (0, or B for a second pass over a permutation),
//          i32 L (images whose layer nodes are written, from the first), w[] (the non-null W
//          in order), b[] (the use_bias() layers' biases in layer order), images[B][3072],
//          i32 labels[B], i32 perm[P]
//   OUT: i32 n_w, i32 n_b, i32 c1_chan_stride (what the class itself holds), then
//        i32 pred[B], f32 p[B], f32 cost[B], f32 probs[B][N], f32 error[B], f32 accuracy[B],
//        i32 correct[B] (the last three: test() over the first k + 1 images); per image of the
//        first L: C1 [16][900] (read at the node's own chan_stride, the padding dropped),
//        P1 [16][196], C2 [64][144], P2 [64][9], local4 [384], local5 [192], FC2 [N]; with a
//        permutation f32 error, f32 accuracy, i32 correct of test() over images[perm[k]]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
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

// a layer's node, map by map at its own chan_stride, the padding behind a map dropped
void write_node(mojo::base_layer* l, FILE* out) {
  const int map = l->node.cols * l->node.rows;
  for (int c = 0; c < l->node.chans; c++) std::fwrite(l->node.x + (size_t)c * l->node.chan_stride, 4, map, out);
}

int run_test(mojo::network& cnn, int N, const std::vector<float>& images, const std::vector<int32_t>& labels,
             const std::vector<int32_t>* order, int B, int L, FILE* out, bool per_image) {
  if (cnn.out_size() != N) return 3;
  std::vector<int32_t> pred(B), correct(B);
  std::vector<float> p(B), cost(B), probs((size_t)B * N), err(B), acc(B);
  int correct_predictions = 0;
  float error = 0;
  std::vector<mojo::base_layer*>& layers = cnn.layer_sets[mojo::network::MAIN_LAYER_SET];
  FILE* nodes = L ? std::tmpfile() : NULL;
  for (int k = 0; k < B; k++) {
    const int row = order ? (*order)[k] : k;
    const float* img = images.data() + (size_t)row * 3072;
    const std::tuple<int, double> result = cnn.predict_class(img);
    std::memcpy(&probs[(size_t)k * N], layers.back()->node.x, sizeof(float) * N);
    if (k < L)
      for (size_t i = 1; i < layers.size(); i++) write_node(layers[i], nodes);
    const float c = mojo::mse::cost(std::get<1>(result), labels[row], 0, 0);
    error += c;
    const double prediction = std::get<0>(result);
    if (prediction == labels[row]) correct_predictions += 1;
    pred[k] = std::get<0>(result);
    p[k] = (float)std::get<1>(result);
    cost[k] = c;
    const int record_cnt = k + 1;
    float e = error;
    e /= (float)record_cnt;
    err[k] = e;
    acc[k] = (float)correct_predictions / record_cnt * 100.f;
    correct[k] = correct_predictions;
  }
  if (per_image) {
    std::fwrite(pred.data(), 4, B, out);
    std::fwrite(p.data(), 4, B, out);
    std::fwrite(cost.data(), 4, B, out);
    std::fwrite(probs.data(), 4, (size_t)B * N, out);
    std::fwrite(err.data(), 4, B, out);
    std::fwrite(acc.data(), 4, B, out);
    std::fwrite(correct.data(), 4, B, out);
    if (nodes) {
      std::rewind(nodes);
      char buf[1 << 16];
      size_t n;
      while ((n = std::fread(buf, 1, sizeof buf, nodes)) > 0) std::fwrite(buf, 1, n, out);
    }
  } else {
    std::fwrite(&err[B - 1], 4, 1, out);
    std::fwrite(&acc[B - 1], 4, 1, out);
    std::fwrite(&correct[B - 1], 4, 1, out);
  }
  if (nodes) std::fclose(nodes);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: ref_cifar_driver IN OUT\n");
    return 2;
  }
  const std::vector<char> raw = slurp(argv[1]);
  FILE* out = std::fopen(argv[2], "wb");
  if (raw.empty() || !out) return 2;
  Reader in{raw.data(), raw.data() + raw.size()};
  int32_t N = 0, B = 0, P = 0, L = 0;
  if (!in.get(&N) || !in.get(&B) || !in.get(&P) || !in.get(&L) || (N != 10 && N != 100) || B <= 0 ||
      (P != 0 && P != B) || L < 0 || L > B)
    return 2;

  mojo::network cnn("sgd");
  cnn.enable_external_threads();
  cnn.set_smart_training(false);
  cnn.set_random_augmentation(1, 1, 0, 0, mojo::edge);
  cnn.push_back("I1", "input 32 32 3");
  cnn.push_back("C1", "convolution 3 16 1 elu");
  cnn.push_back("P1", "max_pool 3 2");
  cnn.push_back("C2", "convolution 3 64 1 elu");
  cnn.push_back("P2", "max_pool 4 4");
  cnn.push_back("local4", "fully_connected 384 relu");
  cnn.push_back("local5", "fully_connected 192 relu");
  cnn.push_back("FC2", N == 10 ? "softmax 10" : "softmax 100");
  cnn.connect_all();

  int32_t n_w = 0, n_b = 0;
  for (auto* m : cnn.W)
    if (m) n_w += m->size();
  std::vector<mojo::base_layer*>& layers = cnn.layer_sets[mojo::network::MAIN_LAYER_SET];
  for (auto* l : layers)
    if (l->use_bias()) n_b += l->bias.size();
  std::vector<float> w(n_w), b(n_b), images((size_t)B * 3072);
  std::vector<int32_t> labels(B), perm(P);
  if (!in.get(w.data(), w.size()) || !in.get(b.data(), b.size()) || !in.get(images.data(), images.size()) ||
      !in.get(labels.data(), labels.size()) || !in.get(perm.data(), perm.size()))
    return 2;
  for (int32_t v : perm)
    if (v < 0 || v >= B) return 2;
  size_t ow = 0, ob = 0;
  for (auto* m : cnn.W)
    if (m) {
      std::memcpy(m->x, w.data() + ow, sizeof(float) * m->size());
      ow += m->size();
    }
  for (auto* l : layers)
    if (l->use_bias()) {
      std::memcpy(l->bias.x, b.data() + ob, sizeof(float) * l->bias.size());
      ob += l->bias.size();
    }
  const int32_t c1_stride = layers[1]->node.chan_stride;
  std::fwrite(&n_w, 4, 1, out);
  std::fwrite(&n_b, 4, 1, out);
  std::fwrite(&c1_stride, 4, 1, out);
  int rc = run_test(cnn, N, images, labels, NULL, B, L, out, true);
  if (!rc && P) rc = run_test(cnn, N, images, labels, &perm, B, 0, out, false);
  std::fclose(out);
  return rc;
}

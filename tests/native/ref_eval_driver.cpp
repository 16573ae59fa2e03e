// tests/native/ref_eval_driver.cpp -- records tests/golden/eval_ref.npz from the reference's
// own network class (tests/golden/make_eval_golden.py compiles this into a temporary
// directory with the reference's flags, -std=c++11 -O0 -DDISTILLATION_MODE=1, against
// commonLib/cppNN, plus -fno-access-control). Nothing of it, and nothing compiled from it,
// is kept in the repository.
//
// The network is set up as the Driver's initializeNative sets it up
// (Driver/src/main/c++/cppNN_backend.cpp:87-117) and evaluated by the loop of its test()
// (:53-75), restated here with the per-image values kept: predict_class per image,
// mse::cost on its probability and the label, the binary32 running sum, and after every
// image what test(..., sample = k + 1) would return.
//
//   ref_eval_driver class IN OUT   the network of :109-115 built by push_back, weights set
//     IN : i32 B, i32 P (0, or B for a second pass over a permutation), w[21448] (the
//          non-null W in order), b[82] (the use_bias() layers' biases in layer order),
//          images[B][784], i32 labels[B], i32 perm[P]
//   ref_eval_driver text IN OUT    cnn.read(text) as fetchParamsNative does (:179-198)
//     IN : i32 B, i32 chain, i32 text bytes, text, images[B][784], i32 labels[B]
//          chain 0: the text itself
//          chain 1: the server's version copy of it (Server/src/main/c++/cppNN_backend.cpp:
//                   176-192: a new network reading cnn.getParams())
//          chain 2: the broadcast text of that copy (getParametersNative, Server :253-259:
//                   save_model_weights, quantization_weight_model, getParams), read again
//   OUT: i32 pred[B], f32 p[B], f32 cost[B], f32 probs[B][10], f32 error[B], f32 accuracy[B],
//        i32 correct[B] (the last three: test() over the first k + 1 images), then with a
//        permutation f32 error, f32 accuracy, i32 correct of test() over images[perm[k]];
//        `text` appends what the evaluated network holds: w[21448], b[82]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
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

// initializeNative's calls before the model exists (:87-93)
void driver_setup(mojo::network& cnn) {
  cnn.enable_external_threads();
  cnn.set_smart_training(false);
  cnn.set_random_augmentation(1, 1, 0, 0, mojo::edge);
}

// fetchParamsNative (:187-195)
void fetch(mojo::network& cnn, const std::string& text) {
  cnn.start_epoch("distillation");
  cnn.set_random_augmentation(1, 1, 0, 0, mojo::edge);
  cnn.clear();
  std::istringstream ss(text);
  cnn.read(ss);
}

// test() (:53-75) over images[order[k]], the per-image values kept
int run_test(mojo::network& cnn, const std::vector<float>& images, const std::vector<int32_t>& labels,
             const std::vector<int32_t>* order, int B, FILE* out, bool per_image) {
  if (cnn.out_size() != 10) return 3;
  std::vector<int32_t> pred(B), correct(B);
  std::vector<float> p(B), cost(B), probs((size_t)B * 10), err(B), acc(B);
  int correct_predictions = 0;
  float error = 0;
  for (int k = 0; k < B; k++) {
    const int row = order ? (*order)[k] : k;
    const float* img = images.data() + (size_t)row * 784;
    const std::tuple<int, double> result = cnn.predict_class(img);
    const float* node = cnn.layer_sets[mojo::network::MAIN_LAYER_SET].back()->node.x;
    std::memcpy(&probs[(size_t)k * 10], node, sizeof(float) * 10);
    const float c = mojo::mse::cost(std::get<1>(result), labels[row], 0, 0);
    error += c;
    const double prediction = std::get<0>(result);
    if (prediction == labels[row]) correct_predictions += 1;
    pred[k] = std::get<0>(result);
    p[k] = (float)std::get<1>(result);
    cost[k] = c;
    // what test(cnn, images, labels, k + 1) returns
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
    std::fwrite(probs.data(), 4, (size_t)B * 10, out);
    std::fwrite(err.data(), 4, B, out);
    std::fwrite(acc.data(), 4, B, out);
    std::fwrite(correct.data(), 4, B, out);
  } else {
    std::fwrite(&err[B - 1], 4, 1, out);
    std::fwrite(&acc[B - 1], 4, 1, out);
    std::fwrite(&correct[B - 1], 4, 1, out);
  }
  return 0;
}

bool read_set(Reader& in, int B, std::vector<float>* images, std::vector<int32_t>* labels) {
  images->resize((size_t)B * 784);
  labels->resize(B);
  return in.get(images->data(), images->size()) && in.get(labels->data(), labels->size());
}

int run_class(Reader in, FILE* out) {
  int32_t B = 0, P = 0;
  if (!in.get(&B) || !in.get(&P) || B <= 0 || (P != 0 && P != B)) return 2;
  std::vector<float> w(21448), b(82), images;
  std::vector<int32_t> labels, perm(P);
  if (!in.get(w.data(), w.size()) || !in.get(b.data(), b.size()) || !read_set(in, B, &images, &labels) ||
      !in.get(perm.data(), perm.size()))
    return 2;
  for (int32_t v : perm)
    if (v < 0 || v >= B) return 2;
  mojo::network cnn("sgd");
  driver_setup(cnn);
  cnn.push_back("I1", "input 28 28 1");
  cnn.push_back("C1", "convolution 5 8 1 elu");
  cnn.push_back("P1", "semi_stochastic_pool 3 3");
  cnn.push_back("C2i", "convolution 1 16 1 elu");
  cnn.push_back("C2", "convolution 5 48 1 elu");
  cnn.push_back("P2", "semi_stochastic_pool 2 2");
  cnn.push_back("FC2", "softmax 10");
  cnn.connect_all();
  size_t ow = 0, ob = 0;
  for (auto* m : cnn.W)
    if (m) {
      if (ow + m->size() > w.size()) return 3;
      std::memcpy(m->x, w.data() + ow, sizeof(float) * m->size());
      ow += m->size();
    }
  for (auto* l : cnn.layer_sets[mojo::network::MAIN_LAYER_SET])
    if (l->use_bias()) {
      if (ob + l->bias.size() > b.size()) return 3;
      std::memcpy(l->bias.x, b.data() + ob, sizeof(float) * l->bias.size());
      ob += l->bias.size();
    }
  if (ow != w.size() || ob != b.size()) return 3;
  int rc = run_test(cnn, images, labels, NULL, B, out, true);
  if (!rc && P) rc = run_test(cnn, images, labels, &perm, B, out, false);
  return rc;
}

int run_text(Reader in, FILE* out) {
  int32_t B = 0, chain = 0, n_text = 0;
  if (!in.get(&B) || !in.get(&chain) || !in.get(&n_text) || B <= 0 || chain < 0 || chain > 2 || n_text <= 0) return 2;
  std::string text((size_t)n_text, '\0');
  std::vector<float> images;
  std::vector<int32_t> labels;
  if (!in.get(&text[0], text.size()) || !read_set(in, B, &images, &labels)) return 2;
  if (chain >= 1) {
    // the server: fetchParamsNative, then initUpdater's model copy
    mojo::network server("sgd");
    fetch(server, text);
    mojo::network copy("sgd");
    copy.start_epoch("distillation");
    copy.set_random_augmentation(1, 1, 0, 0, mojo::edge);
    std::string params = server.getParams();
    std::istringstream ss(params);
    copy.clear();
    copy.read(ss);
    text = params;
    if (chain == 2) {
      std::vector<mojo::matrix*> unquantized_W;
      copy.save_model_weights(&unquantized_W);
      copy.quantization_weight_model();
      text = copy.getParams();
      copy.load_model_weights(unquantized_W);
    }
  }
  mojo::network cnn("sgd");
  driver_setup(cnn);
  fetch(cnn, text);
  const int rc = run_test(cnn, images, labels, NULL, B, out, true);
  for (auto* m : cnn.W)
    if (m) std::fwrite(m->x, sizeof(float), m->size(), out);
  for (auto* l : cnn.layer_sets[mojo::network::MAIN_LAYER_SET])
    if (l->use_bias()) std::fwrite(l->bias.x, sizeof(float), l->bias.size(), out);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: ref_eval_driver class|text IN OUT\n");
    return 2;
  }
  const std::vector<char> in = slurp(argv[2]);
  FILE* out = std::fopen(argv[3], "wb");
  if (in.empty() || !out) return 2;
  Reader r{in.data(), in.data() + in.size()};
  const int rc = std::strcmp(argv[1], "text") ? run_class(r, out) : run_text(r, out);
  std::fclose(out);
  return rc;
}

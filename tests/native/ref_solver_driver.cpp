// tests/native/ref_solver_driver.cpp -- records tests/golden/solver_ref.npz from the
// reference's own classes (tests/golden/make_solver_golden.py compiles this into a
// temporary directory with the reference's flags, -std=c++11 -O0, against
// commonLib/cppNN, plus -fno-access-control: the solvers keep their state private).
// Nothing of it, and nothing compiled from it, is kept in the repository.
//
//   ref_solver_driver class IN OUT   new_solver(name)->increment_w on one matrix
//     IN : i32 solver (1 adagrad, 2 rmsprop, 3 adam), i32 N, i32 steps, f32 L,
//          w0[N], g1_0[N], g2_0[N] (the state the session continues from; zeros = a
//          fresh solver), d[steps][N]
//     OUT: per step w[N], g1[N], g2[N] (g2: zeros unless adam)
//   ref_solver_driver net IN OUT     mojo::network(name) reading a getParams text:
//     (adagrad's state, which the reference leaves uninitialised, zeroed first),
//     one train_class sizes the gradient sets (initUpdater, cppNN_backend.cpp:216-222),
//     then per step set_learning_rate(lr) and descent(vector) (descentNative, :336-352)
//     IN : i32 solver, i32 text bytes, i32 n_g, i32 steps, text, per step f32 lr, g[n_g]
//     OUT: i32 n_w, i32 n_b, then w0[n_w], b0[n_b] and per step w[n_w], b[n_b] (the
//          non-null W in order; the use_bias() layers' biases in layer order)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "mojo.h"

namespace {

const char* const kNames[] = {"sgd", "adagrad", "rmsprop", "adam"};

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

void put(FILE* f, const float* x, size_t n) { std::fwrite(x, sizeof(float), n, f); }

std::vector<mojo::matrix*>* state_of(mojo::solver* s, int solver, int which) {
  if (solver == 1) return which ? NULL : &static_cast<mojo::adagrad*>(s)->G1;
  if (solver == 2) return which ? NULL : &static_cast<mojo::rmsprop*>(s)->G1;
  mojo::adam* a = static_cast<mojo::adam*>(s);
  return which ? &a->G2 : &a->G1;
}

int run_class(Reader in, FILE* out) {
  int32_t solver = 0, N = 0, steps = 0;
  float L = 0;
  if (!in.get(&solver) || !in.get(&N) || !in.get(&steps) || !in.get(&L) || solver < 1 || solver > 3 || N <= 0) return 2;
  std::vector<float> w0(N), g1(N), g2(N), d((size_t)N * steps);
  if (!in.get(w0.data(), N) || !in.get(g1.data(), N) || !in.get(g2.data(), N) || !in.get(d.data(), d.size())) return 2;
  mojo::solver* s = mojo::new_solver(kNames[solver]);
  s->learning_rate = L;
  s->push_back(N, 1, 1);
  mojo::matrix w(N, 1, 1), dW(N, 1, 1);
  if (w.size() != N) return 3;
  std::memcpy(w.x, w0.data(), sizeof(float) * N);
  std::memcpy((*state_of(s, solver, 0))[0]->x, g1.data(), sizeof(float) * N);
  if (solver == 3) std::memcpy((*state_of(s, solver, 1))[0]->x, g2.data(), sizeof(float) * N);
  const std::vector<float> zeros(N, 0.0f);
  for (int i = 0; i < steps; ++i) {
    std::memcpy(dW.x, d.data() + (size_t)i * N, sizeof(float) * N);
    s->increment_w(&w, 0, dW);
    put(out, w.x, N);
    put(out, (*state_of(s, solver, 0))[0]->x, N);
    put(out, solver == 3 ? (*state_of(s, solver, 1))[0]->x : zeros.data(), N);
  }
  delete s;
  return 0;
}

int run_net(Reader in, FILE* out) {
  int32_t solver = 0, n_text = 0, n_g = 0, steps = 0;
  if (!in.get(&solver) || !in.get(&n_text) || !in.get(&n_g) || !in.get(&steps) || solver < 0 || solver > 3) return 2;
  std::string text((size_t)n_text, '\0');
  if (!in.get(&text[0], text.size())) return 2;
  mojo::network cnn(kNames[solver]);
  {
    std::istringstream ss(text);
    cnn.start_epoch("distillation");
    cnn.set_random_augmentation(1, 1, 0, 0, mojo::edge);
    cnn.clear();
    cnn.read(ss);
  }
  // adagrad::push_back leaves G1 as the heap gave it (its fill(0) is commented out,
  // solver.h:105-107), where rmsprop and adam fill theirs: the session is recorded from
  // the zero state the other two start from, which is what this project defines
  if (solver == 1)
    for (mojo::matrix* m : *state_of(cnn._solver, solver, 0)) m->fill(0.f);
  auto& layers = cnn.layer_sets[mojo::network::MAIN_LAYER_SET];
  {
    const mojo::matrix& node = layers.front()->node;
    std::vector<float> blank((size_t)node.cols * node.rows * node.chans, 0.0f);
    const int n_out = layers.back()->node.size();
    std::vector<float> teacher((size_t)n_out, 1.0f / (float)n_out);
    cnn.train_class(blank.data(), 0, &teacher);
  }
  std::vector<float> w, b;
  auto snapshot = [&]() {
    w.clear();
    b.clear();
    for (auto* m : cnn.W)
      if (m) w.insert(w.end(), m->x, m->x + m->size());
    for (auto* l : layers)
      if (l->use_bias()) b.insert(b.end(), l->bias.x, l->bias.x + l->bias.size());
  };
  snapshot();
  const int32_t n_w = (int32_t)w.size(), n_b = (int32_t)b.size();
  std::fwrite(&n_w, 4, 1, out);
  std::fwrite(&n_b, 4, 1, out);
  put(out, w.data(), w.size());
  put(out, b.data(), b.size());
  std::vector<float> g((size_t)n_g);
  for (int i = 0; i < steps; ++i) {
    float lr = 0;
    if (!in.get(&lr) || !in.get(g.data(), g.size())) return 2;
    cnn.set_learning_rate(lr);
    cnn.descent(g);
    snapshot();
    put(out, w.data(), w.size());
    put(out, b.data(), b.size());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: ref_solver_driver class|net IN OUT\n");
    return 2;
  }
  const std::vector<char> in = slurp(argv[2]);
  FILE* out = std::fopen(argv[3], "wb");
  if (in.empty() || !out) return 2;
  Reader r{in.data(), in.data() + in.size()};
  const int rc = std::strcmp(argv[1], "net") ? run_class(r, out) : run_net(r, out);
  std::fclose(out);
  return rc;
}

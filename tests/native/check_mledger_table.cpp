// tests/native/check_mledger_table.cpp -- the model ledger's host bookkeeping
// (fleet_amd/csrc/mledger_table.cpp) against a literal restatement of Kardam.setModel
// (Kardam.java:114-125) over random pick sequences: repeated workers inside one update,
// zero norms between distinct versions, NaN norms, skipped picks, rejected updates and
// eviction pressure. The norms come from a function of the two version ids, so no GPU is
// needed. Stand-alone: build with the table unit, run, exit status 0 and "ALL OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../fleet_amd/csrc/mledger_table.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}
int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

// getNorm(subtract(T_cur, T_prev)) as a function of the ORDERED pair of versions: 0 for a
// version against itself and for some distinct pairs, NaN for some, positive otherwise
double norm_of(int64_t cur, int64_t prev) {
  if (cur == prev) return 0.0;
  const uint64_t h = ((uint64_t)cur * 1000003ull + (uint64_t)prev * 7919ull + 12345ull) % 1009ull;
  if (h % 5 == 0) return 0.0;
  if (h % 11 == 0) return std::nan("");
  return 1.0 + (double)h / 8.0;
}

// Kardam.java:114-125, with a version id standing for the model text
struct Book {
  std::map<int, int64_t> models;
  std::map<int, double> modelDiffNorm;
  uint8_t last_status = 0;
  double last_norm = 0.0;
  void setModel(int workerId, int64_t mcurr) {
    last_status = fleet::kMlFirst, last_norm = std::nan("");
    if (models.count(workerId)) {
      const double norm = norm_of(mcurr, models[workerId]);
      last_norm = norm;
      if (norm == 0) {
        last_status = fleet::kMlIgnored;
        return;
      }
      last_status = fleet::kMlSet;
      modelDiffNorm[workerId] = norm;
    }
    models[workerId] = mcurr;
  }
};

// which versions are resident, restated: at most V that no worker holds, oldest staged leaves
struct Resident {
  std::map<int64_t, uint64_t> age;
  uint64_t clock = 0;
  void stage(int64_t id, const Book& b, int V) {
    if (age.count(id)) {
      age[id] = ++clock;
      return;
    }
    for (;;) {
      std::set<int64_t> held;
      for (const auto& m : b.models) held.insert(m.second);
      int unref = 0;
      int64_t oldest = -1;
      for (const auto& a : age) {
        if (held.count(a.first)) continue;
        ++unref;
        if (oldest < 0 || a.second < age[oldest]) oldest = a.first;
      }
      if (unref < V) break;
      age.erase(oldest);
    }
    age[id] = ++clock;
  }
};

long g_checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++g_checks;                                           \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

bool same_bits(double a, double b) { return (a != a && b != b) || a == b; }

void compare(const fleet::MledgerTable& t, const Book& b, const Resident& res, int W, int V) {
  std::map<int64_t, int> refs;
  for (int w = 0; w < W; ++w) {
    const int r = t.row_of_worker(w);
    CHECK((r >= 0) == (b.models.count(w) != 0), "worker %d: has %d", w, r >= 0);
    if (r < 0) continue;
    CHECK(t.id_of_row(r) == b.models.at(w), "worker %d holds %lld, the book %lld", w, (long long)t.id_of_row(r),
          (long long)b.models.at(w));
    CHECK(t.row_of_id(t.id_of_row(r)) == r, "worker %d's row %d is not its version's", w, r);
    ++refs[t.id_of_row(r)];
  }
  int resident = 0;
  for (int64_t id = -2; id < 40; ++id) {
    const int r = t.row_of_id(id);
    CHECK((r >= 0) == (res.age.count(id) != 0), "version %lld resident: %d", (long long)id, r >= 0);
    if (r < 0) continue;
    ++resident;
    CHECK(r < t.rows() && t.refs_of_row(r) == refs[id], "version %lld: %d references, the book %d", (long long)id,
          t.refs_of_row(r), refs[id]);
  }
  CHECK(resident <= W + V, "%d resident versions in %d rows", resident, W + V);
}

void trial(int W, int V, int steps, int ids) {
  fleet::MledgerTable t(W, V);
  Book book;
  Resident res;
  CHECK(t.rows() == W + V && t.workers() == W && t.max_versions() == V, "shape");
  for (int s = 0; s < steps; ++s) {
    const int op = rnd_in(0, 99);
    if (op < 35) {
      const int64_t id = rnd_in(0, ids - 1);
      const bool was = res.age.count(id) != 0;
      bool fresh = false;
      const int r = t.stage(id, &fresh);
      res.stage(id, book, V);
      CHECK(r >= 0 && r < t.rows() && fresh == !was, "stage %lld: row %d fresh %d", (long long)id, r, fresh);
      if (fresh && rnd_in(0, 9) == 0) {  // the fill failed
        t.unstage(id);
        res.age.erase(id);
      }
    } else if (op < 40) {
      const int w = rnd_in(0, W - 1);
      CHECK(t.forget(w) == (book.models.erase(w) != 0), "forget %d", w);
      book.modelDiffNorm.erase(w);
    } else {
      const int K = rnd_in(0, 14);
      std::vector<int64_t> id((size_t)K);
      std::vector<int32_t> wk((size_t)K);
      std::vector<int64_t> have;
      for (const auto& a : res.age) have.push_back(a.first);
      const bool few = rnd_in(0, 2) == 0;  // few workers: many repeats inside the update
      for (int k = 0; k < K; ++k) {
        wk[(size_t)k] = rnd_in(0, 11) == 0 ? -1 : rnd_in(0, 60) == 0 ? W + rnd_in(0, 2) : rnd_in(0, few ? std::min(W, 2) - 1 : W - 1);
        id[(size_t)k] = have.empty() || rnd_in(0, 40) == 0 ? rnd_in(-2, ids + 1) : have[(size_t)rnd_in(0, (int)have.size() - 1)];
      }
      bool valid = true;
      std::set<int64_t> held, fresh;
      for (const auto& m : book.models) held.insert(m.second);
      for (int k = 0; k < K; ++k) {
        if (wk[(size_t)k] < 0) continue;
        if (wk[(size_t)k] >= W || !res.age.count(id[(size_t)k])) valid = false;
        else if (!held.count(id[(size_t)k])) fresh.insert(id[(size_t)k]);
      }
      if ((int)fresh.size() > V) valid = false;
      std::string err;
      const bool ok = t.resolve(id.data(), wk.data(), K, &err);
      CHECK(ok == valid, "resolve: %d, expected %d (%s)", ok, valid, err.c_str());
      if (!ok) {
        CHECK(!err.empty(), "a rejection says why");
        compare(t, book, res, W, V);  // nothing changed
        continue;
      }
      const size_t P = t.pair_cur().size();
      CHECK(t.pair_prev().size() == P, "pair lists");
      std::set<std::pair<int, int>> seen;
      std::vector<double> norms(P);
      for (size_t i = 0; i < P; ++i) {
        const int c = t.pair_cur()[i], p = t.pair_prev()[i];
        CHECK(c >= 0 && c < t.rows() && p >= 0 && p < t.rows(), "pair %zu rows %d %d", i, c, p);
        CHECK(seen.insert({c, p}).second, "pair (%d, %d) listed twice", c, p);
        norms[i] = norm_of(t.id_of_row(c), t.id_of_row(p));
      }
      compare(t, book, res, W, V);  // resolve changed nothing
      {  // every pair the reference's loop will ask for is listed
        Book ahead = book;
        for (int k = 0; k < K; ++k) {
          if (wk[(size_t)k] < 0) continue;
          if (ahead.models.count(wk[(size_t)k])) {
            const int c = t.row_of_id(id[(size_t)k]), p = t.row_of_id(ahead.models[wk[(size_t)k]]);
            CHECK(seen.count({c, p}) != 0, "pick %d needs the pair (%d, %d), which is not listed", k, c, p);
          }
          ahead.setModel(wk[(size_t)k], id[(size_t)k]);
        }
      }
      std::vector<double> nd((size_t)K, -7.0);
      std::vector<uint8_t> st((size_t)K, 99);
      t.replay(norms.data(), nd.data(), st.data());
      int active = 0;
      for (int k = 0; k < K; ++k) {
        if (wk[(size_t)k] < 0) {
          CHECK(st[(size_t)k] == fleet::kMlSkipped && nd[(size_t)k] != nd[(size_t)k] && t.pick_row(k) == -1, "skipped pick %d", k);
          continue;
        }
        ++active;
        book.setModel(wk[(size_t)k], id[(size_t)k]);
        CHECK(st[(size_t)k] == book.last_status, "pick %d: status %d, the book %d", k, st[(size_t)k], book.last_status);
        CHECK(same_bits(nd[(size_t)k], book.last_norm), "pick %d: norm %g, the book %g", k, nd[(size_t)k], book.last_norm);
        CHECK(t.id_of_row(t.pick_row(k)) == id[(size_t)k], "pick %d's row", k);
      }
      CHECK(t.active() == active, "active picks");
      compare(t, book, res, W, V);
    }
  }
}

}  // namespace

int main() {
  for (int round = 0; round < 300; ++round) {
    const int W = rnd_in(1, 6), V = rnd_in(1, 4);
    trial(W, V, 150, rnd_in(2, 12));
  }
  trial(3, 1, 2000, 4);    // eviction at every other stage
  trial(2, 2, 2000, 3);    // three versions, two workers: A -> B -> A chains
  trial(10, 3, 2000, 20);
  std::printf("%ld checks\nALL OK\n", g_checks);
  return 0;
}

// tests/native/check_dev_mem.cpp -- fleet_amd/csrc/dev_mem.h against a fake HIP allocator.
//
// Stand-alone: hipMalloc, hipFree, hipHostMalloc, hipHostFree and hipMemset are defined
// here over malloc (as fakejvm.cpp does for JNI), so nothing of the HIP runtime is linked.
// The fakes tag every allocation device or pinned, record every size asked for, count what
// is live, can fail the k-th call, and abort on a free of the wrong kind, a double free or
// a free of a pointer they never gave out.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../fleet_amd/csrc/dev_mem.h"

namespace {

enum Kind { kDevice, kPinned };
struct Block {
  Kind kind;
  size_t bytes;
  bool live;
};
std::map<void*, Block> g_blocks;  // every pointer ever handed out (never reused: freed blocks stay allocated)
std::vector<std::pair<Kind, size_t>> g_asked;  // every allocation call, failed ones included
int g_calls = 0, g_fail_at = -1, g_live = 0, g_frees = 0, g_memsets = 0;

[[noreturn]] void die(const char* what, void* p) {
  std::printf("FAKE HIP ABORT: %s (%p)\n", what, p);
  std::fflush(stdout);
  std::abort();
}

bool fails_now() { return g_calls++ == g_fail_at; }

hipError_t fake_alloc(void** out, size_t bytes, Kind kind) {
  g_asked.push_back({kind, bytes});
  if (fails_now()) {
    *out = (void*)(uintptr_t)0xdead0;  // a failed call's output is never to be used or freed
    return hipErrorOutOfMemory;
  }
  void* p = std::malloc(bytes ? bytes : 1);
  std::memset(p, 0xa5, bytes);
  g_blocks[p] = {kind, bytes, true};
  ++g_live;
  *out = p;
  return hipSuccess;
}

hipError_t fake_free(void* p, Kind kind) {
  auto it = g_blocks.find(p);
  if (it == g_blocks.end()) die("free of a pointer the allocator never gave out", p);
  if (!it->second.live) die("double free", p);
  if (it->second.kind != kind) die("free of the wrong kind (device / pinned)", p);
  it->second.live = false;  // the memory stays allocated: no later block takes its address
  --g_live;
  ++g_frees;
  return hipSuccess;
}

void fake_reset(int fail_at = -1) {
  for (auto& b : g_blocks) {
    if (b.second.live) die("a block is still live when the case ends", b.first);
    std::free(b.first);
  }
  g_blocks.clear();
  g_asked.clear();
  g_calls = g_live = g_frees = g_memsets = 0;
  g_fail_at = fail_at;
}

bool is_live(void* p) {
  auto it = g_blocks.find(p);
  return it != g_blocks.end() && it->second.live;
}

int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes, kDevice); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) {
  if (flags != hipHostMallocDefault) die("hipHostMalloc flags are not hipHostMallocDefault", nullptr);
  return fake_alloc(p, bytes, kPinned);
}
hipError_t hipFree(void* p) { return fake_free(p, kDevice); }
hipError_t hipHostFree(void* p) { return fake_free(p, kPinned); }
hipError_t hipMemset(void* p, int v, size_t bytes) {
  ++g_memsets;
  if (fails_now()) return hipErrorInvalidValue;
  auto it = g_blocks.find(p);
  if (it == g_blocks.end() || !it->second.live || it->second.kind != kDevice || bytes > it->second.bytes)
    die("hipMemset outside a live device block", p);
  std::memset(p, v, bytes);
  return hipSuccess;
}
}

using fleet::DevBuf;
using fleet::PinBuf;
using fleet::Retired;

// 1. every allocation made in a scope is freed by the matching call when the scope ends
static void case_scope_exit() {
  fake_reset();
  {
    DevBuf<float> d;
    PinBuf<int> h;
    DevBuf<void> slab;
    PinBuf<volatile int> hv;
    CHECK(!d && !h && d.get() == nullptr && d.cap() == 0);
    CHECK(d.alloc(10) == hipSuccess && h.alloc(16) == hipSuccess && slab.alloc(100, 64) == hipSuccess);
    CHECK(hv.alloc(16) == hipSuccess);
    CHECK(d && h && d.cap() == 10 && h.cap() == 16 && slab.cap() == 100 && g_live == 4);
    hv[1] = 7;  // the volatile read path of the accumulator's error words
    CHECK(hv[1] == 7);
    d.reset();
    CHECK(!d && d.cap() == 0 && g_live == 3);
    d.reset();  // a second reset frees nothing
    CHECK(g_frees == 1);
  }
  CHECK(g_live == 0 && g_frees == 4);
  CHECK(g_asked.size() == 4 && g_asked[0] == std::make_pair(kDevice, 10 * sizeof(float)) &&
        g_asked[1] == std::make_pair(kPinned, 16 * sizeof(int)) && g_asked[2] == std::make_pair(kDevice, (size_t)164) &&
        g_asked[3] == std::make_pair(kPinned, 16 * sizeof(int)));
}

// 2. moves: one free per allocation, the source left empty
static void case_moves() {
  fake_reset();
  {
    DevBuf<int> a;
    CHECK(a.alloc(4) == hipSuccess);
    int* pa = a.get();
    DevBuf<int> b(std::move(a));  // move-construct
    CHECK(!a && a.cap() == 0 && b.get() == pa && b.cap() == 4 && g_live == 1);
    DevBuf<int> c;
    CHECK(c.alloc(8) == hipSuccess);
    int* pc = c.get();
    c = std::move(b);  // move-assign onto a full buffer: its own allocation is freed now
    CHECK(!b && b.cap() == 0 && c.get() == pa && c.cap() == 4 && !is_live(pc) && g_live == 1 && g_frees == 1);
    DevBuf<int>& self = c;
    c = std::move(self);  // self-move keeps the allocation
    CHECK(c.get() == pa && c.cap() == 4 && g_live == 1 && g_frees == 1);
    PinBuf<uint8_t> h, k;
    CHECK(h.alloc(32) == hipSuccess);
    uint8_t* ph = h.get();
    k = std::move(h);
    PinBuf<uint8_t> m(std::move(k));
    PinBuf<uint8_t>& mself = m;
    m = std::move(mself);
    CHECK(!h && !k && m.get() == ph && m.cap() == 32 && g_live == 2);
    // a struct of buffers moves member by member (Window into its handle)
    struct Two {
      size_t n = 0;
      DevBuf<int> x, y;
    } w, v;
    CHECK(w.x.alloc(1) == hipSuccess && w.y.alloc(2) == hipSuccess);
    w.n = 5;
    v = std::move(w);
    CHECK(!w.x && !w.y && v.x && v.y && v.n == 5 && g_live == 4);
  }
  CHECK(g_live == 0 && g_frees == 5 && g_asked.size() == 5);
}

// 3. grow: nothing when need <= cap, the policies' sizes, a failed grow
static void case_grow() {
  fake_reset();
  {
    DevBuf<double> d;
    CHECK(d.grow_doubling(10) == hipSuccess && d.cap() == 10);
    CHECK(g_asked.back() == std::make_pair(kDevice, 10 * sizeof(double) + 64));
    double* p0 = d.get();
    const int calls = g_calls;
    CHECK(d.grow_doubling(10) == hipSuccess && d.grow_doubling(3) == hipSuccess && d.grow_exact(10) == hipSuccess);
    CHECK(g_calls == calls && d.get() == p0 && g_frees == 0);  // need <= cap: no call
    CHECK(d.grow_doubling(11) == hipSuccess && d.cap() == 20);  // max(11, 2 * 10)
    CHECK(g_asked.back() == std::make_pair(kDevice, 20 * sizeof(double) + 64) && !is_live(p0) && g_frees == 1);
    CHECK(d.grow_doubling(100) == hipSuccess && d.cap() == 100);  // max(100, 2 * 20)
    CHECK(g_asked.back() == std::make_pair(kDevice, 100 * sizeof(double) + 64) && g_frees == 2 && g_live == 1);

    DevBuf<float> e;
    CHECK(e.grow_exact(7, 64) == hipSuccess && e.cap() == 7);
    CHECK(g_asked.back() == std::make_pair(kDevice, 7 * sizeof(float) + 64));
    CHECK(e.grow_exact(9) == hipSuccess && e.cap() == 9);
    CHECK(g_asked.back() == std::make_pair(kDevice, 9 * sizeof(float)) && g_frees == 3);

    PinBuf<uint8_t> h;
    CHECK(h.grow_doubling(1000) == hipSuccess && g_asked.back() == std::make_pair(kPinned, (size_t)1064));
    CHECK(h.grow_doubling(1001) == hipSuccess && h.cap() == 2000 && g_asked.back() == std::make_pair(kPinned, (size_t)2064));
    CHECK(h.grow_exact(2001) == hipSuccess && h.cap() == 2001 && g_asked.back() == std::make_pair(kPinned, (size_t)2001));
    CHECK(g_frees == 5);

    // a failed grow: empty, capacity 0, the old allocation freed once; the next grow starts over
    float* pe = e.get();
    g_fail_at = g_calls;
    CHECK(e.grow_doubling(50) == hipErrorOutOfMemory);
    CHECK(!e && e.get() == nullptr && e.cap() == 0 && !is_live(pe) && g_frees == 6);
    CHECK(e.grow_doubling(5) == hipSuccess && e.cap() == 5 && g_asked.back() == std::make_pair(kDevice, 5 * sizeof(float) + 64));
    uint8_t* ph = h.get();
    g_fail_at = g_calls;
    CHECK(h.grow_exact(5000) == hipErrorOutOfMemory && !h && h.cap() == 0 && !is_live(ph) && g_frees == 7);
  }
  CHECK(g_live == 0);
}

// 4. a retiring grow keeps the old allocation live until the Retired dies
static void case_retire() {
  fake_reset();
  void *p0, *p1;
  {
    Retired r;
    {
      DevBuf<double> d;
      CHECK(d.grow_exact(4, 64, &r) == hipSuccess && r.size() == 0);  // nothing to retire yet
      p0 = d.get();
      CHECK(d.grow_exact(4, 64, &r) == hipSuccess && d.get() == p0 && r.size() == 0);
      CHECK(d.grow_exact(6, 64, &r) == hipSuccess && r.size() == 1);
      p1 = d.get();
      CHECK(p1 != p0 && is_live(p0) && g_frees == 0 && g_asked.back() == std::make_pair(kDevice, 6 * sizeof(double) + 64));
      // a failed retiring grow: the old one is retired all the same, the buffer is empty
      g_fail_at = g_calls;
      CHECK(d.grow_exact(8, 64, &r) == hipErrorOutOfMemory && !d && d.cap() == 0 && r.size() == 2);
      CHECK(is_live(p0) && is_live(p1) && g_frees == 0);
    }
    CHECK(is_live(p0) && is_live(p1) && g_live == 2);  // the buffer died, the retired did not
  }
  CHECK(!is_live(p0) && !is_live(p1) && g_live == 0 && g_frees == 2);
}

// 5. a handle built by an && chain, as the library's create functions build theirs
struct Handle {
  DevBuf<uint8_t> d_rows;
  DevBuf<float> d_state[2];
  DevBuf<int> d_err;
  PinBuf<int> h_err;
  PinBuf<uint8_t> h_row[2];
  DevBuf<double> d_part;
  PinBuf<double> h_sums;
  DevBuf<void> d_slab;
};
static bool build(Handle* h) {
  bool ok = h->d_rows.alloc_zero(1000) == hipSuccess;
  for (int i = 0; i < 2 && ok; ++i)
    ok = h->d_state[i].alloc_zero(30, 64) == hipSuccess && h->h_row[i].alloc(544) == hipSuccess;
  return ok && h->d_err.alloc_zero(16) == hipSuccess && h->h_err.alloc(16) == hipSuccess &&
         h->d_part.alloc(256) == hipSuccess && h->h_sums.alloc(8) == hipSuccess && h->d_slab.alloc_zero(4096) == hipSuccess;
}
static void case_failure_sweep() {
  fake_reset();
  int total;
  {
    Handle h;
    CHECK(build(&h) && g_live == 10);
    total = g_calls;  // 10 allocations and 5 fills
  }
  CHECK(total == 15 && g_live == 0 && g_frees == 10);
  for (int k = 0; k <= total; ++k) {
    fake_reset(k);
    {
      Handle* h = new Handle();
      const bool ok = build(h);
      CHECK(ok == (k == total));
      CHECK(g_calls == (ok ? total : k + 1));  // the chain stops at the call that failed
      delete h;  // a create function's failure path
    }
    CHECK(g_live == 0);
  }
}

// 6. a failing fill reports the error and leaks nothing
static void case_zero_fill_failure() {
  fake_reset(1);  // call 0 allocates, call 1 is the fill
  {
    DevBuf<int> d;
    CHECK(d.alloc_zero(16) == hipErrorInvalidValue && g_memsets == 1 && g_live == 1);  // still owned
  }
  CHECK(g_live == 0 && g_frees == 1);
  fake_reset();
  {
    DevBuf<uint8_t> d;
    CHECK(d.alloc_zero(10, 6) == hipSuccess && g_memsets == 1);
    bool zero = true;
    for (int i = 0; i < 16; ++i) zero = zero && d[i] == 0;  // the pad is filled as well
    CHECK(zero);
  }
  CHECK(g_live == 0);
}

int main() {
  case_scope_exit();
  case_moves();
  case_grow();
  case_retire();
  case_failure_sweep();
  case_zero_fill_failure();
  fake_reset();
  if (g_failed) {
    std::printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

// fleet_amd/csrc/fleet_codec.cpp -- host side of the C-ABI (include/fleet_codec.h).
//
// Owns device memory, a HIP stream and pinned staging per context; stages
// host Base64 buffers to HBM, launches the gfx950 kernels (kernels.hip) and
// returns bytes identical to the reference's JNI natives. No CPU compute
// path exists: without a GPU every compute entry point returns FLEET_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sched.h>

#include "../../include/fleet_codec.h"
#include "cifar_forward.h"
#include "kernels.h"
#include "solver_host.h"
#include "solver_math.h"

static_assert(FLEET_MAX_HEADERS == fleet::kMaxHeaderSlots, "the kernels size their LDS header lists by it");
#include "model_codec.h"
#include "codec_device.h"
#include "mledger_table.h"
#include "dev_mem.h"

#define FLEET_VERSION "fleet-mi355x 0.1.0 (gfx950)"

// Persistent host threads for the staging copies of large host-buffer updates
// (one pool per context, created on first use): a thread per part and call
// cost 50-100 us to start on the GPU boxes, more than a part's copy.
class WorkerPool {
 public:
  explicit WorkerPool(int workers) {
    for (int i = 0; i < workers; ++i) ts_.emplace_back([this] { loop(); });
  }
  ~WorkerPool() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : ts_) t.join();
  }
  int workers() const { return (int)ts_.size(); }
  // f(i) for every i in [0, n), on the pool's threads and the caller's
  void run(int n, const std::function<void(int)>& f) {
    {
      std::lock_guard<std::mutex> g(m_);
      f_ = &f;
      n_ = n;
      next_.store(0, std::memory_order_relaxed);
      pending_ = (int)ts_.size();
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [this] { return pending_ == 0; });
    f_ = nullptr;
  }

 private:
  void work() {
    for (int i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < n_;) (*f_)(i);
  }
  void loop() {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> g(m_);
    for (;;) {
      cv_.wait(g, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      g.unlock();
      work();
      g.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> ts_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(int)>* f_ = nullptr;
  int n_ = 0;
  std::atomic<int> next_{0};
  int pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

struct FLEET_MEM_LOCAL fleet_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::string err;
  // device buffers, grown on demand by doubling; the old allocation is freed
  fleet::DevBuf<uint8_t> d_a, d_b, d_out;
  fleet::DevBuf<float> d_f32;
  fleet::DevBuf<double> d_dampen;
  fleet::DevBuf<int32_t> d_hdr;  // {status, count, walk_end, 0, positions[FLEET_MAX_HEADERS]}
  fleet::DevBuf<int> d_err;
  // Device-resident entry points (fleet_*_device) run on the CALLER's stream and
  // may be captured into HIP graphs, so they own parameter buffers of their own:
  // nothing the host-buffer entry points do on the context's stream touches
  // them, and a buffer a captured graph may reference is never freed before
  // fleet_destroy (a grown dampen buffer is retired, not freed).
  fleet::DevBuf<double> d_dev_dampen;  // retired on growth
  fleet::DevBuf<int32_t> d_dev_hdr;
  fleet::DevBuf<int> d_dev_err;       // read by fleet_check
  fleet::Retired retired;             // freed in fleet_destroy
  std::vector<double> dev_dampen;     // what d_dev_dampen holds
  std::vector<int32_t> dev_hdr;       // what d_dev_hdr holds
  bool dev_params_valid = false;
  fleet::DevBuf<double> d_partials;
  // pinned host staging
  fleet::PinBuf<uint8_t> h_stage;  // grown by doubling
  fleet::PinBuf<int32_t> h_hdr;
  fleet::PinBuf<int> h_err;
  std::unique_ptr<WorkerPool> pool;  // staging copy threads (stage_uploads)
  int last_ingress = FLEET_INGRESS_NONE;  // how the last host-buffer update reached HBM
  // the pipelined Kardam form's tile flags (zeroed at allocation) and its launch epoch.
  // FREED on growth although a device-resident entry point uses it on the caller's stream
  // (its siblings below are retired): the call that grows it is synchronous
  fleet::DevBuf<uint32_t> d_kflags;
  uint32_t kflag_epoch = 0;
  uint32_t kflag_test_skew = 0;       // fleet_test_kardam_skew: reduce blocks wait for a later epoch
  // fleet_evaluate_device, fleet_cifar_test_device: the costs and predictions a caller does not take, [B floats | B int32]
  // in 8 bytes per image (retired on growth, not freed: an evaluation on another stream may
  // still write it)
  fleet::DevBuf<uint8_t> d_eval;
  // fleet_client_grads_device: the per-sample gradient rows of one chunk of clients (retired on
  // growth, for the same reason)
  fleet::DevBuf<uint8_t> d_client_ws;
  // the DP forms: clip[C] then sigma[C] of the call (retired on growth), and the 22961
  // standard-normal draws, made on the host on the first DP call and resident from then on
  fleet::DevBuf<float> d_client_dp;
  fleet::DevBuf<double> d_dp_z;
};

namespace {

constexpr size_t kHdrWords = FLEET_MAX_HEADERS + 4;  // {status, count, walk_end, 0, positions}

int fail(fleet_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail((ctx), FLEET_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Every entry point runs on its context's device and leaves the calling
// thread's current device as it found it (a JVM request thread or a torch
// process keeps its own notion of the current GPU): hipGetDevice on entry,
// hipSetDevice back on every return path.
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) {
      (void)hipGetLastError();
      prev = -1;
    }
    ok = prev == device || hipSetDevice(device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (ok && prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_SCOPE(ctx)                                                                       \
  DeviceGuard device_guard_((ctx)->device);                                                     \
  if (!device_guard_.ok) return fail((ctx), FLEET_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device)

// an allocation failure as every grow reports it: the call's name, the bytes asked for, HIP's reason
int nomem(fleet_ctx* c, const char* call, size_t bytes, hipError_t e) {
  return fail(c, FLEET_ERR_NOMEM, "%s(%zu): %s", call, bytes, hipGetErrorString(e));
}

template <typename T>
int grow_dev(fleet_ctx* c, fleet::DevBuf<T>& b, size_t need_elems) {
  const size_t n = std::max(need_elems, b.cap() * 2);
  const hipError_t e = b.grow_doubling(need_elems);
  return e == hipSuccess ? FLEET_OK : nomem(c, "hipMalloc", n * sizeof(T), e);
}

int grow_pinned(fleet_ctx* c, size_t need) {
  const size_t n = std::max(need, c->h_stage.cap() * 2);
  const hipError_t e = c->h_stage.grow_doubling(need);
  return e == hipSuccess ? FLEET_OK : nomem(c, "hipHostMalloc", n, e);
}

inline size_t round16(size_t x) { return (x + 15) / 16 * 16; }
inline size_t groups_of(size_t n_values) { return (n_values + 2) / 3; }

// Device-resident entry points run on the caller's stream; NULL is the null
// (default) stream, as in the HIP libraries. Host-buffer entry points use the
// context's own stream.
hipStream_t pick(fleet_ctx*, void* s) { return (hipStream_t)s; }

// Copy host text (len chars) into device buffer padded to 16-byte groups.
int stage_text(fleet_ctx* c, const char* text, size_t len, fleet::DevBuf<uint8_t>& dbuf) {
  size_t padded = round16(len) + 16;
  int rc = grow_dev(c, dbuf, padded);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(dbuf + (len & ~(size_t)15), 0, padded - (len & ~(size_t)15), c->stream));
  if (len) HIP_TRY(c, hipMemcpyAsync(dbuf, text, len, hipMemcpyHostToDevice, c->stream));
  return FLEET_OK;
}

int check_text_len(fleet_ctx* c, size_t len) {
  if (len % 4 != 0) return fail(c, FLEET_ERR_BASE64, "Base64 length %zu is not a multiple of 4", len);
  return FLEET_OK;
}

int read_err(fleet_ctx* c, hipStream_t s, int* d_errbuf = nullptr) {
  if (!d_errbuf) d_errbuf = c->d_err;
  HIP_TRY(c, hipMemcpyAsync(c->h_err, d_errbuf, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  int e = *c->h_err;
  if (e) {
    HIP_TRY(c, hipMemsetAsync(d_errbuf, 0, sizeof(int), s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  if (e & 1) return fail(c, FLEET_ERR_BASE64, "input is not Base64::encode output (alphabet/padding)");
  if (e & 2) return fail(c, FLEET_ERR_LAYOUT, "uploads disagree on the gradient layout header slots");
  if (e & 4) return fail(c, FLEET_ERR_ARG, "sample index outside the dataset");
  if (e & 8) return fail(c, FLEET_ERR_HIP, "a cross-block hand-off timed out (Kardam reduce blocks)");
  if (e & FLEET_ERRBIT_NAN)
    return fail(c, FLEET_ERR_ARG, "network blew up: a client sample's E is NaN (train_class's bail)");
  return FLEET_OK;
}

// Parse the layout of the upload at d_text (device) into c->d_hdr / c->h_hdr.
int parse_layout(fleet_ctx* c, const uint8_t* d_text, size_t n_up, int* n_hdr, size_t* walk_end = nullptr) {
  HIP_TRY(c, fleet::launch_layout_parse(d_text, (int64_t)n_up, FLEET_MAX_HEADERS, c->d_hdr, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_hdr, c->d_hdr, kHdrWords * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->h_hdr[0] != 0)
    return fail(c, FLEET_ERR_LAYOUT, "upload header does not describe a gradient layout (network.h:1038-1056)");
  *n_hdr = c->h_hdr[1];
  if (walk_end) *walk_end = (size_t)c->h_hdr[2];
  return FLEET_OK;
}

int finish_text(fleet_ctx* c, size_t out_len, char* out, size_t cap, size_t* out_len_p) {
  if (out_len_p) *out_len_p = out_len;
  if (cap < out_len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, out_len);
  if (out_len) HIP_TRY(c, hipMemcpyAsync(out, c->d_out, out_len, hipMemcpyDeviceToHost, c->stream));
  int rc = read_err(c, c->stream);
  return rc;
}

// Host staging copy threads: the plan's stage_threads (fleet_set_plan), else one per
// ~2 MiB of staging, at most 8 and at most the CPUs this process may run on.
int stage_threads(size_t bytes) {
  if (const int t = fleet::plan_overrides().stage_threads) return t;
  int n = 1;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  return (int)std::max<size_t>(1, std::min<size_t>({bytes >> 21, 8, (size_t)std::max(1, n)}));
}

// f(i) for i in [0, n) on `threads` threads (the caller's and the context's pool).
void parallel_for(fleet_ctx* c, int n, int threads, const std::function<void(int)>& f) {
  threads = std::max(1, std::min(threads, n));
  if (threads == 1) {
    for (int i = 0; i < n; ++i) f(i);
    return;
  }
  if (!c->pool || c->pool->workers() != threads - 1) {
    c->pool.reset();
    c->pool.reset(new WorkerPool(threads - 1));
  }
  c->pool->run(n, f);
}

// Copies bytes [col0, col0 + width) of each of the M uploads into the pinned
// staging rows (pitch apart, zero padded) and queues ONE H2D of [rows |
// tail_bytes already written after the rows] into d_a, in parts, each queued as
// soon as its rows are copied, so the DMA of a part overlaps the copy of the
// next (ingress framing). col0 = 0, width = len stages whole
// uploads; a column window is one GPU's element shard (fleet_update_multi).
// Measured on MI355X (probe_e2e2.py (r04 tree), rocprofv3 memory-copy trace): 1 MiB
// H2D parts run at ~35 GB/s with ~9 us gaps, one 7.8 MB copy at ~53 GB/s; three
// parts gave the shortest host-buffer update for MNIST-64 (0.27 vs 0.32 ms with
// one part). Each part is copied by `threads` workers (the context's pool): one
// thread's memcpy into pinned memory, not PCIe, bounded the host-buffer update
// of large batches (synth1m_256: 56.7 -> 27.9 ms; H2D floor 25.1 ms), and 16
// parts beat 3 there (cifar10_256, 8 threads: 9.37 -> 8.68 ms; floor 7.56 ms;
// gpu_e2e_sweep.sh (r04 tree)). MNIST-64: 4 threads 0.26 ms vs 1 thread 0.39 ms.
int stage_uploads(fleet_ctx* c, const char* const* uploads, size_t col0, size_t width, size_t pitch, int M,
                  size_t tail_bytes, int threads) {
  const size_t total = pitch * (size_t)M;
  int pieces = 3;
  if (total >= (256u << 20)) pieces = (int)std::min<size_t>(16, total / (24u << 20));
  if (const int k = fleet::plan_overrides().stage_pieces) pieces = k;
  if (total < (4u << 20)) pieces = 1;
  pieces = std::min(pieces, M);
  for (int k = 0; k < pieces; ++k) {
    const int r0 = (int)((int64_t)M * k / pieces), r1 = (int)((int64_t)M * (k + 1) / pieces);
    parallel_for(c, r1 - r0, threads, [&](int j) {
      const int i = r0 + j;
      uint8_t* row = c->h_stage + (size_t)i * pitch;
      std::memcpy(row, uploads[i] + col0, width);
      std::memset(row + width, 0, pitch - width);
    });
    const size_t off = (size_t)r0 * pitch;
    const size_t bytes = (size_t)(r1 - r0) * pitch + (r1 == M ? tail_bytes : 0);
    HIP_TRY(c, hipMemcpyAsync(c->d_a + off, c->h_stage + off, bytes, hipMemcpyHostToDevice, c->stream));
  }
  return FLEET_OK;
}

// network::flatGrad's header walk (network.h:1206-1223) over the last upload,
// on the host from the caller's buffer -- the same walk as k_layout_parse:
// words = {status (0 ok, 1 malformed), count, walk end, 0, positions...}.
// The caller's buffer is exactly `len` bytes (a JVM array or Python bytes, no
// padding): the group holding value p is copied into a zero-padded local, so a
// short or truncated upload never reads past the end (bytes at or beyond len
// decode as the device path's zero padding).
int32_t host_code_at(const char* text, size_t len, int64_t p, bool* bad) {
  static constexpr auto tab = [] {
    struct T {
      uint8_t v[256];
    } t{};
    for (int i = 0; i < 256; ++i) t.v[i] = fleet::b64_from_value(i);
    return t;
  }();
  uint8_t g[16] = {0};
  const size_t g0 = 16 * (size_t)(p / 3);
  if (g0 < len) std::memcpy(g, text + g0, std::min<size_t>(16, len - g0));
  const int e = (int)(p % 3);
  const uint32_t carry[3] = {0x003fu, 0x07e0u, 0xfc00u};  // chars carrying bytes 4e..4e+3
  uint8_t bytes[12];
  for (int q = 0; q < 4; ++q) {
    uint32_t w = 0;
    for (int i = 0; i < 4; ++i) {
      const uint8_t v = tab.v[g[4 * q + i]];
      if (v == 0xff && ((carry[e] >> (4 * q + i)) & 1u)) *bad = true;
      w = (w << 6) | (v & 63u);
    }
    bytes[3 * q] = (uint8_t)(w >> 16);
    bytes[3 * q + 1] = (uint8_t)(w >> 8);
    bytes[3 * q + 2] = (uint8_t)w;
  }
  uint32_t u = 0;
  for (int i = 3; i >= 0; --i) u = (u << 8) | bytes[4 * e + i];
  return (int32_t)u;
}
void host_layout_parse(const char* up, size_t len, int64_t n, int cap, int32_t* out) {
  int64_t idx = 0;
  int nh = 0;
  bool bad = false;
  int status = 0;
  for (int part = 0; part < 2 && !status; ++part) {
    if (idx >= n || nh >= cap) {
      status = 1;
      break;
    }
    out[4 + nh++] = (int32_t)idx;
    const int cnt = fleet::cvtt(fleet::dec(host_code_at(up, len, idx++, &bad)));
    for (int i = 0; i < cnt; ++i) {
      if (idx >= n || nh >= cap) {
        status = 1;
        break;
      }
      out[4 + nh++] = (int32_t)idx;
      const int size = fleet::cvtt(fleet::dec(host_code_at(up, len, idx++, &bad)));
      if (size < 0 || idx + size > n) {
        status = 1;
        break;
      }
      idx += size;
    }
  }
  if (bad) status = 1;
  out[0] = status;
  out[1] = nh;
  out[2] = (int32_t)idx;
  out[3] = 0;
}

// fleet_update when the host walk of the last upload's header fails: the
// device flow (parse kernel, update, error flags), so the error reported is
// the same as a full device run's (Base64 errors anywhere take precedence).
int update_host_fallback(fleet_ctx* c, const char* const* uploads, size_t len, int M, const double* dampen,
                         char* merged, float* merged_f32) {
  const size_t n = fleet_b64_count(len), groups = groups_of(n), pitch = round16(len), total = pitch * (size_t)M;
  int rc;
  if ((rc = grow_dev(c, c->d_dampen, (size_t)M))) return rc;
  if ((rc = grow_dev(c, c->d_out, 16 * groups + 16))) return rc;
  if (merged_f32 && (rc = grow_dev(c, c->d_f32, 3 * groups + 3))) return rc;
  if ((rc = stage_uploads(c, uploads, 0, len, pitch, M, 0, stage_threads(total)))) return rc;
  std::memcpy(c->h_stage + total, dampen, sizeof(double) * (size_t)M);
  HIP_TRY(c, hipMemcpyAsync(c->d_dampen, c->h_stage + total, sizeof(double) * (size_t)M, hipMemcpyHostToDevice,
                            c->stream));
  HIP_TRY(c, fleet::launch_layout_parse(c->d_a + (size_t)(M - 1) * pitch, (int64_t)n, FLEET_MAX_HEADERS, c->d_hdr,
                                        c->stream));
  HIP_TRY(c, fleet::launch_update(c->d_a, pitch, M, c->d_dampen, (double)1 / M, (int64_t)n, 0, (int64_t)groups,
                                  c->d_hdr, c->d_out, merged_f32 ? c->d_f32 : nullptr, c->d_err, c->stream));
  HIP_TRY(c, hipMemcpyAsync(merged, c->d_out, len, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_hdr, c->d_hdr, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  if (c->h_hdr[0] != 0)
    return fail(c, FLEET_ERR_LAYOUT, "last upload's header does not describe a gradient layout");
  return FLEET_OK;  // not reached for a failed host walk (the device walk is the same)
}

}  // namespace

extern "C" {

const char* fleet_version(void) { return FLEET_VERSION; }

size_t fleet_b64_len(size_t n_values) { return 4 * ((4 * n_values + 2) / 3); }
size_t fleet_b64_count(size_t len) { return 3 * len / 16; }

int fleet_create(int device, fleet_ctx** out) {
  if (!out) return FLEET_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return FLEET_ERR_HIP;
  if (device < 0 || device >= n) return FLEET_ERR_ARG;
  fleet_ctx* c = new fleet_ctx();
  c->device = device;
  int rc = FLEET_OK;
  auto bail = [&](int code) {
    fleet_destroy(c);
    return code;
  };
  DeviceGuard dg(device);
  if (!dg.ok) return bail(FLEET_ERR_HIP);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(FLEET_ERR_HIP);
  constexpr size_t kErrWords = 64 / sizeof(int);  // an error word in 64 bytes of its own
  if (c->d_hdr.alloc(kHdrWords) != hipSuccess) return bail(FLEET_ERR_NOMEM);
  if (c->d_err.alloc(kErrWords) != hipSuccess) return bail(FLEET_ERR_NOMEM);
  if (hipMemset(c->d_err, 0, 64) != hipSuccess) return bail(FLEET_ERR_HIP);
  if (c->d_dev_hdr.alloc(kHdrWords) != hipSuccess) return bail(FLEET_ERR_NOMEM);
  if (c->d_dev_err.alloc(kErrWords) != hipSuccess) return bail(FLEET_ERR_NOMEM);
  if (hipMemset(c->d_dev_err, 0, 64) != hipSuccess) return bail(FLEET_ERR_HIP);
  if (c->h_hdr.alloc(kHdrWords) != hipSuccess) return bail(FLEET_ERR_NOMEM);
  if (c->h_err.alloc(kErrWords) != hipSuccess) return bail(FLEET_ERR_NOMEM);
  (void)rc;
  *out = c;
  return FLEET_OK;
}

void fleet_destroy(fleet_ctx* c) {
  if (!c) return;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  hipStream_t s = c->stream;
  delete c;  // the buffers and the retired allocations go with it
  if (s) (void)hipStreamDestroy(s);
}

const char* fleet_last_error(const fleet_ctx* c) { return c ? c->err.c_str() : "no context"; }

namespace {
std::atomic<int> g_last_ingress{FLEET_INGRESS_NONE};  // the process's most recent one
}

#ifdef FLEET_TRACE
// dev builds only (-DFLEET_TRACE): where the tile kernels write their phase trace
extern "C" __attribute__((visibility("default"))) int fleet_dev_trace(void* d_buf) {
  return fleet::set_trace_buffer(d_buf) == hipSuccess ? FLEET_OK : FLEET_ERR_HIP;
}
#endif

int fleet_last_ingress(fleet_ctx* c) {
  if (!c) return g_last_ingress.load();
  std::lock_guard<std::mutex> lk(c->mu);
  return c->last_ingress;
}

int fleet_sync(fleet_ctx* c, void* stream) {
  if (!c) return FLEET_ERR_ARG;
  HIP_TRY(c, hipStreamSynchronize(pick(c, stream)));
  return FLEET_OK;
}

int fleet_ctx_device(const fleet_ctx* c) { return c ? c->device : -1; }

int fleet_check(fleet_ctx* c, void* stream) {
  if (!c) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  return read_err(c, pick(c, stream), c->d_dev_err);
}

int fleet_layout_from_sizes(const int32_t* w_sizes, int n_w, const int32_t* b_sizes, int n_b, int32_t* header_pos,
                            int cap, int* n_headers, size_t* n_up) {
  if (n_w < 0 || n_b < 0 || (n_w && !w_sizes) || (n_b && !b_sizes)) return FLEET_ERR_ARG;
  size_t idx = 0;
  int nh = 0;
  auto put = [&](size_t p) {
    if (nh < cap && header_pos) header_pos[nh] = (int32_t)p;
    ++nh;
  };
  put(idx++);
  for (int i = 0; i < n_w; ++i) {
    if (w_sizes[i] < 0) return FLEET_ERR_ARG;
    put(idx++);
    idx += (size_t)w_sizes[i];
  }
  put(idx++);
  for (int i = 0; i < n_b; ++i) {
    if (b_sizes[i] < 0) return FLEET_ERR_ARG;
    put(idx++);
    idx += (size_t)b_sizes[i];
  }
  if (n_headers) *n_headers = nh;
  if (n_up) *n_up = idx;
  return nh <= cap ? FLEET_OK : FLEET_ERR_CAPACITY;
}

int fleet_layout_parse(fleet_ctx* c, const char* upload, size_t len, int32_t* header_pos, int cap, int* n_headers,
                       size_t* n_up) {
  if (!c || (!upload && len)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_text_len(c, len);
  if (rc) return rc;
  size_t n = fleet_b64_count(len);
  if ((rc = stage_text(c, upload, len, c->d_a))) return rc;
  int nh = 0;
  size_t walk_end = n;
  if ((rc = parse_layout(c, c->d_a, n, &nh, &walk_end))) return rc;
  if (n_headers) *n_headers = nh;
  if (n_up) *n_up = walk_end;
  if (header_pos) std::memcpy(header_pos, c->h_hdr + 4, sizeof(int32_t) * std::min(nh, cap));
  return nh <= cap ? FLEET_OK : FLEET_ERR_CAPACITY;
}

// ----------------------------------------------------------------- codec

int fleet_encode_f32(fleet_ctx* c, const float* values, size_t n, char* out, size_t cap, size_t* out_len) {
  if (!c || (!values && n)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc;
  if ((rc = grow_dev(c, c->d_f32, n + 3))) return rc;
  if ((rc = grow_dev(c, c->d_out, 16 * groups_of(n) + 16))) return rc;
  if (n) HIP_TRY(c, hipMemcpyAsync(c->d_f32, values, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fleet::launch_encode_f32(c->d_f32, (int64_t)n, 0, 1, c->d_out, 0, c->stream));
  return finish_text(c, fleet_b64_len(n), out, cap, out_len);
}

int fleet_encode_i32(fleet_ctx* c, const int32_t* codes, size_t n, char* out, size_t cap, size_t* out_len) {
  if (!c || (!codes && n)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc;
  if ((rc = grow_dev(c, c->d_a, 4 * n + 16))) return rc;
  if ((rc = grow_dev(c, c->d_out, 16 * groups_of(n) + 16))) return rc;
  if (n) HIP_TRY(c, hipMemcpyAsync(c->d_a, codes, n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fleet::launch_encode_i32((const int32_t*)c->d_a.get(), (int64_t)n, c->d_out, c->stream));
  return finish_text(c, fleet_b64_len(n), out, cap, out_len);
}

static int decode_common(fleet_ctx* c, const char* text, size_t len, void* out, size_t cap, size_t* n_out,
                         int as_codes) {
  if (!c || (!text && len)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_text_len(c, len);
  if (rc) return rc;
  size_t n = fleet_b64_count(len);
  if (n_out) *n_out = n;
  if (cap < n) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu values", cap, n);
  if ((rc = stage_text(c, text, len, c->d_a))) return rc;
  if ((rc = grow_dev(c, c->d_f32, n + 3))) return rc;
  HIP_TRY(c, fleet::launch_decode(c->d_a, (int64_t)n, 0, 1, c->d_f32, 0, as_codes, c->d_err, c->stream));
  if (n) HIP_TRY(c, hipMemcpyAsync(out, c->d_f32, n * 4, hipMemcpyDeviceToHost, c->stream));
  return read_err(c, c->stream);
}

int fleet_decode_f32(fleet_ctx* c, const char* text, size_t len, float* out, size_t cap, size_t* n_out) {
  return decode_common(c, text, len, out, cap, n_out, 0);
}
int fleet_decode_i32(fleet_ctx* c, const char* text, size_t len, int32_t* out, size_t cap, size_t* n_out) {
  return decode_common(c, text, len, out, cap, n_out, 1);
}

// ------------------------------------------------------------- JNI ops

int fleet_flat_gradient(fleet_ctx* c, const char* g, size_t len, char* out, size_t cap, size_t* out_len) {
  if (!c || (!g && len)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_text_len(c, len);
  if (rc) return rc;
  size_t n = fleet_b64_count(len);
  if ((rc = stage_text(c, g, len, c->d_a))) return rc;
  int nh = 0;
  size_t walk_end = 0;
  if ((rc = parse_layout(c, c->d_a, n, &nh, &walk_end))) return rc;
  // network::flatGrad stops after the last bias block: values past the walk are dropped
  const size_t n_flat = walk_end - (size_t)nh;
  if ((rc = grow_dev(c, c->d_out, 16 * groups_of(n_flat) + 16))) return rc;
  HIP_TRY(c, fleet::launch_flat(c->d_a, c->d_hdr + 4, nh, (int64_t)n_flat, c->d_out, c->d_err, c->stream));
  return finish_text(c, fleet_b64_len(n_flat), out, cap, out_len);
}

int fleet_merge_flat_gradient(fleet_ctx* c, const char* g, size_t glen, const char* flat, size_t flen, char* out,
                              size_t cap, size_t* out_len) {
  if (!c || (!g && glen) || (!flat && flen)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_text_len(c, glen);
  if (rc || (rc = check_text_len(c, flen))) return rc;
  size_t n = fleet_b64_count(glen), nf = fleet_b64_count(flen);
  if ((rc = stage_text(c, g, glen, c->d_a))) return rc;
  if ((rc = stage_text(c, flat, flen, c->d_b))) return rc;
  int nh = 0;
  size_t walk_end = 0;
  if ((rc = parse_layout(c, c->d_a, n, &nh, &walk_end))) return rc;
  if (nf < walk_end - (size_t)nh)
    return fail(c, FLEET_ERR_ARG, "flat gradient has %zu values, layout needs %zu", nf, walk_end - (size_t)nh);
  if ((rc = grow_dev(c, c->d_out, 16 * groups_of(n) + 16))) return rc;
  HIP_TRY(c, fleet::launch_merge(c->d_a, c->d_b, c->d_hdr + 4, nh, (int64_t)walk_end, (int64_t)n, c->d_out,
                                 c->d_err, c->stream));
  return finish_text(c, glen, out, cap, out_len);
}

static int elementwise(fleet_ctx* c, const char* a, size_t alen, const char* b, size_t blen, int op, double s,
                       char* out, size_t cap, size_t* out_len) {
  if (!c || (!a && alen) || (op && !b && blen)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_text_len(c, alen);
  if (rc) return rc;
  size_t n = fleet_b64_count(alen);
  if ((rc = stage_text(c, a, alen, c->d_a))) return rc;
  if (op) {
    if ((rc = check_text_len(c, blen))) return rc;
    if (fleet_b64_count(blen) < n) return fail(c, FLEET_ERR_ARG, "second operand shorter than the first");
    if ((rc = stage_text(c, b, blen, c->d_b))) return rc;
  }
  if ((rc = grow_dev(c, c->d_out, 16 * groups_of(n) + 16))) return rc;
  HIP_TRY(c, fleet::launch_elementwise(c->d_a, op ? c->d_b : c->d_a, op, s, (int64_t)n, c->d_out, c->d_err,
                                       c->stream));
  return finish_text(c, fleet_b64_len(n), out, cap, out_len);
}

int fleet_scalar_mul(fleet_ctx* c, const char* v, size_t len, double a, char* out, size_t cap, size_t* out_len) {
  return elementwise(c, v, len, nullptr, 0, 0, a, out, cap, out_len);
}
int fleet_add(fleet_ctx* c, const char* a, size_t alen, const char* b, size_t blen, char* out, size_t cap,
              size_t* out_len) {
  return elementwise(c, a, alen, b, blen, 1, 0.0, out, cap, out_len);
}
int fleet_subtract(fleet_ctx* c, const char* a, size_t alen, const char* b, size_t blen, char* out, size_t cap,
                   size_t* out_len) {
  return elementwise(c, a, alen, b, blen, 2, 0.0, out, cap, out_len);
}

int fleet_norm(fleet_ctx* c, const char* v, size_t len, double* out) {
  if (!c || (!v && len) || !out) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_text_len(c, len);
  if (rc) return rc;
  size_t n = fleet_b64_count(len);
  if ((rc = stage_text(c, v, len, c->d_a))) return rc;
  size_t blocks = (groups_of(n) + 255) / 256 + 1;
  if ((rc = grow_dev(c, c->d_partials, blocks))) return rc;
  int nb = 0;
  HIP_TRY(c, fleet::launch_norm_partials(c->d_a, (int64_t)n, c->d_partials, &nb, c->d_err, c->stream));
  std::vector<double> part((size_t)nb);
  if (nb) HIP_TRY(c, hipMemcpyAsync(part.data(), c->d_partials, nb * sizeof(double), hipMemcpyDeviceToHost,
                                    c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  double s = 0;
  for (double p : part) s += p;  // block partials in index order
  *out = __builtin_sqrt(s);
  return FLEET_OK;
}

// ------------------------------------------------------------ fused update

namespace {

// Validation shared by the host-buffer updates; on success *len = the common length.
int check_update_args(fleet_ctx* c, const char* const* uploads, const size_t* lens, int M, size_t cap,
                      size_t* out_len, size_t* len_out) {
  const size_t len = lens[0];
  int rc = check_text_len(c, len);
  if (rc) return rc;
  for (int i = 0; i < M; ++i) {
    if (!uploads[i] || lens[i] != len)
      return fail(c, FLEET_ERR_ARG, "upload %d has length %zu, expected %zu (one model layout)", i, lens[i], len);
  }
  if (out_len) *out_len = len;
  if (cap < len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, len);
  *len_out = len;
  return FLEET_OK;
}

// The host-buffer update of the groups [gb, ge) on context c (lock held, device
// set): the column window [16*gb, 16*ge) of every upload is staged into pinned
// memory and sent to HBM, the exact chain runs on it, and its merged slice
// (Base64 bytes [16*gb, min(len, 16*ge)), fp32 values [3*gb, min(n, 3*ge))) is
// written into the caller's outputs -- disjoint ranges for disjoint windows.
// hw = the host walk of the last upload's header (whole-upload coordinates).
//   staging block, mirrored on the device in d_a:
//   [window rows M x wpitch | dampen M doubles | header words | err | merged | fp32]
//   one H2D up to err (inclusive, err = 0), one D2H from err on.
// pinned_rows != NULL: the uploads are rows `row_pitch` apart in page-locked
// memory (fleet_host_register, or allocated pinned): the window goes to HBM in
// one 2D DMA straight from them, with no host copy (only the parameter words
// are staged). Bytes past `len` in the last group of a row may hold anything:
// the kernels ignore the chars that carry no value.
int update_window(fleet_ctx* c, const char* const* uploads, size_t len, int M, const double* dampen,
                  const int32_t* hw, size_t gb, size_t ge, char* merged, float* merged_f32, int threads,
                  const char* pinned_rows = nullptr, size_t row_pitch = 0) {
  const size_t n = fleet_b64_count(len);
  const size_t w = ge - gb;
  if (w == 0) return FLEET_OK;
  const size_t wpitch = 16 * w;
  const size_t col0 = 16 * gb, width = std::min(len, 16 * ge) - col0;
  const size_t total = wpitch * (size_t)M;
  const size_t o_damp = total, o_hdr = round16(o_damp + sizeof(double) * (size_t)M);
  const size_t o_err = round16(o_hdr + sizeof(int32_t) * kHdrWords), o_out = o_err + 16;
  const size_t o_f32 = round16(o_out + wpitch + 16), o_end = o_f32 + sizeof(float) * (3 * w + 3);
  int rc;
  if ((rc = grow_pinned(c, o_end + 64))) return rc;
  if ((rc = grow_dev(c, c->d_a, o_end + 64))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // staging buffer reuse
  std::memcpy(c->h_stage + o_hdr, hw, sizeof(int32_t) * kHdrWords);
  std::memcpy(c->h_stage + o_damp, dampen, sizeof(double) * (size_t)M);
  std::memset(c->h_stage + o_err, 0, 16);
  c->last_ingress = pinned_rows ? FLEET_INGRESS_PINNED : FLEET_INGRESS_STAGED;
  g_last_ingress.store(c->last_ingress);
  if (pinned_rows) {
    HIP_TRY(c, hipMemcpy2DAsync(c->d_a, wpitch, pinned_rows + col0, row_pitch, width, (size_t)M,
                                hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_a + total, c->h_stage + total, o_err + 16 - total, hipMemcpyHostToDevice,
                              c->stream));
  } else if ((rc = stage_uploads(c, uploads, col0, width, wpitch, M, o_err + 16 - total, threads))) {
    return rc;
  }
  uint8_t* d = c->d_a;
  // window mode: row and output pointers shifted back by the window's start
  HIP_TRY(c, fleet::launch_update(d - col0, wpitch, M, reinterpret_cast<const double*>(d + o_damp), (double)1 / M,
                                  (int64_t)n, (int64_t)gb, (int64_t)ge, reinterpret_cast<const int32_t*>(d + o_hdr),
                                  d + o_out - col0,
                                  merged_f32 ? reinterpret_cast<float*>(d + o_f32) - 3 * gb : nullptr,
                                  reinterpret_cast<int*>(d + o_err), c->stream));
  const size_t v0 = 3 * gb, v1 = std::min(n, 3 * ge);
  const size_t back = (merged_f32 ? o_f32 + sizeof(float) * (v1 - v0) : o_out + width) - o_err;
  HIP_TRY(c, hipMemcpyAsync(c->h_stage + o_err, d + o_err, back, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int e = *reinterpret_cast<const int*>(c->h_stage + o_err);
  if (e & 1) return fail(c, FLEET_ERR_BASE64, "input is not Base64::encode output (alphabet/padding)");
  if (e & 2) return fail(c, FLEET_ERR_LAYOUT, "uploads disagree on the gradient layout header slots");
  std::memcpy(merged + col0, c->h_stage + o_out, width);
  if (merged_f32) std::memcpy(merged_f32 + v0, c->h_stage + o_f32, sizeof(float) * (v1 - v0));
  return FLEET_OK;
}

}  // namespace

int fleet_update(fleet_ctx* c, const char* const* uploads, const size_t* lens, int M, const double* dampen,
                 char* merged, size_t cap, size_t* out_len, float* merged_f32) {
  if (!c || !uploads || !lens || !dampen || !merged || M <= 0) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t len = 0;
  int rc = check_update_args(c, uploads, lens, M, cap, out_len, &len);
  if (rc) return rc;
  const size_t n = fleet_b64_count(len);
  // layout of the last picked upload (mergeFlatGradient keeps its header), walked on the host
  std::vector<int32_t> hw(kHdrWords);
  host_layout_parse(uploads[M - 1], len, (int64_t)n, FLEET_MAX_HEADERS, hw.data());
  if (hw[0] != 0) return update_host_fallback(c, uploads, len, M, dampen, merged, merged_f32);
  return update_window(c, uploads, len, M, dampen, hw.data(), 0, groups_of(n), merged, merged_f32,
                       stage_threads(round16(len) * (size_t)M));
}

namespace {

// Ranges page-locked by fleet_host_register (process-wide: every context's
// device DMAs from them). The copy-free row path requires the WHOLE row range
// to lie inside ONE recorded registration. A record cannot tell whether its
// memory was freed and reused since (the caller's contract, fleet_codec.h:
// unregister before freeing); it only stops rows that straddle two ranges.
std::mutex g_reg_mu;
std::vector<std::pair<uintptr_t, size_t>> g_registered;  // (base, bytes)

bool in_one_registration(const void* p, size_t bytes) {
  const uintptr_t a = (uintptr_t)p;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (const auto& r : g_registered)
    if (a >= r.first && bytes <= r.second && a - r.first <= r.second - bytes) return true;
  return false;
}

int update_multi_impl(fleet_ctx* const* ctxs, int n_ctx, const char* const* uploads, const size_t* lens, int M,
                      const double* dampen, char* merged, size_t cap, size_t* out_len, float* merged_f32,
                      const char* pinned_rows, size_t row_pitch) {
  for (int k = 0; k < n_ctx; ++k) {
    if (!ctxs[k]) return FLEET_ERR_ARG;
    for (int j = 0; j < k; ++j)
      if (ctxs[j] == ctxs[k]) return fail(ctxs[0], FLEET_ERR_ARG, "context %d is passed twice", k);
  }
  fleet_ctx* c0 = ctxs[0];
  size_t len = 0;
  int rc;
  {
    std::lock_guard<std::mutex> lk(c0->mu);
    if ((rc = check_update_args(c0, uploads, lens, M, cap, out_len, &len))) return rc;
  }
  const size_t n = fleet_b64_count(len), groups = groups_of(n);
  std::vector<int32_t> hw(kHdrWords);
  host_layout_parse(uploads[M - 1], len, (int64_t)n, FLEET_MAX_HEADERS, hw.data());
  // a malformed header: the single-device flow reports the same error as a full device run
  if (hw[0] != 0) {
    std::lock_guard<std::mutex> lk(c0->mu);
    DEVICE_SCOPE(c0);
    return update_host_fallback(c0, uploads, len, M, dampen, merged, merged_f32);
  }
  const int threads = std::max(1, stage_threads(round16(len) * (size_t)M) / n_ctx);
  std::vector<int> rcs((size_t)n_ctx, FLEET_OK);
  auto run = [&](int k) {
    // balanced contiguous split of the groups (fleet_amd.shard.group_range)
    const size_t base = groups / (size_t)n_ctx, rem = groups % (size_t)n_ctx;
    const size_t gb = (size_t)k * base + std::min((size_t)k, rem), ge = gb + base + ((size_t)k < rem ? 1 : 0);
    fleet_ctx* c = ctxs[k];
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) {
      rcs[(size_t)k] = fail(c, FLEET_ERR_HIP, "hipSetDevice(%d) failed", c->device);
      return;
    }
    rcs[(size_t)k] = update_window(c, uploads, len, M, dampen, hw.data(), gb, ge, merged, merged_f32,
                                   n_ctx == 1 ? stage_threads(round16(len) * (size_t)M) : threads, pinned_rows,
                                   row_pitch);
  };
  if (n_ctx == 1) {
    run(0);
  } else {
    std::vector<std::thread> ts;
    ts.reserve((size_t)n_ctx);
    for (int k = 0; k < n_ctx; ++k) ts.emplace_back(run, k);
    for (auto& t : ts) t.join();
  }
  // the first failing shard's error (Base64 errors first, as one device reports them)
  int first = -1;
  for (int k = 0; k < n_ctx; ++k)
    if (rcs[(size_t)k] != FLEET_OK &&
        (first < 0 || (rcs[(size_t)k] == FLEET_ERR_BASE64 && rcs[(size_t)first] != FLEET_ERR_BASE64)))
      first = k;
  if (first < 0) return FLEET_OK;
  if (first != 0) {
    std::lock_guard<std::mutex> lk(c0->mu);
    c0->err = ctxs[first]->err;
  }
  return rcs[(size_t)first];
}

int update_rows_impl(fleet_ctx* const* ctxs, int n_ctx, const char* rows, size_t row_pitch, size_t len, int M,
                     const double* dampen, char* merged, size_t cap, size_t* out_len, float* merged_f32) {
  if (row_pitch < len) return fail(ctxs[0], FLEET_ERR_ARG, "row pitch %zu < upload length %zu", row_pitch, len);
  std::vector<const char*> ptrs((size_t)M);
  std::vector<size_t> lens((size_t)M, len);
  for (int i = 0; i < M; ++i) ptrs[(size_t)i] = rows + (size_t)i * row_pitch;
  const bool pinned = in_one_registration(rows, (size_t)(M - 1) * row_pitch + len);
  return update_multi_impl(ctxs, n_ctx, ptrs.data(), lens.data(), M, dampen, merged, cap, out_len, merged_f32,
                           pinned ? rows : nullptr, row_pitch);
}

}  // namespace

int fleet_update_multi(fleet_ctx* const* ctxs, int n_ctx, const char* const* uploads, const size_t* lens, int M,
                       const double* dampen, char* merged, size_t cap, size_t* out_len, float* merged_f32) {
  if (!ctxs || n_ctx <= 0 || !uploads || !lens || !dampen || !merged || M <= 0) return FLEET_ERR_ARG;
  if (n_ctx == 1) return fleet_update(ctxs[0], uploads, lens, M, dampen, merged, cap, out_len, merged_f32);
  return update_multi_impl(ctxs, n_ctx, uploads, lens, M, dampen, merged, cap, out_len, merged_f32, nullptr, 0);
}

int fleet_update_rows(fleet_ctx* c, const char* rows, size_t row_pitch, size_t len, int M, const double* dampen,
                      char* merged, size_t cap, size_t* out_len, float* merged_f32) {
  if (!c || !rows || !dampen || !merged || M <= 0) return FLEET_ERR_ARG;
  return update_rows_impl(&c, 1, rows, row_pitch, len, M, dampen, merged, cap, out_len, merged_f32);
}

int fleet_update_rows_multi(fleet_ctx* const* ctxs, int n_ctx, const char* rows, size_t row_pitch, size_t len, int M,
                            const double* dampen, char* merged, size_t cap, size_t* out_len, float* merged_f32) {
  if (!ctxs || n_ctx <= 0 || !ctxs[0] || !rows || !dampen || !merged || M <= 0) return FLEET_ERR_ARG;
  return update_rows_impl(ctxs, n_ctx, rows, row_pitch, len, M, dampen, merged, cap, out_len, merged_f32);
}

int fleet_host_register(fleet_ctx* c, void* ptr, size_t bytes) {
  if (!c || !ptr || !bytes) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const uintptr_t a = (uintptr_t)ptr;
  {
    // a live registration overlapping the new range belongs to memory that was
    // freed and reused (a collected direct buffer): it is released first
    std::lock_guard<std::mutex> rk(g_reg_mu);
    for (size_t i = g_registered.size(); i-- > 0;) {
      const auto r = g_registered[i];
      if (r.first < a + bytes && a < r.first + r.second) {
        (void)hipHostUnregister((void*)r.first);
        (void)hipGetLastError();
        g_registered.erase(g_registered.begin() + (long)i);
      }
    }
  }
  HIP_TRY(c, hipHostRegister(ptr, bytes, hipHostRegisterPortable));
  std::lock_guard<std::mutex> rk(g_reg_mu);
  g_registered.emplace_back(a, bytes);
  return FLEET_OK;
}

int fleet_host_unregister(fleet_ctx* c, void* ptr) {
  if (!c || !ptr) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  {
    std::lock_guard<std::mutex> rk(g_reg_mu);
    for (size_t i = g_registered.size(); i-- > 0;)
      if (g_registered[i].first == (uintptr_t)ptr) g_registered.erase(g_registered.begin() + (long)i);
  }
  HIP_TRY(c, hipHostUnregister(ptr));
  return FLEET_OK;
}

// ---------------------------------------------------------- device-resident

namespace {

using fleet::DevBuf;
using fleet::PinBuf;

// A caller's header list for an upload of n values: the kernels search it, so the
// positions are strictly ascending and inside [0, n).
int check_header_positions(fleet_ctx* c, const int32_t* header_pos, int n_headers, size_t n) {
  for (int i = 0; i < n_headers; ++i)
    if (header_pos[i] < 0 || (size_t)header_pos[i] >= n || (i && header_pos[i] <= header_pos[i - 1]))
      return fail(c, FLEET_ERR_ARG, "header position %d (%d) is not ascending inside the upload", i, header_pos[i]);
  return FLEET_OK;
}

// The device-resident update's parameters ({status, count, walk_end, 0, positions}
// and dampen): kept resident in the context's own buffers and re-uploaded (one
// sync) only when they change, so steady-state calls are pure kernel launches.
int dev_params(fleet_ctx* c, hipStream_t s, size_t n, int M, const double* dampen, const int32_t* header_pos,
               int n_headers) {
  std::vector<int32_t> hdr_words((size_t)n_headers + 4);
  hdr_words[0] = 0;
  hdr_words[1] = n_headers;
  hdr_words[2] = (int32_t)n;  // the caller's layout covers the whole upload
  hdr_words[3] = 0;
  if (n_headers) std::memcpy(hdr_words.data() + 4, header_pos, sizeof(int32_t) * (size_t)n_headers);
  if (!c->dev_params_valid || c->dev_hdr != hdr_words || c->dev_dampen.size() != (size_t)M ||
      std::memcmp(c->dev_dampen.data(), dampen, sizeof(double) * (size_t)M) != 0) {
    int rc;
    // the stream kernels binary-search the list and the tiles stride over it: strictly
    // ascending positions inside the upload (fleet_codec.h), as fleet_acc_create asks.
    // Checked here, where the list is new; a steady-state call compares and launches.
    if ((rc = check_header_positions(c, header_pos, n_headers, n))) return rc;
    // new parameters are uploaded synchronously, which a stream under capture
    // cannot do (it would invalidate the capture): the caller makes one eager
    // call with them first (fleet_codec.h, device-resident entry points)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
      return fail(c, FLEET_ERR_ARG,
                  "dampen / header positions changed while the stream is being captured: make one eager call "
                  "with them before capturing");
    (void)hipGetLastError();
    HIP_TRY(c, hipStreamSynchronize(s));
    // grow; the old buffer may sit in a captured graph: retire it
    const hipError_t eg = c->d_dev_dampen.grow_exact((size_t)M, 64, &c->retired);
    if (eg != hipSuccess) return nomem(c, "hipMalloc", sizeof(double) * (size_t)M, eg);
    HIP_TRY(c, hipMemcpy(c->d_dev_dampen, dampen, sizeof(double) * (size_t)M, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_dev_hdr, hdr_words.data(), sizeof(int32_t) * hdr_words.size(), hipMemcpyHostToDevice));
    c->dev_dampen.assign(dampen, dampen + M);
    c->dev_hdr = hdr_words;
    c->dev_params_valid = true;
  }
  return FLEET_OK;
}

int check_device_update(fleet_ctx* c, size_t pitch, size_t len, size_t* group_begin, size_t* group_end) {
  int rc = check_text_len(c, len);
  if (rc) return rc;
  const size_t groups = groups_of(fleet_b64_count(len));
  if (*group_end > groups) *group_end = groups;
  if (*group_begin > *group_end) return FLEET_ERR_ARG;
  // only columns [16*group_begin, 16*group_end) of each row are touched: rows
  // must not overlap there (a full row, or a window of just those columns)
  if (pitch % 16 != 0 || pitch < 16 * (*group_end - *group_begin))
    return fail(c, FLEET_ERR_ARG, "pitch must be a multiple of 16 covering the selected groups");
  return FLEET_OK;
}

}  // namespace

int fleet_update_device(fleet_ctx* c, const void* d_uploads, size_t pitch, size_t len, int M, const double* dampen,
                        const int32_t* header_pos, int n_headers, size_t group_begin, size_t group_end,
                        void* d_merged, void* d_merged_f32, void* stream) {
  if (!c || !d_uploads || !dampen || M <= 0 || !d_merged || n_headers < 0 || n_headers > FLEET_MAX_HEADERS ||
      (n_headers && !header_pos))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_device_update(c, pitch, len, &group_begin, &group_end);
  if (rc) return rc;
  const size_t n = fleet_b64_count(len);
  hipStream_t s = pick(c, stream);
  if ((rc = dev_params(c, s, n, M, dampen, header_pos, n_headers))) return rc;
  HIP_TRY(c, fleet::launch_update((const uint8_t*)d_uploads, pitch, M, c->d_dev_dampen, (double)1 / M, (int64_t)n,
                                  (int64_t)group_begin, (int64_t)group_end, c->d_dev_hdr, (uint8_t*)d_merged,
                                  (float*)d_merged_f32, c->d_dev_err, s));
  return FLEET_OK;
}

int fleet_update_encode_device(fleet_ctx* c, const void* d_uploads, size_t pitch, size_t len, int M,
                               const double* dampen, const int32_t* header_pos, int n_headers, void* d_merged,
                               void* d_merged_f32, const void* d_values, size_t vpitch, void* d_next_uploads,
                               void* stream) {
  if (!c || !d_uploads || !dampen || M <= 0 || !d_merged || !d_values || !d_next_uploads || n_headers < 0 ||
      n_headers > FLEET_MAX_HEADERS || (n_headers && !header_pos))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t gb = 0, ge = SIZE_MAX;
  int rc = check_device_update(c, pitch, len, &gb, &ge);
  if (rc) return rc;
  const size_t n = fleet_b64_count(len);
  if (vpitch < n) return fail(c, FLEET_ERR_ARG, "vpitch %zu < %zu values", vpitch, n);
  // the encode writes rows [0, M) of d_next_uploads while the update reads d_uploads
  const uintptr_t u0 = (uintptr_t)d_uploads, u1 = u0 + pitch * (size_t)M;
  const uintptr_t e0 = (uintptr_t)d_next_uploads, e1 = e0 + pitch * (size_t)M;
  if (u0 < e1 && e0 < u1) return fail(c, FLEET_ERR_ARG, "d_next_uploads overlaps d_uploads");
  hipStream_t s = pick(c, stream);
  if ((rc = dev_params(c, s, n, M, dampen, header_pos, n_headers))) return rc;
  HIP_TRY(c, fleet::launch_update_encode((const uint8_t*)d_uploads, pitch, M, c->d_dev_dampen, (double)1 / M,
                                         (int64_t)n, c->d_dev_hdr, (uint8_t*)d_merged, (float*)d_merged_f32,
                                         c->d_dev_err, (const float*)d_values, vpitch, (uint8_t*)d_next_uploads, s));
  return FLEET_OK;
}

int fleet_update_kardam_device(fleet_ctx* c, const void* d_uploads, size_t pitch, size_t len, int M,
                               const double* dampen, const int32_t* header_pos, int n_headers, double lr,
                               const void* d_prev, const uint8_t* has_prev, void* d_g_out, size_t vpitch,
                               void* d_merged, void* d_merged_f32, double* norm_g, double* norm_diff, void* stream) {
  if (!c || !d_uploads || !dampen || M <= 0 || !d_merged || !norm_g || !norm_diff || n_headers < 0 ||
      n_headers > FLEET_MAX_HEADERS || (n_headers && !header_pos) || (d_prev && !has_prev))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t gb = 0, ge = SIZE_MAX;
  int rc = check_device_update(c, pitch, len, &gb, &ge);
  if (rc) return rc;
  const size_t n = fleet_b64_count(len);
  if ((d_prev || d_g_out) && vpitch < n) return fail(c, FLEET_ERR_ARG, "vpitch %zu < %zu values", vpitch, n);
  hipStream_t s = pick(c, stream);
  if ((rc = dev_params(c, s, n, M, dampen, header_pos, n_headers))) return rc;
  // one snapshot of the launch plan for the sizing call and the launch (a concurrent
  // fleet_set_plan must not give the launch more partial slots than were sized)
  const fleet::PlanOverrides plan = fleet::plan_overrides();
  int nw_sz = 0, parts_sz = 1, flags_sz = 0;  // partial slots, norm parts per client, tile flags (sizing call)
  fleet::KardamOut kd0{lr, nullptr, nullptr, 0, nullptr, nullptr};
  (void)fleet::launch_update_kardam(nullptr, pitch, M, nullptr, 0.0, (int64_t)n, 0, (int64_t)ge, nullptr, nullptr,
                                    nullptr, nullptr, kd0, &nw_sz, nullptr, &parts_sz, &flags_sz, nullptr, 0, plan, s);
  (void)hipGetLastError();
  const size_t n_waves = (size_t)std::max(nw_sz, 1), n_parts = (size_t)std::max(parts_sz, 1);
  // scratch: [partials M x slots x 2 | norms M x parts x 2 | has_prev M]; synchronous call (host outputs)
  const size_t o_norm = sizeof(double) * 2 * (size_t)M * n_waves;
  const size_t o_has = o_norm + sizeof(double) * 2 * (size_t)M * n_parts;
  if ((rc = grow_dev(c, c->d_b, o_has + (size_t)M + 64))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  double* d_part = reinterpret_cast<double*>(c->d_b.get());
  double* d_norm = reinterpret_cast<double*>(c->d_b + o_norm);
  uint8_t* d_has = c->d_b + o_has;
  if (d_prev) HIP_TRY(c, hipMemcpy(d_has, has_prev, (size_t)M, hipMemcpyHostToDevice));
  fleet::KardamOut kd{lr, (const float*)d_prev, d_prev ? d_has : nullptr, vpitch, (float*)d_g_out, d_part};
  if ((size_t)flags_sz > c->d_kflags.cap()) {  // new flags start at 0, which no launch's epoch is
    HIP_TRY(c, c->d_kflags.grow_exact((size_t)flags_sz));  // the old flags are freed (see the member)
    const hipError_t ez = hipMemsetAsync(c->d_kflags, 0, sizeof(uint32_t) * (size_t)flags_sz, s);
    if (ez != hipSuccess) {
      c->d_kflags.reset();  // flags that were not zeroed are not kept
      return fail(c, FLEET_ERR_HIP, "hipMemsetAsync(c->d_kflags, 0, sizeof(uint32_t) * (size_t)flags_sz, s): %s",
                  hipGetErrorString(ez));
    }
    c->kflag_epoch = 0;
  }
  if (++c->kflag_epoch == 0) {  // wrapped: every flag back to 0 before epoch 1 is used again
    if (c->d_kflags.cap()) HIP_TRY(c, hipMemsetAsync(c->d_kflags, 0, sizeof(uint32_t) * c->d_kflags.cap(), s));
    c->kflag_epoch = 1;
  }
  int nw = 0, np = 1, nf = 0;
  HIP_TRY(c, fleet::launch_update_kardam((const uint8_t*)d_uploads, pitch, M, c->d_dev_dampen, (double)1 / M,
                                         (int64_t)n, 0, (int64_t)ge, c->d_dev_hdr, (uint8_t*)d_merged,
                                         (float*)d_merged_f32, c->d_dev_err, kd, &nw, d_norm, &np, &nf, c->d_kflags,
                                         c->kflag_epoch, plan, s, c->kflag_test_skew));
  if ((size_t)np != n_parts || (size_t)std::max(nw, 1) != n_waves)
    return fail(c, FLEET_ERR_HIP, "Kardam launch plan changed between sizing and launch");
  std::vector<double> norms(2 * (size_t)M * n_parts);
  HIP_TRY(c, hipMemcpyAsync(norms.data(), d_norm, sizeof(double) * norms.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(c->h_err, c->d_dev_err, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  // the pipelined form's reduce blocks wait on the tiles' flags with a bound: a flag that
  // never came leaves FLEET_ERRBIT_SYNC, and the norms are not to be trusted. The call is
  // synchronous, so it fails now (the bit is cleared; other sticky bits stay for fleet_check)
  if (*c->h_err & FLEET_ERRBIT_SYNC) {
    *c->h_err &= ~FLEET_ERRBIT_SYNC;
    HIP_TRY(c, hipMemcpyAsync(c->d_dev_err, c->h_err, sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return fail(c, FLEET_ERR_HIP, "Kardam reduce blocks timed out waiting for the tiles' flags");
  }
  for (int i = 0; i < M; ++i) {
    double a = 0.0, b = 0.0;  // the client's chunk sums, in order
    for (size_t k = 0; k < n_parts; ++k) {
      a += norms[2 * ((size_t)i * n_parts + k)];
      b += norms[2 * ((size_t)i * n_parts + k) + 1];
    }
    norm_g[i] = std::sqrt(a);
    norm_diff[i] = (d_prev && has_prev[i]) ? std::sqrt(b) : std::nan("");
  }
  return FLEET_OK;
}

int fleet_test_kardam_skew(fleet_ctx* c, unsigned skew) {
  if (!c) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  c->kflag_test_skew = skew;
  return FLEET_OK;
}

int fleet_encode_device(fleet_ctx* c, const void* d_values, size_t n, size_t vpitch, int M, void* d_out,
                        size_t pitch, void* stream) {
  if (!c || !d_values || !d_out || M <= 0) return FLEET_ERR_ARG;
  if (pitch % 16 != 0 || pitch < 16 * groups_of(n)) return fail(c, FLEET_ERR_ARG, "bad pitch");
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  HIP_TRY(c, fleet::launch_encode_f32((const float*)d_values, (int64_t)n, vpitch, M, (uint8_t*)d_out, pitch,
                                      pick(c, stream)));
  return FLEET_OK;
}

int fleet_decode_device(fleet_ctx* c, const void* d_text, size_t len, size_t pitch, int M, void* d_values,
                        size_t vpitch, void* stream) {
  if (!c || !d_text || !d_values || M <= 0) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = check_text_len(c, len);
  if (rc) return rc;
  HIP_TRY(c, fleet::launch_decode((const uint8_t*)d_text, (int64_t)fleet_b64_count(len), pitch, M, d_values,
                                  vpitch, 0, c->d_dev_err, pick(c, stream)));
  return FLEET_OK;
}

int fleet_synth_device(fleet_ctx* c, uint64_t seed, int M, int client0, const int32_t* header_pos,
                       const float* header_val, int n_headers, size_t n_up, void* d_values, size_t vpitch,
                       void* stream) {
  return fleet_synth_window_device(c, seed, M, client0, 0, header_pos, header_val, n_headers, n_up, d_values, vpitch,
                                   stream);
}

int fleet_synth_window_device(fleet_ctx* c, uint64_t seed, int M, int client0, size_t elem0,
                              const int32_t* header_pos, const float* header_val, int n_headers, size_t n_up,
                              void* d_values, size_t vpitch, void* stream) {
  if (!c || !d_values || M <= 0 || n_headers < 0 || n_headers > FLEET_MAX_HEADERS || vpitch < n_up)
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  if (n_headers && (!header_pos || !header_val))
    return fail(c, FLEET_ERR_ARG, "synth: %d headers without positions or values", n_headers);
  // k_synth_headers stores at row * vpitch + position: every position inside this tensor's columns
  for (int i = 0; i < n_headers; ++i)
    if (header_pos[i] < 0 || (size_t)header_pos[i] >= n_up)
      return fail(c, FLEET_ERR_ARG, "synth: header position %d (%d) is outside [0, %zu)", i, header_pos[i], n_up);
  DEVICE_SCOPE(c);
  hipStream_t s = pick(c, stream);
  DevBuf<int32_t> d_pos;  // freed on every path
  DevBuf<float> d_val;
  if (n_headers) {
    HIP_TRY(c, d_pos.alloc((size_t)n_headers));
    HIP_TRY(c, d_val.alloc((size_t)n_headers));
    HIP_TRY(c, hipMemcpy(d_pos, header_pos, sizeof(int32_t) * (size_t)n_headers, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_val, header_val, sizeof(float) * (size_t)n_headers, hipMemcpyHostToDevice));
  }
  HIP_TRY(c, fleet::launch_synth(seed, client0, (int64_t)elem0, M, (int64_t)n_up, (float*)d_values, vpitch, d_pos,
                                 d_val, n_headers, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return FLEET_OK;
}

// ------------------------------------------------- mode-1 model codec

namespace {

static int model_total(fleet_ctx* c, const int32_t* dims, int n_mats, size_t* n) {
  if (n_mats < 0 || (n_mats && !dims)) return fail(c, FLEET_ERR_ARG, "bad dims");
  size_t t = 0;
  for (int j = 0; j < n_mats; ++j) {
    if (dims[3 * j] < 0 || dims[3 * j + 1] < 0 || dims[3 * j + 2] < 0) return fail(c, FLEET_ERR_ARG, "negative dim");
    t += (size_t)dims[3 * j] * dims[3 * j + 1] * dims[3 * j + 2];
  }
  if (t > (size_t)INT32_MAX) return fail(c, FLEET_ERR_ARG, "model too large for int32 indices");
  *n = t;
  return FLEET_OK;
}

// quantize + dictionary on the device; leaves d_index and the dictionary on the host
static int model_run(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats, size_t n, float* quantized,
              std::vector<float>* dict_host, int32_t* U, DevBuf<int32_t>* d_index_keep) {
  DevBuf<float> dw, dq, dd;
  if (n) {
    HIP_TRY(c, dw.alloc(n));
    HIP_TRY(c, dq.alloc(n));
    HIP_TRY(c, dd.alloc(n));
    HIP_TRY(c, d_index_keep->alloc(n));
    HIP_TRY(c, hipMemcpyAsync(dw, weights, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, fleet::model_quantize_index(dw, dims, n_mats, dq, dd, *d_index_keep, U, c->stream));
  if (quantized && n) HIP_TRY(c, hipMemcpyAsync(quantized, dq, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  dict_host->resize((size_t)*U);
  if (*U) HIP_TRY(c, hipMemcpyAsync(dict_host->data(), dd, (size_t)*U * sizeof(float), hipMemcpyDeviceToHost,
                                    c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLEET_OK;
}

}  // namespace

int fleet_model_quantize_index(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats,
                               float* quantized, float* dict, int* n_dict, int32_t* index) {
  if (!c) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && !weights) return FLEET_ERR_ARG;
  std::vector<float> dh;
  int32_t U = 0;
  DevBuf<int32_t> di;
  if ((rc = model_run(c, weights, dims, n_mats, n, quantized, &dh, &U, &di))) return rc;
  if (dict && U) std::memcpy(dict, dh.data(), sizeof(float) * (size_t)U);
  if (n_dict) *n_dict = U;
  if (index && n) {
    HIP_TRY(c, hipMemcpy(index, di, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return FLEET_OK;
}

int fleet_model_weights_text(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats, char* out,
                             size_t cap, size_t* out_len) {
  if (!c) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && !weights) return FLEET_ERR_ARG;
  std::vector<float> dh;
  int32_t U = 0;
  DevBuf<int32_t> di;
  if ((rc = model_run(c, weights, dims, n_mats, n, nullptr, &dh, &U, &di))) return rc;
  // header and dictionary lines: `ostream << int` / `ostream << float` (precision 6 == %g),
  // U lines of host formatting; the n index tokens are formatted on the device
  std::string head;
  char buf[64];
  snprintf(buf, sizeof buf, "%zu\n%d\n", n, U);
  head += buf;
  for (int32_t k = 0; k < U; ++k) {
    snprintf(buf, sizeof buf, "%d\n%g\n", k, (double)dh[(size_t)k]);
    head += buf;
  }
  std::vector<char> body;
  HIP_TRY(c, fleet::model_index_text(di, dims, n_mats, &body, c->stream));
  const size_t total = head.size() + body.size();
  if (out_len) *out_len = total;
  if (cap < total) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, total);
  std::memcpy(out, head.data(), head.size());
  if (!body.empty()) std::memcpy(out + head.size(), body.data(), body.size());
  return FLEET_OK;
}

namespace {

// the block offsets of fleet_values_text's sizes; empty for the pairs form
static int values_offsets(fleet_ctx* c, size_t n, const int64_t* block_sizes, int n_blocks, std::vector<int64_t>* off) {
  if (n_blocks < 0 || (n_blocks && !block_sizes)) return fail(c, FLEET_ERR_ARG, "values text: bad blocks");
  if (n > (size_t)INT32_MAX) return fail(c, FLEET_ERR_ARG, "values text: %zu values (the limit is 2^31 - 1)", n);
  off->assign((size_t)n_blocks + 1, 0);
  for (int j = 0; j < n_blocks; ++j) {
    if (block_sizes[j] < 0) return fail(c, FLEET_ERR_ARG, "values text: negative block size");
    (*off)[(size_t)j + 1] = (*off)[(size_t)j] + block_sizes[j];
  }
  if (n_blocks && (size_t)off->back() != n)
    return fail(c, FLEET_ERR_ARG, "values text: the blocks hold %lld values, not %zu", (long long)off->back(), n);
  return FLEET_OK;
}

static int values_text_out(fleet_ctx* c, const float* d_values, size_t n, const std::vector<int64_t>& off,
                           int n_blocks, char* out, size_t cap, size_t* out_len, hipStream_t s) {
  std::vector<char> text;
  const hipError_t e = fleet::model_values_text(d_values, (int64_t)n, off.data(), n_blocks, &text, s);
  if (e == hipErrorInvalidValue)
    return fail(c, FLEET_ERR_ARG, "values text: more than 254 empty blocks in a row");
  HIP_TRY(c, e);
  if (out_len) *out_len = text.size();
  if (!out || cap < text.size()) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, text.size());
  if (!text.empty()) std::memcpy(out, text.data(), text.size());
  return FLEET_OK;
}

}  // namespace

int fleet_values_text_device(fleet_ctx* c, const void* d_values, size_t n, const int64_t* block_sizes, int n_blocks,
                             char* out, size_t cap, size_t* out_len, void* stream) {
  if (!c || (n && !d_values)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<int64_t> off;
  int rc = values_offsets(c, n, block_sizes, n_blocks, &off);
  if (rc) return rc;
  DEVICE_SCOPE(c);
  return values_text_out(c, (const float*)d_values, n, off, n_blocks, out, cap, out_len, pick(c, stream));
}

int fleet_values_text(fleet_ctx* c, const float* values, size_t n, const int64_t* block_sizes, int n_blocks, char* out,
                      size_t cap, size_t* out_len) {
  if (!c || (n && !values)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<int64_t> off;
  int rc = values_offsets(c, n, block_sizes, n_blocks, &off);
  if (rc) return rc;
  DEVICE_SCOPE(c);
  DevBuf<float> dv;
  if (n) {
    HIP_TRY(c, dv.alloc(n));
    HIP_TRY(c, hipMemcpyAsync(dv, values, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  return values_text_out(c, dv, n, off, n_blocks, out, cap, out_len, c->stream);
}

int fleet_model_read_weights(fleet_ctx* c, const char* text, size_t len, const int32_t* dims, int n_mats,
                             float* weights_out) {
  if (!c || (!text && len)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && !weights_out) return FLEET_ERR_ARG;
  // header: loop_counter and U lines (getcleanline + atoi), then U pairs read
  // with `>>` (int, float = strtof); the std::map keeps the first value of a key
  std::string t(text, len);
  const char* p = t.c_str();
  char* e = nullptr;
  (void)strtol(p, &e, 10);
  if (e == p) return fail(c, FLEET_ERR_ARG, "weights section: no loop counter");
  p = e;
  const long U = strtol(p, &e, 10);
  if (e == p || U < 0) return fail(c, FLEET_ERR_ARG, "weights section: no dictionary size");
  p = e;
  std::vector<std::pair<int32_t, float>> kv;
  kv.reserve((size_t)U);
  for (long k = 0; k < U; ++k) {
    const long key = strtol(p, &e, 10);
    if (e == p) return fail(c, FLEET_ERR_ARG, "weights section: bad dictionary index %ld", k);
    p = e;
    const float v = strtof(p, &e);
    if (e == p) return fail(c, FLEET_ERR_ARG, "weights section: bad dictionary value %ld", k);
    p = e;
    kv.emplace_back((int32_t)key, v);
  }
  std::stable_sort(kv.begin(), kv.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  std::vector<int32_t> keys;
  std::vector<float> vals;
  for (size_t k = 0; k < kv.size(); ++k)
    if (k == 0 || kv[k].first != kv[k - 1].first) keys.push_back(kv[k].first), vals.push_back(kv[k].second);
  const size_t body = (size_t)(p - t.c_str());
  const size_t blen = len - body;
  DevBuf<uint8_t> dt;
  DevBuf<int32_t> dk;
  DevBuf<float> dv, dw;
  if (blen) HIP_TRY(c, dt.alloc(blen));
  HIP_TRY(c, dk.alloc(keys.size() + 1));
  HIP_TRY(c, dv.alloc(vals.size() + 1));
  if (n) HIP_TRY(c, dw.alloc(n));
  if (blen) HIP_TRY(c, hipMemcpyAsync(dt, text + body, blen, hipMemcpyHostToDevice, c->stream));
  if (!keys.empty()) {
    HIP_TRY(c, hipMemcpyAsync(dk, keys.data(), sizeof(int32_t) * keys.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dv, vals.data(), sizeof(float) * vals.size(), hipMemcpyHostToDevice, c->stream));
  }
  int status = 0;
  HIP_TRY(c, fleet::model_read_index(dt, (int64_t)blen, (int64_t)n, dk, dv, (int32_t)keys.size(), dw, &status,
                                     c->stream));
  if (status == 1) return fail(c, FLEET_ERR_ARG, "weights section: malformed index token");
  if (status == 2) return fail(c, FLEET_ERR_LAYOUT, "weights section: index count differs from the model size");
  if (n) HIP_TRY(c, hipMemcpy(weights_out, dw, sizeof(float) * n, hipMemcpyDeviceToHost));
  return FLEET_OK;
}

// ------------------------------------------ model parameters (getModelParametersNative)

int fleet_model_params_device(fleet_ctx* c, const float* d_weights, size_t n_weights, const float* d_biases,
                              size_t n_biases, int graph_edges, void* d_out, void* stream) {
  if (!c || !d_out || graph_edges < 0 || (n_weights && !d_weights) || (n_biases && graph_edges && !d_biases))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  HIP_TRY(c, fleet::launch_encode_model_params(d_weights, (int64_t)n_weights, d_biases, (int64_t)n_biases,
                                               n_biases ? (int64_t)graph_edges : 0, (uint8_t*)d_out,
                                               pick(c, stream)));
  return FLEET_OK;
}

int fleet_kardam_grads(fleet_ctx* c, const char* const* uploads, const size_t* lens, int M, const double* dampen,
                       double lr, const char* const* prev, char* g_out, size_t g_pitch, size_t* g_len,
                       double* norm_g, double* norm_diff) {
  if (!c || !uploads || !lens || !dampen || M <= 0 || !norm_g || !norm_diff) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const size_t len = lens[0];
  int rc = check_text_len(c, len);
  if (rc) return rc;
  for (int i = 0; i < M; ++i)
    if (!uploads[i] || lens[i] != len)
      return fail(c, FLEET_ERR_ARG, "upload %d has length %zu, expected %zu (one model layout)", i, lens[i], len);
  const size_t n = fleet_b64_count(len);
  // no caller positions here: the list k_kardam_grads counts over is this walk's own,
  // ascending and inside [0, n) by construction (host_layout_parse), so nothing to validate
  std::vector<int32_t> hw(kHdrWords);
  host_layout_parse(uploads[M - 1], len, (int64_t)n, FLEET_MAX_HEADERS, hw.data());
  if (hw[0] != 0) return fail(c, FLEET_ERR_LAYOUT, "last upload's header does not describe a gradient layout");
  const int nh = hw[1];
  const size_t n_flat = (size_t)hw[2] - (size_t)nh;  // flatGrad stops after the last bias block
  const size_t glen = fleet_b64_len(n_flat), gpad = round16(glen) + 16;
  if (g_len) *g_len = glen;
  if (!g_out || g_pitch < glen) return fail(c, FLEET_ERR_CAPACITY, "g row pitch %zu < %zu", g_pitch, glen);
  const size_t pitch = round16(len);
  bool any_prev = false;
  for (int i = 0; prev && i < M; ++i) any_prev |= prev[i] != nullptr;
  // staging: [uploads | prev rows | has_prev | dampen | header positions]; device adds [g rows | partials]
  const size_t o_prev = pitch * (size_t)M, o_has = o_prev + (any_prev ? gpad * (size_t)M : 0);
  const size_t o_damp = round16(o_has + (size_t)M), o_hdr = round16(o_damp + sizeof(double) * (size_t)M);
  const size_t o_g = round16(o_hdr + sizeof(int32_t) * (size_t)(nh + 1));
  const int64_t groups = (int64_t)groups_of(n_flat);
  const int nblk = (int)((groups + 255) / 256);
  const size_t o_part = round16(o_g + gpad * (size_t)M), o_end = o_part + sizeof(double) * 2 * (size_t)M * (nblk + 1);
  if ((rc = grow_pinned(c, o_end))) return rc;
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // staging buffer reuse
  uint8_t* h = c->h_stage;
  for (int i = 0; i < M; ++i) {
    std::memcpy(h + (size_t)i * pitch, uploads[i], len);
    std::memset(h + (size_t)i * pitch + len, 0, pitch - len);
    h[o_has + i] = (uint8_t)(prev && prev[i]);
    if (any_prev) {
      uint8_t* row = h + o_prev + (size_t)i * gpad;
      std::memset(row, 'A', gpad);
      if (prev[i]) std::memcpy(row, prev[i], glen);
    }
  }
  std::memcpy(h + o_damp, dampen, sizeof(double) * (size_t)M);
  std::memcpy(h + o_hdr, hw.data() + 4, sizeof(int32_t) * (size_t)nh);
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, h, o_g, hipMemcpyHostToDevice, c->stream));
  int nb = 0;
  HIP_TRY(c, fleet::launch_kardam_grads(d, pitch, M, (const int32_t*)(d + o_hdr), nh, (int64_t)n_flat,
                                        (const double*)(d + o_damp), lr, any_prev ? d + o_prev : nullptr, gpad,
                                        d + o_has, d + o_g, gpad, (double*)(d + o_part), &nb, c->d_err, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + o_g, d + o_g, o_end - o_g, hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  const double* part = (const double*)(h + o_part);
  for (int i = 0; i < M; ++i) {
    std::memcpy(g_out + (size_t)i * g_pitch, h + o_g + (size_t)i * gpad, glen);
    double sg = 0, sd = 0;
    for (int b = 0; b < nb; ++b) {  // block partials in index order
      sg += part[(size_t)i * 2 * nb + b];
      sd += part[(size_t)i * 2 * nb + nb + b];
    }
    norm_g[i] = std::sqrt(sg);
    norm_diff[i] = (prev && prev[i]) ? std::sqrt(sd) : std::nan("");
  }
  return FLEET_OK;
}

size_t fleet_minibatch_len(int F, int B, int num_labels, int with_teacher) {
  if (F < 0 || B < 0 || num_labels < 0) return 0;
  const size_t n = 7 + (size_t)B * ((size_t)F + (with_teacher ? (size_t)num_labels : 0) + 1) + (with_teacher ? 1 : 0);
  return fleet_b64_len(n);
}

int fleet_minibatch_device(fleet_ctx* c, const void* d_images, size_t n_images, int F, const void* d_labels,
                           const void* d_idx, int B, const void* d_teacher, int num_labels, const float header[7],
                           void* d_out, void* stream) {
  if (!c || !d_out || !header || F < 0 || B < 0 || num_labels < 0 || (B && (!d_idx || !d_labels || !d_images)) ||
      (d_teacher && num_labels == 0))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  HIP_TRY(c, fleet::launch_encode_minibatch((const float*)d_images, (int64_t)n_images, F, (const int32_t*)d_labels,
                                            (const int32_t*)d_idx, B, (const float*)d_teacher, num_labels, header,
                                            (uint8_t*)d_out, c->d_dev_err, pick(c, stream)));
  return FLEET_OK;
}

int fleet_minibatch(fleet_ctx* c, const float* images, size_t n_images, int F, const int32_t* labels,
                    const int32_t* idx, int B, const float* teacher, int num_labels, const float header[7],
                    char* out, size_t cap, size_t* out_len) {
  if (!c || !header || F < 0 || B < 0 || num_labels < 0 || (B && (!idx || !labels || !images)) ||
      (teacher && num_labels == 0))
    return FLEET_ERR_ARG;
  const size_t len = fleet_minibatch_len(F, B, num_labels, teacher != nullptr);
  if (out_len) *out_len = len;
  if (cap < len || !out) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, len);
  for (int b = 0; b < B; ++b)
    if (idx[b] < 0 || (size_t)idx[b] >= n_images)
      return fail(c, FLEET_ERR_ARG, "sample %d: index %d outside the %zu images", b, idx[b], n_images);
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  // staging: [B x F features | B labels | 0..B-1 | B x NL teacher]; the device gathers nothing
  const size_t nl = teacher ? (size_t)num_labels : 0;
  const size_t o_lab = round16(sizeof(float) * (size_t)B * (size_t)F), o_idx = o_lab + round16(4 * (size_t)B);
  const size_t o_tea = o_idx + round16(4 * (size_t)B), o_out = o_tea + round16(sizeof(float) * (size_t)B * nl);
  const size_t o_end = o_out + round16(len) + 16;
  int rc;
  if ((rc = grow_pinned(c, o_end))) return rc;
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // staging buffer reuse
  uint8_t* h = c->h_stage;
  for (int b = 0; b < B; ++b) {
    std::memcpy(h + sizeof(float) * (size_t)b * F, images + (size_t)idx[b] * F, sizeof(float) * (size_t)F);
    reinterpret_cast<int32_t*>(h + o_lab)[b] = labels[idx[b]];
    reinterpret_cast<int32_t*>(h + o_idx)[b] = b;
  }
  if (teacher) std::memcpy(h + o_tea, teacher, sizeof(float) * (size_t)B * nl);
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fleet::launch_encode_minibatch((const float*)d, (int64_t)B, F, (const int32_t*)(d + o_lab),
                                            (const int32_t*)(d + o_idx), B, teacher ? (const float*)(d + o_tea) : nullptr,
                                            num_labels, header, d + o_out, c->d_err, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + o_out, d + o_out, len, hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  std::memcpy(out, h + o_out, len);
  return FLEET_OK;
}

size_t fleet_teacher_weight_count(void) { return (size_t)fleet::teacher_weight_count(); }
size_t fleet_teacher_bias_count(void) { return (size_t)fleet::teacher_bias_count(); }

int fleet_teacher_forward_device(fleet_ctx* c, const void* d_w, const void* d_b, const void* d_images, size_t n_images,
                                 int F, const void* d_idx, int B, float temperature, void* d_probs, void* stream) {
  if (!c || B < 0 || (B && (!d_w || !d_b || !d_images || !d_probs)) || F < 28 * 28) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  HIP_TRY(c, fleet::launch_teacher_forward((const float*)d_w, (const float*)d_b, (const float*)d_images,
                                           (int64_t)n_images, F, (const int32_t*)d_idx, B, temperature,
                                           (float*)d_probs, c->d_dev_err, pick(c, stream)));
  return FLEET_OK;
}

int fleet_teacher_forward(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                          size_t n_images, int F, const int32_t* idx, int B, float temperature, float* probs) {
  if (!c || B < 0 || F < 28 * 28 || (B && (!w || !b || !images || !idx || !probs))) return FLEET_ERR_ARG;
  if (n_w != fleet_teacher_weight_count() || n_b != fleet_teacher_bias_count())
    return fail(c, FLEET_ERR_ARG, "teacher: %zu weights and %zu biases, expected %zu and %zu", n_w, n_b,
                fleet_teacher_weight_count(), fleet_teacher_bias_count());
  for (int i = 0; i < B; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return fail(c, FLEET_ERR_ARG, "sample %d: index %d outside the %zu images", i, idx[i], n_images);
  if (B == 0) return FLEET_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  // staging: [w | b | B gathered rows | B x 10 probs]
  const size_t o_b = round16(sizeof(float) * n_w), o_x = o_b + round16(sizeof(float) * n_b);
  const size_t o_p = o_x + round16(sizeof(float) * (size_t)B * (size_t)F);
  const size_t o_end = o_p + round16(sizeof(float) * (size_t)B * 10);
  int rc;
  if ((rc = grow_pinned(c, o_end))) return rc;
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // staging buffer reuse
  uint8_t* h = c->h_stage;
  std::memcpy(h, w, sizeof(float) * n_w);
  std::memcpy(h + o_b, b, sizeof(float) * n_b);
  for (int i = 0; i < B; ++i)
    std::memcpy(h + o_x + sizeof(float) * (size_t)i * F, images + (size_t)idx[i] * F, sizeof(float) * (size_t)F);
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, h, o_p, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fleet::launch_teacher_forward((const float*)d, (const float*)(d + o_b), (const float*)(d + o_x), B, F,
                                           nullptr, B, temperature, (float*)(d + o_p), c->d_err, c->stream));
  HIP_TRY(c, hipMemcpyAsync(h + o_p, d + o_p, sizeof(float) * (size_t)B * 10, hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  std::memcpy(probs, h + o_p, sizeof(float) * (size_t)B * 10);
  return FLEET_OK;
}

size_t fleet_evaluate_block_images(void) { return (size_t)fleet::eval_block_images(); }
int fleet_evaluate_set_grid(int max_blocks) { return fleet::eval_set_grid(max_blocks); }

int fleet_evaluate_device(fleet_ctx* c, const void* d_w, const void* d_b, const void* d_images, size_t n_images, int F,
                          const void* d_labels, const void* d_idx, int B, void* d_pred, void* d_prob, void* d_cost,
                          void* d_probs10, void* d_result, void* stream) {
  if (!c || !d_w || !d_b || !d_images || !d_labels || !d_result || B <= 0 || F < 28 * 28 || n_images == 0 ||
      (!d_idx && (size_t)B > n_images))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (!d_cost || !d_pred) {
    const hipError_t e = c->d_eval.grow_exact(8 * (size_t)B, 64, &c->retired);
    if (e != hipSuccess) return nomem(c, "hipMalloc", 8 * (size_t)B, e);
  }
  float* cost = d_cost ? (float*)d_cost : (float*)c->d_eval.get();
  int32_t* pred = d_pred ? (int32_t*)d_pred : (int32_t*)(c->d_eval + c->d_eval.cap() / 2);  // behind the costs
  HIP_TRY(c, fleet::launch_eval((const float*)d_w, (const float*)d_b, (const float*)d_images, (int64_t)n_images, F,
                                (const int32_t*)d_labels, (const int32_t*)d_idx, B, pred, (float*)d_prob, cost,
                                (float*)d_probs10, (float*)d_result, c->d_dev_err, pick(c, stream)));
  return FLEET_OK;
}

int fleet_evaluate(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                   size_t n_images, int F, const int32_t* labels, const int32_t* idx, int B, float* error,
                   float* accuracy, int32_t* correct, int32_t* pred, float* prob) {
  if (!c || !w || !b || !images || !labels || B <= 0 || F < 28 * 28 || n_images == 0) return FLEET_ERR_ARG;
  if (n_w != fleet_teacher_weight_count() || n_b != fleet_teacher_bias_count())
    return fail(c, FLEET_ERR_ARG, "evaluate: %zu weights and %zu biases, expected %zu and %zu", n_w, n_b,
                fleet_teacher_weight_count(), fleet_teacher_bias_count());
  if (!idx && (size_t)B > n_images) return fail(c, FLEET_ERR_ARG, "evaluate: %d images asked of %zu", B, n_images);
  for (int i = 0; idx && i < B; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return fail(c, FLEET_ERR_ARG, "image %d: index %d outside the %zu images", i, idx[i], n_images);
  // the images the evaluation reads: all of them with idx, the first B without
  const size_t rows = idx ? n_images : (size_t)B;
  const size_t o_b = round16(sizeof(float) * n_w), o_x = o_b + round16(sizeof(float) * n_b);
  const size_t o_l = o_x + round16(sizeof(float) * rows * (size_t)F), o_i = o_l + round16(4 * rows);
  const size_t o_pred = o_i + round16(4 * (size_t)B), o_prob = o_pred + round16(4 * (size_t)B);
  const size_t o_cost = o_prob + round16(4 * (size_t)B), o_res = o_cost + round16(4 * (size_t)B), o_end = o_res + 16;
  uint8_t* d = nullptr;
  int rc;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DEVICE_SCOPE(c);
    if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    d = c->d_a;
    HIP_TRY(c, hipMemcpyAsync(d, w, sizeof(float) * n_w, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_b, b, sizeof(float) * n_b, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_x, images, sizeof(float) * rows * (size_t)F, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_l, labels, 4 * rows, hipMemcpyHostToDevice, c->stream));
    if (idx) HIP_TRY(c, hipMemcpyAsync(d + o_i, idx, 4 * (size_t)B, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, fleet::launch_eval((const float*)d, (const float*)(d + o_b), (const float*)(d + o_x), (int64_t)rows, F,
                                  (const int32_t*)(d + o_l), idx ? (const int32_t*)(d + o_i) : nullptr, B,
                                  (int32_t*)(d + o_pred), (float*)(d + o_prob), (float*)(d + o_cost), nullptr,
                                  (float*)(d + o_res), c->d_err, c->stream));
    float res[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(res, d + o_res, 12, hipMemcpyDeviceToHost, c->stream));
    if (pred) HIP_TRY(c, hipMemcpyAsync(pred, d + o_pred, 4 * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    if (prob) HIP_TRY(c, hipMemcpyAsync(prob, d + o_prob, 4 * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_err(c, c->stream))) return rc;
    if (error) *error = res[0];
    if (accuracy) *accuracy = res[1];
    if (correct) std::memcpy(correct, &res[2], 4);
  }
  return FLEET_OK;
}

// ------------------------------------------ test() on the CIFAR network (cifar_kernels.hip)

size_t fleet_cifar_weight_count(int classes) { return (size_t)fleet::cifarnet::weight_count(classes); }
size_t fleet_cifar_bias_count(int classes) { return (size_t)fleet::cifarnet::bias_count(classes); }
size_t fleet_cifar_block_images(void) { return (size_t)fleet::cifar_block_images(); }
int fleet_cifar_set_grid(int max_blocks) { return fleet::cifar_set_grid(max_blocks); }

int fleet_cifar_test_device(fleet_ctx* c, int classes, const void* d_w, const void* d_b, const void* d_images,
                            size_t n_images, int F, const void* d_labels, const void* d_idx, int B, void* d_pred,
                            void* d_prob, void* d_cost, void* d_probsN, void* d_result, void* stream) {
  if (!c || !fleet::cifarnet::classes_ok(classes) || !d_w || !d_b || !d_images || !d_labels || !d_result || B <= 0 ||
      F < fleet::cifarnet::kPix || n_images == 0 || (!d_idx && (size_t)B > n_images))
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (!d_cost || !d_pred) {  // the evaluation's workspace and its rule
    const hipError_t e = c->d_eval.grow_exact(8 * (size_t)B, 64, &c->retired);
    if (e != hipSuccess) return nomem(c, "hipMalloc", 8 * (size_t)B, e);
  }
  float* cost = d_cost ? (float*)d_cost : (float*)c->d_eval.get();
  int32_t* pred = d_pred ? (int32_t*)d_pred : (int32_t*)(c->d_eval + c->d_eval.cap() / 2);  // behind the costs
  HIP_TRY(c, fleet::launch_cifar_test(classes, (const float*)d_w, (const float*)d_b, (const float*)d_images,
                                      (int64_t)n_images, F, (const int32_t*)d_labels, (const int32_t*)d_idx, B, pred,
                                      (float*)d_prob, cost, (float*)d_probsN, (float*)d_result, c->d_dev_err,
                                      pick(c, stream)));
  return FLEET_OK;
}

int fleet_cifar_test(fleet_ctx* c, int classes, const float* w, size_t n_w, const float* b, size_t n_b,
                     const float* images, size_t n_images, int F, const int32_t* labels, const int32_t* idx, int B,
                     float* error, float* accuracy, int32_t* correct, int32_t* pred, float* prob, float* cost,
                     float* probsN) {
  if (!c || !w || !b || !images || !labels || B <= 0 || F < fleet::cifarnet::kPix || n_images == 0) return FLEET_ERR_ARG;
  if (!fleet::cifarnet::classes_ok(classes)) return fail(c, FLEET_ERR_ARG, "cifar test: %d classes, the network has 10 or 100", classes);
  if (n_w != fleet_cifar_weight_count(classes) || n_b != fleet_cifar_bias_count(classes))
    return fail(c, FLEET_ERR_ARG, "cifar test: %zu weights and %zu biases, expected %zu and %zu", n_w, n_b,
                fleet_cifar_weight_count(classes), fleet_cifar_bias_count(classes));
  if (!idx && (size_t)B > n_images) return fail(c, FLEET_ERR_ARG, "cifar test: %d images asked of %zu", B, n_images);
  for (int i = 0; idx && i < B; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return fail(c, FLEET_ERR_ARG, "image %d: index %d outside the %zu images", i, idx[i], n_images);
  // the images the evaluation reads: all of them with idx, the first B without
  const size_t rows = idx ? n_images : (size_t)B, nB = (size_t)B;
  const size_t o_b = round16(sizeof(float) * n_w), o_x = o_b + round16(sizeof(float) * n_b);
  const size_t o_l = o_x + round16(sizeof(float) * rows * (size_t)F), o_i = o_l + round16(4 * rows);
  const size_t o_pred = o_i + round16(4 * nB), o_prob = o_pred + round16(4 * nB), o_cost = o_prob + round16(4 * nB);
  const size_t o_pn = o_cost + round16(4 * nB), o_res = o_pn + (probsN ? round16(4 * nB * (size_t)classes) : 0);
  const size_t o_end = o_res + 16;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc;
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, w, sizeof(float) * n_w, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_b, b, sizeof(float) * n_b, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_x, images, sizeof(float) * rows * (size_t)F, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_l, labels, 4 * rows, hipMemcpyHostToDevice, c->stream));
  if (idx) HIP_TRY(c, hipMemcpyAsync(d + o_i, idx, 4 * nB, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fleet::launch_cifar_test(classes, (const float*)d, (const float*)(d + o_b), (const float*)(d + o_x),
                                      (int64_t)rows, F, (const int32_t*)(d + o_l),
                                      idx ? (const int32_t*)(d + o_i) : nullptr, B, (int32_t*)(d + o_pred),
                                      (float*)(d + o_prob), (float*)(d + o_cost),
                                      probsN ? (float*)(d + o_pn) : nullptr, (float*)(d + o_res), c->d_err, c->stream));
  float res[4] = {0, 0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(res, d + o_res, 12, hipMemcpyDeviceToHost, c->stream));
  if (pred) HIP_TRY(c, hipMemcpyAsync(pred, d + o_pred, 4 * nB, hipMemcpyDeviceToHost, c->stream));
  if (prob) HIP_TRY(c, hipMemcpyAsync(prob, d + o_prob, 4 * nB, hipMemcpyDeviceToHost, c->stream));
  if (cost) HIP_TRY(c, hipMemcpyAsync(cost, d + o_cost, 4 * nB, hipMemcpyDeviceToHost, c->stream));
  if (probsN) HIP_TRY(c, hipMemcpyAsync(probsN, d + o_pn, 4 * nB * (size_t)classes, hipMemcpyDeviceToHost, c->stream));
  if ((rc = read_err(c, c->stream))) return rc;
  if (error) *error = res[0];
  if (accuracy) *accuracy = res[1];
  if (correct) std::memcpy(correct, &res[2], 4);
  return FLEET_OK;
}

// ------------------------------------------ the client's getGradients (client_kernels.hip)

size_t fleet_client_grad_len(void) { return (size_t)fleet::client_grad_len(); }
int fleet_client_grad_set_chunk(int max_clients) { return fleet::client_grad_set_chunk(max_clients); }

// Client/app/src/main/cpp/cppNN-lib.cpp:101-113, 218-234; commonLib/cppNN/network.h:1806-2008,
// 1551-1611, 1289-1331, 1038-1056
namespace {

// the cost and the DP parameters of the _ex_ forms, before anything else is looked at
bool client_ex_args_ok(int cost, const float* clip, const float* sigma, int C) {
  if (cost != FLEET_COST_CROSS_ENTROPY && cost != FLEET_COST_DISTILLATION) return false;
  if (!clip != !sigma) return false;
  for (int c = 0; clip && c < C; ++c) {
    if (!(sigma[c] >= 0.0f) || std::isinf(sigma[c])) return false;
    if (sigma[c] > 0.0f && (!(clip[c] > 0.0f) || std::isinf(clip[c]))) return false;
  }
  return true;
}

// every form, the lock held and the device set: the workspace, the launches per chunk of
// clients, the encode of the rows; err: the error word the kernels report to. clip, sigma: host
// [C] or both NULL (checked by client_ex_args_ok).
int client_grads_locked(fleet_ctx* c, const void* d_models, size_t model_pitch, int n_models,
                        const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                        const void* d_labels, const void* d_idx, const void* d_shift, int C, int B, float temperature,
                        int cost, const float* clip, const float* sigma, void* d_grads, size_t grad_pitch,
                        void* d_uploads, size_t upload_pitch, hipStream_t s) {
  const size_t n_up = fleet_client_grad_len();
  const int chunk = fleet::client_grad_chunk(C, B);
  const size_t rows_bytes = fleet::client_grad_workspace_bytes(chunk, B);
  std::vector<uint8_t> dp_of_client;
  bool dp = false;
  if (sigma) {
    dp_of_client.resize((size_t)C);
    for (int i = 0; i < C; ++i) dp |= (dp_of_client[(size_t)i] = sigma[i] > 0.0f) != 0;
  }
  // the scales lie behind the rows, with or without DP, so a DP call grows nothing a plain one made
  const size_t need = rows_bytes + fleet::client_grad_scale_bytes(chunk, B);
  const hipError_t ew = c->d_client_ws.grow_exact(need, 64, &c->retired);
  if (ew != hipSuccess) return nomem(c, "hipMalloc", need, ew);
  if (dp) {
    if (!c->d_dp_z) {  // once per context
      // the host table is made once per process and kept: every context uploads the same draws
      static const std::vector<double> z = [n_up] {
        std::vector<double> t(n_up);
        fleet::client_dp_noise(t.data(), t.size());
        return t;
      }();
      const hipError_t e = c->d_dp_z.alloc(n_up);
      if (e != hipSuccess) return nomem(c, "hipMalloc", sizeof(double) * n_up, e);
      const hipError_t e2 = hipMemcpy(c->d_dp_z, z.data(), sizeof(double) * n_up, hipMemcpyHostToDevice);
      if (e2 != hipSuccess) {
        c->d_dp_z.reset();
        return fail(c, FLEET_ERR_HIP, "the DP noise table: %s", hipGetErrorString(e2));
      }
    }
    const hipError_t ed = c->d_client_dp.grow_exact(2 * (size_t)C, 0, &c->retired);
    if (ed != hipSuccess) return nomem(c, "hipMalloc", 8 * (size_t)C, ed);
    // pageable sources: the copies have left clip and sigma when the call returns
    HIP_TRY(c, hipMemcpyAsync(c->d_client_dp, clip, sizeof(float) * (size_t)C, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_client_dp + C, sigma, sizeof(float) * (size_t)C, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(c, fleet::launch_client_grads_ex((const float*)d_models, (int64_t)model_pitch, n_models,
                                           (const int32_t*)d_model_of_client, (const float*)d_images,
                                           (int64_t)n_images, F, (const int32_t*)d_labels, (const int32_t*)d_idx,
                                           (const int32_t*)d_shift, C, B, chunk, temperature, cost,
                                           dp ? c->d_client_dp : nullptr, dp ? c->d_client_dp + C : nullptr,
                                           dp ? dp_of_client.data() : nullptr, dp ? c->d_dp_z : nullptr,
                                           dp ? (float*)(c->d_client_ws + rows_bytes) : nullptr,
                                           (float*)c->d_client_ws.get(), (float*)d_grads, (int64_t)grad_pitch, c->d_dev_err, s));
  if (d_uploads)
    HIP_TRY(c, fleet::launch_encode_f32((const float*)d_grads, (int64_t)n_up, grad_pitch, C, (uint8_t*)d_uploads,
                                        upload_pitch, s));
  return FLEET_OK;
}

}  // namespace

int fleet_client_dp_noise(double* out, size_t n) {
  if (!out || n > fleet_client_grad_len()) return FLEET_ERR_ARG;
  fleet::client_dp_noise(out, n);
  return FLEET_OK;
}

int fleet_client_ex_grads_device(fleet_ctx* c, const void* d_models, size_t model_pitch, int n_models,
                                 const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                                 const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                                 float temperature, int cost, const float* clip, const float* sigma, void* d_grads,
                                 size_t grad_pitch, void* d_uploads, size_t upload_pitch, void* stream) {
  const size_t n_up = fleet_client_grad_len();
  if (!c || !d_models || !d_images || !d_labels || !d_grads || C <= 0 || B <= 0 || F < 28 * 28 || n_models <= 0 ||
      n_images == 0 || model_pitch < fleet_teacher_weight_count() + fleet_teacher_bias_count() || grad_pitch < n_up ||
      (size_t)C * (size_t)B > (size_t)INT32_MAX || (!d_idx && (size_t)C * (size_t)B > n_images))
    return FLEET_ERR_ARG;
  if (!client_ex_args_ok(cost, clip, sigma, C))
    return fail(c, FLEET_ERR_ARG, "client gradients: cost 0 or 1; clip and sigma both or neither, sigma >= 0 and "
                                  "finite, clip > 0 and finite where sigma > 0");
  if (d_uploads && (upload_pitch % 16 != 0 || upload_pitch < 16 * groups_of(n_up)))
    return fail(c, FLEET_ERR_ARG, "bad upload pitch");
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  return client_grads_locked(c, d_models, model_pitch, n_models, d_model_of_client, d_images, n_images, F, d_labels, d_idx,
                             d_shift, C, B, temperature, cost, clip, sigma, d_grads, grad_pitch, d_uploads, upload_pitch,
                             pick(c, stream));
}

int fleet_client_grads_device(fleet_ctx* c, const void* d_models, size_t model_pitch, int n_models,
                              const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                              const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                              float temperature, void* d_grads, size_t grad_pitch, void* d_uploads,
                              size_t upload_pitch, void* stream) {
  return fleet_client_ex_grads_device(c, d_models, model_pitch, n_models, d_model_of_client, d_images, n_images, F,
                                      d_labels, d_idx, d_shift, C, B, temperature, FLEET_COST_CROSS_ENTROPY, nullptr,
                                      nullptr, d_grads, grad_pitch, d_uploads, upload_pitch, stream);
}

int fleet_client_ex_grads(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                          size_t n_images, int F, const int32_t* labels, const int32_t* idx, const int32_t* shifts,
                          int C, int B, float temperature, int cost, const float* clip, const float* sigma,
                          float* grads, char* uploads, size_t upload_pitch) {
  if (!c || !w || !b || !images || !labels || !grads || C <= 0 || B <= 0 || F < 28 * 28 || n_images == 0)
    return FLEET_ERR_ARG;
  if (!client_ex_args_ok(cost, clip, sigma, C))
    return fail(c, FLEET_ERR_ARG, "client gradients: cost 0 or 1; clip and sigma both or neither, sigma >= 0 and "
                                  "finite, clip > 0 and finite where sigma > 0");
  if (n_w != fleet_teacher_weight_count() || n_b != fleet_teacher_bias_count())
    return fail(c, FLEET_ERR_ARG, "client gradients: %zu weights and %zu biases, expected %zu and %zu", n_w, n_b,
                fleet_teacher_weight_count(), fleet_teacher_bias_count());
  const size_t n = (size_t)C * (size_t)B, n_up = fleet_client_grad_len();
  if (n > (size_t)INT32_MAX) return fail(c, FLEET_ERR_ARG, "client gradients: %d clients of %d samples", C, B);
  if (!idx && n > n_images) return fail(c, FLEET_ERR_ARG, "client gradients: %zu images asked of %zu", n, n_images);
  for (size_t i = 0; idx && i < n; ++i)
    if (idx[i] < 0 || (size_t)idx[i] >= n_images)
      return fail(c, FLEET_ERR_ARG, "sample %zu: index %d outside the %zu images", i, idx[i], n_images);
  for (size_t i = 0; shifts && i < 2 * n; ++i)
    if (shifts[i] < -1 || shifts[i] > 1)
      return fail(c, FLEET_ERR_ARG, "sample %zu: shift %d outside {-1, 0, 1}", i / 2, shifts[i]);
  const size_t up_len = fleet_b64_len(n_up), groups_bytes = 16 * groups_of(n_up);
  if (uploads && upload_pitch < up_len) return fail(c, FLEET_ERR_CAPACITY, "upload pitch %zu < %zu", upload_pitch, up_len);
  const size_t rows = idx ? n_images : n;  // the images the call reads
  const size_t o_x = round16(sizeof(float) * (n_w + n_b)), o_l = o_x + round16(sizeof(float) * rows * (size_t)F);
  const size_t o_i = o_l + round16(4 * rows), o_s = o_i + round16(4 * n), o_g = o_s + round16(8 * n);
  const size_t o_u = o_g + round16(sizeof(float) * (size_t)C * n_up), o_end = o_u + (uploads ? (size_t)C * groups_bytes : 0);
  int rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if ((rc = grow_dev(c, c->d_a, o_end))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint8_t* d = c->d_a;
  HIP_TRY(c, hipMemcpyAsync(d, w, sizeof(float) * n_w, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + sizeof(float) * n_w, b, sizeof(float) * n_b, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_x, images, sizeof(float) * rows * (size_t)F, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d + o_l, labels, 4 * rows, hipMemcpyHostToDevice, c->stream));
  if (idx) HIP_TRY(c, hipMemcpyAsync(d + o_i, idx, 4 * n, hipMemcpyHostToDevice, c->stream));
  if (shifts) HIP_TRY(c, hipMemcpyAsync(d + o_s, shifts, 8 * n, hipMemcpyHostToDevice, c->stream));
  if ((rc = client_grads_locked(c, d, n_w + n_b, 1, nullptr, d + o_x, rows, F, d + o_l, idx ? d + o_i : nullptr,
                                shifts ? d + o_s : nullptr, C, B, temperature, cost, clip, sigma, d + o_g, n_up,
                                uploads ? d + o_u : nullptr, groups_bytes, c->stream)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(grads, d + o_g, sizeof(float) * (size_t)C * n_up, hipMemcpyDeviceToHost, c->stream));
  if (uploads)
    HIP_TRY(c, hipMemcpy2DAsync(uploads, upload_pitch, d + o_u, groups_bytes, up_len, (size_t)C, hipMemcpyDeviceToHost,
                                c->stream));
  return read_err(c, c->stream, c->d_dev_err);
}

int fleet_client_grads(fleet_ctx* c, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                       size_t n_images, int F, const int32_t* labels, const int32_t* idx, const int32_t* shifts, int C,
                       int B, float temperature, float* grads, char* uploads, size_t upload_pitch) {
  return fleet_client_ex_grads(c, w, n_w, b, n_b, images, n_images, F, labels, idx, shifts, C, B, temperature,
                               FLEET_COST_CROSS_ENTROPY, nullptr, nullptr, grads, uploads, upload_pitch);
}

int fleet_model_params(fleet_ctx* c, const float* weights, size_t n_weights, const float* biases, size_t n_biases,
                       int graph_edges, char* out, size_t cap, size_t* out_len) {
  if (!c || graph_edges < 0 || (n_weights && !weights) || (n_biases && !biases)) return FLEET_ERR_ARG;
  const size_t n = n_biases * (size_t)graph_edges + n_weights;
  const size_t len = fleet_b64_len(n);
  if (out_len) *out_len = len;
  if (cap < len || !out) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, len);
  DevBuf<float> dw, db;  // declared out here: freed after the lock and the device scope end
  DevBuf<uint8_t> dt;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DEVICE_SCOPE(c);
    if (n_weights) HIP_TRY(c, dw.alloc(n_weights));
    if (n_biases) HIP_TRY(c, db.alloc(n_biases));
    HIP_TRY(c, dt.alloc(16 * groups_of(n) + 16));
    if (n_weights) HIP_TRY(c, hipMemcpyAsync(dw, weights, n_weights * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (n_biases) HIP_TRY(c, hipMemcpyAsync(db, biases, n_biases * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, fleet::launch_encode_model_params(dw, (int64_t)n_weights, db, (int64_t)n_biases,
                                                 n_biases ? (int64_t)graph_edges : 0, dt, c->stream));
    if (len) HIP_TRY(c, hipMemcpyAsync(out, dt, len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FLEET_OK;
}

// ------------------------------------------ SGD epilogue (descentNative)

namespace {

// Segments of network::descent(vector)'s walk over the gradients() layout
// (network.h:1185-1202): weight blocks of non-null W, bias blocks of the
// fully-connected layers. Also the layout's total length and the model sizes.
// Segments of the model step; with [vb, ve) only the parts whose gradient
// positions fall in that window of upload values (an element shard), with
// gradient offsets relative to vb.
static int descent_segments(fleet_ctx* c, const int32_t* w_sizes, const uint8_t* w_present, int n_w,
                     const int32_t* b_sizes, const uint8_t* fc_layer, int n_b, size_t* n_up, size_t* n_weights,
                     size_t* n_fc, std::vector<fleet::DescentSegs>* segs, size_t vb = 0, size_t ve = SIZE_MAX) {
  if (n_w < 0 || n_b < 0 || (n_w && (!w_sizes || !w_present)) || (n_b && (!b_sizes || !fc_layer)))
    return fail(c, FLEET_ERR_ARG, "bad descent layout arguments");
  segs->clear();
  auto add = [&](int kind, size_t g, size_t m, size_t len) {
    const size_t lo = std::max(g, vb), hi = std::min(g + len, ve);
    if (lo >= hi) return;
    m += lo - g;
    len = hi - lo;
    g = lo - vb;
    if (segs->empty() || segs->back().n == fleet::kMaxDescentSegs) {
      segs->emplace_back();
      segs->back().n = 0;
    }
    fleet::DescentSegs& d = segs->back();
    d.kind[d.n] = kind;
    d.grad_off[d.n] = (int64_t)g;
    d.model_off[d.n] = (int64_t)m;
    d.len[d.n] = (int64_t)len;
    ++d.n;
  };
  size_t idx = 1, wo = 0, bo = 0;
  for (int i = 0; i < n_w; ++i) {
    if (w_sizes[i] < 0) return fail(c, FLEET_ERR_ARG, "negative weight block size");
    ++idx;
    if (w_present[i] && w_sizes[i] > 0) add(0, idx, wo, (size_t)w_sizes[i]);
    if (w_present[i]) wo += (size_t)w_sizes[i];
    idx += (size_t)w_sizes[i];
  }
  ++idx;
  for (int k = 0; k < n_b; ++k) {
    if (b_sizes[k] < 0) return fail(c, FLEET_ERR_ARG, "negative bias block size");
    ++idx;
    if (fc_layer[k] && b_sizes[k] > 0) add(1, idx, bo, (size_t)b_sizes[k]);
    if (fc_layer[k]) bo += (size_t)b_sizes[k];
    idx += (size_t)b_sizes[k];
  }
  *n_up = idx;
  *n_weights = wo;
  *n_fc = bo;
  return FLEET_OK;
}

}  // namespace

int fleet_descent_device(fleet_ctx* c, float* d_weights, float* d_fc_bias, const float* d_grad,
                         const int32_t* w_sizes, const uint8_t* w_present, int n_w, const int32_t* b_sizes,
                         const uint8_t* fc_layer, int n_b, float lr, void* stream) {
  if (!c || !d_grad) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  if (rc) return rc;
  if ((nw && !d_weights) || (nf && !d_fc_bias)) return FLEET_ERR_ARG;
  for (const auto& sg : segs)
    HIP_TRY(c, fleet::launch_descent(d_weights, d_fc_bias, d_grad, sg, lr, pick(c, stream)));
  return FLEET_OK;
}

int fleet_descent_window_device(fleet_ctx* c, float* d_weights, float* d_fc_bias, const float* d_grad_window,
                                size_t value_begin, size_t value_end, const int32_t* w_sizes,
                                const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer,
                                int n_b, float lr, void* stream) {
  if (!c || !d_grad_window || value_end < value_begin) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs, value_begin,
                            value_end);
  if (rc) return rc;
  if ((nw && !d_weights) || (nf && !d_fc_bias)) return FLEET_ERR_ARG;
  for (const auto& sg : segs)
    HIP_TRY(c, fleet::launch_descent(d_weights, d_fc_bias, d_grad_window, sg, lr, pick(c, stream)));
  return FLEET_OK;
}

int fleet_descent(fleet_ctx* c, float* weights, size_t n_weights, float* fc_bias, size_t n_fc_bias,
                  const float* grad, size_t n_grad, const int32_t* w_sizes, const uint8_t* w_present, int n_w,
                  const int32_t* b_sizes, const uint8_t* fc_layer, int n_b, float lr) {
  if (!c || !grad) return FLEET_ERR_ARG;
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  }
  if (rc) return rc;
  if (n_grad != n_up || n_weights != nw || n_fc_bias != nf || (nw && !weights) || (nf && !fc_bias))
    return fail(c, FLEET_ERR_ARG, "descent: sizes do not match the layout (grad %zu/%zu, weights %zu/%zu, bias %zu/%zu)",
                n_grad, n_up, n_weights, nw, n_fc_bias, nf);
  // the header floats network::descent(vector) reads its block sizes from
  size_t idx = 0;
  bool ok = grad[idx++] == (float)n_w;
  for (int i = 0; i < n_w && ok; ++i) {
    ok = grad[idx++] == (float)w_sizes[i];
    idx += (size_t)w_sizes[i];
  }
  ok = ok && grad[idx++] == (float)n_b;
  for (int k = 0; k < n_b && ok; ++k) {
    ok = grad[idx++] == (float)b_sizes[k];
    idx += (size_t)b_sizes[k];
  }
  if (!ok) return fail(c, FLEET_ERR_LAYOUT, "descent: gradient header does not match the model layout");
  DevBuf<float> dw, db, dg;  // freed after the lock and the device scope end
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DEVICE_SCOPE(c);
    if (nw) HIP_TRY(c, dw.alloc(nw));
    if (nf) HIP_TRY(c, db.alloc(nf));
    HIP_TRY(c, dg.alloc(n_grad));
    if (nw) HIP_TRY(c, hipMemcpyAsync(dw, weights, nw * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(db, fc_bias, nf * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dg, grad, n_grad * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (const auto& sg : segs) HIP_TRY(c, fleet::launch_descent(dw, db, dg, sg, lr, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(weights, dw, nw * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(fc_bias, db, nf * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FLEET_OK;
}

// The same step under the reference's other solvers (solver_kernels.hip, solver_math.h)

int fleet_solver_from_name(const char* name) {
  if (!name) return -1;
  static const char* const names[] = {"sgd", "adagrad", "rmsprop", "adam"};  // new_solver (solver.h:198-208)
  for (int i = 0; i < 4; ++i)
    if (!std::strcmp(name, names[i])) return i;
  return -1;
}

namespace {
static int solver_args(fleet_ctx* c, int solver, const void* g1, const void* g2, size_t nw) {
  if (solver < FLEET_SOLVER_SGD || solver > FLEET_SOLVER_ADAM) return fail(c, FLEET_ERR_ARG, "no solver %d", solver);
  if (nw && ((solver != FLEET_SOLVER_SGD && !g1) || (solver == FLEET_SOLVER_ADAM && !g2)))
    return fail(c, FLEET_ERR_ARG, "descent: solver %d needs its state row%s", solver,
                solver == FLEET_SOLVER_ADAM ? "s g1 and g2" : " g1");
  return FLEET_OK;
}
}  // namespace

int fleet_descent_solver_device(fleet_ctx* c, int solver, float* d_weights, float* d_g1, float* d_g2,
                                float* d_fc_bias, const float* d_grad, const int32_t* w_sizes,
                                const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer,
                                int n_b, float lr, void* stream) {
  if (!c || !d_grad) return FLEET_ERR_ARG;
  if (solver == FLEET_SOLVER_SGD)
    return fleet_descent_device(c, d_weights, d_fc_bias, d_grad, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, lr,
                                stream);
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  if (rc) return rc;
  if ((nw && !d_weights) || (nf && !d_fc_bias)) return FLEET_ERR_ARG;
  if ((rc = solver_args(c, solver, d_g1, d_g2, nw))) return rc;
  float b1_t, b2_t;  // a fresh solver's
  fleet::adam_bias_terms(0, &b1_t, &b2_t);
  for (const auto& sg : segs)
    HIP_TRY(c, fleet::launch_descent_solver(solver, d_weights, d_g1, d_g2, d_fc_bias, d_grad, sg, lr, b1_t, b2_t,
                                            pick(c, stream)));
  return FLEET_OK;
}

int fleet_descent_solver(fleet_ctx* c, int solver, float* weights, size_t n_weights, float* g1, float* g2,
                         float* fc_bias, size_t n_fc_bias, const float* grad, size_t n_grad, const int32_t* w_sizes,
                         const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer, int n_b,
                         float lr) {
  return fleet::descent_solver_host(c, solver, 0, weights, n_weights, g1, g2, fc_bias, n_fc_bias, grad, n_grad, w_sizes,
                                    w_present, n_w, b_sizes, fc_layer, n_b, lr);
}

}  // extern "C"

// fleet_descent_solver with adam's b1_t, b2_t after `adam_resets` resets (solver_host.h)
int fleet::descent_solver_host(fleet_ctx* c, int solver, int adam_resets, float* weights, size_t n_weights, float* g1,
                               float* g2, float* fc_bias, size_t n_fc_bias, const float* grad, size_t n_grad,
                               const int32_t* w_sizes, const uint8_t* w_present, int n_w, const int32_t* b_sizes,
                               const uint8_t* fc_layer, int n_b, float lr) {
  if (!c || !grad) return FLEET_ERR_ARG;
  if (solver == FLEET_SOLVER_SGD)
    return fleet_descent(c, weights, n_weights, fc_bias, n_fc_bias, grad, n_grad, w_sizes, w_present, n_w, b_sizes,
                         fc_layer, n_b, lr);
  size_t n_up = 0, nw = 0, nf = 0;
  std::vector<fleet::DescentSegs> segs;
  int rc;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    rc = descent_segments(c, w_sizes, w_present, n_w, b_sizes, fc_layer, n_b, &n_up, &nw, &nf, &segs);
  }
  if (rc) return rc;
  if (n_grad != n_up || n_weights != nw || n_fc_bias != nf || (nw && !weights) || (nf && !fc_bias))
    return fail(c, FLEET_ERR_ARG, "descent: sizes do not match the layout (grad %zu/%zu, weights %zu/%zu, bias %zu/%zu)",
                n_grad, n_up, n_weights, nw, n_fc_bias, nf);
  if ((rc = solver_args(c, solver, g1, g2, nw))) return rc;
  size_t idx = 0;  // fleet_descent's header check
  bool ok = grad[idx++] == (float)n_w;
  for (int i = 0; i < n_w && ok; ++i) {
    ok = grad[idx++] == (float)w_sizes[i];
    idx += (size_t)w_sizes[i];
  }
  ok = ok && grad[idx++] == (float)n_b;
  for (int k = 0; k < n_b && ok; ++k) {
    ok = grad[idx++] == (float)b_sizes[k];
    idx += (size_t)b_sizes[k];
  }
  if (!ok) return fail(c, FLEET_ERR_LAYOUT, "descent: gradient header does not match the model layout");
  const bool two = solver == FLEET_SOLVER_ADAM;
  float b1_t, b2_t;
  fleet::adam_bias_terms(adam_resets, &b1_t, &b2_t);
  DevBuf<float> dw, d1, d2, db, dg;  // freed after the lock and the device scope end
  {
    std::lock_guard<std::mutex> lk(c->mu);
    DEVICE_SCOPE(c);
    const size_t wb = nw * sizeof(float);
    if (nw) HIP_TRY(c, dw.alloc(nw));
    if (nw) HIP_TRY(c, d1.alloc(nw));
    if (nw && two) HIP_TRY(c, d2.alloc(nw));
    if (nf) HIP_TRY(c, db.alloc(nf));
    HIP_TRY(c, dg.alloc(n_grad));
    if (nw) HIP_TRY(c, hipMemcpyAsync(dw, weights, wb, hipMemcpyHostToDevice, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(d1, g1, wb, hipMemcpyHostToDevice, c->stream));
    if (nw && two) HIP_TRY(c, hipMemcpyAsync(d2, g2, wb, hipMemcpyHostToDevice, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(db, fc_bias, nf * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dg, grad, n_grad * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (const auto& sg : segs)
      HIP_TRY(c, fleet::launch_descent_solver(solver, dw, d1, d2, db, dg, sg, lr, b1_t, b2_t, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(weights, dw, wb, hipMemcpyDeviceToHost, c->stream));
    if (nw) HIP_TRY(c, hipMemcpyAsync(g1, d1, wb, hipMemcpyDeviceToHost, c->stream));
    if (nw && two) HIP_TRY(c, hipMemcpyAsync(g2, d2, wb, hipMemcpyDeviceToHost, c->stream));
    if (nf) HIP_TRY(c, hipMemcpyAsync(fc_bias, db, nf * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FLEET_OK;
}

extern "C" {

// descentNative's model copy in DISTILLATION_MODE=1 (cppNN_backend.cpp:355-372):
// cnnNew->read(cnn.getParams()) of the unquantised model. getParams prints the
// biases and the first-occurrence dictionary values with `ostream << float`
// (precision 6 = %g) and read() parses them back (strtof); every weight takes
// its dictionary entry's value. All on the device: the dictionary (sort-based,
// no O(n*U) scans), the %g / strtof round trip of the U values and the biases
// (decimal6.h: exact integer arithmetic, checked against libc on every finite
// binary32, digest fn 22) and the gather; no host round trip of the values.
int fleet_model_version(fleet_ctx* c, const float* weights, const int32_t* dims, int n_mats, const float* biases,
                        size_t n_biases, float* weights_out, float* biases_out) {
  if (!c || (n_biases && (!biases || !biases_out))) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  size_t n = 0;
  int rc = model_total(c, dims, n_mats, &n);
  if (rc) return rc;
  if (n && (!weights || !weights_out)) return FLEET_ERR_ARG;
  DevBuf<float> dw, dd, db;
  DevBuf<int32_t> di;
  // the biases' text round trip on the device as well (getParams prints them with `<<` too)
  if (n_biases) {
    HIP_TRY(c, db.alloc(n_biases));
    HIP_TRY(c, hipMemcpyAsync(db, biases, n_biases * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
    HIP_TRY(c, fleet::model_g6_inplace(db, (int64_t)n_biases, c->d_err, c->stream));
    HIP_TRY(c, hipMemcpyAsync(biases_out, db, n_biases * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (*c->h_err) {
      HIP_TRY(c, hipMemset(c->d_err, 0, sizeof(int)));
      return fail(c, FLEET_ERR_ARG, "non-finite bias: the reference's text read fails");
    }
  }
  if (!n) return FLEET_OK;
  HIP_TRY(c, dw.alloc(n));
  HIP_TRY(c, dd.alloc(n + 1));
  HIP_TRY(c, di.alloc(n));
  HIP_TRY(c, hipMemcpyAsync(dw, weights, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  int32_t U = 0;
  HIP_TRY(c, fleet::model_quantize_index(dw, dims, n_mats, nullptr, dd, di, &U, c->stream, false));
  // the U dictionary values through `<<` / `>>` (decimal6.h), in place, then the gather
  HIP_TRY(c, hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
  HIP_TRY(c, fleet::model_g6_inplace(dd, (int64_t)U, c->d_err, c->stream));
  HIP_TRY(c, fleet::model_dict_gather(di, (int64_t)n, dd, dw, c->stream));
  HIP_TRY(c, hipMemcpyAsync(weights_out, dw, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*c->h_err) {
    HIP_TRY(c, hipMemset(c->d_err, 0, sizeof(int)));
    return fail(c, FLEET_ERR_ARG, "non-finite weight: the reference's text read fails");
  }
  return FLEET_OK;
}

// ------------------------------------------------------ streaming aggregation

// (static: a helper in an unnamed namespace inside this file's extern "C" block still gets
// an unmangled dynamic symbol, and a name such as OpenACC's acc_free, which the OpenMP
// runtime torch loads exports, would then be called in its place)
namespace {

constexpr size_t kAccPiece = 1 << 20;  // host rows: copy and DMA overlap in pieces

// The part of an upload that an accumulator or a pool keeps: the groups [gb, ge) of
// uploads of `len` characters (n values), bytes [col0, col0 + width) of the text. Rows
// and state on the device hold the window alone; merged outputs are addressed by the
// whole upload (kernels.h).
struct FLEET_MEM_LOCAL Window {
  size_t len = 0, n = 0, gb = 0, ge = 0, ng = 0, col0 = 0, width = 0;
  int n_hdr = 0;
  DevBuf<int32_t> d_hdr;     // {0, count, walk_end, 0, positions}
  DevBuf<int32_t> d_hfirst;  // the batch's first upload's header codes
  size_t row_bytes() const { return 16 * ng + 64; }
  size_t state_bytes() const { return sizeof(float) * 3 * ng + 64; }
  fleet::AccWindow launch() const { return {(int64_t)n, (int64_t)gb, (int64_t)ge, d_hdr, d_hfirst}; }
};

// Checks the arguments that describe the window (the entry points made the bare
// FLEET_ERR_ARG checks), fills the geometry, allocates d_hfirst and uploads the header
// block. A failed allocation returns FLEET_ERR_NOMEM with the geometry filled and no
// message: the caller's names what it was creating.
static int window_open(fleet_ctx* c, size_t len, const int32_t* header_pos, int n_headers, size_t group_begin,
                       size_t group_end, Window* w) {
  int rc = check_text_len(c, len);
  if (rc) return rc;
  const size_t n = fleet_b64_count(len), groups = groups_of(n);
  if (16 * groups + 16 >= ((size_t)1 << 31)) return fail(c, FLEET_ERR_ARG, "upload of %zu bytes: 2 GiB or more", len);
  if (group_end > groups) group_end = groups;
  if (group_begin > group_end) return fail(c, FLEET_ERR_ARG, "group window [%zu, %zu) is empty or reversed", group_begin, group_end);
  if ((rc = check_header_positions(c, header_pos, n_headers, n))) return rc;
  w->len = len, w->n = n, w->n_hdr = n_headers;
  w->gb = group_begin, w->ge = group_end, w->ng = group_end - group_begin;
  w->col0 = 16 * w->gb;
  w->width = w->ng ? std::min(len, 16 * w->ge) - w->col0 : 0;
  // walk_end = n: the caller's layout covers the whole upload (as fleet_update_device)
  std::vector<int32_t> hw{0, n_headers, (int32_t)n, 0};
  if (n_headers) hw.insert(hw.end(), header_pos, header_pos + n_headers);
  if (w->d_hdr.alloc(hw.size()) != hipSuccess || w->d_hfirst.alloc((size_t)n_headers + 16) != hipSuccess ||
      hipMemcpy(w->d_hdr, hw.data(), sizeof(int32_t) * hw.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    w->d_hdr.reset();
    w->d_hfirst.reset();
    return FLEET_ERR_NOMEM;
  }
  return FLEET_OK;
}

// `whose`: "the accumulator's", "the pool's"
static int window_len_arg(fleet_ctx* c, const Window& w, size_t len, const char* whose) {
  if (len != w.len) return fail(c, FLEET_ERR_ARG, "upload has length %zu, %s is %zu", len, whose, w.len);
  return FLEET_OK;
}

// An upload's window from host memory to the device row `d` through the pinned row `h`,
// in pieces on `s`. Bytes past `len` in a row's last group stay zero: the copy stops at len.
static int window_copy_in(fleet_ctx* c, const Window& w, const char* upload, uint8_t* h, uint8_t* d, hipStream_t s) {
  for (size_t o = 0; o < w.width; o += kAccPiece) {
    const size_t m = std::min(kAccPiece, w.width - o);
    std::memcpy(h + o, upload + w.col0 + o, m);
    HIP_TRY(c, hipMemcpyAsync(d + o, h + o, m, hipMemcpyHostToDevice, s));
  }
  return FLEET_OK;
}

// A host finish's outputs from the spare device buffers that hold them, d_out and d_f32,
// to the caller's buffers on `s`. The two hold the window alone: the kernel, which
// addresses its outputs by the whole upload's group index, was given them shifted back
// by the window's start.
static int window_read_back(fleet_ctx* c, const Window& w, const uint8_t* d_out, const float* d_f32, char* merged,
                            float* merged_f32, hipStream_t s) {
  const size_t v0 = 3 * w.gb, v1 = std::max(v0, std::min(w.n, 3 * w.ge));
  if (w.width) HIP_TRY(c, hipMemcpyAsync(merged + w.col0, d_out, w.width, hipMemcpyDeviceToHost, s));
  if (merged_f32 && v1 > v0)
    HIP_TRY(c, hipMemcpyAsync(merged_f32 + v0, d_f32, sizeof(float) * (v1 - v0), hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// Device-side calls still in flight on the caller's stream.
struct InFlight {
  bool pending = false;
  hipStream_t stream = nullptr;
  void on(hipStream_t s) { pending = true, stream = s; }
  void done() { pending = false; }  // the caller synchronised `stream` itself
};

// Waits for them, unless they run on `same`, which orders the caller's next work itself.
static int settle(fleet_ctx* c, InFlight* f, hipStream_t same, bool wait) {
  if (f->pending && (wait || f->stream != same)) {
    HIP_TRY(c, hipStreamSynchronize(f->stream));
    f->done();
  }
  return FLEET_OK;
}

}  // namespace

// One upload folded into a resident sum per call (acc_kernels.hip). The buffers come
// in pairs: state[cur] holds the sum and the step writes state[cur ^ 1]; row[last]
// holds the last accepted upload's window (the merge keeps its header codes) and the
// incoming upload lands in row[last ^ 1]. A host push flips the two indices only after
// its error word came back clean. The host finish borrows the two spare buffers for its
// outputs (the next push overwrites both), so the accumulator holds nothing else.
struct FLEET_MEM_LOCAL fleet_acc {
  fleet_ctx* c = nullptr;
  Window w;
  DevBuf<float> d_state[2];
  DevBuf<uint8_t> d_row[2];
  PinBuf<uint8_t> h_row[2];
  DevBuf<int> d_err;
  PinBuf<volatile int> h_err;              // [0] synchronous reads, [1] written back after device pushes
  int cur = 0, last = 0, count = 0;
  int sticky = 0;                          // a device push's error, until fleet_acc_reset
  InFlight fly;                            // device pushes
  // host bursts: rows 0..K-2 of a launch, window bytes at stage_pitch apart; grown on
  // demand to at most kAccBurst rows and kept until fleet_acc_destroy
  DevBuf<uint8_t> d_stage;  // both freed on growth, after the context's stream was waited for
  PinBuf<uint8_t> h_stage;
  size_t stage_rows = 0, stage_pitch = 0;
};

namespace {

static int acc_code(fleet_ctx* c, int e) {
  if (e & FLEET_ERRBIT_BASE64) return fail(c, FLEET_ERR_BASE64, "input is not Base64::encode output (alphabet/padding)");
  if (e & FLEET_ERRBIT_LAYOUT)
    return fail(c, FLEET_ERR_LAYOUT, "upload's layout header slots differ from the batch's first upload");
  return FLEET_OK;
}

static int acc_sticky(fleet_acc* a) {
  if (a->sticky == FLEET_ERR_BASE64) return acc_code(a->c, FLEET_ERRBIT_BASE64);
  return acc_code(a->c, FLEET_ERRBIT_LAYOUT);
}

// Settles the device pushes in flight and turns an error they wrote back into the sticky one.
static int acc_settle(fleet_acc* a, hipStream_t same, bool wait) {
  const int rc = settle(a->c, &a->fly, same, wait);
  if (rc) return rc;
  const int e = a->h_err[1];
  if (e && !a->sticky) a->sticky = (e & FLEET_ERRBIT_BASE64) ? FLEET_ERR_BASE64 : FLEET_ERR_LAYOUT;
  return a->sticky ? acc_sticky(a) : FLEET_OK;
}

static int acc_clear_err(fleet_acc* a, hipStream_t s) {
  HIP_TRY(a->c, hipMemsetAsync(a->d_err, 0, sizeof(int), s));
  HIP_TRY(a->c, hipStreamSynchronize(s));
  a->h_err[0] = 0;
  a->h_err[1] = 0;
  return FLEET_OK;
}

// the error word of the steps just enqueued on `s`, read synchronously; an error
// leaves nothing committed
static int acc_verdict(fleet_acc* a, hipStream_t s) {
  fleet_ctx* c = a->c;
  HIP_TRY(c, hipMemcpyAsync((void*)a->h_err.get(), a->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const int e = a->h_err[0];
  if (e) {
    const int rc = acc_clear_err(a, s);
    return rc ? rc : acc_code(c, e);
  }
  return FLEET_OK;
}

}  // namespace

int fleet_acc_create(fleet_ctx* c, size_t len, const int32_t* header_pos, int n_headers, size_t group_begin,
                     size_t group_end, fleet_acc** out) {
  if (!c || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (len == 0 || n_headers < 0 || n_headers > FLEET_MAX_HEADERS || (n_headers && !header_pos)) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  Window w;
  const int rc = window_open(c, len, header_pos, n_headers, group_begin, group_end, &w);
  if (rc == FLEET_ERR_NOMEM)
    return fail(c, FLEET_ERR_NOMEM, "fleet_acc_create: allocating the accumulator of %zu groups failed", w.ng);
  if (rc) return rc;
  fleet_acc* a = new fleet_acc();
  a->c = c;
  a->w = std::move(w);
  const size_t ng = a->w.ng, row_bytes = a->w.row_bytes(), st_bytes = a->w.state_bytes();
  bool ok = true;
  for (int i = 0; i < 2 && ok; ++i) {
    ok = a->d_state[i].alloc(3 * ng, 64) == hipSuccess && a->d_row[i].alloc(row_bytes) == hipSuccess &&
         a->h_row[i].alloc(row_bytes) == hipSuccess;
    // bytes past `len` in a row's last group stay zero: the uploads' copies stop at len
    if (ok) std::memset(a->h_row[i], 0, row_bytes);
    ok = ok && hipMemset(a->d_row[i], 0, row_bytes) == hipSuccess && hipMemset(a->d_state[i], 0, st_bytes) == hipSuccess;
  }
  ok = ok && a->d_err.alloc_zero(16) == hipSuccess && a->h_err.alloc(16) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete a;
    return fail(c, FLEET_ERR_NOMEM, "fleet_acc_create: allocating the accumulator of %zu groups failed", ng);
  }
  a->h_err[0] = 0;
  a->h_err[1] = 0;
  *out = a;
  return FLEET_OK;
}

void fleet_acc_destroy(fleet_acc* a) {
  if (!a) return;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)settle(c, &a->fly, nullptr, true);
  (void)hipStreamSynchronize(c->stream);
  delete a;
}

int fleet_acc_count(const fleet_acc* a) { return a ? a->count : FLEET_ERR_ARG; }

int fleet_acc_push(fleet_acc* a, const char* upload, size_t len, double dampen) {
  if (!a || !upload) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = window_len_arg(c, a->w, len, "the accumulator's");
  if (rc) return rc;
  if ((rc = acc_settle(a, c->stream, true))) return rc;
  const int spare = a->last ^ 1;
  if ((rc = window_copy_in(c, a->w, upload, a->h_row[spare], a->d_row[spare], c->stream))) return rc;
  HIP_TRY(c, fleet::launch_acc_push(a->d_row[spare], a->d_state[a->cur], a->d_state[a->cur ^ 1], a->count == 0, dampen,
                                    a->w.launch(), a->d_err, c->stream));
  if ((rc = acc_verdict(a, c->stream))) return rc;  // rejected: state[cur], row[last] and the count are as before
  a->cur ^= 1;
  a->last = spare;
  ++a->count;
  return FLEET_OK;
}

int fleet_acc_push_device(fleet_acc* a, const void* d_upload, double dampen, void* stream) {
  if (!a || !d_upload) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  hipStream_t s = pick(c, stream);
  int rc = acc_settle(a, s, false);
  if (rc) return rc;
  const int spare = a->last ^ 1;
  if (a->w.width)
    HIP_TRY(c, hipMemcpyAsync(a->d_row[spare], (const uint8_t*)d_upload + a->w.col0, a->w.width, hipMemcpyDeviceToDevice, s));
  HIP_TRY(c, fleet::launch_acc_push(a->d_row[spare], a->d_state[a->cur], a->d_state[a->cur ^ 1], a->count == 0, dampen,
                                    a->w.launch(), a->d_err, s));
  HIP_TRY(c, hipMemcpyAsync((void*)(a->h_err + 1), a->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
  a->cur ^= 1;
  a->last = spare;
  ++a->count;
  a->fly.on(s);
  return FLEET_OK;
}

int fleet_acc_finish(fleet_acc* a, char* merged, size_t cap, size_t* out_len, float* merged_f32) {
  if (!a || !merged) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = acc_settle(a, c->stream, true);
  if (rc) return rc;
  if (a->count == 0) return fail(c, FLEET_ERR_ARG, "fleet_acc_finish: nothing was pushed");
  if (out_len) *out_len = a->w.len;
  if (cap < a->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, a->w.len);
  uint8_t* d_out = a->d_row[a->last ^ 1];  // the spare row and the spare state
  float* d_f32 = a->d_state[a->cur ^ 1];
  HIP_TRY(c, fleet::launch_acc_finish(a->d_row[a->last], a->d_state[a->cur], (double)1 / a->count, a->w.launch(),
                                      d_out - a->w.col0, merged_f32 ? d_f32 - 3 * a->w.gb : nullptr, c->stream));
  if ((rc = window_read_back(c, a->w, d_out, d_f32, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  a->count = 0;
  return FLEET_OK;
}

int fleet_acc_finish_device(fleet_acc* a, void* d_merged, void* d_merged_f32, void* stream) {
  if (!a || !d_merged) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  hipStream_t s = pick(c, stream);
  int rc = acc_settle(a, s, false);
  if (rc) return rc;
  if (a->count == 0) return fail(c, FLEET_ERR_ARG, "fleet_acc_finish_device: nothing was pushed");
  HIP_TRY(c, fleet::launch_acc_finish(a->d_row[a->last], a->d_state[a->cur], (double)1 / a->count, a->w.launch(),
                                      (uint8_t*)d_merged, (float*)d_merged_f32, s));
  HIP_TRY(c, hipMemcpyAsync((void*)(a->h_err + 1), a->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  a->fly.done();
  if ((rc = acc_settle(a, s, false))) return rc;  // a device push of this batch was malformed
  a->count = 0;
  return FLEET_OK;
}

// --- bursts: K uploads per call, kAccBurst per launch (k_acc_push_many)

namespace {

static int acc_stage_reserve(fleet_acc* a, size_t rows) {
  fleet_ctx* c = a->c;
  if (rows <= a->stage_rows || a->w.ng == 0) return FLEET_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  a->d_stage.reset();
  a->h_stage.reset();
  a->stage_rows = 0;
  a->stage_pitch = a->w.row_bytes();
  const size_t bytes = rows * a->stage_pitch;
  if (a->d_stage.alloc(bytes) != hipSuccess || a->h_stage.alloc(bytes) != hipSuccess ||
      hipMemsetAsync(a->d_stage, 0, bytes, c->stream) != hipSuccess) {  // on the stream the rows' copies follow on
    (void)hipGetLastError();
    a->d_stage.reset();
    a->h_stage.reset();
    return fail(c, FLEET_ERR_NOMEM, "burst staging of %zu rows of %zu bytes failed", rows, a->stage_pitch);
  }
  std::memset(a->h_stage, 0, bytes);  // as the rows of fleet_acc_create
  a->stage_rows = rows;
  return FLEET_OK;
}

// Enqueues the burst's copies and launches on `s` and commits nothing: the steps go
// from state[cur] into state[cur ^ 1] (a burst longer than kAccBurst: the first launch
// reads state[cur], the later ones read and write state[cur ^ 1] in place), row K-1
// lands in the spare row. Host rows (`uploads`) go through the staging; device rows
// (`d_rows`: the window's first byte of row 0, `pitch` apart) are read in place. With
// `finish` the last launch is the finish form, writing d_merged / d_f32.
static int acc_fold(fleet_acc* a, const char* const* uploads, const uint8_t* d_rows, size_t pitch, int K,
                    const double* dampen, hipStream_t s, bool finish, uint8_t* d_merged, float* d_f32) {
  fleet_ctx* c = a->c;
  if (a->w.ng == 0) return FLEET_OK;
  constexpr int B = fleet::kAccBurst;
  const int spare = a->last ^ 1;
  int rc;
  // a launch's rows but the burst's last one, which goes to the spare row
  if (uploads && (rc = acc_stage_reserve(a, (size_t)(K > B ? B : K - 1)))) return rc;
  const double inv = (double)1 / (a->count + K);
  for (int k0 = 0; k0 < K; k0 += B) {
    const int kc = std::min(B, K - k0);
    const bool last_chunk = k0 + kc == K;
    const uint8_t *rows, *last_row;
    size_t rp;
    if (uploads) {
      if (k0) HIP_TRY(c, hipStreamSynchronize(s));  // the pinned staging is read by the previous chunk's copies
      for (int k = 0; k < kc; ++k) {
        const bool to_spare = last_chunk && k == kc - 1;
        uint8_t* h = to_spare ? a->h_row[spare] : a->h_stage + (size_t)k * a->stage_pitch;
        uint8_t* d = to_spare ? a->d_row[spare] : a->d_stage + (size_t)k * a->stage_pitch;
        if ((rc = window_copy_in(c, a->w, uploads[k0 + k], h, d, s))) return rc;
      }
      rows = a->d_stage;
      rp = a->stage_pitch;
    } else {
      rows = d_rows + (size_t)k0 * pitch;
      rp = pitch;
      if (last_chunk)
        HIP_TRY(c, hipMemcpyAsync(a->d_row[spare], rows + (size_t)(kc - 1) * pitch, a->w.width, hipMemcpyDeviceToDevice, s));
    }
    last_row = last_chunk ? a->d_row[spare] : rows + (size_t)(kc - 1) * rp;
    const bool fin = finish && last_chunk;
    HIP_TRY(c, fleet::launch_acc_push_many(rows, rp, last_row, a->d_state[k0 ? a->cur ^ 1 : a->cur], a->d_state[a->cur ^ 1],
                                           k0 == 0 && a->count == 0, kc, dampen + k0, fin, inv, a->w.launch(), a->d_err,
                                           fin ? d_merged : nullptr, fin ? d_f32 : nullptr, s));
  }
  return FLEET_OK;
}

static int acc_host_args(fleet_acc* a, const char* const* uploads, const size_t* lens, int K, const char* what) {
  for (int k = 0; k < K; ++k) {
    if (!uploads[k]) return fail(a->c, FLEET_ERR_ARG, "%s: upload %d is NULL", what, k);
    if (lens[k] != a->w.len)
      return fail(a->c, FLEET_ERR_ARG, "%s: upload %d has length %zu, the accumulator's is %zu", what, k, lens[k], a->w.len);
  }
  return FLEET_OK;
}

// rows 0..K-2 are read in place with 16-byte loads
static int acc_device_args(fleet_acc* a, const void* d_uploads, size_t pitch, int K, const char* what) {
  if (K > 1 && (pitch % 16 != 0 || pitch < 16 * groups_of(a->w.n) || (uintptr_t)d_uploads % 16 != 0))
    return fail(a->c, FLEET_ERR_ARG, "%s: rows must be 16-byte aligned, the pitch a multiple of 16 covering the upload's groups", what);
  return FLEET_OK;
}

}  // namespace

int fleet_acc_burst(void) { return fleet::kAccBurst; }

int fleet_acc_push_many(fleet_acc* a, const char* const* uploads, const size_t* lens, int K, const double* dampen) {
  if (!a || !uploads || !lens || !dampen || K <= 0) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = acc_host_args(a, uploads, lens, K, "fleet_acc_push_many");
  if (rc) return rc;
  if ((rc = acc_settle(a, c->stream, true))) return rc;
  if ((rc = acc_fold(a, uploads, nullptr, 0, K, dampen, c->stream, false, nullptr, nullptr))) return rc;
  if ((rc = acc_verdict(a, c->stream))) return rc;  // rejected: state[cur], row[last] and the count are as before
  a->cur ^= 1;
  a->last ^= 1;
  a->count += K;
  return FLEET_OK;
}

int fleet_acc_push_many_device(fleet_acc* a, const void* d_uploads, size_t pitch, int K, const double* dampen,
                               void* stream) {
  if (!a || !d_uploads || !dampen || K <= 0) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = acc_device_args(a, d_uploads, pitch, K, "fleet_acc_push_many_device");
  if (rc) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = acc_settle(a, s, false))) return rc;
  if ((rc = acc_fold(a, nullptr, (const uint8_t*)d_uploads + a->w.col0, pitch, K, dampen, s, false, nullptr, nullptr)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync((void*)(a->h_err + 1), a->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
  a->cur ^= 1;
  a->last ^= 1;
  a->count += K;
  a->fly.on(s);
  return FLEET_OK;
}

int fleet_acc_push_finish(fleet_acc* a, const char* const* uploads, const size_t* lens, int K, const double* dampen,
                          char* merged, size_t cap, size_t* out_len, float* merged_f32) {
  if (!a || !uploads || !lens || !dampen || !merged || K <= 0) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = acc_host_args(a, uploads, lens, K, "fleet_acc_push_finish");
  if (rc) return rc;
  if ((rc = acc_settle(a, c->stream, true))) return rc;
  if (out_len) *out_len = a->w.len;
  if (cap < a->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, a->w.len);
  uint8_t* d_out = a->d_row[a->last ^ 1];  // over row K-1, which the lane has read by then
  float* d_f32 = a->d_state[a->cur ^ 1];
  if ((rc = acc_fold(a, uploads, nullptr, 0, K, dampen, c->stream, true, d_out - a->w.col0,
                     merged_f32 ? d_f32 - 3 * a->w.gb : nullptr)))
    return rc;
  if ((rc = window_read_back(c, a->w, d_out, d_f32, merged, merged_f32, c->stream))) return rc;
  if ((rc = acc_verdict(a, c->stream))) return rc;  // rejected: nothing committed (the outputs are not meaningful)
  a->count = 0;
  return FLEET_OK;
}

int fleet_acc_push_finish_device(fleet_acc* a, const void* d_uploads, size_t pitch, int K, const double* dampen,
                                 void* d_merged, void* d_merged_f32, void* stream) {
  if (!a || !d_uploads || !dampen || !d_merged || K <= 0) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = acc_device_args(a, d_uploads, pitch, K, "fleet_acc_push_finish_device");
  if (rc) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = acc_settle(a, s, false))) return rc;
  if ((rc = acc_fold(a, nullptr, (const uint8_t*)d_uploads + a->w.col0, pitch, K, dampen, s, true, (uint8_t*)d_merged,
                     (float*)d_merged_f32)))
    return rc;
  // device pushes of this batch still in flight are on `s` and wrote their error word
  // back before this burst ran: theirs is sticky and comes first, the burst's own is not
  HIP_TRY(c, hipMemcpyAsync((void*)a->h_err.get(), a->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  a->fly.done();
  if ((rc = acc_settle(a, s, false))) return rc;
  const int e = a->h_err[0];
  if (e) {
    rc = acc_clear_err(a, s);
    return rc ? rc : acc_code(c, e);
  }
  a->count = 0;
  return FLEET_OK;
}

int fleet_acc_reset(fleet_acc* a) {
  if (!a) return FLEET_ERR_ARG;
  fleet_ctx* c = a->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = settle(c, &a->fly, nullptr, true);
  if (rc || (rc = acc_clear_err(a, c->stream))) return rc;
  a->sticky = 0;
  a->count = 0;
  return FLEET_OK;
}

// ---------------------------------------------------------------- upload pool

// The reference's `acc` for staleSize > 0 (CppNNUpdater.java:394-407) kept in HBM: uploads
// go into slots when they arrive, an update folds any subset of the slots in any order
// (k_pool_fold) and leaves every slot as it was. d_rows holds slots + 1 rows of the
// window's bytes: row `slots` receives the host update's merged bytes, whose fp32 go over
// the state (the finish launch reads a lane's 12 bytes before it writes them).
struct FLEET_MEM_LOCAL fleet_pool {
  fleet_ctx* c = nullptr;
  Window w;
  size_t pitch = 0;
  int slots = 0;
  DevBuf<uint8_t> d_rows;
  DevBuf<float> d_state;   // the running value between the launches of an update of more than kAccBurst picks
  DevBuf<int> d_status;    // one error word per slot, cleared by every update
  PinBuf<int> h_status;    // what the last update left in d_status
  PinBuf<uint8_t> h_row;   // a host put's way in
  std::vector<uint8_t> occupied;
  std::vector<uint8_t> seen;  // update: the picks so far
  InFlight fly;               // device puts
};

namespace {

static int pool_slot_arg(fleet_pool* p, int slot, const char* what) {
  if (slot < 0 || slot >= p->slots) return fail(p->c, FLEET_ERR_ARG, "%s: slot %d outside [0, %d)", what, slot, p->slots);
  return FLEET_OK;
}

// FLEET_ERR_ARG before anything is launched: a pick outside the pool, of an empty slot, or repeated
static int pool_update_args(fleet_pool* p, const int32_t* picks, int K, const char* what) {
  std::fill(p->seen.begin(), p->seen.end(), 0);
  for (int k = 0; k < K; ++k) {
    const int rc = pool_slot_arg(p, picks[k], what);
    if (rc) return rc;
    if (!p->occupied[picks[k]]) return fail(p->c, FLEET_ERR_ARG, "%s: pick %d names slot %d, which holds no upload", what, k, picks[k]);
    if (p->seen[picks[k]]) return fail(p->c, FLEET_ERR_ARG, "%s: slot %d is picked twice", what, picks[k]);
    p->seen[picks[k]] = 1;
  }
  return FLEET_OK;
}

// Enqueues an update on `s`: status[] cleared, the picks folded kAccBurst per launch (the
// last launch the finish form), status[] copied back. Nothing in the pool but the state,
// hfirst[] and status[] is written.
static int pool_fold(fleet_pool* p, const int32_t* picks, int K, const double* dampen, hipStream_t s, uint8_t* d_merged,
                     float* d_f32) {
  fleet_ctx* c = p->c;
  constexpr int B = fleet::kAccBurst;
  HIP_TRY(c, hipMemsetAsync(p->d_status, 0, sizeof(int) * (size_t)p->slots, s));
  for (int k0 = 0; k0 < K; k0 += B) {
    const int kc = std::min(B, K - k0);
    HIP_TRY(c, fleet::launch_pool_fold(p->d_rows, p->pitch, picks + k0, p->d_state, k0 == 0, kc, dampen + k0, k0 + kc == K,
                                       (double)1 / K, p->w.launch(), p->d_status, d_merged, d_f32, s));
  }
  HIP_TRY(c, hipMemcpyAsync(p->h_status, p->d_status, sizeof(int) * (size_t)p->slots, hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// after the stream was synchronised: BASE64 before LAYOUT, as acc_code
static int pool_verdict(fleet_pool* p, const int32_t* picks, int K) {
  int all = 0, bad_slot = -1, layout_slot = -1;
  for (int k = K - 1; k >= 0; --k) {
    const int e = p->h_status[picks[k]];
    all |= e;
    if (e & FLEET_ERRBIT_BASE64) bad_slot = picks[k];
    if (e & FLEET_ERRBIT_LAYOUT) layout_slot = picks[k];
  }
  if (all & FLEET_ERRBIT_BASE64)
    return fail(p->c, FLEET_ERR_BASE64, "slot %d: input is not Base64::encode output (alphabet/padding)", bad_slot);
  if (all & FLEET_ERRBIT_LAYOUT)
    return fail(p->c, FLEET_ERR_LAYOUT, "slot %d: upload's layout header slots differ from the update's first pick", layout_slot);
  return FLEET_OK;
}

}  // namespace

int fleet_pool_create(fleet_ctx* c, size_t len, const int32_t* header_pos, int n_headers, size_t group_begin,
                      size_t group_end, int slots, fleet_pool** out) {
  if (!c || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (len == 0 || n_headers < 0 || n_headers > FLEET_MAX_HEADERS || (n_headers && !header_pos) || slots < 1)
    return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  Window w;
  const int rc = window_open(c, len, header_pos, n_headers, group_begin, group_end, &w);
  if (rc == FLEET_ERR_NOMEM)
    return fail(c, FLEET_ERR_NOMEM, "fleet_pool_create: allocating %d slots of %zu groups failed", slots, w.ng);
  if (rc) return rc;
  fleet_pool* p = new fleet_pool();
  p->c = c;
  p->w = std::move(w);
  p->pitch = p->w.row_bytes();
  p->slots = slots;
  p->occupied.assign((size_t)slots, 0);
  p->seen.assign((size_t)slots, 0);
  const size_t ng = p->w.ng;
  // the rows are zeroed once: the puts' copies stop at len
  const bool ok = p->d_rows.alloc_zero(((size_t)slots + 1) * p->pitch) == hipSuccess &&
                  p->d_state.alloc_zero(3 * ng, 64) == hipSuccess &&
                  p->d_status.alloc_zero((size_t)slots) == hipSuccess &&
                  p->h_status.alloc((size_t)slots) == hipSuccess && p->h_row.alloc(p->pitch) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete p;
    return fail(c, FLEET_ERR_NOMEM, "fleet_pool_create: allocating %d slots of %zu groups failed", slots, ng);
  }
  std::memset(p->h_status, 0, sizeof(int) * (size_t)slots);
  *out = p;
  return FLEET_OK;
}

void fleet_pool_destroy(fleet_pool* p) {
  if (!p) return;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)settle(c, &p->fly, nullptr, true);
  (void)hipStreamSynchronize(c->stream);
  delete p;
}

int fleet_pool_slots(const fleet_pool* p) { return p ? p->slots : FLEET_ERR_ARG; }

int fleet_pool_occupied(const fleet_pool* p, int slot) {
  if (!p || slot < 0 || slot >= p->slots) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(p->c->mu);
  return p->occupied[slot] ? 1 : 0;
}

int fleet_pool_slot_status(const fleet_pool* p, int slot) {
  if (!p || slot < 0 || slot >= p->slots) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(p->c->mu);
  return p->h_status[slot];
}

int fleet_pool_put(fleet_pool* p, int slot, const char* upload, size_t len) {
  if (!p || !upload) return FLEET_ERR_ARG;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = pool_slot_arg(p, slot, "fleet_pool_put");
  if (rc) return rc;
  if ((rc = window_len_arg(c, p->w, len, "the pool's"))) return rc;
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  if ((rc = window_copy_in(c, p->w, upload, p->h_row, p->d_rows + (size_t)slot * p->pitch, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  p->occupied[slot] = 1;
  return FLEET_OK;
}

int fleet_pool_put_device(fleet_pool* p, int slot, const void* d_upload, void* stream) {
  if (!p || !d_upload) return FLEET_ERR_ARG;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = pool_slot_arg(p, slot, "fleet_pool_put_device");
  if (rc) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if (p->w.width)
    HIP_TRY(c, hipMemcpyAsync(p->d_rows + (size_t)slot * p->pitch, (const uint8_t*)d_upload + p->w.col0, p->w.width,
                              hipMemcpyDeviceToDevice, s));
  p->occupied[slot] = 1;
  p->fly.on(s);
  return FLEET_OK;
}

int fleet_pool_drop(fleet_pool* p, int slot) {
  if (!p) return FLEET_ERR_ARG;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  const int rc = pool_slot_arg(p, slot, "fleet_pool_drop");
  if (rc) return rc;
  p->occupied[slot] = 0;  // the bytes stay until the next put: every upload has the pool's length
  return FLEET_OK;
}

int fleet_pool_update(fleet_pool* p, const int32_t* picks, int K, const double* dampen, char* merged, size_t cap,
                      size_t* out_len, float* merged_f32) {
  if (!p || !picks || !dampen || !merged || K <= 0) return FLEET_ERR_ARG;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = pool_update_args(p, picks, K, "fleet_pool_update");
  if (rc) return rc;
  if (out_len) *out_len = p->w.len;
  if (cap < p->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, p->w.len);
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  uint8_t* d_out = p->d_rows + (size_t)p->slots * p->pitch;  // the pool's spare row; the fp32 go over the state
  if ((rc = pool_fold(p, picks, K, dampen, c->stream, d_out - p->w.col0,
                      merged_f32 ? p->d_state - 3 * p->w.gb : nullptr)))
    return rc;
  if ((rc = window_read_back(c, p->w, d_out, p->d_state, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return pool_verdict(p, picks, K);  // on an error the outputs are not meaningful; the pool is as before
}

int fleet_pool_update_device(fleet_pool* p, const int32_t* picks, int K, const double* dampen, void* d_merged,
                             void* d_merged_f32, void* stream) {
  if (!p || !picks || !dampen || !d_merged || K <= 0) return FLEET_ERR_ARG;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = pool_update_args(p, picks, K, "fleet_pool_update_device");
  if (rc) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if ((rc = pool_fold(p, picks, K, dampen, s, (uint8_t*)d_merged, (float*)d_merged_f32))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  p->fly.done();
  return pool_verdict(p, picks, K);
}

// ---------------------------------------------------------------- arrival gate

// What can be said of an upload when it arrives, beside a pool (k_pool_vet): the fold's
// Base64 verdict, the header codes against the model's, and the flat gradient's squared
// norm and largest magnitude -- new ByteVec(getFlatGradient(g)).getNorm(),
// cppNN_backend.cpp:701-720, 779-795. One launch's status words and per-wave partials
// (kAccBurst slots), and the results of a host vet of up to the pool's slots in HBM and
// pinned. The gate writes nothing of the pool's but, in fleet_gate_put, the row of a free slot.
struct FLEET_MEM_LOCAL fleet_gate {
  fleet_pool* p = nullptr;
  int cap = 0;                    // result entries: max(the pool's slots, kAccBurst)
  DevBuf<int32_t> d_expected;  // the header codes an upload must carry (empty: not checked)
  DevBuf<int> d_work;          // one launch's status words
  DevBuf<double> d_part;       // one launch's per-wave partials
  DevBuf<int32_t> d_status;
  DevBuf<double> d_sumsq;
  DevBuf<float> d_max;
  PinBuf<int32_t> h_status;
  PinBuf<double> h_sumsq;
  PinBuf<float> h_max;
};

namespace {

// the launches of a vet of K checked slots on `s`, kAccBurst slots each, into device arrays of K
static int gate_launch(fleet_gate* g, const int32_t* slots, int K, int32_t* d_status, double* d_sumsq, float* d_max,
                       hipStream_t s) {
  fleet_pool* p = g->p;
  constexpr int B = fleet::kAccBurst;
  for (int k0 = 0; k0 < K; k0 += B)
    HIP_TRY(p->c, fleet::launch_pool_vet(p->d_rows, p->pitch, slots + k0, std::min(B, K - k0), p->w.launch(), g->d_expected,
                                         g->d_work, g->d_part, d_status + k0, d_sumsq + k0, d_max + k0, s));
  return FLEET_OK;
}

// gate_launch into the gate's own arrays on the context's stream, read back and waited for
static int gate_vet_host(fleet_gate* g, const int32_t* slots, int K, int32_t* status, double* sumsq, float* max_abs) {
  fleet_ctx* c = g->p->c;
  const int rc = gate_launch(g, slots, K, g->d_status, g->d_sumsq, g->d_max, c->stream);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(g->h_status, g->d_status, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(g->h_sumsq, g->d_sumsq, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(g->h_max, g->d_max, sizeof(float) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::copy(g->h_status.get(), g->h_status + K, status);
  std::copy(g->h_sumsq.get(), g->h_sumsq + K, sumsq);
  std::copy(g->h_max.get(), g->h_max + K, max_abs);
  return FLEET_OK;
}

}  // namespace

int fleet_gate_header_codes(const float* values, int n, int32_t* codes) {
  if (n < 0 || (n && (!values || !codes))) return FLEET_ERR_ARG;
  for (int i = 0; i < n; ++i) codes[i] = fleet::enc(values[i]);  // Base64::float2int (Base64.cpp:60-73)
  return FLEET_OK;
}

int fleet_gate_create(fleet_pool* p, const int32_t* header_codes, int n_headers, fleet_gate** out) {
  if (!p || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (header_codes && n_headers != p->w.n_hdr)
    return fail(c, FLEET_ERR_ARG, "fleet_gate_create: %d header codes for the pool's %d headers", n_headers, p->w.n_hdr);
  fleet_gate* g = new fleet_gate();
  g->p = p;
  g->cap = std::max(p->slots, fleet::kAccBurst);
  const size_t n = (size_t)g->cap;
  bool ok = g->d_work.alloc(fleet::kAccBurst) == hipSuccess &&
            g->d_part.alloc((size_t)fleet::pool_vet_partial_doubles(p->w.launch())) == hipSuccess &&
            g->d_status.alloc(n) == hipSuccess && g->d_sumsq.alloc(n) == hipSuccess && g->d_max.alloc(n) == hipSuccess &&
            g->h_status.alloc(n) == hipSuccess && g->h_sumsq.alloc(n) == hipSuccess && g->h_max.alloc(n) == hipSuccess;
  if (ok && header_codes)
    ok = g->d_expected.alloc_zero((size_t)p->w.n_hdr + 16) == hipSuccess &&
         (!n_headers || hipMemcpy(g->d_expected, header_codes, sizeof(int32_t) * (size_t)n_headers, hipMemcpyHostToDevice) == hipSuccess);
  if (!ok) {
    (void)hipGetLastError();
    delete g;
    return fail(c, FLEET_ERR_NOMEM, "fleet_gate_create: allocating the gate of a pool of %d slots failed", p->slots);
  }
  *out = g;
  return FLEET_OK;
}

void fleet_gate_destroy(fleet_gate* g) {
  if (!g) return;
  fleet_ctx* c = g->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)settle(c, &g->p->fly, nullptr, true);  // a device vet in flight reads the gate's buffers
  (void)hipStreamSynchronize(c->stream);
  delete g;
}

int fleet_gate_vet(fleet_gate* g, const int32_t* slots, int K, int32_t* status, double* sumsq, float* max_abs) {
  if (!g || !slots || !status || !sumsq || !max_abs || K <= 0) return FLEET_ERR_ARG;
  fleet_pool* p = g->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = pool_update_args(p, slots, K, "fleet_gate_vet");
  if (rc) return rc;
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  return gate_vet_host(g, slots, K, status, sumsq, max_abs);
}

int fleet_gate_vet_device(fleet_gate* g, const int32_t* slots, int K, void* d_status, void* d_sumsq, void* d_max_abs,
                          void* stream) {
  if (!g || !slots || !d_status || !d_sumsq || !d_max_abs || K <= 0) return FLEET_ERR_ARG;
  fleet_pool* p = g->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = pool_update_args(p, slots, K, "fleet_gate_vet_device");
  if (rc) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if ((rc = gate_launch(g, slots, K, (int32_t*)d_status, (double*)d_sumsq, (float*)d_max_abs, s))) return rc;
  p->fly.on(s);  // the launch's words and partials are in use until `s` has run it
  return FLEET_OK;
}

int fleet_gate_put(fleet_gate* g, int slot, const char* upload, size_t len, int32_t* status, double* sumsq,
                   float* max_abs) {
  if (!g || !upload || !status || !sumsq || !max_abs) return FLEET_ERR_ARG;
  fleet_pool* p = g->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int rc = pool_slot_arg(p, slot, "fleet_gate_put");
  if (rc) return rc;
  if (p->occupied[slot]) return fail(c, FLEET_ERR_ARG, "fleet_gate_put: slot %d holds an upload", slot);
  if ((rc = window_len_arg(c, p->w, len, "the pool's"))) return rc;
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  if ((rc = window_copy_in(c, p->w, upload, p->h_row, p->d_rows + (size_t)slot * p->pitch, c->stream))) return rc;
  const int32_t one = slot;
  if ((rc = gate_vet_host(g, &one, 1, status, sumsq, max_abs))) return rc;
  // a refused upload's slot stays free: its bytes are what a dropped slot's are, gone with the next put
  if (*status & FLEET_ERRBIT_BASE64)
    return fail(c, FLEET_ERR_BASE64, "slot %d: input is not Base64::encode output (alphabet/padding)", slot);
  if (*status & FLEET_ERRBIT_LAYOUT)
    return fail(c, FLEET_ERR_LAYOUT, "slot %d: upload's layout header slots differ from the model's", slot);
  p->occupied[slot] = 1;
  return FLEET_OK;
}

// --------------------------------------------------------------- Kardam ledger

// Kardam.java's `grads` map (worker -> (g, epoch), Kardam.java:40, 56-71) with every g
// one fp32 row of a slab in HBM (upload coordinates, header slots 0). An update's picks
// are resolved against the tables on the host, in pick order, into (mode, prev row, out
// row) per pick; G always goes to a free row, and the tables change after the slot
// status came back clean, so a rejected update leaves no trace.
struct fleet_kledger {
  fleet_pool* p = nullptr;
  int workers = 0, max_store = 0, rows = 0;
  size_t vpitch = 0;           // floats per row: 12 G bytes rounded up to 16
  DevBuf<float> d_slab;
  DevBuf<double> d_part;       // one launch's per-wave partials
  DevBuf<double> d_sums;       // 2 sums per pick of an update (picks are distinct slots)
  PinBuf<double> h_sums;
  std::vector<int32_t> row_of, epoch_of, free_rows;
  // one update's resolution
  std::vector<int32_t> t_row, t_epoch, t_free, t_release, k_prev, k_out;
  std::vector<uint8_t> k_mode, k_set;
};

namespace {

static int kledger_worker_arg(const fleet_kledger* l, int worker, const char* what) {
  if (worker < 0 || worker >= l->workers)
    return fail(l->p->c, FLEET_ERR_ARG, "%s: worker %d outside [0, %d)", what, worker, l->workers);
  if (l->row_of[worker] < 0) return fail(l->p->c, FLEET_ERR_ARG, "%s: worker %d is not in the ledger", what, worker);
  return FLEET_OK;
}

// Kardam.setGrad's decisions (Kardam.java:56-71) for the picks in order, on copies of the
// tables; FLEET_ERR_ARG before anything is launched.
static int kledger_resolve(fleet_kledger* l, int K, const int32_t* worker, const int32_t* epoch, const char* what) {
  fleet_ctx* c = l->p->c;
  for (int k = 0; k < K; ++k)
    if (worker[k] >= l->workers) return fail(c, FLEET_ERR_ARG, "%s: pick %d names worker %d of %d", what, k, worker[k], l->workers);
  l->t_row = l->row_of, l->t_epoch = l->epoch_of, l->t_free = l->free_rows;
  l->t_release.clear();
  l->k_mode.assign((size_t)K, 0), l->k_set.assign((size_t)K, 0);
  l->k_prev.assign((size_t)K, -1), l->k_out.assign((size_t)K, -1);
  int stores = 0;
  for (int k = 0; k < K; ++k) {
    const int w = worker[k];
    if (w < 0) continue;  // Kardam does not run for this pick (CppNNUpdater.java:472-474)
    const int32_t cur = l->t_row[w];
    if (cur >= 0 && l->t_epoch[w] == epoch[k]) {  // the push is ignored (Kardam.java:59-62)
      l->k_mode[k] = 1;
      continue;
    }
    if (++stores > l->max_store || l->t_free.empty())
      return fail(c, FLEET_ERR_ARG, "%s: more than %d picks store a row", what, l->max_store);
    const int32_t out = l->t_free.back();
    l->t_free.pop_back();
    l->k_out[k] = out;
    l->k_mode[k] = 1 | 4;
    if (cur >= 0) {  // Kardam.java:63-65
      l->k_mode[k] |= 2;
      l->k_prev[k] = cur;
      l->k_set[k] = 1;
      l->t_release.push_back(cur);
    }
    l->t_row[w] = out, l->t_epoch[w] = epoch[k];
  }
  return FLEET_OK;
}

// pool_fold with the side outputs: every launch's sums land in d_sums[2 k0 ..)
static int kledger_fold(fleet_kledger* l, const int32_t* picks, int K, const double* dampen, double lr, hipStream_t s,
                        uint8_t* d_merged, float* d_f32) {
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  constexpr int B = fleet::kAccBurst;
  HIP_TRY(c, hipMemsetAsync(p->d_status, 0, sizeof(int) * (size_t)p->slots, s));
  for (int k0 = 0; k0 < K; k0 += B) {
    const int kc = std::min(B, K - k0);
    const fleet::PoolKd kd{lr, l->k_mode.data() + k0, l->k_prev.data() + k0, l->k_out.data() + k0, l->d_slab, l->vpitch,
                           l->rows, l->d_part, l->d_sums + 2 * (size_t)k0};
    HIP_TRY(c, fleet::launch_pool_fold_kd(p->d_rows, p->pitch, picks + k0, p->d_state, k0 == 0, kc, dampen + k0,
                                          k0 + kc == K, (double)1 / K, p->w.launch(), p->d_status, d_merged, d_f32, kd, s));
  }
  HIP_TRY(c, hipMemcpyAsync(p->h_status, p->d_status, sizeof(int) * (size_t)p->slots, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(l->h_sums, l->d_sums, sizeof(double) * 2 * (size_t)K, hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// after the stream was synchronised: the verdict, and on a clean one the commit and the outputs
static int kledger_commit(fleet_kledger* l, const int32_t* picks, int K, double* norm_g, double* norm_diff, uint8_t* set) {
  const int rc = pool_verdict(l->p, picks, K);
  if (rc) return rc;  // the tables, the free list and every row a worker names are as before
  l->row_of.swap(l->t_row), l->epoch_of.swap(l->t_epoch), l->free_rows.swap(l->t_free);
  l->free_rows.insert(l->free_rows.end(), l->t_release.begin(), l->t_release.end());
  for (int k = 0; k < K; ++k) {
    norm_g[k] = (l->k_mode[k] & 1) ? std::sqrt(l->h_sums[2 * k]) : std::nan("");
    norm_diff[k] = (l->k_mode[k] & 2) ? std::sqrt(l->h_sums[2 * k + 1]) : std::nan("");
    set[k] = l->k_set[k];
  }
  return FLEET_OK;
}

}  // namespace

int fleet_kledger_create(fleet_pool* p, int workers, int max_store, fleet_kledger** out) {
  if (!p || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (workers < 1 || max_store < 1) return FLEET_ERR_ARG;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (p->w.gb != 0 || p->w.ng != groups_of(p->w.n) || p->w.ng == 0)
    return fail(c, FLEET_ERR_ARG, "fleet_kledger_create: the pool holds the groups [%zu, %zu) of %zu (the norms are sums over the whole upload)",
                p->w.gb, p->w.ge, groups_of(p->w.n));
  if ((size_t)workers + (size_t)max_store > (size_t)1 << 24)
    return fail(c, FLEET_ERR_ARG, "fleet_kledger_create: %d workers + %d rows", workers, max_store);
  fleet_kledger* l = new fleet_kledger();
  l->p = p;
  l->workers = workers, l->max_store = max_store, l->rows = workers + max_store;
  l->vpitch = (12 * p->w.ng + 15) / 16 * 4;
  l->row_of.assign((size_t)workers, -1);
  l->epoch_of.assign((size_t)workers, 0);
  for (int r = l->rows - 1; r >= 0; --r) l->free_rows.push_back(r);
  const bool ok = l->d_slab.alloc_zero(l->vpitch * (size_t)l->rows) == hipSuccess &&
                  l->d_part.alloc((size_t)fleet::pool_kd_partial_doubles(p->w.launch())) == hipSuccess &&
                  l->d_sums.alloc(2 * (size_t)p->slots) == hipSuccess &&
                  l->h_sums.alloc(2 * (size_t)p->slots) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete l;
    return fail(c, FLEET_ERR_NOMEM, "fleet_kledger_create: allocating %d rows of %zu groups failed", workers + max_store, p->w.ng);
  }
  *out = l;
  return FLEET_OK;
}

void fleet_kledger_destroy(fleet_kledger* l) {
  if (!l) return;
  fleet_ctx* c = l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete l;
}

int fleet_kledger_workers(const fleet_kledger* l) { return l ? l->workers : FLEET_ERR_ARG; }

int fleet_kledger_has(const fleet_kledger* l, int worker) {
  if (!l || worker < 0 || worker >= l->workers) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->p->c->mu);
  return l->row_of[worker] >= 0 ? 1 : 0;
}

int fleet_kledger_epoch(const fleet_kledger* l, int worker, int* epoch) {
  if (!l || !epoch) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->p->c->mu);
  const int rc = kledger_worker_arg(l, worker, "fleet_kledger_epoch");
  if (rc) return rc;
  *epoch = l->epoch_of[worker];
  return FLEET_OK;
}

int fleet_kledger_forget(fleet_kledger* l, int worker) {
  if (!l) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->p->c->mu);
  const int rc = kledger_worker_arg(l, worker, "fleet_kledger_forget");
  if (rc) return rc;
  l->free_rows.push_back(l->row_of[worker]);  // every update synchronised: nothing in flight reads the row
  l->row_of[worker] = -1;
  return FLEET_OK;
}

int fleet_kledger_read(fleet_kledger* l, int worker, float* g, size_t cap) {
  if (!l || !g) return FLEET_ERR_ARG;
  fleet_ctx* c = l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const int rc = kledger_worker_arg(l, worker, "fleet_kledger_read");
  if (rc) return rc;
  const size_t n = l->p->w.n;
  if (cap < n) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu values", cap, n);
  HIP_TRY(c, hipMemcpyAsync(g, l->d_slab + (size_t)l->row_of[worker] * l->vpitch, sizeof(float) * n, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLEET_OK;
}

int fleet_kledger_update(fleet_kledger* l, const int32_t* picks, int K, const double* dampen, const int32_t* worker,
                         const int32_t* epoch, double lr, char* merged, size_t cap, size_t* out_len, float* merged_f32,
                         double* norm_g, double* norm_diff, uint8_t* set) {
  if (!l || !picks || !dampen || !merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set)
    return FLEET_ERR_ARG;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kledger_update: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kledger_update");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kledger_update"))) return rc;
  if (out_len) *out_len = p->w.len;
  if (cap < p->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, p->w.len);
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  uint8_t* d_out = p->d_rows + (size_t)p->slots * p->pitch;  // as fleet_pool_update
  if ((rc = kledger_fold(l, picks, K, dampen, lr, c->stream, d_out, merged_f32 ? p->d_state : nullptr))) return rc;
  if ((rc = window_read_back(c, p->w, d_out, p->d_state, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return kledger_commit(l, picks, K, norm_g, norm_diff, set);
}

int fleet_kledger_update_device(fleet_kledger* l, const int32_t* picks, int K, const double* dampen,
                                const int32_t* worker, const int32_t* epoch, double lr, void* d_merged,
                                void* d_merged_f32, double* norm_g, double* norm_diff, uint8_t* set, void* stream) {
  if (!l || !picks || !dampen || !d_merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set)
    return FLEET_ERR_ARG;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kledger_update_device: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kledger_update_device");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kledger_update_device"))) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if ((rc = kledger_fold(l, picks, K, dampen, lr, s, (uint8_t*)d_merged, (float*)d_merged_f32))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  p->fly.done();
  return kledger_commit(l, picks, K, norm_g, norm_diff, set);
}

// ------------------------------------------------------ Kardam Byzantine filter

// What Kardam.checkByz reads of an update's picks (Kardam.java:136-185; CppNNUpdater.java:
// 488 without its `true ||`), beside a ledger: lastGrad as two fp32 rows in upload
// coordinates (d_lg[lg] is read by the update's kernel, d_lg[lg ^ 1] receives the avg of
// the update's result as lastGrad decodes it, Q(f32(f64(A) / accepted)); the two swap when
// a resolve ends with an average), currModel / lastModel as two rows of a slab (d_m, rows mc and mc ^ 1), and the
// optimistic result of the pending update (d_out, d_f32).
struct FLEET_MEM_LOCAL fleet_kfilter {
  fleet_kledger* l = nullptr;
  size_t n_w = 0, n_b = 0, n_m = 0, mpitch = 0;
  int edges = 0;
  DevBuf<float> d_lg[2];
  int lg = 0;
  bool has_last = false;
  DevBuf<uint8_t> d_out;        // the merged bytes of the pending update
  DevBuf<float> d_f32;          // and their decodeFloat
  DevBuf<double> d_part;        // one launch's per-wave partials (four sums a pick)
  DevBuf<double> d_sums;        // 4 sums per pick of an update
  PinBuf<double> h_sums;
  DevBuf<float> d_m;            // two model rows
  int mc = 0;
  bool has_model = false, has_last_model = false;  // row mc was staged since the last resolve / row mc ^ 1 holds lastModel
  DevBuf<float> d_w, d_b;       // the host form's staging of a model
  DevBuf<double> d_mpart;       // kAccBurst * kMlMaxTiles partials
  DevBuf<double> d_msq;         // {row norm, pair norm}
  PinBuf<double> h_msq;
  // the pending update
  bool pending = false;
  std::vector<int32_t> picks;
  std::vector<double> dampen;
};

namespace {

// kledger_fold through the filter form: the merged bytes and their fp32 go to the filter's
// own rows, the avg to the lastGrad row that is not read, the four sums of every pick to
// d_sums[4 k ..)
static int kfilter_fold(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen, double lr, hipStream_t s) {
  fleet_kledger* l = f->l;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  constexpr int B = fleet::kAccBurst;
  HIP_TRY(c, hipMemsetAsync(p->d_status, 0, sizeof(int) * (size_t)p->slots, s));
  for (int k0 = 0; k0 < K; k0 += B) {
    const int kc = std::min(B, K - k0);
    const fleet::PoolKd kd{lr, l->k_mode.data() + k0, l->k_prev.data() + k0, l->k_out.data() + k0, l->d_slab, l->vpitch,
                           l->rows, f->d_part, f->d_sums + 4 * (size_t)k0};
    HIP_TRY(c, fleet::launch_pool_fold_kf(p->d_rows, p->pitch, picks + k0, p->d_state, k0 == 0, kc, dampen + k0,
                                          k0 + kc == K, (double)1 / K, p->w.launch(), p->d_status, f->d_out, f->d_f32,
                                          kd, f->has_last ? f->d_lg[f->lg] : nullptr, f->d_lg[f->lg ^ 1], s));
  }
  HIP_TRY(c, hipMemcpyAsync(p->h_status, p->d_status, sizeof(int) * (size_t)p->slots, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(f->h_sums, f->d_sums, sizeof(double) * 4 * (size_t)K, hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// after the stream was synchronised: kledger_commit on the first two sums of every pick,
// and on a clean verdict the filter's norms and the pending update
static int kfilter_commit(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen, double* norm_g,
                          double* norm_diff, uint8_t* set, double* norm_p, double* norm_pdiff) {
  fleet_kledger* l = f->l;
  for (int k = 0; k < K; ++k) l->h_sums[2 * k] = f->h_sums[4 * k], l->h_sums[2 * k + 1] = f->h_sums[4 * k + 1];
  const int rc = kledger_commit(l, picks, K, norm_g, norm_diff, set);
  if (rc) return rc;
  for (int k = 0; k < K; ++k) {
    norm_p[k] = std::sqrt(f->h_sums[4 * k + 2]);
    norm_pdiff[k] = f->has_last ? std::sqrt(f->h_sums[4 * k + 3]) : std::nan("");
  }
  f->picks.assign(picks, picks + K);
  f->dampen.assign(dampen, dampen + K);
  f->pending = true;
  return FLEET_OK;
}

// the device outputs of an update or a resolve from the filter's rows, on s
static int kfilter_copy_out(fleet_kfilter* f, void* d_merged, void* d_merged_f32, hipStream_t s) {
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  HIP_TRY(c, hipMemcpyAsync(d_merged, f->d_out, 16 * p->w.ng, hipMemcpyDeviceToDevice, s));
  if (d_merged_f32)
    HIP_TRY(c, hipMemcpyAsync(d_merged_f32, f->d_f32, sizeof(float) * p->w.n, hipMemcpyDeviceToDevice, s));
  return FLEET_OK;
}

// A resolve's checks (FLEET_ERR_ARG with everything untouched) and the count of accepted picks.
static int kfilter_resolve_args(fleet_kfilter* f, const uint8_t* accept, int K, const char* what, int* accepted) {
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  if (!f->pending) return fail(c, FLEET_ERR_ARG, "%s: no update is pending", what);
  if (K != (int)f->picks.size())
    return fail(c, FLEET_ERR_ARG, "%s: %d decisions for the pending update's %zu picks", what, K, f->picks.size());
  for (int k = 0; k < K; ++k)
    if (!p->occupied[f->picks[k]])
      return fail(c, FLEET_ERR_ARG, "%s: pick %d's slot %d holds no upload any more", what, k, f->picks[k]);
  int n = 0;
  for (int k = 0; k < K; ++k) n += accept[k] ? 1 : 0;
  *accepted = n;
  return FLEET_OK;
}

// The refold of a proper subset (CppNNUpdater.java:490-508 over the accepted picks): the
// pool's fold without its finish over the accepted slots in pick order, then the finish
// with the last of all K picks' row, so the header and the unwalked slots are that pick's
// whether it was accepted or not (:508, pickedG). Overwrites the filter's output rows.
static int kfilter_refold(fleet_kfilter* f, const uint8_t* accept, int accepted, hipStream_t s) {
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  constexpr int B = fleet::kAccBurst;
  const int K = (int)f->picks.size();
  std::vector<int32_t> slots;
  std::vector<double> d;
  for (int k = 0; k < K; ++k)
    if (accept[k]) slots.push_back(f->picks[k]), d.push_back(f->dampen[k]);
  HIP_TRY(c, hipMemsetAsync(p->d_status, 0, sizeof(int) * (size_t)p->slots, s));
  for (int k0 = 0; k0 < accepted; k0 += B) {
    const int kc = std::min(B, accepted - k0);
    HIP_TRY(c, fleet::launch_pool_fold(p->d_rows, p->pitch, slots.data() + k0, p->d_state, k0 == 0, kc, d.data() + k0, false,
                                       (double)1 / accepted, p->w.launch(), p->d_status, nullptr, nullptr, s));
  }
  HIP_TRY(c, fleet::launch_acc_finish(p->d_rows + (size_t)f->picks[K - 1] * p->pitch, p->d_state, (double)1 / accepted,
                                      p->w.launch(), f->d_out, f->d_f32, s));
  HIP_TRY(c, fleet::launch_acc_avg_row(p->d_state, (double)1 / accepted, p->w.launch(), f->d_lg[f->lg ^ 1], s));
  HIP_TRY(c, hipMemcpyAsync(p->h_status, p->d_status, sizeof(int) * (size_t)p->slots, hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

// a resolve that ended with an average: lastGrad and lastModel advance (CppNNUpdater.java:510-511)
static void kfilter_advance(fleet_kfilter* f) {
  f->lg ^= 1;
  f->has_last = true;
  if (f->has_model) {
    f->mc ^= 1;
    f->has_last_model = true;
  }
}

// currModel from device vectors on s, its norm and the norm of its difference to lastModel
static int kfilter_model_on(fleet_kfilter* f, const float* d_w, const float* d_b, hipStream_t s, double* norm_model,
                            double* norm_model_diff) {
  fleet_ctx* c = f->l->p->c;
  HIP_TRY(c, fleet::launch_mrow_stage(d_w, (int64_t)f->n_w, d_b, (int64_t)f->n_b, f->n_b ? (int64_t)f->edges : 0,
                                      f->d_m + (size_t)f->mc * f->mpitch, f->d_mpart, f->d_msq, s));
  if (f->has_last_model) {
    const int32_t cur = f->mc, prev = f->mc ^ 1;
    HIP_TRY(c, fleet::launch_mrow_pair_norms(f->d_m, f->mpitch, 2, (int64_t)f->n_m, &cur, &prev, 1, f->d_mpart, f->d_msq + 1, s));
  }
  HIP_TRY(c, hipMemcpyAsync(f->h_msq, f->d_msq, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  f->has_model = true;
  *norm_model = std::sqrt(f->h_msq[0]);
  *norm_model_diff = f->has_last_model ? std::sqrt(f->h_msq[1]) : std::nan("");
  return FLEET_OK;
}

}  // namespace

int fleet_kfilter_create(fleet_kledger* l, size_t n_weights, size_t n_biases, int graph_edges, fleet_kfilter** out) {
  if (!l || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (graph_edges < 0) return FLEET_ERR_ARG;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (n_weights >= (size_t)fleet::kMlMaxValues || n_biases >= (size_t)fleet::kMlMaxValues)
    return fail(c, FLEET_ERR_ARG, "fleet_kfilter_create: %zu weights, %zu biases", n_weights, n_biases);
  const size_t n = n_biases * (size_t)graph_edges + n_weights;
  if (n == 0 || n >= (size_t)fleet::kMlMaxValues) return fail(c, FLEET_ERR_ARG, "fleet_kfilter_create: a model of %zu values", n);
  fleet_kfilter* f = new fleet_kfilter();
  f->l = l;
  f->n_w = n_weights, f->n_b = n_biases, f->edges = graph_edges, f->n_m = n;
  f->mpitch = (n + 3) / 4 * 4;
  const size_t lg = 3 * p->w.ng;  // the floats of a state row (Window::state_bytes: and 64 bytes)
  const bool ok =
      f->d_lg[0].alloc_zero(lg, 64) == hipSuccess && f->d_lg[1].alloc_zero(lg, 64) == hipSuccess &&
      f->d_out.alloc_zero(p->w.row_bytes()) == hipSuccess && f->d_f32.alloc_zero(lg, 64) == hipSuccess &&
      f->d_part.alloc((size_t)fleet::pool_kf_partial_doubles(p->w.launch())) == hipSuccess &&
      f->d_sums.alloc(4 * (size_t)p->slots) == hipSuccess && f->h_sums.alloc(4 * (size_t)p->slots) == hipSuccess &&
      f->d_m.alloc_zero(2 * f->mpitch) == hipSuccess && f->d_w.alloc(std::max<size_t>(1, n_weights)) == hipSuccess &&
      f->d_b.alloc(std::max<size_t>(1, n_biases)) == hipSuccess &&
      f->d_mpart.alloc((size_t)fleet::kAccBurst * fleet::kMlMaxTiles) == hipSuccess &&
      f->d_msq.alloc(2) == hipSuccess && f->h_msq.alloc(2) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete f;
    return fail(c, FLEET_ERR_NOMEM, "fleet_kfilter_create: allocating the rows of %zu groups and %zu model values failed", p->w.ng, n);
  }
  *out = f;
  return FLEET_OK;
}

void fleet_kfilter_destroy(fleet_kfilter* f) {
  if (!f) return;
  fleet_ctx* c = f->l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete f;
}

int fleet_kfilter_has_last(const fleet_kfilter* f) {
  if (!f) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(f->l->p->c->mu);
  return f->has_last ? 1 : 0;
}

int fleet_kfilter_set_model(fleet_kfilter* f, const float* weights, const float* biases, double* norm_model,
                            double* norm_model_diff) {
  if (!f || (f->n_w && !weights) || (f->n_b && !biases) || !norm_model || !norm_model_diff) return FLEET_ERR_ARG;
  fleet_ctx* c = f->l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (f->n_w) HIP_TRY(c, hipMemcpyAsync(f->d_w, weights, sizeof(float) * f->n_w, hipMemcpyHostToDevice, c->stream));
  if (f->n_b) HIP_TRY(c, hipMemcpyAsync(f->d_b, biases, sizeof(float) * f->n_b, hipMemcpyHostToDevice, c->stream));
  return kfilter_model_on(f, f->d_w, f->d_b, c->stream, norm_model, norm_model_diff);
}

int fleet_kfilter_set_model_device(fleet_kfilter* f, const float* d_weights, const float* d_biases, double* norm_model,
                                   double* norm_model_diff, void* stream) {
  if (!f || (f->n_w && !d_weights) || (f->n_b && !d_biases) || !norm_model || !norm_model_diff) return FLEET_ERR_ARG;
  fleet_ctx* c = f->l->p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  return kfilter_model_on(f, d_weights, d_biases, pick(c, stream), norm_model, norm_model_diff);
}

int fleet_kfilter_update(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen, const int32_t* worker,
                         const int32_t* epoch, double lr, char* merged, size_t cap, size_t* out_len, float* merged_f32,
                         double* norm_g, double* norm_diff, uint8_t* set, double* norm_p, double* norm_pdiff) {
  if (!f || !picks || !dampen || !merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set || !norm_p ||
      !norm_pdiff)
    return FLEET_ERR_ARG;
  fleet_kledger* l = f->l;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  f->pending = false;
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kfilter_update: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kfilter_update");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kfilter_update"))) return rc;
  if (out_len) *out_len = p->w.len;
  if (cap < p->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, p->w.len);
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  if ((rc = kfilter_fold(f, picks, K, dampen, lr, c->stream))) return rc;
  if ((rc = window_read_back(c, p->w, f->d_out, f->d_f32, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return kfilter_commit(f, picks, K, dampen, norm_g, norm_diff, set, norm_p, norm_pdiff);
}

int fleet_kfilter_update_device(fleet_kfilter* f, const int32_t* picks, int K, const double* dampen,
                                const int32_t* worker, const int32_t* epoch, double lr, void* d_merged,
                                void* d_merged_f32, double* norm_g, double* norm_diff, uint8_t* set, double* norm_p,
                                double* norm_pdiff, void* stream) {
  if (!f || !picks || !dampen || !d_merged || K <= 0 || !worker || !epoch || !norm_g || !norm_diff || !set || !norm_p ||
      !norm_pdiff)
    return FLEET_ERR_ARG;
  fleet_kledger* l = f->l;
  fleet_pool* p = l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  f->pending = false;
  if (!std::isfinite(lr)) return fail(c, FLEET_ERR_ARG, "fleet_kfilter_update_device: the learning rate is not finite");
  int rc = pool_update_args(p, picks, K, "fleet_kfilter_update_device");
  if (rc || (rc = kledger_resolve(l, K, worker, epoch, "fleet_kfilter_update_device"))) return rc;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if ((rc = kfilter_fold(f, picks, K, dampen, lr, s))) return rc;
  if ((rc = kfilter_copy_out(f, d_merged, d_merged_f32, s))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  p->fly.done();
  return kfilter_commit(f, picks, K, dampen, norm_g, norm_diff, set, norm_p, norm_pdiff);
}

int fleet_kfilter_resolve(fleet_kfilter* f, const uint8_t* accept, int K, char* merged, size_t cap, size_t* out_len,
                          float* merged_f32) {
  if (!f || !accept || !merged || !out_len || K <= 0) return FLEET_ERR_ARG;
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int accepted = 0;
  int rc = kfilter_resolve_args(f, accept, K, "fleet_kfilter_resolve", &accepted);
  if (rc) return rc;
  if (accepted && cap < p->w.len) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu", cap, p->w.len);
  f->pending = false;
  *out_len = 0;
  if (!accepted) return FLEET_OK;  // no average: lastGrad and lastModel stay (CppNNUpdater.java:506)
  if ((rc = settle(c, &p->fly, c->stream, true))) return rc;
  if (accepted < K && (rc = kfilter_refold(f, accept, accepted, c->stream))) return rc;
  if ((rc = window_read_back(c, p->w, f->d_out, f->d_f32, merged, merged_f32, c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (accepted < K && (rc = pool_verdict(p, f->picks.data(), K))) return rc;
  *out_len = p->w.len;
  kfilter_advance(f);
  return FLEET_OK;
}

int fleet_kfilter_resolve_device(fleet_kfilter* f, const uint8_t* accept, int K, void* d_merged, void* d_merged_f32,
                                 size_t* out_len, void* stream) {
  if (!f || !accept || !d_merged || !out_len || K <= 0) return FLEET_ERR_ARG;
  fleet_pool* p = f->l->p;
  fleet_ctx* c = p->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  int accepted = 0;
  int rc = kfilter_resolve_args(f, accept, K, "fleet_kfilter_resolve_device", &accepted);
  if (rc) return rc;
  f->pending = false;
  *out_len = 0;
  if (!accepted) return FLEET_OK;
  hipStream_t s = pick(c, stream);
  if ((rc = settle(c, &p->fly, s, false))) return rc;
  if (accepted < K && (rc = kfilter_refold(f, accept, accepted, s))) return rc;
  if ((rc = kfilter_copy_out(f, d_merged, d_merged_f32, s))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s));
  p->fly.done();
  if (accepted < K && (rc = pool_verdict(p, f->picks.data(), K))) return rc;
  *out_len = p->w.len;
  kfilter_advance(f);
  return FLEET_OK;
}

// --------------------------------------------------------- Kardam model ledger

// Kardam.java's `models` map (worker -> model, Kardam.java:114-125) over a slab of fp32
// rows that belong to model versions (mledger_table.h keeps the tables and resolves an
// update into row pairs; mledger_kernels.hip fills rows and computes the pairs' norms).
struct FLEET_MEM_LOCAL fleet_mledger {
  fleet_ctx* c = nullptr;
  size_t n_w = 0, n_b = 0, n = 0;
  int edges = 0;
  size_t vpitch = 0;            // floats per row: n rounded up to 4
  std::unique_ptr<fleet::MledgerTable> t;
  DevBuf<float> d_slab;
  DevBuf<float> d_w, d_b;          // the host form's staging of one version
  DevBuf<double> d_stage_part;     // kMlMaxTiles partials per row: stages on different streams do not meet
  DevBuf<double> d_row_sq;         // per row: sum (double)(a * a)
  DevBuf<double> d_pair_part;      // one launch of pairs
  DevBuf<double> d_pair_sq;        // an update's pairs; freed on growth
  PinBuf<double> h_sq;             // rows row sums, then the pairs'; freed on growth
  hipEvent_t staged = nullptr;     // orders the context's stream after a stage on a caller's stream
  std::vector<double> pair_norm;
  ~fleet_mledger() {
    if (staged) (void)hipEventDestroy(staged);
  }
};

namespace {

static int mledger_worker_arg(const fleet_mledger* l, int worker, const char* what) {
  if (worker < 0 || worker >= l->t->workers())
    return fail(l->c, FLEET_ERR_ARG, "%s: worker %d outside [0, %d)", what, worker, l->t->workers());
  if (l->t->row_of_worker(worker) < 0) return fail(l->c, FLEET_ERR_ARG, "%s: worker %d holds no model", what, worker);
  return FLEET_OK;
}

// room for an update's P pairs in HBM and pinned memory
static int mledger_pair_room(fleet_mledger* l, size_t P) {
  fleet_ctx* c = l->c;
  const size_t rows = (size_t)l->t->rows();
  if (P > l->d_pair_sq.cap())
    HIP_TRY(c, l->d_pair_sq.grow_exact(std::max<size_t>(2 * P, 4 * (size_t)fleet::kAccBurst)));
  HIP_TRY(c, l->h_sq.grow_exact(rows + l->d_pair_sq.cap()));
  return FLEET_OK;
}

// version `id` from device vectors on stream s; the caller holds the context's mutex
static int mledger_stage_on(fleet_mledger* l, int64_t id, const float* d_w, const float* d_b, hipStream_t s) {
  fleet_ctx* c = l->c;
  bool fresh = false;
  const int row = l->t->stage(id, &fresh);
  if (!fresh) return FLEET_OK;
  const hipError_t e = fleet::launch_mrow_stage(d_w, (int64_t)l->n_w, d_b, (int64_t)l->n_b, l->n_b ? (int64_t)l->edges : 0,
                                                l->d_slab + (size_t)row * l->vpitch,
                                                l->d_stage_part + (size_t)row * fleet::kMlMaxTiles, l->d_row_sq + row, s);
  if (e != hipSuccess) {
    l->t->unstage(id);
    return fail(c, FLEET_ERR_HIP, "launch_mrow_stage: %s", hipGetErrorString(e));
  }
  return FLEET_OK;
}

static int mledger_read_row(fleet_mledger* l, int row, float* params, size_t cap) {
  fleet_ctx* c = l->c;
  if (cap < l->n) return fail(c, FLEET_ERR_CAPACITY, "output capacity %zu < %zu values", cap, l->n);
  HIP_TRY(c, hipMemcpyAsync(params, l->d_slab + (size_t)row * l->vpitch, sizeof(float) * l->n, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLEET_OK;
}

}  // namespace

int fleet_mledger_create(fleet_ctx* c, size_t n_weights, size_t n_biases, int graph_edges, int workers,
                         int max_versions, fleet_mledger** out) {
  if (!c || !out) return FLEET_ERR_ARG;
  *out = nullptr;
  if (workers < 1 || max_versions < 1 || graph_edges < 0) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (n_weights >= (size_t)fleet::kMlMaxValues || n_biases >= (size_t)fleet::kMlMaxValues ||
      (size_t)workers + (size_t)max_versions > (size_t)1 << 24)
    return fail(c, FLEET_ERR_ARG, "fleet_mledger_create: %zu weights, %zu biases, %d workers + %d versions", n_weights,
                n_biases, workers, max_versions);
  const size_t n = n_biases * (size_t)graph_edges + n_weights;
  if (n == 0 || n >= (size_t)fleet::kMlMaxValues)
    return fail(c, FLEET_ERR_ARG, "fleet_mledger_create: a model of %zu values", n);
  fleet_mledger* l = new fleet_mledger();
  l->c = c;
  l->n_w = n_weights, l->n_b = n_biases, l->edges = graph_edges, l->n = n;
  l->vpitch = (n + 3) / 4 * 4;
  l->t.reset(new fleet::MledgerTable(workers, max_versions));
  const size_t rows = (size_t)l->t->rows();
  const bool ok =
      l->d_slab.alloc_zero(l->vpitch * rows) == hipSuccess && l->d_w.alloc(std::max<size_t>(1, n_weights)) == hipSuccess &&
      l->d_b.alloc(std::max<size_t>(1, n_biases)) == hipSuccess &&
      l->d_stage_part.alloc(rows * fleet::kMlMaxTiles) == hipSuccess && l->d_row_sq.alloc_zero(rows) == hipSuccess &&
      l->d_pair_part.alloc((size_t)fleet::kAccBurst * fleet::kMlMaxTiles) == hipSuccess &&
      hipEventCreateWithFlags(&l->staged, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete l;
    return fail(c, FLEET_ERR_NOMEM, "fleet_mledger_create: allocating %zu rows of %zu values failed", rows, n);
  }
  *out = l;
  return FLEET_OK;
}

void fleet_mledger_destroy(fleet_mledger* l) {
  if (!l) return;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dg(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete l;
}

fleet_ctx* fleet_ctx_of_mledger(const fleet_mledger* l) { return l ? l->c : nullptr; }

int fleet_mledger_shape(const fleet_mledger* l, size_t* n_weights, size_t* n_biases, int* graph_edges, int* workers,
                        int* max_versions) {
  if (!l) return FLEET_ERR_ARG;
  if (n_weights) *n_weights = l->n_w;
  if (n_biases) *n_biases = l->n_b;
  if (graph_edges) *graph_edges = l->edges;
  if (workers) *workers = l->t->workers();
  if (max_versions) *max_versions = l->t->max_versions();
  return FLEET_OK;
}

int fleet_mledger_launch_shape(int* wave, int* block_values, int* max_blocks) {
  if (wave) *wave = 64;
  if (block_values) *block_values = fleet::mrow_block_values();
  if (max_blocks) *max_blocks = fleet::kMlMaxTiles;
  return FLEET_OK;
}

int fleet_mledger_stage(fleet_mledger* l, int64_t id, const float* weights, const float* biases) {
  if (!l || (l->n_w && !weights) || (l->n_b && !biases)) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  if (l->t->row_of_id(id) >= 0) {  // resident: only its age changes
    bool fresh;
    (void)l->t->stage(id, &fresh);
    return FLEET_OK;
  }
  if (l->n_w) HIP_TRY(c, hipMemcpyAsync(l->d_w, weights, sizeof(float) * l->n_w, hipMemcpyHostToDevice, c->stream));
  if (l->n_b) HIP_TRY(c, hipMemcpyAsync(l->d_b, biases, sizeof(float) * l->n_b, hipMemcpyHostToDevice, c->stream));
  const int rc = mledger_stage_on(l, id, l->d_w, l->d_b, c->stream);
  if (rc) return rc;
  const hipError_t e = hipStreamSynchronize(c->stream);  // the caller's vectors and d_w / d_b are free again
  if (e != hipSuccess) {
    l->t->unstage(id);
    return fail(c, FLEET_ERR_HIP, "fleet_mledger_stage: %s", hipGetErrorString(e));
  }
  return FLEET_OK;
}

int fleet_mledger_stage_device(fleet_mledger* l, int64_t id, const float* d_weights, const float* d_biases,
                               void* stream) {
  if (!l || (l->n_w && !d_weights) || (l->n_b && !d_biases)) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  hipStream_t s = pick(c, stream);
  const bool was = l->t->row_of_id(id) >= 0;
  const int rc = mledger_stage_on(l, id, d_weights, d_biases, s);
  if (rc || was || s == c->stream) return rc;
  HIP_TRY(c, hipEventRecord(l->staged, s));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, l->staged, 0));
  return FLEET_OK;
}

int fleet_mledger_resident(const fleet_mledger* l, int64_t id) {
  if (!l) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  return l->t->row_of_id(id) >= 0 ? 1 : 0;
}

int fleet_mledger_has(const fleet_mledger* l, int worker) {
  if (!l || worker < 0 || worker >= l->t->workers()) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  return l->t->row_of_worker(worker) >= 0 ? 1 : 0;
}

int fleet_mledger_version(const fleet_mledger* l, int worker, int64_t* id) {
  if (!l || !id) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  const int rc = mledger_worker_arg(l, worker, "fleet_mledger_version");
  if (rc) return rc;
  *id = l->t->id_of_row(l->t->row_of_worker(worker));
  return FLEET_OK;
}

int fleet_mledger_forget(fleet_mledger* l, int worker) {
  if (!l) return FLEET_ERR_ARG;
  std::lock_guard<std::mutex> lk(l->c->mu);
  const int rc = mledger_worker_arg(l, worker, "fleet_mledger_forget");
  if (rc) return rc;
  (void)l->t->forget(worker);
  return FLEET_OK;
}

int fleet_mledger_read(fleet_mledger* l, int worker, float* params, size_t cap) {
  if (!l || !params) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const int rc = mledger_worker_arg(l, worker, "fleet_mledger_read");
  if (rc) return rc;
  return mledger_read_row(l, l->t->row_of_worker(worker), params, cap);
}

int fleet_mledger_read_version(fleet_mledger* l, int64_t id, float* params, size_t cap) {
  if (!l || !params) return FLEET_ERR_ARG;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  const int row = l->t->row_of_id(id);
  if (row < 0) return fail(c, FLEET_ERR_ARG, "fleet_mledger_read_version: version %lld is not resident", (long long)id);
  return mledger_read_row(l, row, params, cap);
}

int fleet_mledger_update(fleet_mledger* l, const int64_t* id, const int32_t* worker, int K, double* norm_model,
                         double* norm_diff, uint8_t* status) {
  if (!l || K < 0 || !id || !worker || !norm_model || !norm_diff || !status) return FLEET_ERR_ARG;
  if (K == 0) return FLEET_OK;
  fleet_ctx* c = l->c;
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  fleet::MledgerTable& t = *l->t;
  std::string why;
  if (!t.resolve(id, worker, K, &why)) return fail(c, FLEET_ERR_ARG, "fleet_mledger_update: %s", why.c_str());
  const size_t rows = (size_t)t.rows(), P = t.pair_cur().size();
  if (t.active()) {  // (none: every pick is skipped and nothing is launched or copied)
    int rc = mledger_pair_room(l, P);
    if (rc) return rc;
    constexpr int B = fleet::kAccBurst;
    for (size_t p0 = 0; p0 < P; p0 += B) {
      const int pc = (int)std::min<size_t>(B, P - p0);
      HIP_TRY(c, fleet::launch_mrow_pair_norms(l->d_slab, l->vpitch, (int)rows, (int64_t)l->n, t.pair_cur().data() + p0,
                                               t.pair_prev().data() + p0, pc, l->d_pair_part, l->d_pair_sq + p0,
                                               c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(l->h_sq, l->d_row_sq, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
    if (P)
      HIP_TRY(c, hipMemcpyAsync(l->h_sq + rows, l->d_pair_sq, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  l->pair_norm.resize(P);
  for (size_t i = 0; i < P; ++i) l->pair_norm[i] = std::sqrt(l->h_sq[rows + i]);
  t.replay(l->pair_norm.data(), norm_diff, status);  // Kardam.java:114-125 in pick order; the tables change here
  for (int k = 0; k < K; ++k)
    norm_model[k] = t.pick_row(k) >= 0 ? std::sqrt(l->h_sq[(size_t)t.pick_row(k)]) : std::nan("");
  return FLEET_OK;
}

const char* fleet_update_kernel(size_t len) {
  static thread_local std::string name;
  name = fleet::update_kernel_name((int64_t)groups_of(fleet_b64_count(len)));
  return name.c_str();
}

int fleet_update_plan_grid(size_t len, int* kind, int64_t* blocks, int64_t* n_a, int64_t* n_w, int64_t* n_n) {
  if (!kind || !blocks || !n_a || !n_w || !n_n) return FLEET_ERR_ARG;
  fleet::update_plan_grid((int64_t)groups_of(fleet_b64_count(len)), kind, blocks, n_a, n_w, n_n);
  return FLEET_OK;
}

const char* fleet_update_encode_kernel(size_t len) {
  static thread_local std::string name;
  name = fleet::update_encode_kernel_name((int64_t)groups_of(fleet_b64_count(len)));
  return name.c_str();
}

int fleet_set_plan(const char* spec, char* err, size_t cap) {
  std::string e;
  if (fleet::set_plan_overrides(spec, &e) == 0) return FLEET_OK;
  if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
  return FLEET_ERR_ARG;
}

const char* fleet_plan(void) {
  static thread_local std::string spec;
  spec = fleet::plan_spec();
  return spec.c_str();
}

int fleet_selftest_digest(fleet_ctx* c, int fn, uint64_t* out) {
  if (!c || !out) return FLEET_ERR_ARG;
  if (fn < 0 || fn > 30) return fail(c, FLEET_ERR_ARG, "no self-test function %d", fn);
  std::lock_guard<std::mutex> lk(c->mu);
  DEVICE_SCOPE(c);
  DevBuf<unsigned long long> d;  // freed on every path
  HIP_TRY(c, d.alloc(1));
  HIP_TRY(c, hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream));
  HIP_TRY(c, fn >= 25 ? fleet::launch_digest_solver(fn, d, c->stream) : fleet::launch_digest(fn, d, c->stream));
  unsigned long long h = 0;
  HIP_TRY(c, hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *out = h;
  return FLEET_OK;
}

}  // extern "C"

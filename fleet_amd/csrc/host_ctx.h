// fleet_amd/csrc/host_ctx.h -- the context, and what more than one host unit of the C-ABI
// needs of it (fleet_codec.cpp, net_entry.cpp, stream_state.cpp, kardam_state.cpp).
//
// Internal to those four units: not installed, and nothing under include/ includes it. The
// other state units (model_state.cpp, rmodel_state.cpp, sampler_state.cpp) reach a context
// through include/fleet_codec.h alone. The helpers live in fleet::host, hidden, and no host unit
// opens an extern "C" block: an entry point takes its C linkage from its declaration in
// fleet_codec.h, so a helper cannot end up with an unmangled name.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fleet_codec.h"
#include "dev_mem.h"

namespace fleet {
namespace host FLEET_MEM_LOCAL {
class WorkerPool;  // fleet_codec.cpp
}
}  // namespace fleet

struct FLEET_MEM_LOCAL fleet_ctx {
  ~fleet_ctx();  // fleet_codec.cpp, where WorkerPool is complete
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
  std::unique_ptr<fleet::host::WorkerPool> pool;  // staging copy threads (stage_uploads)
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
  // the same table continued to the CIFAR-100 vector's 331,237 draws (2.65 MB), uploaded on
  // the first DP call on the CIFAR network
  fleet::DevBuf<double> d_rgb_z;
};

namespace fleet {
namespace host FLEET_MEM_LOCAL {

using fleet::DevBuf;
using fleet::PinBuf;

constexpr size_t kHdrWords = FLEET_MAX_HEADERS + 4;  // {status, count, walk_end, 0, positions}

inline int fail(fleet_ctx* c, int code, const char* fmt, ...) {
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
    if (e_ != hipSuccess) {                                                                      \
      (void)hipGetLastError(); /* reported here, not by the thread's next launch check */        \
      return fail((ctx), FLEET_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));                 \
    }                                                                                            \
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
inline int nomem(fleet_ctx* c, const char* call, size_t bytes, hipError_t e) {
  return fail(c, FLEET_ERR_NOMEM, "%s(%zu): %s", call, bytes, hipGetErrorString(e));
}

template <typename T>
int grow_dev(fleet_ctx* c, fleet::DevBuf<T>& b, size_t need_elems) {
  const size_t n = std::max(need_elems, b.cap() * 2);
  const hipError_t e = b.grow_doubling(need_elems);
  return e == hipSuccess ? FLEET_OK : nomem(c, "hipMalloc", n * sizeof(T), e);
}

inline int grow_pinned(fleet_ctx* c, size_t need) {
  const size_t n = std::max(need, c->h_stage.cap() * 2);
  const hipError_t e = c->h_stage.grow_doubling(need);
  return e == hipSuccess ? FLEET_OK : nomem(c, "hipHostMalloc", n, e);
}

inline size_t round16(size_t x) { return (x + 15) / 16 * 16; }
inline size_t groups_of(size_t n_values) { return (n_values + 2) / 3; }

// Device-resident entry points run on the caller's stream; NULL is the null
// (default) stream, as in the HIP libraries. Host-buffer entry points use the
// context's own stream.
inline hipStream_t pick(fleet_ctx*, void* s) { return (hipStream_t)s; }

// defined once, in fleet_codec.cpp
int check_text_len(fleet_ctx* c, size_t len);
int read_err(fleet_ctx* c, hipStream_t s, int* d_errbuf = nullptr);
int check_header_positions(fleet_ctx* c, const int32_t* header_pos, int n_headers, size_t n);

}  // namespace host
}  // namespace fleet

// fleet_amd/csrc/stream_state.cpp -- streaming aggregation behind the C-ABI: the accumulator
// (fleet_acc), the upload pool (fleet_pool) and the arrival gate (fleet_gate), over the
// kernels of acc_kernels.hip. The pool's layout is in pool_state.h, for the Kardam handles.
#include <cstring>

#include "pool_state.h"
#include "codec_math.h"

using namespace fleet::host;

namespace {

constexpr size_t kAccPiece = 1 << 20;  // host rows: copy and DMA overlap in pieces

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

}  // namespace

// A host finish's outputs from the spare device buffers that hold them, d_out and d_f32,
// to the caller's buffers on `s`. The two hold the window alone: the kernel, which
// addresses its outputs by the whole upload's group index, was given them shifted back
// by the window's start.
int fleet::host::window_read_back(fleet_ctx* c, const Window& w, const uint8_t* d_out, const float* d_f32, char* merged,
                                  float* merged_f32, hipStream_t s) {
  const size_t v0 = 3 * w.gb, v1 = std::max(v0, std::min(w.n, 3 * w.ge));
  if (w.width) HIP_TRY(c, hipMemcpyAsync(merged + w.col0, d_out, w.width, hipMemcpyDeviceToHost, s));
  if (merged_f32 && v1 > v0)
    HIP_TRY(c, hipMemcpyAsync(merged_f32 + v0, d_f32, sizeof(float) * (v1 - v0), hipMemcpyDeviceToHost, s));
  return FLEET_OK;
}

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

// ---------------------------------------------------------------- upload pool (struct fleet_pool: pool_state.h)

static int pool_slot_arg(fleet_pool* p, int slot, const char* what) {
  if (slot < 0 || slot >= p->slots) return fail(p->c, FLEET_ERR_ARG, "%s: slot %d outside [0, %d)", what, slot, p->slots);
  return FLEET_OK;
}

// FLEET_ERR_ARG before anything is launched: a pick outside the pool, of an empty slot, or repeated
int fleet::host::pool_update_args(fleet_pool* p, const int32_t* picks, int K, const char* what) {
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
int fleet::host::pool_fold(fleet_pool* p, const int32_t* picks, int K, const double* dampen, hipStream_t s,
                           uint8_t* d_merged, float* d_f32) {
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
int fleet::host::pool_verdict(fleet_pool* p, const int32_t* picks, int K) {
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


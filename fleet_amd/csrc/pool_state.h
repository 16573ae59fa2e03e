// fleet_amd/csrc/pool_state.h -- the upload pool as its own unit (stream_state.cpp) and the
// Kardam handles beside it (kardam_state.cpp) see it: the ledger, the filter and the gate
// read and write the pool's members. Internal, as host_ctx.h.
#pragma once

#include "host_ctx.h"
#include "kernels.h"

namespace fleet {
namespace host FLEET_MEM_LOCAL {

// The part of an upload that an accumulator or a pool keeps: the groups [gb, ge) of
// uploads of `len` characters (n values), bytes [col0, col0 + width) of the text. Rows
// and state on the device hold the window alone; merged outputs are addressed by the
// whole upload (kernels.h).
struct Window {
  size_t len = 0, n = 0, gb = 0, ge = 0, ng = 0, col0 = 0, width = 0;
  int n_hdr = 0;
  DevBuf<int32_t> d_hdr;     // {0, count, walk_end, 0, positions}
  DevBuf<int32_t> d_hfirst;  // the batch's first upload's header codes
  size_t row_bytes() const { return 16 * ng + 64; }
  size_t state_bytes() const { return sizeof(float) * 3 * ng + 64; }
  fleet::AccWindow launch() const { return {(int64_t)n, (int64_t)gb, (int64_t)ge, d_hdr, d_hfirst}; }
};

// Device-side calls still in flight on the caller's stream.
struct InFlight {
  bool pending = false;
  hipStream_t stream = nullptr;
  void on(hipStream_t s) { pending = true, stream = s; }
  void done() { pending = false; }  // the caller synchronised `stream` itself
};

// Waits for them, unless they run on `same`, which orders the caller's next work itself.
inline int settle(fleet_ctx* c, InFlight* f, hipStream_t same, bool wait) {
  if (f->pending && (wait || f->stream != same)) {
    HIP_TRY(c, hipStreamSynchronize(f->stream));
    f->done();
  }
  return FLEET_OK;
}

}  // namespace host
}  // namespace fleet

// The reference's `acc` for staleSize > 0 (CppNNUpdater.java:394-407) kept in HBM: uploads
// go into slots when they arrive, an update folds any subset of the slots in any order
// (k_pool_fold) and leaves every slot as it was. d_rows holds slots + 1 rows of the
// window's bytes: row `slots` receives the host update's merged bytes, whose fp32 go over
// the state (the finish launch reads a lane's 12 bytes before it writes them).
struct FLEET_MEM_LOCAL fleet_pool {
  fleet_ctx* c = nullptr;
  fleet::host::Window w;
  size_t pitch = 0;
  int slots = 0;
  fleet::DevBuf<uint8_t> d_rows;
  fleet::DevBuf<float> d_state;   // the running value between the launches of an update of more than kAccBurst picks
  fleet::DevBuf<int> d_status;    // one error word per slot, cleared by every update
  fleet::PinBuf<int> h_status;    // what the last update left in d_status
  fleet::PinBuf<uint8_t> h_row;   // a host put's way in
  std::vector<uint8_t> occupied;
  std::vector<uint8_t> seen;  // update: the picks so far
  fleet::host::InFlight fly;  // device puts
};

namespace fleet {
namespace host FLEET_MEM_LOCAL {

// what an update of the pool's is made of (stream_state.cpp); the ledger's and the filter's
// updates are the same steps around launches of their own
int window_read_back(fleet_ctx* c, const Window& w, const uint8_t* d_out, const float* d_f32, char* merged,
                     float* merged_f32, hipStream_t s);
int pool_update_args(fleet_pool* p, const int32_t* picks, int K, const char* what);
int pool_fold(fleet_pool* p, const int32_t* picks, int K, const double* dampen, hipStream_t s, uint8_t* d_merged,
              float* d_f32);
int pool_verdict(fleet_pool* p, const int32_t* picks, int K);

}  // namespace host
}  // namespace fleet

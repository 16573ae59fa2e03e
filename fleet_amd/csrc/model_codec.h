// fleet_amd/csrc/model_codec.h -- internal launchers of the DISTILLATION_MODE=1
// model codec (model_codec.hip <-> fleet_codec.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace fleet {
// pieces of a workspace: 256-byte aligned, laid out from base (nullptr: sizes only)
struct Carver {
  uint8_t* base;
  size_t at = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + at) : nullptr;
    at += (sizeof(T) * (count ? count : 1) + 255) & ~(size_t)255;
    return p;
  }
};

// A caller-owned workspace of the dictionary pipeline for models of up to n
// weights in n_mats matrices: every buffer model_quantize_index would allocate,
// the rocPRIM temporary storage included. model_dict_ws_carve lays it out from
// `base` (256-byte aligned pieces) and returns the bytes it takes; with
// base == nullptr it only sizes. 0 on a rocPRIM sizing error.
struct DictWs {
  int64_t* off;
  int32_t* dims;
  void* prm;
  uint32_t *key, *key2;
  int32_t *idx, *sidx, *start, *cid, *cbeg, *creator, *scratch, *rank, *flag32;
  uint8_t* is_creator;
  void* tmp;
  size_t tmp_bytes;
};
size_t model_dict_ws_carve(void* base, int64_t n, int n_mats, DictWs* ws);
// The same for the text emitters (model_values_text_ws, model_index_text_ws) over up to n values.
struct TextWs {
  int64_t *len, *pos;
  void* cell;  // 16 bytes per value
  void* tmp;
  size_t tmp_bytes;
};
size_t model_text_ws_carve(void* base, int64_t n, TextWs* ws);

// quantization_weight_model + dictionary + selected-index set on the device.
// d_w: n weights (n = sum of cols*rows*chans over h_dims); outputs d_wq[n],
// d_dict[n] (first *h_U entries used), d_index[n] (nullable). Synchronous.
// quantize = false: the dictionary of d_w itself (d_wq unused). With a
// workspace nothing is allocated (the scalar read-backs stay).
hipError_t model_quantize_index(const float* d_w, const int32_t* h_dims, int n_mats, float* d_wq, float* d_dict,
                                int32_t* d_index, int32_t* h_U, hipStream_t s, bool quantize = true,
                                const DictWs* ws = nullptr);
// w[i] = vals[index[i]] (0.0f for index -1)
hipError_t model_dict_gather(const int32_t* d_index, int64_t n, const float* d_vals, float* d_w, hipStream_t s);
// v[i] = strtof(sprintf("%.6g", v[i])) in place (decimal6.h: getParams' `<<` and
// read's `>>` of a value); *d_bad |= 1 for a non-finite value
hipError_t model_g6_inplace(float* d_v, int64_t n, int* d_bad, hipStream_t s);
// the index lines of getParams' mode-1 section, formatted on the device
hipError_t model_index_text(const int32_t* d_index, const int32_t* h_dims, int n_mats, std::vector<char>* out,
                            hipStream_t s);
// `ostream << float` text of n device values, formatted on the device (decimal6.h
// g6_text). n_blocks > 0: h_off[n_blocks + 1] block offsets, "value " per value
// and '\n' after each block (bias lines, mode-0 weight lines; an empty block
// prints its lone '\n'). n_blocks == 0: "i\nvalue\n" pairs (the mode-1
// dictionary section). Synchronous.
hipError_t model_values_text(const float* d_v, int64_t n, const int64_t* h_off, int n_blocks, std::vector<char>* out,
                             hipStream_t s);
// The same into a device buffer, from a caller-owned workspace and device block
// offsets d_off[n_blocks + 1] (no run of more than 254 empty blocks: the caller
// checks). Writes at d_out, at most cap bytes (hipErrorOutOfMemory beyond, with
// nothing written); *h_total = the bytes the text takes. n > 0. Synchronous.
hipError_t model_values_text_ws(const float* d_v, int64_t n, const int64_t* d_off, int n_blocks, const TextWs& ws,
                                char* d_out, int64_t cap, int64_t* h_total, hipStream_t s);
// The index lines likewise (no empty matrix: every non-null W has weights).
hipError_t model_index_text_ws(const int32_t* d_index, int64_t n, const int64_t* d_off, int n_mats, const TextWs& ws,
                               char* d_out, int64_t cap, int64_t* h_total, hipStream_t s);
// parse the index lines (device text) into weights: w[t] = value of key token t
// (std::map semantics: 0.0f for an absent key). *h_status: 0 ok, 1 malformed
// token, 2 token count != n_w.
hipError_t model_read_index(const uint8_t* d_text, int64_t len, int64_t n_w, const int32_t* d_keys,
                            const float* d_vals, int32_t n_keys, float* d_w, int* h_status, hipStream_t s);
}  // namespace fleet

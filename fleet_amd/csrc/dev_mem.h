// fleet_amd/csrc/dev_mem.h -- the one owner of device and pinned memory in the host library.
//
// Host-only and header-only: every hipMalloc / hipFree / hipHostMalloc / hipHostFree of the
// library is made here. A buffer frees its allocation when it dies or is reset; an
// allocation that a captured graph or a launch on another stream may still use is handed
// to a Retired list on growth instead and lives as long as that list. The operations
// return hipError_t: the call sites keep their own error codes and messages.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

// (hidden: inline members of these types add no dynamic symbol to the library)
#define FLEET_MEM_LOCAL __attribute__((visibility("hidden")))

namespace fleet {

namespace mem_detail {
template <typename T>
constexpr size_t elem_size() { return sizeof(T); }
template <>
constexpr size_t elem_size<void>() { return 1; }  // byte slabs
constexpr size_t kGrowPad = 64;  // the doubling policy's slack after the last element
}  // namespace mem_detail

// Device allocations kept alive after their buffer grew; freed when the list dies.
class FLEET_MEM_LOCAL Retired {
 public:
  Retired() = default;
  Retired(const Retired&) = delete;
  Retired& operator=(const Retired&) = delete;
  ~Retired() {
    for (void* p : v_) (void)hipFree(p);
  }
  void push(void* p) {
    if (p) v_.push_back(p);
  }
  size_t size() const { return v_.size(); }

 private:
  std::vector<void*> v_;
};

// One hipMalloc allocation: pointer and capacity in elements (bytes for void). Move-only.
template <typename T>
class FLEET_MEM_LOCAL DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }  // reads as the raw pointer did: d + off, d[i], if (d)
  size_t cap() const { return cap_; }
  void reset() {
    if (p_) (void)hipFree((void*)p_);
    p_ = nullptr;
    cap_ = 0;
  }

  // exactly n elements and pad_bytes more; what the buffer held is freed first
  hipError_t alloc(size_t n, size_t pad_bytes = 0) {
    reset();
    const hipError_t e = hipMalloc((void**)&p_, bytes(n) + pad_bytes);
    if (e != hipSuccess) p_ = nullptr;
    else cap_ = n;
    return e;
  }
  // the same, zero-filled (pad included); the allocation stays owned if the fill fails
  hipError_t alloc_zero(size_t n, size_t pad_bytes = 0) {
    const hipError_t e = alloc(n, pad_bytes);
    return e != hipSuccess ? e : hipMemset((void*)p_, 0, bytes(n) + pad_bytes);
  }
  // need <= cap: nothing. Else the old allocation is freed, then max(need, 2 * cap) elements
  // and 64 bytes are allocated. A failure leaves the buffer empty.
  hipError_t grow_doubling(size_t need) {
    if (need <= cap_) return hipSuccess;
    const size_t n = need > 2 * cap_ ? need : 2 * cap_;
    return alloc(n, mem_detail::kGrowPad);
  }
  // need <= cap: nothing. Else the old allocation is freed, or handed to `retire`, and
  // exactly need elements and pad_bytes are allocated. A failure leaves the buffer empty.
  hipError_t grow_exact(size_t need, size_t pad_bytes = 0, Retired* retire = nullptr) {
    if (need <= cap_) return hipSuccess;
    if (retire) {
      retire->push((void*)p_);
      p_ = nullptr;
    }
    return alloc(need, pad_bytes);
  }

 private:
  static size_t bytes(size_t n) { return n * mem_detail::elem_size<T>(); }
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// The same over hipHostMalloc(..., hipHostMallocDefault) and hipHostFree: pinned host memory.
template <typename T>
class FLEET_MEM_LOCAL PinBuf {
 public:
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~PinBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }
  void reset() {
    if (p_) (void)hipHostFree((void*)p_);
    p_ = nullptr;
    cap_ = 0;
  }

  hipError_t alloc(size_t n, size_t pad_bytes = 0) {
    reset();
    const hipError_t e = hipHostMalloc((void**)&p_, bytes(n) + pad_bytes, hipHostMallocDefault);
    if (e != hipSuccess) p_ = nullptr;
    else cap_ = n;
    return e;
  }
  hipError_t grow_doubling(size_t need) {
    if (need <= cap_) return hipSuccess;
    const size_t n = need > 2 * cap_ ? need : 2 * cap_;
    return alloc(n, mem_detail::kGrowPad);
  }
  hipError_t grow_exact(size_t need, size_t pad_bytes = 0) {
    if (need <= cap_) return hipSuccess;
    return alloc(need, pad_bytes);
  }

 private:
  static size_t bytes(size_t n) { return n * mem_detail::elem_size<T>(); }
  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace fleet

// The owners of everything the host code takes from the HIP runtime: device memory, pinned host memory, events and streams.
// A handle declares its resources as members of these types and its destroy function is `delete`; a local's destructor runs on
// every way out of its function.  Move-only; no pooling and no stream-ordered allocation: an owner calls the runtime's plain
// allocate / create once and its release / destroy once.  Kernels and their argument structs take raw pointers, through get();
// a raw pointer member of a handle is therefore a view or a borrowed pointer, never an allocation.
// These are the only calls of the runtime's allocate / create / release functions (tests/test_device_ownership.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>
#include <vector>

#include "../common.hpp"

#define HIP_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t _e = (expr);                                                                               \
    if (_e != hipSuccess)                                                                                 \
      return rdoom::fail(_e == hipErrorOutOfMemory ? RDOOM_OOM : RDOOM_HIP_ERROR, "%s failed: %s", #expr, \
                         hipGetErrorString(_e));                                                          \
  } while (0)

namespace rdoom {

// what one resource kind needs of an owner: the handle, the moves, the release
template <class Handle, class Release>
class Owner {
 public:
  Owner() = default;
  Owner(Owner &&o) noexcept : h_(std::exchange(o.h_, Handle{})) {}
  Owner &operator=(Owner &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, Handle{});
    }
    return *this;
  }
  ~Owner() { reset(); }
  Handle get() const { return h_; }
  explicit operator bool() const { return h_ != Handle{}; }
  void reset() {
    if (h_ != Handle{}) Release{}(h_);
    h_ = Handle{};
  }

 protected:
  Handle h_{};
};

struct DeviceRelease {
  void operator()(void *p) const { (void)hipFree(p); }
};
struct PinnedRelease {
  void operator()(void *p) const { (void)hipHostFree(p); }
};
struct EventRelease {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
struct StreamRelease {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};

// the bytes the world units give an empty table: a valid pointer nobody reads (upload's `empty_bytes`)
constexpr size_t EMPTY_TABLE_BYTES = 16;

// Device memory on the device that is current at the allocation.  An allocation that is already there is kept: a member that is
// allocated on first use calls alloc each time.
template <class T>
class DeviceArray : public Owner<T *, DeviceRelease> {
 public:
  rdoom_status alloc_bytes(size_t bytes) {
    if (!this->h_) HIP_TRY(hipMalloc((void **)&this->h_, bytes));
    return RDOOM_OK;
  }
  rdoom_status alloc(size_t count) { return alloc_bytes(count * sizeof(T)); }
  // `count` elements from the host.  An empty table stays a null pointer, or is `empty_bytes` that are never written
  rdoom_status upload(const T *src, size_t count, size_t empty_bytes = 0) {
    if (!count && !empty_bytes) return RDOOM_OK;
    if (rdoom_status s = alloc_bytes(count ? count * sizeof(T) : empty_bytes)) return s;
    if (count) HIP_TRY(hipMemcpy(this->h_, src, count * sizeof(T), hipMemcpyHostToDevice));
    return RDOOM_OK;
  }
  rdoom_status upload(const std::vector<T> &src, size_t empty_bytes = 0) { return upload(src.data(), src.size(), empty_bytes); }
};

// page-locked host memory
template <class T>
class PinnedArray : public Owner<T *, PinnedRelease> {
 public:
  rdoom_status alloc(size_t count) {
    if (!this->h_) HIP_TRY(hipHostMalloc((void **)&this->h_, count * sizeof(T), hipHostMallocDefault));
    return RDOOM_OK;
  }
};

class Event : public Owner<hipEvent_t, EventRelease> {
 public:
  rdoom_status create() {
    if (!h_) HIP_TRY(hipEventCreate(&h_));
    return RDOOM_OK;
  }
};

class Stream : public Owner<hipStream_t, StreamRelease> {
 public:
  rdoom_status create(unsigned flags) {
    if (!h_) HIP_TRY(hipStreamCreateWithFlags(&h_, flags));
    return RDOOM_OK;
  }
};

}  // namespace rdoom

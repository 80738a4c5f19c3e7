// Device memory, pinned memory, streams and events as owned members
// ("Ownership"): the HIP side of owner.h, and HIPCHK.
//
// In a handle the Stream is declared BEFORE the buffers and events that work
// on it: members are destroyed in reverse order, so the stream goes last.
// A handle's destroy function synchronises the stream before it deletes.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "../../include/sfm_amd.h"
#include "owner.h"
#include "sfm_error.h"

// 0, or `code` with "<what>: <error>" for the HIP error e (a hipError_t, or a memory policy's int)
inline int hip_rc(int code, const char* what, int e) {
  return e ? fail(code, std::string(what) + ": " + hipGetErrorString(hipError_t(e))) : 0;
}
#define HIPCHK(expr)                                                   \
  do {                                                                 \
    if (const int rc_ = hip_rc(SFM_EIO, #expr, int(expr))) return rc_; \
  } while (0)

namespace sfm {

struct DeviceMem {
  using Stream = hipStream_t;
  static int alloc(void** p, size_t bytes) { return int(hipMalloc(p, bytes)); }
  static void release(void* p) { (void)hipFree(p); }
  static int drain(hipStream_t s) { return int(hipStreamSynchronize(s)); }
  static int copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
    return int(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  }
};
struct PinnedMem {
  using Stream = hipStream_t;
  static int alloc(void** p, size_t bytes) { return int(hipHostMalloc(p, bytes)); }
  static void release(void* p) { (void)hipHostFree(p); }
  static int drain(hipStream_t s) { return int(hipStreamSynchronize(s)); }
};
using DevBuf = Buf<DeviceMem>;
using PinBuf = Buf<PinnedMem>;
using DevPool = Pool<DeviceMem>;
// a Buf that kernels, copies and pointer arithmetic take as a T*
template <typename T, typename Mem>
struct Arr : Buf<Mem> {
  operator T*() const { return this->template as<T>(); }
  T* operator->() const { return this->template as<T>(); }
};
template <typename T>
using DevArr = Arr<T, DeviceMem>;
template <typename T>
using PinArr = Arr<T, PinnedMem>;

// Move-only owner of a stream; the destructor waits for its work first.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s_, o.s_);
    return *this;
  }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (!s_) return;
    (void)hipStreamSynchronize(s_);
    (void)hipStreamDestroy(s_);
  }
  hipError_t create(unsigned flags) { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, flags); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(e_, o.e_);
    return *this;
  }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  hipError_t create(unsigned flags) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace sfm

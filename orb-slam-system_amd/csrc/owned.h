// owned.h -- the GPU resources a long-lived handle holds, owned by type: a
// member is declared once, acquired through alloc() / create(), and released
// when its handle is deleted (or by reset(), or when it is acquired again).
// An owner converts to the raw pointer / stream / event it holds, so it is
// used like one.  The resource is released on whichever device is current:
// a handle's destructor selects its device first.
#ifndef ORBX_OWNED_H
#define ORBX_OWNED_H

#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/orbx.h"

namespace orbx {

enum { OWN_DEVICE = 0, OWN_PINNED, OWN_STREAM, OWN_EVENT, OWN_KINDS };

// owned resources alive in the process, per kind (orbx_debug_live_resources)
inline std::atomic<int> g_own_live[OWN_KINDS];
// orbx_debug_fail_acquire: this thread's acquisitions left before one fails
inline thread_local int g_own_fail_in = 0;

// H: a pointer-like handle, null when empty; Destroy releases one
template <class H, void (*Destroy)(H), int Kind>
class Owned {
 public:
  Owned() = default;
  ~Owned() { reset(); }
  Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = H(); }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = H();
    }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;

  operator H() const { return h_; }
  void reset() {
    if (!h_) return;
    Destroy(h_);
    g_own_live[Kind].fetch_sub(1, std::memory_order_relaxed);
    h_ = H();
  }

 protected:
  // releases what is held, then holds what make(&h) produced (true = made)
  template <class Make>
  int acquire(Make&& make) {
    reset();
    if (g_own_fail_in > 0 && --g_own_fail_in == 0) return ORBX_ERR_HIP;
    H h = H();
    if (!make(&h)) return ORBX_ERR_HIP;
    h_ = h;
    g_own_live[Kind].fetch_add(1, std::memory_order_relaxed);
    return ORBX_OK;
  }

 private:
  H h_ = H();
};

template <class T>
inline void dev_destroy(T* p) { (void)hipFree(p); }
template <class T>
inline void pinned_destroy(T* p) { (void)hipHostFree(p); }
inline void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
inline void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }

// n elements of device memory (at least 16 bytes)
template <class T>
struct DevBuf : Owned<T*, dev_destroy<T>, OWN_DEVICE> {
  int alloc(size_t n) {
    return this->acquire([n](T** p) { return hipMalloc((void**)p, n ? n * sizeof(T) : 16) == hipSuccess; });
  }
};

// n elements of pinned host memory
template <class T>
struct PinnedBuf : Owned<T*, pinned_destroy<T>, OWN_PINNED> {
  int alloc(size_t n) {
    return this->acquire(
        [n](T** p) { return hipHostMalloc((void**)p, n * sizeof(T), hipHostMallocDefault) == hipSuccess; });
  }
};

// a non-blocking stream
struct Stream : Owned<hipStream_t, stream_destroy, OWN_STREAM> {
  int create() {
    return acquire([](hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess; });
  }
};

struct Event : Owned<hipEvent_t, event_destroy, OWN_EVENT> {
  int create(unsigned flags = hipEventDefault) {
    return acquire([flags](hipEvent_t* e) { return hipEventCreateWithFlags(e, flags) == hipSuccess; });
  }
};

}  // namespace orbx

// The two debug entry points (include/orbx.h) read and arm the bookkeeping
// above; `used` keeps the one definition every translation unit shares.
extern "C" __attribute__((used)) inline int orbx_debug_live_resources(int counts[4]) {
  if (!counts) return ORBX_ERR_ARG;
  for (int k = 0; k < orbx::OWN_KINDS; ++k) counts[k] = orbx::g_own_live[k].load(std::memory_order_relaxed);
  return ORBX_OK;
}

extern "C" __attribute__((used)) inline int orbx_debug_fail_acquire(int nth) {
  orbx::g_own_fail_in = nth > 0 ? nth : 0;
  return ORBX_OK;
}

#endif

// call_arena.h -- the typed per-call arena of the synchronous drop-in entry
// points: the whole protocol over a pooled CallWs (api_common.h) in one class.
//
//   CallArena A(device);            // leases a workspace
//   auto a = A.in(src, n);          // input: copied into staging by upload()
//   auto t = A.in<Table>(k);        //   ... or built in place through A.h(t)
//   auto v = A.in_opt(valid, n);    //   ... or absent: no space, A.d(v) == nullptr
//   auto r = A.out(dst, n);         // output: copied to dst by finish()
//   auto s = A.scratch<int2>(rows); // device-only
//   A.commit();                     // the one reserve; h() / d() valid from here
//   A.upload();                     // [0, in_end) up in one stage_in
//   launch<<<.., A.stream()>>>(A.d(a), A.d(r), A.d(s));
//   return A.finish();              // [in_end, out_end) back in one finish_call
//
// Slots are 256-byte aligned, in declaration order.  That order must be inputs,
// outputs, scratch -- the upload and the download are one range each -- and a
// slot declared out of order traps.
#ifndef ORBX_CALL_ARENA_H
#define ORBX_CALL_ARENA_H

#include <string.h>

#include <vector>

#include "api_common.h"

namespace orbx {

// n elements of T at byte offset off.  A default-constructed slot is an absent
// optional one: no space, nullptr on both sides
template <class T>
struct Slot {
  size_t off = 0, n = 0;
  bool present = false;
  size_t bytes() const { return n * sizeof(T); }
};

class CallArena {
 public:
  // leases a pooled workspace of `device` (after hipSetDevice); !ok() on failure
  explicit CallArena(int device) : w_(ws_acquire(device)), leased_(true) {}
  // over a workspace the caller owns (host tests: both buffers preallocated)
  explicit CallArena(CallWs* w) : w_(w), leased_(false) {}
  ~CallArena() {
    if (leased_ && w_) ws_release(w_);
  }
  CallArena(const CallArena&) = delete;
  CallArena& operator=(const CallArena&) = delete;

  bool ok() const { return w_ != nullptr; }
  hipStream_t stream() const { return w_->stream; }

  template <class T>
  Slot<T> in(size_t n) { return take<T>(kIn, n, nullptr, nullptr); }
  template <class T>
  Slot<T> in(const T* src, size_t n) { return take<T>(kIn, n, src, nullptr); }
  template <class T>
  Slot<T> in_opt(const T* src, size_t n) { return src ? in(src, n) : Slot<T>(); }
  template <class T>
  Slot<T> out(T* dst, size_t n) { return take<T>(kOut, n, nullptr, dst); }
  template <class T>
  Slot<T> scratch(size_t n) { return take<T>(kScratch, n, nullptr, nullptr); }

  // the device arena holds everything, the pinned staging buffer the inputs
  // and outputs.  ORBX_OK or ORBX_ERR_HIP
  int commit() {
    enter(kCommitted);
    return w_->reserve(off_, out_end_);
  }
  size_t in_end() const { return in_end_; }
  size_t out_end() const { return out_end_; }
  size_t total() const { return off_; }
  // a slot in the pinned staging buffer (inputs and outputs only) ...
  template <class T>
  T* h(const Slot<T>& s) const {
    require(phase_ == kCommitted && s.off + s.bytes() <= out_end_);
    return s.present ? reinterpret_cast<T*>(w_->h + s.off) : nullptr;
  }
  // ... and in the device arena
  template <class T>
  T* d(const Slot<T>& s) const {
    require(phase_ == kCommitted);
    return s.present ? reinterpret_cast<T*>(w_->d + s.off) : nullptr;
  }

  // the host halves of upload() and finish(): declared sources into staging,
  // staged outputs to their destinations
  void gather() const {
    for (const Copy& c : copies_)
      if (c.src) memcpy(w_->h + c.off, c.src, c.bytes);
  }
  void scatter() const {
    for (const Copy& c : copies_)
      if (c.dst) memcpy(c.dst, w_->h + c.off, c.bytes);
  }
  int upload() const {
    gather();
    return stage_in(w_->d, w_->h, in_end_, w_->stream);
  }
  // launch errors so far, the download, the completion wait, the outputs
  int finish() const {
    const int rc = finish_call(w_, in_end_, out_end_);
    if (rc == ORBX_OK) scatter();
    return rc;
  }

 private:
  enum Phase { kIn, kOut, kScratch, kCommitted };
  struct Copy {
    size_t off, bytes;
    const void* src;
    void* dst;
  };

  static void require(bool cond) {
    if (!cond) __builtin_trap();
  }
  // phases only move forward; in_end / out_end are fixed when theirs is left
  void enter(Phase p) {
    require(phase_ != kCommitted && p >= phase_);
    if (phase_ < kOut && p >= kOut) in_end_ = off_;
    if (phase_ < kScratch && p >= kScratch) out_end_ = off_;
    phase_ = p;
  }
  template <class T>
  Slot<T> take(Phase p, size_t n, const void* src, void* dst) {
    enter(p);
    const Slot<T> s = {off_, n, true};
    off_ += (s.bytes() + 255) & ~(size_t)255;
    if (n && (src || dst)) copies_.push_back({s.off, s.bytes(), src, dst});
    return s;
  }

  CallWs* w_;
  bool leased_;
  Phase phase_ = kIn;
  size_t off_ = 0, in_end_ = 0, out_end_ = 0;
  std::vector<Copy> copies_;
};

}  // namespace orbx

#endif

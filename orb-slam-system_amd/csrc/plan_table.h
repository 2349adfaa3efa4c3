// plan_table.h -- what the asynchronous plan forms on device pointers share
// (orbm_proj_plan, orbm_kf_plan, orbm_pose_plan): a problem
// table with its pinned staging, and the two events that order one call of a
// plan against the next.  Host only.
//
// A call runs  fence.begin(s) / fill the tables' rows / table.upload(n, s) per
// table / fence.staged(s) / the launches / fence.end(s).
#ifndef ORBX_PLAN_TABLE_H
#define ORBX_PLAN_TABLE_H

#include "api_common.h"

namespace orbx {

// a device table and the pinned rows it is filled from: both held, or neither
template <class T, class Dev = DevBuf<T>, class Host = PinnedBuf<T>>
class PlanTable {
 public:
  // n rows each, the device's first; a failure leaves the table empty
  int alloc(size_t n) {
    if (d_.alloc(n) == ORBX_OK && h_.alloc(n) == ORBX_OK) return ORBX_OK;
    reset();
    return ORBX_ERR_HIP;
  }
  void reset() {
    d_.reset();
    h_.reset();
  }
  explicit operator bool() const { return d_ && h_; }
  T& operator[](size_t i) { return h_[i]; }  // a staging row
  T* host() { return h_; }
  const T* dev() const { return d_; }
  // the first n staging rows into the device table, ordered on s
  int upload(size_t n, hipStream_t s) {
    ORBX_TRY(hipMemcpyAsync(d_, h_, n * sizeof(T), hipMemcpyHostToDevice, s));
    return ORBX_OK;
  }

 private:
  Dev d_;
  Host h_;
};

// The order between two calls of one plan.  Every call refills the plan's
// pinned staging and reuses its device side (problem tables, grids,
// candidates, query rows), on whichever stream the caller names.
struct PlanFence {
  int create() {
    return (staged_.create(hipEventDisableTiming) || done_.create(hipEventDisableTiming)) ? ORBX_ERR_HIP : ORBX_OK;
  }
  // before the rows are filled.  The host waits until the previous call's
  // tables have left the staging.  The device side is still read by that
  // call's kernels: a call on another stream than theirs must not overwrite
  // it under them, so the stream waits for them on the device,
  // with no host block
  int begin(hipStream_t s) {
    ORBX_TRY(hipEventSynchronize(staged_));
    ORBX_TRY(hipStreamWaitEvent(s, done_, 0));
    return ORBX_OK;
  }
  // after the last upload: the staging is reusable once this has passed
  int staged(hipStream_t s) {
    ORBX_TRY(hipEventRecord(staged_, s));
    return ORBX_OK;
  }
  // after the launches: their error, then the mark the next call's stream waits for
  int end(hipStream_t s) {
    if (hipGetLastError() != hipSuccess) return ORBX_ERR_HIP;
    ORBX_TRY(hipEventRecord(done_, s));
    return ORBX_OK;
  }

 private:
  Event staged_;  // the last call's table uploads
  Event done_;    // the last call's kernels
};

}  // namespace orbx

#endif

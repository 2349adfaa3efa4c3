// api_common.h -- host helpers shared by the C-ABI translation units.
#ifndef ORBX_API_COMMON_H
#define ORBX_API_COMMON_H

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "../../include/orbx.h"
#include "owned.h"

#define ORBX_TRY(expr)                              \
  do {                                              \
    if ((expr) != hipSuccess) return ORBX_ERR_HIP;  \
  } while (0)

enum {
  ORBX_STAGE_RESIZE = 0,
  ORBX_STAGE_FAST,
  ORBX_STAGE_QUADTREE,
  ORBX_STAGE_BLUR,
  ORBX_STAGE_BRIEF,
  ORBX_STAGE_MSELECT,
  ORBX_STAGE_MCAND,
  ORBX_STAGE_MRESOLVE,
  ORBX_STAGE_MFINAL,
  ORBX_STAGE_SROWS,
  ORBX_STAGE_SMATCH,
  ORBX_STAGE_SFILTER,
  ORBX_NSTAGES
};

namespace orbx {

// HIP events recorded around every launch group of a stage, on the stream
// the kernels run on.  collect() must be called after that stream is idle.
// The timer owns its events: they go with the handle that holds it.
struct StageTimer {
  bool enabled = false;
  struct Rec {
    int stage;
    Event a, b;
  };
  std::vector<Rec> recs;
  std::vector<Event> pool;
  Event pending[ORBX_NSTAGES];

  Event get() {
    Event e;
    if (!pool.empty()) {
      e = std::move(pool.back());
      pool.pop_back();
    } else {
      e.create();
    }
    return e;
  }
  void begin(int stage, hipStream_t s) {
    if (!enabled) return;
    pending[stage] = get();
    hipEventRecord(pending[stage], s);
  }
  void end(int stage, hipStream_t s) {
    if (!enabled || !pending[stage]) return;
    Event b = get();
    hipEventRecord(b, s);
    recs.push_back({stage, std::move(pending[stage]), std::move(b)});
  }
  void reset(bool en) {
    for (auto& r : recs) {
      pool.push_back(std::move(r.a));
      pool.push_back(std::move(r.b));
    }
    recs.clear();
    enabled = en;
  }
  int collect(double* ms, int* launches, int n) {
    for (int i = 0; i < n; ++i) {
      if (ms) ms[i] = 0;
      if (launches) launches[i] = 0;
    }
    for (auto& r : recs) {
      float t = 0;
      if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) return ORBX_ERR_HIP;
      if (r.stage < n) {
        if (ms) ms[r.stage] += t;
        if (launches) launches[r.stage] += 1;
      }
    }
    reset(enabled);
    return ORBX_OK;
  }
};

// fills dst from v (room for at least one element): a blocking copy, or one
// ordered on stream s, which v must outlive
template <typename T>
int upload(DevBuf<T>& dst, const std::vector<T>& v, bool blocking, hipStream_t s = nullptr) {
  if (dst.alloc(v.size() ? v.size() : 1)) return ORBX_ERR_HIP;
  if (v.empty()) return ORBX_OK;
  const size_t bytes = v.size() * sizeof(T);
  const hipError_t e = blocking ? hipMemcpy(dst, v.data(), bytes, hipMemcpyHostToDevice)
                                : hipMemcpyAsync(dst, v.data(), bytes, hipMemcpyHostToDevice, s);
  return e == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
}

// ---------------------------------------------------------------------------
// Per-call workspaces of the synchronous drop-in entry points
// (orbm_search_by_bow, orbm_descriptor_distance_batch,
// orbm_search_by_projection, ...): a grow-only device arena, a grow-only
// pinned host staging buffer and a non-blocking stream.  Workspaces live in a
// per-device pool: a call takes one (a concurrent call takes another, so the
// entry points stay re-entrant from the Tracking / LocalMapping /
// LoopClosing threads) and returns it; steady-state calls do no hipMalloc,
// hipFree or stream creation, and never synchronise the device.
//
// An entry point does not touch a workspace's buffers itself: it declares
// typed slots on a CallArena (call_arena.h), which leases the workspace, lays
// the slots out (inputs, outputs, scratch), sizes the buffers once, and does
// the one upload (stage_in) and the one download (finish_call) below.
// ---------------------------------------------------------------------------
// Not owners (owned.h): a workspace lives as long as the process, and the
// arena's host test points d and h at plain host memory.
struct CallWs {
  int device = -1;
  hipStream_t stream = nullptr;
  uint8_t* d = nullptr;  // device arena
  size_t dcap = 0;
  uint8_t* h = nullptr;  // pinned host staging
  size_t hcap = 0;
  // grow-only; a grow waits for this workspace's stream only
  int reserve(size_t dbytes, size_t hbytes);
};

CallWs* ws_acquire(int device);  // after hipSetDevice(device); nullptr on failure
void ws_release(CallWs* w);

// Completion wait of the synchronous drop-in calls: the caller (Tracking,
// LoopClosing) blocks on the result anyway, so the stream is polled for up
// to ORBX_SPIN_US microseconds before falling back to hipStreamSynchronize,
// whose blocking wake-up showed up as 2-4x p50 outliers in the per-call
// latency (bench latency leg).
hipError_t stream_wait(hipStream_t s);

// hipFuncAttributeMaxDynamicSharedMemorySize is process-wide per kernel:
// set it once per (kernel, device) to the CU's whole LDS, never per call (a
// concurrent call writing a smaller value could undercut a larger launch).
int set_max_dynamic_lds(const void* kernel, int device);

// a drop-in call's inputs [0, bytes) from its pinned staging buffer h into
// its device arena d, on stream s: a kernel (k_stage_in, kernels_misc.hip) when
// ORBM_STAGE_KERNEL, else a DMA copy.  bytes: a multiple of 16 (CallArena's
// 256-byte slots)
int stage_in(void* d, const void* h, size_t bytes, hipStream_t s);
// its results [.., + bytes) from the device arena d back into the pinned
// staging h (device-accessible host memory): the copy kernel writing host
// memory when ORBM_STAGE_KERNEL, else a DMA copy.  bytes: a multiple of 16
int stage_out(void* h, const void* d, size_t bytes, hipStream_t s);
// the tail of a drop-in call on workspace w: launch errors so far, the
// results [out_begin, out_end) of the arena back into the staging buffer,
// then the completion wait.  ORBX_OK or ORBX_ERR_HIP
int finish_call(CallWs* w, size_t out_begin, size_t out_end);

// ORBX_OK if `device` names a visible device, else ORBX_ERR_NO_DEVICE
int check_device(int device);

// a FeatureVector over n features (nnodes nodes, node j's features
// feat[node_off[j] .. node_off[j + 1])): the three pointers non-null when
// nnodes > 0, node_id strictly ascending (std::map keys), node_off
// non-decreasing, every feat[i] < n.  ORBX_OK or ORBX_ERR_ARG
int check_feature_vector(int n, int nnodes, const uint32_t* node_id, const uint32_t* node_off,
                         const uint32_t* feat);

// merge-join of two checked FeatureVectors (ORBmatcher.cc:305-350): calls
// f(off1, n1, off2, n2), node j's list being feat[off .. off + n), for every
// common NodeId in ascending order.  A non-zero return of f ends the walk and
// is returned; otherwise ORBX_OK
template <class F>
int for_common_nodes(const uint32_t* id1, const uint32_t* off1, int nnodes1, const uint32_t* id2,
                     const uint32_t* off2, int nnodes2, F&& f) {
  for (int i = 0, j = 0; i < nnodes1 && j < nnodes2;) {
    if (id1[i] < id2[j]) {
      ++i;
    } else if (id2[j] < id1[i]) {
      ++j;
    } else {
      const int rc = f(off1[i], off1[i + 1] - off1[i], off2[j], off2[j + 1] - off2[j]);
      if (rc) return rc;
      ++i;
      ++j;
    }
  }
  return ORBX_OK;
}

// marks idx[0 .. count) in `seen` (one byte per feature): true if one of them
// was marked before, by this call or an earlier one on the same table.  An
// index past the table counts as a repeat (a caller that has not validated
// the FeatureVector yet rejects both alike)
inline bool index_repeats(std::vector<uint8_t>& seen, const uint32_t* idx, size_t count) {
  for (size_t i = 0; i < count; ++i) {
    if (idx[i] >= seen.size() || seen[idx[i]]) return true;
    seen[idx[i]] = 1;
  }
  return false;
}

}  // namespace orbx

#endif

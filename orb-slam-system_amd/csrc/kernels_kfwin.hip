// kernels_kfwin.hip -- the keyframe window search of ORBmatcher::Fuse (both
// forms) and SearchBySim3 (src/ORBmatcher.cc:532-551, :600-619, :696-714) for
// gfx950, batched over the keyframes of LocalMapping::SearchInNeighbors.
//
//   k_kfwin_grid    one workgroup per keyframe: the ix-major stable cell order
//                   of its features (PosInGrid, src/Frame.cc:362-372; index
//                   order inside a cell, as AssignFeaturesToGrid pushes them),
//                   the prefix of the cell sizes, and the features written in
//                   that order as 48-byte records;
//   k_kfwin_search  KFW_G lanes per query, queries flattened over the
//                   problems: KeyFrame::GetFeaturesInArea's cell bounds
//                   (src/KeyFrame.cc:554-568), then every column's run of
//                   records KFW_G at a time: box test, octave gate, Hamming
//                   distance, and the group minimum of distance << 16 | rank.
//
// k_kfwin_grid_kp and k_kfwin_search_plan are the same two bodies for
// orbm_kf_plan (api_kfbuild.hip): the keys read as orbx_keypoint
// rows, problems on blockIdx.y with their own queries, pool and results.
//
// The reference visits (ix, iy, position in the cell) and keeps the first
// strict minimum; a record's position in the keyframe's order ("rank") grows
// in exactly that order, so the first strict minimum is the smallest
// (distance, rank) key.  Queries never interact: nothing is claimed.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/orbx.h"
#include "kfbuild_internal.h"
#include "kfwin_internal.h"
#include "orbm_device.h"

namespace orbx {

// float -> int as the reference's x86 object converts (cvttss2si): a value
// outside int's range, or a NaN, gives INT_MIN
__device__ __forceinline__ int kfw_f2i(float v) {
  return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT_MIN;
}

// Key: the row type PP.key points at -- KfwKey as the host form uploads it, or
// orbx_keypoint (28 bytes) where the caller's mvKeysUn is on the device
template <class Key>
__device__ __forceinline__ void kfwin_grid(const KfwProblem& PP, uint32_t* sk) {
  const Key* __restrict__ keys = reinterpret_cast<const Key*>(PP.key);
  int* __restrict__ cell_off = PP.cell_off;
  if (!cell_off) return;  // a problem without queries: the whole block leaves
  int P = 1;
  while (P < PP.n) P <<= 1;
  const int tid = threadIdx.x;
  for (int i = tid; i < P; i += 1024) {
    uint32_t key = 0xFFFFFFFFu;
    if (i < PP.n) {
      const Key k = keys[i];
      const int px = kfw_f2i(roundf((k.x - PP.minX) * PP.wInv));  // PosInGrid (:364-365)
      const int py = kfw_f2i(roundf((k.y - PP.minY) * PP.hInv));
      if (!(px < 0 || px >= KFW_COLS || py < 0 || py >= KFW_ROWS))
        key = ((uint32_t)(px * KFW_ROWS + py) << 16) | (uint32_t)i;
    }
    sk[i] = key;
  }
  __syncthreads();
  // bitonic sort: P and the stage count depend on n alone (uniform barriers)
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += 1024) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint32_t x = sk[lo], y = sk[hi];
        if ((x > y) == up) {
          sk[lo] = y;
          sk[hi] = x;
        }
      }
      __syncthreads();
    }
  // cell_off[c] = the first position whose cell is >= c: position i opens
  // every cell after its predecessor's up to its own, and the first position
  // past the gridded features opens the rest (and cell_off[KFW_CELLS])
  for (int i = tid; i <= P; i += 1024) {
    const uint32_t cur = i < P ? sk[i] : 0xFFFFFFFFu;
    const uint32_t prev = i > 0 ? sk[i - 1] : 0u;
    if (i > 0 && prev == 0xFFFFFFFFu) continue;  // already past the end
    const int first = i > 0 ? (int)(prev >> 16) + 1 : 0;
    const int last = cur != 0xFFFFFFFFu ? (int)(cur >> 16) : KFW_CELLS;
    for (int c = first; c <= last; ++c) cell_off[c] = i;
  }
  const uint8_t* __restrict__ desc = PP.desc;
  KfwRec* __restrict__ rec = PP.rec;
  for (int i = tid; i < P; i += 1024) {
    const uint32_t key = sk[i];
    if (key == 0xFFFFFFFFu) continue;
    const int idx = (int)(key & 0xFFFFu);
    const Key k = keys[idx];
    const uint4* dp = reinterpret_cast<const uint4*>(desc + (size_t)idx * 32);
    const uint4 d0 = dp[0], d1 = dp[1];
    uint4* out = reinterpret_cast<uint4*>(rec + i);
    out[0] = make_uint4(__float_as_uint(k.x), __float_as_uint(k.y), (uint32_t)idx, (uint32_t)k.octave);
    out[1] = d0;
    out[2] = d1;
  }
}

__global__ __launch_bounds__(1024) void k_kfwin_grid(const KfwProblem* __restrict__ probs) {
  __shared__ uint32_t sk[KFW_MAXN];  // cell << 16 | index, 0xFFFFFFFF = in no cell
  const KfwProblem PP = probs[blockIdx.x];
  kfwin_grid<KfwKey>(PP, sk);
}

// the plan's form: one workgroup per problem, keys as orbx_keypoint rows
__global__ __launch_bounds__(1024) void k_kfwin_grid_kp(const KfwPlanProblem* __restrict__ probs) {
  __shared__ uint32_t sk[KFW_MAXN];
  const KfwProblem PP = probs[blockIdx.x].kf;
  kfwin_grid<orbx_keypoint>(PP, sk);
}

// one query by its lane group: Q's window in PP's records; lane 0 of the group
// writes best_idx[qi] / best_dist[qi]
__device__ __forceinline__ void kfwin_search_one(const KfwProblem& PP, const orbx_kf_query& Q,
                                                 const uint8_t* __restrict__ qdesc, int gl, int qi,
                                                 int32_t* __restrict__ best_idx,
                                                 int32_t* __restrict__ best_dist) {
  const uint4* qd = reinterpret_cast<const uint4*>(qdesc + (size_t)Q.desc * 32);
  const uint4 q0 = qd[0], q1 = qd[1];
  const int* __restrict__ cell_off = PP.cell_off;
  const KfwRec* __restrict__ rec = PP.rec;
  const float x = Q.x, y = Q.y, r = Q.radius;
  uint32_t best = 0xFFFFFFFFu;
  // KeyFrame::GetFeaturesInArea (:554-568): the four early returns
  const int x0 = max(0, kfw_f2i(floorf((x - PP.minX - r) * PP.wInv)));
  const int x1 = min(KFW_COLS - 1, kfw_f2i(ceilf((x - PP.minX + r) * PP.wInv)));
  const int y0 = max(0, kfw_f2i(floorf((y - PP.minY - r) * PP.hInv)));
  const int y1 = min(KFW_ROWS - 1, kfw_f2i(ceilf((y - PP.minY + r) * PP.hInv)));
  if (!(x0 >= KFW_COLS || x1 < 0 || y0 >= KFW_ROWS || y1 < 0)) {
    for (int ix = x0; ix <= x1; ++ix) {
      // cells (ix, y0..y1) are one run of the ix-major order (empty if y1 < y0)
      const int b = cell_off[ix * KFW_ROWS + y0];
      const int e = y1 >= y0 ? cell_off[ix * KFW_ROWS + y1 + 1] : b;
      for (int j = b + gl; j < e; j += KFW_G) {
        const uint4* rp = reinterpret_cast<const uint4*>(rec + j);
        const uint4 h = rp[0];
        const float distx = __uint_as_float(h.x) - x, disty = __uint_as_float(h.y) - y;
        if (!(fabsf(distx) < r && fabsf(disty) < r)) continue;  // :581
        const int octave = (int)h.w;
        if (Q.level >= 0 && (octave < Q.level - 1 || octave > Q.level)) continue;  // ORBmatcher.cc:542
        const uint4 b0 = rp[1], b1 = rp[2];
        const uint32_t d = ham256_popc(q0, q1, b0, b1);
        best = min(best, (d << 16) | (uint32_t)j);  // rank j < KFW_MAXN, d <= 256
      }
    }
  }
#pragma unroll
  for (int d = KFW_G >> 1; d >= 1; d >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, d, KFW_G));
  if (gl == 0) {
    if (best == 0xFFFFFFFFu) {
      best_idx[qi] = -1;
      best_dist[qi] = INT_MAX;
    } else {
      best_idx[qi] = rec[best & 0xFFFFu].index;
      best_dist[qi] = (int32_t)(best >> 16);
    }
  }
}

__global__ __launch_bounds__(KFW_BLOCK) void k_kfwin_search(
    const KfwProblem* __restrict__ probs, const orbx_kf_query* __restrict__ qs,
    const int32_t* __restrict__ qoff, const int32_t* __restrict__ blk_prob,
    const uint8_t* __restrict__ qdesc, int nq, int32_t* __restrict__ best_idx,
    int32_t* __restrict__ best_dist) {
  const int gl = threadIdx.x & (KFW_G - 1);
  const int qi = blockIdx.x * (KFW_BLOCK / KFW_G) + (threadIdx.x / KFW_G);
  if (qi >= nq) return;  // whole groups leave: the shuffles below stay inside a group
  // the problem of the block's first query comes from the host's table; the
  // few problem boundaries inside a block are walked (qi < nq = qoff[nprob])
  int p = blk_prob[blockIdx.x];
  while (qi >= qoff[p + 1]) ++p;
  const KfwProblem PP = probs[p];
  const orbx_kf_query Q = qs[qi];
  kfwin_search_one(PP, Q, qdesc, gl, qi, best_idx, best_dist);
}

// the plan's form: problems on blockIdx.y, each with its own queries, pool
// and results (no flattening, so no offset or block tables).  A desc outside
// the problem's pool is answered like an empty window, without a read
__global__ __launch_bounds__(KFW_BLOCK) void k_kfwin_search_plan(const KfwPlanProblem* __restrict__ probs) {
  const KfwPlanProblem& PL = probs[blockIdx.y];
  const int nq = PL.nq;
  const int gl = threadIdx.x & (KFW_G - 1);
  const int qi = blockIdx.x * (KFW_BLOCK / KFW_G) + (threadIdx.x / KFW_G);
  if (qi >= nq) return;  // whole groups leave
  const KfwProblem PP = PL.kf;
  const orbx_kf_query Q = PL.qs[qi];
  if ((uint32_t)Q.desc >= (uint32_t)nq) {  // uniform over the group
    if (gl == 0) {
      PL.best_idx[qi] = -1;
      PL.best_dist[qi] = INT_MAX;
    }
    return;
  }
  kfwin_search_one(PP, Q, PL.qdesc, gl, qi, PL.best_idx, PL.best_dist);
}

}  // namespace orbx

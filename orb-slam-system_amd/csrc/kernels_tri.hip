// kernels_tri.hip -- ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:
// 368-467) and CheckDistEpipolarLine (:71-85) for gfx950, batched over the
// neighbour keyframes of one KeyFrame.
//
//   k_tri_init      every problem's per-row results to "no match", its
//                   rotation histogram to zero;
//   k_tri_search    one wavefront per item (problem, node pair, 64 KF1 rows),
//                   one lane per row: the node's KF2 list goes through LDS in
//                   chunks of TRI_CHUNK and every lane walks it in list order;
//   k_tri_finalize  one workgroup per problem: ComputeThreeMaxima over the
//                   event counts, the rotation reset, match12 and nmatches.
//
// Rows never interact (this reference never writes vbMatched2, :382,409), so
// the order of the reference's loops only matters inside a row, where a lane
// keeps it.  The rotation histogram is kept as event counts per bin plus, per
// row, a mask of the bins it touched: "every idx1 pushed into a dropped bin is
// reset" (:448-457) is "a row whose mask has a bit outside the kept bins".
// Integer adds commute, so the counts do not depend on the schedule.
#include <hip/hip_runtime.h>

#include "match_internal.h"
#include "orbm_device.h"
#include "tri_internal.h"

namespace orbx {

// CheckDistEpipolarLine's line through kp1 (:72-74), in the floating-point
// form the reference's -O3 -march=native object has: one
// product rounded, the other fused into the add, under -ffp-contract=off
__device__ __forceinline__ void tri_line(const float* __restrict__ F, float x1, float y1, float& a,
                                         float& b, float& c) {
  a = __builtin_fmaf(x1, F[0], y1 * F[3]) + F[6];
  b = __builtin_fmaf(x1, F[1], y1 * F[4]) + F[7];
  c = __builtin_fmaf(y1, F[5], x1 * F[2]) + F[8];
}

// :76-84; thr = 3.84 * (double)mvLevelSigma2[kp2.octave].  A NaN den is not
// == 0: it goes on and fails the compare, as in the reference
__device__ __forceinline__ bool tri_epipolar(float a, float b, float c, float den, float x2,
                                             float y2, double thr) {
  if (den == 0) return false;
  const float num = __builtin_fmaf(b, y2, a * x2) + c;
  const float dsqr = (num * num) / den;
  return (double)dsqr < thr;
}

__global__ __launch_bounds__(256) void k_tri_init(const TriProblem* __restrict__ probs, int n1) {
  const TriProblem& P = probs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n1) P.row[i] = make_int2(-1, 0);
  if (blockIdx.x == 0 && threadIdx.x < 32) P.hist[threadIdx.x] = 0;
}

__global__ __launch_bounds__(TRI_ROWS) void k_tri_search(const TriProblem* __restrict__ probs,
                                                        const TriItem* __restrict__ items,
                                                        TriFrame kf1, int check_ori) {
  __shared__ uint4 s_desc[TRI_CHUNK][2];
  __shared__ double s_thr[TRI_CHUNK];
  __shared__ float4 s_key[TRI_CHUNK];  // x, y, angle, idx2 (bits; -1 = skipped)
  __shared__ int s_hist[32];
  __shared__ float s_F[9];
  const int lane = threadIdx.x;
  const TriItem it = items[blockIdx.x];
  const TriProblem& P = probs[it.prob];
  if (lane < 32) s_hist[lane] = 0;
  if (lane < 9) s_F[lane] = P.F[lane];
  __syncthreads();

  // this lane's row: a KF1 feature with a MapPoint is skipped (:399-400)
  const bool has_row = lane < it.n1;
  const uint32_t idx1 = has_row ? kf1.feat[it.off1 + lane] : 0;
  const bool active = has_row && !(kf1.has_mp && kf1.has_mp[idx1]);
  uint32_t d1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ang1 = 0, a = 0, b = 0, c = 0, den = 0;
  if (active) {
    const uint4* dp = reinterpret_cast<const uint4*>(kf1.desc + (size_t)idx1 * 32);
    const uint4 lo = dp[0], hi = dp[1];
    d1[0] = lo.x; d1[1] = lo.y; d1[2] = lo.z; d1[3] = lo.w;
    d1[4] = hi.x; d1[5] = hi.y; d1[6] = hi.z; d1[7] = hi.w;
    const TriKey k1 = kf1.key[idx1];
    ang1 = k1.angle;
    tri_line(s_F, k1.x, k1.y, a, b, c);
    den = __builtin_fmaf(a, a, b * b);  // :77
  }
  // an inactive lane accepts nothing: no distance is <= -1
  int best_dist = active ? ORBM_TH_LOW : -1, best_idx = -1;  // :405-406
  uint32_t mask = 0;
  const float factor = 1.0f / ORBM_HISTO;

  for (int c0 = 0; c0 < it.n2; c0 += TRI_CHUNK) {
    const int cn = min(TRI_CHUNK, it.n2 - c0);
    if (c0) __syncthreads();  // the previous chunk has been read
    if (lane < cn) {
      const uint32_t idx2 = P.kf2.feat[it.off2 + c0 + lane];
      // a KF2 feature with a MapPoint is never a candidate (:409)
      const bool skip = P.kf2.has_mp && P.kf2.has_mp[idx2];
      const uint4* dp = reinterpret_cast<const uint4*>(P.kf2.desc + (size_t)idx2 * 32);
      const TriKey k2 = P.kf2.key[idx2];
      s_desc[lane][0] = dp[0];
      s_desc[lane][1] = dp[1];
      s_thr[lane] = 3.84 * (double)P.sigma2[k2.octave];  // :84
      s_key[lane] = make_float4(k2.x, k2.y, k2.angle, __int_as_float(skip ? -1 : (int)idx2));
    }
    __syncthreads();
    for (int j = 0; j < cn; ++j) {  // list order; every lane reads the same entry
      const float4 k2 = s_key[j];
      const int idx2 = __float_as_int(k2.w);
      if (idx2 < 0) continue;
      const uint4 lo = s_desc[j][0], hi = s_desc[j][1];
      // by value: handing the d1 array itself to a helper reorders this kernel's code
      const int dist = ham256_popc(make_uint4(d1[0], d1[1], d1[2], d1[3]),
                                   make_uint4(d1[4], d1[5], d1[6], d1[7]), lo, hi);
      if (dist > best_dist) continue;  // :414 (best_dist <= TH_LOW); equality goes on
      if (!tri_epipolar(a, b, c, den, k2.x, k2.y, s_thr[j])) continue;  // :417
      best_idx = idx2;
      best_dist = dist;
      if (check_ori) {  // every acceptance is a rotation event (:420-426)
        float rot = ang1 - k2.z;
        if (rot < 0.0f) rot += 360.0f;
        const int bin = (int)roundf(rot * factor) % ORBM_HISTO;
        // angles in [0, 360) give bins 0..12; anything else would index
        // rotHist out of range in the reference and is dropped here
        if ((unsigned)bin < (unsigned)ORBM_HISTO) {
          mask |= 1u << bin;
          atomicAdd(&s_hist[bin], 1);
        }
      }
    }
  }
  // a KF1 feature sits in one node (checked by the caller), so this is the
  // only write of its row
  if (active && best_idx >= 0) P.row[idx1] = make_int2(best_idx, (int)mask);
  __syncthreads();
  if (lane < ORBM_HISTO && s_hist[lane]) atomicAdd(&P.hist[lane], s_hist[lane]);
}

__global__ __launch_bounds__(256) void k_tri_finalize(const TriProblem* __restrict__ probs, int n1,
                                                      int check_ori) {
  __shared__ uint32_t s_keep;
  __shared__ int s_count;
  const TriProblem& P = probs[blockIdx.x];
  const int tid = threadIdx.x;
  if (tid == 0) {
    // the kept bins of ComputeThreeMaxima over the bins' event counts
    s_keep = 0xFFFFFFFFu;
    if (check_ori) {
      int ind[3];
      three_maxima(P.hist, ind);
      s_keep = kept_bins_mask(ind);
    }
    s_count = 0;
  }
  __syncthreads();
  const uint32_t keep = s_keep;
  int count = 0;
  for (int i = tid; i < n1; i += 256) {
    const int2 r = P.row[i];
    int m = r.x;
    // any event in a dropped bin resets the row, whatever bin its final
    // candidate fell in (:448-457); -2 = matched, then reset
    if (m >= 0 && ((uint32_t)r.y & ~keep)) m = -2;
    P.match12[i] = m;
    count += m >= 0;
  }
  if (count) atomicAdd(&s_count, count);
  __syncthreads();
  if (tid == 0) *P.nmatches = s_count;
}

}  // namespace orbx

// kernels_bowdb.hip -- gfx950 kernel of the DBoW2 score and of the keyframe
// database's candidate search:
//   TemplatedVocabulary::score(a, b)          TemplatedVocabulary.h:1199-1203
//   L1 / L2 / ChiSquare / DotProduct scoring  Thirdparty/DBoW2/DBoW2/ScoringObject.cpp
//   the word walk of KeyFrameDatabase::DetectLoopCandidates /
//   DetectRelocalizationCandidates            src/KeyFrameDatabase.cc:56-85,179-203
//
// k_bowdb_query: one launch per query.  The query's words (strictly ascending)
// are staged once per workgroup in LDS; a wavefront takes one stored vector at
// a time, the grid striding over them.  Its lanes read the vector's words 64
// at a time (coalesced) and each binary-searches the LDS copy; the ballot of
// the hits is the chunk's common words in ascending word order.  The double
// sum then walks the set bits of that ballot in lane order, every lane adding
// the same lane's term, so the sum is the reference's left-to-right sum over
// the common words (its lower_bound jumps only skip words that are not
// common) -- no tree or butterfly ever touches the double.  The ballots also
// give the number of common words and the smallest one.  -ffp-contract=off:
// the terms are the reference's expressions, never fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bowdb_internal.h"

namespace orbx {

__device__ __forceinline__ double lane_double(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}

// scoring: 0 L1, 1 L2 (the closing sqrt step is the caller's), 2 chi-square,
// 5 dot product.  256 threads = 4 wavefronts; dynamic LDS: nq words.
__global__ __launch_bounds__(256) void k_bowdb_query(
    const uint32_t* __restrict__ qword, const double* __restrict__ qvalue, int nq,
    const BowdbSlot* __restrict__ slots, int nslots, const uint32_t* __restrict__ words,
    const double* __restrict__ values, int scoring, BowdbRec* __restrict__ out) {
  extern __shared__ uint32_t s_q[];
  for (int i = threadIdx.x; i < nq; i += blockDim.x) s_q[i] = qword[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int nwaves = (int)(gridDim.x * (blockDim.x >> 6));
  for (int j = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); j < nslots; j += nwaves) {
    const BowdbSlot s = slots[j];
    double acc = 0.0;
    int cnt = 0;
    uint32_t first = 0;
    const uint32_t len = s.alive ? s.len : 0u;
    for (uint32_t base = 0; base < len; base += 64) {
      const uint32_t i = base + (uint32_t)lane;
      uint32_t w = 0;
      int pos = 0;
      bool hit = false;
      if (i < len) {
        w = words[(size_t)s.off + i];
        int lo = 0, hi = nq;  // lower_bound of w in s_q[0, nq)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_q[mid] < w) lo = mid + 1;
          else hi = mid;
        }
        pos = lo;
        hit = lo < nq && s_q[lo] == w;
      }
      const unsigned long long mask = __ballot(hit);
      if (mask == 0ull) continue;  // wave-uniform
      double term = 0.0;
      bool add = hit;
      if (hit) {
        const double vi = qvalue[pos];                 // v1: the query
        const double wi = values[(size_t)s.off + i];  // v2: the stored vector
        if (scoring == 0) {
          term = fabs(vi - wi) - fabs(vi) - fabs(wi);
        } else if (scoring == 2) {
          add = vi + wi != 0.0;
          if (add) term = vi * wi / (vi + wi);
        } else {
          term = vi * wi;
        }
      }
      if (cnt == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)__builtin_ctzll(mask));
      cnt += (int)__builtin_popcountll(mask);
      unsigned long long m = __ballot(add);
      while (m) {  // ascending lanes = ascending words
        const int l = (int)__builtin_ctzll(m);
        m &= m - 1;
        acc += lane_double(term, l);
      }
    }
    if (lane == 0) {
      double sc = acc;
      if (scoring == 0) sc = -acc / 2.0;
      else if (scoring == 2) sc = 2. * acc;
      BowdbRec r;
      r.id = s.id;
      r.seq = s.seq;
      r.score = sc;
      r.ncommon = cnt;
      r.first = first;
      out[j] = r;
    }
  }
}

}  // namespace orbx

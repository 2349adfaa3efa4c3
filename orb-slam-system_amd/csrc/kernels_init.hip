// kernels_init.hip -- ORBmatcher::SearchForInitialization
// (src/ORBmatcher.cc:197-276) for gfx950, batched over independent pairs.
// F2's grid comes from k_grid_build (kernels_proj.hip).
//
//   k_init_cand  IN_G lanes per F1 row: Frame::GetFeaturesInArea around
//                vbPrevMatched (src/Frame.cc:307-358), the Hamming distance of
//                every candidate, and of those below the cut distance the
//                IN_T smallest (distance << 16 | rank) keys and their number;
//   k_init_walk  one workgroup per pair: vMatchedDistance, vnMatches21 and the
//                feature every row was accepted with in LDS; the first wave
//                walks the rows in order, the whole workgroup then does the
//                rotation check, vnMatches12 and vbPrevMatched.
//
// The cut: a row is accepted only with bestDist <= TH_LOW, and
// every bestDist2 >= dcut passes the ratio test for such a bestDist exactly as
// INT_MAX does.  So candidates at dcut or beyond never change a result and
// only the few below it are listed.  The walk's filter dist <
// vMatchedDistance[i2] is applied to the list in key order: the first entry
// that passes is the best (first strict minimum = smallest (distance, rank)),
// the second one's distance is bestDist2.  That is exact when the list is
// complete, when two entries pass, or when the first that passes is beyond
// TH_LOW; any other row scans its window again under the current claims.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/orbx.h"
#include "grid_device.h"
#include "init_internal.h"
#include "orbm_device.h"
#include "wave_ops.h"

namespace orbx {

#define IN_NONE 0xFFFFu  // 16-bit tables: no holder / never accepted / INT_MAX

// the level gate of GetFeaturesInArea(.., minLevel = maxLevel = kp1.octave)
// for the octaves that reach it (<= 0): bCheckLevels only at octave 0, which
// then admits octave 0 alone; a negative octave searches every level
__device__ __forceinline__ bool init_level_ok(int oct1, int oct2) { return oct1 < 0 || oct2 == 0; }

__global__ __launch_bounds__(IN_BLOCK) void k_init_cand(const InitPair* __restrict__ pairs, float window,
                                                       int dcut) {
  const InitPair PP = pairs[blockIdx.y];
  const int gl = threadIdx.x & (IN_G - 1);
  const int row = blockIdx.x * (IN_BLOCK / IN_G) + (threadIdx.x / IN_G);
  if (row >= PP.n1) return;  // whole groups leave: the shuffles below stay inside a group
  const ProjFrame F = PP.F2;
  const orbx_keypoint* __restrict__ keys2 = PP.keys2;
  const uint8_t* __restrict__ desc2 = PP.desc2;
  const int* __restrict__ cell_off = PP.cell_off;
  const int* __restrict__ cell_feat = PP.cell_feat;
  const int oct1 = PP.keys1[row].octave;
  uint32_t L[IN_T];
#pragma unroll
  for (int t = 0; t < IN_T; ++t) L[t] = 0xFFFFFFFFu;
  int nl = 0;  // candidates below the cut seen by this lane
  int x0, x1, y0, y1;
  const float x = PP.prev_in[2 * row], y = PP.prev_in[2 * row + 1];
  if (oct1 <= 0 && area_cells(F, x, y, window, &x0, &x1, &y0, &y1)) {  // :212
    const uint4* qd = reinterpret_cast<const uint4*>(PP.desc1 + (size_t)row * 32);
    const uint4 q0 = qd[0], q1 = qd[1];
    for (int ix = x0; ix <= x1; ++ix) {
      // cells (ix, y0..y1) are contiguous in the ix-major list
      const int b = cell_off[ix * PG_ROWS + y0], e = cell_off[ix * PG_ROWS + y1 + 1];
      for (int j = b + gl; j < e; j += IN_G) {
        const int idx = cell_feat[j];
        if (!init_level_ok(oct1, keys2[idx].octave)) continue;
        const float distx = keys2[idx].x - x, disty = keys2[idx].y - y;
        if (!(fabsf(distx) < window && fabsf(disty) < window)) continue;
        const uint4* dp = reinterpret_cast<const uint4*>(desc2 + (size_t)idx * 32);
        const uint4 b0 = dp[0], b1 = dp[1];
        const int d = ham256_popc(q0, q1, b0, b1);
        if (d >= dcut) continue;
        ++nl;
        uint32_t k = ((uint32_t)d << 16) | (uint32_t)j;
#pragma unroll
        for (int t = 0; t < IN_T; ++t) {
          const uint32_t lo = min(L[t], k);
          k = max(L[t], k);
          L[t] = lo;
        }
      }
    }
  }
  // merge the group's lists: IN_T rounds of a group minimum
  int total = nl;
#pragma unroll
  for (int d = IN_G >> 1; d >= 1; d >>= 1) total += __shfl_xor(total, d, IN_G);
  int head = 0;
  uint32_t out = 0xFFFFFFFFu;
  for (int t = 0; t < IN_T; ++t) {
    const uint32_t mine = head < IN_T ? L[0] : 0xFFFFFFFFu;
    uint32_t m = mine;
#pragma unroll
    for (int d = IN_G >> 1; d >= 1; d >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, d, IN_G));
    if (gl == t) out = m;
    if (mine == m && m != 0xFFFFFFFFu) {  // keys are unique (rank): one winner
#pragma unroll
      for (int s = 0; s < IN_T - 1; ++s) L[s] = L[s + 1];
      L[IN_T - 1] = 0xFFFFFFFFu;
      ++head;
    }
  }
  // the smallest key (lane 0's) holds the row's smallest distance: beyond
  // TH_LOW the row cannot be accepted whatever is claimed, and a row that is
  // not accepted changes nothing: the walk passes over it (nlow = 0)
  const uint32_t first = (uint32_t)__shfl((int)out, 0, IN_G);
  if (first != 0xFFFFFFFFu && (first >> 16) > IN_TH_LOW) total = 0;
  if (gl < IN_T) {
    // the order is settled: the walk wants the feature, not its rank
    if (out != 0xFFFFFFFFu) out = (out & 0xFFFF0000u) | (uint32_t)cell_feat[out & 0xFFFFu];
    PP.cand[(size_t)row * IN_T + gl] = out;
  }
  if (gl == 0) PP.nlow[row] = total;
}

// exact step of one row under the current claims (first wave, 64 lanes): over
// the window in visiting order, among candidates with dist < matched[i2], the
// smallest (distance << 16 | rank) key and the second-smallest distance
__device__ void init_rescan(const InitPair& PP, int row, float window, const uint16_t* md, uint32_t* k1,
                            uint32_t* d2) {
  const int lane = threadIdx.x & 63;
  const ProjFrame F = PP.F2;
  const orbx_keypoint* __restrict__ keys2 = PP.keys2;
  const int* __restrict__ cell_off = PP.cell_off;
  const int* __restrict__ cell_feat = PP.cell_feat;
  const int oct1 = PP.keys1[row].octave;
  const float x = PP.prev_in[2 * row], y = PP.prev_in[2 * row + 1];
  const uint4* qd = reinterpret_cast<const uint4*>(PP.desc1 + (size_t)row * 32);
  const uint4 q0 = qd[0], q1 = qd[1];
  uint32_t a = 0xFFFFFFFFu, b = 0xFFFFFFFFu;
  int x0, x1, y0, y1;
  if (area_cells(F, x, y, window, &x0, &x1, &y0, &y1)) {
    for (int ix = x0; ix <= x1; ++ix) {
      const int bb = cell_off[ix * PG_ROWS + y0], e = cell_off[ix * PG_ROWS + y1 + 1];
      for (int j = bb + lane; j < e; j += 64) {
        const int idx = cell_feat[j];
        if (!init_level_ok(oct1, keys2[idx].octave)) continue;
        const float distx = keys2[idx].x - x, disty = keys2[idx].y - y;
        if (!(fabsf(distx) < window && fabsf(disty) < window)) continue;
        const uint4* dp = reinterpret_cast<const uint4*>(PP.desc2 + (size_t)idx * 32);
        const uint4 b0 = dp[0], b1 = dp[1];
        const uint32_t d = (uint32_t)ham256_popc(q0, q1, b0, b1);
        if (!(d < (uint32_t)md[idx])) continue;  // :224 (IN_NONE = INT_MAX: every distance passes)
        const uint32_t k = (d << 16) | (uint32_t)j;
        if (k < a) {
          b = min(b, a >> 16);
          a = k;
        } else {
          b = min(b, k >> 16);
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t oa = (uint32_t)__shfl_xor((int)a, d, 64);
    const uint32_t ob = (uint32_t)__shfl_xor((int)b, d, 64);
    const uint32_t lo = min(a, oa), hi = max(a, oa);
    b = min(min(b, ob), hi >> 16);
    a = lo;
  }
  *k1 = a == 0xFFFFFFFFu ? a : ((a & 0xFFFF0000u) | (uint32_t)cell_feat[a & 0xFFFFu]);
  *d2 = b;
}

// rotation bin of an accepted pair (:246-249)
__device__ __forceinline__ int init_bin(float a1, float a2) {
  float rot = a1 - a2;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * (1.0f / ORBM_HISTO));
  if (bin == ORBM_HISTO) bin = 0;
  return bin;
}

__global__ __launch_bounds__(IN_BLOCK) void k_init_walk(const InitPair* __restrict__ pairs, float window,
                                                       float nnratio, int check_ori) {
  __shared__ uint16_t md[IN_MAXN];   // vMatchedDistance, IN_NONE = INT_MAX
  __shared__ uint16_t m21[IN_MAXN];  // vnMatches21, IN_NONE = -1
  __shared__ uint16_t acc[IN_MAXN];  // the feature a row was accepted with (kept when displaced)
  __shared__ uint32_t sl[IN_BATCH * IN_T];
  __shared__ int snl[IN_BATCH];
  __shared__ int hist[32];
  __shared__ int s_nm, s_resc;
  __shared__ uint32_t s_keep;
  const InitPair PP = pairs[blockIdx.x];
  const int n1 = PP.n1, n2 = PP.F2.n;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < n2; i += IN_BLOCK) {
    md[i] = IN_NONE;
    m21[i] = IN_NONE;
  }
  for (int i = tid; i < n1; i += IN_BLOCK) acc[i] = IN_NONE;
  if (tid < 32) hist[tid] = 0;
  if (tid == 0) {
    s_nm = 0;
    s_resc = 0;
    s_keep = 0;
  }
  int resc = 0;
  // n1 is the same for the whole workgroup: every barrier below is uniform
  for (int base = 0; base < n1; base += IN_BATCH) {
    const int cnt = min(IN_BATCH, n1 - base);
    __syncthreads();  // the tables above; the previous batch's lists are done with
    for (int i = tid; i < cnt * IN_T; i += IN_BLOCK) sl[i] = PP.cand[(size_t)base * IN_T + i];
    for (int i = tid; i < cnt; i += IN_BLOCK) snl[i] = PP.nlow[base + i];
    __syncthreads();
    if (tid >= 64) continue;  // the first wave walks; the others wait at the barrier above
    for (int sub = 0; sub < cnt; sub += 64) {
      const int v = sub + lane < cnt ? snl[sub + lane] : 0;
      unsigned long long todo = __ballot(v > 0);  // rows without a candidate below the cut: nothing to do
      while (todo) {
        const int rl = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int r = sub + rl, row = base + r;
        const int nl = lane_value(v, rl);
        const uint32_t e = lane < IN_T ? sl[r * IN_T + lane] : 0xFFFFFFFFu;
        const bool pass = e != 0xFFFFFFFFu && (e >> 16) < (uint32_t)md[e & 0xFFFFu];  // :224
        const unsigned long long pb = __ballot(pass);
        const int npass = __popcll(pb);
        uint32_t k1 = 0xFFFFFFFFu, d2 = 0xFFFFFFFFu;
        if (npass >= 1) k1 = lane_value(e, __ffsll(pb) - 1);
        if (npass >= 2) d2 = lane_value(e, __ffsll(pb & (pb - 1)) - 1) >> 16;
        if (!(nl <= IN_T || npass >= 2 || (npass == 1 && (k1 >> 16) > IN_TH_LOW))) {
          init_rescan(PP, row, window, md, &k1, &d2);
          ++resc;
        }
        if (k1 == 0xFFFFFFFFu) continue;
        const int bestDist = (int)(k1 >> 16), bestIdx2 = (int)(k1 & 0xFFFFu);
        const int bestDist2 = d2 == 0xFFFFFFFFu ? INT_MAX : (int)d2;
        if (!(bestDist <= IN_TH_LOW && (float)bestDist < (float)bestDist2 * nnratio)) continue;  // :235
        if (lane == 0) {  // :236-243; the displaced row is found through m21 afterwards
          m21[bestIdx2] = (uint16_t)row;
          md[bestIdx2] = (uint16_t)bestDist;
          acc[row] = (uint16_t)bestIdx2;
        }
        // the next row's lanes read what lane 0 wrote
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
    }
  }
  __syncthreads();
  if (check_ori) {  // every accepted row votes, a displaced one too (:250)
    for (int i = tid; i < n1; i += IN_BLOCK) {
      const int idx = acc[i];
      if (idx != IN_NONE) atomicAdd(&hist[init_bin(PP.keys1[i].angle, PP.keys2[idx].angle)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int ind[3];
      three_maxima(hist, ind);
      s_keep = kept_bins_mask(ind);
    }
    __syncthreads();
  }
  const uint32_t keep = s_keep;
  int nm = 0;
  bool bad = false;
  for (int i = tid; i < n1; i += IN_BLOCK) {
    int m = PP.match_in[i];  // not accepted by this call: the caller's entry stays (:199)
    const int idx = acc[i];
    if (idx != IN_NONE) {
      m = m21[idx] == i ? idx : -1;  // :237
      if (m >= 0 && check_ori && !((keep >> init_bin(PP.keys1[i].angle, PP.keys2[idx].angle)) & 1u))
        m = -1;  // :262-265
      if (m >= 0) ++nm;
    }
    float px = PP.prev_in[2 * i], py = PP.prev_in[2 * i + 1];
    if (m >= n2) {
      bad = true;  // :272 would read past F2.mvKeysUn
    } else if (m >= 0) {
      px = PP.keys2[m].x;
      py = PP.keys2[m].y;
    }
    PP.match_out[i] = m;
    PP.prev_out[2 * i] = px;
    PP.prev_out[2 * i + 1] = py;
  }
  if (nm) atomicAdd(&s_nm, nm);
  if (resc && lane == 0) atomicAdd(&s_resc, resc);
  const int anybad = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0) {
    *PP.nmatches = s_nm;
    *PP.err = anybad ? 1 : 0;
    *PP.nrescan = s_resc;
  }
}

}  // namespace orbx

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
//
// k_bowdb_query_batch / k_bowdb_order (below): many queries per launch, and
// the ordering and the word gate of each query's list on the device.
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

// ---------------------------------------------------------------------------
// Batched queries.  The queries of a call come in one of two layouts: CSR
// (q_off != nullptr: query q at [q_off[q], q_off[q + 1])) or rows
// (q_off == nullptr: query q at [q * qstride, q * qstride + d_n[q]), the
// layout of orbv_transform_batch's outputs; d_n[q] < 0 counts as 0 and
// d_n[q] > qstride marks a query that is not run).
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool batch_query(const uint32_t* q_off, const int* d_n, int qstride, int q, size_t* at,
                                            int* n) {
  if (q_off) {
    *at = q_off[q];
    *n = (int)(q_off[q + 1] - q_off[q]);
    return true;
  }
  const int k = d_n[q];
  *at = (size_t)q * (size_t)qstride;
  *n = k < 0 ? 0 : k;
  return k <= qstride;
}

// k_bowdb_query with the query index in blockIdx.y: the same LDS staging, the
// same per-lane lower_bound and the same ballot-ordered wave-uniform double
// sum.  Per (query, slot) it leaves a BowdbBatchRec: the score, the number of
// common words and the rank in the query of the smallest one -- the pos the
// first hit lane holds.  Unsorted query words (the row layout is not checked)
// give wrong counts, never an access out of range: every pos is below n, and
// n is at most the LDS staged.  Dynamic LDS: the longest query's words.
__global__ __launch_bounds__(256) void k_bowdb_query_batch(
    const uint32_t* __restrict__ q_off, const int* __restrict__ d_n, int qstride,
    const uint32_t* __restrict__ qword, const double* __restrict__ qvalue, int nqueries,
    const BowdbSlot* __restrict__ slots, int nslots, const uint32_t* __restrict__ words,
    const double* __restrict__ values, int scoring, BowdbBatchRec* __restrict__ out) {
  extern __shared__ uint32_t s_q[];
  const int lane = threadIdx.x & 63;
  const int nwaves = (int)(gridDim.x * (blockDim.x >> 6));
  for (int q = (int)blockIdx.y; q < nqueries; q += (int)gridDim.y) {  // block-uniform
    size_t at;
    int nq;
    if (!batch_query(q_off, d_n, qstride, q, &at, &nq)) nq = 0;
    const uint32_t* qw = qword + at;
    const double* qv = qvalue + at;
    __syncthreads();  // the previous query's words are done with
    for (int i = threadIdx.x; i < nq; i += blockDim.x) s_q[i] = qw[i];
    __syncthreads();
    BowdbBatchRec* orec = out + (size_t)q * (size_t)nslots;
    for (int j = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); j < nslots; j += nwaves) {
      const BowdbSlot s = slots[j];
      double acc = 0.0;
      int cnt = 0;
      uint32_t rank = 0;
      const uint32_t len = s.alive ? s.len : 0u;
      for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        int pos = 0;
        bool hit = false;
        if (i < len) {
          const uint32_t w = words[(size_t)s.off + i];
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
          const double vi = qv[pos];                      // v1: the query
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
        if (cnt == 0) rank = (uint32_t)__builtin_amdgcn_readlane(pos, (int)__builtin_ctzll(mask));
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
        BowdbBatchRec r;
        r.score = sc;
        r.ncommon = cnt;
        r.rank = rank;
        orec[j] = r;
      }
    }
  }
}

// sum / max of one int per thread over the workgroup (4 wavefronts), the
// result in every thread; s_part: 4 ints, free again on return
template <bool MAX>
__device__ __forceinline__ int block_combine(int v, int* s_part) {
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(v, d, 64);
    v = MAX ? (o > v ? o : v) : v + o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = s_part[0], b = s_part[1], c = s_part[2], d = s_part[3];
  if (MAX) return max(max(a, b), max(c, d));
  return a + b + c + d;
}

// k_bowdb_order: one workgroup (BOWDB_ORDER_TILE threads) per query turns the
// query's records into the list orbv_db_query returns -- the sharing
// keyframes by (rank, slot) -- with integer work only:
//   the largest ncommon, which gives the gate when ORBV_QUERY_GATED is set;
//   a histogram of the passing records over the query's ranks in LDS;
//   its exclusive scan: every bin's start, and the query's count;
//   a stable placement: slots in ascending tiles; within a tile a record's
//   offset in its bin is the number of earlier passing records of the tile
//   with its rank, read from an LDS copy of the tile's ranks (every lane reads
//   the same address: a broadcast); the bins' cursors advance once the tile's
//   positions are taken.
// The atomics only count: no position depends on the order they arrive in.
// mode 0: cnt[q] = the query's count, nothing placed.
// mode 1: placed into the packed arrays from sum(cnt[0 .. q)) on.
// mode 2: placed into row q of [nqueries][cap], the entries below cap only;
//         nsharing[q] = the count, or -1 for a query that is not run.
// Dynamic LDS: one u32 per rank of the longest query (at most 32 KB).
__global__ __launch_bounds__(BOWDB_ORDER_TILE) void k_bowdb_order(
    const BowdbBatchRec* __restrict__ rec, const BowdbSlot* __restrict__ slots, int nslots, int nqueries,
    const uint32_t* __restrict__ q_off, const int* __restrict__ d_n, int qstride, int gated, int mode, int cap,
    int* cnt, uint64_t* __restrict__ kf_id, int32_t* __restrict__ ncommon, double* __restrict__ score,
    int* __restrict__ nsharing) {
  extern __shared__ uint32_t s_bin[];
  __shared__ __attribute__((aligned(16))) uint32_t s_rank[BOWDB_ORDER_TILE];
  __shared__ int s_part[4];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int q = (int)blockIdx.x; q < nqueries; q += (int)gridDim.x) {  // block-uniform
    size_t at;
    int n;
    if (!batch_query(q_off, d_n, qstride, q, &at, &n)) {
      if (t == 0 && mode == 2) nsharing[q] = -1;
      continue;
    }
    const BowdbBatchRec* r = rec + (size_t)q * (size_t)nslots;
    int gate = 0;
    if (gated) {
      int m = 0;
      for (int j = t; j < nslots; j += BOWDB_ORDER_TILE) m = max(m, r[j].ncommon);
      gate = bowdb_gate(block_combine<true>(m, s_part));
    }
    __syncthreads();  // the previous query's bins are done with
    for (int i = t; i < n; i += BOWDB_ORDER_TILE) s_bin[i] = 0u;
    __syncthreads();
    for (int j = t; j < nslots; j += BOWDB_ORDER_TILE) {
      const BowdbBatchRec x = r[j];
      if (x.ncommon > gate && x.rank < (uint32_t)n) atomicAdd(&s_bin[x.rank], 1u);
    }
    __syncthreads();
    // exclusive scan, BOWDB_ORDER_TILE bins at a time; `total` is block-uniform
    int total = 0;
    for (int base = 0; base < n; base += BOWDB_ORDER_TILE) {
      const int i = base + t;
      const int v = i < n ? (int)s_bin[i] : 0;
      int incl = v;
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
      }
      __syncthreads();
      if (lane == 63) s_part[wave] = incl;
      __syncthreads();
      int before = 0, all = 0;
      for (int w = 0; w < 4; ++w) {
        const int p = s_part[w];
        if (w < wave) before += p;
        all += p;
      }
      if (i < n) s_bin[i] = (uint32_t)(total + before + incl - v);
      total += all;
    }
    __syncthreads();
    if (mode == 0) {
      if (t == 0) cnt[q] = total;
      continue;
    }
    size_t out_at;
    int limit;
    if (mode == 1) {
      int mine = 0;
      for (int i = t; i < q; i += BOWDB_ORDER_TILE) mine += cnt[i];
      out_at = (size_t)block_combine<false>(mine, s_part);
      limit = total;
    } else {
      if (t == 0) nsharing[q] = total;
      out_at = (size_t)q * (size_t)cap;
      limit = cap;
    }
    if (total == 0) continue;
    for (int base = 0; base < nslots; base += BOWDB_ORDER_TILE) {
      const int j = base + t;
      BowdbBatchRec x;
      x.score = 0.0;
      x.ncommon = 0;
      x.rank = 0u;
      if (j < nslots) x = r[j];
      const bool pass = x.ncommon > gate && x.rank < (uint32_t)n;
      const uint32_t rk = pass ? x.rank : 0xFFFFFFFFu;
      s_rank[t] = rk;
      __syncthreads();
      if (__ballot(pass) != 0ull) {  // wave-uniform
        int before = 0;
        const int end = (wave + 1) * 64;
        for (int u = 0; u < end; u += 4) {  // u is wave-uniform: broadcast reads
          const uint4 y = *reinterpret_cast<const uint4*>(&s_rank[u]);
          before += (int)(y.x == rk && u < t) + (int)(y.y == rk && u + 1 < t) + (int)(y.z == rk && u + 2 < t) +
                    (int)(y.w == rk && u + 3 < t);
        }
        if (pass) {
          const int pos = (int)s_bin[rk] + before;
          if (pos < limit) {
            const size_t o = out_at + (size_t)pos;
            kf_id[o] = slots[j].id;
            ncommon[o] = x.ncommon;
            score[o] = x.score;
          }
        }
      }
      __syncthreads();  // the tile's positions are taken
      if (pass) atomicAdd(&s_bin[rk], 1u);
      __syncthreads();
    }
  }
}

}  // namespace orbx

// kernels_initrecon.hip -- Initializer's ReconstructH / ReconstructF
// (src/Initializer.cc:406-864), batched over pairs.  All the
// arithmetic is initrecon_math.h's, the same text the CPU restatement runs.
//
//   k_rc_candidates  one pair per lane: the model to its 8 or 4 (R, t, P2, O2),
//                    or to ReconstructH's exit (no candidate)
//   k_rc_check       (pair, candidate, tile of inlier matches), one match per
//                    lane: Triangulate and CheckRT's tests into a record
//   k_rc_select      (pair, candidate): nGood, the order statistic of the
//                    cosines by a radix select, the parallax
//   k_rc_decide      per pair: the reference's decision, the result record, and
//                    the winner's points triangulated again into P3D
//
// Every count is an integer and every float is computed by one lane from its own
// inputs, so no result depends on an order of summation across lanes.
#include "initrecon_internal.h"

namespace orbx {

// One pair per lane; the lane's 3x3 work matrices in LDS lane-minor, as
// k_ir_hypothesis keeps its own.  Candidates go straight to global memory.
__global__ __launch_bounds__(RC_CAND_W) void k_rc_candidates(const RcProblem* __restrict__ probs, int npair) {
  __shared__ float lds[18 * RC_CAND_W];
  const int lane = threadIdx.x, p = blockIdx.x * RC_CAND_W + lane;
  if (p >= npair) return;
  const RcProblem& P = probs[p];
  float K[9], M[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    K[e] = P.K[e];
    M[e] = P.M[e];
  }
  float* A = lds + lane;
  float* V = lds + 9 * RC_CAND_W + lane;
  int ncand = 0;
  if (P.present) {
    if (P.model == ORBX_RECON_H)
      ncand = rc_candidates_h(M, K, A, V, RC_CAND_W, P.cand, nullptr);
    else
      ncand = rc_candidates_f(M, K, A, V, RC_CAND_W, P.cand, nullptr);
  }
  RcStat* st = P.stat;
  st->ncand = ncand;
#pragma unroll
  for (int c = 0; c < RC_MAXCAND; ++c) {
    st->nGood[c] = 0;
    st->parallax[c] = 0.0f;
  }
}

// One inlier match per lane.  The lane's 4x4 A and V live in LDS lane-minor
// (element * RC_TILE + lane): conflict-free, registers indexed by unrolled loops
// only, and no barrier since a lane only touches its own column.  Workgroups of
// a candidate slot the pair does not use, or past the pair's last match, leave
// before they read anything but the pair's header.
__global__ __launch_bounds__(RC_TILE) void k_rc_check(const RcProblem* __restrict__ probs, float th2) {
  __shared__ float lds[32 * RC_TILE];
  const RcProblem& P = probs[blockIdx.z];
  const int c = blockIdx.y, lane = threadIdx.x;
  const int i = blockIdx.x * RC_TILE + lane;
  const int N = P.N;
  if (c >= P.stat->ncand || i >= N) return;
  const rc_cand C = P.cand[c];
  float K[9], P1[12];
#pragma unroll
  for (int e = 0; e < 9; ++e) K[e] = P.K[e];
  rc_p1(K, P1);
  const IrRec r = P.rec[i];
  float p3d[3], cosp;
  const int b = rc_check_match(&C, P1, K[0], K[4], K[2], K[5], r.u1, r.v1, r.u2, r.v2, th2, lds + lane,
                               lds + 16 * RC_TILE + lane, RC_TILE, p3d, &cosp, nullptr);
  P.cosv[(size_t)c * N + i] = cosp;
  P.code[(size_t)c * N + i] = b == RC_GOOD ? 2 : (b == RC_COUNTED ? 1 : 0);
}

// nGood and the element at index min(50, nGood - 1) of the ascending cosines
// (:833-840): four radix passes of 8 bits over rc_key's order-preserving keys,
// each a histogram of the keys that share the prefix found so far.  Selecting
// the k-th smallest key equals sorting and indexing.
__global__ __launch_bounds__(RC_SELECT_T) void k_rc_select(const RcProblem* __restrict__ probs) {
  __shared__ uint32_t s_hist[RC_SELECT_T];
  __shared__ uint32_t s_prefix;
  __shared__ int s_k, s_n;
  const RcProblem& P = probs[blockIdx.y];
  const int c = blockIdx.x, t = threadIdx.x;
  RcStat* st = P.stat;
  if (c >= st->ncand) return;
  const int N = P.N;
  const float* cosv = P.cosv + (size_t)c * N;
  const uint8_t* code = P.code + (size_t)c * N;
  if (t == 0) s_n = 0;
  __syncthreads();
  int mine = 0;
  for (int i = t; i < N; i += RC_SELECT_T) mine += code[i] != 0;
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  const int nGood = s_n;
  if (nGood == 0) return;  // parallax = 0 (:840): the candidates kernel left both slots zero
  int k = rc_parallax_index(nGood);
  uint32_t prefix = 0, mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[t] = 0;
    __syncthreads();
    for (int i = t; i < N; i += RC_SELECT_T)
      if (code[i]) {
        const uint32_t key = rc_key(cosv[i]);
        if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
      }
    __syncthreads();
    if (t == 0) {
      int cum = 0, digit = 255;
      for (int b = 0; b < 256; ++b) {
        const int h = (int)s_hist[b];
        if (k < cum + h) {
          digit = b;
          break;
        }
        cum += h;
      }
      s_k = k - cum;
      s_prefix = prefix | ((uint32_t)digit << shift);
    }
    __syncthreads();
    k = s_k;
    prefix = s_prefix;
    mask |= 255u << shift;
  }
  if (t == 0) {
    st->nGood[c] = nGood;
    st->parallax[c] = rc_parallax(rc_unkey(prefix));
  }
}

// The decision on the eight or four (nGood, parallax), the result record, and
// P3D / triangulated over all n1 keys: zero everywhere, then the counted
// matches of the winning candidate, whose points are triangulated again (the
// same function on the same inputs as k_rc_check, so the same words).
__global__ __launch_bounds__(RC_DECIDE_T) void k_rc_decide(const RcProblem* __restrict__ probs, float min_parallax,
                                                           int min_triangulated) {
  __shared__ float lds[32 * RC_DECIDE_T];
  __shared__ int s_best, s_ok;
  const RcProblem& P = probs[blockIdx.x];
  const int t = threadIdx.x;
  const int N = P.N, n1 = P.n1;
  if (t == 0) {
    const RcStat* st = P.stat;
    const int ncand = st->ncand;
    int best = -1, ok = 0;
    if (P.model == ORBX_RECON_H) {
      if (ncand == 8) ok = rc_decide_h(st->nGood, st->parallax, N, min_parallax, min_triangulated, &best) == RC_H_OK;
    } else {
      if (ncand == 4) ok = rc_decide_f(st->nGood, st->parallax, N, min_parallax, min_triangulated, &best) < RC_F_MINGOOD;
    }
    orbx_recon_result* res = P.res;
    res->ok = ok;
    res->model_used = P.model;
    for (int e = 0; e < 9; ++e) res->R21[e] = ok ? P.cand[best].R[e] : 0.0f;
    for (int e = 0; e < 3; ++e) res->t21[e] = ok ? P.cand[best].t[e] : 0.0f;
    res->best = best;
    res->ncand = ncand;
    for (int c = 0; c < RC_MAXCAND; ++c) {
      res->nGood[c] = st->nGood[c];
      res->parallax[c] = st->parallax[c];
    }
    res->n_inliers = N;
    s_best = best;
    s_ok = ok;
  }
  for (int i = t; i < n1; i += RC_DECIDE_T) {
    P.P3D[3 * (size_t)i + 0] = 0.0f;
    P.P3D[3 * (size_t)i + 1] = 0.0f;
    P.P3D[3 * (size_t)i + 2] = 0.0f;
    P.tri[i] = 0;
  }
  __syncthreads();  // the zeros are down before a lane writes another lane's row
  if (!s_ok) return;
  const int best = s_best;
  const rc_cand C = P.cand[best];
  float K[9], P1[12];
#pragma unroll
  for (int e = 0; e < 9; ++e) K[e] = P.K[e];
  rc_p1(K, P1);
  const uint8_t* code = P.code + (size_t)best * N;
  for (int i = t; i < N; i += RC_DECIDE_T) {
    const int cd = code[i];
    if (!cd) continue;
    const IrRec r = P.rec[i];
    float p3d[3];
    rc_triangulate(P1, C.P2, r.u1, r.v1, r.u2, r.v2, lds + t, lds + 16 * RC_DECIDE_T + t, RC_DECIDE_T, p3d, nullptr);
    const int f = P.first[i];
    P.P3D[3 * (size_t)f + 0] = p3d[0];
    P.P3D[3 * (size_t)f + 1] = p3d[1];
    P.P3D[3 * (size_t)f + 2] = p3d[2];
    P.tri[f] = cd == 2;
  }
}

void launch_initrecon(const RcProblem* d_probs, int npair, int maxN, float th2, float min_parallax,
                      int min_triangulated, hipStream_t s) {
  hipLaunchKernelGGL(k_rc_candidates, dim3((unsigned)((npair + RC_CAND_W - 1) / RC_CAND_W)), dim3(RC_CAND_W), 0, s,
                     d_probs, npair);
  if (maxN > 0) {
    const unsigned tiles = (unsigned)((maxN + RC_TILE - 1) / RC_TILE);
    hipLaunchKernelGGL(k_rc_check, dim3(tiles, RC_MAXCAND, (unsigned)npair), dim3(RC_TILE), 0, s, d_probs, th2);
    hipLaunchKernelGGL(k_rc_select, dim3(RC_MAXCAND, (unsigned)npair), dim3(RC_SELECT_T), 0, s, d_probs);
  }
  hipLaunchKernelGGL(k_rc_decide, dim3((unsigned)npair), dim3(RC_DECIDE_T), 0, s, d_probs, min_parallax,
                     min_triangulated);
}

}  // namespace orbx

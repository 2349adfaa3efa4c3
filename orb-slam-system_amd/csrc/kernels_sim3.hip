// kernels_sim3.hip -- Sim3Solver's RANSAC (src/Sim3Solver.cc), batched over
// solvers.  All the arithmetic is sim3_math.h's, the same text
// the CPU restatement runs.  One launch, one workgroup per problem:
//
//   prologue  the constructor's values of every correspondence (camera
//             coordinates, image points, the two bounds), one per lane
//   phase A   one hypothesis per lane: gather the three point pairs, Horn's
//             closed form with the 4x4 Jacobi in registers, (T12, T21) into LDS
//             lane-minor and the whole hypothesis into the problem's scratch
//   phase B   the inlier counts: a wavefront per hypothesis, lanes over the
//             correspondences, a ballot and a population count per 64
//   phase C   the reference's sequential choice as a prefix maximum over the
//             counts, then the winner's transformation and its flags
//
// Phases A and B alternate over chunks of S3_T hypotheses.  The counts are
// integers: nothing here depends on a summation order.
#include <limits.h>

#include "sim3_internal.h"

namespace orbx {

__global__ __launch_bounds__(S3_T) void k_sim3(const S3Problem* __restrict__ probs) {
  __shared__ float s_T[S3_TF][S3_T];
  __shared__ int s_cnt[S3_MAXIT];
  __shared__ int s_seg[S3_T];
  __shared__ float s_win[S3_HYP];
  __shared__ int s_hit, s_best;
  const S3Problem& P = probs[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ncorr = P.ncorr, nit = P.nit;
  float K1[4], K2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) K1[e] = P.cams[e], K2[e] = P.cams[4 + e];

  if (nit > 0) {
    float pose[24];
#pragma unroll
    for (int e = 0; e < 24; ++e) pose[e] = P.pose[e];
    for (int i = t; i < ncorr; i += S3_T) {
      S3Rec r;
      s3_make_corr(P.pos1 + 3 * i, P.pos2 + 3 * i, P.sigma2_1[i], P.sigma2_2[i], pose, pose + 9, pose + 12, pose + 21,
                   K1, K2, &r.c);
      P.corr[i] = r;
    }
  }
  __syncthreads();  // the records are read by other lanes from here on

  for (int base = 0; base < nit; base += S3_T) {
    const int it = base + t;
    if (it < nit) {
      // a lane touches only its own column of s_T and of the scratch
      const int i0 = P.triples[3 * it], i1 = P.triples[3 * it + 1], i2 = P.triples[3 * it + 2];
      const S3Rec a = P.corr[i0], b = P.corr[i1], c = P.corr[i2];
      s3_hyp H;
      s3_compute_sim3(a.c.X1, b.c.X1, c.c.X1, a.c.X2, b.c.X2, c.c.X2, P.fix_scale, &H, nullptr, nullptr);
#pragma unroll
      for (int e = 0; e < 9; ++e) s_T[e][t] = H.sR12[e], s_T[12 + e][t] = H.sR21[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) s_T[9 + e][t] = H.t[e], s_T[21 + e][t] = H.t21[e];
      float* hyp = P.hyp + it;
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        hyp[(size_t)e * nit] = H.R[e];
        hyp[(size_t)(13 + e) * nit] = H.sR12[e];
        hyp[(size_t)(22 + e) * nit] = H.sR21[e];
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        hyp[(size_t)(9 + e) * nit] = H.t[e];
        hyp[(size_t)(31 + e) * nit] = H.t21[e];
      }
      hyp[(size_t)12 * nit] = H.s;
    }
    __syncthreads();
    const int nchunk = nit - base < S3_T ? nit - base : S3_T;
    for (int h = wave; h < nchunk; h += S3_T / 64) {
      float T[S3_TF];  // wave-uniform: every lane reads the same word
#pragma unroll
      for (int e = 0; e < S3_TF; ++e) T[e] = s_T[e][h];
      int n = 0;
      for (int i0 = 0; i0 < ncorr; i0 += 64) {
        const int i = i0 + lane;
        int in = 0;
        if (i < ncorr) {
          const S3Rec r = P.corr[i];
          in = s3_check(T, T + 9, T + 12, T + 21, K1, K2, &r.c);
        }
        n += __popcll(__ballot(in));
      }
      if (lane == 0) s_cnt[base + h] = n;
    }
    __syncthreads();  // s_T is written again by the next chunk; s_cnt is read below
  }

  // With m_i = max(best_in, c_j for j < i): the loop's `>=` test (:163) holds
  // at i where c_i >= m_i; it returns at the first such i with c_i >
  // min_inliers (:172); the state it leaves is that of the last such i up to
  // there.  Lane t owns the iterations [t K, t K + K)
  const int K = (nit + S3_T - 1) / S3_T;
  const int lo = t * K < nit ? t * K : nit, hi = lo + K < nit ? lo + K : nit;
  int mx = -1;
  for (int i = lo; i < hi; ++i) mx = s_cnt[i] > mx ? s_cnt[i] : mx;
  s_seg[t] = mx;
  if (t == 0) s_hit = INT_MAX, s_best = -1;
  __syncthreads();
  int m0 = P.best_in;
  for (int j = 0; j < t; ++j) m0 = s_seg[j] > m0 ? s_seg[j] : m0;
  const int min_inliers = P.min_inliers;
  int first = INT_MAX;
  for (int i = lo, m = m0; i < hi; ++i) {
    const int c = s_cnt[i];
    if (c >= m) {
      m = c;
      if (c > min_inliers && first == INT_MAX) first = i;
    }
  }
  if (first != INT_MAX) atomicMin(&s_hit, first);
  __syncthreads();
  const int hit = s_hit == INT_MAX ? -1 : s_hit;
  const int end = hit >= 0 ? hit + 1 : nit;
  int last = -1;
  for (int i = lo, m = m0; i < hi && i < end; ++i) {
    const int c = s_cnt[i];
    if (c >= m) {
      m = c;
      last = i;
    }
  }
  if (last >= 0) atomicMax(&s_best, last);
  __syncthreads();
  const int best = s_best;
  if (t < S3_HYP) s_win[t] = best >= 0 ? P.hyp[(size_t)t * nit + best] : 0.0f;
  __syncthreads();
  // the flags of the winner: the same function on the same inputs as phase B
  for (int i = t; i < ncorr; i += S3_T) {
    int in = 0;
    if (best >= 0) {
      const S3Rec r = P.corr[i];
      in = s3_check(s_win + 13, s_win + 9, s_win + 22, s_win + 31, K1, K2, &r.c);
    }
    P.inl[i] = (uint8_t)in;
  }
  orbx_sim3_result* res = P.res;
  if (t < 9) res->R12[t] = s_win[t], res->sR21[t] = s_win[22 + t];
  if (t < 3) res->t12[t] = s_win[9 + t], res->t21[t] = s_win[31 + t];
  if (t == 0) {
    res->s12 = s_win[12];
    res->it_hit = hit;
    res->it_best = best;
    res->n_best = best >= 0 ? s_cnt[best] : P.best_in;
    res->ncorr = ncorr;
  }
}

void launch_sim3(const S3Problem* d_probs, int nprob, hipStream_t s) {
  hipLaunchKernelGGL(k_sim3, dim3((unsigned)nprob), dim3(S3_T), 0, s, d_probs);
}

}  // namespace orbx

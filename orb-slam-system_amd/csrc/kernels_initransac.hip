// kernels_initransac.hip -- Initializer's homography / fundamental RANSAC
// (src/Initializer.cc:80-404), batched over pairs.  All the
// arithmetic is initransac_math.h's, the same text the CPU restatement runs.
//
//   k_ir_hypothesis<MODEL>  one hypothesis per lane: gather the 8 normalised
//                           pairs, DLT matrix, one-sided Jacobi, denormalise
//   k_ir_score              the chi-squares of a tile of matches side by side
//                           into LDS, then added in list order, one hypothesis
//                           per lane (the reference's sequential float sum)
//   k_ir_select             per pair: the first strict maximum of each model,
//                           its matrix, the inlier flags, SH, SF, RH
#include "initransac_internal.h"

namespace orbx {

// One hypothesis per lane.  The lane's DLT matrix (M x 9) and V (9 x 9) live in
// LDS lane-minor (element * IR_W + lane): every lane of the wavefront touches
// the same element at once, so the accesses are conflict-free, and registers
// are indexed by unrolled loops only (no scratch).  A lane only ever touches
// its own column, so the kernel has no barrier: lanes that converge after fewer
// sweeps just sit out the rest of the loop.
template <int MODEL>
__global__ __launch_bounds__(IR_W) void k_ir_hypothesis(const IrProblem* __restrict__ probs, int nit, int nchunk) {
  constexpr int M = MODEL ? 8 : 16;
  __shared__ float lds[(M * 9 + 81) * IR_W];
  const int p = blockIdx.x / nchunk, chunk = blockIdx.x - p * nchunk;
  const int lane = threadIdx.x;
  const int it = chunk * IR_W + lane;
  if (it >= nit) return;
  const IrProblem& P = probs[p];
  float pn[8][4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const IrRec r = P.recn[P.sets[it * 8 + j]];
    pn[j][0] = r.u1, pn[j][1] = r.v1, pn[j][2] = r.u2, pn[j][3] = r.v2;
  }
  float T1[9], T2[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    T1[e] = P.T1[e];
    T2[e] = MODEL ? P.T2t[e] : P.T2inv[e];
  }
  float* A = lds + lane;
  float* V = lds + M * 9 * IR_W + lane;
  float* hyp = P.hyp + it;
  if (MODEL == 0) {
    float H21i[9], H12i[9];
    ir_hypothesis_h(pn, T1, T2, A, V, IR_W, H21i, H12i, nullptr);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      hyp[(size_t)e * nit] = H21i[e];
      hyp[(size_t)(9 + e) * nit] = H12i[e];
    }
  } else {
    float F21i[9];
    ir_hypothesis_f(pn, T1, T2, A, V, IR_W, F21i, nullptr, nullptr);
#pragma unroll
    for (int e = 0; e < 9; ++e) hyp[(size_t)(18 + e) * nit] = F21i[e];
  }
}

// The score of one hypothesis is a sequential float sum over the match list,
// two terms per match, and stays one: the chi-squares of a tile of IR_TILE
// matches x 64 hypotheses are computed side by side by the whole workgroup into
// LDS ([match][term][hypothesis], lane-minor), then the first wavefront adds
// them in list order, one hypothesis per lane, with the running sum carried
// across tiles in a register (ir_accumulate: the comparison and the addition of
// the sequential form, on the same values).  Two tile buffers and one barrier per
// tile: while the first wavefront adds tile k, the others fill tile k + 1; tile
// k's buffer is written again only after the barrier of tile k + 1, which the
// first wavefront reaches after its additions.
__global__ __launch_bounds__(IR_SCORE_T) void k_ir_score(const IrProblem* __restrict__ probs, int nit, int nchunk,
                                                         float inv_sigma2) {
  __shared__ float s_chi[2][IR_TILE][2][IR_W];
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  const int p = b >> 1, model = b & 1;
  const int h = threadIdx.x & (IR_W - 1), sub = threadIdx.x / IR_W;  // sub is wave-uniform
  const int it = chunk * IR_W + h;
  const int itc = it < nit ? it : nit - 1;  // lanes past the end repeat the last hypothesis and write nothing
  const IrProblem& P = probs[p];
  const IrRec* __restrict__ rec = P.rec;
  const int nmatch = P.nmatch;
  const float* hyp = P.hyp + itc;
  float M[18];
#pragma unroll
  for (int e = 0; e < 18; ++e) M[e] = (model == 0 || e < 9) ? hyp[(size_t)((model ? 18 : 0) + e) * nit] : 0.0f;
  const float th = model ? IR_TH_F : IR_TH_H;
  float score = 0.0f;
  for (int base = 0, k = 0; base < nmatch; base += IR_TILE, ++k) {
    float(*chi)[2][IR_W] = s_chi[k & 1];
#pragma unroll
    for (int j = 0; j < IR_TILE / IR_SCORE_SUB; ++j) {
      const int m = j * IR_SCORE_SUB + sub;
      if (base + m < nmatch) {
        const IrRec r = rec[base + m];
        float c1, c2;
        if (model == 0)
          ir_chi_h(M, M + 9, r.u1, r.v1, r.u2, r.v2, inv_sigma2, &c1, &c2);
        else
          ir_chi_f(M, r.u1, r.v1, r.u2, r.v2, inv_sigma2, &c1, &c2);
        chi[m][0][h] = c1;
        chi[m][1][h] = c2;
      }
    }
    __syncthreads();
    if (sub == 0) {
      const int cnt = nmatch - base < IR_TILE ? nmatch - base : IR_TILE;
      for (int m = 0; m < cnt; ++m) {
        ir_accumulate(chi[m][0][h], th, IR_TH_SCORE, &score);
        ir_accumulate(chi[m][1][h], th, IR_TH_SCORE, &score);
      }
    }
  }
  if (sub == 0 && it < nit) P.score[(size_t)model * nit + it] = score;
}

// `if (currentScore > score)` from score = 0 in iteration order
// (:114, :159) leaves the largest score above 0 at its first iteration; a NaN
// compares false and never wins.  Each lane scans its iterations in ascending
// order, then a tree takes the larger score, of equal scores the lower
// iteration.  The flags are recomputed from the winner's matrix: the same
// function on the same inputs as the score pass.
__global__ __launch_bounds__(IR_SELECT_T) void k_ir_select(const IrProblem* __restrict__ probs, int nit,
                                                           float inv_sigma2) {
  __shared__ float s_best[IR_SELECT_T];
  __shared__ int s_it[IR_SELECT_T];
  __shared__ float s_M[18];
  __shared__ float s_S[2];
  const IrProblem& P = probs[blockIdx.x];
  const int t = threadIdx.x;
  const int nmatch = P.nmatch;
  for (int model = 0; model < 2; ++model) {
    const float* score = P.score + (size_t)model * nit;
    float best = 0.0f;
    int bi = -1;
    for (int it = t; it < nit; it += IR_SELECT_T) {
      const float s = score[it];
      if (s > best) {
        best = s;
        bi = it;
      }
    }
    s_best[t] = best;
    s_it[t] = bi;
    __syncthreads();
    for (int off = IR_SELECT_T / 2; off > 0; off >>= 1) {
      if (t < off) {
        const float ob = s_best[t + off];
        const int oi = s_it[t + off];
        // oi >= 0 implies ob > 0; an empty slot (score 0, -1) never displaces
        if (oi >= 0 && (ob > s_best[t] || (ob == s_best[t] && oi < s_it[t]))) {
          s_best[t] = ob;
          s_it[t] = oi;
        }
      }
      __syncthreads();
    }
    const int win = s_it[0];
    const float S = s_best[0];
    const int nm = model ? 9 : 18, base = model ? 18 : 0;
    if (t < nm) s_M[t] = win >= 0 ? P.hyp[(size_t)(base + t) * nit + win] : 0.0f;
    __syncthreads();
    uint8_t* inl = model ? P.inl_F : P.inl_H;
    for (int i = t; i < nmatch; i += IR_SELECT_T) {
      int in = 0;
      if (win >= 0) {
        const IrRec r = P.rec[i];
        float unused = 0.0f;
        in = model ? ir_check_f(s_M, r.u1, r.v1, r.u2, r.v2, inv_sigma2, &unused)
                   : ir_check_h(s_M, s_M + 9, r.u1, r.v1, r.u2, r.v2, inv_sigma2, &unused);
      }
      inl[i] = (uint8_t)in;
    }
    if (t < 9) (model ? P.res->F21 : P.res->H21)[t] = s_M[t];
    if (t == 0) {
      s_S[model] = S;
      if (model)
        P.res->it_F = win;
      else
        P.res->it_H = win;
    }
    __syncthreads();  // s_M, s_best and s_it are reused by the next model
  }
  if (t == 0) {
    const float SH = s_S[0], SF = s_S[1];
    P.res->SH = SH;
    P.res->SF = SF;
    P.res->RH = SH / (SH + SF);  // :72
    P.res->nmatch = nmatch;
  }
}

void launch_initransac(const IrProblem* d_probs, int npair, int nit, float inv_sigma2, hipStream_t s) {
  if (nit > 0) {
    const int nchunk = (nit + IR_W - 1) / IR_W;
    const dim3 grid((unsigned)npair * (unsigned)nchunk);
    hipLaunchKernelGGL(k_ir_hypothesis<0>, grid, dim3(IR_W), 0, s, d_probs, nit, nchunk);
    hipLaunchKernelGGL(k_ir_hypothesis<1>, grid, dim3(IR_W), 0, s, d_probs, nit, nchunk);
    hipLaunchKernelGGL(k_ir_score, dim3(2u * grid.x), dim3(IR_SCORE_T), 0, s, d_probs, nit, nchunk, inv_sigma2);
  }
  hipLaunchKernelGGL(k_ir_select, dim3((unsigned)npair), dim3(IR_SELECT_T), 0, s, d_probs, nit, inv_sigma2);
}

}  // namespace orbx

/* initrecon_ref.c -- CPU restatement of Initializer::ReconstructH /
 * ReconstructF with CheckRT (src/Initializer.cc:406-864) over
 * csrc/initrecon_math.h, which holds all the arithmetic.  Built
 * by tests/initrecon_util.py with gcc -O2 -ffp-contract=off and loaded with
 * ctypes.
 *
 * The control flow stated here:
 *   - N = the set flags (:409-415, :496-502); CheckRT visits the match list in
 *     order and skips the matches whose flag is clear (:757-761)
 *   - ReconstructH's exit on close singular values returns before any CheckRT
 *   - per candidate: nGood counts the matches that pass the five tests, their
 *     cosines are collected (:824), vP3D[first] is written for each (:825) and
 *     vbGood[first] only under `cosParallax < 0.99998` (:827)
 *   - the parallax is that of the element at min(50, nGood - 1) of the sorted
 *     cosines (:833-840), 0 without a counted match; the sort is over rc_key's
 *     total order (NaN last: a deviation, the reference's is undefined there)
 *   - the decisions of :434-489 and :609-650 (rc_decide_f / rc_decide_h); on
 *     false R21, t21, the points and the flags are zero here
 *   - an absent model matrix (the RANSAC had no winner) gives false with no
 *     candidate */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../orb-slam-system_amd/csrc/initrecon_math.h"

enum {
  RCC_ABSENT,                      /* the model's matrix is absent */
  RCC_EARLY_EXIT,                  /* :517-520 */
  RCC_BRANCH,                      /* RC_NBRANCH counters: CheckRT's exits over all candidates */
  RCC_H_OUT = RCC_BRANCH + RC_NBRANCH, /* RC_H_NOUT counters */
  RCC_F_OUT = RCC_H_OUT + RC_H_NOUT,   /* RC_F_NOUT counters */
  RCC_NAN_COS = RCC_F_OUT + RC_F_NOUT, /* counted matches whose cosine is NaN */
  RCC_J4_SWEEPS_MAX,               /* the 4x4 Jacobi */
  RCC_J4_CAPPED,
  RCC_J3_SWEEPS_MAX,               /* the 3x3 Jacobi of the candidates */
  RCC_J3_CAPPED,
  RCC_WINNER_COUNTED_NOT_GOOD,     /* matches of the winner with a point but no flag */
  RCC_N
};

int rc_ref_ncounters(void) { return RCC_N; }
int rc_ref_choose_model(float RH) { return rc_choose_model(RH); }
double rc_ref_acos(double x) { return rc_acos(x); }
float rc_ref_parallax(float c) { return rc_parallax(c); }
float rc_ref_th2(float sigma) { return rc_th2(sigma); }
uint32_t rc_ref_key(float c) { return rc_key(c); }
float rc_ref_unkey(uint32_t k) { return rc_unkey(k); }

static int cmp_u32(const void* a, const void* b) {
  const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
  return x < y ? -1 : x > y;
}

/* res: the 33 words of orbx_recon_result (ok, model_used, R21[9], t21[3], best,
 * ncand, nGood[8], parallax[8], n_inliers).  keys: x, y at keys[i * kstride].
 * model: 0 = H, 1 = F; M its matrix, present = 0 when the RANSAC left none;
 * flags: one per entry of the match list.  P3D[n1][3], tri[n1].  Optional:
 * counters[RCC_N], cand[8][27] (R, t, P2, O2), branches[8][N] (the RC_* exit of
 * every inlier match under every candidate, inlier order), cosv[8][N].
 * Returns N, or -1 for an index the reference would read out of range. */
int rc_ref_reconstruct(int n1, const float* keys1, int n2, const float* keys2, int kstride, const int32_t* match12,
                       const float* K, int model, int present, const float* M, const uint8_t* flags, float sigma,
                       float minParallax, int minTriangulated, int32_t* res, float* P3D, uint8_t* tri,
                       int32_t* counters, float* cand_out, uint8_t* branches, float* cosv) {
  int nmatch = 0;
  for (int i = 0; i < n1; ++i) {
    if (match12[i] >= n2) return -1;
    nmatch += match12[i] >= 0;
  }
  int N = 0;
  for (int i = 0; i < nmatch; ++i) N += flags[i] != 0;
  int32_t* first = (int32_t*)malloc(sizeof(int32_t) * (N + 1) * 2);
  int32_t* second = first + N + 1;
  for (int i = 0, m = 0, k = 0; i < n1; ++i)
    if (match12[i] >= 0 && flags[m++]) {
      first[k] = i;
      second[k++] = match12[i];
    }
  if (counters) memset(counters, 0, sizeof(int32_t) * RCC_N);
  memset(res, 0, sizeof(int32_t) * 33);
  memset(P3D, 0, sizeof(float) * 3 * n1);
  memset(tri, 0, n1);
  float* resf = (float*)res;
  int32_t* nGood = res + 16;
  float* parallax = resf + 24;
  res[1] = model;
  res[14] = -1;
  res[32] = N;
  rc_cand cand[8];
  memset(cand, 0, sizeof cand);
  float A[16], V[16];
  ir_jacobi_stats st3;
  memset(&st3, 0, sizeof st3);
  int ncand = 0;
  if (!present) {
    if (counters) ++counters[RCC_ABSENT];
  } else if (model == 0) {
    ncand = rc_candidates_h(M, K, A, V, 1, cand, &st3);
    if (ncand == 0 && counters) ++counters[RCC_EARLY_EXIT];
  } else {
    ncand = rc_candidates_f(M, K, A, V, 1, cand, &st3);
  }
  if (counters) {
    counters[RCC_J3_SWEEPS_MAX] = st3.sweeps;
    counters[RCC_J3_CAPPED] = st3.capped;
  }
  res[15] = ncand;
  if (cand_out) memcpy(cand_out, cand, sizeof cand);
  float P1[12];
  rc_p1(K, P1);
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float th2 = rc_th2(sigma);
  float* p3d = (float*)malloc(sizeof(float) * 3 * 8 * (N + 1));
  uint8_t* code = (uint8_t*)malloc(8 * (N + 1));
  uint32_t* keys = (uint32_t*)malloc(sizeof(uint32_t) * (N + 1));
  memset(code, 0, 8 * (N + 1));
  for (int c = 0; c < ncand; ++c) {
    int n = 0;
    for (int i = 0; i < N; ++i) {
      const float u1 = keys1[(long)first[i] * kstride], v1 = keys1[(long)first[i] * kstride + 1];
      const float u2 = keys2[(long)second[i] * kstride], v2 = keys2[(long)second[i] * kstride + 1];
      float cosp;
      ir_jacobi_stats st;
      memset(&st, 0, sizeof st);
      const int b = rc_check_match(&cand[c], P1, fx, fy, cx, cy, u1, v1, u2, v2, th2, A, V, 1, p3d + 3 * (c * N + i),
                                   &cosp, &st);
      if (counters) {
        ++counters[RCC_BRANCH + b];
        if (st.sweeps > counters[RCC_J4_SWEEPS_MAX]) counters[RCC_J4_SWEEPS_MAX] = st.sweeps;
        counters[RCC_J4_CAPPED] += st.capped;
      }
      if (cosv) cosv[c * N + i] = cosp;
      if (branches) branches[c * N + i] = (uint8_t)b;
      if (b == RC_COUNTED || b == RC_GOOD) {
        code[c * N + i] = b == RC_GOOD ? 2 : 1;
        keys[n++] = rc_key(cosp);
        if (counters && cosp != cosp) ++counters[RCC_NAN_COS];
      }
    }
    nGood[c] = n;
    if (n > 0) {
      qsort(keys, n, sizeof(uint32_t), cmp_u32);
      parallax[c] = rc_parallax(rc_unkey(keys[rc_parallax_index(n)]));
    } else {
      parallax[c] = 0;
    }
  }
  int best = -1, ok = 0;
  if (ncand == 8) {
    const int out = rc_decide_h(nGood, parallax, N, minParallax, minTriangulated, &best);
    if (counters) ++counters[RCC_H_OUT + out];
    ok = out == RC_H_OK;
  } else if (ncand == 4) {
    const int out = rc_decide_f(nGood, parallax, N, minParallax, minTriangulated, &best);
    if (counters) ++counters[RCC_F_OUT + out];
    ok = out < RC_F_MINGOOD;
  }
  res[0] = ok;
  res[14] = best;
  if (ok) {
    memcpy(resf + 2, cand[best].R, sizeof(float) * 9);
    memcpy(resf + 11, cand[best].t, sizeof(float) * 3);
    for (int i = 0; i < N; ++i) {
      const int cd = code[best * N + i];
      if (!cd) continue;
      memcpy(P3D + 3 * first[i], p3d + 3 * (best * N + i), sizeof(float) * 3);
      tri[first[i]] = cd == 2;
      if (counters && cd == 1) ++counters[RCC_WINNER_COUNTED_NOT_GOOD];
    }
  }
  free(keys);
  free(code);
  free(p3d);
  free(first);
  return N;
}

/* initransac_math.h -- the f32 arithmetic of Initializer's homography /
 * fundamental RANSAC, shared by the kernels
 * (kernels_initransac.hip), the host side of the call (api_initransac.hip) and
 * the CPU restatement (tests/cpp/initransac_ref.c) so that all round alike:
 * plain C, IEEE add / sub / mul / div and sqrtf only, no other libm call,
 * compiled with -ffp-contract=off on both targets.
 *
 * What is restated from the reference (src/Initializer.cc):
 *   Normalize                           :669-721
 *   the DLT rows of ComputeH21/F21      :171-205, :211-235
 *   CheckHomography / CheckFundamental  :250-328, :330-404 (per-match terms)
 * What is a fixed form of this header because OpenCV cannot be read here
 * ("unpinned"): cv::SVDecomp (one-sided Jacobi below), cv::Mat's
 * 3x3 products (summed left to right) and cv::Mat::inv (adjugate in double).
 *
 * Matrices are addressed with a stride: element e of a matrix at base M is
 * M[e * S].  The restatement passes S = 1; a kernel keeps one matrix per lane
 * in LDS, lane-minor, and passes S = 64. */
#ifndef ORBX_INITRANSAC_MATH_H
#define ORBX_INITRANSAC_MATH_H

#include <math.h>

#include "orbx_sincos.h" /* ORBX_HD */

#define IR_TH_H 5.991f     /* CheckHomography :278 */
#define IR_TH_F 3.841f     /* CheckFundamental :348 */
#define IR_TH_SCORE 5.991f /* :349 */

/* the Jacobi's fixed parameters: a pair is left alone when its columns are
 * orthogonal to IR_TOL (gamma^2 <= IR_TOL^2 alpha beta) or when one of them has
 * vanished (squared norm <= IR_FLOOR x the squared Frobenius norm of the input:
 * a column of rounding noise never passes the first test); a sweep without a
 * rotation ends the loop, IR_SWEEPS caps it */
#define IR_SWEEPS 30
#define IR_MAXROWS 16 /* the largest m ir_jacobi is called with */
#define IR_TOL2 5.6843419e-14f /* (2^-22)^2 */
#define IR_FLOOR 1e-13f

/* coverage counters of one Jacobi run (the restatement's; NULL on the device) */
typedef struct {
  int sweeps, rotations, skipped_orth, skipped_floor, capped;
} ir_jacobi_stats;

/* Normalize (:669-721) over n points (x, y at pts[i * stride], pts[i * stride
 * + 1]): sequential float sums over all of them; 1.0 / meanDev is a double
 * division rounded to float (:705-706).  out[2 n], T row-major 3x3 */
static ORBX_HD inline void ir_normalize(const float* pts, int stride, int n, float* out, float T[9]) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; ++i) {
    meanX += pts[(long)i * stride];
    meanY += pts[(long)i * stride + 1];
  }
  meanX = meanX / n;
  meanY = meanY / n;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; ++i) {
    const float x = pts[(long)i * stride] - meanX, y = pts[(long)i * stride + 1] - meanY;
    out[2 * i] = x;
    out[2 * i + 1] = y;
    meanDevX += x < 0 ? -x : x; /* fabs; a float sum of floats either way */
    meanDevY += y < 0 ? -y : y;
  }
  meanDevX = meanDevX / n;
  meanDevY = meanDevY / n;
  const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
  for (int i = 0; i < n; ++i) {
    out[2 * i] *= sX;
    out[2 * i + 1] *= sY;
  }
  T[0] = sX, T[1] = 0, T[2] = -meanX * sX;
  T[3] = 0, T[4] = sY, T[5] = -meanY * sY;
  T[6] = 0, T[7] = 0, T[8] = 1;
}

/* rows 2 i and 2 i + 1 of ComputeH21's A (:185-203) */
static ORBX_HD inline void ir_rows_h(float* A, int S, int i, float u1, float v1, float u2, float v2) {
  float* r = A + (long)(2 * i) * 9 * S;
  r[0 * S] = 0.0f, r[1 * S] = 0.0f, r[2 * S] = 0.0f;
  r[3 * S] = -u1, r[4 * S] = -v1, r[5 * S] = -1.0f;
  r[6 * S] = v2 * u1, r[7 * S] = v2 * v1, r[8 * S] = v2;
  r += 9 * S;
  r[0 * S] = u1, r[1 * S] = v1, r[2 * S] = 1.0f;
  r[3 * S] = 0.0f, r[4 * S] = 0.0f, r[5 * S] = 0.0f;
  r[6 * S] = -u2 * u1, r[7 * S] = -u2 * v1, r[8 * S] = -u2;
}

/* row i of ComputeF21's A (:225-233) */
static ORBX_HD inline void ir_row_f(float* A, int S, int i, float u1, float v1, float u2, float v2) {
  float* r = A + (long)i * 9 * S;
  r[0 * S] = u2 * u1, r[1 * S] = u2 * v1, r[2 * S] = u2;
  r[3 * S] = v2 * u1, r[4 * S] = v2 * v1, r[5 * S] = v2;
  r[6 * S] = u1, r[7 * S] = v1, r[8 * S] = 1.0f;
}

/* One-sided (Hestenes) Jacobi on the n columns of the m x n matrix A (row-major,
 * stride S): A <- A V with orthogonal columns, V (n x n, stride S) accumulated
 * from the identity.  Pairs (p, q), p < q, in cyclic row order.  Standing in for
 * cv::SVDecomp (:207, :239, :243).  Returns the sweeps run. */
static ORBX_HD inline int ir_jacobi(float* A, int m, int n, float* V, int S, ir_jacobi_stats* st) {
  float fro2 = 0;
  for (int e = 0; e < m * n; ++e) fro2 += A[e * S] * A[e * S];
  const float floor2 = IR_FLOOR * fro2;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[(i * n + j) * S] = i == j ? 1.0f : 0.0f;
  int sweep = 0, rotated = 1;
  while (rotated && sweep < IR_SWEEPS) {
    rotated = 0;
    ++sweep;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        /* both columns are read once, before anything is written: on the device
         * the reads then go out together instead of one per LDS round trip
         * (m and n are constants at every call site, so the loops unroll and
         * the copies stay in registers) */
        float ap[IR_MAXROWS], aq[IR_MAXROWS];
        for (int i = 0; i < m; ++i) {
          ap[i] = A[(i * n + p) * S];
          aq[i] = A[(i * n + q) * S];
        }
        float alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < m; ++i) {
          alpha += ap[i] * ap[i];
          beta += aq[i] * aq[i];
          gamma += ap[i] * aq[i];
        }
        if (alpha <= floor2 || beta <= floor2) {
          if (st) ++st->skipped_floor;
          continue;
        }
        if (gamma * gamma <= IR_TOL2 * (alpha * beta)) {
          if (st) ++st->skipped_orth;
          continue;
        }
        rotated = 1;
        if (st) ++st->rotations;
        float vp[9], vq[9];
        for (int i = 0; i < n; ++i) {
          vp[i] = V[(i * n + p) * S];
          vq[i] = V[(i * n + q) * S];
        }
        const float zeta = (beta - alpha) / (2.0f * gamma);
        const float az = zeta < 0 ? -zeta : zeta;
        float t = 1.0f / (az + sqrtf(1.0f + zeta * zeta));
        if (zeta < 0) t = -t;
        const float c = 1.0f / sqrtf(1.0f + t * t), s = c * t;
        for (int i = 0; i < m; ++i) {
          A[(i * n + p) * S] = c * ap[i] - s * aq[i];
          A[(i * n + q) * S] = s * ap[i] + c * aq[i];
        }
        for (int i = 0; i < n; ++i) {
          V[(i * n + p) * S] = c * vp[i] - s * vq[i];
          V[(i * n + q) * S] = s * vp[i] + c * vq[i];
        }
      }
  }
  if (st) {
    st->sweeps += sweep;
    if (rotated) ++st->capped;
  }
  return sweep;
}

/* the squared norm of column j of the rotated A */
static ORBX_HD inline float ir_colnorm2(const float* A, int m, int n, int j, int S) {
  float a = 0;
  for (int i = 0; i < m; ++i) a += A[(i * n + j) * S] * A[(i * n + j) * S];
  return a;
}

/* vt.row(8) (:208, :241): the column of V whose singular value comes last in
 * the descending order, which is stable (of equal norms the later column) */
static ORBX_HD inline void ir_null_vector(const float* A, int m, const float* V, int S, float h[9]) {
  int best = 0;
  float nb = ir_colnorm2(A, m, 9, 0, S);
  for (int j = 1; j < 9; ++j) {
    const float nj = ir_colnorm2(A, m, 9, j, S);
    if (nj <= nb) { /* a NaN norm never displaces the current one */
      nb = nj;
      best = j;
    }
  }
  for (int i = 0; i < 9; ++i) h[i] = V[(i * 9 + best) * S];
}

/* ComputeF21's tail (:243-247): the SVD of Fpre by the same Jacobi (A and V
 * are work space of 9 elements each, stride S), w[2] = 0, u diag(w) vt with
 * each entry summed left to right.  U's columns are the rotated columns over
 * their norms; a column of norm 0 gives a zero column of U */
static ORBX_HD inline void ir_rank2(const float Fpre[9], float* A, float* V, int S, float F[9], ir_jacobi_stats* st) {
  for (int e = 0; e < 9; ++e) A[e * S] = Fpre[e];
  ir_jacobi(A, 3, 3, V, S, st);
  float w0 = sqrtf(ir_colnorm2(A, 3, 3, 0, S)), w1 = sqrtf(ir_colnorm2(A, 3, 3, 1, S)),
        w2 = sqrtf(ir_colnorm2(A, 3, 3, 2, S));
  int o0 = 0, o1 = 1, o2 = 2;
  /* stable insertion sort, descending (scalars: nothing indexed by a variable) */
#define IR_SWAP(wa, wb, oa, ob) \
  do {                          \
    const float tw = wa;        \
    wa = wb;                    \
    wb = tw;                    \
    const int to = oa;          \
    oa = ob;                    \
    ob = to;                    \
  } while (0)
  if (w1 > w0) IR_SWAP(w0, w1, o0, o1);
  if (w2 > w1) {
    IR_SWAP(w1, w2, o1, o2);
    if (w1 > w0) IR_SWAP(w0, w1, o0, o1);
  }
#undef IR_SWAP
  float uw[9]; /* u * diag(w), w[2] = 0 */
  for (int i = 0; i < 3; ++i) {
    const float u0 = w0 > 0 ? A[(i * 3 + o0) * S] / w0 : 0.0f;
    const float u1 = w1 > 0 ? A[(i * 3 + o1) * S] / w1 : 0.0f;
    const float u2 = w2 > 0 ? A[(i * 3 + o2) * S] / w2 : 0.0f;
    uw[i * 3 + 0] = u0 * w0;
    uw[i * 3 + 1] = u1 * w1;
    uw[i * 3 + 2] = u2 * 0.0f;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      F[i * 3 + j] = (uw[i * 3 + 0] * V[(j * 3 + o0) * S] + uw[i * 3 + 1] * V[(j * 3 + o1) * S]) +
                     uw[i * 3 + 2] * V[(j * 3 + o2) * S];
}

/* C = A * B, 3x3 row-major, each entry summed left to right in float */
static ORBX_HD inline void ir_mul3(const float A[9], const float B[9], float C[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = (A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j]) + A[i * 3 + 2] * B[2 * 3 + j];
}

static ORBX_HD inline void ir_transpose3(const float A[9], float At[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) At[i * 3 + j] = A[j * 3 + i];
}

/* T2.inv() (:87) and H21i.inv() (:110): the adjugate over the determinant in
 * double, rounded to float; a zero determinant leaves the zero matrix */
static ORBX_HD inline void ir_inv3(const float M[9], float R[9]) {
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
  const double A0 = e * i - f * h, A1 = c * h - b * i, A2 = b * f - c * e;
  const double A3 = f * g - d * i, A4 = a * i - c * g, A5 = c * d - a * f;
  const double A6 = d * h - e * g, A7 = b * g - a * h, A8 = a * e - b * d;
  const double det = (a * A0 + b * A3) + c * A6;
  if (det == 0.0) {
    for (int k = 0; k < 9; ++k) R[k] = 0.0f;
    return;
  }
  R[0] = (float)(A0 / det), R[1] = (float)(A1 / det), R[2] = (float)(A2 / det);
  R[3] = (float)(A3 / det), R[4] = (float)(A4 / det), R[5] = (float)(A5 / det);
  R[6] = (float)(A6 / det), R[7] = (float)(A7 / det), R[8] = (float)(A8 / det);
}

/* invSigmaSquare (:280, :351): sigma * sigma in float, the division in double */
static ORBX_HD inline float ir_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

/* `if (chiSquare > th) bIn = false; else score += thScore - chiSquare;`
 * (:302-305, :376-379): kept as a comparison, so a NaN chi adds NaN to the score
 * and leaves the match an inlier.  Returns 0 where bIn is cleared */
static ORBX_HD inline int ir_accumulate(float chiSquare, float th, float thScore, float* score) {
  if (chiSquare > th) return 0;
  *score += thScore - chiSquare;
  return 1;
}

/* chiSquare1 and chiSquare2 of one match in CheckHomography (:290-313).  The
 * reference's 1.0 / w is a double division rounded to float; that equals the
 * correctly rounded float division (a quotient of two p-bit numbers rounded
 * first to 2 p + 2 = 50 <= 53 bits and then to p bits is correctly rounded), so
 * the float division stands here */
static ORBX_HD inline void ir_chi_h(const float H[9], const float Hi[9], float u1, float v1, float u2, float v2,
                                    float invSigmaSquare, float* chiSquare1, float* chiSquare2) {
  const float w2in1inv = 1.0f / (Hi[6] * u2 + Hi[7] * v2 + Hi[8]);
  const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
  const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  *chiSquare1 = squareDist1 * invSigmaSquare;
  const float w1in2inv = 1.0f / (H[6] * u1 + H[7] * v1 + H[8]);
  const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
  const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  *chiSquare2 = squareDist2 * invSigmaSquare;
}

/* chiSquare1 and chiSquare2 of one match in CheckFundamental (:361-389) */
static ORBX_HD inline void ir_chi_f(const float F[9], float u1, float v1, float u2, float v2, float invSigmaSquare,
                                    float* chiSquare1, float* chiSquare2) {
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  *chiSquare1 = squareDist1 * invSigmaSquare;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  *chiSquare2 = squareDist2 * invSigmaSquare;
}

/* One match of CheckHomography (:285-323): adds its two terms to *score, in the
 * reference's order, and returns bIn */
static ORBX_HD inline int ir_check_h(const float H[9], const float Hi[9], float u1, float v1, float u2, float v2,
                                     float invSigmaSquare, float* score) {
  float chiSquare1, chiSquare2;
  ir_chi_h(H, Hi, u1, v1, u2, v2, invSigmaSquare, &chiSquare1, &chiSquare2);
  const int in1 = ir_accumulate(chiSquare1, IR_TH_H, IR_TH_H, score);
  const int in2 = ir_accumulate(chiSquare2, IR_TH_H, IR_TH_H, score);
  return in1 & in2;
}

/* One match of CheckFundamental (:356-399), as above */
static ORBX_HD inline int ir_check_f(const float F[9], float u1, float v1, float u2, float v2, float invSigmaSquare,
                                     float* score) {
  float chiSquare1, chiSquare2;
  ir_chi_f(F, u1, v1, u2, v2, invSigmaSquare, &chiSquare1, &chiSquare2);
  const int in1 = ir_accumulate(chiSquare1, IR_TH_F, IR_TH_SCORE, score);
  const int in2 = ir_accumulate(chiSquare2, IR_TH_F, IR_TH_SCORE, score);
  return in1 & in2;
}

/* One hypothesis of FindHomography (:98-110) from its 8 normalised point pairs
 * pn[8][4] = (u1, v1, u2, v2): A (16 x 9) and V (9 x 9) are work space of
 * stride S.  H21i = T2inv * Hn * T1, H12i = H21i.inv() */
static ORBX_HD inline void ir_hypothesis_h(const float pn[8][4], const float T1[9], const float T2inv[9], float* A,
                                           float* V, int S, float H21i[9], float H12i[9], ir_jacobi_stats* st) {
  for (int j = 0; j < 8; ++j) ir_rows_h(A, S, j, pn[j][0], pn[j][1], pn[j][2], pn[j][3]);
  ir_jacobi(A, 16, 9, V, S, st);
  float Hn[9], tmp[9];
  ir_null_vector(A, 16, V, S, Hn);
  ir_mul3(T2inv, Hn, tmp);
  ir_mul3(tmp, T1, H21i);
  ir_inv3(H21i, H12i);
}

/* One hypothesis of FindFundamental (:145-155): F21i = T2t * Fn * T1.  A
 * (8 x 9) and V (9 x 9) as above; both are reused for the 3 x 3 SVD */
static ORBX_HD inline void ir_hypothesis_f(const float pn[8][4], const float T1[9], const float T2t[9], float* A,
                                           float* V, int S, float F21i[9], ir_jacobi_stats* st3,
                                           ir_jacobi_stats* st) {
  for (int j = 0; j < 8; ++j) ir_row_f(A, S, j, pn[j][0], pn[j][1], pn[j][2], pn[j][3]);
  ir_jacobi(A, 8, 9, V, S, st);
  float Fpre[9], Fn[9], tmp[9];
  ir_null_vector(A, 8, V, S, Fpre);
  ir_rank2(Fpre, A, V, S, Fn, st3);
  ir_mul3(T2t, Fn, tmp);
  ir_mul3(tmp, T1, F21i);
}

#endif

/* initrecon_math.h -- the arithmetic of Initializer's ReconstructH /
 * ReconstructF, shared by the kernels (kernels_initrecon.hip),
 * the host side of the call (api_initrecon.hip) and the CPU restatement
 * (tests/cpp/initrecon_ref.c) so that all round alike.  The rules are
 * initransac_math.h's: plain C, f32 unless the reference widens, IEEE add /
 * sub / mul / div and sqrtf / sqrt only, -ffp-contract=off on both targets,
 * matrices addressed with a stride S where they live in LDS.
 *
 * What is restated from the reference (src/Initializer.cc):
 *   ReconstructF   :406-490      ReconstructH   :493-651
 *   Triangulate    :654-667      CheckRT        :725-843
 *   DecomposeE     :844-864      the choice of the model :73
 * What is a fixed form of this header because OpenCV cannot be read here
 * ("unpinned"): the 4x4 and 3x3 full SVD (ir_jacobi, singular
 * values in stable descending order, Vt's rows from V's columns, U's columns
 * the rotated columns over their norms), cv::determinant (rc_det3), cv::norm
 * and cv::Mat::dot of 3-vectors (squares / products summed in double), the
 * 3x3 and 3x4 products (left to right in float), K.inv() (ir_inv3), Mat /
 * scalar (a division per entry), s * U (a product per entry) and acos
 * (rc_acos). */
#ifndef ORBX_INITRECON_MATH_H
#define ORBX_INITRECON_MATH_H

#include <stdint.h>

#include "initransac_math.h"

#define RC_COS_MAX 0.99998 /* :784, :792, :827: a double literal */
#define RC_RATIO_MIN 1.00001 /* :517: a double literal */
#define RC_RH_MIN 0.40 /* :73: a double literal */
#define RC_RANK_TOL 1e-4f /* rc_svd3: a singular value at most this share of the largest has vanished */
#define RC_PI 3.1415926535897932384626433832795 /* CV_PI */

/* the branch one match of CheckRT leaves through */
enum {
  RC_NONFINITE, /* :769 */
  RC_BEHIND1,   /* :784 */
  RC_BEHIND2,   /* :792 */
  RC_ERR1,      /* :805 */
  RC_ERR2,      /* :818 */
  RC_COUNTED,   /* :824-826, cosParallax >= 0.99998 or NaN: vbGood stays false */
  RC_GOOD,      /* :827-828 */
  RC_NBRANCH
};

/* the outcome of ReconstructH's decision (:640): the first term of the && chain
 * that fails */
enum { RC_H_OK, RC_H_SIMILAR, RC_H_PARALLAX, RC_H_MINTRI, RC_H_INLIERS, RC_H_NOUT };
/* of ReconstructF's (:451-489): RC_F_OK + k for candidate k */
enum { RC_F_OK, RC_F_MINGOOD = 4, RC_F_SIMILAR, RC_F_FALLTHROUGH, RC_F_NOUT };

/* one (R, t) candidate with what CheckRT derives from it (:745-750) */
typedef struct {
  float R[9], t[3], P2[12], O2[3];
} rc_cand;

/* `if (RH > 0.40)` (:73): the float is widened to double and compared with the
 * double literal; a NaN RH takes the else branch.  Returns 0 for H, 1 for F */
static ORBX_HD inline int rc_choose_model(float RH) { return (double)RH > RC_RH_MIN ? 0 : 1; }

/* th2 = 4.0 * mSigma2 (:429, :622): mSigma2 = sigma * sigma in float, the
 * product in double, rounded to CheckRT's float parameter */
static ORBX_HD inline float rc_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

/* isfinite without libm: a NaN compares false */
static ORBX_HD inline int rc_finite(float x) { return (x < 0 ? -x : x) <= 3.4028234663852886e38f; }

/* cv::determinant of a 3x3 (unpinned): the expansion along the first row, in
 * float */
static ORBX_HD inline float rc_det3(const float m[9]) {
  return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

/* cv::norm of a 3-vector (unpinned): the squares summed in double left to
 * right, the root in double; the callers round it to float */
static ORBX_HD inline double rc_norm3(float a, float b, float c) {
  return sqrt(((double)a * (double)a + (double)b * (double)b) + (double)c * (double)c);
}

/* acos (unpinned; the one call per candidate is made in double): for a = |x|,
 * acos(a) = 2 atan(r) with r = sqrt((1 - a) / (1 + a)) in [0, 1]; three
 * halvings atan(r) = 2 atan(r / (1 + sqrt(1 + r r))) leave r <= tan(pi / 32),
 * where ten terms of the series end below 1e-19; acos(-a) = pi - acos(a).
 * |x| > 1 and NaN give NaN, as libm does */
static ORBX_HD inline double rc_acos(double x) {
  const double a = x < 0 ? -x : x;
  double r = sqrt((1.0 - a) / (1.0 + a));
  for (int k = 0; k < 3; ++k) r = r / (1.0 + sqrt(1.0 + r * r));
  const double z = r * r;
  double p = 1.0 / 19.0;
  p = 1.0 / 17.0 - z * p;
  p = 1.0 / 15.0 - z * p;
  p = 1.0 / 13.0 - z * p;
  p = 1.0 / 11.0 - z * p;
  p = 1.0 / 9.0 - z * p;
  p = 1.0 / 7.0 - z * p;
  p = 1.0 / 5.0 - z * p;
  p = 1.0 / 3.0 - z * p;
  p = 1.0 - z * p;
  const double v = 16.0 * (r * p);
  return x < 0 ? RC_PI - v : v;
}

/* `acos(vCosParallax[idx]) * 180 / CV_PI` (:837), rounded to the float
 * parallax */
static ORBX_HD inline float rc_parallax(float c) { return (float)(rc_acos((double)c) * 180 / RC_PI); }

/* The total order that stands for std::sort's `<` on the cosines (:835):
 * ascending, -0 before +0, every NaN last (a deviation: the reference's sort is
 * undefined on a NaN).  Keys compare as unsigned integers */
static ORBX_HD inline uint32_t rc_key(float c) {
  if (c != c) return 0xFFFFFFFFu;
  uint32_t u;
  __builtin_memcpy(&u, &c, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static ORBX_HD inline float rc_unkey(uint32_t k) {
  uint32_t u = k == 0xFFFFFFFFu ? 0x7FC00000u : ((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
  float c;
  __builtin_memcpy(&c, &u, 4);
  return c;
}

/* the index CheckRT reads after the sort (:836); nGood > 0 */
static ORBX_HD inline int rc_parallax_index(int nGood) { return nGood - 1 < 50 ? nGood - 1 : 50; }

/* The full SVD of a 3x3 (:508, :847; unpinned): M = U diag(w) Vt with w in
 * stable descending order.  A and V are work space of 9 elements each, stride
 * S.  U's columns are the rotated columns over their norms.  A one-sided Jacobi
 * has no left vector for a singular value that has vanished, and an essential
 * matrix always has one (DecomposeE reads exactly that column, :849), so the
 * third column is completed as OpenCV's FULL_UV completes it, here in a fixed
 * form: when w2 <= RC_RANK_TOL * w0 and w1 is above that bound, U's third column
 * is the cross product of the first two (so det(U) is +1; its sign is not
 * paired with Vt's third row, which is without effect on DecomposeE, where both
 * signs of t are tried and R is negated by its determinant).  Any other column
 * of norm 0 gives a zero column of U: in ReconstructH det(U) and so s are then
 * 0 and every R the zero matrix */
static ORBX_HD inline void rc_svd3(const float M[9], float* A, float* V, int S, float U[9], float w[3], float Vt[9],
                                   ir_jacobi_stats* st) {
  for (int e = 0; e < 9; ++e) A[e * S] = M[e];
  ir_jacobi(A, 3, 3, V, S, st);
  float w0 = sqrtf(ir_colnorm2(A, 3, 3, 0, S)), w1 = sqrtf(ir_colnorm2(A, 3, 3, 1, S)),
        w2 = sqrtf(ir_colnorm2(A, 3, 3, 2, S));
  int o0 = 0, o1 = 1, o2 = 2;
#define RC_SWAP(wa, wb, oa, ob) \
  do {                          \
    const float tw = wa;        \
    wa = wb;                    \
    wb = tw;                    \
    const int to = oa;          \
    oa = ob;                    \
    ob = to;                    \
  } while (0)
  if (w1 > w0) RC_SWAP(w0, w1, o0, o1);
  if (w2 > w1) {
    RC_SWAP(w1, w2, o1, o2);
    if (w1 > w0) RC_SWAP(w0, w1, o0, o1);
  }
#undef RC_SWAP
  for (int i = 0; i < 3; ++i) {
    U[i * 3 + 0] = w0 > 0 ? A[(i * 3 + o0) * S] / w0 : 0.0f;
    U[i * 3 + 1] = w1 > 0 ? A[(i * 3 + o1) * S] / w1 : 0.0f;
    U[i * 3 + 2] = w2 > 0 ? A[(i * 3 + o2) * S] / w2 : 0.0f;
    Vt[0 * 3 + i] = V[(i * 3 + o0) * S];
    Vt[1 * 3 + i] = V[(i * 3 + o1) * S];
    Vt[2 * 3 + i] = V[(i * 3 + o2) * S];
  }
  if (w2 <= RC_RANK_TOL * w0 && w1 > RC_RANK_TOL * w0) {
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
  }
  w[0] = w0, w[1] = w1, w[2] = w2;
}

/* P1 = [K | 0] (:740-741) */
static ORBX_HD inline void rc_p1(const float K[9], float P1[12]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P1[r * 4 + c] = K[r * 3 + c];
    P1[r * 4 + 3] = 0.0f;
  }
}

/* what CheckRT derives from (R, t) before its loop (:745-750): P2 = K [R | t],
 * each entry summed left to right, and O2 = -R.t() * t (the negated transpose
 * times t, left to right) */
static ORBX_HD inline void rc_finish_cand(const float K[9], const float R[9], const float t[3], rc_cand* out) {
  for (int e = 0; e < 9; ++e) out->R[e] = R[e];
  for (int e = 0; e < 3; ++e) out->t[e] = t[e];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      out->P2[r * 4 + c] = (K[r * 3 + 0] * R[0 * 3 + c] + K[r * 3 + 1] * R[1 * 3 + c]) + K[r * 3 + 2] * R[2 * 3 + c];
    out->P2[r * 4 + 3] = (K[r * 3 + 0] * t[0] + K[r * 3 + 1] * t[1]) + K[r * 3 + 2] * t[2];
  }
  for (int i = 0; i < 3; ++i) out->O2[i] = ((-R[0 * 3 + i]) * t[0] + (-R[1 * 3 + i]) * t[1]) + (-R[2 * 3 + i]) * t[2];
}

/* `t / cv::norm(t)` (:556, :595, :850; unpinned): the norm in double, a double
 * division per entry, rounded to float */
static ORBX_HD inline void rc_unit3(const float t[3], float out[3]) {
  const double n = rc_norm3(t[0], t[1], t[2]);
  for (int i = 0; i < 3; ++i) out[i] = (float)((double)t[i] / n);
}

/* Triangulate (:654-667): the four rows of A (a float product and a float
 * difference per entry), the 4x4 SVD (unpinned: ir_jacobi), vt.row(3) = the
 * column of V whose singular value comes last in the stable descending order,
 * and the division by its fourth entry (per entry, in float).  A and V are work
 * space of 16 elements each, stride S */
static ORBX_HD inline void rc_triangulate(const float P1[12], const float P2[12], float u1, float v1, float u2, float v2,
                                          float* A, float* V, int S, float x3D[3], ir_jacobi_stats* st) {
  for (int j = 0; j < 4; ++j) {
    A[(0 * 4 + j) * S] = u1 * P1[8 + j] - P1[0 + j];
    A[(1 * 4 + j) * S] = v1 * P1[8 + j] - P1[4 + j];
    A[(2 * 4 + j) * S] = u2 * P2[8 + j] - P2[0 + j];
    A[(3 * 4 + j) * S] = v2 * P2[8 + j] - P2[4 + j];
  }
  ir_jacobi(A, 4, 4, V, S, st);
  int best = 0;
  float nb = ir_colnorm2(A, 4, 4, 0, S);
  for (int j = 1; j < 4; ++j) {
    const float nj = ir_colnorm2(A, 4, 4, j, S);
    if (nj <= nb) { /* a NaN norm never displaces the current one */
      nb = nj;
      best = j;
    }
  }
  const float x0 = V[(0 * 4 + best) * S], x1 = V[(1 * 4 + best) * S], x2 = V[(2 * 4 + best) * S],
              x3 = V[(3 * 4 + best) * S];
  x3D[0] = x0 / x3;
  x3D[1] = x1 / x3;
  x3D[2] = x2 / x3;
}

/* One inlier match of CheckRT's loop (:763-830), term by term.  Returns the
 * branch it leaves through; p3dC1 and *cosParallax are those of the reference
 * wherever it computes them.
 *   - dist1, dist2: cv::norm, rounded to the float it is assigned to (:777, :780)
 *   - cosParallax (:782): cv::Mat::dot is a double (products and sum in double,
 *     left to right), dist1 * dist2 a float product widened, the quotient a
 *     double rounded to the float
 *   - `z <= 0 && cosParallax < 0.99998` (:784, :792) is kept as written: the
 *     float is widened and compared with the double literal, and a NaN cosine
 *     makes the conjunction false, so the match goes on
 *   - invZ = 1.0 / z (:799, :812) is a double division rounded to float, which
 *     equals the float division (ir_chi_h's argument)
 *   - `squareError > th2` (:805, :818) in float: a NaN error passes */
static ORBX_HD inline int rc_check_match(const rc_cand* C, const float P1[12], float fx, float fy, float cx, float cy,
                                         float u1, float v1, float u2, float v2, float th2, float* A, float* V, int S,
                                         float p3dC1[3], float* cosParallax, ir_jacobi_stats* st) {
  rc_triangulate(P1, C->P2, u1, v1, u2, v2, A, V, S, p3dC1, st);
  *cosParallax = 0.0f;
  if (!rc_finite(p3dC1[0]) || !rc_finite(p3dC1[1]) || !rc_finite(p3dC1[2])) return RC_NONFINITE;
  /* normal1 = p3dC1 - O1 with O1 = 0: the point itself */
  const float n1x = p3dC1[0] - 0.0f, n1y = p3dC1[1] - 0.0f, n1z = p3dC1[2] - 0.0f;
  const float dist1 = (float)rc_norm3(n1x, n1y, n1z);
  const float n2x = p3dC1[0] - C->O2[0], n2y = p3dC1[1] - C->O2[1], n2z = p3dC1[2] - C->O2[2];
  const float dist2 = (float)rc_norm3(n2x, n2y, n2z);
  const double dot = ((double)n1x * (double)n2x + (double)n1y * (double)n2y) + (double)n1z * (double)n2z;
  const float cosp = (float)(dot / (double)(dist1 * dist2));
  *cosParallax = cosp;
  if (p3dC1[2] <= 0 && (double)cosp < RC_COS_MAX) return RC_BEHIND1;
  const float* R = C->R;
  const float x2 = ((R[0] * p3dC1[0] + R[1] * p3dC1[1]) + R[2] * p3dC1[2]) + C->t[0];
  const float y2 = ((R[3] * p3dC1[0] + R[4] * p3dC1[1]) + R[5] * p3dC1[2]) + C->t[1];
  const float z2 = ((R[6] * p3dC1[0] + R[7] * p3dC1[1]) + R[8] * p3dC1[2]) + C->t[2];
  if (z2 <= 0 && (double)cosp < RC_COS_MAX) return RC_BEHIND2;
  const float invZ1 = 1.0f / p3dC1[2];
  const float im1x = fx * p3dC1[0] * invZ1 + cx;
  const float im1y = fy * p3dC1[1] * invZ1 + cy;
  const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
  if (squareError1 > th2) return RC_ERR1;
  const float invZ2 = 1.0f / z2;
  const float im2x = fx * x2 * invZ2 + cx;
  const float im2y = fy * y2 * invZ2 + cy;
  const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
  if (squareError2 > th2) return RC_ERR2;
  return (double)cosp < RC_COS_MAX ? RC_GOOD : RC_COUNTED;
}

/* ReconstructH's candidates (:504-607): A = invK * H21 * K, its SVD, s, the
 * `d1 / d2 < 1.00001 || d2 / d3 < 1.00001` exit (float quotients widened; a NaN
 * quotient does not leave), then the eight (R, t) in the reference's order,
 * each finished with P2 and O2 into cand[0..7].  R = s * U * Rp * Vt is taken
 * as ((s U) Rp) Vt.  The normals vn (:558-566, :597-605) enter no output and
 * are not computed.  sqrt of a float expression rounded to float is sqrtf.
 * A and V are work space of 9 elements each, stride S.  Returns 8, or 0 at the
 * exit */
static ORBX_HD inline int rc_candidates_h(const float H21[9], const float K[9], float* A, float* V, int S, rc_cand* cand,
                                          ir_jacobi_stats* st) {
  float invK[9], tmp[9], M[9], U[9], w[3], Vt[9];
  ir_inv3(K, invK);
  ir_mul3(invK, H21, tmp);
  ir_mul3(tmp, K, M);
  rc_svd3(M, A, V, S, U, w, Vt, st);
  const float s = (float)((double)rc_det3(U) * (double)rc_det3(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < RC_RATIO_MIN || (double)(d2 / d3) < RC_RATIO_MIN) return 0;
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  float sU[9];
  for (int e = 0; e < 9; ++e) sU[e] = s * U[e];
  for (int half = 0; half < 2; ++half)
    for (int i = 0; i < 4; ++i) {
      float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
      float tp[3];
      if (half == 0) {
        Rp[0] = ctheta, Rp[2] = -stheta[i], Rp[6] = stheta[i], Rp[8] = ctheta;
        tp[0] = x1[i], tp[1] = 0.0f, tp[2] = -x3[i];
        for (int e = 0; e < 3; ++e) tp[e] *= d1 - d3;
      } else {
        Rp[0] = cphi, Rp[2] = sphi[i], Rp[4] = -1.0f, Rp[6] = sphi[i], Rp[8] = -cphi;
        tp[0] = x1[i], tp[1] = 0.0f, tp[2] = x3[i];
        for (int e = 0; e < 3; ++e) tp[e] *= d1 + d3;
      }
      float R[9], t[3], tu[3];
      ir_mul3(sU, Rp, tmp);
      ir_mul3(tmp, Vt, R);
      for (int r = 0; r < 3; ++r) t[r] = (U[r * 3 + 0] * tp[0] + U[r * 3 + 1] * tp[1]) + U[r * 3 + 2] * tp[2];
      rc_unit3(t, tu);
      rc_finish_cand(K, R, tu, cand + half * 4 + i);
    }
  return 8;
}

/* ReconstructF's candidates (:417-432): E21 = K.t() * F21 * K, DecomposeE
 * (:844-864: t = u.col(2) over its norm, R1 = u W vt, R2 = u W.t() vt, each
 * negated when its determinant is below 0), then (R1, t), (R2, t), (R1, -t),
 * (R2, -t) into cand[0..3].  Returns 4 */
static ORBX_HD inline int rc_candidates_f(const float F21[9], const float K[9], float* A, float* V, int S, rc_cand* cand,
                                          ir_jacobi_stats* st) {
  float Kt[9], tmp[9], E[9], U[9], w[3], Vt[9];
  ir_transpose3(K, Kt);
  ir_mul3(Kt, F21, tmp);
  ir_mul3(tmp, K, E);
  rc_svd3(E, A, V, S, U, w, Vt, st);
  const float tc[3] = {U[2], U[5], U[8]};
  float t1[3], t2[3];
  rc_unit3(tc, t1);
  for (int e = 0; e < 3; ++e) t2[e] = -t1[e];
  const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  float Wt[9], R1[9], R2[9];
  ir_transpose3(W, Wt);
  ir_mul3(U, W, tmp);
  ir_mul3(tmp, Vt, R1);
  if (rc_det3(R1) < 0)
    for (int e = 0; e < 9; ++e) R1[e] = -R1[e];
  ir_mul3(U, Wt, tmp);
  ir_mul3(tmp, Vt, R2);
  if (rc_det3(R2) < 0)
    for (int e = 0; e < 9; ++e) R2[e] = -R2[e];
  rc_finish_cand(K, R1, t1, cand + 0);
  rc_finish_cand(K, R2, t1, cand + 1);
  rc_finish_cand(K, R1, t2, cand + 2);
  rc_finish_cand(K, R2, t2, cand + 3);
  return 4;
}

/* ReconstructH's decision (:609-650) over the eight nGood / parallax: the
 * running best and second best, then `secondBestGood < 0.75 * bestGood &&
 * bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 *
 * N` (the ints widened to double against the double products; the parallax
 * compared in float, a NaN failing).  *best = bestSolutionIdx (-1 when no
 * candidate counts a match).  Returns the outcome */
static ORBX_HD inline int rc_decide_h(const int32_t* nGood, const float* parallax, int N, float minParallax,
                                      int minTriangulated, int* best) {
  int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
  float bestParallax = -1;
  for (int i = 0; i < 8; ++i) {
    if (nGood[i] > bestGood) {
      secondBestGood = bestGood;
      bestGood = nGood[i];
      bestSolutionIdx = i;
      bestParallax = parallax[i];
    } else if (nGood[i] > secondBestGood) {
      secondBestGood = nGood[i];
    }
  }
  *best = bestSolutionIdx;
  if (!((double)secondBestGood < 0.75 * (double)bestGood)) return RC_H_SIMILAR;
  if (!(bestParallax >= minParallax)) return RC_H_PARALLAX;
  if (!(bestGood > minTriangulated)) return RC_H_MINTRI;
  if (!((double)bestGood > 0.9 * (double)N)) return RC_H_INLIERS;
  return RC_H_OK;
}

/* ReconstructF's decision (:434-489): maxGood, nMinGood = max(static_cast<int>(
 * 0.9 * N), minTriangulated), nsimilar over `nGood > 0.7 * maxGood` (int against
 * double), the `maxGood < nMinGood || nsimilar > 1` exit, then the chain
 * `maxGood == nGoodK && parallaxK > minParallax` in candidate order, which falls
 * through to false when the candidates holding maxGood all lack the parallax.
 * *best = the chosen candidate or -1.  Returns the outcome */
static ORBX_HD inline int rc_decide_f(const int32_t* nGood, const float* parallax, int N, float minParallax,
                                      int minTriangulated, int* best) {
  int maxGood = nGood[3];
  if (nGood[2] > maxGood) maxGood = nGood[2];
  if (nGood[1] > maxGood) maxGood = nGood[1];
  if (nGood[0] > maxGood) maxGood = nGood[0];
  int nMinGood = (int)(0.9 * (double)N);
  if (minTriangulated > nMinGood) nMinGood = minTriangulated;
  int nsimilar = 0;
  for (int k = 0; k < 4; ++k)
    if ((double)nGood[k] > 0.7 * (double)maxGood) nsimilar++;
  *best = -1;
  if (maxGood < nMinGood) return RC_F_MINGOOD;
  if (nsimilar > 1) return RC_F_SIMILAR;
  for (int k = 0; k < 4; ++k)
    if (maxGood == nGood[k] && parallax[k] > minParallax) {
      *best = k;
      return RC_F_OK + k;
    }
  return RC_F_FALLTHROUGH;
}

#endif

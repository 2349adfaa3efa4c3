/* sim3_math.h -- the arithmetic of Sim3Solver, shared by the
 * kernel (kernels_sim3.hip), the host side of the call (api_sim3.hip) and the
 * CPU restatement (tests/cpp/sim3_ref.c) so that all round alike.  The rules are
 * initransac_math.h's: plain C, f32 unless the reference widens, IEEE add / sub
 * / mul / div, fused multiply-add where the reference's object has one
 * (__builtin_fmaf: one instruction on both targets), sqrtf / sqrt and an exact
 * floor; no other libm call; -ffp-contract=off on both targets.
 *
 * What is restated from the reference (src/Sim3Solver.cc):
 *   the constructor's per-correspondence values  :64-78, :88-89
 *   ComputeCentroid :195-204      ComputeSim3 :206-317
 *   CheckInliers    :320-344      Project :362-383, FromCameraToImage :385-403
 * What is pinned from the reference's object (Sim3Solver.cc.o): Project and
 * FromCameraToImage are vdivss (1 / z), two vmulss (invz * X, invz * Y) and two
 * vfmadd132ss (x * fx + cx fused); the constructor's bound is vcvtss2sd, vmulsd
 * by 9.210, vcvttsd2si (truncation to an integer); CheckInliers converts the
 * double dot to float (vcvtsd2ss), the integer bound to float (vcvtsi2ss) and
 * takes `vucomiss bound, err; jbe out`: an inlier needs bound > err, a NaN err
 * is none.
 * What is a fixed form of this header because OpenCV and libm cannot be read
 * here ("unpinned"): cv::reduce and C / P.cols (s3_centroid), the
 * 3x3 products and R * X + t (left to right in float, as §17 and §20 have
 * them), cv::eigen of the symmetric 4x4 (s3_eigen4), Mat::dot and cv::norm
 * (accumulated in double, left to right), atan2 (s3_atan2), 2 * ang * vec /
 * norm(vec), cv::Rodrigues with its sin and cos (s3_rodrigues), and the scaled
 * products s * R * O2, s * R, (1 / s) * R^T and -sRinv * t. */
#ifndef ORBX_SIM3_MATH_H
#define ORBX_SIM3_MATH_H

#include <math.h>
#include <stdint.h>

#include "orbx_sincos.h" /* ORBX_HD, the Cody-Waite constants, orbx_ksin / orbx_kcos */

#define S3_CHI2 9.210 /* :67-68: a double literal */
#define S3_PI 3.1415926535897932384626433832795
#define S3_DBL_EPSILON 2.2204460492503131e-16
/* s3_eigen4: a pair is left alone when apq^2 <= S3_FLOOR x the squared
 * Frobenius norm of N (|apq| <= 1e-7 |N|; kept as that comparison, so a NaN
 * rotates); a sweep without a rotation ends the loop, S3_SWEEPS caps it */
#define S3_SWEEPS 16
#define S3_FLOOR 1e-14f
#define S3_HYP 34 /* floats of one hypothesis: R12 t12 s12 sR12 sR21 t21 */

/* coverage counters of one hypothesis (the restatement's; NULL on the device) */
typedef struct {
  int sweeps, rotations, skipped, capped;
  int rod_identity; /* Rodrigues took theta < DBL_EPSILON */
} s3_stats;

/* one hypothesis: mR12i, mt12i, ms12i, and mT12i / mT21i as (sR, t) */
typedef struct {
  float R[9], t[3], s;
  float sR12[9]; /* rows 0..2 of mT12i are (sR12 | t) */
  float sR21[9], t21[3];
} s3_hyp;

/* what the constructor keeps per correspondence */
typedef struct {
  float X1[3], X2[3]; /* mvX3Dc1, mvX3Dc2 */
  float p1[2], p2[2]; /* mvP1im1, mvP2im2 */
  float th1, th2;     /* mvnMaxError1 / 2 as CheckInliers compares them */
} s3_corr;

static ORBX_HD inline int s3_finite(float x) { return (x < 0 ? -x : x) <= 3.4028234663852886e38f; }

/* one row of a cv::Mat product R * p + t: products summed left to right in
 * float, then + t */
static ORBX_HD inline float s3_row(const float* r, float x, float y, float z, float t) {
  float s = r[0] * x;
  s = s + r[1] * y;
  s = s + r[2] * z;
  return s + t;
}

/* `mvnMaxError1.push_back(9.210 * sigmaSquare1)` (:67) into a vector<size_t>,
 * then `err1 < mvnMaxError1[i]` (:336): the double product truncated to an
 * integer, that integer converted to float.  The caller has checked 0 <=
 * 9.210 * sigma2 < 2^31 */
static ORBX_HD inline float s3_max_error(float sigma2) { return (float)(int32_t)(S3_CHI2 * (double)sigma2); }
/* the host's check of that range; a NaN fails it */
static ORBX_HD inline int s3_sigma2_ok(float sigma2) {
  const double v = S3_CHI2 * (double)sigma2;
  return sigma2 >= 0.0f && v < 2147483648.0;
}

/* FromCameraToImage (:397-401) and the tail of Project (:377-381) */
static ORBX_HD inline void s3_to_image(float X, float Y, float Z, float fx, float fy, float cx, float cy, float* u,
                                       float* v) {
  const float invz = 1.0f / Z;
  const float x = X * invz;
  const float y = Y * invz;
  *u = __builtin_fmaf(x, fx, cx);
  *v = __builtin_fmaf(y, fy, cy);
}

/* the constructor's values of one correspondence (:64-78, :88-89) */
static ORBX_HD inline void s3_make_corr(const float* pos1, const float* pos2, float sigma2_1, float sigma2_2,
                                        const float Rcw1[9], const float tcw1[3], const float Rcw2[9],
                                        const float tcw2[3], const float K1[4], const float K2[4], s3_corr* c) {
  for (int r = 0; r < 3; ++r) {
    c->X1[r] = s3_row(Rcw1 + 3 * r, pos1[0], pos1[1], pos1[2], tcw1[r]);
    c->X2[r] = s3_row(Rcw2 + 3 * r, pos2[0], pos2[1], pos2[2], tcw2[r]);
  }
  s3_to_image(c->X1[0], c->X1[1], c->X1[2], K1[0], K1[1], K1[2], K1[3], &c->p1[0], &c->p1[1]);
  s3_to_image(c->X2[0], c->X2[1], c->X2[2], K2[0], K2[1], K2[2], K2[3], &c->p2[0], &c->p2[1]);
  c->th1 = s3_max_error(sigma2_1);
  c->th2 = s3_max_error(sigma2_2);
}

/* ComputeCentroid (:195-204) on the three columns (points) a, b, c; unpinned:
 * cv::reduce adds the columns left to right in float, C / P.cols multiplies by
 * the double 1 / 3. and rounds to float */
static ORBX_HD inline void s3_centroid(const float a[3], const float b[3], const float c[3], float O[3], float Pr[9]) {
  for (int r = 0; r < 3; ++r) {
    const float sum = (a[r] + b[r]) + c[r];
    O[r] = (float)((double)sum * (1.0 / 3.0));
    Pr[3 * r + 0] = a[r] - O[r];
    Pr[3 * r + 1] = b[r] - O[r];
    Pr[3 * r + 2] = c[r] - O[r];
  }
}

/* one rotation of the two-sided Jacobi on the pair (p, q): app, aqq, apq and,
 * for the two other indices r and s, the entries (arp, arq), (asp, asq); then
 * the columns p and q of V.  tau = (aqq - app) / (2 apq), t = sgn(tau) / (|tau|
 * + sqrt(tau^2 + 1)) (tau = 0 takes +1), c = 1 / sqrt(t^2 + 1), s = t c */
#define S3_ROT2(x, y)                    \
  do {                                   \
    const float x_ = c * (x) - s * (y); \
    const float y_ = s * (x) + c * (y); \
    (x) = x_;                            \
    (y) = y_;                            \
  } while (0)
#define S3_PAIR(app, aqq, apq, arp, arq, asp, asq, v0p, v0q, v1p, v1q, v2p, v2q, v3p, v3q) \
  do {                                                                                     \
    if ((apq) * (apq) <= floor2) {                                                         \
      ++skipped;                                                                           \
    } else {                                                                               \
      const float tau = ((aqq) - (app)) / (2.0f * (apq));                                  \
      const float at = tau < 0 ? -tau : tau;                                               \
      const float tt = 1.0f / (at + sqrtf(tau * tau + 1.0f));                              \
      const float t = tau < 0 ? -tt : tt;                                                  \
      const float c = 1.0f / sqrtf(t * t + 1.0f);                                          \
      const float s = t * c;                                                               \
      (app) = (app) - t * (apq);                                                           \
      (aqq) = (aqq) + t * (apq);                                                           \
      (apq) = 0.0f;                                                                        \
      S3_ROT2(arp, arq);                                                                   \
      S3_ROT2(asp, asq);                                                                   \
      S3_ROT2(v0p, v0q);                                                                   \
      S3_ROT2(v1p, v1q);                                                                   \
      S3_ROT2(v2p, v2q);                                                                   \
      S3_ROT2(v3p, v3q);                                                                   \
      ++rotated;                                                                           \
    }                                                                                      \
  } while (0)

/* cv::eigen of the symmetric 4x4 N (:252; unpinned), as far as ComputeSim3
 * reads it: the eigenvector of the largest eigenvalue, the first of equal ones
 * (eigenvalues descending, stable).  A cyclic two-sided Jacobi in float on the
 * upper triangle, pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), V from the
 * identity; its sign is what the rotations leave.  All on scalars: nothing is
 * indexed by a variable.  n = N11 N12 N13 N14 N22 N23 N24 N33 N34 N44.  Returns
 * the sweeps run */
static ORBX_HD inline int s3_eigen4(const float n[10], float q[4], float w[4], s3_stats* st) {
  float a00 = n[0], a01 = n[1], a02 = n[2], a03 = n[3], a11 = n[4], a12 = n[5], a13 = n[6], a22 = n[7], a23 = n[8],
        a33 = n[9];
  float v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0, v20 = 0, v21 = 0, v22 = 1, v23 = 0,
        v30 = 0, v31 = 0, v32 = 0, v33 = 1;
  float fro2 = a00 * a00;
  fro2 += a11 * a11;
  fro2 += a22 * a22;
  fro2 += a33 * a33;
  fro2 += 2.0f * (a01 * a01);
  fro2 += 2.0f * (a02 * a02);
  fro2 += 2.0f * (a03 * a03);
  fro2 += 2.0f * (a12 * a12);
  fro2 += 2.0f * (a13 * a13);
  fro2 += 2.0f * (a23 * a23);
  const float floor2 = S3_FLOOR * fro2;
  int sweep = 0, rotated = 1, skipped = 0, rotations = 0;
  while (rotated && sweep < S3_SWEEPS) {
    rotated = 0;
    S3_PAIR(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);
    S3_PAIR(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);
    S3_PAIR(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);
    S3_PAIR(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);
    S3_PAIR(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);
    S3_PAIR(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);
    rotations += rotated;
    ++sweep;
  }
  if (st) {
    st->sweeps = sweep;
    st->rotations = rotations;
    st->skipped = skipped;
    st->capped = rotated != 0; /* the last sweep still rotated */
  }
  w[0] = a00, w[1] = a11, w[2] = a22, w[3] = a33;
  /* the first strict maximum; a NaN never displaces */
  float best = a00;
  q[0] = v00, q[1] = v10, q[2] = v20, q[3] = v30;
  if (a11 > best) best = a11, q[0] = v01, q[1] = v11, q[2] = v21, q[3] = v31;
  if (a22 > best) best = a22, q[0] = v02, q[1] = v12, q[2] = v22, q[3] = v32;
  if (a33 > best) best = a33, q[0] = v03, q[1] = v13, q[2] = v23, q[3] = v33;
  return sweep;
}

/* atan(r) for r in [0, 1] in double: rc_acos's core (csrc/initrecon_math.h).
 * Three halvings atan(r) = 2 atan(r / (1 + sqrt(1 + r r))) leave r <= tan(pi /
 * 32), where ten terms of the series end below 1e-19 */
static ORBX_HD inline double s3_atan01(double r) {
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
  return 8.0 * (r * p);
}

/* atan2(y, x) in double for y = a norm (>= 0 or NaN) and x = a float (:258;
 * unpinned).  As IEEE atan2 for y >= 0: a NaN gives NaN, (0, +0) is 0, (0, -0)
 * is pi, (0, x) is 0 or pi by x's sign, (y, 0) is pi / 2, x < 0 is pi minus the
 * angle of |x|.  Infinite arguments are not special-cased (inf / inf is NaN) */
static ORBX_HD inline double s3_atan2(double y, float xf) {
  const double x = (double)xf;
  if (y != y || x != x) return y + x;
  const int xneg = (orbx_f2u(xf) >> 31) != 0; /* -0 included */
  if (y == 0.0) return xneg ? S3_PI : 0.0;
  if (x == 0.0) return S3_PI / 2;
  const double ax = xneg ? -x : x;
  const double a = y <= ax ? s3_atan01(y / ax) : S3_PI / 2 - s3_atan01(ax / y);
  return xneg ? S3_PI - a : a;
}

/* sin and cos in double of a double argument, |x| < 1e5: the Cody-Waite
 * reduction and fdlibm kernels of orbx_sincos.h before its rounding to float */
static ORBX_HD inline void s3_sincos(double x, double* s, double* c) {
  const double kd = orbx_floor_d(x * ORBX_INVPIO2 + 0.5);
  const int k = (int)kd;
  const double r = (x - kd * ORBX_PIO2_1) - kd * ORBX_PIO2_1T;
  const double sr = orbx_ksin(r), cr = orbx_kcos(r);
  const double s0 = (k & 1) ? cr : sr, c0 = (k & 1) ? sr : cr;
  *s = (k & 2) ? -s0 : s0;
  *c = ((k + 1) & 2) ? -c0 : c0;
}

/* cv::Rodrigues of three floats (:264; unpinned), in double: theta = |r|; theta
 * < DBL_EPSILON gives I (a NaN theta takes the else branch); else R = c I + (1
 * - c) r r^T + s [r]x with r / theta taken as r * (1 / theta); each entry
 * rounded to float.  A theta past 1e5 (no quaternion gives one) is outside
 * s3_sincos's range */
static ORBX_HD inline void s3_rodrigues(float vx, float vy, float vz, float R[9], s3_stats* st) {
  double rx = vx, ry = vy, rz = vz;
  const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
  if (theta < S3_DBL_EPSILON) {
    R[0] = 1, R[1] = 0, R[2] = 0, R[3] = 0, R[4] = 1, R[5] = 0, R[6] = 0, R[7] = 0, R[8] = 1;
    if (st) st->rod_identity = 1;
    return;
  }
  double s, c;
  s3_sincos(theta, &s, &c);
  const double c1 = 1.0 - c, itheta = 1.0 / theta;
  rx = rx * itheta, ry = ry * itheta, rz = rz * itheta;
  R[0] = (float)(c + c1 * (rx * rx));
  R[1] = (float)(c1 * (rx * ry) - s * rz);
  R[2] = (float)(c1 * (rx * rz) + s * ry);
  R[3] = (float)(c1 * (rx * ry) + s * rz);
  R[4] = (float)(c + c1 * (ry * ry));
  R[5] = (float)(c1 * (ry * rz) - s * rx);
  R[6] = (float)(c1 * (rx * rz) - s * ry);
  R[7] = (float)(c1 * (ry * rz) + s * rx);
  R[8] = (float)(c + c1 * (rz * rz));
}

/* ComputeSim3 (:206-317) on the three sampled pairs: a1 b1 c1 the columns of
 * P3Dc1i, a2 b2 c2 of P3Dc2i.  q_out (may be NULL) receives the quaternion */
static ORBX_HD inline void s3_compute_sim3(const float a1[3], const float b1[3], const float c1[3], const float a2[3],
                                           const float b2[3], const float c2[3], int fix_scale, s3_hyp* H,
                                           float* q_out, s3_stats* st) {
  /* Step 1 (:218-219) */
  float O1[3], O2[3], Pr1[9], Pr2[9];
  s3_centroid(a1, b1, c1, O1, Pr1);
  s3_centroid(a2, b2, c2, O2, Pr2);
  /* Step 2 (:223): M = Pr2 * Pr1.t() */
  float M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      M[3 * i + j] = (Pr2[3 * i] * Pr1[3 * j] + Pr2[3 * i + 1] * Pr1[3 * j + 1]) + Pr2[3 * i + 2] * Pr1[3 * j + 2];
  /* Step 3 (:231-240): the right-hand sides are float expressions, so the
   * doubles N11..N44 hold float sums and the Mat_<float> takes them unchanged */
  float n[10];
  n[0] = (M[0] + M[4]) + M[8];
  n[1] = M[5] - M[7];
  n[2] = M[6] - M[2];
  n[3] = M[1] - M[3];
  n[4] = (M[0] - M[4]) - M[8];
  n[5] = M[1] + M[3];
  n[6] = M[6] + M[2];
  n[7] = (-M[0] + M[4]) - M[8];
  n[8] = M[5] + M[7];
  n[9] = (-M[0] - M[4]) + M[8];
  /* Step 4 (:252-264) */
  float q[4], w[4];
  s3_eigen4(n, q, w, st);
  if (q_out) q_out[0] = q[0], q_out[1] = q[1], q_out[2] = q[2], q_out[3] = q[3];
  const double nrm = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) + (double)q[3] * (double)q[3]);
  const double ang = s3_atan2(nrm, q[0]); /* :258 */
  /* :260, unpinned: one double factor (2 ang) * (1 / norm), each entry rounded */
  const double f = (2.0 * ang) * (1.0 / nrm);
  const float vx = (float)(f * (double)q[1]), vy = (float)(f * (double)q[2]), vz = (float)(f * (double)q[3]);
  s3_rodrigues(vx, vy, vz, H->R, st);
  const float* R = H->R;
  /* Step 5 (:268): P3 = R * Pr2 */
  float P3[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) P3[3 * i + j] = (R[3 * i] * Pr2[j] + R[3 * i + 1] * Pr2[3 + j]) + R[3 * i + 2] * Pr2[6 + j];
  /* Step 6 (:272-291): Mat::dot in double; cv::pow squares in float, the sum in
   * double, element order */
  if (!fix_scale) {
    double nom = 0, den = 0;
    for (int e = 0; e < 9; ++e) nom += (double)Pr1[e] * (double)P3[e];
    for (int e = 0; e < 9; ++e) den += (double)(P3[e] * P3[e]);
    H->s = (float)(nom / den);
  } else {
    H->s = 1.0f;
  }
  const float s = H->s;
  /* Step 7 (:296), unpinned: R * O2 left to right in float, times s, O1 minus it */
  for (int i = 0; i < 3; ++i) {
    const float ro = (R[3 * i] * O2[0] + R[3 * i + 1] * O2[1]) + R[3 * i + 2] * O2[2];
    H->t[i] = O1[i] - s * ro;
  }
  /* Step 8 (:303, :312-315): s * R per entry; (1.0 / s) in double times R^T,
   * rounded per entry; tinv = -(sRinv * t) */
  const double sinv = 1.0 / (double)s;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      H->sR12[3 * i + j] = s * R[3 * i + j];
      H->sR21[3 * i + j] = (float)(sinv * (double)R[3 * j + i]);
    }
  for (int i = 0; i < 3; ++i)
    H->t21[i] = -((H->sR21[3 * i] * H->t[0] + H->sR21[3 * i + 1] * H->t[1]) + H->sR21[3 * i + 2] * H->t[2]);
}

/* Project (:362-383) of X under (sR | t) and the camera K = fx fy cx cy */
static ORBX_HD inline void s3_project(const float sR[9], const float t[3], const float X[3], const float K[4], float* u,
                                      float* v) {
  const float x = s3_row(sR + 0, X[0], X[1], X[2], t[0]);
  const float y = s3_row(sR + 3, X[0], X[1], X[2], t[1]);
  const float z = s3_row(sR + 6, X[0], X[1], X[2], t[2]);
  s3_to_image(x, y, z, K[0], K[1], K[2], K[3], u, v);
}

/* one correspondence of CheckInliers (:323-343): T12 = (sR12 | t12) with K1,
 * T21 = (sR21 | t21) with K2; dist.dot(dist) in double, rounded to float; the
 * comparison of :336 as the object has it */
static ORBX_HD inline void s3_errors(const float sR12[9], const float t12[3], const float sR21[9], const float t21[3],
                                     const float K1[4], const float K2[4], const s3_corr* c, float* err1,
                                     float* err2) {
  float u, v;
  s3_project(sR12, t12, c->X2, K1, &u, &v); /* vP2im1 */
  const float d1x = c->p1[0] - u, d1y = c->p1[1] - v;
  s3_project(sR21, t21, c->X1, K2, &u, &v); /* vP1im2 */
  const float d2x = u - c->p2[0], d2y = v - c->p2[1];
  *err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
  *err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
}
static ORBX_HD inline int s3_check(const float sR12[9], const float t12[3], const float sR21[9], const float t21[3],
                                   const float K1[4], const float K2[4], const s3_corr* c) {
  float err1, err2;
  s3_errors(sR12, t12, sR21, t21, K1, K2, c, &err1, &err2);
  return (c->th1 > err1) & (c->th2 > err2);
}

#endif /* ORBX_SIM3_MATH_H */

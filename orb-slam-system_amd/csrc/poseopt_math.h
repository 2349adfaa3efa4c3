/* poseopt_math.h -- the scalar double arithmetic of the pose-only optimisation
 * (DESIGN.md §19), shared by the kernel (kernels_poseopt.hip) and the CPU
 * restatement (tests/cpp/poseopt_ref.c) so that both round alike: plain C,
 * IEEE add / sub / mul / div / sqrt only, no libm, compiled with
 * -ffp-contract=off on both sides.
 *
 * What is restated from the reference (g2o as ORB-SLAM2 ships it):
 *   SE3Quat::exp, operator*, map, normalizeRotation   types/se3quat.h:104-110,217-285
 *   the two *OnlyPose edges                           types/types_six_dof_expmap.{h,cpp}
 *   RobustKernelHuber::robustify                      core/robust_kernel_impl.cpp:65-91
 * What is a standard form because Eigen cannot be read here (DESIGN §19,
 * "unpinned"): quaternion from matrix, quaternion * vector, quaternion to
 * matrix, normalisation, the small dense products and the 6x6 LDLT. */
#ifndef ORBX_POSEOPT_MATH_H
#define ORBX_POSEOPT_MATH_H

#include <math.h>

#include "orbx_sincos.h"

/* the fixed summation order: lane t of PO_T adds slots t, t + PO_T,
 * .. in increasing order, then a halving tree over the PO_T partial sums */
#define PO_T 256
/* sums of one linearisation: 21 of H's upper triangle, 6 of b, 1 of chi2 */
#define PO_NSUM 28
#define PO_DBL_MAX 1.7976931348623157e308

typedef struct {
  double q[4]; /* x y z w */
  double t[3];
} po_pose;

typedef struct {
  double fx, fy, cx, cy, bf;
} po_cam;

typedef struct {
  double obs[3]; /* u, v, uright */
  double X[3];   /* Xw */
  double w;      /* invSigma2 */
  int stereo;
} po_edge;

/* sin and cos of a double: orbx_sincos_core's Cody-Waite reduction and kernel
 * polynomials, kept in double.  The quadrant is taken in double arithmetic so
 * that a NaN or huge argument gives the same (NaN) result on every target */
static ORBX_HD inline void po_sincos(double x, double* s, double* c) {
  const double kd = orbx_floor_d(x * ORBX_INVPIO2 + 0.5);
  const double r = (x - kd * ORBX_PIO2_1) - kd * ORBX_PIO2_1T;
  const double sr = orbx_ksin(r), cr = orbx_kcos(r);
  const double m = kd - 4.0 * orbx_floor_d(kd * 0.25);
  if (m == 1.0) {
    *s = cr;
    *c = -sr;
  } else if (m == 2.0) {
    *s = -sr;
    *c = -cr;
  } else if (m == 3.0) {
    *s = -cr;
    *c = sr;
  } else {
    *s = sr;
    *c = cr;
  }
}

/* SE3Quat::normalizeRotation (se3quat.h:280-285) */
static ORBX_HD inline void po_normalize(double q[4]) {
  if (q[3] < 0) {
    q[0] = -q[0];
    q[1] = -q[1];
    q[2] = -q[2];
    q[3] = -q[3];
  }
  const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  q[0] = q[0] / nrm;
  q[1] = q[1] / nrm;
  q[2] = q[2] / nrm;
  q[3] = q[3] / nrm;
}

/* quaternion of a 3x3 matrix (row-major), Shepperd's method */
static ORBX_HD inline void po_quat_from_matrix(const double R[9], double q[4]) {
  double t = (R[0] + R[4]) + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
  } else if (R[0] >= R[4] && R[0] >= R[8]) { /* i = 0, j = 1, k = 2 */
    t = sqrt(((R[0] - R[4]) - R[8]) + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[7] - R[5]) * t;
    q[1] = (R[3] + R[1]) * t;
    q[2] = (R[6] + R[2]) * t;
  } else if (R[4] >= R[8]) { /* i = 1, j = 2, k = 0 */
    t = sqrt(((R[4] - R[8]) - R[0]) + 1.0);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[2] - R[6]) * t;
    q[2] = (R[7] + R[5]) * t;
    q[0] = (R[1] + R[3]) * t;
  } else { /* i = 2, j = 0, k = 1 */
    t = sqrt(((R[8] - R[0]) - R[4]) + 1.0);
    q[2] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3] - R[1]) * t;
    q[0] = (R[2] + R[6]) * t;
    q[1] = (R[5] + R[7]) * t;
  }
}

/* quaternion * vector: v + 2w (q x v) + 2 q x (q x v) */
static ORBX_HD inline void po_rotate(const double q[4], const double v[3], double out[3]) {
  double uv[3];
  uv[0] = q[1] * v[2] - q[2] * v[1];
  uv[1] = q[2] * v[0] - q[0] * v[2];
  uv[2] = q[0] * v[1] - q[1] * v[0];
  uv[0] += uv[0];
  uv[1] += uv[1];
  uv[2] += uv[2];
  out[0] = (v[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]);
  out[1] = (v[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]);
  out[2] = (v[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0]);
}

/* SE3Quat::map (se3quat.h:217-220): _r * xyz + _t */
static ORBX_HD inline void po_map(const po_pose* T, const double X[3], double out[3]) {
  double r[3];
  po_rotate(T->q, X, r);
  out[0] = r[0] + T->t[0];
  out[1] = r[1] + T->t[1];
  out[2] = r[2] + T->t[2];
}

/* SE3Quat::operator* (se3quat.h:104-110): a * b */
static ORBX_HD inline void po_mul(const po_pose* a, const po_pose* b, po_pose* out) {
  double r[3];
  po_rotate(a->q, b->t, r);
  const double ax = a->q[0], ay = a->q[1], az = a->q[2], aw = a->q[3];
  const double bx = b->q[0], by = b->q[1], bz = b->q[2], bw = b->q[3];
  out->t[0] = a->t[0] + r[0];
  out->t[1] = a->t[1] + r[1];
  out->t[2] = a->t[2] + r[2];
  out->q[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
  out->q[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
  out->q[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
  out->q[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
  po_normalize(out->q);
}

/* Converter::toSE3Quat (src/Converter.cc:18-26): floats widened to double */
static ORBX_HD inline void po_from_tcw(const float Tcw[12], po_pose* out) {
  double R[9];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)Tcw[4 * r + c];
    out->t[r] = (double)Tcw[4 * r + 3];
  }
  po_quat_from_matrix(R, out->q);
  po_normalize(out->q);
}

/* Converter::toCvMat(SE3Quat) (src/Converter.cc:28-31,40-48): the homogeneous
 * matrix in double, each entry rounded to float */
static ORBX_HD inline void po_to_tcw(const po_pose* T, float out[16]) {
  const double x = T->q[0], y = T->q[1], z = T->q[2], w = T->q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  out[0] = (float)(1.0 - (tyy + tzz));
  out[1] = (float)(txy - twz);
  out[2] = (float)(txz + twy);
  out[4] = (float)(txy + twz);
  out[5] = (float)(1.0 - (txx + tzz));
  out[6] = (float)(tyz - twx);
  out[8] = (float)(txz - twy);
  out[9] = (float)(tyz + twx);
  out[10] = (float)(1.0 - (txx + tyy));
  out[3] = (float)T->t[0];
  out[7] = (float)T->t[1];
  out[11] = (float)T->t[2];
  out[12] = 0.0f;
  out[13] = 0.0f;
  out[14] = 0.0f;
  out[15] = 1.0f;
}

/* SE3Quat::exp (se3quat.h:223-257); update = (omega, upsilon) */
static ORBX_HD inline void po_exp(const double u[6], po_pose* out) {
  const double ox = u[0], oy = u[1], oz = u[2];
  const double theta = sqrt((ox * ox + oy * oy) + oz * oz);
  const double O[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0}; /* skew(omega) */
  double O2[9], R[9], V[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
  if (theta < 0.00001) {
    for (int i = 0; i < 9; ++i) {
      const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
      R[i] = (id + O[i]) + O2[i];
      V[i] = R[i];
    }
  } else {
    double s, c;
    po_sincos(theta, &s, &c);
    const double a = s / theta;
    const double b = (1 - c) / (theta * theta);
    const double d = (theta - s) / (theta * theta * theta); /* pow(theta, 3) as a product */
    for (int i = 0; i < 9; ++i) {
      const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
      R[i] = (id + a * O[i]) + b * O2[i];
      V[i] = (id + b * O[i]) + d * O2[i];
    }
  }
  po_quat_from_matrix(R, out->q);
  for (int r = 0; r < 3; ++r) out->t[r] = (V[3 * r] * u[3] + V[3 * r + 1] * u[4]) + V[3 * r + 2] * u[5];
  po_normalize(out->q); /* SE3Quat(q, t) */
}

/* computeError of the two edges (types_six_dof_expmap.h:153-157,184-188 with
 * cam_project, .cpp:290-306): e = obs - proj.  Returns the edge's dimension */
static ORBX_HD inline int po_edge_error(const po_cam* K, const po_pose* T, const po_edge* E, double e[3]) {
  double p[3];
  po_map(T, E->X, p);
  if (!E->stereo) {
    /* project2d divides in double */
    e[0] = E->obs[0] - ((p[0] / p[2]) * K->fx + K->cx);
    e[1] = E->obs[1] - ((p[1] / p[2]) * K->fy + K->cy);
    e[2] = 0.0;
    return 2;
  }
  const float invzf = (float)(1.0 / p[2]); /* const float invz = 1.0f/trans_xyz[2] */
  const double invz = (double)invzf;
  const double r0 = p[0] * invz * K->fx + K->cx;
  const double r1 = p[1] * invz * K->fy + K->cy;
  e[0] = E->obs[0] - r0;
  e[1] = E->obs[1] - r1;
  e[2] = E->obs[2] - (r0 - K->bf * invz);
  return 3;
}

/* information * error with information = Identity * w held dense: the zero
 * off-diagonal entries take part, so an infinite error makes a NaN */
static ORBX_HD inline void po_info_times(int D, double w, const double e[3], double we[3]) {
  for (int i = 0; i < D; ++i) {
    double s = (i == 0 ? w : 0.0) * e[0];
    for (int j = 1; j < D; ++j) s = s + (i == j ? w : 0.0) * e[j];
    we[i] = s;
  }
}

/* BaseEdge::chi2: _error.dot(information() * _error) */
static ORBX_HD inline double po_chi2(int D, double w, const double e[3]) {
  double we[3];
  po_info_times(D, w, e, we);
  double s = e[0] * we[0];
  for (int i = 1; i < D; ++i) s = s + e[i] * we[i];
  return s;
}

/* linearizeOplus of the two edges (types_six_dof_expmap.cpp:266-288,335-364) */
static ORBX_HD inline void po_edge_jacobian(const po_cam* K, const po_pose* T, const po_edge* E, double J[18]) {
  double p[3];
  po_map(T, E->X, p);
  const double x = p[0], y = p[1];
  const double invz = 1.0 / p[2];
  const double invz_2 = invz * invz;
  const double fx = K->fx, fy = K->fy;
  J[0] = x * y * invz_2 * fx;
  J[1] = -(1 + (x * x * invz_2)) * fx;
  J[2] = y * invz * fx;
  J[3] = -invz * fx;
  J[4] = 0;
  J[5] = x * invz_2 * fx;
  J[6] = (1 + y * y * invz_2) * fy;
  J[7] = -x * y * invz_2 * fy;
  J[8] = -x * invz * fy;
  J[9] = 0;
  J[10] = -invz * fy;
  J[11] = y * invz_2 * fy;
  if (E->stereo) {
    const double bf = K->bf;
    J[12] = J[0] - bf * y * invz_2;
    J[13] = J[1] + bf * x * invz_2;
    J[14] = J[2];
    J[15] = J[3];
    J[16] = 0;
    J[17] = J[5] - bf * invz_2;
  } else {
    for (int i = 12; i < 18; ++i) J[i] = 0.0;
  }
}

/* RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1].
 * delta is the float threshold widened; dsqr is g2o's `float dsqr` */
static ORBX_HD inline void po_huber(double e, double delta, float dsqr, double rho[2]) {
  if (e <= (double)dsqr) {
    rho[0] = e;
    rho[1] = 1.;
  } else {
    const double sqrte = sqrt(e);
    rho[0] = 2 * sqrte * delta - (double)dsqr;
    rho[1] = delta / sqrte;
  }
}

/* One active edge's terms of a linearisation, added to acc[PO_NSUM]:
 * constructQuadraticForm (base_unary_edge.hpp:43-72) and activeRobustChi2.
 *   acc[0..20]  H += A^T (rho1 Omega) A, upper triangle by rows
 *   acc[21..26] A^T Omega e scaled by rho1 (b is minus this sum)
 *   acc[27]     rho[0], or chi2 without the kernel */
static ORBX_HD inline void po_edge_accumulate_d(const int D, const po_cam* K, const po_pose* T, const po_edge* E,
                                                int robust, double delta, float dsqr, double acc[PO_NSUM]) {
  double e[3], we[3], J[18], rho[2];
  po_edge_error(K, T, E, e);
  const double chi2 = po_chi2(D, E->w, e);
  if (robust) {
    po_huber(chi2, delta, dsqr, rho);
  } else {
    rho[0] = chi2;
    rho[1] = 1.;
  }
  po_edge_jacobian(K, T, E, J);
  po_info_times(D, E->w, e, we);
  const double w1 = rho[1] * E->w;
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      double s = (J[r] * w1) * J[c];
      for (int i = 1; i < D; ++i) s = s + (J[6 * i + r] * w1) * J[6 * i + c];
      acc[k] = acc[k] + s;
      ++k;
    }
  for (int r = 0; r < 6; ++r) {
    double s = J[r] * we[0];
    for (int i = 1; i < D; ++i) s = s + J[6 * i + r] * we[i];
    acc[21 + r] = acc[21 + r] + rho[1] * s;
  }
  acc[27] = acc[27] + rho[0];
}

/* D as a literal, so that the loops over it unroll */
static ORBX_HD inline void po_edge_accumulate(const po_cam* K, const po_pose* T, const po_edge* E, int robust,
                                              double delta, float dsqr, double acc[PO_NSUM]) {
  if (E->stereo)
    po_edge_accumulate_d(3, K, T, E, robust, delta, dsqr, acc);
  else
    po_edge_accumulate_d(2, K, T, E, robust, delta, dsqr, acc);
}

/* BaseEdge::chi2 of the edge at T */
static ORBX_HD inline double po_edge_chi2(const po_cam* K, const po_pose* T, const po_edge* E) {
  double e[3];
  po_edge_error(K, T, E, e);
  return E->stereo ? po_chi2(3, E->w, e) : po_chi2(2, E->w, e);
}

/* an edge's term of activeRobustChi2 alone */
static ORBX_HD inline double po_edge_robust_chi2(const po_cam* K, const po_pose* T, const po_edge* E, int robust,
                                                 double delta, float dsqr) {
  double rho[2];
  const double chi2 = po_edge_chi2(K, T, E);
  if (!robust) return chi2;
  po_huber(chi2, delta, dsqr, rho);
  return rho[0];
}

/* (H + lambda I) x = b by LDL^T with pivoting on the largest remaining
 * |diagonal|; S = the PO_NSUM sums, b = -S[21..26].  Returns 0, leaving x as it
 * was, when a pivot is negative (LinearSolverDense: !isPositive()).  W is 42
 * doubles of work space. */
static ORBX_HD inline int po_solve(const double* S, double lambda, double* W, double* x) {
  double* A = W;      /* 6 x 6 */
  double* y = W + 36; /* 6 */
  int perm[6];
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      A[6 * r + c] = S[k];
      A[6 * c + r] = S[k];
      ++k;
    }
  for (int r = 0; r < 6; ++r) {
    A[7 * r] = A[7 * r] + lambda;
    y[r] = -S[21 + r];
    perm[r] = r;
  }
  for (k = 0; k < 6; ++k) {
    int p = k;
    double best = A[7 * k] < 0 ? -A[7 * k] : A[7 * k];
    for (int i = k + 1; i < 6; ++i) {
      const double a = A[7 * i] < 0 ? -A[7 * i] : A[7 * i];
      if (a > best) {
        best = a;
        p = i;
      }
    }
    if (p != k) {
      for (int c = 0; c < 6; ++c) {
        const double t = A[6 * k + c];
        A[6 * k + c] = A[6 * p + c];
        A[6 * p + c] = t;
      }
      for (int r = 0; r < 6; ++r) {
        const double t = A[6 * r + k];
        A[6 * r + k] = A[6 * r + p];
        A[6 * r + p] = t;
      }
      const double t = y[k];
      y[k] = y[p];
      y[p] = t;
      const int ti = perm[k];
      perm[k] = perm[p];
      perm[p] = ti;
    }
    const double d = A[7 * k];
    if (d < 0) return 0;
    if (d != 0) {
      for (int i = k + 1; i < 6; ++i) A[6 * i + k] = A[6 * i + k] / d; /* L */
      for (int j = k + 1; j < 6; ++j)
        for (int i = j; i < 6; ++i) {
          A[6 * i + j] = A[6 * i + j] - (A[6 * i + k] * d) * A[6 * j + k];
          A[6 * j + i] = A[6 * i + j];
        }
    }
  }
  for (int i = 1; i < 6; ++i) /* L z = P b */
    for (int j = 0; j < i; ++j) y[i] = y[i] - A[6 * i + j] * y[j];
  const double tol = 1.0 / PO_DBL_MAX;
  for (int i = 0; i < 6; ++i) { /* D: a vanished pivot gives 0 */
    const double d = A[7 * i];
    const double ad = d < 0 ? -d : d;
    y[i] = (ad > tol) ? y[i] / d : 0.0;
  }
  for (int i = 4; i >= 0; --i) /* L^T */
    for (int j = i + 1; j < 6; ++j) y[i] = y[i] - A[6 * j + i] * y[j];
  for (int i = 0; i < 6; ++i) x[perm[i]] = y[i];
  return 1;
}

#endif /* ORBX_POSEOPT_MATH_H */

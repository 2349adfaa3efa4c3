/* kfbuild_ref.c -- CPU restatement of the projection that feeds the keyframe
 * window search: the statements of ORBmatcher::Fuse (both
 * forms; src/ORBmatcher.cc:514-531, :582-599) and of SearchBySim3 (:676-694),
 * KeyFrame::IsInImage (src/KeyFrame.cc:590-593) and MapPoint::PredictScale
 * (the KeyFrame* overload, src/MapPoint.cc:353-362) with the host's own logf.
 * Built by tests/kfbuild_util.py with gcc -O2 -ffp-contract=off: fmaf stands
 * where the reference's object has a fused operation (u and v), sqrt is the
 * host's correctly rounded double root.  One row per point; a point the
 * reference `continue`s past is an inert row.  branch[i] names the statement
 * that decided the point.  fused == 0 gives the variant a compiler without
 * contraction would build from the source text (fx * x + cx in two roundings):
 * the tests use it only to show that the scenes can tell the two apart. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define KB_MAX_LEVELS 32
#define KB_FORM_FUSE 1
#define KB_FORM_SIM3 2

typedef struct {
  float Rcw[9], tcw[3], ow[3], sR21[9], t21[3];
  float fx, fy, cx, cy;
  float min_x, max_x, min_y, max_y;
  int nlevels;
  float sf[KB_MAX_LEVELS];
  float lsf;
} kb_camera;

typedef struct {
  const float* pos;
  const float* min_dist_inv;
  const float* max_dist_inv;
  const float* max_dist;
  const uint8_t* skip;
} kb_points;

typedef struct {
  float x, y, radius;
  int32_t level, desc;
} kb_query;

enum {
  KB_LIVE = 0, KB_SKIP, KB_DEPTH, KB_U_LOW, KB_U_HIGH, KB_V_LOW, KB_V_HIGH, KB_DIST_LOW, KB_DIST_HIGH,
  KB_NONFINITE
};

/* (int) of a float as vcvttss2si does it: INT_MIN for NaN and out of range */
static int cvtt(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT32_MIN; }

/* MapPoint::PredictScale(dist, pKF): vdivss, logf, vdivss, vroundss (ceil),
 * vcvttss2si, min(.., nlevels - 1), max(0, ..) */
int kb_predict_scale(float max_dist, float dist, float lsf, int nlevels) {
  const float ratio = max_dist / dist;
  const int s = cvtt(ceilf(logf(ratio) / lsf));
  const int m = s < nlevels - 1 ? s : nlevels - 1;
  return m > 0 ? m : 0;
}

/* one row of a cv::Mat product R * p + t: products summed left to right in
 * float, then + t */
static float row(const float* r, const float* p, float t) {
  float s = r[0] * p[0];
  s = s + r[1] * p[1];
  s = s + r[2] * p[2];
  return s + t;
}

/* cv::norm of a CV_32F 3-vector: the squares summed in double, sqrt, to float */
static float norm3(const float* a) {
  double s = (double)a[0] * (double)a[0];
  s = s + (double)a[1] * (double)a[1];
  s = s + (double)a[2] * (double)a[2];
  return (float)sqrt(s);
}

static int decide(int form, int fused, const kb_camera* C, const kb_points* P, int i, float th, kb_query* Q) {
  float c[3], invz, x, y, u, v, dist, radius;
  const float* p = P->pos + 3 * (size_t)i;
  int level;
  if (P->skip && P->skip[i]) return KB_SKIP;
  c[0] = row(C->Rcw + 0, p, C->tcw[0]);
  c[1] = row(C->Rcw + 3, p, C->tcw[1]);
  c[2] = row(C->Rcw + 6, p, C->tcw[2]);
  if (form == KB_FORM_SIM3) { /* p3Dc2 = sR21 * p3Dc1 + t21 */
    float c2[3];
    c2[0] = row(C->sR21 + 0, c, C->t21[0]);
    c2[1] = row(C->sR21 + 3, c, C->t21[1]);
    c2[2] = row(C->sR21 + 6, c, C->t21[2]);
    c[0] = c2[0];
    c[1] = c2[1];
    c[2] = c2[2];
  }
  if (c[2] < 0.0f) return KB_DEPTH;
  invz = 1.0f / c[2];
  x = c[0] * invz;
  y = c[1] * invz;
  if (fused) {
    u = fmaf(x, C->fx, C->cx);
    v = fmaf(y, C->fy, C->cy);
  } else {
    u = C->fx * x + C->cx;
    v = C->fy * y + C->cy;
  }
  /* IsInImage: x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY */
  if (!(u >= C->min_x)) return KB_U_LOW;
  if (!(u < C->max_x)) return KB_U_HIGH;
  if (!(v >= C->min_y)) return KB_V_LOW;
  if (!(v < C->max_y)) return KB_V_HIGH;
  if (form == KB_FORM_SIM3) {
    dist = norm3(c);
  } else {
    float o[3];
    o[0] = p[0] - C->ow[0];
    o[1] = p[1] - C->ow[1];
    o[2] = p[2] - C->ow[2];
    dist = norm3(o);
  }
  if (dist < P->min_dist_inv[i]) return KB_DIST_LOW;
  if (dist > P->max_dist_inv[i]) return KB_DIST_HIGH;
  level = kb_predict_scale(P->max_dist[i], dist, C->lsf, C->nlevels);
  radius = th * C->sf[level];
  if (!isfinite(radius)) return KB_NONFINITE;
  Q->x = u;
  Q->y = v;
  Q->radius = radius;
  Q->level = level;
  return KB_LIVE;
}

/* q, level, branch: npts entries; counts[0] = live rows, counts[1] = rows with
 * a non-finite radius */
void kb_project(int form, int fused, const kb_camera* C, const kb_points* P, int npts, int32_t desc_base,
                float th, kb_query* q, int32_t* level, int32_t* branch, int32_t* counts) {
  int i;
  counts[0] = counts[1] = 0;
  for (i = 0; i < npts; ++i) {
    kb_query Q = {0.0f, 0.0f, -1.0f, -1, 0};
    const kb_query inert = {0.0f, 0.0f, -1.0f, -1, 0};
    const int b = decide(form, fused, C, P, i, th, &Q);
    if (b != KB_LIVE) Q = inert;
    Q.desc = desc_base + i;
    q[i] = Q;
    level[i] = Q.level;
    branch[i] = b;
    counts[0] += b == KB_LIVE;
    counts[1] += b == KB_NONFINITE;
  }
}

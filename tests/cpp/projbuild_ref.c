/* projbuild_ref.c -- CPU restatement of the projection that feeds the
 * projection matchers: Frame::isInFrustum with the radius and
 * levels of SearchByProjection(Frame&, vector<MapPoint*>&, th) (mode 1), the
 * projection of the last-frame form (mode 2) and of the keyframe form (mode
 * 3), and MapPoint::PredictScale with the host's own logf.  Built by
 * tests/projbuild_util.py with gcc -O2 -ffp-contract=off: fmaf stands where
 * the reference's object has a fused operation, sqrt is the host's
 * (correctly rounded) double root.  One row per point; a skipped point is an
 * inert row.  branch[i] names the statement that decided the point. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define PB_MAX_LEVELS 32

typedef struct {
  float Rcw[9], tcw[3], ow[3];
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y;
  int nlevels;
  float sf[PB_MAX_LEVELS];
  float lsf;
} pb_camera;

typedef struct {
  const float* pos;
  const float* normal;
  const float* min_dist_inv;
  const float* max_dist_inv;
  const float* max_dist;
  const int32_t* octave;
  const float* angle;
  const uint8_t* skip;
} pb_points;

typedef struct {
  float x, y, radius;
  int32_t min_level, max_level;
  float xr, angle;
} pb_query;

enum {
  PB_LIVE = 0, PB_SKIP, PB_DEPTH, PB_U_LOW, PB_U_HIGH, PB_V_LOW, PB_V_HIGH, PB_DIST_LOW, PB_DIST_HIGH,
  PB_VIEW_COS, PB_NONFINITE
};

/* (int) of a float as vcvttss2si does it: INT_MIN for NaN and out of range */
static int cvtt(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT32_MIN; }

int pb_predict_scale(float max_dist, float dist, float lsf, int nlevels) {
  const float ratio = max_dist / dist;
  const int s = cvtt(ceilf(logf(ratio) / lsf));
  const int m = s < nlevels - 1 ? s : nlevels - 1;
  return m > 0 ? m : 0;
}

/* one row of Rcw * P + tcw: products summed left to right in float, then + t */
static float row(const float* r, const float* p, float t) {
  float s = r[0] * p[0];
  s = s + r[1] * p[1];
  s = s + r[2] * p[2];
  return s + t;
}

static double dot3(const float* a, const float* b) {
  double s = (double)a[0] * (double)b[0];
  s = s + (double)a[1] * (double)b[1];
  s = s + (double)a[2] * (double)b[2];
  return s;
}

static int decide(int mode, const pb_camera* C, const pb_points* P, int i, float th, float vcl, int rule,
                  pb_query* Q, int* level, float* vcos) {
  float Pc[3], PO[3], u, v;
  const float* p = P->pos + 3 * (size_t)i;
  if (P->skip && P->skip[i]) return PB_SKIP;
  Pc[0] = row(C->Rcw + 0, p, C->tcw[0]);
  Pc[1] = row(C->Rcw + 3, p, C->tcw[1]);
  Pc[2] = row(C->Rcw + 6, p, C->tcw[2]);
  if (mode == 1) {
    float invz, dist, vc, r;
    if (Pc[2] < 0.0f) return PB_DEPTH;
    invz = 1.0f / Pc[2];
    u = fmaf(C->fx * Pc[0], invz, C->cx);
    v = fmaf(C->fy * Pc[1], invz, C->cy);
    if (u < C->min_x) return PB_U_LOW;
    if (u > C->max_x) return PB_U_HIGH;
    if (v < C->min_y) return PB_V_LOW;
    if (v > C->max_y) return PB_V_HIGH;
    PO[0] = p[0] - C->ow[0];
    PO[1] = p[1] - C->ow[1];
    PO[2] = p[2] - C->ow[2];
    dist = (float)sqrt(dot3(PO, PO));
    if (dist < P->min_dist_inv[i]) return PB_DIST_LOW;
    if (dist > P->max_dist_inv[i]) return PB_DIST_HIGH;
    vc = (float)(dot3(PO, P->normal + 3 * (size_t)i) / (double)dist);
    if (vc < vcl) return PB_VIEW_COS;
    if (!(isfinite(u) && isfinite(v))) return PB_NONFINITE;
    *level = pb_predict_scale(P->max_dist[i], dist, C->lsf, C->nlevels);
    r = ((double)vc > 0.998 ? 2.5f : 4.0f) * ((double)th != 1.0 ? th : 1.0f);
    Q->radius = r * C->sf[*level];
    Q->min_level = *level - 1;
    Q->max_level = *level;
    Q->xr = fmaf(-invz, C->mbf, u);
    *vcos = vc;
  } else if (mode == 2) {
    int oct;
    if (Pc[2] <= 0.0f) return PB_DEPTH;
    u = C->fx * Pc[0] / Pc[2] + C->cx;
    v = C->fy * Pc[1] / Pc[2] + C->cy;
    if (u < C->min_x) return PB_U_LOW;
    if (u > C->max_x) return PB_U_HIGH;
    if (v < C->min_y) return PB_V_LOW;
    if (v > C->max_y) return PB_V_HIGH;
    oct = P->octave[i];
    if (oct < 0 || oct >= C->nlevels || !(isfinite(u) && isfinite(v))) return PB_NONFINITE;
    *level = oct;
    Q->radius = th * C->sf[oct];
    if (rule == 1) {
      Q->min_level = oct;
      Q->max_level = -1;
    } else if (rule == 2) {
      Q->min_level = 0;
      Q->max_level = oct;
    } else {
      Q->min_level = oct - 1;
      Q->max_level = oct + 1;
    }
    Q->angle = P->angle[i];
  } else {
    float invz, dist;
    invz = 1.0f / Pc[2];
    u = fmaf(C->fx * Pc[0], invz, C->cx);
    v = fmaf(C->fy * Pc[1], invz, C->cy);
    if (u < C->min_x) return PB_U_LOW;
    if (u > C->max_x) return PB_U_HIGH;
    if (v < C->min_y) return PB_V_LOW;
    if (v > C->max_y) return PB_V_HIGH;
    if (!(isfinite(u) && isfinite(v))) return PB_NONFINITE;
    PO[0] = p[0] - C->ow[0];
    PO[1] = p[1] - C->ow[1];
    PO[2] = p[2] - C->ow[2];
    dist = (float)sqrt(dot3(PO, PO));
    *level = pb_predict_scale(P->max_dist[i], dist, C->lsf, C->nlevels);
    Q->radius = th * C->sf[*level];
    Q->min_level = *level - 1;
    Q->max_level = *level + 1;
    Q->angle = P->angle[i];
  }
  Q->x = u;
  Q->y = v;
  return PB_LIVE;
}

/* q, level, branch: npts entries; vcos may be NULL; counts[0] = live rows,
 * counts[1] = non-finite points */
void pb_project(int mode, const pb_camera* C, const pb_points* P, int npts, float th, float vcl, int rule,
                pb_query* q, int32_t* level, float* vcos, int32_t* branch, int32_t* counts) {
  int i;
  counts[0] = counts[1] = 0;
  for (i = 0; i < npts; ++i) {
    pb_query Q = {0.0f, 0.0f, 0.0f, -1, -1, 0.0f, 0.0f};
    int lv = -1;
    float vc = 0.0f;
    const int b = decide(mode, C, P, i, th, vcl, rule, &Q, &lv, &vc);
    if (b != PB_LIVE) {
      const pb_query inert = {0.0f, 0.0f, -1.0f, -1, -1, 0.0f, 0.0f};
      Q = inert;
      lv = -1;
      vc = 0.0f;
    }
    q[i] = Q;
    level[i] = lv;
    if (vcos) vcos[i] = vc;
    branch[i] = b;
    counts[0] += b == PB_LIVE;
    counts[1] += b == PB_NONFINITE;
  }
}

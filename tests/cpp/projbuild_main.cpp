// Host-side ASan/UBSan run of the device-side projection's host code
// (csrc/projbuild_internal.h, csrc/api_projbuild.hip): the PredictScale
// threshold builder over ordinary and extreme scales, the plans' cache of its
// tables (hit, miss, the clear when full), and every argument check
// of orbm_predict_scale_thresholds / orbm_project_points / the plan methods
// that returns before a device is needed.  No GPU is touched (the test hides
// the devices: a well-formed call ends in ORBX_ERR_NO_DEVICE).  Built by
// `make sanitize`.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "orbx.h"
#include "projbuild_internal.h"
#include "expect.h"

static float prev_float(float v) { return nextafterf(v, -INFINITY); }

static void thresholds(float lsf, int nlevels) {
  // exactly nlevels - 1 floats are written
  std::vector<float> thr((size_t)(nlevels > 1 ? nlevels - 1 : 0));
  EXPECT(orbm_predict_scale_thresholds(lsf, nlevels, thr.data()) == ORBX_OK);
  for (int L = 0; L + 1 < nlevels; ++L) {
    EXPECT(thr[L] > 0);
    if (L) EXPECT(thr[L] >= thr[L - 1]);
    if (isfinite(thr[L])) {
      // above L, not L + 1: under a tiny log_scale_factor one float step crosses several levels
      EXPECT(orbx::predict_scale_level_host(thr[L], lsf, nlevels) > L);
      EXPECT(orbx::predict_scale_level_host(prev_float(thr[L]), lsf, nlevels) <= L);
    } else {
      EXPECT(orbx::predict_scale_level_host(FLT_MAX, lsf, nlevels) <= L);
    }
  }
}

// the row the plans' cache writes for (lsf, nlevels): the thresholds of
// orbm_predict_scale_thresholds in front, zeros behind
static void cached_row(orbx::PredictScaleCache& cache, float lsf, int nlevels) {
  float want[ORBX_PROJ_MAX_LEVELS] = {};
  EXPECT(orbm_predict_scale_thresholds(lsf, nlevels, want) == ORBX_OK);
  float row[ORBX_PROJ_MAX_LEVELS];
  memset(row, 0xff, sizeof row);
  cache.fill(lsf, nlevels, row);
  EXPECT(memcmp(row, want, sizeof row) == 0);
  for (int L = nlevels > 1 ? nlevels - 1 : 0; L < ORBX_PROJ_MAX_LEVELS; ++L) EXPECT(row[L] == 0.0f);
}

static void threshold_cache() {
  orbx::PredictScaleCache cache;
  const float lsf = logf(1.2f);
  const float keys[][2] = {{lsf, 8}, {lsf, 1}, {logf(2.0f), 32}, {nextafterf(lsf, 1.0f), 8}};
  for (int pass = 0; pass < 2; ++pass) {  // the miss, then the hit
    for (const auto& k : keys) cached_row(cache, k[0], (int)k[1]);
    EXPECT(cache.n == 4);  // the neighbouring bit pattern of lsf is an entry of its own
  }
  // seventeen distinct keys in a row: the full cache is cleared, then serves again
  orbx::PredictScaleCache full;
  for (int i = 0; i < 17; ++i) {
    cached_row(full, logf(1.1f + 0.01f * (float)i), 8);
    EXPECT(full.n == (i < 16 ? i + 1 : 1));
  }
  cached_row(full, logf(1.1f), 8);  // the first key, gone with the clear
  EXPECT(full.n == 2);
  cached_row(full, logf(1.1f), 8);
  EXPECT(full.n == 2);
}

int main() {
  threshold_cache();
  thresholds(logf(1.2f), 8);
  thresholds(logf(2.0f), 4);
  thresholds(logf(1.05f), 12);
  thresholds(logf(1.2f), 1);
  thresholds(logf(1.2f), ORBX_PROJ_MAX_LEVELS);
  thresholds(4.2e-8f, ORBX_PROJ_MAX_LEVELS);  // the smallest accepted order of magnitude
  thresholds(80.0f, 8);                       // levels past 1 need ratios beyond FLT_MAX: +inf entries
  thresholds(FLT_MAX, 3);
  float one[ORBX_PROJ_MAX_LEVELS];
  const float bad_lsf[] = {0.0f, -1.0f, NAN, INFINITY, -INFINITY, 1e-8f, FLT_MIN};
  for (float lsf : bad_lsf) EXPECT(orbm_predict_scale_thresholds(lsf, 8, one) == ORBX_ERR_ARG);
  const int bad_levels[] = {0, -1, ORBX_PROJ_MAX_LEVELS + 1, 1 << 30};
  for (int nl : bad_levels) EXPECT(orbm_predict_scale_thresholds(logf(1.2f), nl, one) == ORBX_ERR_ARG);
  EXPECT(orbm_predict_scale_thresholds(logf(1.2f), 2, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_predict_scale_thresholds(logf(1.2f), 1, nullptr) == ORBX_OK);

  // orbm_project_points
  orbx_proj_camera cam;
  memset(&cam, 0, sizeof cam);
  cam.nlevels = 8;
  cam.log_scale_factor = logf(1.2f);
  for (int l = 0; l < 8; ++l) cam.scale_factors[l] = powf(1.2f, (float)l);
  const int n = 5;
  std::vector<float> f3((size_t)n * 3, 1.0f), f1((size_t)n, 1.0f);
  std::vector<int32_t> oct((size_t)n, 0);
  orbx_proj_points pts = {f3.data(), f3.data(), f1.data(), f1.data(), f1.data(), oct.data(), f1.data(), nullptr};
  orbx_proj_params prm = {1.0f, 0.5f, ORBX_LEVEL_RULE_NEITHER};
  std::vector<orbx_query_proj> q((size_t)n);
  std::vector<int32_t> level((size_t)n);
  int npts = n, niv = -7;
  EXPECT(orbm_project_points(1, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
  int zero = 0;
  EXPECT(orbm_project_points(1, 1, &cam, &pts, &zero, &prm, 0, nullptr, nullptr, nullptr, &niv) == ORBX_OK);
  EXPECT(niv == 0);
  for (int mode : {0, 4, -3})
    EXPECT(orbm_project_points(mode, 1, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, -1, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 70000, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  int neg = -1;
  EXPECT(orbm_project_points(1, 1, &cam, &pts, &neg, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 1, nullptr, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 1, &cam, nullptr, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 1, &cam, &pts, nullptr, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 1, &cam, &pts, &npts, nullptr, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 1, &cam, &pts, &npts, &prm, 0, nullptr, level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 1, &cam, &pts, &npts, &prm, 0, q.data(), nullptr, nullptr, &niv) == ORBX_ERR_ARG);
  EXPECT(orbm_project_points(1, 1, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, nullptr) == ORBX_ERR_ARG);
  for (int mode = 1; mode <= 3; ++mode) {
    const float** fields[] = {&pts.pos, &pts.normal, &pts.min_dist_inv, &pts.max_dist_inv, &pts.max_dist, &pts.angle};
    const bool reads[3][6] = {{1, 1, 1, 1, 1, 0}, {1, 0, 0, 0, 0, 1}, {1, 0, 0, 0, 1, 1}};
    for (int k = 0; k < 6; ++k) {
      const float* keep = *fields[k];
      *fields[k] = nullptr;
      const int rc = orbm_project_points(mode, 1, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv);
      EXPECT(reads[mode - 1][k] ? rc == ORBX_ERR_ARG : rc == ORBX_ERR_NO_DEVICE);
      *fields[k] = keep;
    }
  }
  pts.octave = nullptr;
  EXPECT(orbm_project_points(2, 1, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  pts.octave = oct.data();
  prm.level_rule = 3;
  EXPECT(orbm_project_points(2, 1, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  prm.level_rule = ORBX_LEVEL_RULE_BACKWARD;
  for (float lsf : bad_lsf) {
    orbx_proj_camera c = cam;
    c.log_scale_factor = lsf;
    EXPECT(orbm_project_points(1, 1, &c, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  }
  for (int nl : bad_levels) {
    orbx_proj_camera c = cam;
    c.nlevels = nl;
    EXPECT(orbm_project_points(1, 1, &c, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_ARG);
  }
  // well formed: refused only for want of a device, nothing written
  niv = -7;
  EXPECT(orbm_project_points(2, 1, &cam, &pts, &npts, &prm, 0, q.data(), level.data(), nullptr, &niv) == ORBX_ERR_NO_DEVICE);
  EXPECT(niv == -7);

  // the plan methods without a plan
  orbx_proj_build_problem pb;
  memset(&pb, 0, sizeof pb);
  EXPECT(orbm_proj_plan_project(nullptr, 1, 1, &pb, &prm, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_proj_plan_track(nullptr, 1, 1, &pb, &prm, 0.6f, 100, 1, nullptr) == ORBX_ERR_ARG);

  printf("projbuild_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

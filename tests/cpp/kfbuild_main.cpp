// Host-side ASan/UBSan run of the keyframe projection's host code
// (csrc/api_kfbuild.hip): every argument check of orbm_keyframe_project and of
// the orbm_kf_plan_* entry points that returns before a device is needed.  No
// GPU is touched (the test hides the devices: a well-formed call ends in
// ORBX_ERR_NO_DEVICE).  Built by `make sanitize`.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "orbx.h"
#include "expect.h"

int main() {
  orbx_kf_camera cam;
  memset(&cam, 0, sizeof cam);
  cam.nlevels = 8;
  cam.log_scale_factor = logf(1.2f);
  for (int l = 0; l < 8; ++l) cam.scale_factors[l] = powf(1.2f, (float)l);
  const int n = 5;
  std::vector<float> f3((size_t)n * 3, 1.0f), f1((size_t)n, 1.0f);
  std::vector<uint8_t> skip((size_t)n, 0);
  orbx_kf_points pts = {f3.data(), f1.data(), f1.data(), f1.data(), skip.data()};
  std::vector<orbx_kf_query> q((size_t)n);
  std::vector<int32_t> level((size_t)n);
  int npts = n, nlive = -7, zero = 0, neg = -1;
  const int F = ORBX_KF_FORM_FUSE, S = ORBX_KF_FORM_SIM3;

  EXPECT(orbm_keyframe_project(F, 0, nullptr, nullptr, nullptr, nullptr, 3.0f, 0, nullptr, nullptr, nullptr) == ORBX_OK);
  EXPECT(orbm_keyframe_project(S, 1, &cam, &pts, &zero, nullptr, 3.0f, 0, nullptr, nullptr, &nlive) == ORBX_OK);
  EXPECT(nlive == 0);
  nlive = -7;
  for (int form : {0, 3, -3})
    EXPECT(orbm_keyframe_project(form, 1, &cam, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, -1, &cam, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 70000, &cam, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, &neg, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 1, nullptr, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 1, &cam, nullptr, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, nullptr, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, &npts, nullptr, 3.0f, 0, nullptr, level.data(), &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, &npts, nullptr, 3.0f, 0, q.data(), nullptr, &nlive) == ORBX_ERR_ARG);
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), nullptr) == ORBX_ERR_ARG);
  int32_t base = -1;
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, &npts, &base, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  base = INT32_MAX - 2;
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, &npts, &base, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  for (int form : {F, S}) {
    const float** fields[] = {&pts.pos, &pts.min_dist_inv, &pts.max_dist_inv, &pts.max_dist};
    for (const float** f : fields) {
      const float* keep = *f;
      *f = nullptr;
      EXPECT(orbm_keyframe_project(form, 1, &cam, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
      *f = keep;
    }
  }
  const float bad_lsf[] = {0.0f, -1.0f, NAN, INFINITY, -INFINITY, 1e-8f};
  for (float lsf : bad_lsf) {
    orbx_kf_camera c = cam;
    c.log_scale_factor = lsf;
    EXPECT(orbm_keyframe_project(F, 1, &c, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  }
  const int bad_levels[] = {0, -1, ORBX_PROJ_MAX_LEVELS + 1, 1 << 30};
  for (int nl : bad_levels) {
    orbx_kf_camera c = cam;
    c.nlevels = nl;
    EXPECT(orbm_keyframe_project(S, 1, &c, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  }
  // a second problem's errors are found too
  {
    orbx_kf_camera cams[2] = {cam, cam};
    orbx_kf_points pp[2] = {pts, pts};
    int nn[2] = {n, n};
    pp[1].max_dist = nullptr;
    EXPECT(orbm_keyframe_project(F, 2, cams, pp, nn, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_ARG);
  }
  // well formed (skip may be NULL): refused only for want of a device, nothing written
  EXPECT(nlive == -7);
  EXPECT(orbm_keyframe_project(F, 1, &cam, &pts, &npts, nullptr, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_NO_DEVICE);
  pts.skip = nullptr;
  base = 11;
  EXPECT(orbm_keyframe_project(S, 1, &cam, &pts, &npts, &base, 3.0f, 0, q.data(), level.data(), &nlive) == ORBX_ERR_NO_DEVICE);
  EXPECT(nlive == -7);

  // the plan: create's checks, then the methods without a plan
  orbm_kf_plan* plan = reinterpret_cast<orbm_kf_plan*>(&cam);
  EXPECT(orbm_kf_plan_create(1, 100, 10, 0, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_kf_plan_create(0, 100, 10, 0, &plan) == ORBX_ERR_ARG);
  plan = reinterpret_cast<orbm_kf_plan*>(&cam);
  EXPECT(orbm_kf_plan_create(1, 0, 10, 0, &plan) == ORBX_ERR_ARG && plan == nullptr);
  EXPECT(orbm_kf_plan_create(1, 100, -1, 0, &plan) == ORBX_ERR_ARG && plan == nullptr);
  EXPECT(orbm_kf_plan_create(1, 8193, 10, 0, &plan) == ORBX_ERR_UNSUPPORTED && plan == nullptr);
  EXPECT(orbm_kf_plan_create(65536, 100, 10, 0, &plan) == ORBX_ERR_UNSUPPORTED && plan == nullptr);
  EXPECT(orbm_kf_plan_create(1, 100, 10, 0, &plan) == ORBX_ERR_NO_DEVICE && plan == nullptr);
  EXPECT(orbm_kf_plan_destroy(nullptr) == ORBX_OK);
  orbx_kf_problem pb;
  memset(&pb, 0, sizeof pb);
  EXPECT(orbm_kf_plan_search(nullptr, 1, &pb, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_kf_plan_project(nullptr, F, 1, &pb, 3.0f, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_kf_plan_project_search(nullptr, S, 1, &pb, 3.0f, nullptr) == ORBX_ERR_ARG);
  int counts[4] = {-1, -1, -1, -1};
  EXPECT(orbx_debug_live_resources(counts) == ORBX_OK);
  EXPECT(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0);

  printf("kfbuild_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

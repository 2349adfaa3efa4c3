// Host-side ASan/UBSan run of the pose optimisation's host code
// (csrc/api_poseopt.hip): every argument check of orbm_pose_optimization and of
// the orbm_pose_plan_* entry points that returns before a device is needed.  No
// GPU is touched (the test hides the devices: a well-formed call ends in
// ORBX_ERR_NO_DEVICE).  Built by `make sanitize`.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "orbx.h"
#include "expect.h"

int main() {
  orbx_pose_camera cam;
  memset(&cam, 0, sizeof cam);
  cam.Tcw[0] = cam.Tcw[5] = cam.Tcw[10] = 1.0f;
  cam.fx = cam.fy = 500.0f;
  cam.cx = 320.0f;
  cam.cy = 240.0f;
  cam.mbf = 40.0f;
  cam.nlevels = 8;
  for (int l = 0; l < 8; ++l) cam.inv_level_sigma2[l] = 1.0f;
  const int n = 6;
  std::vector<orbx_keypoint> keys((size_t)n);
  memset(keys.data(), 0, sizeof(orbx_keypoint) * n);
  for (int i = 0; i < n; ++i) keys[i].octave = i;
  std::vector<float> ur((size_t)n, -1.0f), pos((size_t)n * 3, 1.0f);
  std::vector<int32_t> idx = {0, 1, -1, 3, 4, 5};
  std::vector<uint8_t> has((size_t)n, 1);
  orbx_pose_obs obs = {n, keys.data(), ur.data(), pos.data(), nullptr, nullptr, n};
  float T[16];
  uint8_t outlier[n];
  int nin = -7;
  for (float& v : T) v = 7.0f;
  memset(outlier, 9, sizeof outlier);
  auto untouched = [&] {
    for (float v : T)
      if (v != 7.0f) return false;
    for (uint8_t v : outlier)
      if (v != 9) return false;
    return nin == -7;
  };
  auto call = [&](int nprob, const orbx_pose_camera* c, const orbx_pose_obs* o) {
    return orbm_pose_optimization(nprob, c, o, 0, T, outlier, &nin);
  };

  EXPECT(orbm_pose_optimization(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == ORBX_OK);
  EXPECT(call(-1, &cam, &obs) == ORBX_ERR_ARG);
  EXPECT(call(70000, &cam, &obs) == ORBX_ERR_ARG);
  EXPECT(call(1, nullptr, &obs) == ORBX_ERR_ARG);
  EXPECT(call(1, &cam, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_pose_optimization(1, &cam, &obs, 0, nullptr, outlier, &nin) == ORBX_ERR_ARG);
  EXPECT(orbm_pose_optimization(1, &cam, &obs, 0, T, nullptr, &nin) == ORBX_ERR_ARG);
  EXPECT(orbm_pose_optimization(1, &cam, &obs, 0, T, outlier, nullptr) == ORBX_ERR_ARG);
  for (int bad_n : {-1, ORBX_POSE_MAX_N + 1}) {
    orbx_pose_obs o = obs;
    o.n = bad_n;
    EXPECT(call(1, &cam, &o) == ORBX_ERR_ARG);
  }
  for (int bad_npos : {-1, n - 1}) {  // without point_index, pos holds a row per feature
    orbx_pose_obs o = obs;
    o.npos = bad_npos;
    EXPECT(call(1, &cam, &o) == ORBX_ERR_ARG);
  }
  for (int nl : {0, -1, ORBX_PROJ_MAX_LEVELS + 1, 1 << 30, 5 /* octave 5 is outside [0, 5) */}) {
    orbx_pose_camera c = cam;
    c.nlevels = nl;
    EXPECT(call(1, &c, &obs) == ORBX_ERR_ARG);
  }
  {
    orbx_pose_obs o = obs;
    o.keys = nullptr;
    EXPECT(call(1, &cam, &o) == ORBX_ERR_ARG);
    o = obs;
    o.pos = nullptr;
    EXPECT(call(1, &cam, &o) == ORBX_ERR_ARG);
  }
  {  // octaves: read only where the feature has a point
    std::vector<orbx_keypoint> k2 = keys;
    k2[2].octave = 8;
    orbx_pose_obs o = obs;
    o.keys = k2.data();
    EXPECT(call(1, &cam, &o) == ORBX_ERR_ARG);
    k2[2].octave = -1;
    EXPECT(call(1, &cam, &o) == ORBX_ERR_ARG);
    o.point_index = idx.data();  // feature 2 has no point: its octave is not read
    EXPECT(call(1, &cam, &o) == ORBX_ERR_NO_DEVICE);
    o.point_index = nullptr;
    std::vector<uint8_t> h2 = has;
    h2[2] = 0;
    o.has_point = h2.data();
    EXPECT(call(1, &cam, &o) == ORBX_ERR_NO_DEVICE);
  }
  for (int32_t bad : {-2, n, INT32_MAX, INT32_MIN}) {
    std::vector<int32_t> i2 = idx;
    i2[4] = bad;
    orbx_pose_obs o = obs;
    o.point_index = i2.data();
    EXPECT(call(1, &cam, &o) == ORBX_ERR_ARG);
  }
  {  // a pool smaller than the frame is fine with point_index
    std::vector<int32_t> i2 = {0, 1, -1, 1, 0, 1};
    orbx_pose_obs o = obs;
    o.point_index = i2.data();
    o.npos = 2;
    EXPECT(call(1, &cam, &o) == ORBX_ERR_NO_DEVICE);
  }
  {  // a second problem's errors are found too
    orbx_pose_camera cams[2] = {cam, cam};
    orbx_pose_obs oo[2] = {obs, obs};
    oo[1].n = -1;
    EXPECT(orbm_pose_optimization(2, cams, oo, 0, T, outlier, &nin) == ORBX_ERR_ARG);
  }
  EXPECT(untouched());
  // well formed (uright may be NULL; an empty frame needs no arrays)
  EXPECT(call(1, &cam, &obs) == ORBX_ERR_NO_DEVICE);
  {
    orbx_pose_obs o = obs;
    o.uright = nullptr;
    EXPECT(call(1, &cam, &o) == ORBX_ERR_NO_DEVICE);
    orbx_pose_obs e;
    memset(&e, 0, sizeof e);
    EXPECT(orbm_pose_optimization(1, &cam, &e, 0, T, nullptr, &nin) == ORBX_ERR_NO_DEVICE);
  }
  EXPECT(untouched());

  // the plan: create's checks, then optimize without a plan
  orbm_pose_plan* plan = reinterpret_cast<orbm_pose_plan*>(&cam);
  EXPECT(orbm_pose_plan_create(1, 100, 0, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_pose_plan_create(0, 100, 0, &plan) == ORBX_ERR_ARG && plan == nullptr);
  plan = reinterpret_cast<orbm_pose_plan*>(&cam);
  EXPECT(orbm_pose_plan_create(1, 0, 0, &plan) == ORBX_ERR_ARG && plan == nullptr);
  EXPECT(orbm_pose_plan_create(1, ORBX_POSE_MAX_N + 1, 0, &plan) == ORBX_ERR_UNSUPPORTED && plan == nullptr);
  EXPECT(orbm_pose_plan_create(65536, 100, 0, &plan) == ORBX_ERR_UNSUPPORTED && plan == nullptr);
  EXPECT(orbm_pose_plan_create(1, 100, 0, &plan) == ORBX_ERR_NO_DEVICE && plan == nullptr);
  EXPECT(orbm_pose_plan_destroy(nullptr) == ORBX_OK);
  orbx_pose_problem pb;
  memset(&pb, 0, sizeof pb);
  EXPECT(orbm_pose_plan_optimize(nullptr, 1, &pb, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_pose_plan_optimize(nullptr, 0, nullptr, nullptr) == ORBX_ERR_ARG);
  int counts[4] = {-1, -1, -1, -1};
  EXPECT(orbx_debug_live_resources(counts) == ORBX_OK);
  EXPECT(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0);

  printf("poseopt_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

// Host-side ASan/UBSan run of the Sim3 solver's host code (csrc/api_sim3.hip):
// every argument check of orbm_sim3_solve, all of which return before a device
// is needed.  No GPU is touched (the test hides the devices: a well-formed call
// ends in ORBX_ERR_NO_DEVICE).  Built by `make sanitize`.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "orbx.h"
#include "expect.h"

int main() {
  const int n = 10, nit = 4;
  std::vector<float> pos1((size_t)n * 3), pos2((size_t)n * 3), s1((size_t)n, 1.0f), s2((size_t)n, 1.44f);
  for (int i = 0; i < n; ++i) {
    pos1[3 * i] = 0.3f * i - 1.0f, pos1[3 * i + 1] = 0.1f * (i % 4), pos1[3 * i + 2] = 4.0f + 0.5f * i;
    pos2[3 * i] = pos1[3 * i] + 0.2f, pos2[3 * i + 1] = pos1[3 * i + 1] - 0.1f, pos2[3 * i + 2] = pos1[3 * i + 2] + 0.05f;
  }
  std::vector<int32_t> tri = {0, 1, 2, 3, 4, 5, 9, 8, 7, 2, 2, 6};  // the last one repeats an index: allowed
  orbx_sim3_problem P;
  memset(&P, 0, sizeof P);
  P.ncorr = n;
  P.pos1 = pos1.data(), P.pos2 = pos2.data(), P.sigma2_1 = s1.data(), P.sigma2_2 = s2.data();
  P.Rcw1[0] = P.Rcw1[4] = P.Rcw1[8] = 1.0f;
  P.Rcw2[0] = P.Rcw2[4] = P.Rcw2[8] = 1.0f;
  P.fx1 = P.fy1 = P.fx2 = P.fy2 = 500.0f;
  P.cx1 = P.cx2 = 320.0f, P.cy1 = P.cy2 = 240.0f;
  P.nit = nit;
  P.triples = tri.data();
  P.min_inliers = 5;
  orbx_sim3_result res[2];
  uint8_t inl[2 * n];
  int32_t off[3] = {0, n, 2 * n};
  memset(res, 0x5A, sizeof res);
  memset(inl, 9, sizeof inl);
  auto untouched = [&] {
    const unsigned char* r = reinterpret_cast<const unsigned char*>(res);
    for (size_t i = 0; i < sizeof res; ++i)
      if (r[i] != 0x5A) return false;
    for (int i = 0; i < 2 * n; ++i)
      if (inl[i] != 9) return false;
    return true;
  };
  auto call = [&](int nprob, const orbx_sim3_problem* p) { return orbm_sim3_solve(nprob, p, 0, res, inl, off); };
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

  EXPECT(orbm_sim3_solve(0, nullptr, 0, nullptr, nullptr, nullptr) == ORBX_OK);
  EXPECT(call(-1, &P) == ORBX_ERR_ARG);
  EXPECT(call(1, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_sim3_solve(1, &P, 0, nullptr, inl, off) == ORBX_ERR_ARG);
  EXPECT(orbm_sim3_solve(1, &P, 0, res, nullptr, off) == ORBX_ERR_ARG);
  EXPECT(orbm_sim3_solve(1, &P, 0, res, inl, nullptr) == ORBX_ERR_ARG);
  EXPECT(call(65536, &P) == ORBX_ERR_UNSUPPORTED);  // refused before the table is read
  {  // the counts and the problem's pointers
    orbx_sim3_problem q = P;
    q.ncorr = -1;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.nit = -1;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.min_inliers = -1;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.best_in = -1;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.pos1 = nullptr;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.pos2 = nullptr;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.sigma2_1 = nullptr;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.sigma2_2 = nullptr;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.triples = nullptr;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q.nit = 0;  // nit == 0: triples is not read
    EXPECT(call(1, &q) == ORBX_ERR_NO_DEVICE);
    // the limits are refused before anything of that length is read
    q = P, q.ncorr = 8193;
    EXPECT(call(1, &q) == ORBX_ERR_UNSUPPORTED);
    q = P, q.nit = 4097;
    EXPECT(call(1, &q) == ORBX_ERR_UNSUPPORTED);
    // fewer than three correspondences in a problem that is not inert
    q = P, q.ncorr = 2, q.min_inliers = 2;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q.min_inliers = 3;  // inert: nothing of it is read
    q.pos1 = q.pos2 = q.sigma2_1 = q.sigma2_2 = nullptr, q.triples = nullptr;
    EXPECT(call(1, &q) == ORBX_ERR_NO_DEVICE);
    q = P, q.min_inliers = n + 1;  // inert with every array absent
    q.pos1 = q.pos2 = q.sigma2_1 = q.sigma2_2 = nullptr, q.triples = nullptr;
    EXPECT(call(1, &q) == ORBX_ERR_NO_DEVICE);
    q = P, q.ncorr = 3, q.min_inliers = 3;  // three is enough
    std::vector<int32_t> t3 = {0, 1, 2, 2, 1, 0, 0, 0, 0, 1, 1, 2};
    q.triples = t3.data();
    EXPECT(call(1, &q) == ORBX_ERR_NO_DEVICE);
  }
  for (float bad : {nan, inf, -inf}) {  // positions, poses, cameras
    for (int which = 0; which < 2; ++which) {
      std::vector<float> a = pos1, b = pos2;
      (which ? b : a)[which ? 3 * n - 1 : 4] = bad;
      orbx_sim3_problem q = P;
      q.pos1 = a.data(), q.pos2 = b.data();
      EXPECT(call(1, &q) == ORBX_ERR_ARG);
    }
    orbx_sim3_problem q = P;
    q.Rcw1[8] = bad;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.tcw1[0] = bad;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.Rcw2[0] = bad;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    q = P, q.tcw2[2] = bad;
    EXPECT(call(1, &q) == ORBX_ERR_ARG);
    float* cams[8] = {&q.fx1, &q.fy1, &q.cx1, &q.cy1, &q.fx2, &q.fy2, &q.cx2, &q.cy2};
    for (int e = 0; e < 8; ++e) {
      q = P, *cams[e] = bad;
      EXPECT(call(1, &q) == ORBX_ERR_ARG);
    }
  }
  for (float bad : {nan, inf, -inf, -1e-30f, 2.4e8f, 3e38f}) {  // sigma2: finite, >= 0, 9.210 * sigma2 < 2^31
    for (int which = 0; which < 2; ++which) {
      std::vector<float> a = s1, b = s2;
      (which ? b : a)[which ? n - 1 : 0] = bad;
      orbx_sim3_problem q = P;
      q.sigma2_1 = a.data(), q.sigma2_2 = b.data();
      EXPECT(call(1, &q) == ORBX_ERR_ARG);
    }
  }
  for (float good : {0.0f, 0.1f, 2.3e8f}) {
    std::vector<float> a = s1;
    a[3] = good;
    orbx_sim3_problem q = P;
    q.sigma2_1 = a.data();
    EXPECT(call(1, &q) == ORBX_ERR_NO_DEVICE);
  }
  for (int32_t bad : {-1, n, INT32_MAX, INT32_MIN}) {  // a triple index outside [0, ncorr)
    for (int at : {0, nit * 3 - 1}) {
      std::vector<int32_t> t = tri;
      t[at] = bad;
      orbx_sim3_problem q = P;
      q.triples = t.data();
      EXPECT(call(1, &q) == ORBX_ERR_ARG);
    }
  }
  {  // the flag segments
    int32_t narrow[2] = {0, n - 1}, neg[2] = {-1, n}, wide[2] = {3, 3 + n};
    EXPECT(orbm_sim3_solve(1, &P, 0, res, inl, narrow) == ORBX_ERR_ARG);
    EXPECT(orbm_sim3_solve(1, &P, 0, res, inl, neg) == ORBX_ERR_ARG);
    EXPECT(orbm_sim3_solve(1, &P, 0, res, inl, wide) == ORBX_ERR_NO_DEVICE);
    int32_t second[3] = {0, n, 2 * n - 1};
    orbx_sim3_problem two[2] = {P, P};
    EXPECT(orbm_sim3_solve(2, two, 0, res, inl, second) == ORBX_ERR_ARG);
    two[1].min_inliers = n + 1;  // an inert problem still needs room for its cleared flags
    EXPECT(orbm_sim3_solve(2, two, 0, res, inl, second) == ORBX_ERR_ARG);
  }
  {  // a second problem's errors are found too
    orbx_sim3_problem two[2] = {P, P};
    two[1].ncorr = 9;  // triple index 9 is now out of range
    EXPECT(call(2, two) == ORBX_ERR_ARG);
    two[1] = P;
    EXPECT(call(2, two) == ORBX_ERR_NO_DEVICE);
  }
  EXPECT(untouched());
  // well formed
  EXPECT(call(1, &P) == ORBX_ERR_NO_DEVICE);
  {
    orbx_sim3_problem q = P;
    q.fix_scale = 1, q.best_in = 7;
    EXPECT(call(1, &q) == ORBX_ERR_NO_DEVICE);
  }
  EXPECT(untouched());
  int counts[4] = {-1, -1, -1, -1};
  EXPECT(orbx_debug_live_resources(counts) == ORBX_OK);
  EXPECT(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0);

  printf("sim3_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

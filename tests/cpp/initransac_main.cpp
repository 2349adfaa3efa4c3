// Host-side ASan/UBSan run of the initializer RANSAC's host code
// (csrc/api_initransac.hip): every argument check of orbm_initializer_ransac,
// all of which return before a device is needed.  No GPU is touched (the test
// hides the devices: a well-formed call ends in ORBX_ERR_NO_DEVICE).  Built by
// `make sanitize`.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "orbx.h"
#include "expect.h"

int main() {
  const int n1 = 14, n2 = 12, nit = 3;
  std::vector<orbx_keypoint> k1((size_t)n1), k2((size_t)n2);
  memset(k1.data(), 0, sizeof(orbx_keypoint) * n1);
  memset(k2.data(), 0, sizeof(orbx_keypoint) * n2);
  for (int i = 0; i < n1; ++i) k1[i].x = 10.0f * i, k1[i].y = 7.0f * (i % 5);
  for (int i = 0; i < n2; ++i) k2[i].x = 10.0f * i + 3.0f, k2[i].y = 7.0f * (i % 5) + 1.0f;
  // ten matches, rows 3, 7, 11 and 13 unmatched
  std::vector<int32_t> m12 = {0, 1, 2, -1, 4, 5, 6, -1, 8, 9, 10, -1, 11, -1};
  const int nmatch = 10;
  std::vector<int32_t> sets = {0, 1, 2, 3, 4, 5, 6, 7, 9, 8, 7, 6, 5, 4, 3, 2, 0, 2, 4, 6, 8, 9, 1, 3};
  orbx_ransac_pair pair = {n1, n2, k1.data(), k2.data(), m12.data(), sets.data()};
  orbx_ransac_result res[2];
  uint8_t inlH[2 * nmatch], inlF[2 * nmatch];
  int32_t off[3] = {0, nmatch, 2 * nmatch};
  memset(res, 0x5A, sizeof res);
  memset(inlH, 9, sizeof inlH);
  memset(inlF, 9, sizeof inlF);
  auto untouched = [&] {
    const unsigned char* r = reinterpret_cast<const unsigned char*>(res);
    for (size_t i = 0; i < sizeof res; ++i)
      if (r[i] != 0x5A) return false;
    for (int i = 0; i < 2 * nmatch; ++i)
      if (inlH[i] != 9 || inlF[i] != 9) return false;
    return true;
  };
  auto call = [&](int npair, const orbx_ransac_pair* p, int it, float sigma = 1.0f) {
    return orbm_initializer_ransac(npair, p, it, sigma, 0, res, inlH, inlF, off);
  };
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

  EXPECT(orbm_initializer_ransac(0, nullptr, 200, 1.0f, 0, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
  EXPECT(call(-1, &pair, nit) == ORBX_ERR_ARG);
  EXPECT(call(1, &pair, -1) == ORBX_ERR_ARG);
  EXPECT(call(1, nullptr, nit) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_ransac(1, &pair, nit, 1.0f, 0, nullptr, inlH, inlF, off) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_ransac(1, &pair, nit, 1.0f, 0, res, nullptr, inlF, off) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_ransac(1, &pair, nit, 1.0f, 0, res, inlH, nullptr, off) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_ransac(1, &pair, nit, 1.0f, 0, res, inlH, inlF, nullptr) == ORBX_ERR_ARG);
  EXPECT(call(1, &pair, nit, nan) == ORBX_ERR_ARG);
  EXPECT(call(1, &pair, nit, inf) == ORBX_ERR_ARG);
  EXPECT(call(1, &pair, nit, -inf) == ORBX_ERR_ARG);
  {  // the pair's pointers and counts
    orbx_ransac_pair p = pair;
    p.keys1 = nullptr;
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    p = pair, p.keys2 = nullptr;
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    p = pair, p.match12 = nullptr;
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    p = pair, p.sets = nullptr;
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    EXPECT(call(1, &p, 0) == ORBX_ERR_NO_DEVICE);  // nit == 0: sets is not read
    p = pair, p.n1 = -1;
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    p = pair, p.n2 = -1;
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    // the limits are refused before anything of that length is read
    p = pair, p.n1 = 8193;
    EXPECT(call(1, &p, nit) == ORBX_ERR_UNSUPPORTED);
    p = pair, p.n2 = 8193;
    EXPECT(call(1, &p, nit) == ORBX_ERR_UNSUPPORTED);
    EXPECT(call(1, &pair, 4097) == ORBX_ERR_UNSUPPORTED);
    EXPECT(call(65536, &pair, nit) == ORBX_ERR_UNSUPPORTED);
  }
  for (float bad : {nan, inf, -inf}) {  // every key of both frames, matched or not
    for (int which = 0; which < 4; ++which) {
      std::vector<orbx_keypoint> a = k1, b = k2;
      if (which == 0) a[3].x = bad;        // an unmatched key of frame 1
      if (which == 1) a[n1 - 2].y = bad;
      if (which == 2) b[7].x = bad;        // frame 2's key 7 is matched by no row
      if (which == 3) b[0].y = bad;
      orbx_ransac_pair p = pair;
      p.keys1 = a.data(), p.keys2 = b.data();
      EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    }
  }
  for (int32_t bad : {n2, n2 + 1, INT32_MAX}) {  // match12 >= n2 (anything negative is "no match")
    std::vector<int32_t> m = m12;
    m[5] = bad;
    orbx_ransac_pair p = pair;
    p.match12 = m.data();
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
  }
  {
    std::vector<int32_t> m = m12;
    m[5] = INT32_MIN;  // one match fewer, still nine: set index 9 is now out of range
    orbx_ransac_pair p = pair;
    p.match12 = m.data();
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    std::vector<int32_t> s = sets;
    for (int32_t& v : s) v = v == 9 ? 0 : v;
    p.sets = s.data();
    int32_t o9[2] = {0, 9};
    EXPECT(orbm_initializer_ransac(1, &p, nit, 1.0f, 0, res, inlH, inlF, o9) == ORBX_ERR_NO_DEVICE);
  }
  for (int32_t bad : {-1, nmatch, INT32_MAX, INT32_MIN}) {  // a set index outside [0, nmatch)
    for (int at : {0, nit * 8 - 1}) {
      std::vector<int32_t> s = sets;
      s[at] = bad;
      orbx_ransac_pair p = pair;
      p.sets = s.data();
      EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    }
  }
  {  // fewer than 8 matches
    std::vector<int32_t> m = m12;
    m[0] = m[1] = m[2] = -1;
    std::vector<int32_t> s((size_t)nit * 8, 0);
    orbx_ransac_pair p = pair;
    p.match12 = m.data(), p.sets = s.data();
    EXPECT(call(1, &p, nit) == ORBX_ERR_ARG);
    m[2] = 2;  // eight
    for (size_t i = 0; i < s.size(); ++i) s[i] = (int32_t)(i % 8);
    EXPECT(call(1, &p, nit) == ORBX_ERR_NO_DEVICE);
  }
  {  // the flag segments
    int32_t narrow[2] = {0, nmatch - 1}, neg[2] = {-1, nmatch}, wide[2] = {3, 3 + nmatch};
    EXPECT(orbm_initializer_ransac(1, &pair, nit, 1.0f, 0, res, inlH, inlF, narrow) == ORBX_ERR_ARG);
    EXPECT(orbm_initializer_ransac(1, &pair, nit, 1.0f, 0, res, inlH, inlF, neg) == ORBX_ERR_ARG);
    EXPECT(orbm_initializer_ransac(1, &pair, nit, 1.0f, 0, res, inlH, inlF, wide) == ORBX_ERR_NO_DEVICE);
    int32_t second[3] = {0, nmatch, 2 * nmatch - 1};
    orbx_ransac_pair two[2] = {pair, pair};
    EXPECT(orbm_initializer_ransac(2, two, nit, 1.0f, 0, res, inlH, inlF, second) == ORBX_ERR_ARG);
  }
  {  // a second pair's errors are found too
    orbx_ransac_pair two[2] = {pair, pair};
    two[1].n2 = 11;  // row 12 matches key 11
    EXPECT(call(2, two, nit) == ORBX_ERR_ARG);
    two[1] = pair;
    EXPECT(call(2, two, nit) == ORBX_ERR_NO_DEVICE);
  }
  EXPECT(untouched());
  // well formed
  EXPECT(call(1, &pair, nit) == ORBX_ERR_NO_DEVICE);
  EXPECT(call(1, &pair, 0) == ORBX_ERR_NO_DEVICE);
  EXPECT(call(1, &pair, nit, 0.0f) == ORBX_ERR_NO_DEVICE);  // finite: 1 / 0 is the reference's own
  EXPECT(untouched());
  int counts[4] = {-1, -1, -1, -1};
  EXPECT(orbx_debug_live_resources(counts) == ORBX_OK);
  EXPECT(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0);

  printf("initransac_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

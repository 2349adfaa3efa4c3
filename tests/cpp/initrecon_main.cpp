// Host-side ASan/UBSan run of the initializer reconstruction's host code
// (csrc/api_initrecon.hip): every argument check of
// orbm_initializer_reconstruct, the choice of the model and the count of the
// flags, all of which return before a device is needed.  No GPU is touched (the
// test hides the devices: a well-formed call ends in ORBX_ERR_NO_DEVICE).  Built
// by `make sanitize`.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "orbx.h"
#include "expect.h"

int main() {
  const int n1 = 14, n2 = 12;
  std::vector<orbx_keypoint> k1((size_t)n1), k2((size_t)n2);
  memset(k1.data(), 0, sizeof(orbx_keypoint) * n1);
  memset(k2.data(), 0, sizeof(orbx_keypoint) * n2);
  for (int i = 0; i < n1; ++i) k1[i].x = 10.0f * i, k1[i].y = 7.0f * (i % 5);
  for (int i = 0; i < n2; ++i) k2[i].x = 10.0f * i + 3.0f, k2[i].y = 7.0f * (i % 5) + 1.0f;
  // ten matches, rows 3, 7, 11 and 13 unmatched
  std::vector<int32_t> m12 = {0, 1, 2, -1, 4, 5, 6, -1, 8, 9, 10, -1, 11, -1};
  const int nmatch = 10;
  // exactly nmatch flags each: a read past them is a heap overflow under ASan
  std::vector<uint8_t> fH = {1, 1, 0, 1, 1, 1, 0, 1, 1, 1}, fF = {1, 0, 1, 1, 1, 1, 1, 1, 0, 1};
  orbx_ransac_result rs;
  memset(&rs, 0, sizeof rs);
  for (int i = 0; i < 9; ++i) rs.H21[i] = rs.F21[i] = i % 4 == 0 ? 1.0f : 0.01f * i;
  rs.SH = 10.0f, rs.SF = 10.0f, rs.RH = 0.5f, rs.it_H = 3, rs.it_F = 4, rs.nmatch = nmatch;
  orbx_recon_pair pair;
  memset(&pair, 0, sizeof pair);
  pair.n1 = n1, pair.n2 = n2, pair.keys1 = k1.data(), pair.keys2 = k2.data(), pair.match12 = m12.data();
  const float K[9] = {500.0f, 0.0f, 320.0f, 0.0f, 500.0f, 240.0f, 0.0f, 0.0f, 1.0f};
  memcpy(pair.K, K, sizeof K);
  pair.model = ORBX_RECON_AUTO, pair.ransac = &rs, pair.inliers_H = fH.data(), pair.inliers_F = fF.data();

  orbx_recon_result res[2];
  std::vector<float> P3D((size_t)2 * n1 * 3);
  std::vector<uint8_t> tri((size_t)2 * n1);
  int32_t off[3] = {0, n1, 2 * n1};
  memset(res, 0x5A, sizeof res);
  memset(P3D.data(), 0x5A, P3D.size() * sizeof(float));
  memset(tri.data(), 9, tri.size());
  auto untouched = [&] {
    const unsigned char* r = reinterpret_cast<const unsigned char*>(res);
    for (size_t i = 0; i < sizeof res; ++i)
      if (r[i] != 0x5A) return false;
    const unsigned char* q = reinterpret_cast<const unsigned char*>(P3D.data());
    for (size_t i = 0; i < P3D.size() * sizeof(float); ++i)
      if (q[i] != 0x5A) return false;
    for (uint8_t v : tri)
      if (v != 9) return false;
    return true;
  };
  auto call = [&](int npair, const orbx_recon_pair* p, float sigma = 1.0f, float minpar = 1.0f) {
    return orbm_initializer_reconstruct(npair, p, sigma, minpar, 50, 0, res, P3D.data(), tri.data(), off);
  };
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

  EXPECT(orbm_initializer_reconstruct(0, nullptr, 1.0f, 1.0f, 50, 0, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
  EXPECT(call(-1, &pair) == ORBX_ERR_ARG);
  EXPECT(call(1, nullptr) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_reconstruct(1, &pair, 1.0f, 1.0f, 50, 0, nullptr, P3D.data(), tri.data(), off) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_reconstruct(1, &pair, 1.0f, 1.0f, 50, 0, res, nullptr, tri.data(), off) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_reconstruct(1, &pair, 1.0f, 1.0f, 50, 0, res, P3D.data(), nullptr, off) == ORBX_ERR_ARG);
  EXPECT(orbm_initializer_reconstruct(1, &pair, 1.0f, 1.0f, 50, 0, res, P3D.data(), tri.data(), nullptr) == ORBX_ERR_ARG);
  for (float bad : {nan, inf, -inf}) {
    EXPECT(call(1, &pair, bad) == ORBX_ERR_ARG);
    EXPECT(call(1, &pair, 1.0f, bad) == ORBX_ERR_ARG);
  }
  EXPECT(call(65536, &pair) == ORBX_ERR_UNSUPPORTED);
  {  // the pair's pointers, counts and model
    orbx_recon_pair p = pair;
    p.keys1 = nullptr;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p = pair, p.keys2 = nullptr;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p = pair, p.match12 = nullptr;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p = pair, p.ransac = nullptr;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p = pair, p.n1 = -1;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p = pair, p.n2 = -1;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    for (int32_t m : {-1, 3, INT32_MAX, INT32_MIN}) {
      p = pair, p.model = m;
      EXPECT(call(1, &p) == ORBX_ERR_ARG);
    }
    // the limits are refused before anything of that length is read
    p = pair, p.n1 = 8193;
    EXPECT(call(1, &p) == ORBX_ERR_UNSUPPORTED);
    p = pair, p.n2 = 8193;
    EXPECT(call(1, &p) == ORBX_ERR_UNSUPPORTED);
  }
  {  // the flag arrays: AUTO needs both, a forced model only its own
    orbx_recon_pair p = pair;
    p.inliers_H = nullptr;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p.model = ORBX_RECON_H;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p.model = ORBX_RECON_F;
    EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
    p = pair, p.inliers_F = nullptr;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p.model = ORBX_RECON_F;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    p.model = ORBX_RECON_H;
    EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
  }
  for (float bad : {nan, inf, -inf})  // every entry of K
    for (int e = 0; e < 9; ++e) {
      orbx_recon_pair p = pair;
      p.K[e] = bad;
      EXPECT(call(1, &p) == ORBX_ERR_ARG);
    }
  for (float bad : {nan, inf, -inf}) {  // every key of both frames, matched or not
    for (int which = 0; which < 4; ++which) {
      std::vector<orbx_keypoint> a = k1, b = k2;
      if (which == 0) a[3].x = bad;
      if (which == 1) a[n1 - 2].y = bad;
      if (which == 2) b[7].x = bad;
      if (which == 3) b[0].y = bad;
      orbx_recon_pair p = pair;
      p.keys1 = a.data(), p.keys2 = b.data();
      EXPECT(call(1, &p) == ORBX_ERR_ARG);
    }
  }
  for (int32_t bad : {n2, n2 + 1, INT32_MAX}) {  // match12 >= n2
    std::vector<int32_t> m = m12;
    m[5] = bad;
    orbx_recon_pair p = pair;
    p.match12 = m.data();
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
  }
  {  // ransac->nmatch against the match list
    std::vector<int32_t> m = m12;
    m[5] = INT32_MIN;  // nine matches now
    orbx_recon_pair p = pair;
    p.match12 = m.data();
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    orbx_ransac_result r9 = rs;
    r9.nmatch = 9;
    p.ransac = &r9;
    EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
    r9.nmatch = 11;  // one more than the list: the flags are never read past it
    p = pair, p.ransac = &r9;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
    r9.nmatch = -1;
    EXPECT(call(1, &p) == ORBX_ERR_ARG);
  }
  {  // the key segments
    int32_t narrow[2] = {0, n1 - 1}, neg[2] = {-1, n1}, wide[2] = {3, 3 + n1};
    EXPECT(orbm_initializer_reconstruct(1, &pair, 1.0f, 1.0f, 50, 0, res, P3D.data(), tri.data(), narrow) == ORBX_ERR_ARG);
    EXPECT(orbm_initializer_reconstruct(1, &pair, 1.0f, 1.0f, 50, 0, res, P3D.data(), tri.data(), neg) == ORBX_ERR_ARG);
    EXPECT(orbm_initializer_reconstruct(1, &pair, 1.0f, 1.0f, 50, 0, res, P3D.data(), tri.data(), wide) ==
           ORBX_ERR_NO_DEVICE);
    int32_t second[3] = {0, n1, 2 * n1 - 1};
    orbx_recon_pair two[2] = {pair, pair};
    EXPECT(orbm_initializer_reconstruct(2, two, 1.0f, 1.0f, 50, 0, res, P3D.data(), tri.data(), second) == ORBX_ERR_ARG);
  }
  {  // a second pair's errors are found too
    orbx_recon_pair two[2] = {pair, pair};
    two[1].n2 = 11;  // row 12 matches key 11
    EXPECT(call(2, two) == ORBX_ERR_ARG);
    two[1] = pair;
    EXPECT(call(2, two) == ORBX_ERR_NO_DEVICE);
  }
  EXPECT(untouched());
  // well formed: every model, either side of the RH threshold, absent matrices, no inlier, no key
  for (int32_t m : {ORBX_RECON_H, ORBX_RECON_F, ORBX_RECON_AUTO}) {
    orbx_recon_pair p = pair;
    p.model = m;
    EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
  }
  {
    orbx_ransac_result r = rs;
    orbx_recon_pair p = pair;
    p.ransac = &r;
    for (float rh : {0.39f, 0.40f, 0.41f, nan, inf}) {
      r.RH = rh;
      EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
    }
    r = rs, r.it_H = r.it_F = -1;
    EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
    std::vector<uint8_t> none((size_t)nmatch, 0);
    p = pair, p.inliers_H = p.inliers_F = none.data();
    EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
    r = rs, r.nmatch = 0;
    p = pair, p.ransac = &r, p.n1 = 0;  // no key in frame 1: no match, no flag is read
    p.inliers_H = p.inliers_F = none.data();
    EXPECT(call(1, &p) == ORBX_ERR_NO_DEVICE);
  }
  EXPECT(call(1, &pair, 0.0f, -5.0f) == ORBX_ERR_NO_DEVICE);  // finite: th2 = 0 is the reference's own
  EXPECT(untouched());
  int counts[4] = {-1, -1, -1, -1};
  EXPECT(orbx_debug_live_resources(counts) == ORBX_OK);
  EXPECT(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0);

  printf("initrecon_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

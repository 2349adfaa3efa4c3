// tri_compat_main.cpp -- ORBmatcher::SearchForTriangulation called as
// LocalMapping::CreateNewMapPoints calls it (src/LocalMapping.cc:177-191), on
// a stand-in KeyFrame with the members the matcher reads, through
// cpp/orbslam2_compat.hpp: once per neighbour (the reference's form) and once
// batched.  argv: input file (written by tests/test_triangulation_compat.py),
// output file (text: "S p i j" = pair (i, j) of the single call on neighbour
// p, "NS p n" = its return value, "B p i j" / "NB total" = the batched call).
#include <stdio.h>

#include <map>
#include <utility>
#include <vector>

#include "orbslam2_compat.hpp"

namespace ORB_SLAM2 {
class MapPoint {};
class KeyFrame {
 public:
  int N = 0;
  std::vector<cv::KeyPoint> mvKeysUn;
  cv::Mat mDescriptors;
  std::map<unsigned int, std::vector<unsigned int>> mFeatVec;  // DBoW2::FeatureVector
  std::vector<float> mvLevelSigma2;
  MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
  std::vector<MapPoint*> mvpMapPoints;
};
}  // namespace ORB_SLAM2
using namespace ORB_SLAM2;
using std::pair;
using std::vector;

static MapPoint g_mp;

template <class T>
static bool rd(FILE* f, T* p, size_t n) {
  return n == 0 || fread(p, sizeof(T), n, f) == n;
}

static bool read_kf(FILE* f, KeyFrame& kf) {
  int hdr[4];  // n, nnodes, nfeat, nlevels
  if (!rd(f, hdr, 4)) return false;
  kf.N = hdr[0];
  kf.mvKeysUn.resize(hdr[0]);
  kf.mDescriptors.create(hdr[0], 32, CV_8U);
  std::vector<unsigned char> mp(hdr[0]);
  std::vector<unsigned int> ids(hdr[1]), off(hdr[1] + 1), feat(hdr[2]);
  kf.mvLevelSigma2.resize(hdr[3]);
  if (!rd(f, kf.mvKeysUn.data(), hdr[0]) || !rd(f, kf.mDescriptors.data, (size_t)hdr[0] * 32) ||
      !rd(f, mp.data(), hdr[0]) || !rd(f, ids.data(), hdr[1]) || !rd(f, off.data(), hdr[1] + 1) ||
      !rd(f, feat.data(), hdr[2]) || !rd(f, kf.mvLevelSigma2.data(), hdr[3]))
    return false;
  kf.mvpMapPoints.assign(hdr[0], nullptr);
  for (int i = 0; i < hdr[0]; ++i)
    if (mp[i]) kf.mvpMapPoints[i] = &g_mp;
  for (int j = 0; j < hdr[1]; ++j)
    kf.mFeatVec[ids[j]] = std::vector<unsigned int>(feat.begin() + off[j], feat.begin() + off[j + 1]);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int nk = 0;
  if (!rd(f, &nk, 1) || nk < 0) return 2;
  KeyFrame kf1;
  std::vector<KeyFrame> kf2(nk);
  if (!read_kf(f, kf1)) return 2;
  for (int p = 0; p < nk; ++p)
    if (!read_kf(f, kf2[p])) return 2;
  std::vector<cv::Mat> vF12;
  for (int p = 0; p < nk; ++p) {
    cv::Mat F12(3, 3, CV_32F);
    for (int r = 0; r < 3; ++r)
      if (!rd(f, F12.ptr<float>(r), 3)) return 2;
    vF12.push_back(F12);
  }
  fclose(f);
  FILE* o = fopen(argv[2], "w");
  if (!o) return 2;
  try {
    ORBmatcher matcher(0.6, true);
    KeyFrame* pKF = &kf1;
    // the reference's loop: one call per neighbour (LocalMapping.cc:177-191)
    for (int p = 0; p < nk; ++p) {
      KeyFrame* pKF2 = &kf2[p];
      vector<pair<size_t, size_t> > vMatchedIndices;
      const int n = matcher.SearchForTriangulation(pKF, pKF2, vF12[p], vMatchedIndices, false);
      fprintf(o, "NS %d %d\n", p, n);
      for (const auto& m : vMatchedIndices) fprintf(o, "S %d %zu %zu\n", p, m.first, m.second);
    }
    // bOnlyStereo: nothing
    if (nk > 0) {
      vector<pair<size_t, size_t> > vMatchedIndices(3);
      const int n = matcher.SearchForTriangulation(pKF, &kf2[0], vF12[0], vMatchedIndices, true);
      fprintf(o, "STEREO %d %zu\n", n, vMatchedIndices.size());
    }
    // the same loop as one batched call
    std::vector<KeyFrame*> vpNeighKFs;
    for (int p = 0; p < nk; ++p) vpNeighKFs.push_back(&kf2[p]);
    std::vector<vector<pair<size_t, size_t> > > vv;
    const int total = matcher.SearchForTriangulation(pKF, vpNeighKFs, vF12, vv, false);
    fprintf(o, "NB %d\n", total);
    for (int p = 0; p < nk; ++p)
      for (const auto& m : vv[p]) fprintf(o, "B %d %zu %zu\n", p, m.first, m.second);
  } catch (const cv::Exception& e) {
    fprintf(stderr, "cv::Exception %d: %s\n", e.code, e.what());
    fclose(o);
    return 1;
  }
  fclose(o);
  return 0;
}

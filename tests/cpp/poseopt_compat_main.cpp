// poseopt_compat_main.cpp -- ORB_SLAM2::Optimizer::PoseOptimization of
// cpp/orbslam2_compat.hpp over a stand-in Frame (poseopt_mocks.hpp) against the
// CPU restatement (tests/cpp/poseopt_ref.c, linked in, DEVICE order) fed
// straight from the same objects: mvbOutlier, the pose handed to SetPose word
// for word, and the return value; the single-frame and the batched overload,
// and the reference's return-0 path.  Prints one line per check; exit status
// = failures.
#include <stdio.h>
#include <string.h>

#include "poseopt_mocks.hpp"
#include "expect.h"

extern "C" {
typedef struct {
  double obs[3], X[3], w;
  int stereo;
} po_edge;
int po_pose_optimization(const float Tcw[12], const float intr[5], int nlevels, const float* inv_level_sigma2, int n,
                         const orbx_keypoint* keys, const float* uright, const float* pos, const int32_t* point_index,
                         const uint8_t* has_point, int npos, int order, float Tcw_out[16], uint8_t* outlier,
                         int* counters, po_edge* E, uint8_t* has, uint8_t* ever, double pose7[7]);
}

using namespace ORB_SLAM2;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uni() {  // [0, 1)
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0;
}
static double uni(double a, double b) { return a + (b - a) * uni(); }

static cv::Mat pose(double ay, double ax, double tx, double ty, double tz) {
  cv::Mat T(4, 4, CV_32F);
  const double R[3][3] = {{cos(ay), sin(ay) * sin(ax), sin(ay) * cos(ax)},
                          {0, cos(ax), -sin(ax)},
                          {-sin(ay), cos(ay) * sin(ax), cos(ay) * cos(ax)}};
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T.at<float>(r, c) = r == c ? 1.0f : 0.0f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T.at<float>(r, c) = (float)R[r][c];
  T.at<float>(0, 3) = (float)tx;
  T.at<float>(1, 3) = (float)ty;
  T.at<float>(2, 3) = (float)tz;
  return T;
}

// a frame of n features seen from `truth`, a fifth of them without a map
// point, a fifth of the rest displaced by 30-60 px, every third monocular;
// its pose starts a few degrees / centimetres off
static void make_frame(PoseFrame& F, vector<TrackPoint>& pts, int n, int npoints, const cv::Mat& truth,
                       const cv::Mat& start) {
  F.N = n;
  F.mvInvLevelSigma2.assign(1, 1.0f);
  float sf = 1.0f;
  for (int l = 1; l < 8; ++l) {
    sf *= 1.2f;
    F.mvInvLevelSigma2.push_back(1.0f / (sf * sf));
  }
  F.mvKeysUn.resize(n);
  F.mvuRight.assign(n, -1.0f);
  F.mvpMapPoints.assign(n, nullptr);
  F.mvbOutlier.assign(n, true);  // stale flags: those of features with a point are rewritten
  pts.resize(n);
  int given = 0;
  for (int i = 0; i < n; ++i) {
    const double z = uni(2, 30), u = uni(20, 1221), v = uni(20, 356);
    const double Pc[3] = {(u - F.cx) / F.fx * z, (v - F.cy) / F.fy * z, z};
    TrackPoint& p = pts[i];
    p.id = i;
    p.pos.create(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      double w = 0;
      for (int k = 0; k < 3; ++k) w += (double)truth.at<float>(k, r) * (Pc[k] - (double)truth.at<float>(k, 3));
      p.pos.at<float>(r) = (float)w;
    }
    const bool out = uni() < 0.2;
    const double a = uni(0, 6.283), m = uni(30, 60);
    cv::KeyPoint& kp = F.mvKeysUn[i];
    kp.pt.x = (float)(u + uni(-0.5, 0.5) + (out ? m * cos(a) : 0));
    kp.pt.y = (float)(v + uni(-0.5, 0.5) + (out ? m * sin(a) : 0));
    kp.octave = (int)(uni() * 8) & 7;
    if (i % 3) F.mvuRight[i] = (float)(u - F.mbf / z + uni(-0.5, 0.5));
    const bool with_point = npoints < 0 ? uni() >= 0.2 : given < npoints;
    if (with_point) {
      F.mvpMapPoints[i] = &p;
      ++given;
    }
  }
  F.SetPose(start);
  F.nSetPose = 0;
}

struct Ref {
  float T[16];
  vector<uint8_t> outlier;
  int ninliers;
};

static Ref restate(PoseFrame& F) {
  const int n = F.N;
  vector<float> pos((size_t)n * 3, 0.0f);
  vector<uint8_t> has(n, 0), has2(n ? n : 1), ever(n ? n : 1);
  for (int i = 0; i < n; ++i)
    if (F.mvpMapPoints[i]) {
      has[i] = 1;
      for (int c = 0; c < 3; ++c) pos[3 * i + c] = F.mvpMapPoints[i]->pos.at<float>(c);
    }
  float Tcw[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) Tcw[4 * r + c] = F.mTcw.at<float>(r, c);
  const float intr[5] = {F.fx, F.fy, F.cx, F.cy, F.mbf};
  Ref R;
  R.outlier.assign(n ? n : 1, 0);
  vector<po_edge> E(n ? n : 1);
  int counters[16];
  double pose7[7];
  R.ninliers = po_pose_optimization(Tcw, intr, (int)F.mvInvLevelSigma2.size(), F.mvInvLevelSigma2.data(), n,
                                    reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data()), F.mvuRight.data(),
                                    pos.data(), nullptr, has.data(), n, 1, R.T, R.outlier.data(), counters, E.data(),
                                    has2.data(), ever.data(), pose7);
  return R;
}

// the frame after PoseOptimization against the restatement run before it
static void check(const char* what, PoseFrame& F, const Ref& R, int ret, const vector<bool>& flags_before) {
  int same = 0, with_point = 0, kept = 0;
  for (int i = 0; i < F.N; ++i) {
    if (F.mvpMapPoints[i]) {
      ++with_point;
      same += F.mvbOutlier[i] == (R.outlier[i] != 0);
    } else {
      kept += F.mvbOutlier[i] == flags_before[i];  // the reference does not touch these
    }
  }
  EXPECT(same == with_point);
  EXPECT(kept == F.N - with_point);
  EXPECT(ret == R.ninliers);
  int words = 0;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) words += memcmp(&F.mTcw.at<float>(r, c), &R.T[4 * r + c], 4) == 0;
  EXPECT(words == 16);
  printf("%s: %d inliers, %d of %d flags, %d of 16 pose words, SetPose x %d\n", what, ret, same, with_point, words,
         F.nSetPose);
}

int main() {
  const cv::Mat truth = pose(0.2, -0.1, 0.5, -0.3, 1.0);
  const cv::Mat start = pose(0.22, -0.12, 0.54, -0.27, 1.03);
  {
    PoseFrame F;
    vector<TrackPoint> pts;
    make_frame(F, pts, 600, -1, truth, start);
    const Ref R = restate(F);
    const vector<bool> before = F.mvbOutlier;
    const int ret = Optimizer::PoseOptimization(&F);
    EXPECT(F.nSetPose == 1 && ret > 300);
    check("single frame", F, R, ret, before);
  }
  {  // the batched overload: unequal sizes, one frame on the return-0 path, one empty
    const int sizes[5] = {600, 65, 40, 0, 257}, npoints[5] = {-1, -1, 2, -1, -1};
    PoseFrame F[5];
    vector<TrackPoint> pts[5];
    vector<Ref> R;
    vector<vector<bool> > before;
    vector<PoseFrame*> vp;
    for (int f = 0; f < 5; ++f) {
      make_frame(F[f], pts[f], sizes[f], npoints[f], truth, start);
      R.push_back(restate(F[f]));
      before.push_back(F[f].mvbOutlier);
      vp.push_back(&F[f]);
    }
    const vector<int> ret = Optimizer::PoseOptimization(vp);
    EXPECT(ret.size() == 5);
    for (int f = 0; f < 5; ++f) {
      char what[32];
      snprintf(what, sizeof what, "batch frame %d", f);
      check(what, F[f], R[f], ret[f], before[f]);
    }
    // fewer than 3 correspondences: 0, the two flags cleared, SetPose not called
    EXPECT(ret[2] == 0 && F[2].nSetPose == 0 && ret[3] == 0 && F[3].nSetPose == 0);
    EXPECT(F[0].nSetPose == 1 && F[1].nSetPose == 1 && F[4].nSetPose == 1);
  }
  {  // a Frame whose octave is out of range is refused before anything is written
    PoseFrame F;
    vector<TrackPoint> pts;
    make_frame(F, pts, 65, 65, truth, start);
    F.mvKeysUn[7].octave = 8;
    const vector<bool> before = F.mvbOutlier;
    bool thrown = false;
    try {
      Optimizer::PoseOptimization(&F);
    } catch (const cv::Exception&) {
      thrown = true;
    }
    EXPECT(thrown && F.nSetPose == 0 && F.mvbOutlier == before);
  }
  printf("poseopt_compat_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

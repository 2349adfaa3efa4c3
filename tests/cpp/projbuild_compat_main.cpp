// projbuild_compat_main.cpp -- the device-side projection's call sites of
// cpp/orbslam2_compat.hpp over stand-in Frame / KeyFrame / MapPoint classes:
// ORBmatcher::SearchLocalPoints (the frustum test of a whole vector) and the
// last-frame and keyframe forms of SearchByProjection, against the CPU
// restatement (tests/cpp/projbuild_ref.c, linked in) fed straight from the same
// objects: the helper's written-back fields bit for bit, and the members'
// matches against orbm_search_by_projection on the restatement's live rows
// only, compacted in order and mapped back.  Prints one line per check;
// exit status = failures.
#include <stdio.h>
#include <string.h>

#include <set>

#include "projbuild_mocks.hpp"
#include "expect.h"

extern "C" {
typedef struct {
  float Rcw[9], tcw[3], ow[3], fx, fy, cx, cy, mbf, min_x, max_x, min_y, max_y;
  int nlevels;
  float sf[32], lsf;
} pb_camera;
typedef struct {
  const float *pos, *normal, *min_dist_inv, *max_dist_inv, *max_dist;
  const int32_t* octave;
  const float* angle;
  const uint8_t* skip;
} pb_points;
void pb_project(int mode, const pb_camera* C, const pb_points* P, int npts, float th, float vcl, int rule,
                orbx_query_proj* q, int32_t* level, float* vcos, int32_t* branch, int32_t* counts);
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

static void init_frame(TrackFrame& F, long id, const cv::Mat& Tcw) {
  F.mnId = id;
  F.mvScaleFactors.assign(1, 1.0f);
  for (int l = 1; l < 8; ++l) F.mvScaleFactors.push_back(F.mvScaleFactors.back() * 1.2f);
  F.SetPose(Tcw);
}

// map points spread around the frustum of F: behind it, beside it, beyond both
// distance gates, to both sides of the viewing-angle limit
static void make_points(const TrackFrame& F, int n, vector<TrackPoint>& pts) {
  pts.resize(n);
  for (int i = 0; i < n; ++i) {
    TrackPoint& p = pts[i];
    p.id = i;
    const double z = uni() < 0.1 ? uni(-8, -0.5) : uni(0.5, 40);
    const double u = uni(-0.1, 1.1) * 1241, v = uni(-0.1, 1.1) * 376;
    const double Pc[3] = {(u - F.cx) / F.fx * z, (v - F.cy) / F.fy * z, z};
    p.pos.create(3, 1, CV_32F);
    double PO[3], d2 = 0;
    for (int r = 0; r < 3; ++r) {
      double w = 0;
      for (int k = 0; k < 3; ++k) w += (double)F.mTcw.at<float>(k, r) * (Pc[k] - (double)F.mTcw.at<float>(k, 3));
      p.pos.at<float>(r) = (float)w;
      PO[r] = w - (double)F.mOw.at<float>(r);
      d2 += PO[r] * PO[r];
    }
    const double dist = sqrt(d2);
    p.mfMaxDistance = (float)(dist * pow(1.2, uni(-1.4, 8.6)));
    p.mfMinDistance = p.mfMaxDistance / F.mvScaleFactors[7];
    // a unit normal at cos c to PO
    const double c = uni() < 0.2 ? uni(0.9975, 1.0) : uni(0.35, 0.9975);
    double a[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)}, dot = 0, an = 0;
    for (int r = 0; r < 3; ++r) dot += a[r] * PO[r] / dist;
    for (int r = 0; r < 3; ++r) {
      a[r] -= dot * PO[r] / dist;
      an += a[r] * a[r];
    }
    p.normal.create(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) p.normal.at<float>(r) = (float)(c * PO[r] / dist + sqrt(1 - c * c) * a[r] / sqrt(an));
    p.desc.create(1, 32, CV_8UC1);
    for (int b = 0; b < 32; ++b) p.desc.ptr(0)[b] = (uint8_t)(uni() * 256);
    p.bad = uni() < 0.05;
    p.mnLastFrameSeen = uni() < 0.05 ? F.mnId : -1;
  }
}

static pb_camera camera_of(const TrackFrame& F, const cv::Mat& Ow) {
  pb_camera c;
  memset(&c, 0, sizeof c);
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) c.Rcw[3 * r + k] = F.mTcw.at<float>(r, k);
    c.tcw[r] = F.mTcw.at<float>(r, 3);
    c.ow[r] = Ow.at<float>(r);
  }
  c.fx = F.fx, c.fy = F.fy, c.cx = F.cx, c.cy = F.cy, c.mbf = F.mbf;
  c.min_x = F.mnMinX, c.max_x = F.mnMaxX, c.min_y = F.mnMinY, c.max_y = F.mnMaxY;
  c.nlevels = 8;
  for (int l = 0; l < 8; ++l) c.sf[l] = F.mvScaleFactors[l];
  c.lsf = F.mfLogScaleFactor;
  return c;
}

struct Rows {
  vector<float> pos, normal, dmin, dmax, draw, angle, vcos;
  vector<int32_t> octave, level, branch;
  vector<uint8_t> skip, desc;
  vector<orbx_query_proj> q;
  int32_t counts[2] = {0, 0};
  explicit Rows(int n)
      : pos(3 * n), normal(3 * n), dmin(n), dmax(n), draw(n), angle(n), vcos(n), octave(n), level(n), branch(n),
        skip(n), desc(32 * n), q(n) {}
  void point(int i, TrackPoint* p) {
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = p->pos.at<float>(k), normal[3 * i + k] = p->normal.at<float>(k);
    dmin[i] = 0.8f * p->mfMinDistance;
    dmax[i] = 1.2f * p->mfMaxDistance;
    draw[i] = p->mfMaxDistance;
    memcpy(&desc[32 * i], p->desc.ptr(0), 32);
  }
  void project(int mode, const pb_camera& C, float th, float vcl, int rule) {
    const pb_points P = {pos.data(), normal.data(), dmin.data(), dmax.data(), draw.data(), octave.data(),
                         angle.data(), skip.data()};
    pb_project(mode, &C, &P, (int)skip.size(), th, vcl, rule, q.data(), level.data(), vcos.data(), branch.data(),
               counts);
  }
};

// a current frame of nf features around the live rows' projections; a tenth
// already holds a map point
static void make_features(TrackFrame& F, const Rows& R, vector<TrackPoint>& pts_of_row, int nf, TrackPoint* held) {
  vector<int> live;
  for (size_t i = 0; i < R.branch.size(); ++i)
    if (R.branch[i] == 0) live.push_back((int)i);
  F.N = nf;
  F.mvKeysUn.resize(nf);
  F.mDescriptors.create(nf, 32, CV_8UC1);
  F.mvpMapPoints.assign(nf, nullptr);
  for (int j = 0; j < nf; ++j) {
    const int s = live[(size_t)(uni() * live.size())];
    cv::KeyPoint& k = F.mvKeysUn[j];
    k.pt.x = R.q[s].x + (float)uni(-3, 3);
    k.pt.y = R.q[s].y + (float)uni(-3, 3);
    k.octave = std::min(7, std::max(0, R.level[s] + (int)(uni() * 3) - 1));
    k.angle = (float)fmod(R.q[s].angle + uni(-8, 8) + 360.0, 360.0);
    memcpy(F.mDescriptors.ptr(j), &R.desc[32 * (size_t)s], 32);
    for (int f = (int)(uni() * 30); f > 0; --f) {
      const int b = (int)(uni() * 256);
      F.mDescriptors.ptr(j)[b >> 3] ^= (uint8_t)(1u << (b & 7));
    }
    if (uni() < 0.1) F.mvpMapPoints[j] = held;
  }
  F.mvKeys = F.mvKeysUn;
  (void)pts_of_row;
}

// orbm_search_by_projection on the live rows only, mapped back to row numbers
static int expected_matches(int mode, const TrackFrame& F, const Rows& R, float nnratio, int th_dist, bool ori,
                            vector<int32_t>& row_of_feature) {
  vector<orbx_query_proj> q;
  vector<uint8_t> qd;
  vector<int> keep;
  for (size_t i = 0; i < R.branch.size(); ++i)
    if (R.branch[i] == 0) {
      q.push_back(R.q[i]);
      qd.insert(qd.end(), &R.desc[32 * i], &R.desc[32 * i] + 32);
      keep.push_back((int)i);
    }
  vector<uint8_t> occ(F.N);
  for (int i = 0; i < F.N; ++i) occ[i] = F.mvpMapPoints[i] != nullptr;
  orbx_proj_frame pf = {F.N, reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data()), F.mDescriptors.data, nullptr,
                        occ.data(), F.mnMinX, F.mnMinY, F.mfGridElementWidthInv, F.mfGridElementHeightInv};
  vector<int32_t> m(F.N, -1);
  int nm = 0;
  EXPECT(orbm_search_by_projection(mode, &pf, q.data(), qd.data(), (int)q.size(), nnratio, th_dist, ori ? 1 : 0, 0,
                                   m.data(), &nm) == ORBX_OK);
  row_of_feature.assign(F.N, -1);
  for (int i = 0; i < F.N; ++i)
    if (m[i] >= 0) row_of_feature[i] = keep[m[i]];
  return nm;
}

static void check_matches(const char* what, const TrackFrame& F, const vector<TrackPoint*>& before,
                          const vector<TrackPoint*>& who, const vector<int32_t>& row_of_feature, int got, int want) {
  int same = 0;
  for (int i = 0; i < F.N; ++i) {
    TrackPoint* e = row_of_feature[i] >= 0 ? who[row_of_feature[i]] : before[i];
    same += F.mvpMapPoints[i] == e;
  }
  EXPECT(same == F.N);
  EXPECT(got == want);
  EXPECT(want >= 40);
  printf("%s: %d matches, %d of %d features as expected\n", what, got, same, F.N);
}

int main() {
  const int NP = 900, NF = 400;
  ORBmatcher matcher(0.9f, true);
  TrackPoint held;

  // ---- SearchLocalPoints
  {
    TrackFrame F;
    init_frame(F, 7, pose(0.1, 0.05, 0.3, -0.2, 0.5));
    vector<TrackPoint> pts;
    make_points(F, NP, pts);
    vector<TrackPoint*> vp;
    Rows R(NP);
    for (int i = 0; i < NP; ++i) {
      vp.push_back(&pts[i]);
      R.point(i, &pts[i]);
      R.skip[i] = pts[i].mnLastFrameSeen == F.mnId || pts[i].bad;
      pts[i].mbTrackInView = i % 2;  // stale values the helper must overwrite (or leave, for skipped points)
    }
    R.project(1, camera_of(F, F.mOw), 1.0f, 0.5f, 0);
    const int n = matcher.SearchLocalPoints(F, vp, 0.5f);
    int same = 0, skipped_kept = 0;
    for (int i = 0; i < NP; ++i) {
      const TrackPoint& p = pts[i];
      if (R.skip[i]) {
        skipped_kept += p.mbTrackInView == (bool)(i % 2) && p.mnTrackScaleLevel == -1;
        continue;
      }
      const bool live = R.branch[i] == 0;
      bool ok = p.mbTrackInView == live;
      if (live)
        ok = ok && !memcmp(&p.mTrackProjX, &R.q[i].x, 4) && !memcmp(&p.mTrackProjY, &R.q[i].y, 4) &&
             !memcmp(&p.mTrackProjXR, &R.q[i].xr, 4) && p.mnTrackScaleLevel == R.level[i] &&
             !memcmp(&p.mTrackViewCos, &R.vcos[i], 4);
      else
        ok = ok && p.mnTrackScaleLevel == -1;
      same += ok;
    }
    int nskip = 0;
    for (int i = 0; i < NP; ++i) nskip += R.skip[i];
    EXPECT(n == R.counts[0] && n >= 100 && R.counts[1] == 0);
    EXPECT(same == NP - nskip && skipped_kept == nskip && nskip >= 20);
    printf("SearchLocalPoints: nToMatch %d, %d of %d points as the restatement, %d skipped\n", n, same, NP - nskip, nskip);
  }

  // ---- SearchByProjection(Current, Last, th, bMono)
  for (int variant = 0; variant < 3; ++variant) {  // forward, backward, neither (bMono)
    TrackFrame Last, Cur;
    init_frame(Last, 8, pose(0.1, 0.05, 0.3, -0.2, 0.5));
    init_frame(Cur, 9, pose(0.12, 0.04, 0.25, -0.2, variant == 1 ? 2.5 : -1.5));
    vector<TrackPoint> pts;
    make_points(Cur, NP, pts);
    Last.N = NP;
    Last.mvKeys.resize(NP);
    Last.mvpMapPoints.assign(NP, nullptr);
    Last.mvbOutlier.assign(NP, false);
    Rows R(NP);
    for (int i = 0; i < NP; ++i) {
      Last.mvKeys[i].octave = (int)(uni() * 8);
      Last.mvKeys[i].angle = (float)uni(0, 360);
      if (uni() >= 0.1) Last.mvpMapPoints[i] = &pts[i];
      Last.mvbOutlier[i] = uni() < 0.1;
      R.point(i, &pts[i]);
      R.octave[i] = Last.mvKeys[i].octave;
      R.angle[i] = Last.mvKeys[i].angle;
      R.skip[i] = !Last.mvpMapPoints[i] || Last.mvbOutlier[i];
    }
    const bool bMono = variant == 2;
    const cv::Mat Rcw = Cur.mTcw.rowRange(0, 3).colRange(0, 3), tcw = Cur.mTcw.rowRange(0, 3).col(3);
    const cv::Mat twc = -Rcw.t() * tcw;
    const cv::Mat tlc = Last.mTcw.rowRange(0, 3).colRange(0, 3) * twc + Last.mTcw.rowRange(0, 3).col(3);
    const bool fwd = tlc.at<float>(2) > Cur.mb && !bMono, bwd = -tlc.at<float>(2) > Cur.mb && !bMono;
    EXPECT(variant == 0 ? fwd : variant == 1 ? bwd : (!fwd && !bwd));
    R.project(2, camera_of(Cur, twc), 15.0f, 0.0f, fwd ? 1 : bwd ? 2 : 0);
    make_features(Cur, R, pts, NF, &held);
    const vector<TrackPoint*> before = Cur.mvpMapPoints;
    vector<int32_t> rows;
    const int want = expected_matches(2, Cur, R, 0.9f, ORBmatcher::TH_HIGH, true, rows);
    const int got = matcher.SearchByProjection(Cur, Last, 15.0f, bMono);
    check_matches(variant == 0 ? "last frame, forward" : variant == 1 ? "last frame, backward" : "last frame, mono",
                  Cur, before, Last.mvpMapPoints, rows, got, want);
  }

  // ---- SearchByProjection(Current, KeyFrame*, sAlreadyFound, th, ORBdist)
  {
    TrackFrame Cur;
    init_frame(Cur, 10, pose(-0.08, 0.03, -0.4, 0.1, 0.7));
    vector<TrackPoint> pts;
    make_points(Cur, NP, pts);
    TrackKeyFrame KF;
    KF.mvKeys.resize(NP);
    KF.mvpMapPoints.assign(NP, nullptr);
    std::set<TrackPoint*> found;
    Rows R(NP);
    for (int i = 0; i < NP; ++i) {
      KF.mvKeys[i].angle = (float)uni(0, 360);
      if (uni() >= 0.1) KF.mvpMapPoints[i] = &pts[i];
      if (uni() < 0.1) found.insert(&pts[i]);
      R.point(i, &pts[i]);
      R.angle[i] = KF.mvKeys[i].angle;
      R.skip[i] = !KF.mvpMapPoints[i] || pts[i].bad || found.count(&pts[i]);
    }
    const cv::Mat Rcw = Cur.mTcw.rowRange(0, 3).colRange(0, 3), tcw = Cur.mTcw.rowRange(0, 3).col(3);
    R.project(3, camera_of(Cur, -Rcw.t() * tcw), 10.0f, 0.0f, 0);
    make_features(Cur, R, pts, NF, &held);
    const vector<TrackPoint*> before = Cur.mvpMapPoints;
    vector<int32_t> rows;
    const int want = expected_matches(3, Cur, R, 0.9f, 64, true, rows);
    const int got = matcher.SearchByProjection(Cur, &KF, found, 10.0f, 64);
    check_matches("keyframe", Cur, before, KF.mvpMapPoints, rows, got, want);
  }
  printf("projbuild_compat_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

// kfbuild_compat_main.cpp -- ORBmatcher::Fuse (both forms, and the batched
// form) and SearchBySim3 of cpp/orbslam2_compat.hpp with
// SetKfProjection(KfProjection::Device), on the stand-in classes and planted
// scenes of kfwin_compat_main.cpp, next to the restatement
// (tests/cpp/kfbuild_ref.c, linked in) followed by the reference's search and
// walk over the same classes.  argv: seed, output file; the output has
// kfwin_compat_main.cpp's form (side H = restatement + walk, D = compat header).
//
// The scene builder, the search loop (ref_best) and the dump are
// kfwin_compat_main.cpp's own, taken in with its main() renamed.
#define main kfwin_compat_main_unused
#include "kfwin_compat_main.cpp"
#undef main

// the stand-in MapPoint has no GetMaxDistance(): the header finds this one by
// argument-dependent lookup
namespace ORB_SLAM2 {
inline float GetMaxDistance(MapPoint* p) { return p->mfMaxDistance; }
}  // namespace ORB_SLAM2

extern "C" {
typedef struct {
  float Rcw[9], tcw[3], ow[3], sR21[9], t21[3];
  float fx, fy, cx, cy;
  float min_x, max_x, min_y, max_y;
  int nlevels;
  float sf[32];
  float lsf;
} kb_camera;
typedef struct {
  const float* pos;
  const float* min_dist_inv;
  const float* max_dist_inv;
  const float* max_dist;
  const uint8_t* skip;
} kb_points;
typedef struct {
  float x, y, radius;
  int32_t level, desc;
} kb_query;
void kb_project(int form, int fused, const kb_camera* C, const kb_points* P, int npts, int32_t desc_base, float th,
                kb_query* q, int32_t* level, int32_t* branch, int32_t* counts);
}

static int g_projected = 0, g_live = 0;

static kb_camera rs_camera(KeyFrame* pKFi, KeyFrame* pKFs, const cv::Mat& R, const cv::Mat& t, const cv::Mat* Ow,
                           const cv::Mat* sR21, const cv::Mat* t21) {
  kb_camera c;
  memset(&c, 0, sizeof c);
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) {
      c.Rcw[3 * r + k] = R.at<float>(r, k);
      if (sR21) c.sR21[3 * r + k] = sR21->at<float>(r, k);
    }
    c.tcw[r] = t.at<float>(r);
    if (Ow) c.ow[r] = Ow->at<float>(r);
    if (t21) c.t21[r] = t21->at<float>(r);
  }
  c.fx = pKFi->fx;
  c.fy = pKFi->fy;
  c.cx = pKFi->cx;
  c.cy = pKFi->cy;
  c.min_x = pKFs->mnMinX;
  c.max_x = pKFs->mnMaxX;
  c.min_y = pKFs->mnMinY;
  c.max_y = pKFs->mnMaxY;
  c.nlevels = pKFs->mnScaleLevels;
  for (int l = 0; l < c.nlevels; ++l) c.sf[l] = pKFs->mvScaleFactors[l];
  c.lsf = pKFs->mfLogScaleFactor;
  return c;
}

// the restatement on one map point; false where the reference `continue`s
static bool rs_project(int form, const kb_camera& cam, MapPoint* pMP, float th, float& u, float& v, float& radius,
                       int& level) {
  const cv::Mat P = pMP->GetWorldPos();
  const float pos[3] = {P.at<float>(0), P.at<float>(1), P.at<float>(2)};
  const float dmin = pMP->GetMinDistanceInvariance(), dmax = pMP->GetMaxDistanceInvariance();
  const float draw = pMP->mfMaxDistance;
  const kb_points pts = {pos, &dmin, &dmax, &draw, nullptr};
  kb_query q;
  int32_t lv = -1, branch = 0, counts[2];
  kb_project(form, 1, &cam, &pts, 1, 0, th, &q, &lv, &branch, counts);
  ++g_projected;
  if (lv < 0) return false;
  ++g_live;
  u = q.x;
  v = q.y;
  radius = q.radius;
  level = lv;
  return true;
}

static int rs_fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th) {
  const cv::Mat Ow = pKF->GetCameraCenter();
  const kb_camera cam = rs_camera(pKF, pKF, pKF->GetRotation(), pKF->GetTranslation(), &Ow, nullptr, nullptr);
  int nFused = 0;
  for (auto pMP : vpMapPoints) {
    if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
    float u, v, radius;
    int level, bestIdx;
    if (!rs_project(1, cam, pMP, th, u, v, radius, level)) continue;
    const cv::Mat MPdescriptor = pMP->GetDescriptor();
    int bestDist = ref_best(pKF, u, v, radius, level, MPdescriptor, bestIdx);
    if (bestDist <= TH_LOW) {
      MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) {
          if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
        }
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
  }
  return nFused;
}

static int rs_fuse_scw(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
                       vector<MapPoint*>& vpReplacePoint) {
  cv::Mat Rcw = Scw.rowRange(0, 3).colRange(0, 3);
  cv::Mat tcw = Scw.rowRange(0, 3).col(3);
  cv::Mat Ow = -Rcw.t() * tcw;
  const kb_camera cam = rs_camera(pKF, pKF, Rcw, tcw, &Ow, nullptr, nullptr);
  int nFused = 0;
  for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
    MapPoint* pMP = vpPoints[iMP];
    if (!pMP || pMP->isBad() || pKF->GetMapPoint(pMP->GetIndexInKeyFrame(pKF))) continue;
    float u, v, radius;
    int level, bestIdx;
    if (!rs_project(1, cam, pMP, th, u, v, radius, level)) continue;
    const cv::Mat dMP = pMP->GetDescriptor();
    int bestDist = ref_best(pKF, u, v, radius, level, dMP, bestIdx);
    if (bestDist <= TH_LOW) {
      MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
  }
  return nFused;
}

static int rs_sim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, const float& s12,
                   const cv::Mat& R12, const cv::Mat& t12, const float th) {
  cv::Mat sR21 = (1.0 / s12) * R12.t();
  cv::Mat t21 = -sR21 * t12;
  const kb_camera cam = rs_camera(pKF1, pKF2, pKF1->GetRotation(), pKF1->GetTranslation(), nullptr, &sR21, &t21);
  const vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  vector<bool> vbAlreadyMatched1(vpMapPoints1.size(), false);
  vector<int> vnMatch1(vpMapPoints1.size(), -1);
  for (size_t i = 0; i < vpMatches12.size(); i++) {
    MapPoint* pMP = vpMatches12[i];
    if (pMP) {
      int idx2 = pMP->GetIndexInKeyFrame(pKF2);
      if (idx2 >= 0) vbAlreadyMatched1[i] = true;
    }
  }
  int nMatches = 0;
  for (size_t i1 = 0; i1 < vpMapPoints1.size(); ++i1) {
    MapPoint* pMP1 = vpMapPoints1[i1];
    if (!pMP1 || vbAlreadyMatched1[i1] || pMP1->isBad()) continue;
    float u, v, radius;
    int predictedLevel, bestIdx2;
    if (!rs_project(2, cam, pMP1, th, u, v, radius, predictedLevel)) continue;
    const cv::Mat dMP1 = pMP1->GetDescriptor();
    int bestDist = ref_best(pKF2, u, v, radius, predictedLevel, dMP1, bestIdx2);
    if (bestDist <= TH_HIGH) {
      vnMatch1[i1] = bestIdx2;
      nMatches++;
    }
  }
  vpMatches12 = vector<MapPoint*>(vpMapPoints1.size(), nullptr);
  for (size_t i = 0; i < vnMatch1.size(); i++)
    if (vnMatch1[i] >= 0) vpMatches12[i] = pKF2->GetMapPoint(vnMatch1[i]);
  return nMatches;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint64_t seed = strtoull(argv[1], nullptr, 10);
  FILE* o = fopen(argv[2], "w");
  if (!o) return 2;
  try {
    ORBmatcher matcher(0.8, true);
    matcher.SetKfProjection(ORBmatcher::KfProjection::Device);
    for (int side = 0; side < 2; ++side) {
      const char c = side ? 'D' : 'H';
      {
        Scene S;
        build(S, seed, 1, 400, 300);
        KeyFrame* pKFi = S.kfs[0];
        const int n = side ? matcher.Fuse(pKFi, S.cand) : rs_fuse(pKFi, S.cand, 3.0);
        dump(o, "FUSE", c, n, S, nullptr);
      }
      {
        Scene S;
        build(S, seed + 1, 1, 400, 300);
        KeyFrame* pKF = S.kfs[0];
        cv::Mat Scw = pKF->Tcw.clone();
        vector<MapPoint*> vpReplacePoints(S.cand.size(), static_cast<MapPoint*>(nullptr));
        const int n = side ? matcher.Fuse(pKF, Scw, S.cand, 4, vpReplacePoints)
                           : rs_fuse_scw(pKF, Scw, S.cand, 4, vpReplacePoints);
        dump(o, "SCW", c, n, S, &vpReplacePoints);
      }
      {
        Scene S;
        build(S, seed + 2, 2, 400, 300);
        KeyFrame *pKF1 = S.kfs[0], *pKF2 = S.kfs[1];
        size_t at = 0;
        for (int i = 0; i < pKF1->N && at < S.cand.size(); ++i)
          if (!pKF1->mvpMapPoints[i]) {
            while (at < S.cand.size() && !S.cand[at]) ++at;
            if (at < S.cand.size()) pKF1->mvpMapPoints[i] = S.cand[at++];
          }
        cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
        cv::Mat R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
        cv::Mat R12 = R1w * R2w.t();
        cv::Mat t12 = -R12 * t2w + t1w;
        const float s12 = 1.01f;
        vector<MapPoint*> vpMatches12(pKF1->N, static_cast<MapPoint*>(nullptr));
        for (int i = 0; i < pKF1->N; i += 9) vpMatches12[i] = pKF2->GetMapPoint(i % pKF2->N);
        const int n = side ? matcher.SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, 7.5)
                           : rs_sim3(pKF1, pKF2, vpMatches12, s12, R12, t12, 7.5);
        dump(o, "SIM3", c, n, S, &vpMatches12);
      }
      {
        Scene S;
        build(S, seed + 3, 5, 400, 250, false);
        int n = 0;
        if (side) {
          n = matcher.Fuse(S.kfs, S.cand);
        } else {
          for (KeyFrame* pKFi : S.kfs) n += rs_fuse(pKFi, S.cand, 3.0);
        }
        dump(o, "BATCH", c, n, S, nullptr);
      }
    }
    fprintf(o, "RS projected %d live %d\n", g_projected, g_live);
  } catch (const cv::Exception& e) {
    fprintf(stderr, "cv::Exception %d: %s\n", e.code, e.what());
    fclose(o);
    return 1;
  }
  fclose(o);
  return 0;
}

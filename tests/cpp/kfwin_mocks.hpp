// kfwin_mocks.hpp -- stand-in KeyFrame / MapPoint classes with the members
// ORBmatcher::Fuse (both forms) and SearchBySim3 read (src/ORBmatcher.cc:
// 504-730), shared by tests/cpp/kfwin_compat_main.cpp and the signature probes
// of tests/test_kfwindow_compat.py.  Replace / AddObservation / AddMapPoint
// are recorded as events.
#ifndef KFWIN_MOCKS_HPP
#define KFWIN_MOCKS_HPP

#include <limits.h>
#include <math.h>
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

#include "orbslam2_compat.hpp"

using std::vector;

static vector<std::string> g_events;
static void event(const char* fmt, long a, long b, long c) {
  char buf[96];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  g_events.push_back(buf);
}

namespace ORB_SLAM2 {
class KeyFrame;

// observations in keyframe-id order, not address order: Replace walks them,
// and the order of its events must not depend on where the allocator put
// each scene's keyframes
struct KeyFrameById {
  bool operator()(const KeyFrame* a, const KeyFrame* b) const;
};

class MapPoint {
 public:
  long id = 0;
  cv::Mat pos, desc;  // 3x1 CV_32F, 1x32 CV_8U
  bool bad = false;
  int nObs = 0;
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::map<KeyFrame*, size_t, KeyFrameById> obs;

  bool isBad() { return bad; }
  bool IsInKeyFrame(KeyFrame* pKF) { return obs.count(pKF) != 0; }
  int GetIndexInKeyFrame(KeyFrame* pKF) { return obs.count(pKF) ? (int)obs[pKF] : -1; }
  cv::Mat GetWorldPos() { return pos.clone(); }
  float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
  int PredictScale(const float& currentDist, KeyFrame* pKF);
  cv::Mat GetDescriptor() { return desc.clone(); }
  int Observations() { return nObs; }
  void AddObservation(KeyFrame* pKF, size_t idx);
  void Replace(MapPoint* pMP);
};

class KeyFrame {
 public:
  long id = 0;
  int N = 0;
  float fx = 500, fy = 500, cx = 320, cy = 240;
  int mnMinX = 0, mnMinY = 0, mnMaxX = 640, mnMaxY = 480;
  int mnGridCols = 64, mnGridRows = 48;
  float mfGridElementWidthInv = 64.0f / 640.0f, mfGridElementHeightInv = 48.0f / 480.0f;
  int mnScaleLevels = 8;
  float mfLogScaleFactor = logf(1.2f);
  vector<float> mvScaleFactors;
  vector<cv::KeyPoint> mvKeysUn;
  cv::Mat mDescriptors;
  cv::Mat Tcw;  // 4x4
  vector<MapPoint*> mvpMapPoints;
  vector<vector<vector<size_t> > > mGrid;

  cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
  cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
  cv::Mat GetCameraCenter() { return -GetRotation().t() * GetTranslation(); }
  bool IsInImage(const float& x, const float& y) const {
    return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY);
  }
  // an index the reference would read out of range (GetIndexInKeyFrame = -1)
  // is "no map point" here
  MapPoint* GetMapPoint(const size_t& idx) { return idx < mvpMapPoints.size() ? mvpMapPoints[idx] : nullptr; }
  vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  void AddMapPoint(MapPoint* pMP, const size_t& idx) {
    event("M %ld %ld %ld", id, pMP->id, (long)idx);
    mvpMapPoints[idx] = pMP;
  }
  void ReplaceMapPointMatch(const size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
  void EraseMapPointMatch(const size_t& idx) { mvpMapPoints[idx] = nullptr; }

  // Frame::AssignFeaturesToGrid (the KeyFrame copies the Frame's grid)
  void AssignFeaturesToGrid() {
    mGrid.assign(mnGridCols, vector<vector<size_t> >(mnGridRows));
    for (int i = 0; i < N; i++) {
      const cv::KeyPoint& kp = mvKeysUn[i];
      const int posX = round((kp.pt.x - mnMinX) * mfGridElementWidthInv);
      const int posY = round((kp.pt.y - mnMinY) * mfGridElementHeightInv);
      if (posX < 0 || posX >= mnGridCols || posY < 0 || posY >= mnGridRows) continue;
      mGrid[posX][posY].push_back(i);
    }
  }
  // KeyFrame::GetFeaturesInArea, for the host loop
  vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r) const {
    vector<size_t> vIndices;
    const int nMinCellX = std::max(0, (int)floor((x - mnMinX - r) * mfGridElementWidthInv));
    if (nMinCellX >= mnGridCols) return vIndices;
    const int nMaxCellX = std::min((int)mnGridCols - 1, (int)ceil((x - mnMinX + r) * mfGridElementWidthInv));
    if (nMaxCellX < 0) return vIndices;
    const int nMinCellY = std::max(0, (int)floor((y - mnMinY - r) * mfGridElementHeightInv));
    if (nMinCellY >= mnGridRows) return vIndices;
    const int nMaxCellY = std::min((int)mnGridRows - 1, (int)ceil((y - mnMinY + r) * mfGridElementHeightInv));
    if (nMaxCellY < 0) return vIndices;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
      for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
        const vector<size_t>& vCell = mGrid[ix][iy];
        for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
          const cv::KeyPoint& kpUn = mvKeysUn[vCell[j]];
          const float distx = kpUn.pt.x - x;
          const float disty = kpUn.pt.y - y;
          if (fabs(distx) < r && fabs(disty) < r) vIndices.push_back(vCell[j]);
        }
      }
    return vIndices;
  }
};

inline bool KeyFrameById::operator()(const KeyFrame* a, const KeyFrame* b) const { return a->id < b->id; }

inline int MapPoint::PredictScale(const float& currentDist, KeyFrame* pKF) {  // src/MapPoint.cc
  float ratio = mfMaxDistance / currentDist;
  int nScale = ceil(log(ratio) / pKF->mfLogScaleFactor);
  if (nScale < 0) nScale = 0;
  else if (nScale >= pKF->mnScaleLevels) nScale = pKF->mnScaleLevels - 1;
  return nScale;
}
inline void MapPoint::AddObservation(KeyFrame* pKF, size_t idx) {
  event("A %ld %ld %ld", id, pKF->id, (long)idx);
  if (obs.count(pKF)) return;
  obs[pKF] = idx;
  nObs++;
}
// MapPoint::Replace: the observations move to pMP, this point turns bad, and
// pMP's descriptor is recomputed (here: one bit of it flips)
inline void MapPoint::Replace(MapPoint* pMP) {
  if (pMP->id == id) return;
  event("R %ld %ld %ld", id, pMP->id, 0);
  std::map<KeyFrame*, size_t, KeyFrameById> o = obs;
  obs.clear();
  bad = true;
  for (auto& kv : o) {
    if (!pMP->IsInKeyFrame(kv.first)) {
      kv.first->ReplaceMapPointMatch(kv.second, pMP);
      pMP->AddObservation(kv.first, kv.second);
    } else {
      kv.first->EraseMapPointMatch(kv.second);
    }
  }
  pMP->desc.ptr(0)[(pMP->nObs + id) & 31] ^= 1;
}
}  // namespace ORB_SLAM2

#endif

// projbuild_mocks.hpp -- what the device-side projection's call sites read
// beside kfwin_mocks.hpp: a MapPoint with the tracking fields and the raw
// maximum distance, a Frame with a pose, and a KeyFrame with distorted keys
// (tests/cpp/projbuild_compat_main.cpp).
#ifndef PROJBUILD_MOCKS_HPP
#define PROJBUILD_MOCKS_HPP

#include "kfwin_mocks.hpp"

namespace ORB_SLAM2 {

class TrackPoint : public MapPoint {
 public:
  cv::Mat normal;  // 3x1 CV_32F
  long mnLastFrameSeen = -1;
  bool mbTrackInView = false;
  float mTrackProjX = -1, mTrackProjY = -1, mTrackProjXR = -1, mTrackViewCos = -1;
  int mnTrackScaleLevel = -1;
  cv::Mat GetNormal() { return normal.clone(); }
  float GetMaxDistance() { return mfMaxDistance; }  // the accessor the call site adds
};

class TrackFrame {
 public:
  long mnId = 0;
  int N = 0;
  cv::Mat mTcw, mOw;  // 4x4, 3x1
  float fx = 718.856f, fy = 718.856f, cx = 607.19f, cy = 185.22f, mbf = 386.1448f, mb = 0.5372f;
  float mnMinX = 0, mnMaxX = 1241, mnMinY = 0, mnMaxY = 376;
  float mfGridElementWidthInv = 64.0f / 1241.0f, mfGridElementHeightInv = 48.0f / 376.0f;
  int mnScaleLevels = 8;
  float mfLogScaleFactor = logf(1.2f);
  vector<float> mvScaleFactors;
  vector<cv::KeyPoint> mvKeys, mvKeysUn;
  cv::Mat mDescriptors;
  vector<TrackPoint*> mvpMapPoints;
  vector<bool> mvbOutlier;

  void SetPose(const cv::Mat& Tcw) {
    mTcw = Tcw.clone();
    const cv::Mat R = mTcw.rowRange(0, 3).colRange(0, 3), t = mTcw.rowRange(0, 3).col(3);
    mOw = -R.t() * t;
  }
};

class TrackKeyFrame {
 public:
  vector<cv::KeyPoint> mvKeys;
  vector<TrackPoint*> mvpMapPoints;
  vector<TrackPoint*> GetMapPointMatches() { return mvpMapPoints; }
};

}  // namespace ORB_SLAM2

#endif

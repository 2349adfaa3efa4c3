// poseopt_mocks.hpp -- what Optimizer::PoseOptimization reads beside
// projbuild_mocks.hpp: a Frame with right coordinates and the per-level
// inverse sigmas (tests/cpp/poseopt_compat_main.cpp).
#ifndef POSEOPT_MOCKS_HPP
#define POSEOPT_MOCKS_HPP

#include "projbuild_mocks.hpp"

namespace ORB_SLAM2 {

class PoseFrame : public TrackFrame {
 public:
  vector<float> mvuRight;
  vector<float> mvInvLevelSigma2;
  int nSetPose = 0;
  void SetPose(const cv::Mat& Tcw) {
    ++nSetPose;
    TrackFrame::SetPose(Tcw);
  }
};

}  // namespace ORB_SLAM2

#endif

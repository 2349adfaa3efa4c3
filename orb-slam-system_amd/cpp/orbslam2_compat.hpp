// orbslam2_compat.hpp -- the reference's own class surface for the hot path,
// over liborbx, for code bases without OpenCV.
//
// The reference's call sites (Frame::ExtractORB, src/Frame.cc:227-233; the
// Frame ctors' scale getters, :49-55,107-113,162-168; Tracking's extractor
// construction, src/Tracking.cc:76-82; LoopClosing::ComputeSim3 ->
// SearchByBoW(KF, KF), src/LoopClosing.cc:149; DescriptorDistance callers,
// src/Frame.cc:521, src/MapPoint.cc:252) compile unchanged against this
// header:
//   * namespace cv: the subset of OpenCV 3.4 types those signatures use
//     (Mat for CV_8UC1 data, InputArray / OutputArray, KeyPoint, Point_),
//     with OpenCV's value semantics (Mat headers share a ref-counted buffer);
//   * ORB_SLAM2::ORBextractor with the public surface of the reference's
//     include/ORBextractor.h:25-91 (constructor, operator(), the six getters,
//     public mvImagePyramid);
//   * ORB_SLAM2::ORBmatcher with ORBmatcher.h's DescriptorDistance and the
//     two SearchByBoW overloads (include/ORBmatcher.h:20-45),
//     SearchForInitialization (:48), SearchForTriangulation (:51-52),
//     SearchBySim3 (:56) and both Fuse forms
//     (:59, :62) as templates over the caller's KeyFrame / MapPoint / Frame
//     classes, reading exactly the members the reference reads
//     (GetMapPointMatches, GetMapPoint, isBad, mvKeysUn, mFeatVec,
//     mDescriptors, mvLevelSigma2, N; for Fuse / SearchBySim3 also the pose
//     getters, fx .. cy, IsInImage, mvScaleFactors, the grid constants and
//     the MapPoint members of src/ORBmatcher.cc:504-730), and the last-frame
//     and keyframe forms of SearchByProjection (:34-39) with a
//     SearchLocalPoints helper for Tracking's frustum loop, projected and
//     searched on the device (these read mTcw, mOw, the intrinsics, the image
//     bounds, the scale tables and, beyond the reference, MapPoint::GetMaxDistance()).
// A project that has OpenCV keeps its cv:: and uses INTEGRATION.md's glue
// instead; define ORBX_COMPAT_NO_CV to take cv:: from OpenCV headers.
#ifndef ORBX_ORBSLAM2_COMPAT_HPP
#define ORBX_ORBSLAM2_COMPAT_HPP

#include <stdint.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/orbx.h"

#ifndef ORBX_COMPAT_NO_CV
#ifndef CV_8U
#define CV_8U 0
#endif
#ifndef CV_8UC1
#define CV_8UC1 0
#endif
#ifndef CV_32F
#define CV_32F 5
#endif

namespace cv {

template <typename T>
struct Point_ {
  T x = 0, y = 0;
  Point_() {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<float> Point2f;
typedef Point_<int> Point2i;
typedef Point2i Point;

template <typename T>
struct Point3_ {
  T x = 0, y = 0, z = 0;
  Point3_() {}
  Point3_(T x_, T y_, T z_) : x(x_), y(y_), z(z_) {}
};
typedef Point3_<float> Point3f;

// cv::KeyPoint: 28 bytes, the field order orbx_keypoint mirrors
struct KeyPoint {
  Point2f pt;
  float size = 0, angle = -1, response = 0;
  int octave = 0, class_id = -1;
  KeyPoint() {}
  KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0,
           int class_id_ = -1)
      : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
};

class Exception : public std::runtime_error {
 public:
  int code;
  Exception(int c, const std::string& msg) : std::runtime_error(msg), code(c) {}
};

// 2-D single-channel matrix header (CV_8UC1 images and descriptors; CV_32F for
// the small float matrices the matcher takes, e.g. F12, and the poses and
// points of Fuse / SearchBySim3) over a shared byte buffer (OpenCV value
// semantics: copies share data, create() reallocates only when the shape
// changes).  The CV_32F operators below (*, +, -, unary minus, t(), norm) are
// plain float arithmetic in source order; their rounding against OpenCV's
// small-matrix product (gemm, with its own accumulation order and a folded
// scale) is unpinned, as DESIGN.md §11 says of undistortPoints: a code base
// with OpenCV defines ORBX_COMPAT_NO_CV and gets OpenCV's rounding.
class Mat {
 public:
  int rows = 0, cols = 0;
  uint8_t* data = nullptr;
  size_t step = 0;

  Mat() {}
  Mat(int r, int c, int type) { create(r, c, type); }
  // wraps external data (not owned), like cv::Mat(rows, cols, type, data, step)
  Mat(int r, int c, int type, void* d, size_t st = 0)
      : rows(r), cols(c), data(static_cast<uint8_t*>(d)), step(st ? st : (size_t)c * esz(type)), type_(type) {}

  void create(int r, int c, int type) {
    if (buf_ && r == rows && c == cols && type == type_ && step == (size_t)c * esz(type)) return;
    buf_ = std::make_shared<std::vector<uint8_t>>((size_t)r * c * esz(type));
    rows = r;
    cols = c;
    step = (size_t)c * esz(type);
    type_ = type;
    data = buf_->data();
  }
  void release() {
    buf_.reset();
    data = nullptr;
    rows = cols = 0;
    step = 0;
  }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  int type() const { return type_; }
  bool isContinuous() const { return step == (size_t)cols * esz(type_); }
  size_t elemSize() const { return esz(type_); }
  template <typename T>
  T* ptr(int r = 0) { return reinterpret_cast<T*>(data + (size_t)r * step); }
  template <typename T>
  const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data + (size_t)r * step); }
  uint8_t* ptr(int r = 0) { return data + (size_t)r * step; }
  const uint8_t* ptr(int r = 0) const { return data + (size_t)r * step; }
  template <typename T>
  T& at(int r, int c) { return ptr<T>(r)[c]; }
  template <typename T>
  const T& at(int r, int c) const { return ptr<T>(r)[c]; }
  // at(i) of a row or column vector (Mat::at(int i0))
  template <typename T>
  T& at(int i) { return cols == 1 ? ptr<T>(i)[0] : ptr<T>(i / cols)[i % cols]; }
  template <typename T>
  const T& at(int i) const { return cols == 1 ? ptr<T>(i)[0] : ptr<T>(i / cols)[i % cols]; }
  Mat row(int r) const { return rowRange(r, r + 1); }
  Mat rowRange(int r0, int r1) const {
    Mat m(*this);
    m.rows = r1 - r0;
    m.data = data + (size_t)r0 * step;
    return m;
  }
  Mat col(int c) const { return colRange(c, c + 1); }
  Mat colRange(int c0, int c1) const {
    Mat m(*this);
    m.cols = c1 - c0;
    m.data = data + (size_t)c0 * esz(type_);
    return m;
  }
  Mat t() const {  // CV_32F
    Mat m(cols, rows, type_);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) m.at<float>(c, r) = at<float>(r, c);
    return m;
  }
  Mat clone() const {
    Mat m(rows, cols, type_);
    for (int r = 0; r < rows; ++r) memcpy(m.ptr(r), ptr(r), (size_t)cols * esz(type_));
    return m;
  }
  void copyTo(Mat& dst) const {
    if (dst.data == data && dst.rows == rows && dst.cols == cols) return;
    Mat src(*this);  // keeps the source alive if dst aliases it
    dst.create(rows, cols, type_);
    for (int r = 0; r < rows; ++r) memcpy(dst.ptr(r), src.ptr(r), (size_t)cols * esz(type_));
  }

 private:
  static size_t esz(int type) { return type == CV_32F ? sizeof(float) : 1; }
  std::shared_ptr<std::vector<uint8_t>> buf_;
  int type_ = CV_8UC1;
};

// CV_32F arithmetic, float, in source order (see the note above class Mat)
inline Mat operator*(const Mat& a, const Mat& b) {
  if (a.cols != b.rows) throw Exception(-1, "cv::Mat operator*: shapes");
  Mat m(a.rows, b.cols, CV_32F);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < b.cols; ++c) {
      float acc = 0.0f;
      for (int k = 0; k < a.cols; ++k) {
        const float prod = a.at<float>(r, k) * b.at<float>(k, c);
        acc = k == 0 ? prod : acc + prod;
      }
      m.at<float>(r, c) = acc;
    }
  return m;
}
inline Mat operator*(double s, const Mat& a) {
  Mat m(a.rows, a.cols, CV_32F);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = (float)(s * (double)a.at<float>(r, c));
  return m;
}
inline Mat operator*(const Mat& a, double s) { return s * a; }
inline Mat operator+(const Mat& a, const Mat& b) {
  if (a.rows != b.rows || a.cols != b.cols) throw Exception(-1, "cv::Mat operator+: shapes");
  Mat m(a.rows, a.cols, CV_32F);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = a.at<float>(r, c) + b.at<float>(r, c);
  return m;
}
inline Mat operator-(const Mat& a, const Mat& b) {
  if (a.rows != b.rows || a.cols != b.cols) throw Exception(-1, "cv::Mat operator-: shapes");
  Mat m(a.rows, a.cols, CV_32F);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = a.at<float>(r, c) - b.at<float>(r, c);
  return m;
}
inline Mat operator-(const Mat& a) {
  Mat m(a.rows, a.cols, CV_32F);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = -a.at<float>(r, c);
  return m;
}
// cv::norm(m), NORM_L2 of a CV_32F matrix: the squares summed in double, as
// OpenCV's normL2 accumulates floats
inline double norm(const Mat& a) {
  double s = 0.0;
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) s += (double)a.at<float>(r, c) * (double)a.at<float>(r, c);
  return __builtin_sqrt(s);
}

class _InputArray {
 public:
  _InputArray(const Mat& m) : m_(&m) {}
  Mat getMat() const { return *m_; }
  bool empty() const { return m_->empty(); }
  int type() const { return m_->type(); }

 private:
  const Mat* m_;
};
typedef const _InputArray& InputArray;

class _OutputArray {
 public:
  _OutputArray(Mat& m) : m_(&m) {}
  void create(int r, int c, int type) const { m_->create(r, c, type); }
  void release() const { m_->release(); }
  Mat& getMatRef() const { return *m_; }
  Mat getMat() const { return *m_; }

 private:
  Mat* m_;
};
typedef const _OutputArray& OutputArray;

}  // namespace cv
#endif  // ORBX_COMPAT_NO_CV

namespace ORB_SLAM2 {

inline void orbx_throw(int rc, const char* what) {
  if (rc != ORBX_OK) throw cv::Exception(rc, std::string(what) + ": " + orbx_status_string(rc));
}

static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint layout");

// ORB_SLAM2::ORBextractor (reference include/ORBextractor.h:25-91) over
// orbx_extractor: one liborbx extractor (own HIP stream and scratch) per
// instance, so the stereo threads of Frame::Frame (src/Frame.cc:58-61) run
// two instances concurrently as before.
class ORBextractor {
 public:
  enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

  ORBextractor(int nfeatures_, float scaleFactor_, int nlevels_, int iniThFAST_, int minThFAST_)
      : nfeatures(nfeatures_), scaleFactor(scaleFactor_), nlevels(nlevels_),
        iniThFAST(iniThFAST_), minThFAST(minThFAST_) {
    // cell_guard: 0 reproduces the reference (throws on negative-extent FAST
    // cells, e.g. at 1920x1080); ORBX_CELL_GUARD=1 in the environment selects
    // upstream ORB-SLAM2's skip
    const char* g = getenv("ORBX_CELL_GUARD");
    orbx_params p = {nfeatures_, scaleFactor_, nlevels_, iniThFAST_, minThFAST_, g && *g == '1'};
    mvScaleFactor.resize(nlevels);
    mvInvScaleFactor.resize(nlevels);
    mvLevelSigma2.resize(nlevels);
    mvInvLevelSigma2.resize(nlevels);
    mnFeaturesPerLevel.resize(nlevels);
    umax.resize(16);
    orbx_throw(orbx_tables(&p, mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(),
                           mvInvLevelSigma2.data(), mnFeaturesPerLevel.data(), umax.data()),
               "ORBextractor");
    orbx_throw(orbx_extractor_create(&p, 0, &h_), "ORBextractor");
    orbx_throw(orbx_extractor_set_options(h_, ORBX_EXTRACTOR_PYRAMID_TO_HOST), "ORBextractor");
    mvImagePyramid.resize(nlevels);
  }
  ~ORBextractor() { orbx_extractor_destroy(h_); }
  ORBextractor(const ORBextractor&) = delete;
  ORBextractor& operator=(const ORBextractor&) = delete;

  // operator() (src/ORBextractor.cc:442-495); the mask is ignored there too
  void operator()(cv::InputArray _image, cv::InputArray /*_mask*/,
                  std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors) {
    if (_image.empty()) return;  // :444-445
    cv::Mat image = _image.getMat();
    if (image.type() != CV_8UC1) orbx_throw(ORBX_ERR_ARG, "ORBextractor: CV_8UC1 expected");  // :448
    int cap = 0, n = 0;
    orbx_throw(orbx_extractor_capacity(h_, image.cols, image.rows, &cap), "ORBextractor");
    kbuf_.resize(cap > 0 ? cap : 1);
    dbuf_.resize((size_t)(cap > 0 ? cap : 1) * 32);
    orbx_throw(orbx_extract(h_, image.data, image.cols, image.rows, image.step,
                            reinterpret_cast<orbx_keypoint*>(kbuf_.data()), cap, dbuf_.data(), &n),
               "ORBextractor::operator()");
    if (pyramid_to_host_) fill_pyramid();
    if (n == 0) {  // :460-463: descriptors released, keypoints untouched
      _descriptors.release();
      return;
    }
    _keypoints.assign(kbuf_.begin(), kbuf_.begin() + n);
    _descriptors.create(n, 32, CV_8U);
    cv::Mat& d = _descriptors.getMatRef();
    for (int r = 0; r < n; ++r) memcpy(d.ptr(r), dbuf_.data() + (size_t)r * 32, 32);
  }

  int inline GetLevels() { return nlevels; }
  float inline GetScaleFactor() { return (float)scaleFactor; }
  std::vector<float> inline GetScaleFactors() { return mvScaleFactor; }
  std::vector<float> inline GetInverseScaleFactors() { return mvInvScaleFactor; }
  std::vector<float> inline GetScaleSigmaSquares() { return mvLevelSigma2; }
  std::vector<float> inline GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

  // the reference fills this on every call (read by Frame::ComputeStereoMatches,
  // src/Frame.cc:453,543,555,560).  The pyramid comes back with the call (one
  // D2H of the level buffer overlapped with FAST .. BRIEF; level 0 is the
  // staged copy of the image) and the headers point into the extractor's
  // pinned buffers, which the next operator() call overwrites -- the
  // reference's call sites read it before extracting again.  Monocular
  // callers may turn it off.
  std::vector<cv::Mat> mvImagePyramid;
  void SetPyramidToHost(bool on) {
    pyramid_to_host_ = on;
    orbx_throw(orbx_extractor_set_options(h_, on ? ORBX_EXTRACTOR_PYRAMID_TO_HOST : 0), "ORBextractor");
  }
  orbx_extractor* Orbx() const { return h_; }

 protected:
  void fill_pyramid() {
    for (int l = 0; l < nlevels; ++l) {
      const uint8_t* d = nullptr;
      size_t st = 0;
      int w = 0, h = 0;
      orbx_throw(orbx_extractor_level_host(h_, l, &d, &st, &w, &h), "mvImagePyramid");
      mvImagePyramid[l] = cv::Mat(h, w, CV_8U, const_cast<uint8_t*>(d), st);
    }
  }

  int nfeatures;
  double scaleFactor;
  int nlevels;
  int iniThFAST;
  int minThFAST;
  std::vector<int> mnFeaturesPerLevel;
  std::vector<int> umax;
  std::vector<float> mvScaleFactor;
  std::vector<float> mvInvScaleFactor;
  std::vector<float> mvLevelSigma2;
  std::vector<float> mvInvLevelSigma2;

 private:
  orbx_extractor* h_ = nullptr;
  bool pyramid_to_host_ = true;
  std::vector<cv::KeyPoint> kbuf_;
  std::vector<uint8_t> dbuf_;
};

// ORB_SLAM2::ORBmatcher: DescriptorDistance, SearchByBoW,
// SearchForInitialization, SearchForTriangulation, SearchBySim3 and Fuse
// (include/ORBmatcher.h:20-62;
// src/ORBmatcher.cc:88-119,197-276,278-366,368-467,504-730,896-908).
class ORBmatcher {
 public:
  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;  // ORBmatcher.cc:13-15

  ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

  // Hamming distance of two 32-byte rows (ORBmatcher.cc:896-908): an exact
  // host popcount -- the per-pair callers (stereo search, projection search,
  // MapPoint::ComputeDistinctiveDescriptors) sit in CPU loops, where a
  // device round trip per pair would cost far more than the 8 popcounts
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
    const uint8_t* pa = a.ptr(0);
    const uint8_t* pb = b.ptr(0);
    int dist = 0;
    for (int i = 0; i < 8; ++i) {
      uint32_t va, vb;
      memcpy(&va, pa + 4 * i, 4);
      memcpy(&vb, pb + 4 * i, 4);
      dist += __builtin_popcount(va ^ vb);
    }
    return dist;
  }

  // SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (:278-366) on the
  // device.  KF: the reference's KeyFrame (GetMapPointMatches(), mvKeysUn,
  // mFeatVec, mDescriptors); MP: its MapPoint (isBad()).
  template <class KF, class MP>
  int SearchByBoW(KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches12) {
    const std::vector<MP*> vpMapPoints1 = pKF1->GetMapPointMatches();
    const std::vector<MP*> vpMapPoints2 = pKF2->GetMapPointMatches();
    Flat f1, f2;
    flatten(pKF1, vpMapPoints1, f1);
    flatten(pKF2, vpMapPoints2, f2);
    std::vector<int32_t> m12(vpMapPoints1.size(), -1);
    int n = 0;
    orbx_throw(orbm_search_by_bow(&f1.f, &f2.f, mfNNratio, mbCheckOrientation ? 1 : 0, 0,
                                  m12.data(), &n),
               "SearchByBoW");
    // as the reference (:289, :330, :359): the caller's entries survive the
    // resize; matched ones are overwritten, rotation-rejected ones reset
    vpMatches12.resize(vpMapPoints1.size(), static_cast<MP*>(nullptr));
    for (size_t i = 0; i < m12.size(); ++i) {
      if (m12[i] >= 0) vpMatches12[i] = vpMapPoints2[m12[i]];
      else if (m12[i] == -2) vpMatches12[i] = static_cast<MP*>(nullptr);
    }
    return n;
  }

  // SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (:88-119) is a stub
  // in the reference: F.N null matches, returns 0.  That stays the default
  // (SURVEY.md §5 switch bow_kf_frame=stub); SetBowKFFrame(BowKFFrame::Full)
  // selects upstream ORB-SLAM2's search on the device
  // (orbm_search_by_bow_kf_frame): KF MapPoints matched to the Frame's
  // features over common vocabulary nodes.  FR: the reference's Frame (N,
  // mvKeys, mFeatVec after ComputeBoW, mDescriptors).
  enum class BowKFFrame { Stub, Full };
  void SetBowKFFrame(BowKFFrame m) { mBowKFFrame = m; }
  template <class KF, class FR, class MP>
  int SearchByBoW(KF* pKF, FR& F, std::vector<MP*>& vpMapPointMatches) {
    if (mBowKFFrame == BowKFFrame::Stub) {
      vpMapPointMatches.resize(F.N, static_cast<MP*>(nullptr));  // :90
      return 0;
    }
    const std::vector<MP*> vpMapPointsKF = pKF->GetMapPointMatches();
    Flat fk, ff;
    flatten(pKF, vpMapPointsKF, fk);
    flatten_frame(F, ff);
    std::vector<int32_t> mf(F.N > 0 ? (size_t)F.N : 1, -1);
    int n = 0;
    orbx_throw(orbm_search_by_bow_kf_frame(&fk.f, &ff.f, mfNNratio, mbCheckOrientation ? 1 : 0, 0, mf.data(), &n),
               "SearchByBoW");
    vpMapPointMatches.assign(F.N, static_cast<MP*>(nullptr));  // upstream: vector<MapPoint*>(F.N, NULL)
    for (int i = 0; i < F.N; ++i)
      if (mf[i] >= 0) vpMapPointMatches[i] = vpMapPointsKF[mf[i]];
    return n;
  }

  // SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12,
  // vector<pair<size_t, size_t>>&, bOnlyStereo) (:368-467) on the device.  KF:
  // the reference's KeyFrame (GetMapPoint(i), mvKeysUn, mDescriptors,
  // mFeatVec, mvLevelSigma2, N); M: a 3x3 matrix with at<float>(r, c)
  // (cv::Mat, CV_32F).  With bOnlyStereo the reference matches nothing (its
  // `!bOnlyStereo &&` at :417), and so does this.
  template <class KF, class M>
  int SearchForTriangulation(KF* pKF1, KF* pKF2, M F12,
                             std::vector<std::pair<size_t, size_t> >& vMatchedPairs,
                             const bool bOnlyStereo) {
    std::vector<std::vector<std::pair<size_t, size_t> > > vv;
    const int n = SearchForTriangulation(pKF1, std::vector<KF*>(1, pKF2), std::vector<M>(1, F12), vv,
                                         bOnlyStereo);
    vMatchedPairs.swap(vv[0]);
    return n;
  }

  // The neighbour loop of LocalMapping::CreateNewMapPoints
  // (src/LocalMapping.cc:177-191) as one batched device call: pKF1 against
  // every vpKF2[p] under vF12[p].  vvMatchedPairs[p] is what the single call
  // returns for neighbour p on the MapPoints as they are now; the return
  // value is the total number of pairs.  The reference's loop triangulates
  // between its calls: a caller that adds MapPoints to pKF1 while walking
  // neighbour p's pairs drops the later pairs whose pKF1 feature has one by
  // then (exact with checkOri = false, as CreateNewMapPoints builds its
  // matcher).
  template <class KF, class M>
  int SearchForTriangulation(KF* pKF1, const std::vector<KF*>& vpKF2, const std::vector<M>& vF12,
                             std::vector<std::vector<std::pair<size_t, size_t> > >& vvMatchedPairs,
                             const bool bOnlyStereo) {
    if (vpKF2.size() != vF12.size()) orbx_throw(ORBX_ERR_ARG, "SearchForTriangulation");
    const size_t nk = vpKF2.size(), n1 = pKF1->N > 0 ? (size_t)pKF1->N : 0;
    TriFlat f1;
    flatten_tri(pKF1, f1);
    std::vector<TriFlat> f2(nk);
    std::vector<orbx_tri_frame> frames(nk);
    std::vector<float> F(nk * 9);
    for (size_t p = 0; p < nk; ++p) {
      flatten_tri(vpKF2[p], f2[p]);
      frames[p] = f2[p].f;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) F[p * 9 + 3 * r + c] = vF12[p].template at<float>(r, c);
    }
    std::vector<int32_t> m12(nk * n1 ? nk * n1 : 1, -1);
    std::vector<int> nm(nk ? nk : 1, 0);
    orbx_throw(orbm_search_for_triangulation(&f1.f, (int)nk, frames.data(), F.data(), bOnlyStereo ? 1 : 0,
                                             mbCheckOrientation ? 1 : 0, 0, m12.data(), nm.data()),
               "SearchForTriangulation");
    vvMatchedPairs.assign(nk, std::vector<std::pair<size_t, size_t> >());
    int total = 0;
    for (size_t p = 0; p < nk; ++p) {
      vvMatchedPairs[p].reserve(nm[p]);  // :459-465
      for (size_t i = 0; i < n1; ++i)
        if (m12[p * n1 + i] >= 0) vvMatchedPairs[p].push_back(std::make_pair(i, (size_t)m12[p * n1 + i]));
      total += nm[p];
    }
    return total;
  }

  // Where the queries of Fuse (both forms, and the batched form) and of
  // SearchBySim3 are built.  Host (the default): the reference's own cv::Mat
  // statements, one map point at a time, in this header.  Device: one
  // orbm_keyframe_project call over the map points' arrays; the
  // rows then go to orbm_keyframe_search as they are, inert where the reference
  // `continue`s, and the walk and its bookkeeping are the same.  u and v follow
  // the reference's object there (one fused multiply-add), which a build of
  // this header without contraction differs from in the last place.  MP then
  // needs GetMaxDistance() (the raw mfMaxDistance that PredictScale divides),
  // as a member or as a free function found by argument-dependent lookup.
  enum class KfProjection { Host, Device };
  void SetKfProjection(KfProjection m) { mKfProjection = m; }

  // Fuse(KeyFrame*, const vector<MapPoint*>&, th) (:504-568).  Three steps:
  // the queries are built with the reference's own statements, one
  // orbm_keyframe_search call finds every query's best feature, and the map
  // points are walked in order with the reference's bookkeeping against live
  // state (isBad / IsInKeyFrame re-tested at walk time, so a point an earlier
  // entry of the list replaced or added is skipped as the reference skips it).
  // Exact: within one call the only descriptors that change (Replace ->
  // ComputeDistinctiveDescriptors) belong to map points already in pKF, and
  // those are not queries.  KF: GetRotation / GetTranslation / GetCameraCenter,
  // fx fy cx cy, IsInImage, mvScaleFactors, mvKeysUn, mDescriptors, N, mnMinX,
  // mnMinY, mfGridElementWidthInv / HeightInv, GetMapPoint, AddMapPoint.  MP:
  // isBad, IsInKeyFrame, GetWorldPos, Get{Min,Max}DistanceInvariance,
  // PredictScale, GetDescriptor, Observations, Replace, AddObservation.
  template <class KF, class MP>
  int Fuse(KF* pKF, const std::vector<MP*>& vpMapPoints, const float th = 3.0) {
    return Fuse(std::vector<KF*>(1, pKF), vpMapPoints, th);
  }

  // The first loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:
  // 255-260): Fuse(vpTargetKFs[p], vpMapPoints, th) for every target keyframe,
  // as one device call; a map point's descriptor goes up once however many
  // keyframes it projects into.  Returns the sum of the calls' return values.
  // The walk is keyframe by keyframe, in order, against live state, but every
  // query carries the map point's descriptor as it was when the call began: a
  // map point that an earlier keyframe's Replace recomputed may match
  // differently in a later keyframe than in the reference's loop
  // (INTEGRATION.md 3e).  With one keyframe it is the reference's call, exact.
  template <class KF, class MP>
  int Fuse(const std::vector<KF*>& vpTargetKFs, const std::vector<MP*>& vpMapPoints, const float th = 3.0) {
    KfSearch S;
    std::vector<int32_t> slot(vpTargetKFs.size() * vpMapPoints.size(), -1);
    if (mKfProjection == KfProjection::Device) {
      // one shared point set (row i = vpMapPoints[i], desc_base = 0), a skip array per keyframe
      KfPoints I(vpMapPoints);
      for (size_t p = 0; p < vpTargetKFs.size(); ++p) {
        KF* pKF = vpTargetKFs[p];
        std::vector<uint8_t>& skip = I.begin(S, pKF, kf_camera(pKF, pKF, pKF->GetRotation(), pKF->GetTranslation(),
                                                               pKF->GetCameraCenter()));
        for (size_t i = 0; i < vpMapPoints.size(); ++i) {
          MP* pMP = vpMapPoints[i];
          skip[i] = !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF);
        }
      }
      I.run(S, ORBX_KF_FORM_FUSE, th, slot, "Fuse");
    } else {
      for (size_t p = 0; p < vpTargetKFs.size(); ++p) {
        KF* pKF = vpTargetKFs[p];
        cv::Mat Rcw = pKF->GetRotation();
        cv::Mat tcw = pKF->GetTranslation();
        cv::Mat Ow = pKF->GetCameraCenter();
        S.begin(pKF);
        for (size_t i = 0; i < vpMapPoints.size(); ++i) {
          MP* pMP = vpMapPoints[i];
          if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
          slot[p * vpMapPoints.size() + i] = fuse_query(S, pKF, Rcw, tcw, Ow, pMP, th);
        }
        S.end();
      }
      S.run("Fuse");
    }
    int nFused = 0;
    for (size_t p = 0; p < vpTargetKFs.size(); ++p) {
      KF* pKF = vpTargetKFs[p];
      for (size_t i = 0; i < vpMapPoints.size(); ++i) {
        MP* pMP = vpMapPoints[i];
        if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        const int32_t j = slot[p * vpMapPoints.size() + i];
        if (j < 0) continue;
        const int bestDist = S.best_dist[j];
        const int bestIdx = S.best_idx[j];
        if (bestDist <= TH_LOW) {
          MP* pMPinKF = pKF->GetMapPoint(bestIdx);
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
    }
    return nFused;
  }

  // Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, th, vpReplacePoint)
  // (:570-634), LoopClosing::SearchAndFuse's form: the same three steps; the
  // skip test is GetMapPoint(GetIndexInKeyFrame(pKF)), read as the reference
  // reads it, and an occupied feature is reported in vpReplacePoint.  M: the
  // caller's matrix type (cv::Mat, CV_32F).
  template <class KF, class M, class MP>
  int Fuse(KF* pKF, M Scw, const std::vector<MP*>& vpPoints, float th, std::vector<MP*>& vpReplacePoint) {
    M Rcw = Scw.rowRange(0, 3).colRange(0, 3);
    M tcw = Scw.rowRange(0, 3).col(3);
    M Ow = -Rcw.t() * tcw;
    KfSearch S;
    std::vector<int32_t> slot(vpPoints.size(), -1);
    if (mKfProjection == KfProjection::Device) {
      KfPoints I(vpPoints);
      std::vector<uint8_t>& skip = I.begin(S, pKF, kf_camera(pKF, pKF, Rcw, tcw, Ow));
      for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
        MP* pMP = vpPoints[iMP];
        skip[iMP] = !pMP || pMP->isBad() || pKF->GetMapPoint(pMP->GetIndexInKeyFrame(pKF));
      }
      I.run(S, ORBX_KF_FORM_FUSE, th, slot, "Fuse");
    } else {
      S.begin(pKF);
      for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
        MP* pMP = vpPoints[iMP];
        if (!pMP || pMP->isBad() || pKF->GetMapPoint(pMP->GetIndexInKeyFrame(pKF))) continue;
        slot[iMP] = fuse_query(S, pKF, Rcw, tcw, Ow, pMP, th);
      }
      S.end();
      S.run("Fuse");
    }
    int nFused = 0;
    for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
      MP* pMP = vpPoints[iMP];
      if (!pMP || pMP->isBad() || pKF->GetMapPoint(pMP->GetIndexInKeyFrame(pKF))) continue;
      if (slot[iMP] < 0) continue;
      const int bestDist = S.best_dist[slot[iMP]];
      const int bestIdx = S.best_idx[slot[iMP]];
      if (bestDist <= TH_LOW) {
        MP* pMPinKF = pKF->GetMapPoint(bestIdx);
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

  // SearchBySim3 (:636-730; this reference searches one direction only, KF1's
  // map points in KF2, and accepts at TH_HIGH).  Nothing changes during its
  // loop, so the walk only fills vnMatch1.
  template <class KF, class MP, class M>
  int SearchBySim3(KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches12, const float& s12, const M& R12,
                   const M& t12, const float th) {
    const float& fx = pKF1->fx;
    const float& fy = pKF1->fy;
    const float& cx = pKF1->cx;
    const float& cy = pKF1->cy;
    M R1w = pKF1->GetRotation();
    M t1w = pKF1->GetTranslation();
    M sR21 = (1.0 / s12) * R12.t();
    M t21 = -sR21 * t12;
    const std::vector<MP*> vpMapPoints1 = pKF1->GetMapPointMatches();
    // the reference indexes vbAlreadyMatched1 (this size) with vpMatches12's
    if (vpMatches12.size() > vpMapPoints1.size()) orbx_throw(ORBX_ERR_ARG, "SearchBySim3");
    std::vector<bool> vbAlreadyMatched1(vpMapPoints1.size(), false);
    std::vector<int> vnMatch1(vpMapPoints1.size(), -1);
    for (size_t i = 0; i < vpMatches12.size(); i++) {
      MP* pMP = vpMatches12[i];
      if (pMP) {
        int idx2 = pMP->GetIndexInKeyFrame(pKF2);
        if (idx2 >= 0) vbAlreadyMatched1[i] = true;
      }
    }
    KfSearch S;
    std::vector<int32_t> slot(vpMapPoints1.size(), -1);
    if (mKfProjection == KfProjection::Device) {
      // intrinsics of pKF1, bounds and scale tables of pKF2, as the reference reads them
      orbx_kf_camera cam = kf_camera(pKF1, pKF2, R1w, t1w, t1w);
      for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) cam.sR21[3 * r + k] = sR21.template at<float>(r, k);
        cam.t21[r] = t21.template at<float>(r);
        cam.ow[r] = 0.0f;
      }
      KfPoints I(vpMapPoints1);
      std::vector<uint8_t>& skip = I.begin(S, pKF2, cam);
      for (size_t i1 = 0; i1 < vpMapPoints1.size(); ++i1) {
        MP* pMP1 = vpMapPoints1[i1];
        skip[i1] = !pMP1 || vbAlreadyMatched1[i1] || pMP1->isBad();
      }
      I.run(S, ORBX_KF_FORM_SIM3, th, slot, "SearchBySim3");
    } else {
      S.begin(pKF2);
      for (size_t i1 = 0; i1 < vpMapPoints1.size(); ++i1) {
        MP* pMP1 = vpMapPoints1[i1];
        if (!pMP1 || vbAlreadyMatched1[i1] || pMP1->isBad()) continue;
        M p3Dw = pMP1->GetWorldPos();
        M p3Dc1 = R1w * p3Dw + t1w;
        M p3Dc2 = sR21 * p3Dc1 + t21;
        if (p3Dc2.template at<float>(2) < 0.0f) continue;
        float invz = 1.0f / p3Dc2.template at<float>(2);
        float x = p3Dc2.template at<float>(0) * invz;
        float y = p3Dc2.template at<float>(1) * invz;
        float u = fx * x + cx;
        float v = fy * y + cy;
        if (!pKF2->IsInImage(u, v)) continue;
        float dist = cv::norm(p3Dc2);
        if (dist < pMP1->GetMinDistanceInvariance() || dist > pMP1->GetMaxDistanceInvariance()) continue;
        int predictedLevel = pMP1->PredictScale(dist, pKF2);
        float radius = th * pKF2->mvScaleFactors[predictedLevel];
        slot[i1] = S.add(pMP1, u, v, radius, predictedLevel);
      }
      S.end();
      S.run("SearchBySim3");
    }
    int nMatches = 0;
    for (size_t i1 = 0; i1 < vpMapPoints1.size(); ++i1) {
      if (slot[i1] < 0) continue;
      if (S.best_dist[slot[i1]] <= TH_HIGH) {
        vnMatch1[i1] = S.best_idx[slot[i1]];
        nMatches++;
      }
    }
    vpMatches12 = std::vector<MP*>(vpMapPoints1.size(), static_cast<MP*>(nullptr));
    for (size_t i = 0; i < vnMatch1.size(); i++) {
      if (vnMatch1[i] >= 0) vpMatches12[i] = pKF2->GetMapPoint(vnMatch1[i]);
    }
    return nMatches;
  }

  // SearchForInitialization(Frame&, Frame&, vector<cv::Point2f>&,
  // vector<int>&, int windowSize=10) (include/ORBmatcher.h:48;
  // src/ORBmatcher.cc:197-276) on the device.  FR: the reference's Frame
  // (mvKeysUn, mDescriptors, mnMinX, mnMinY, mfGridElementWidthInv,
  // mfGridElementHeightInv).  vnMatches12 is resized as :199 does, without
  // clearing: Tracking hands in the same mvIniMatches while an initializer
  // lives, and rows this call does not match keep their entries.
  template <class FR>
  int SearchForInitialization(FR& F1, FR& F2, std::vector<cv::Point2f>& vbPrevMatched,
                              std::vector<int>& vnMatches12, int windowSize = 10) {
    orbx_init_pair P = init_pair(F1, F2, vbPrevMatched, vnMatches12);
    int n = 0;
    orbx_throw(orbm_search_for_initialization(1, &P, windowSize, mfNNratio, mbCheckOrientation ? 1 : 0, 0, &n),
               "SearchForInitialization");
    return n;
  }

  // batched form (no counterpart in the reference): pair i = (*vpF1[i],
  // *vpF2[i]) with its own vbPrevMatched / vnMatches12, for several streams
  // bootstrapping at once: one upload, one set of launches, one download.
  // Returns the nmatches of every pair.
  template <class FR>
  std::vector<int> SearchForInitialization(const std::vector<FR*>& vpF1, const std::vector<FR*>& vpF2,
                                           std::vector<std::vector<cv::Point2f> >& vvbPrevMatched,
                                           std::vector<std::vector<int> >& vvnMatches12, int windowSize = 10) {
    const size_t np = vpF1.size();
    if (vpF2.size() != np || vvbPrevMatched.size() != np || vvnMatches12.size() != np)
      orbx_throw(ORBX_ERR_ARG, "SearchForInitialization");
    std::vector<orbx_init_pair> P(np);
    for (size_t i = 0; i < np; ++i) P[i] = init_pair(*vpF1[i], *vpF2[i], vvbPrevMatched[i], vvnMatches12[i]);
    std::vector<int> n(np ? np : 1, 0);
    orbx_throw(orbm_search_for_initialization((int)np, P.data(), windowSize, mfNNratio,
                                              mbCheckOrientation ? 1 : 0, 0, n.data()),
               "SearchForInitialization");
    n.resize(np);
    return n;
  }

  // The frustum test of Tracking::SearchLocalPoints for a whole vector of map
  // points in one device call (Frame::isInFrustum per point in the reference,
  // src/Frame.cc:249-305): writes mbTrackInView, mTrackProjX / Y / XR,
  // mnTrackScaleLevel and mTrackViewCos back and returns nToMatch.  Points
  // with mnLastFrameSeen == F.mnId and bad points are skipped as there (their
  // mbTrackInView is left alone for the former, as Tracking.cc does).  MP
  // needs one accessor the reference lacks: GetMaxDistance(), the raw
  // mfMaxDistance that PredictScale divides.
  template <class FR, class MP>
  int SearchLocalPoints(FR& F, const std::vector<MP*>& vpMapPoints, float viewingCosLimit = 0.5f) {
    const int n = (int)vpMapPoints.size();
    ProjInputs I(n);
    for (int i = 0; i < n; ++i) {
      MP* pMP = vpMapPoints[i];
      I.skip[i] = !pMP || pMP->mnLastFrameSeen == F.mnId || pMP->isBad();
      if (I.skip[i]) continue;
      pMP->mbTrackInView = false;
      I.set_pos(i, pMP->GetWorldPos());
      const cv::Mat N = pMP->GetNormal();
      for (int k = 0; k < 3; ++k) I.normal[3 * i + k] = N.template at<float>(k);
      I.dmin[i] = pMP->GetMinDistanceInvariance();
      I.dmax[i] = pMP->GetMaxDistanceInvariance();
      I.draw[i] = pMP->GetMaxDistance();
    }
    const orbx_proj_camera cam = proj_camera(F, F.mOw);
    const orbx_proj_params prm = {1.0f, viewingCosLimit, ORBX_LEVEL_RULE_NEITHER};
    int nToMatch = 0;
    I.project(1, cam, prm, &nToMatch, "SearchLocalPoints");
    for (int i = 0; i < n; ++i) {
      if (I.level[i] < 0) continue;
      MP* pMP = vpMapPoints[i];
      pMP->mbTrackInView = true;
      pMP->mTrackProjX = I.q[i].x;
      pMP->mTrackProjY = I.q[i].y;
      pMP->mTrackProjXR = I.q[i].xr;
      pMP->mnTrackScaleLevel = I.level[i];
      pMP->mTrackViewCos = I.vcos[i];
    }
    return nToMatch;
  }

  // SearchByProjection(Frame& Current, const Frame& Last, th, bMono)
  // (:732-818): projection and search on the device; row i is
  // LastFrame.mvpMapPoints[i].
  template <class FR>
  int SearchByProjection(FR& CurrentFrame, const FR& LastFrame, const float th, const bool bMono) {
    const auto Rcw = CurrentFrame.mTcw.rowRange(0, 3).colRange(0, 3);
    const auto tcw = CurrentFrame.mTcw.rowRange(0, 3).col(3);
    const auto twc = -Rcw.t() * tcw;
    const auto Rlw = LastFrame.mTcw.rowRange(0, 3).colRange(0, 3);
    const auto tlw = LastFrame.mTcw.rowRange(0, 3).col(3);
    const auto tlc = Rlw * twc + tlw;
    const bool bForward = tlc.template at<float>(2) > CurrentFrame.mb && !bMono;
    const bool bBackward = -tlc.template at<float>(2) > CurrentFrame.mb && !bMono;
    const int n = LastFrame.N;
    ProjInputs I(n);
    for (int i = 0; i < n; ++i) {
      auto* pMP = LastFrame.mvpMapPoints[i];
      I.skip[i] = !pMP || LastFrame.mvbOutlier[i];
      if (I.skip[i]) continue;
      I.set_pos(i, pMP->GetWorldPos());
      I.set_desc(i, pMP->GetDescriptor());
      I.octave[i] = LastFrame.mvKeys[i].octave;
      I.angle[i] = LastFrame.mvKeys[i].angle;
    }
    const orbx_proj_camera cam = proj_camera(CurrentFrame, twc);
    const orbx_proj_params prm = {th, 0.0f, bForward ? ORBX_LEVEL_RULE_FORWARD
                                            : bBackward ? ORBX_LEVEL_RULE_BACKWARD : ORBX_LEVEL_RULE_NEITHER};
    int nLive = 0;
    I.project(2, cam, prm, &nLive, "SearchByProjection");
    return I.search(2, CurrentFrame, LastFrame.mvpMapPoints, mfNNratio, TH_HIGH, mbCheckOrientation);
  }

  // SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, th, ORBdist)
  // (:820-894); row i is pKF->GetMapPointMatches()[i].
  template <class FR, class KF, class MP>
  int SearchByProjection(FR& CurrentFrame, KF* pKF, const std::set<MP*>& sAlreadyFound, const float th,
                         const int ORBdist) {
    const auto Rcw = CurrentFrame.mTcw.rowRange(0, 3).colRange(0, 3);
    const auto tcw = CurrentFrame.mTcw.rowRange(0, 3).col(3);
    const auto Ow = -Rcw.t() * tcw;
    const std::vector<MP*> vpMPs = pKF->GetMapPointMatches();
    const int n = (int)vpMPs.size();
    ProjInputs I(n);
    for (int i = 0; i < n; ++i) {
      MP* pMP = vpMPs[i];
      I.skip[i] = !pMP || pMP->isBad() || sAlreadyFound.count(pMP);
      if (I.skip[i]) continue;
      I.set_pos(i, pMP->GetWorldPos());
      I.set_desc(i, pMP->GetDescriptor());
      I.draw[i] = pMP->GetMaxDistance();
      I.angle[i] = pKF->mvKeys[i].angle;
    }
    const orbx_proj_camera cam = proj_camera(CurrentFrame, Ow);
    const orbx_proj_params prm = {th, 0.0f, ORBX_LEVEL_RULE_NEITHER};
    int nLive = 0;
    I.project(3, cam, prm, &nLive, "SearchByProjection");
    return I.search(3, CurrentFrame, vpMPs, mfNNratio, ORBdist, mbCheckOrientation);
  }

 protected:
  // orbx_proj_camera of a Frame; Ow = mOw (mode 1) or twc (modes 2, 3)
  template <class FR, class M>
  static orbx_proj_camera proj_camera(const FR& F, const M& Ow) {
    orbx_proj_camera c;
    memset(&c, 0, sizeof c);
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) c.Rcw[3 * r + k] = F.mTcw.template at<float>(r, k);
      c.tcw[r] = F.mTcw.template at<float>(r, 3);
      c.ow[r] = Ow.template at<float>(r);
    }
    c.fx = F.fx;
    c.fy = F.fy;
    c.cx = F.cx;
    c.cy = F.cy;
    c.mbf = F.mbf;
    c.min_x = F.mnMinX;
    c.max_x = F.mnMaxX;
    c.min_y = F.mnMinY;
    c.max_y = F.mnMaxY;
    c.nlevels = F.mnScaleLevels;
    if (c.nlevels < 1 || c.nlevels > ORBX_PROJ_MAX_LEVELS || (int)F.mvScaleFactors.size() < c.nlevels)
      orbx_throw(ORBX_ERR_ARG, "projection camera");
    for (int l = 0; l < c.nlevels; ++l) c.scale_factors[l] = F.mvScaleFactors[l];
    c.log_scale_factor = F.mfLogScaleFactor;
    return c;
  }

  // the point arrays of one orbm_project_points problem, its rows, and the
  // search over them
  struct ProjInputs {
    int n;
    std::vector<float> pos, normal, dmin, dmax, draw, angle, vcos;
    std::vector<int32_t> octave, level;
    std::vector<uint8_t> skip, qdesc;
    std::vector<orbx_query_proj> q;
    explicit ProjInputs(int n_)
        : n(n_), pos(3 * (size_t)n_), normal(3 * (size_t)n_), dmin(n_), dmax(n_), draw(n_), angle(n_),
          vcos(n_ ? n_ : 1), octave(n_), level(n_ ? n_ : 1, -1), skip(n_), qdesc(32 * (size_t)n_),
          q(n_ ? n_ : 1) {}
    template <class M>
    void set_pos(int i, const M& P) {
      for (int k = 0; k < 3; ++k) pos[3 * (size_t)i + k] = P.template at<float>(k);
    }
    template <class M>
    void set_desc(int i, const M& d) { memcpy(&qdesc[32 * (size_t)i], d.ptr(0), 32); }
    void project(int mode, const orbx_proj_camera& cam, const orbx_proj_params& prm, int* nlive, const char* what) {
      const orbx_proj_points P = {pos.data(), normal.data(), dmin.data(), dmax.data(), draw.data(),
                                  octave.data(), angle.data(), skip.data()};
      orbx_throw(orbm_project_points(mode, 1, &cam, &P, &n, &prm, 0, q.data(), level.data(), vcos.data(), nlive),
                 what);
    }
    // F.mvpMapPoints[idx] = who[row] for every feature a row took
    template <class FR, class MPV>
    int search(int mode, FR& F, const MPV& who, float nnratio, int th_dist, bool check_ori) {
      std::vector<uint8_t> occ(F.N > 0 ? F.N : 0);
      for (int i = 0; i < F.N; ++i) occ[i] = F.mvpMapPoints[i] != nullptr;
      orbx_proj_frame pf;
      pf.n = F.N;
      pf.keys = reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data());
      pf.desc = F.mDescriptors.data;
      pf.uright = nullptr;
      pf.occupied = occ.data();
      pf.min_x = F.mnMinX;
      pf.min_y = F.mnMinY;
      pf.grid_w_inv = F.mfGridElementWidthInv;
      pf.grid_h_inv = F.mfGridElementHeightInv;
      std::vector<int32_t> m(F.N > 0 ? F.N : 1, -1);
      int nm = 0;
      orbx_throw(orbm_search_by_projection(mode, &pf, q.data(), qdesc.data(), n, nnratio, th_dist,
                                           check_ori ? 1 : 0, 0, m.data(), &nm),
                 "SearchByProjection");
      for (int i = 0; i < F.N; ++i)
        if (m[i] >= 0) F.mvpMapPoints[i] = who[m[i]];
      return nm;
    }
  };

  template <class FR>
  static orbx_kf_frame init_frame(FR& F) {
    orbx_kf_frame f;
    f.n = (int)F.mvKeysUn.size();
    f.keys = reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data());
    f.desc = F.mDescriptors.data;
    f.min_x = F.mnMinX;
    f.min_y = F.mnMinY;
    f.grid_w_inv = F.mfGridElementWidthInv;
    f.grid_h_inv = F.mfGridElementHeightInv;
    return f;
  }
  template <class FR>
  static orbx_init_pair init_pair(FR& F1, FR& F2, std::vector<cv::Point2f>& vbPrevMatched,
                                  std::vector<int>& vnMatches12) {
    static_assert(sizeof(cv::Point2f) == 2 * sizeof(float) && sizeof(int) == sizeof(int32_t) &&
                      sizeof(cv::KeyPoint) == sizeof(orbx_keypoint),
                  "vbPrevMatched / vnMatches12 / mvKeysUn are handed over in place");
    vnMatches12.resize(F1.mvKeysUn.size(), -1);  // :199
    // the reference indexes vbPrevMatched[i1] unchecked
    if (vbPrevMatched.size() < F1.mvKeysUn.size()) orbx_throw(ORBX_ERR_ARG, "SearchForInitialization");
    orbx_init_pair P;
    P.f1 = init_frame(F1);
    P.f2 = init_frame(F2);
    P.prev_matched = reinterpret_cast<float*>(vbPrevMatched.data());
    P.match12 = reinterpret_cast<int32_t*>(vnMatches12.data());
    return P;
  }

  // the queries of one orbm_keyframe_search call: begin(KF) .. add(..)* ..
  // end() per problem, then run()
  struct KfSearch {
    std::vector<orbx_kf_frame> frames;
    std::vector<orbx_kf_query> q;
    std::vector<int32_t> qoff = std::vector<int32_t>(1, 0);
    std::vector<uint8_t> pool;
    std::map<const void*, int32_t> row;  // map point -> its pool row
    std::vector<int32_t> best_idx, best_dist;

    template <class KF>
    void begin(KF* kf) {
      orbx_kf_frame f;
      f.n = kf->N;
      f.keys = reinterpret_cast<const orbx_keypoint*>(kf->mvKeysUn.data());
      f.desc = kf->mDescriptors.data;
      f.min_x = kf->mnMinX;
      f.min_y = kf->mnMinY;
      f.grid_w_inv = kf->mfGridElementWidthInv;
      f.grid_h_inv = kf->mfGridElementHeightInv;
      frames.push_back(f);
    }
    void end() { qoff.push_back((int32_t)q.size()); }
    // returns the query's index in best_idx / best_dist
    template <class MP>
    int32_t add(MP* pMP, float u, float v, float radius, int level) {
      std::map<const void*, int32_t>::iterator it = row.find(pMP);
      if (it == row.end()) {
        const cv::Mat d = pMP->GetDescriptor();
        it = row.insert(std::make_pair((const void*)pMP, (int32_t)(pool.size() / 32))).first;
        pool.insert(pool.end(), d.ptr(0), d.ptr(0) + 32);
      }
      orbx_kf_query Q = {u, v, radius, level, it->second};
      q.push_back(Q);
      return (int32_t)q.size() - 1;
    }
    void run(const char* what) {
      best_idx.assign(q.size() ? q.size() : 1, -1);
      best_dist.assign(q.size() ? q.size() : 1, 0x7FFFFFFF);
      orbx_throw(orbm_keyframe_search((int)frames.size(), frames.data(), q.data(), qoff.data(), pool.data(),
                                      (int)(pool.size() / 32), 0, best_idx.data(), best_dist.data()),
                 what);
    }
  };

  // MapPoint::GetMaxDistance(): a member, else a free function found by
  // argument-dependent lookup; a map point type with neither cannot take the
  // device route
  struct Rank0 {};
  struct Rank1 : Rank0 {};
  struct Rank2 : Rank1 {};
  template <class MP>
  static auto max_distance(MP* p, Rank2) -> decltype((float)p->GetMaxDistance()) {
    return p->GetMaxDistance();
  }
  template <class MP>
  static auto max_distance(MP* p, Rank1) -> decltype((float)GetMaxDistance(p)) {
    return GetMaxDistance(p);
  }
  template <class MP>
  static float max_distance(MP*, Rank0) {
    orbx_throw(ORBX_ERR_UNSUPPORTED, "KfProjection::Device needs MapPoint::GetMaxDistance()");
    return 0.0f;
  }

  // orbx_kf_camera: intrinsics of pKFi, bounds and scale tables of pKFs (the
  // searched keyframe), the pose from the caller's matrices
  template <class KF, class M1, class M2, class M3>
  static orbx_kf_camera kf_camera(KF* pKFi, KF* pKFs, const M1& Rcw, const M2& tcw, const M3& Ow) {
    orbx_kf_camera c;
    memset(&c, 0, sizeof c);
    const cv::Mat R = Rcw, t = tcw, O = Ow;
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) c.Rcw[3 * r + k] = R.template at<float>(r, k);
      c.tcw[r] = t.template at<float>(r);
      c.ow[r] = O.template at<float>(r);
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
    if (c.nlevels < 1 || c.nlevels > ORBX_PROJ_MAX_LEVELS || (int)pKFs->mvScaleFactors.size() < c.nlevels)
      orbx_throw(ORBX_ERR_ARG, "keyframe projection camera");
    for (int l = 0; l < c.nlevels; ++l) c.scale_factors[l] = pKFs->mvScaleFactors[l];
    c.log_scale_factor = pKFs->mfLogScaleFactor;
    return c;
  }

  // the device route's inputs: one point set (row i = the list's entry i, its
  // descriptor pool row i) shared by every problem, and per problem a camera
  // and a skip array.  run() projects, hands the rows to KfSearch unchanged and
  // fills slot[p * n + i] = the query's index, -1 for an inert row
  struct KfPoints {
    int n;
    std::vector<float> pos, dmin, dmax, draw;
    std::vector<uint8_t> pool;
    std::vector<orbx_kf_camera> cams;
    std::vector<std::vector<uint8_t> > skips;
    template <class MP>
    explicit KfPoints(const std::vector<MP*>& v)
        : n((int)v.size()), pos(3 * v.size()), dmin(v.size()), dmax(v.size()), draw(v.size()),
          pool(32 * v.size()) {
      for (int i = 0; i < n; ++i) {
        MP* pMP = v[i];
        if (!pMP || pMP->isBad()) continue;  // skipped in every problem
        const cv::Mat P = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) pos[3 * (size_t)i + k] = P.template at<float>(k);
        dmin[i] = pMP->GetMinDistanceInvariance();
        dmax[i] = pMP->GetMaxDistanceInvariance();
        draw[i] = max_distance(pMP, Rank2());
        const cv::Mat d = pMP->GetDescriptor();
        memcpy(&pool[32 * (size_t)i], d.ptr(0), 32);
      }
    }
    template <class KF>
    std::vector<uint8_t>& begin(KfSearch& S, KF* kf, const orbx_kf_camera& cam) {
      S.begin(kf);
      cams.push_back(cam);
      skips.push_back(std::vector<uint8_t>((size_t)n, 1));
      return skips.back();
    }
    void run(KfSearch& S, int form, float th, std::vector<int32_t>& slot, const char* what) {
      const size_t K = cams.size(), total = K * (size_t)n;
      std::vector<orbx_kf_points> P(K);
      std::vector<int> npts(K, n), nlive(K ? K : 1, 0);
      std::vector<int32_t> base(K, 0), level(total ? total : 1, -1);
      for (size_t p = 0; p < K; ++p) {
        const orbx_kf_points one = {pos.data(), dmin.data(), dmax.data(), draw.data(), skips[p].data()};
        P[p] = one;
      }
      S.q.assign(total ? total : 1, orbx_kf_query());
      orbx_throw(orbm_keyframe_project(form, (int)K, cams.data(), P.data(), npts.data(), base.data(), th, 0,
                                       S.q.data(), level.data(), nlive.data()),
                 what);
      S.q.resize(total);
      S.qoff.assign(1, 0);
      for (size_t p = 0; p < K; ++p) S.qoff.push_back((int32_t)((p + 1) * (size_t)n));
      S.pool = pool;
      for (size_t j = 0; j < total; ++j) slot[j] = level[j] >= 0 ? (int32_t)j : -1;
      S.run(what);
    }
  };

  // the projection statements both Fuse forms share (:514-531, :582-599);
  // -1 where the reference `continue`s
  template <class KF, class MP, class M>
  static int32_t fuse_query(KfSearch& S, KF* pKF, const M& Rcw, const M& tcw, const M& Ow, MP* pMP, float th) {
    M p3Dw = pMP->GetWorldPos();
    M p3Dc = Rcw * p3Dw + tcw;
    if (p3Dc.template at<float>(2) < 0.0f) return -1;
    float invz = 1.0 / p3Dc.template at<float>(2);
    float x = p3Dc.template at<float>(0) * invz;
    float y = p3Dc.template at<float>(1) * invz;
    float u = pKF->fx * x + pKF->cx;
    float v = pKF->fy * y + pKF->cy;
    if (!pKF->IsInImage(u, v)) return -1;
    float dist = cv::norm(p3Dw - Ow);
    if (dist < pMP->GetMinDistanceInvariance() || dist > pMP->GetMaxDistanceInvariance()) return -1;
    int level = pMP->PredictScale(dist, pKF);
    float radius = th * pKF->mvScaleFactors[level];
    return S.add(pMP, u, v, radius, level);
  }

  struct Flat {
    orbx_bow_frame f;
    std::vector<uint8_t> valid;
    std::vector<float> angle;
    std::vector<uint32_t> ids, off, feat;
  };
  template <class KF, class MP>
  static void flatten(KF* kf, const std::vector<MP*>& mps, Flat& o) {
    o.valid.resize(mps.size());
    for (size_t i = 0; i < mps.size(); ++i) o.valid[i] = mps[i] && !mps[i]->isBad();
    o.angle.resize(kf->mvKeysUn.size());
    for (size_t i = 0; i < kf->mvKeysUn.size(); ++i) o.angle[i] = kf->mvKeysUn[i].angle;
    o.off.push_back(0);
    for (const auto& node : kf->mFeatVec) {  // std::map: ascending NodeId
      o.ids.push_back(node.first);
      o.feat.insert(o.feat.end(), node.second.begin(), node.second.end());
      o.off.push_back((uint32_t)o.feat.size());
    }
    o.f.n = (int)mps.size();
    o.f.desc = kf->mDescriptors.data;
    o.f.angle = o.angle.data();
    o.f.valid = o.valid.data();
    o.f.nnodes = (int)o.ids.size();
    o.f.node_id = o.ids.data();
    o.f.node_off = o.off.data();
    o.f.feat = o.feat.data();
  }

  template <class FR>
  static void flatten_frame(FR& F, Flat& o) {
    o.angle.resize(F.mvKeys.size());
    for (size_t i = 0; i < F.mvKeys.size(); ++i) o.angle[i] = F.mvKeys[i].angle;
    o.off.push_back(0);
    for (const auto& node : F.mFeatVec) {  // std::map: ascending NodeId
      o.ids.push_back(node.first);
      o.feat.insert(o.feat.end(), node.second.begin(), node.second.end());
      o.off.push_back((uint32_t)o.feat.size());
    }
    o.f.n = F.N;
    o.f.desc = F.mDescriptors.data;
    o.f.angle = o.angle.data();
    o.f.valid = nullptr;
    o.f.nnodes = (int)o.ids.size();
    o.f.node_id = o.ids.data();
    o.f.node_off = o.off.data();
    o.f.feat = o.feat.data();
  }

  struct TriFlat {
    orbx_tri_frame f;
    std::vector<uint8_t> mp;
    std::vector<uint32_t> ids, off, feat;
  };
  template <class KF>
  static void flatten_tri(KF* kf, TriFlat& o) {
    o.mp.resize(kf->N > 0 ? (size_t)kf->N : 0);
    for (int i = 0; i < kf->N; ++i) o.mp[i] = kf->GetMapPoint(i) != nullptr;  // no isBad() (:399,409)
    o.off.push_back(0);
    for (const auto& node : kf->mFeatVec) {  // std::map: ascending NodeId
      o.ids.push_back(node.first);
      o.feat.insert(o.feat.end(), node.second.begin(), node.second.end());
      o.off.push_back((uint32_t)o.feat.size());
    }
    o.f.n = kf->N;
    o.f.keys = reinterpret_cast<const orbx_keypoint*>(kf->mvKeysUn.data());
    o.f.desc = kf->mDescriptors.data;
    o.f.has_mp = o.mp.data();
    o.f.nnodes = (int)o.ids.size();
    o.f.node_id = o.ids.data();
    o.f.node_off = o.off.data();
    o.f.feat = o.feat.data();
    o.f.level_sigma2 = kf->mvLevelSigma2.data();
    o.f.nlevels = (int)kf->mvLevelSigma2.size();
  }

  float mfNNratio;
  bool mbCheckOrientation;
  BowKFFrame mBowKFFrame = BowKFFrame::Stub;
  KfProjection mKfProjection = KfProjection::Host;
};

}  // namespace ORB_SLAM2

// ---------------------------------------------------------------------------
// SURVEY.md §8(f), the callers either side of the path, with the reference's
// own shapes:
//   * DBoW2::BowVector / FeatureVector (Thirdparty/DBoW2/DBoW2/BowVector.h,
//     FeatureVector.h: std::maps keyed by word / node id) and
//     ORB_SLAM2::ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor,
//     FORB>, include/ORBVocabulary.h) with loadFromTextFile / empty /
//     transform(features, BowVector&, FeatureVector&, levelsup), as
//     Frame::ComputeBoW (src/Frame.cc:373-382) and System's loader call them,
//     and size() / score(a, b) as KeyFrameDatabase and LoopClosing::DetectLoop
//     call them (plus a batched score for DetectLoop's whole loop);
//   * ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h) as a template
//     over the caller's KeyFrame and Frame: add / erase / clear,
//     DetectLoopCandidates, DetectRelocalizationCandidates;
//   * Frame::ComputeStereoMatches (src/Frame.cc:446-620) as a template over
//     the caller's Frame, reading and writing exactly the members the
//     reference's member function does.
// ---------------------------------------------------------------------------
#ifndef ORBX_COMPAT_NO_DBOW2
namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;
class BowVector : public std::map<WordId, WordValue> {};
class FeatureVector : public std::map<NodeId, std::vector<unsigned int> > {};
}  // namespace DBoW2
#endif

namespace ORB_SLAM2 {

class ORBVocabulary {
 public:
  ORBVocabulary() {}
  ~ORBVocabulary() { orbv_vocab_destroy(v_); }
  ORBVocabulary(const ORBVocabulary&) = delete;
  ORBVocabulary& operator=(const ORBVocabulary&) = delete;

  // TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1126-1259)
  bool loadFromTextFile(const std::string& filename) {
    orbv_vocab* v = nullptr;
    if (orbv_vocab_load_text(filename.c_str(), 0, &v) != ORBX_OK) return false;
    orbv_vocab_destroy(v_);
    v_ = v;
    return true;
  }
  bool empty() const {
    int nwords = 0;
    return !v_ || orbv_vocab_info(v_, nullptr, nullptr, nullptr, nullptr, nullptr, &nwords) || nwords == 0;
  }
  // transform(features, v, fv, levelsup) (TemplatedVocabulary.h:1338-1424):
  // features = Converter::toDescriptorVector(mDescriptors), one 1 x 32 row each
  void transform(const std::vector<cv::Mat>& features, DBoW2::BowVector& v, DBoW2::FeatureVector& fv,
                 int levelsup) const {
    v.clear();
    fv.clear();
    const int n = (int)features.size();
    if (n == 0) return;
    std::vector<uint8_t> desc((size_t)n * 32);
    for (int i = 0; i < n; ++i) memcpy(desc.data() + (size_t)i * 32, features[i].ptr(0), 32);
    std::vector<uint32_t> word(n), node(n), off(n + 1), feat(n);
    std::vector<double> value(n);
    int nb = 0, nf = 0;
    orbx_throw(orbv_transform(v_, desc.data(), n, levelsup, word.data(), value.data(), &nb, node.data(),
                              off.data(), feat.data(), &nf),
               "ORBVocabulary::transform");
    for (int i = 0; i < nb; ++i) v.insert(v.end(), std::make_pair(word[i], value[i]));
    for (int j = 0; j < nf; ++j)
      fv.insert(fv.end(), std::make_pair(node[j], std::vector<unsigned int>(feat.begin() + off[j],
                                                                              feat.begin() + off[j + 1])));
  }

  // TemplatedVocabulary::size() (:1001-1004): the number of words;
  // KeyFrameDatabase's constructor sizes its inverted file by it
  unsigned int size() const {
    int nwords = 0;
    if (!v_ || orbv_vocab_info(v_, nullptr, nullptr, nullptr, nullptr, nullptr, &nwords)) return 0;
    return (unsigned int)nwords;
  }
  // TemplatedVocabulary::score(a, b) (:1199-1203) with the vocabulary's scoring
  double score(const DBoW2::BowVector& a, const DBoW2::BowVector& b) const {
    std::vector<const DBoW2::BowVector*> one(1, &b);
    std::vector<double> s;
    score(a, one, s);
    return s[0];
  }
  // the same for many b in one call (LoopClosing::DetectLoop's minScore loop,
  // src/LoopClosing.cc:67-74): scores[j] = score(a, *b[j])
  void score(const DBoW2::BowVector& a, const std::vector<const DBoW2::BowVector*>& b,
             std::vector<double>& scores) const {
    std::vector<uint32_t> aw, bw, off(1, 0u);
    std::vector<double> av, bv;
    Flatten(a, aw, av);
    for (const DBoW2::BowVector* p : b) {
      Flatten(*p, bw, bv);
      off.push_back((uint32_t)bw.size());
    }
    scores.assign(b.size(), 0.0);
    orbx_throw(orbv_score(v_, aw.data(), av.data(), (int)aw.size(), off.data(), bw.data(), bv.data(), (int)b.size(),
                          scores.data()),
               "ORBVocabulary::score");
  }

  // appends a BowVector (a std::map: ascending words) to the C ABI's layout
  static void Flatten(const DBoW2::BowVector& v, std::vector<uint32_t>& word, std::vector<double>& value) {
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
      word.push_back(it->first);
      value.push_back(it->second);
    }
  }
  const orbv_vocab* Orbv() const { return v_; }

 private:
  orbv_vocab* v_ = nullptr;
};

// KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) as a
// template over the caller's KeyFrame and Frame classes.  The inverted file
// is the device store behind orbv_db: add / erase / clear keep it, and one
// orbv_db_query per Detect*Candidates call returns what the reference's walk
// over mvInvertedFile collects -- every keyframe sharing a word, in
// lKFsSharingWords' order, with its number of common words and its score
// (the vector form of DetectRelocalizationCandidates: one
// orbv_db_query_batch for all its frames).
// Everything after the walk needs the caller's graph and runs here on that
// list as the reference words it, reading and writing exactly the members the
// reference does: KF::mnId, mBowVec, mnLoopQuery, mnLoopWords, mLoopScore,
// mnRelocQuery, mnRelocWords, mRelocScore, GetConnectedKeyFrames(),
// GetBestCovisibilityKeyFrames(int); FR::mnId, mBowVec.
template <class KF, class FR>
class KeyFrameDatabase {
 public:
  explicit KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc) {
    orbx_throw(orbv_db_create(voc.Orbv(), 0, 0, &db_), "KeyFrameDatabase");
  }
  ~KeyFrameDatabase() { orbv_db_destroy(db_); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  void add(KF* pKF) {  // :20-26
    std::unique_lock<std::mutex> lock(mMutex);
    std::vector<uint32_t> w;
    std::vector<double> v;
    ORBVocabulary::Flatten(pKF->mBowVec, w, v);
    orbx_throw(orbv_db_add(db_, (uint64_t)pKF->mnId, w.data(), v.data(), (int)w.size()), "KeyFrameDatabase::add");
    kfs_[(uint64_t)pKF->mnId] = pKF;
  }
  void erase(KF* pKF) {  // :28-47
    std::unique_lock<std::mutex> lock(mMutex);
    typename std::map<uint64_t, KF*>::iterator it = kfs_.find((uint64_t)pKF->mnId);
    if (it == kfs_.end() || it->second != pKF) return;
    orbx_throw(orbv_db_erase(db_, (uint64_t)pKF->mnId), "KeyFrameDatabase::erase");
    kfs_.erase(it);
  }
  void clear() {  // :49-53
    std::unique_lock<std::mutex> lock(mMutex);
    orbx_throw(orbv_db_clear(db_), "KeyFrameDatabase::clear");
    kfs_.clear();
  }

  // :56-177
  std::vector<KF*> DetectLoopCandidates(KF* pKF, float minScore) {
    std::set<KF*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::list<Sharing> lKFsSharingWords;
    {
      std::unique_lock<std::mutex> lock(mMutex);
      std::vector<Sharing> all;
      Query(pKF->mBowVec, all);
      // the walk's marks, one keyframe's encounters at a time (its marks
      // depend on no other keyframe's)
      for (size_t i = 0; i < all.size(); ++i) {
        KF* pKFi = all[i].kf;
        if (pKFi->mnLoopQuery != pKF->mnId) {
          if (!spConnectedKeyFrames.count(pKFi)) {
            pKFi->mnLoopWords = all[i].ncommon;  // reset at the first encounter, counted at each
            pKFi->mnLoopQuery = pKF->mnId;
            lKFsSharingWords.push_back(all[i]);
          } else {
            pKFi->mnLoopWords = 1;  // never stamped: every encounter resets it, the last leaves 1
          }
        } else {
          pKFi->mnLoopWords += all[i].ncommon;  // stamped by an earlier call with this id
        }
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KF*>();

    std::list<std::pair<float, KF*> > lScoreAndMatch;
    int maxCommonWords = 0;
    for (typename std::list<Sharing>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++)
      if (lit->kf->mnLoopWords > maxCommonWords) maxCommonWords = lit->kf->mnLoopWords;
    int minCommonWords = maxCommonWords * 0.8f;

    for (typename std::list<Sharing>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
      KF* pKFi = lit->kf;
      if (pKFi->mnLoopWords > minCommonWords) {
        float si = lit->score;
        pKFi->mLoopScore = si;
        if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KF*>();

    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = minScore;
    for (typename std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin();
         it != lScoreAndMatch.end(); it++) {
      KF* pKFi = it->second;
      std::vector<KF*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = it->first;
      KF* pBestKF = pKFi;
      for (typename std::vector<KF*>::iterator vit = vpNeighs.begin(); vit != vpNeighs.end(); vit++) {
        KF* pKF2 = *vit;
        if (pKF2->mnLoopQuery == pKF->mnId && pKF2->mnLoopWords > minCommonWords) {
          accScore += pKF2->mLoopScore;
          if (pKF2->mLoopScore > bestScore) {
            pBestKF = pKF2;
            bestScore = pKF2->mLoopScore;
          }
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    return Retain(lAccScoreAndMatch, 0.75f * bestAccScore);
  }

  // :179-289
  std::vector<KF*> DetectRelocalizationCandidates(FR* F) {
    std::vector<Sharing> all;
    {
      std::unique_lock<std::mutex> lock(mMutex);
      Query(F->mBowVec, all);
    }
    return RelocalizationCandidates(F, all);
  }

  // The same for a batch of lost frames (a relocalisation sweep): one ungated
  // orbv_db_query_batch for all of them, then the host step frame after frame
  // in list order.  This equals calling the single form on vpF[0], vpF[1],
  // ... in turn: the search reads none of the members the host step writes
  // (mnRelocQuery, mnRelocWords, mRelocScore), so every frame's list is the
  // one its own call would have fetched -- provided no keyframe is added or
  // erased while the call runs, which the single calls would have seen
  // between frames.  The list is fetched ungated: the host step stamps
  // mnRelocQuery / mnRelocWords on every sharing keyframe, the ones under the
  // word gate included, and a later frame's accumulation reads them.
  std::vector<std::vector<KF*> > DetectRelocalizationCandidates(const std::vector<FR*>& vpF) {
    std::vector<std::vector<Sharing> > all;
    {
      std::unique_lock<std::mutex> lock(mMutex);
      std::vector<const DBoW2::BowVector*> bows;
      for (size_t f = 0; f < vpF.size(); ++f) bows.push_back(&vpF[f]->mBowVec);
      QueryBatch(bows, all);
    }
    std::vector<std::vector<KF*> > vvpCandidates;
    vvpCandidates.reserve(vpF.size());
    for (size_t f = 0; f < vpF.size(); ++f) vvpCandidates.push_back(RelocalizationCandidates(vpF[f], all[f]));
    return vvpCandidates;
  }

 protected:
  struct Sharing {
    KF* kf;
    int ncommon;
    double score;
  };

  // :181-289 on the walk's result `all`
  std::vector<KF*> RelocalizationCandidates(FR* F, const std::vector<Sharing>& all) {
    std::list<Sharing> lKFsSharingWords;
    {
      std::unique_lock<std::mutex> lock(mMutex);
      for (size_t i = 0; i < all.size(); ++i) {
        KF* pKFi = all[i].kf;
        if (pKFi->mnRelocQuery != F->mnId) {
          pKFi->mnRelocWords = all[i].ncommon;
          pKFi->mnRelocQuery = F->mnId;
          lKFsSharingWords.push_back(all[i]);
        } else {
          pKFi->mnRelocWords += all[i].ncommon;
        }
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KF*>();

    int maxCommonWords = 0;
    for (typename std::list<Sharing>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++)
      if (lit->kf->mnRelocWords > maxCommonWords) maxCommonWords = lit->kf->mnRelocWords;
    int minCommonWords = maxCommonWords * 0.8f;

    std::list<std::pair<float, KF*> > lScoreAndMatch;
    for (typename std::list<Sharing>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
      KF* pKFi = lit->kf;
      if (pKFi->mnRelocWords > minCommonWords) {
        float si = lit->score;
        pKFi->mRelocScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KF*>();

    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = 0;
    for (typename std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin();
         it != lScoreAndMatch.end(); it++) {
      KF* pKFi = it->second;
      std::vector<KF*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KF* pBestKF = pKFi;
      for (typename std::vector<KF*>::iterator vit = vpNeighs.begin(); vit != vpNeighs.end(); vit++) {
        KF* pKF2 = *vit;
        if (pKF2->mnRelocQuery != F->mnId) continue;
        accScore += pKF2->mRelocScore;  // whatever it holds, also under the word gate
        if (pKF2->mRelocScore > bestScore) {
          pBestKF = pKF2;
          bestScore = pKF2->mRelocScore;
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    return Retain(lAccScoreAndMatch, 0.75f * bestAccScore);
  }

  // every stored keyframe sharing a word with `bow`, in the walk's order
  void Query(const DBoW2::BowVector& bow, std::vector<Sharing>& out) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    ORBVocabulary::Flatten(bow, w, v);
    const size_t cap = kfs_.size();
    std::vector<uint64_t> id(cap);
    std::vector<int32_t> nc(cap);
    std::vector<double> sc(cap);
    int n = 0;
    orbx_throw(orbv_db_query(db_, w.data(), v.data(), (int)w.size(), (int)cap, id.data(), nc.data(), sc.data(), &n),
               "KeyFrameDatabase: query");
    out.clear();
    for (int i = 0; i < n; ++i) {
      Sharing s = {kfs_[id[i]], nc[i], sc[i]};
      out.push_back(s);
    }
  }
  // the same for several BowVectors in one orbv_db_query_batch: out[f] is
  // what Query(*bows[f], ..) gives
  void QueryBatch(const std::vector<const DBoW2::BowVector*>& bows, std::vector<std::vector<Sharing> >& out) {
    std::vector<uint32_t> off(bows.size() + 1, 0u), w;
    std::vector<double> v;
    for (size_t f = 0; f < bows.size(); ++f) {
      ORBVocabulary::Flatten(*bows[f], w, v);
      off[f + 1] = (uint32_t)w.size();
    }
    std::vector<uint32_t> seg(bows.size() + 1, 0u);
    size_t cap = kfs_.size();  // most frames share with a part of the map; the call says when it needs more
    std::vector<uint64_t> id;
    std::vector<int32_t> nc;
    std::vector<double> sc;
    for (int attempt = 0;; ++attempt) {
      id.resize(cap);
      nc.resize(cap);
      sc.resize(cap);
      const int rc = orbv_db_query_batch(db_, (int)bows.size(), off.data(), w.data(), v.data(), 0, (int)cap, seg.data(),
                                         id.data(), nc.data(), sc.data());
      if (rc == ORBX_ERR_CAPACITY && attempt == 0) {
        cap = seg[bows.size()];
        continue;
      }
      orbx_throw(rc, "KeyFrameDatabase: batched query");
      break;
    }
    out.assign(bows.size(), std::vector<Sharing>());
    for (size_t f = 0; f < bows.size(); ++f)
      for (uint32_t i = seg[f]; i < seg[f + 1]; ++i) {
        Sharing s = {kfs_[id[i]], nc[i], sc[i]};
        out[f].push_back(s);
      }
  }
  // all those with an accumulated score above the bar, each once, first seen first
  static std::vector<KF*> Retain(const std::list<std::pair<float, KF*> >& lAccScoreAndMatch, float minScoreToRetain) {
    std::set<KF*> spAlreadyAddedKF;
    std::vector<KF*> vpCandidates;
    vpCandidates.reserve(lAccScoreAndMatch.size());
    for (typename std::list<std::pair<float, KF*> >::const_iterator it = lAccScoreAndMatch.begin();
         it != lAccScoreAndMatch.end(); it++) {
      if (it->first > minScoreToRetain) {
        KF* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    }
    return vpCandidates;
  }

  const ORBVocabulary* mpVoc;
  orbv_db* db_ = nullptr;
  std::map<uint64_t, KF*> kfs_;  // mnId -> keyframe, for the ids the store returns
  std::mutex mMutex;
};

// Frame::ComputeStereoMatches (src/Frame.cc:446-620) for a stereo Frame whose
// two extractors just ran on its images (their pyramids stay on the device
// for the search).  FR: the reference's Frame -- reads N, mvKeys, mvKeysRight,
// mDescriptors, mDescriptorsRight, mb, mbf, mpORBextractorLeft / Right;
// writes mvuRight / mvDepth (-1 where no match survives, :448-449).
template <class FR>
void ComputeStereoMatches(FR& F) {
  F.mvuRight = std::vector<float>(F.N, -1.0f);
  F.mvDepth = std::vector<float>(F.N, -1.0f);
  int kept = 0;
  orbx_throw(orbx_stereo_match(F.mpORBextractorLeft->Orbx(), F.mpORBextractorRight->Orbx(),
                               reinterpret_cast<const orbx_keypoint*>(F.mvKeys.data()), F.mDescriptors.data,
                               (int)F.mvKeys.size(), reinterpret_cast<const orbx_keypoint*>(F.mvKeysRight.data()),
                               F.mDescriptorsRight.data, (int)F.mvKeysRight.size(), F.mb, F.mbf,
                               F.mvuRight.data(), F.mvDepth.data(), &kept),
             "ComputeStereoMatches");
}

// Optimizer::PoseOptimization (src/Optimizer.cc:220-432) on the device
// (orbm_pose_optimization).  FR: the reference's Frame -- reads
// mTcw, N, mvpMapPoints (GetWorldPos()), mvKeysUn, mvuRight, mvInvLevelSigma2,
// fx fy cx cy mbf; writes mvbOutlier of the features with a map point, calls
// SetPose and returns the inlier count.  With fewer than 3 correspondences it
// returns 0 with those flags cleared and the pose as it was.  The batched
// overload runs every frame in one launch.
class Optimizer {
 public:
  template <class FR>
  static int PoseOptimization(FR* pFrame, int device = 0) {
    std::vector<FR*> one(1, pFrame);
    return PoseOptimization(one, device)[0];
  }

  template <class FR>
  static std::vector<int> PoseOptimization(const std::vector<FR*>& vpFrames, int device = 0) {
    const size_t nf = vpFrames.size();
    std::vector<orbx_pose_camera> cams(nf);
    std::vector<orbx_pose_obs> obs(nf);
    std::vector<std::vector<float> > pos(nf);
    std::vector<std::vector<uint8_t> > has(nf);
    size_t total = 0;
    for (size_t f = 0; f < nf; ++f) {
      FR& F = *vpFrames[f];
      orbx_pose_camera& C = cams[f];
      memset(&C, 0, sizeof(C));
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) C.Tcw[4 * r + c] = F.mTcw.template at<float>(r, c);
      C.fx = F.fx;
      C.fy = F.fy;
      C.cx = F.cx;
      C.cy = F.cy;
      C.mbf = F.mbf;
      C.nlevels = (int)F.mvInvLevelSigma2.size();
      if (C.nlevels < 1 || C.nlevels > ORBX_PROJ_MAX_LEVELS) orbx_throw(ORBX_ERR_ARG, "PoseOptimization");
      for (int l = 0; l < C.nlevels; ++l) C.inv_level_sigma2[l] = F.mvInvLevelSigma2[l];
      const int N = F.N;
      pos[f].assign((size_t)N * 3, 0.0f);
      has[f].assign((size_t)N, 0);
      for (int i = 0; i < N; ++i) {
        auto* pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        const cv::Mat Xw = pMP->GetWorldPos();
        for (int c = 0; c < 3; ++c) pos[f][3 * (size_t)i + c] = Xw.template at<float>(c);
        has[f][i] = 1;
      }
      orbx_pose_obs& O = obs[f];
      memset(&O, 0, sizeof(O));
      O.n = N;
      O.keys = reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data());
      O.uright = F.mvuRight.data();
      O.pos = pos[f].data();
      O.has_point = has[f].data();
      O.npos = N;
      total += (size_t)N;
    }
    std::vector<float> T(nf * 16);
    std::vector<uint8_t> outlier(total ? total : 1);
    std::vector<int> ninliers(nf);
    orbx_throw(orbm_pose_optimization((int)nf, cams.data(), obs.data(), device, T.data(), outlier.data(),
                                      ninliers.data()),
               "PoseOptimization");
    size_t off = 0;
    for (size_t f = 0; f < nf; ++f) {
      FR& F = *vpFrames[f];
      int ncorr = 0;
      for (int i = 0; i < F.N; ++i)
        if (has[f][i]) {
          F.mvbOutlier[i] = outlier[off + i] != 0;
          ++ncorr;
        }
      off += (size_t)F.N;
      if (ncorr < 3) continue;  // Optimizer.cc:345-346: the pose is not written
      cv::Mat pose(4, 4, CV_32F);
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) pose.at<float>(r, c) = T[16 * f + 4 * r + c];
      F.SetPose(pose);
    }
    return ninliers;
  }
};

// Initializer (include/Initializer.h, src/Initializer.cc) on the device
// (orbm_initializer_ransac, orbm_initializer_reconstruct):
// the reference's constructor, the match list and index draw of Initialize
// (:19-63, SetMatches here), FindHomography / FindFundamental, ReconstructH /
// ReconstructF and Initialize with the reference's signatures, and a static
// Initialize over several initializers that makes one device call for the
// models and one for the reconstruction of all of them.  One device call
// computes both models; the two Find* members share its result, so the
// reference's two threads (:68-71) may call them concurrently.  FR: the
// reference's Frame -- reads mK and mvKeysUn.
class Initializer {
 public:
  typedef std::pair<int, int> Match;

  template <class FR>
  Initializer(const FR& ReferenceFrame, float sigma = 1.0, int iterations = 200) {
    mK = ReferenceFrame.mK.clone();
    mvKeys1 = ReferenceFrame.mvKeysUn;
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
  }

  // DUtils::Random::SeedRandOnce(int) and RandomInt
  // (Thirdparty/DBoW2/DUtils/Random.cpp:38-50): one srand per process
  static void SeedRandOnce(int seed) {
    static bool already_seeded = false;
    if (!already_seeded) {
      srand((unsigned)seed);
      already_seeded = true;
    }
  }
  static int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
  }

  // Initialize :19-63: mvKeys2, mvMatches12, mvbMatched1 and the mvSets draw
  // with rand().  Fewer than 8 matches: the reference's draw runs its index
  // vector empty; here it throws instead
  template <class FR>
  void SetMatches(const FR& CurrentFrame, const std::vector<int>& vMatches12) {
    std::lock_guard<std::mutex> lk(mMutex);
    mbComputed = false;
    mvKeys2 = CurrentFrame.mvKeysUn;
    mvIniMatches.assign(vMatches12.begin(), vMatches12.end());
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.resize(mvKeys1.size());
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
      if (vMatches12[i] >= 0) {
        mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
        mvbMatched1[i] = true;
      } else {
        mvbMatched1[i] = false;
      }
    }
    const int N = (int)mvMatches12.size();
    if (N < 8) orbx_throw(ORBX_ERR_ARG, "Initializer: fewer than 8 matches");
    std::vector<size_t> vAllIndices;
    vAllIndices.reserve(N);
    std::vector<size_t> vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    mvSets = std::vector<std::vector<size_t> >(mMaxIterations, std::vector<size_t>(8, 0));
    SeedRandOnce(0);
    for (int it = 0; it < mMaxIterations; it++) {
      vAvailableIndices = vAllIndices;
      for (size_t j = 0; j < 8; j++) {
        const int randi = RandomInt(0, (int)vAvailableIndices.size() - 1);
        const int idx = (int)vAvailableIndices[randi];
        mvSets[it][j] = idx;
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
  }

  // :80-122 and :126-167.  With no hypothesis scoring above 0 the matrix is
  // left as it was, as the reference leaves it
  void FindHomography(std::vector<bool>& vbMatchesInliers, float& score, cv::Mat& H21, int device = 0) {
    Compute(device);
    Report(mResult.H21, mResult.SH, mResult.it_H, mvInliersH, vbMatchesInliers, score, H21);
  }
  void FindFundamental(std::vector<bool>& vbMatchesInliers, float& score, cv::Mat& F21, int device = 0) {
    Compute(device);
    Report(mResult.F21, mResult.SF, mResult.it_F, mvInliersF, vbMatchesInliers, score, F21);
  }
  // SH / (SH + SF) of :72 and the whole result record
  float RH(int device = 0) {
    Compute(device);
    return mResult.RH;
  }
  const orbx_ransac_result& Result(int device = 0) {
    Compute(device);
    return mResult;
  }

  // Both models of several initializers (each after its SetMatches) in one
  // device call; their Find* members then only report.  All must share sigma
  // and the iteration count
  static void FindModels(const std::vector<Initializer*>& vpInit, int device = 0) {
    const size_t n = vpInit.size();
    if (n == 0) return;
    std::vector<std::unique_lock<std::mutex> > locks;
    for (Initializer* I : vpInit) locks.emplace_back(I->mMutex);
    std::vector<orbx_ransac_pair> pairs(n);
    std::vector<std::vector<int32_t> > sets(n);
    std::vector<int32_t> off(n + 1, 0);
    const int nit = vpInit[0]->mMaxIterations;
    const float sigma = vpInit[0]->mSigma;
    for (size_t p = 0; p < n; ++p) {
      Initializer& I = *vpInit[p];
      if (I.mMaxIterations != nit || I.mSigma != sigma || (int)I.mvSets.size() != nit ||
          I.mvIniMatches.size() != I.mvKeys1.size())
        orbx_throw(ORBX_ERR_ARG, "Initializer::FindModels");
      sets[p].reserve((size_t)nit * 8);
      for (const std::vector<size_t>& s : I.mvSets)
        for (size_t v : s) sets[p].push_back((int32_t)v);
      pairs[p].n1 = (int)I.mvKeys1.size();
      pairs[p].n2 = (int)I.mvKeys2.size();
      pairs[p].keys1 = reinterpret_cast<const orbx_keypoint*>(I.mvKeys1.data());
      pairs[p].keys2 = reinterpret_cast<const orbx_keypoint*>(I.mvKeys2.data());
      pairs[p].match12 = I.mvIniMatches.data();
      pairs[p].sets = sets[p].data();
      off[p + 1] = off[p] + (int32_t)I.mvMatches12.size();
    }
    std::vector<orbx_ransac_result> res(n);
    std::vector<uint8_t> inlH((size_t)off[n] + 1), inlF((size_t)off[n] + 1);
    orbx_throw(orbm_initializer_ransac((int)n, pairs.data(), nit, sigma, device, res.data(), inlH.data(),
                                       inlF.data(), off.data()),
               "Initializer::FindModels");
    for (size_t p = 0; p < n; ++p) {
      Initializer& I = *vpInit[p];
      I.mResult = res[p];
      I.mvInliersH.assign(inlH.begin() + off[p], inlH.begin() + off[p + 1]);
      I.mvInliersF.assign(inlF.begin() + off[p], inlF.begin() + off[p + 1]);
      I.mbComputed = true;
    }
  }

  // :406-490 and :493-651 on the matches of the last SetMatches.  On false R21
  // and t21 are released (ReconstructF's :436-437; ReconstructH leaves them in
  // the reference, where Initialize hands in fresh matrices) and vP3D /
  // vbTriangulated are left as they were
  bool ReconstructF(std::vector<bool>& vbMatchesInliers, cv::Mat& F21, cv::Mat& K, cv::Mat& R21, cv::Mat& t21,
                    std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated, float minParallax,
                    int minTriangulated, int device = 0) {
    return ReconstructOne(ORBX_RECON_F, vbMatchesInliers, F21, K, R21, t21, vP3D, vbTriangulated, minParallax,
                          minTriangulated, device);
  }
  bool ReconstructH(std::vector<bool>& vbMatchesInliers, cv::Mat& H21, cv::Mat& K, cv::Mat& R21, cv::Mat& t21,
                    std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated, float minParallax,
                    int minTriangulated, int device = 0) {
    return ReconstructOne(ORBX_RECON_H, vbMatchesInliers, H21, K, R21, t21, vP3D, vbTriangulated, minParallax,
                          minTriangulated, device);
  }

  // :16-77: SetMatches, both models, the choice of :73 and the reconstruction
  // with minParallax = 1.0 and minTriangulated = 50
  template <class FR>
  bool Initialize(const FR& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                  std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated, int device = 0) {
    std::vector<cv::Mat> vR(1), vt(1);
    std::vector<std::vector<cv::Point3f> > vvP(1);
    std::vector<std::vector<bool> > vvT(1);
    vvP[0].swap(vP3D);
    vvT[0].swap(vbTriangulated);
    const std::vector<bool> ok =
        Initialize(std::vector<Initializer*>(1, this), std::vector<const FR*>(1, &CurrentFrame),
                   std::vector<const std::vector<int>*>(1, &vMatches12), vR, vt, vvP, vvT, device);
    vvP[0].swap(vP3D);
    vvT[0].swap(vbTriangulated);
    R21 = vR[0];
    t21 = vt[0];
    return ok[0];
  }

  // Initialize of several initializers: one orbm_initializer_ransac call and one
  // orbm_initializer_reconstruct call for all of them.  The vectors are resized
  // to vpInit.size(); entry p is written as the single form writes its
  // arguments.  All must share sigma and the iteration count
  template <class FR>
  static std::vector<bool> Initialize(const std::vector<Initializer*>& vpInit, const std::vector<const FR*>& vpFrames,
                                      const std::vector<const std::vector<int>*>& vpMatches12,
                                      std::vector<cv::Mat>& vR21, std::vector<cv::Mat>& vt21,
                                      std::vector<std::vector<cv::Point3f> >& vvP3D,
                                      std::vector<std::vector<bool> >& vvbTriangulated, int device = 0) {
    const size_t n = vpInit.size();
    if (vpFrames.size() != n || vpMatches12.size() != n) orbx_throw(ORBX_ERR_ARG, "Initializer::Initialize");
    vR21.resize(n);
    vt21.resize(n);
    vvP3D.resize(n);
    vvbTriangulated.resize(n);
    if (n == 0) return std::vector<bool>();
    for (size_t p = 0; p < n; ++p) vpInit[p]->SetMatches(*vpFrames[p], *vpMatches12[p]);
    FindModels(vpInit, device);
    std::vector<ReconJob> jobs(n);
    for (size_t p = 0; p < n; ++p) {
      Initializer& I = *vpInit[p];
      std::lock_guard<std::mutex> lk(I.mMutex);
      jobs[p].init = &I;
      jobs[p].model = ORBX_RECON_AUTO;
      jobs[p].ransac = I.mResult;
      jobs[p].inlH = I.mvInliersH;
      jobs[p].inlF = I.mvInliersF;
      MatTo9(I.mK, jobs[p].K);
    }
    Reconstruct(jobs, vpInit[0]->mSigma, 1.0f, 50, device);
    std::vector<bool> ok(n);
    for (size_t p = 0; p < n; ++p) ok[p] = Deliver(jobs[p], vR21[p], vt21[p], vvP3D[p], vvbTriangulated[p]);
    return ok;
  }

  // the record of the last reconstruction through this object (diagnostics)
  const orbx_recon_result& ReconResult() const { return mRecon; }

  // the reference's members (include/Initializer.h:60-80)
  std::vector<cv::KeyPoint> mvKeys1, mvKeys2;
  std::vector<Match> mvMatches12;
  std::vector<bool> mvbMatched1;
  cv::Mat mK;
  float mSigma, mSigma2;
  int mMaxIterations;
  std::vector<std::vector<size_t> > mvSets;

 private:
  void Compute(int device) {
    std::lock_guard<std::mutex> once(mComputeMutex);  // the second of two threads waits, then reports
    {
      std::lock_guard<std::mutex> lk(mMutex);
      if (mbComputed) return;
    }
    FindModels(std::vector<Initializer*>(1, this), device);
  }
  void Report(const float M[9], float S, int it, const std::vector<uint8_t>& inl, std::vector<bool>& vbMatchesInliers,
              float& score, cv::Mat& M21) {
    std::lock_guard<std::mutex> lk(mMutex);
    vbMatchesInliers.assign(inl.size(), false);
    for (size_t i = 0; i < inl.size(); ++i) vbMatchesInliers[i] = inl[i] != 0;
    score = S;
    if (it < 0) return;
    M21.create(3, 3, CV_32F);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) M21.at<float>(r, c) = M[3 * r + c];
  }

  struct ReconJob {
    Initializer* init = nullptr;
    int model = ORBX_RECON_AUTO;
    orbx_ransac_result ransac;
    std::vector<uint8_t> inlH, inlF;
    float K[9];
    orbx_recon_result res;
    std::vector<float> P3D;
    std::vector<uint8_t> tri;
  };
  static void MatTo9(const cv::Mat& M, float out[9]) {
    if (M.rows != 3 || M.cols != 3 || M.type() != CV_32F) orbx_throw(ORBX_ERR_ARG, "Initializer: a 3x3 CV_32F matrix");
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) out[3 * r + c] = M.at<float>(r, c);
  }
  // one device call for all jobs
  static void Reconstruct(std::vector<ReconJob>& jobs, float sigma, float minParallax, int minTriangulated,
                          int device) {
    const size_t n = jobs.size();
    std::vector<orbx_recon_pair> pairs(n);
    std::vector<int32_t> off(n + 1, 0);
    for (size_t p = 0; p < n; ++p) {
      Initializer& I = *jobs[p].init;
      if (I.mSigma != sigma || I.mvIniMatches.size() != I.mvKeys1.size())
        orbx_throw(ORBX_ERR_ARG, "Initializer::Reconstruct");
      orbx_recon_pair& P = pairs[p];
      P.n1 = (int)I.mvKeys1.size();
      P.n2 = (int)I.mvKeys2.size();
      P.keys1 = reinterpret_cast<const orbx_keypoint*>(I.mvKeys1.data());
      P.keys2 = reinterpret_cast<const orbx_keypoint*>(I.mvKeys2.data());
      P.match12 = I.mvIniMatches.data();
      for (int e = 0; e < 9; ++e) P.K[e] = jobs[p].K[e];
      P.model = jobs[p].model;
      P.ransac = &jobs[p].ransac;
      // an empty vector still hands over a pointer: a pair may have no match
      jobs[p].inlH.reserve(1);
      jobs[p].inlF.reserve(1);
      P.inliers_H = jobs[p].model == ORBX_RECON_F ? nullptr : jobs[p].inlH.data();
      P.inliers_F = jobs[p].model == ORBX_RECON_H ? nullptr : jobs[p].inlF.data();
      off[p + 1] = off[p] + P.n1;
    }
    std::vector<orbx_recon_result> res(n);
    std::vector<float> P3D((size_t)off[n] * 3 + 3);
    std::vector<uint8_t> tri((size_t)off[n] + 1);
    orbx_throw(orbm_initializer_reconstruct((int)n, pairs.data(), sigma, minParallax, minTriangulated, device,
                                            res.data(), P3D.data(), tri.data(), off.data()),
               "Initializer::Reconstruct");
    for (size_t p = 0; p < n; ++p) {
      jobs[p].res = res[p];
      jobs[p].P3D.assign(P3D.begin() + 3 * (size_t)off[p], P3D.begin() + 3 * (size_t)off[p + 1]);
      jobs[p].tri.assign(tri.begin() + off[p], tri.begin() + off[p + 1]);
      std::lock_guard<std::mutex> lk(jobs[p].init->mMutex);
      jobs[p].init->mRecon = res[p];
    }
  }
  // the outputs of one job as the reference's Reconstruct* leaves them
  static bool Deliver(const ReconJob& J, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                      std::vector<bool>& vbTriangulated) {
    if (!J.res.ok) {
      R21 = cv::Mat();
      t21 = cv::Mat();
      return false;
    }
    cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R.at<float>(r, c) = J.res.R21[3 * r + c];
      t.at<float>(r, 0) = J.res.t21[r];
    }
    R21 = R;
    t21 = t;
    const size_t n1 = J.tri.size();
    vP3D.resize(n1);
    vbTriangulated.assign(n1, false);
    for (size_t i = 0; i < n1; ++i) {
      vP3D[i] = cv::Point3f(J.P3D[3 * i], J.P3D[3 * i + 1], J.P3D[3 * i + 2]);
      vbTriangulated[i] = J.tri[i] != 0;
    }
    return true;
  }
  bool ReconstructOne(int model, std::vector<bool>& vbMatchesInliers, cv::Mat& M21, cv::Mat& K, cv::Mat& R21,
                      cv::Mat& t21, std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated,
                      float minParallax, int minTriangulated, int device) {
    std::vector<ReconJob> jobs(1);
    ReconJob& J = jobs[0];
    {
      std::lock_guard<std::mutex> lk(mMutex);
      if (vbMatchesInliers.size() != mvMatches12.size()) orbx_throw(ORBX_ERR_ARG, "Initializer: a flag per match");
      J.init = this;
      J.model = model;
      memset(&J.ransac, 0, sizeof J.ransac);
      J.ransac.it_H = J.ransac.it_F = -1;
      J.ransac.nmatch = (int32_t)mvMatches12.size();
      std::vector<uint8_t>& fl = model == ORBX_RECON_H ? J.inlH : J.inlF;
      fl.resize(vbMatchesInliers.size());
      for (size_t i = 0; i < fl.size(); ++i) fl[i] = vbMatchesInliers[i] ? 1 : 0;
      if (!M21.empty()) {  // an empty matrix is the absent model: false without a candidate
        MatTo9(M21, model == ORBX_RECON_H ? J.ransac.H21 : J.ransac.F21);
        (model == ORBX_RECON_H ? J.ransac.it_H : J.ransac.it_F) = 0;
      }
      MatTo9(K, J.K);
    }
    Reconstruct(jobs, mSigma, minParallax, minTriangulated, device);
    return Deliver(J, R21, t21, vP3D, vbTriangulated);
  }

  orbx_recon_result mRecon = orbx_recon_result();
  std::vector<int32_t> mvIniMatches;  // vMatches12 as given: the ABI's match12
  std::mutex mMutex, mComputeMutex;
  bool mbComputed = false;
  orbx_ransac_result mResult;
  std::vector<uint8_t> mvInliersH, mvInliersF;
};

// ---------------------------------------------------------------------------
// Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) over orbm_sim3_solve
// (DESIGN.md §22): the reference's constructor with its filtering (:42-83),
// SetRansacParameters, iterate, find and the three getters with the reference's
// signatures, and a static IterateAll that advances several solvers by one
// device call -- the form for the candidate loop of LoopClosing.cc:167-197.
// KF / MP: the reference's KeyFrame and MapPoint -- reads GetMapPointMatches,
// GetRotation, GetTranslation, mvKeysUn, mvLevelSigma2, mK; isBad,
// GetIndexInKeyFrame, GetWorldPos.
// One deviation: a call draws all its triples from rand() before the device
// evaluates them, so a call that returns a transformation before its last
// iteration has drawn triples the reference would not have; solvers that draw
// later see a different rand() stream.  Each solver's result is the reference's
// for the triples it was given (mvTriples keeps those of the last call).
template <class KF, class MP>
class Sim3Solver {
 public:
  Sim3Solver(KF* pKF1, KF* pKF2, const std::vector<MP*>& vpMatched12, const bool bFixScale = true)
      : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale) {
    mpKF1 = pKF1;
    mpKF2 = pKF2;
    std::vector<MP*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    mvpMapPoints1.reserve(mN1);
    mvpMapPoints2.reserve(mN1);
    mvpMatches12 = vpMatched12;
    mvnIndices1.reserve(mN1);
    ToArray(pKF1->GetRotation(), 3, 3, mP.Rcw1);
    ToArray(pKF1->GetTranslation(), 3, 1, mP.tcw1);
    ToArray(pKF2->GetRotation(), 3, 3, mP.Rcw2);
    ToArray(pKF2->GetTranslation(), 3, 1, mP.tcw2);
    for (int i1 = 0; i1 < mN1; i1++) {
      if (vpMatched12[i1]) {
        MP* pMP1 = vpKeyFrameMP1[i1];
        MP* pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        const cv::KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
        const cv::KeyPoint& kp2 = pKF2->mvKeysUn[indexKF2];
        mvSigma2_1.push_back(pKF1->mvLevelSigma2[kp1.octave]);  // the bounds of :67-68 are the device's
        mvSigma2_2.push_back(pKF2->mvLevelSigma2[kp2.octave]);
        mvpMapPoints1.push_back(pMP1);
        mvpMapPoints2.push_back(pMP2);
        mvnIndices1.push_back(i1);
        float p[3];
        ToArray(pMP1->GetWorldPos(), 3, 1, p);  // mvX3Dc1 / 2 and mvP1im1 / 2 (:75-78, :88-89) are the device's
        mvPos1.insert(mvPos1.end(), p, p + 3);
        ToArray(pMP2->GetWorldPos(), 3, 1, p);
        mvPos2.insert(mvPos2.end(), p, p + 3);
      }
    }
    const cv::Mat K1 = pKF1->mK, K2 = pKF2->mK;
    mP.fx1 = K1.template at<float>(0, 0), mP.fy1 = K1.template at<float>(1, 1);
    mP.cx1 = K1.template at<float>(0, 2), mP.cy1 = K1.template at<float>(1, 2);
    mP.fx2 = K2.template at<float>(0, 0), mP.fy2 = K2.template at<float>(1, 1);
    mP.cx2 = K2.template at<float>(0, 2), mP.cy2 = K2.template at<float>(1, 2);
    SetRansacParameters();
  }

  // :94-118
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    N = (int)mvpMapPoints1.size();
    float epsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N)
      nIterations = 1;
    else
      nIterations = (int)ceil(log(1 - mRansacProb) / log(1 - pow(epsilon, 3)));
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    mnIterations = 0;
  }

  // :120-187
  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, int device = 0) {
    IterateAll(std::vector<Sim3Solver*>(1, this), nIterations, device);
    return Collect(bNoMore, vbInliers, nInliers);
  }

  // :189-193
  cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers, int device = 0) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers, device);
  }

  // nIterations iterations of every listed solver in one device call; the
  // triples are drawn from rand() in list order.  Each solver's Collect then
  // reports what its iterate would have returned
  static void IterateAll(const std::vector<Sim3Solver*>& vpSolvers, int nIterations, int device = 0) {
    const size_t n = vpSolvers.size();
    if (n == 0) return;
    std::vector<orbx_sim3_problem> probs(n);
    std::vector<int32_t> off(n + 1, 0);
    for (size_t p = 0; p < n; ++p) {
      Sim3Solver& S = *vpSolvers[p];
      S.mbHit = false;
      S.mvTriples.clear();
      int k = 0;
      if (S.N >= S.mRansacMinInliers) {  // :126
        if (S.N < 3) orbx_throw(ORBX_ERR_ARG, "Sim3Solver: fewer than 3 correspondences");
        k = std::max(0, std::min(nIterations, S.mRansacMaxIts - S.mnIterations));  // :138
      }
      std::vector<size_t> vAvailableIndices;
      for (int it = 0; it < k; ++it) {  // :143-157
        vAvailableIndices.resize((size_t)S.N);
        for (int i = 0; i < S.N; ++i) vAvailableIndices[i] = (size_t)i;
        for (short i = 0; i < 3; ++i) {
          int randi = Initializer::RandomInt(0, (int)vAvailableIndices.size() - 1);
          S.mvTriples.push_back((int32_t)vAvailableIndices[randi]);
          vAvailableIndices[randi] = vAvailableIndices.back();
          vAvailableIndices.pop_back();
        }
      }
      orbx_sim3_problem& P = probs[p];
      P = S.mP;
      P.ncorr = S.N;
      P.pos1 = S.mvPos1.data(), P.pos2 = S.mvPos2.data();
      P.sigma2_1 = S.mvSigma2_1.data(), P.sigma2_2 = S.mvSigma2_2.data();
      P.nit = k;
      P.triples = S.mvTriples.data();
      P.min_inliers = S.mRansacMinInliers;
      P.fix_scale = S.mbFixScale ? 1 : 0;
      P.best_in = S.mnBestInliers;
      off[p + 1] = off[p] + S.N;
    }
    std::vector<orbx_sim3_result> res(n);
    std::vector<uint8_t> inl((size_t)off[n] + 1);
    orbx_throw(orbm_sim3_solve((int)n, probs.data(), device, res.data(), inl.data(), off.data()), "Sim3Solver::iterate");
    for (size_t p = 0; p < n; ++p) {
      Sim3Solver& S = *vpSolvers[p];
      const orbx_sim3_result& r = res[p];
      S.mnIterations += r.it_hit >= 0 ? r.it_hit + 1 : probs[p].nit;  // :141
      if (r.it_best >= 0) {  // :165-170
        S.mResult = r;
        S.mnBestInliers = r.n_best;
        S.mvbBestInliers.assign(inl.begin() + off[p], inl.begin() + off[p + 1]);
        S.mBestRotation = cv::Mat(3, 3, CV_32F);
        S.mBestTranslation = cv::Mat(3, 1, CV_32F);
        S.mBestT12 = cv::Mat(4, 4, CV_32F);
        S.mBestScale = r.s12;
        for (int i = 0; i < 4; ++i)
          for (int j = 0; j < 4; ++j) S.mBestT12.template at<float>(i, j) = i == j ? 1.0f : 0.0f;
        for (int i = 0; i < 3; ++i) {
          for (int j = 0; j < 3; ++j) {
            S.mBestRotation.template at<float>(i, j) = r.R12[3 * i + j];
            S.mBestT12.template at<float>(i, j) = r.s12 * r.R12[3 * i + j];  // :303
          }
          S.mBestTranslation.template at<float>(i, 0) = r.t12[i];
          S.mBestT12.template at<float>(i, 3) = r.t12[i];
        }
      }
      S.mbHit = r.it_hit >= 0;
    }
  }

  // the outputs of iterate after an IterateAll (:122-130, :172-186)
  cv::Mat Collect(bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (N < mRansacMinInliers) {
      bNoMore = true;
      return cv::Mat();
    }
    if (mbHit) {
      nInliers = mnBestInliers;
      for (int i = 0; i < N; i++)
        if (mvbBestInliers[i]) vbInliers[mvnIndices1[i]] = true;
      return mBestT12;
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return cv::Mat();
  }

  cv::Mat GetEstimatedRotation() { return mBestRotation.clone(); }
  cv::Mat GetEstimatedTranslation() { return mBestTranslation.clone(); }
  float GetEstimatedScale() { return mBestScale; }

  // the record of the iteration the best state comes from: sR21 and t21 are
  // orbx_kf_camera's, for ORBmatcher::SearchBySim3's device form
  const orbx_sim3_result& Result() const { return mResult; }

  // the reference's members (include/Sim3Solver.h:48-97) that survive; the
  // per-correspondence vectors it derives (:75-89) live on the device
  KF* mpKF1;
  KF* mpKF2;
  std::vector<MP*> mvpMapPoints1, mvpMapPoints2, mvpMatches12;
  std::vector<size_t> mvnIndices1;
  int N, mN1;
  std::vector<uint8_t> mvbBestInliers;
  int mnIterations, mnBestInliers;
  cv::Mat mBestT12, mBestRotation, mBestTranslation;
  float mBestScale = 0.0f;
  bool mbFixScale;
  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts;
  std::vector<int32_t> mvTriples;  // the draw of the last call, three indices per iteration

 private:
  static void ToArray(const cv::Mat& M, int rows, int cols, float* out) {
    if (M.rows != rows || M.cols != cols || M.type() != CV_32F) orbx_throw(ORBX_ERR_ARG, "Sim3Solver: a CV_32F matrix");
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) out[r * cols + c] = M.template at<float>(r, c);
  }
  orbx_sim3_problem mP = orbx_sim3_problem();  // the poses and cameras; the rest is filled per call
  orbx_sim3_result mResult = orbx_sim3_result();
  std::vector<float> mvPos1, mvPos2, mvSigma2_1, mvSigma2_2;
  bool mbHit = false;
};

}  // namespace ORB_SLAM2

#endif

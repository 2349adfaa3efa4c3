// ORB_SLAM2::Initializer::Initialize of cpp/orbslam2_compat.hpp over a stand-in
// Frame: single and batched over three initializers against the CPU
// restatements (tests/cpp/initransac_ref.c for the models, initrecon_ref.c for
// the reconstruction) bit for bit, ReconstructH / ReconstructF called directly,
// and the false path leaving vP3D / vbTriangulated as they were.  Needs a GPU.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "orbslam2_compat.hpp"
#include "expect.h"

extern "C" int ir_ref_initialize(int n1, const float* keys1, int n2, const float* keys2, int kstride,
                                 const int32_t* match12, int nit, const int32_t* sets, float sigma, float* H21,
                                 float* F21, float* scores, int32_t* its, uint8_t* inl_H, uint8_t* inl_F,
                                 int32_t* counters, float* hyp, float* it_scores);
extern "C" int rc_ref_reconstruct(int n1, const float* keys1, int n2, const float* keys2, int kstride,
                                  const int32_t* match12, const float* K, int model, int present, const float* M,
                                  const uint8_t* flags, float sigma, float minParallax, int minTriangulated,
                                  int32_t* res, float* P3D, uint8_t* tri, int32_t* counters, float* cand_out,
                                  uint8_t* branches, float* cosv);
extern "C" int rc_ref_choose_model(float RH);

struct Frame {
  cv::Mat mK;
  std::vector<cv::KeyPoint> mvKeysUn;
};

static uint32_t lcg_state = 2468;
static double uni(double a, double b) {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return a + (b - a) * ((lcg_state >> 8) / 16777216.0);
}

// two views of nm points, on an oblique plane or with depth spread, a sixth of
// the matches displaced, with unmatched keys in between
static void make_scene(int nm, bool planar, Frame& F1, Frame& F2, std::vector<int>& match12) {
  const double fx = 500, cx = 320, cy = 240, a = 0.03;
  F1.mK = cv::Mat(3, 3, CV_32F);
  memset(F1.mK.data, 0, 9 * sizeof(float));
  F1.mK.at<float>(0, 0) = F1.mK.at<float>(1, 1) = (float)fx;
  F1.mK.at<float>(0, 2) = (float)cx;
  F1.mK.at<float>(1, 2) = (float)cy;
  F1.mK.at<float>(2, 2) = 1.0f;
  F2.mK = F1.mK.clone();
  F1.mvKeysUn.clear();
  F2.mvKeysUn.clear();
  match12.clear();
  for (int i = 0; i < nm; ++i) {
    const double u = uni(30, 610), v = uni(30, 450);
    const double rx = (u - cx) / fx, ry = (v - cy) / fx;
    // plane (1, 0.1, 1) . X = 5 sqrt(2.01)
    const double z = planar ? 5.0 * sqrt(2.01) / (rx + 0.1 * ry + 1.0) : uni(3, 10);
    const double X = rx * z, Y = ry * z;
    const double X2 = cos(a) * X + sin(a) * z + 0.4, Y2 = Y + 0.05, Z2 = -sin(a) * X + cos(a) * z + 0.02;
    double u2 = fx * X2 / Z2 + cx + uni(-0.3, 0.3), v2 = fx * Y2 / Z2 + cy + uni(-0.3, 0.3);
    if (i % 6 == 5) {
      const double ang = uni(0, 6.283), mag = uni(30, 60);
      u2 += mag * cos(ang), v2 += mag * sin(ang);
    }
    if (i % 3 == 0) {
      F1.mvKeysUn.push_back(cv::KeyPoint((float)uni(0, 640), (float)uni(0, 480), 31.0f));
      match12.push_back(-1);
      F2.mvKeysUn.push_back(cv::KeyPoint((float)uni(0, 640), (float)uni(0, 480), 31.0f));
    }
    F1.mvKeysUn.push_back(cv::KeyPoint((float)(u + uni(-0.3, 0.3)), (float)(v + uni(-0.3, 0.3)), 31.0f));
    match12.push_back((int)F2.mvKeysUn.size());
    F2.mvKeysUn.push_back(cv::KeyPoint((float)u2, (float)v2, 31.0f));
  }
  F2.mvKeysUn.push_back(cv::KeyPoint(1.0f, 2.0f, 31.0f));
}

struct Ref {
  int32_t res[33];
  std::vector<float> P3D;
  std::vector<uint8_t> tri;
  float RH;
};

// Initialize restated: the models, the choice of :73, the reconstruction
static Ref restate(const Frame& F1, const Frame& F2, const std::vector<int>& m12,
                   const std::vector<std::vector<size_t> >& sets, float sigma) {
  Ref r;
  std::vector<int32_t> m(m12.begin(), m12.end()), s;
  for (const auto& v : sets)
    for (size_t x : v) s.push_back((int32_t)x);
  std::vector<uint8_t> inlH(m12.size() + 1, 0), inlF(m12.size() + 1, 0);
  float H[9], F[9], scores[3];
  int32_t its[2];
  const int n1 = (int)F1.mvKeysUn.size(), n2 = (int)F2.mvKeysUn.size();
  const int ks = (int)(sizeof(cv::KeyPoint) / sizeof(float));
  ir_ref_initialize(n1, &F1.mvKeysUn[0].pt.x, n2, &F2.mvKeysUn[0].pt.x, ks, m.data(), (int)sets.size(), s.data(), sigma,
                    H, F, scores, its, inlH.data(), inlF.data(), nullptr, nullptr, nullptr);
  r.RH = scores[2];
  const int model = rc_ref_choose_model(scores[2]);
  float K[9];
  for (int i = 0; i < 9; ++i) K[i] = F1.mK.at<float>(i / 3, i % 3);
  r.P3D.assign((size_t)n1 * 3, 0.0f);
  r.tri.assign((size_t)n1, 0);
  rc_ref_reconstruct(n1, &F1.mvKeysUn[0].pt.x, n2, &F2.mvKeysUn[0].pt.x, ks, m.data(), K, model, its[model] >= 0,
                     model ? F : H, model ? inlF.data() : inlH.data(), sigma, 1.0f, 50, r.res, r.P3D.data(),
                     r.tri.data(), nullptr, nullptr, nullptr, nullptr);
  return r;
}

static bool same_word(float a, float b) { return (a != a && b != b) || memcmp(&a, &b, 4) == 0; }

// the words of R21, t21, the points and the flags that equal the restatement's
static void compare(const char* what, bool ok, const cv::Mat& R21, const cv::Mat& t21,
                    const std::vector<cv::Point3f>& vP3D, const std::vector<bool>& vbTri, const Ref& r,
                    const orbx_recon_result& rec) {
  int words = 0, total = 0, flags = 0;
  const float* rf = reinterpret_cast<const float*>(r.res);
  EXPECT(ok == (r.res[0] != 0));
  EXPECT(memcmp(&rec, r.res, sizeof rec) == 0);  // the whole record, diagnostics included
  if (ok && r.res[0]) {
    EXPECT(R21.rows == 3 && R21.cols == 3 && t21.rows == 3 && t21.cols == 1);
    for (int i = 0; i < 9; ++i) words += same_word(R21.at<float>(i / 3, i % 3), rf[2 + i]);
    for (int i = 0; i < 3; ++i) words += same_word(t21.at<float>(i), rf[11 + i]);
    total = 12;
    EXPECT(vP3D.size() == r.tri.size() && vbTri.size() == r.tri.size());
    for (size_t i = 0; i < r.tri.size() && i < vP3D.size(); ++i) {
      words += same_word(vP3D[i].x, r.P3D[3 * i]) + same_word(vP3D[i].y, r.P3D[3 * i + 1]) +
               same_word(vP3D[i].z, r.P3D[3 * i + 2]);
      flags += vbTri[i] == (r.tri[i] != 0);
      total += 3;
    }
  } else {
    EXPECT(R21.empty() && t21.empty());
  }
  int ntri = 0;
  for (bool b : vbTri) ntri += b;
  printf("%s: ok %d, model %d, %d of %d words, %d of %zu flags, %d triangulated, RH %.4f\n", what, (int)ok, r.res[1],
         words, total, flags, ok ? r.tri.size() : (size_t)0, ok ? ntri : 0, (double)r.RH);
  EXPECT(words == total && (!ok || flags == (int)r.tri.size()));
}

int main() {
  const int sizes[4] = {150, 120, 90, 20};
  const bool planar[4] = {true, false, true, false};
  Frame F1[4], F2[4];
  std::vector<int> m12[4];
  for (int k = 0; k < 4; ++k) make_scene(sizes[k], planar[k], F1[k], F2[k], m12[k]);
  const int nit = 200;

  // single: the planar pair goes through H, the general pair through F
  std::vector<std::unique_ptr<ORB_SLAM2::Initializer> > init;
  Ref refs[4];
  for (int k = 0; k < 2; ++k) {
    init.emplace_back(new ORB_SLAM2::Initializer(F1[k], 1.0f, nit));
    cv::Mat R21, t21;
    std::vector<cv::Point3f> vP3D;
    std::vector<bool> vbTri;
    const bool ok = init[k]->Initialize(F2[k], m12[k], R21, t21, vP3D, vbTri);
    refs[k] = restate(F1[k], F2[k], m12[k], init[k]->mvSets, 1.0f);
    char what[32];
    snprintf(what, sizeof what, "single pair %d", k);
    compare(what, ok, R21, t21, vP3D, vbTri, refs[k], init[k]->ReconResult());
    EXPECT(ok);
    EXPECT(init[k]->ReconResult().model_used == (k == 0 ? ORBX_RECON_H : ORBX_RECON_F));
  }

  // ReconstructH / ReconstructF called as the reference's Initialize calls them
  {
    std::vector<bool> in;
    float S;
    cv::Mat F, R21, t21;
    init[1]->FindFundamental(in, S, F);
    std::vector<cv::Point3f> vP3D;
    std::vector<bool> vbTri;
    const bool ok = init[1]->ReconstructF(in, F, init[1]->mK, R21, t21, vP3D, vbTri, 1.0f, 50);
    compare("ReconstructF pair 1", ok, R21, t21, vP3D, vbTri, refs[1], init[1]->ReconResult());
    cv::Mat H;
    init[0]->FindHomography(in, S, H);
    const bool okh = init[0]->ReconstructH(in, H, init[0]->mK, R21, t21, vP3D, vbTri, 1.0f, 50);
    compare("ReconstructH pair 0", okh, R21, t21, vP3D, vbTri, refs[0], init[0]->ReconResult());
  }

  // batched over three initializers, the last with too few matches to succeed
  {
    std::vector<std::unique_ptr<ORB_SLAM2::Initializer> > b;
    std::vector<ORB_SLAM2::Initializer*> ptrs;
    std::vector<const Frame*> frames;
    std::vector<const std::vector<int>*> matches;
    for (int k = 1; k < 4; ++k) {
      b.emplace_back(new ORB_SLAM2::Initializer(F1[k], 1.0f, nit));
      ptrs.push_back(b.back().get());
      frames.push_back(&F2[k]);
      matches.push_back(&m12[k]);
    }
    std::vector<cv::Mat> vR, vt;
    std::vector<std::vector<cv::Point3f> > vvP(3);
    std::vector<std::vector<bool> > vvT(3);
    vvP[2].assign(7, cv::Point3f(1.5f, 2.5f, 3.5f));  // must survive the false return
    vvT[2].assign(7, true);
    const std::vector<bool> ok = ORB_SLAM2::Initializer::Initialize(ptrs, frames, matches, vR, vt, vvP, vvT);
    EXPECT(ok.size() == 3);
    for (int k = 1; k < 4; ++k) {
      refs[k] = restate(F1[k], F2[k], m12[k], b[k - 1]->mvSets, 1.0f);
      char what[32];
      snprintf(what, sizeof what, "batch pair %d", k);
      compare(what, ok[k - 1], vR[k - 1], vt[k - 1], vvP[k - 1], vvT[k - 1], refs[k], b[k - 1]->ReconResult());
    }
    EXPECT(ok[0] && ok[1] && !ok[2]);
    bool kept = vvP[2].size() == 7 && vvT[2].size() == 7;
    for (size_t i = 0; kept && i < 7; ++i)
      kept = vvP[2][i].x == 1.5f && vvP[2][i].y == 2.5f && vvP[2][i].z == 3.5f && vvT[2][i];
    printf("false path: vP3D and vbTriangulated %s\n", kept ? "untouched" : "CHANGED");
    EXPECT(kept);
  }

  // the single form's false path
  {
    ORB_SLAM2::Initializer I(F1[3], 1.0f, nit);
    cv::Mat R21(3, 3, CV_32F), t21(3, 1, CV_32F);
    std::vector<cv::Point3f> vP3D(5, cv::Point3f(9.0f, 8.0f, 7.0f));
    std::vector<bool> vbTri(5, true);
    const bool ok = I.Initialize(F2[3], m12[3], R21, t21, vP3D, vbTri);
    EXPECT(!ok && R21.empty() && t21.empty() && vP3D.size() == 5 && vP3D[4].x == 9.0f && vbTri.size() == 5 && vbTri[0]);
    EXPECT(I.ReconResult().ok == 0 && I.ReconResult().n_inliers <= 20);
  }
  printf("initrecon_compat_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

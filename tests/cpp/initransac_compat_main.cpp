// ORB_SLAM2::Initializer of cpp/orbslam2_compat.hpp over a stand-in Frame:
// the rand() draw against a restated draw after srand(0), FindHomography /
// FindFundamental against the CPU restatement (tests/cpp/initransac_ref.c) bit
// for bit, and the batched FindModels against the single form.  Needs a GPU.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <thread>
#include <vector>

#include "orbslam2_compat.hpp"
#include "expect.h"

extern "C" int ir_ref_initialize(int n1, const float* keys1, int n2, const float* keys2, int kstride,
                                 const int32_t* match12, int nit, const int32_t* sets, float sigma, float* H21,
                                 float* F21, float* scores, int32_t* its, uint8_t* inl_H, uint8_t* inl_F,
                                 int32_t* counters, float* hyp, float* it_scores);

struct Frame {
  cv::Mat mK;
  std::vector<cv::KeyPoint> mvKeysUn;
};

// a small linear congruential generator: the scene must not touch rand()
static uint32_t lcg_state = 12345;
static double uni(double a, double b) {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return a + (b - a) * ((lcg_state >> 8) / 16777216.0);
}

// two views of nm points (planar or with depth spread) as in
// tests/initransac_util.py, a fifth displaced, with unmatched keys in between
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
    const double u = uni(20, 620), v = uni(20, 460);
    const double z = planar ? 5.0 + 0.3 * (u - cx) / cx : 5.0 + uni(-2, 5);
    const double X = (u - cx) / fx * z, Y = (v - cy) / fx * z;
    const double X2 = cos(a) * X + sin(a) * z + 0.4, Y2 = Y + 0.05, Z2 = -sin(a) * X + cos(a) * z + 0.02;
    double u2 = fx * X2 / Z2 + cx + uni(-0.3, 0.3), v2 = fx * Y2 / Z2 + cy + uni(-0.3, 0.3);
    if (i % 5 == 4) {
      const double ang = uni(0, 6.283), mag = uni(30, 60);
      u2 += mag * cos(ang), v2 += mag * sin(ang);
    }
    if (i % 3 == 0) {  // an unmatched key in each frame
      F1.mvKeysUn.push_back(cv::KeyPoint((float)uni(0, 640), (float)uni(0, 480), 31.0f));
      match12.push_back(-1);
      F2.mvKeysUn.push_back(cv::KeyPoint((float)uni(0, 640), (float)uni(0, 480), 31.0f));
    }
    F1.mvKeysUn.push_back(cv::KeyPoint((float)(u + uni(-0.3, 0.3)), (float)(v + uni(-0.3, 0.3)), 31.0f));
    match12.push_back((int)F2.mvKeysUn.size());
    F2.mvKeysUn.push_back(cv::KeyPoint((float)u2, (float)v2, 31.0f));
  }
  F2.mvKeysUn.push_back(cv::KeyPoint(1.0f, 2.0f, 31.0f));  // n1 != n2
}

static std::vector<int32_t> flat(const std::vector<std::vector<size_t> >& sets) {
  std::vector<int32_t> f;
  for (const auto& s : sets)
    for (size_t v : s) f.push_back((int32_t)v);
  return f;
}

struct Ref {
  float H[9], F[9], scores[3];
  int32_t its[2];
  std::vector<uint8_t> inlH, inlF;
};

static Ref restate(const Frame& F1, const Frame& F2, const std::vector<int>& m12,
                   const std::vector<std::vector<size_t> >& sets, float sigma) {
  Ref r;
  std::vector<int32_t> m(m12.begin(), m12.end()), s = flat(sets);
  r.inlH.assign(m12.size() + 1, 0);
  r.inlF.assign(m12.size() + 1, 0);
  const int nm = ir_ref_initialize((int)F1.mvKeysUn.size(), &F1.mvKeysUn[0].pt.x, (int)F2.mvKeysUn.size(),
                                   &F2.mvKeysUn[0].pt.x, (int)(sizeof(cv::KeyPoint) / sizeof(float)), m.data(),
                                   (int)sets.size(), s.data(), sigma, r.H, r.F, r.scores, r.its, r.inlH.data(),
                                   r.inlF.data(), nullptr, nullptr, nullptr);
  r.inlH.resize(nm);
  r.inlF.resize(nm);
  return r;
}

static bool same_word(float a, float b) { return (a != a && b != b) || memcmp(&a, &b, 4) == 0; }

// words of the six outputs that equal the restatement's
static int compare(const char* what, ORB_SLAM2::Initializer& I, const Ref& r, bool threads) {
  std::vector<bool> inH, inF;
  float SH = -1, SF = -1;
  cv::Mat H, F;
  if (threads) {  // as Initialize :68-71 calls them
    std::thread tH([&] { I.FindHomography(inH, SH, H); });
    std::thread tF([&] { I.FindFundamental(inF, SF, F); });
    tH.join();
    tF.join();
  } else {
    I.FindHomography(inH, SH, H);
    I.FindFundamental(inF, SF, F);
  }
  int words = 0, flags = 0;
  // without a winner the caller's matrix is left as it was (empty here)
  if (r.its[0] < 0) words += H.empty() ? 9 : 0;
  if (r.its[1] < 0) words += F.empty() ? 9 : 0;
  if (r.its[0] >= 0 && !H.empty())
    for (int i = 0; i < 9; ++i) words += same_word(H.at<float>(i / 3, i % 3), r.H[i]);
  if (r.its[1] >= 0 && !F.empty())
    for (int i = 0; i < 9; ++i) words += same_word(F.at<float>(i / 3, i % 3), r.F[i]);
  words += same_word(SH, r.scores[0]) + same_word(SF, r.scores[1]) + same_word(I.RH(), r.scores[2]);
  words += I.Result().it_H == r.its[0];
  words += I.Result().it_F == r.its[1];
  EXPECT(inH.size() == r.inlH.size() && inF.size() == r.inlF.size());
  for (size_t i = 0; i < inH.size() && i < r.inlH.size(); ++i) flags += inH[i] == (r.inlH[i] != 0);
  for (size_t i = 0; i < inF.size() && i < r.inlF.size(); ++i) flags += inF[i] == (r.inlF[i] != 0);
  printf("%s: %d of 23 words, %d of %zu flags, RH %.4f, %d H inliers\n", what, words, flags, 2 * r.inlH.size(),
         (double)I.RH(), (int)std::count(inH.begin(), inH.end(), true));
  EXPECT(words == 23 && flags == (int)(2 * r.inlH.size()));
  return words;
}

int main() {
  const int sizes[4] = {120, 40, 257, 8};
  Frame F1[4], F2[4];
  std::vector<int> m12[4];
  for (int k = 0; k < 4; ++k) make_scene(sizes[k], k % 2 == 0, F1[k], F2[k], m12[k]);

  // the draw restated: srand(0), then per initializer, in order, :49-63
  const int nit = 200;
  std::vector<std::vector<std::vector<size_t> > > want(4);
  srand(0);
  for (int k = 0; k < 4; ++k) {
    want[k].assign(nit, std::vector<size_t>(8, 0));
    for (int it = 0; it < nit; ++it) {
      std::vector<size_t> avail;
      for (int i = 0; i < sizes[k]; ++i) avail.push_back(i);
      for (int j = 0; j < 8; ++j) {
        const int d = (int)avail.size();
        const int randi = int(((double)rand() / ((double)RAND_MAX + 1.0)) * d);
        want[k][it][j] = avail[randi];
        avail[randi] = avail.back();
        avail.pop_back();
      }
    }
  }
  srand(12345);  // SeedRandOnce(0) must put the stream back to srand(0), once
  std::vector<std::unique_ptr<ORB_SLAM2::Initializer> > init;
  int draws = 0;
  for (int k = 0; k < 4; ++k) {
    init.emplace_back(new ORB_SLAM2::Initializer(F1[k], 1.0f, nit));
    init[k]->SetMatches(F2[k], m12[k]);
    EXPECT((int)init[k]->mvMatches12.size() == sizes[k]);
    draws += init[k]->mvSets == want[k];
  }
  printf("draw: %d of 4 set tables equal the restated draw\n", draws);
  EXPECT(draws == 4);
  EXPECT(init[0]->mvbMatched1.size() == F1[0].mvKeysUn.size() && !init[0]->mvbMatched1[0] && init[0]->mvbMatched1[1]);

  // single, the first from two threads
  Ref refs[4];
  for (int k = 0; k < 4; ++k) refs[k] = restate(F1[k], F2[k], m12[k], init[k]->mvSets, 1.0f);
  for (int k = 0; k < 4; ++k)
    printf("restatement pair %d: RH %.4f, winners %d %d\n", k, (double)refs[k].scores[2], refs[k].its[0], refs[k].its[1]);
  EXPECT(refs[0].scores[2] > 0.40f && refs[1].scores[2] <= 0.40f);  // planar, general
  compare("single pair 0", *init[0], refs[0], true);
  compare("single pair 1", *init[1], refs[1], false);
  EXPECT(init[0]->RH() > 0.40f);   // planar
  EXPECT(init[1]->RH() <= 0.40f);  // general

  // batched: fresh initializers with the same sets, one device call
  std::vector<std::unique_ptr<ORB_SLAM2::Initializer> > b;
  std::vector<ORB_SLAM2::Initializer*> ptrs;
  for (int k = 0; k < 4; ++k) {
    b.emplace_back(new ORB_SLAM2::Initializer(F1[k], 1.0f, nit));
    b[k]->SetMatches(F2[k], m12[k]);
    b[k]->mvSets = init[k]->mvSets;
    ptrs.push_back(b[k].get());
  }
  ORB_SLAM2::Initializer::FindModels(ptrs);
  for (int k = 0; k < 4; ++k) {
    char what[32];
    snprintf(what, sizeof what, "batch pair %d", k);
    compare(what, *b[k], refs[k], false);
  }
  for (int k = 0; k < 2; ++k)  // batched equals single, word for word
    EXPECT(memcmp(&b[k]->Result(), &init[k]->Result(), sizeof(orbx_ransac_result)) == 0);

  // fewer than 8 matches and unequal iteration counts are refused
  {
    std::vector<int> few(m12[3]);
    for (int& v : few)
      if (v >= 0) {
        v = -1;
        break;
      }
    ORB_SLAM2::Initializer I(F1[3], 1.0f, 10);
    bool threw = false;
    try {
      I.SetMatches(F2[3], few);
    } catch (const cv::Exception& e) {
      threw = e.code == ORBX_ERR_ARG;
    }
    EXPECT(threw);
    ORB_SLAM2::Initializer J(F1[3], 1.0f, 10);
    J.SetMatches(F2[3], m12[3]);
    threw = false;
    try {
      ORB_SLAM2::Initializer::FindModels({b[0].get(), &J});
    } catch (const cv::Exception& e) {
      threw = e.code == ORBX_ERR_ARG;
    }
    EXPECT(threw);
  }
  printf("initransac_compat_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

// ORB_SLAM2::Sim3Solver of cpp/orbslam2_compat.hpp over stand-in KeyFrame and
// MapPoint classes: the constructor's filtering, the rand() draw against a
// restated draw after srand(0), iterate and the getters against the CPU
// restatement (tests/cpp/sim3_ref.c) bit for bit, IterateAll against successive
// single calls given the same triples, a continued solver, and two solvers from
// two threads.  Needs a GPU.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <thread>
#include <vector>

#include "orbslam2_compat.hpp"
#include "expect.h"

extern "C" int s3_ref_solve(int ncorr, const float* pos1, const float* pos2, const float* sig1, const float* sig2,
                            const float* pose, const float* cams, int nit, const int32_t* triples, int min_inliers,
                            int fix_scale, int best_in, int eval_all, int32_t* ires, float* fres, uint8_t* inliers,
                            int32_t* counters, int32_t* counts, float* hyp, float* quat, float* corr_out);

struct KeyFrame;
struct MapPoint {
  cv::Mat pos;
  bool bad = false;
  int idx1 = -1, idx2 = -1;
  KeyFrame *kf1 = nullptr, *kf2 = nullptr;
  bool isBad() { return bad; }
  int GetIndexInKeyFrame(KeyFrame* kf) { return kf == kf1 ? idx1 : kf == kf2 ? idx2 : -1; }
  cv::Mat GetWorldPos() { return pos.clone(); }
};
struct KeyFrame {
  cv::Mat mK, R, t;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvLevelSigma2;
  std::vector<MapPoint*> matches;
  std::vector<MapPoint*> GetMapPointMatches() { return matches; }
  cv::Mat GetRotation() { return R.clone(); }
  cv::Mat GetTranslation() { return t.clone(); }
};
typedef ORB_SLAM2::Sim3Solver<KeyFrame, MapPoint> Solver;

// a small linear congruential generator: the scene must not touch rand()
static uint32_t lcg_state = 2024;
static double uni(double a, double b) {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return a + (b - a) * ((lcg_state >> 8) / 16777216.0);
}

static void rodrigues(const double a[3], double ang, double R[9]) {
  const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), x = a[0] / n, y = a[1] / n, z = a[2] / n;
  const double c = cos(ang), s = sin(ang), c1 = 1 - c;
  const double M[9] = {c + c1 * x * x, c1 * x * y - s * z, c1 * x * z + s * y, c1 * x * y + s * z, c + c1 * y * y,
                       c1 * y * z - s * x, c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z};
  memcpy(R, M, sizeof M);
}

static cv::Mat mat(int r, int c, const double* v) {
  cv::Mat m(r, c, CV_32F);
  for (int i = 0; i < r * c; ++i) m.at<float>(i / c, i % c) = (float)v[i];
  return m;
}

// One pair of keyframes with n matched map points, as tests/sim3_util.py builds
// them: X1c = s R X2c + t, 2 mm of noise, every fourth match wrong; besides, a
// null match, a bad point and a point that keyframe 2 does not observe, which
// the constructor drops
struct Scene {
  KeyFrame kf1, kf2;
  std::vector<std::unique_ptr<MapPoint> > own;
  std::vector<MapPoint*> matched12;
  std::vector<size_t> kept;  // the rows of matched12 that survive, = mvnIndices1
  // the restatement's inputs
  std::vector<float> pos1, pos2, sig1, sig2;
  float pose[24], cams[8];
};

static void make_scene(int n, double s, Scene& S) {
  const double K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
  const double ax[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
  double R[9], R1[9], R2[9];
  rodrigues(ax, 0.1, R);
  const double a1[3] = {uni(-1, 1), uni(-1, 1), 0.3}, a2[3] = {0.2, uni(-1, 1), uni(-1, 1)};
  rodrigues(a1, uni(0.2, 1.0), R1);
  rodrigues(a2, uni(0.2, 1.0), R2);
  const double t[3] = {uni(-0.3, 0.3), uni(-0.3, 0.3), uni(-0.3, 0.3)};
  const double t1[3] = {uni(-2, 2), uni(-2, 2), uni(-2, 2)}, t2[3] = {uni(-2, 2), uni(-2, 2), uni(-2, 2)};
  for (KeyFrame* kf : {&S.kf1, &S.kf2}) {
    kf->mK = mat(3, 3, K);
    kf->mvLevelSigma2 = {1.0f, 1.44f, 2.0736f, 2.985984f};
  }
  S.kf1.R = mat(3, 3, R1), S.kf1.t = mat(3, 1, t1);
  S.kf2.R = mat(3, 3, R2), S.kf2.t = mat(3, 1, t2);
  const int rows = n + 3;
  S.kf1.matches.assign(rows, nullptr);
  S.matched12.assign(rows, nullptr);
  for (int r = 0, i = 0; r < rows; ++r) {
    const int special = r == 2 ? 1 : r == 5 ? 2 : r == 9 ? 3 : 0;  // null match, bad point, not in keyframe 2
    const double z = uni(3, 15), u = uni(40, 600), v = uni(40, 440);
    double X1[3] = {(u - 320) / 500 * z, (v - 240) / 500 * z, z}, X2[3], d[3] = {X1[0] - t[0], X1[1] - t[1], X1[2] - t[2]};
    for (int k = 0; k < 3; ++k) X2[k] = (R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2]) / s + uni(-0.003, 0.003);
    if (!special && i % 4 == 3) {
      const double zb = uni(3, 15);
      X2[0] = uni(-0.5, 0.5) * zb, X2[1] = uni(-0.4, 0.4) * zb, X2[2] = zb;
    }
    double w1[3], w2[3], e1[3] = {X1[0] - t1[0], X1[1] - t1[1], X1[2] - t1[2]},
                         e2[3] = {X2[0] - t2[0], X2[1] - t2[1], X2[2] - t2[2]};
    for (int k = 0; k < 3; ++k) {
      w1[k] = R1[k] * e1[0] + R1[3 + k] * e1[1] + R1[6 + k] * e1[2];
      w2[k] = R2[k] * e2[0] + R2[3 + k] * e2[1] + R2[6 + k] * e2[2];
    }
    S.own.emplace_back(new MapPoint);
    MapPoint* p1 = S.own.back().get();
    S.own.emplace_back(new MapPoint);
    MapPoint* p2 = S.own.back().get();
    p1->pos = mat(3, 1, w1), p2->pos = mat(3, 1, w2);
    p1->kf1 = p2->kf1 = &S.kf1, p1->kf2 = p2->kf2 = &S.kf2;
    cv::KeyPoint k1((float)u, (float)v, 31.0f), k2((float)u, (float)v, 31.0f);
    k1.octave = (int)uni(0, 3.999), k2.octave = (int)uni(0, 3.999);
    p1->idx1 = (int)S.kf1.mvKeysUn.size(), p2->idx2 = (int)S.kf2.mvKeysUn.size();
    S.kf1.mvKeysUn.push_back(k1), S.kf2.mvKeysUn.push_back(k2);
    S.kf1.matches[r] = p1;
    S.matched12[r] = special == 1 ? nullptr : p2;
    if (special == 2) p1->bad = true;
    if (special == 3) p2->idx2 = -1;
    if (special) continue;
    S.kept.push_back((size_t)r);
    for (int k = 0; k < 3; ++k) S.pos1.push_back(p1->pos.at<float>(k, 0)), S.pos2.push_back(p2->pos.at<float>(k, 0));
    S.sig1.push_back(S.kf1.mvLevelSigma2[k1.octave]), S.sig2.push_back(S.kf2.mvLevelSigma2[k2.octave]);
    ++i;
  }
  for (int e = 0; e < 9; ++e) S.pose[e] = (float)R1[e], S.pose[12 + e] = (float)R2[e];
  for (int e = 0; e < 3; ++e) S.pose[9 + e] = (float)t1[e], S.pose[21 + e] = (float)t2[e];
  const float cams[8] = {500, 500, 320, 240, 500, 500, 320, 240};
  memcpy(S.cams, cams, sizeof cams);
}

struct Ref {
  int32_t ires[4];
  float fres[25];
  std::vector<uint8_t> inl;
};

static Ref restate(const Scene& S, const std::vector<int32_t>& triples, int min_inliers, bool fix, int best_in) {
  Ref r;
  const int n = (int)S.sig1.size();
  r.inl.assign((size_t)n + 1, 0);
  const int32_t none[3] = {0, 0, 0};
  s3_ref_solve(n, S.pos1.data(), S.pos2.data(), S.sig1.data(), S.sig2.data(), S.pose, S.cams, (int)triples.size() / 3,
               triples.empty() ? none : triples.data(), min_inliers, fix ? 1 : 0, best_in, 0, r.ires, r.fres,
               r.inl.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  r.inl.resize((size_t)n);
  return r;
}

static bool same_word(float a, float b) { return (a != a && b != b) || memcmp(&a, &b, 4) == 0; }

// what one iterate call left against the restatement of the triples it drew:
// the 13 words of the getters, the 12 of T12's rows, the flags and the counts
static void compare(const char* what, Solver& S, const Scene& sc, const Ref& r, const cv::Mat& T12, bool bNoMore,
                    const std::vector<bool>& vbInliers, int nInliers, int its_before) {
  int words = 0, flags = 0;
  const bool hit = r.ires[0] >= 0;
  EXPECT(T12.empty() == !hit);
  EXPECT(nInliers == (hit ? r.ires[2] : 0));
  EXPECT(S.mnBestInliers == r.ires[2]);
  EXPECT(S.mnIterations == its_before + (hit ? r.ires[0] + 1 : (int)S.mvTriples.size() / 3));
  EXPECT(bNoMore == (!hit && S.mnIterations >= S.mRansacMaxIts));
  if (r.ires[1] >= 0) {
    const cv::Mat R = S.GetEstimatedRotation(), t = S.GetEstimatedTranslation();
    for (int i = 0; i < 9; ++i) words += same_word(R.at<float>(i / 3, i % 3), r.fres[i]);
    for (int i = 0; i < 3; ++i) words += same_word(t.at<float>(i, 0), r.fres[9 + i]);
    words += same_word(S.GetEstimatedScale(), r.fres[12]);
    for (int i = 0; i < 9; ++i) words += same_word(S.Result().sR21[i], r.fres[13 + i]);
    for (int i = 0; i < 3; ++i) words += same_word(S.Result().t21[i], r.fres[22 + i]);
    if (hit)
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) words += same_word(T12.at<float>(i, j), r.fres[12] * r.fres[3 * i + j]);
        words += same_word(T12.at<float>(i, 3), r.fres[9 + i]);
      }
    else
      words += 12;
  } else {
    words = 37;
  }
  EXPECT(vbInliers.size() == sc.matched12.size());
  std::vector<bool> want(sc.matched12.size(), false);
  if (hit)
    for (size_t i = 0; i < r.inl.size(); ++i) want[sc.kept[i]] = r.inl[i] != 0;
  for (size_t i = 0; i < want.size() && i < vbInliers.size(); ++i) flags += vbInliers[i] == want[i];
  printf("%s: %d of 37 words, %d of %zu flags, it_hit %d, %d inliers\n", what, words, flags, want.size(), r.ires[0],
         nInliers);
  EXPECT(words == 37 && flags == (int)want.size());
}

// one iterate call, and its check against the restatement afterwards
struct Single {
  int before = 0, best_in = 0, nIn = -1;
  bool bNoMore = false;
  std::vector<bool> vb;
  cv::Mat T12;
  void call(Solver& S, int n) {
    before = S.mnIterations, best_in = S.mnBestInliers;
    T12 = S.iterate(n, bNoMore, vb, nIn);
  }
  void check(const char* what, Solver& S, const Scene& sc) {
    const Ref r = restate(sc, S.mvTriples, S.mRansacMinInliers, S.mbFixScale, best_in);
    compare(what, S, sc, r, T12, bNoMore, vb, nIn, before);
  }
};

static void run_single(const char* what, Solver& S, const Scene& sc, int n) {
  Single c;
  c.call(S, n);
  c.check(what, S, sc);
}

int main() {
  const int sizes[3] = {60, 24, 130};
  const double scales[3] = {1.0, 0.7, 1.4};
  Scene sc[3];
  for (int k = 0; k < 3; ++k) make_scene(sizes[k], scales[k], sc[k]);
  auto fresh = [&](int k, int min_inliers, int max_its) {
    std::unique_ptr<Solver> S(new Solver(&sc[k].kf1, &sc[k].kf2, sc[k].matched12, k == 0));
    S->SetRansacParameters(0.99, min_inliers, max_its);
    return S;
  };

  {  // the constructor's filtering and SetRansacParameters
    auto S = fresh(0, 20, 300);
    EXPECT(S->N == sizes[0] && S->mN1 == sizes[0] + 3 && S->mvnIndices1 == sc[0].kept);
    const float eps = 20.0f / 60;
    EXPECT(S->mRansacMaxIts == std::max(1, std::min((int)ceil(log(1 - 0.99) / log(1 - pow(eps, 3))), 300)));
    auto T = fresh(1, 24, 300);
    EXPECT(T->mRansacMaxIts == 1);  // mRansacMinInliers == N
  }

  // the draw restated: srand(0), then per solver, in list order, :143-157; a
  // solver draws min(n, mRansacMaxIts) triples (:138)
  const int n = 40;
  std::vector<std::unique_ptr<Solver> > all;
  std::vector<Solver*> ptrs;
  for (int k = 0; k < 3; ++k) {
    all.push_back(fresh(k, k == 1 ? 12 : 20, 300));
    ptrs.push_back(all[k].get());
  }
  EXPECT(all[0]->mRansacMaxIts > n && all[1]->mRansacMaxIts == 35 && all[2]->mRansacMaxIts == 300);
  std::vector<std::vector<int32_t> > want(3);
  srand(0);
  for (int k = 0; k < 3; ++k)
    for (int it = 0; it < std::min(n, all[k]->mRansacMaxIts); ++it) {
      std::vector<size_t> avail;
      for (int i = 0; i < sizes[k]; ++i) avail.push_back(i);
      for (int j = 0; j < 3; ++j) {
        const int randi = int(((double)rand() / ((double)RAND_MAX + 1.0)) * (int)avail.size());
        want[k].push_back((int32_t)avail[randi]);
        avail[randi] = avail.back();
        avail.pop_back();
      }
    }
  srand(0);
  Solver::IterateAll(ptrs, n);
  int draws = 0;
  for (int k = 0; k < 3; ++k) draws += all[k]->mvTriples == want[k];
  printf("draw: %d of 3 triple tables equal the restated draw\n", draws);
  EXPECT(draws == 3);
  for (int k = 0; k < 3; ++k) {  // IterateAll against the restatement
    bool bNoMore = false;
    std::vector<bool> vb;
    int nIn = -1;
    const cv::Mat T12 = all[k]->Collect(bNoMore, vb, nIn);
    const Ref r = restate(sc[k], want[k], all[k]->mRansacMinInliers, k == 0, 0);
    char what[32];
    snprintf(what, sizeof what, "batch solver %d", k);
    compare(what, *all[k], sc[k], r, T12, bNoMore, vb, nIn, 0);
  }

  // successive single calls after the same seed draw the same triples: word for word the batch
  srand(0);
  for (int k = 0; k < 3; ++k) {
    auto S = fresh(k, k == 1 ? 12 : 20, 300);
    char what[32];
    snprintf(what, sizeof what, "single solver %d", k);
    run_single(what, *S, sc[k], n);
    EXPECT(S->mvTriples == all[k]->mvTriples);
    EXPECT(memcmp(&S->Result(), &all[k]->Result(), sizeof(orbx_sim3_result)) == 0);
    EXPECT(S->mvbBestInliers == all[k]->mvbBestInliers && S->mnIterations == all[k]->mnIterations);
  }

  {  // a solver that cannot return (98 of its 130 matches are right, and 98 > 98 never holds), continued
    auto S = fresh(2, 98, 300);
    EXPECT(S->mRansacMaxIts == 9);  // ceil(log(0.01) / log(1 - (98 / 130)^3))
    run_single("continued 1", *S, sc[2], 4);
    run_single("continued 2", *S, sc[2], 4);
    run_single("continued 3", *S, sc[2], 4);  // only one is left
    EXPECT(S->mnIterations == 9 && S->mvTriples.size() == 3);
    bool bNoMore = false;
    std::vector<bool> vb;
    int nIn = -1;
    EXPECT(S->iterate(5, bNoMore, vb, nIn).empty() && bNoMore && S->mvTriples.empty());
  }
  {  // fewer correspondences than min_inliers: no draw, no more
    auto S = fresh(1, 25, 300);
    srand(5);
    const int next = rand();
    srand(5);
    bool bNoMore = false;
    std::vector<bool> vb(3, true);
    int nIn = -1;
    EXPECT(S->iterate(10, bNoMore, vb, nIn).empty() && bNoMore && nIn == 0 && S->mnIterations == 0);
    EXPECT(vb.size() == sc[1].matched12.size() && rand() == next);
  }
  {  // find
    auto S = fresh(0, 20, 300);
    std::vector<bool> vb;
    int nIn = -1;
    const cv::Mat T12 = S->find(vb, nIn);
    const Ref r = restate(sc[0], S->mvTriples, 20, true, 0);
    compare("find", *S, sc[0], r, T12, false, vb, nIn, 0);
    EXPECT(!T12.empty() && T12.rows == 4 && T12.at<float>(3, 3) == 1.0f && T12.at<float>(3, 0) == 0.0f);
  }
  {  // two solvers from two threads: each equals the restatement of the triples it drew
    auto A = fresh(0, 20, 300), B = fresh(2, 20, 300);
    Single ca, cb;
    std::thread ta([&] { ca.call(*A, 30); });
    std::thread tb([&] { cb.call(*B, 30); });
    ta.join();
    tb.join();
    ca.check("thread 0", *A, sc[0]);
    cb.check("thread 1", *B, sc[2]);
  }
  printf("sim3_compat_main: %d failures\n", fails);
  return fails ? 1 : 0;
}

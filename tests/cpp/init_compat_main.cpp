// init_compat_main.cpp -- ORBmatcher::SearchForInitialization of
// cpp/orbslam2_compat.hpp inside a loop shaped like
// Tracking::MonocularInitialization (src/Tracking.cc:305-333): the initial
// frame sets mvbPrevMatched and mvIniMatches, then three frames are searched
// with both carried along.  Next to it runs a straight host loop written from
// src/ORBmatcher.cc:197-276 over the same stand-in Frame class (its mGrid and
// GetFeaturesInArea written from src/Frame.cc:210-225,307-372), on its own copy
// of the two vectors.  argv: seed, output file.  Output per side (H = host
// loop, D = compat header) and frame f:
//   "<side> RET f n", "<side> M f i match x y" for every row (x, y as bits).
// The last line pair is the batched overload on two of the frames.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "orbslam2_compat.hpp"

using std::vector;

namespace ORB_SLAM2 {
#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

class Frame {
 public:
  int N = 0;
  vector<cv::KeyPoint> mvKeys, mvKeysUn;
  cv::Mat mDescriptors;
  float mnMinX = 0, mnMinY = 0, mnMaxX = 640, mnMaxY = 480;
  float mfGridElementWidthInv = 64.0f / 640.0f, mfGridElementHeightInv = 48.0f / 480.0f;
  vector<size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];

  bool PosInGrid(const cv::KeyPoint& kp, int& posX, int& posY) {
    posX = round((kp.pt.x - mnMinX) * mfGridElementWidthInv);
    posY = round((kp.pt.y - mnMinY) * mfGridElementHeightInv);
    if (posX < 0 || posX >= FRAME_GRID_COLS || posY < 0 || posY >= FRAME_GRID_ROWS) return false;
    return true;
  }
  void AssignFeaturesToGrid() {
    for (int i = 0; i < N; i++) {
      const cv::KeyPoint& kp = mvKeysUn[i];
      int nGridPosX, nGridPosY;
      if (PosInGrid(kp, nGridPosX, nGridPosY)) mGrid[nGridPosX][nGridPosY].push_back(i);
    }
  }
  vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const int minLevel,
                                   const int maxLevel) const {
    vector<size_t> vIndices;
    vIndices.reserve(N);
    const int nMinCellX = std::max(0, (int)floor((x - mnMinX - r) * mfGridElementWidthInv));
    if (nMinCellX >= FRAME_GRID_COLS) return vIndices;
    const int nMaxCellX = std::min((int)FRAME_GRID_COLS - 1, (int)ceil((x - mnMinX + r) * mfGridElementWidthInv));
    if (nMaxCellX < 0) return vIndices;
    const int nMinCellY = std::max(0, (int)floor((y - mnMinY - r) * mfGridElementHeightInv));
    if (nMinCellY >= FRAME_GRID_ROWS) return vIndices;
    const int nMaxCellY = std::min((int)FRAME_GRID_ROWS - 1, (int)ceil((y - mnMinY + r) * mfGridElementHeightInv));
    if (nMaxCellY < 0) return vIndices;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
      for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
        const vector<size_t> vCell = mGrid[ix][iy];
        if (vCell.empty()) continue;
        for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
          const cv::KeyPoint& kpUn = mvKeysUn[vCell[j]];
          if (bCheckLevels) {
            if (kpUn.octave < minLevel) continue;
            if (maxLevel >= 0)
              if (kpUn.octave > maxLevel) continue;
          }
          const float distx = kpUn.pt.x - x;
          const float disty = kpUn.pt.y - y;
          if (fabs(distx) < r && fabs(disty) < r) vIndices.push_back(vCell[j]);
        }
      }
    }
    return vIndices;
  }
};
}  // namespace ORB_SLAM2

using namespace ORB_SLAM2;

// ---------------------------------------------------------------- host loop
static const int TH_LOW = 50, HISTO_LENGTH = 30;

static void ComputeThreeMaxima(vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int s = histo[i].size();
    if (s > max1) {
      max3 = max2; max2 = max1; max1 = s;
      ind3 = ind2; ind2 = ind1; ind1 = i;
    } else if (s > max2) {
      max3 = max2; max2 = s;
      ind3 = ind2; ind2 = i;
    } else if (s > max3) {
      max3 = s;
      ind3 = i;
    }
  }
  if (max2 < 0.1f * (float)max1) {
    ind2 = -1;
    ind3 = -1;
  } else if (max3 < 0.1f * (float)max1) {
    ind3 = -1;
  }
}

static int ref_search(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12,
                      int windowSize, float mfNNratio, bool mbCheckOrientation) {
  int nmatches = 0;
  vnMatches12.resize(F1.mvKeysUn.size(), -1);
  vector<int> rotHist[HISTO_LENGTH];
  const float factor = 1.0f / HISTO_LENGTH;
  vector<int> vMatchedDistance(F2.mvKeysUn.size(), INT_MAX);
  vector<int> vnMatches21(F2.mvKeysUn.size(), -1);
  for (size_t i1 = 0; i1 < F1.mvKeysUn.size(); ++i1) {
    const cv::KeyPoint& kp1 = F1.mvKeysUn[i1];
    if (kp1.octave > 0) continue;
    auto vIndices2 = F2.GetFeaturesInArea(vbPrevMatched[i1].x, vbPrevMatched[i1].y, windowSize, kp1.octave, kp1.octave);
    if (vIndices2.empty()) continue;
    const cv::Mat& d1 = F1.mDescriptors.row(i1);
    int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
    for (auto i2 : vIndices2) {
      const cv::Mat& d2 = F2.mDescriptors.row(i2);
      int dist = ORBmatcher::DescriptorDistance(d1, d2);
      if (dist < vMatchedDistance[i2]) {
        if (dist < bestDist) {
          bestDist2 = bestDist;
          bestDist = dist;
          bestIdx2 = i2;
        } else if (dist < bestDist2) {
          bestDist2 = dist;
        }
      }
    }
    if (bestDist <= TH_LOW && bestDist < static_cast<float>(bestDist2) * mfNNratio) {
      if (vnMatches21[bestIdx2] >= 0) {
        vnMatches12[vnMatches21[bestIdx2]] = -1;
        nmatches--;
      }
      vnMatches12[i1] = bestIdx2;
      vnMatches21[bestIdx2] = i1;
      vMatchedDistance[bestIdx2] = bestDist;
      nmatches++;
      if (mbCheckOrientation) {
        float rot = kp1.angle - F2.mvKeysUn[bestIdx2].angle;
        if (rot < 0.0) rot += 360.0f;
        int bin = round(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        rotHist[bin].push_back(i1);
      }
    }
  }
  if (mbCheckOrientation) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    ComputeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; ++i) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int idx1 : rotHist[i]) {
        if (vnMatches12[idx1] >= 0) {
          vnMatches12[idx1] = -1;
          nmatches--;
        }
      }
    }
  }
  for (size_t i1 = 0; i1 < vnMatches12.size(); ++i1) {
    if (vnMatches12[i1] >= 0) vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt;
  }
  return nmatches;
}

// ---------------------------------------------------------------- planted frames
static uint32_t g_state = 1;
static uint32_t rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state >> 8;
}
static float uni(float a, float b) { return a + (b - a) * (float)(rnd() & 0xFFFF) / 65536.0f; }

static void finish(Frame& F, const vector<cv::KeyPoint>& keys, const vector<uint8_t>& desc) {
  F.N = (int)keys.size();
  F.mvKeys = keys;
  F.mvKeysUn = keys;
  F.mDescriptors = cv::Mat(F.N, 32, CV_8U);
  if (F.N) memcpy(F.mDescriptors.data, desc.data(), desc.size());
  F.AssignFeaturesToGrid();
}

static void initial_frame(Frame& F, int n) {
  vector<cv::KeyPoint> keys;
  vector<uint8_t> desc((size_t)n * 32);
  for (auto& b : desc) b = (uint8_t)rnd();
  for (int i = 0; i < n; i++) {
    const uint32_t u = rnd() % 100;
    const int octave = u < 60 ? 0 : u < 64 ? -1 : 1 + (int)(rnd() % 7);
    keys.push_back(cv::KeyPoint(uni(5, 635), uni(5, 475), 31.0f, uni(0, 360), 0, octave));
    if (i > 0 && rnd() % 4 == 0) {  // a near-duplicate of an earlier row: contention
      const int j = (int)(rnd() % i);
      keys[i].pt = cv::Point2f(keys[j].pt.x + uni(-20, 20), keys[j].pt.y + uni(-20, 20));
      keys[i].octave = keys[j].octave;
      memcpy(&desc[(size_t)i * 32], &desc[(size_t)j * 32], 32);
      for (int k = (int)(rnd() % 6); k > 0; k--) desc[(size_t)i * 32 + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
    }
  }
  finish(F, keys, desc);
}

// a moved, shuffled copy of F0 with noise on positions and descriptors, a
// quarter of random features, most angles turned by `rot`
static void next_frame(Frame& F, const Frame& F0, int n, float shift, float rot) {
  vector<cv::KeyPoint> keys;
  vector<uint8_t> desc((size_t)n * 32);
  vector<int> perm(F0.N);
  for (int i = 0; i < F0.N; i++) perm[i] = i;
  for (int i = F0.N - 1; i > 0; i--) std::swap(perm[i], perm[rnd() % (i + 1)]);
  for (int i = 0; i < n; i++) {
    if (i % 4 == 3 || i >= F0.N) {
      keys.push_back(cv::KeyPoint(uni(0, 640), uni(0, 480), 31.0f, uni(0, 360), 0, rnd() % 2 ? 0 : (int)(rnd() % 8)));
      for (int k = 0; k < 32; k++) desc[(size_t)i * 32 + k] = (uint8_t)rnd();
      continue;
    }
    const int j = perm[i];
    const cv::KeyPoint& k0 = F0.mvKeysUn[j];
    float a = k0.angle - rot;
    if (a < 0) a += 360.0f;
    if (rnd() % 5 == 0) a = uni(0, 360);
    keys.push_back(cv::KeyPoint(k0.pt.x + shift + uni(-12, 12), k0.pt.y + uni(-12, 12), 31.0f, a, 0, k0.octave));
    memcpy(&desc[(size_t)i * 32], F0.mDescriptors.data + (size_t)j * 32, 32);
    for (int k = (int)(rnd() % 40); k > 0; k--) desc[(size_t)i * 32 + rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
  }
  finish(F, keys, desc);
}

static void dump(FILE* f, const char* side, int frame, int ret, const vector<int>& m, const vector<cv::Point2f>& pv) {
  fprintf(f, "%s RET %d %d\n", side, frame, ret);
  for (size_t i = 0; i < m.size(); i++) {
    uint32_t bx, by;
    memcpy(&bx, &pv[i].x, 4);
    memcpy(&by, &pv[i].y, 4);
    fprintf(f, "%s M %d %zu %d %08x %08x\n", side, frame, i, m[i], bx, by);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  g_state = (uint32_t)atoi(argv[1]);
  FILE* f = fopen(argv[2], "w");
  if (!f) return 2;
  const int n = 400;
  Frame mInitialFrame;
  initial_frame(mInitialFrame, n);
  vector<Frame> frames(3);
  for (int k = 0; k < 3; k++) next_frame(frames[k], mInitialFrame, k == 1 ? 450 : n, 6.0f * (k + 1), 35.0f);

  for (int side = 0; side < 2; side++) {
    // Tracking.cc:310-316
    vector<cv::Point2f> mvbPrevMatched(mInitialFrame.mvKeysUn.size());
    for (size_t i = 0; i < mInitialFrame.mvKeysUn.size(); i++) mvbPrevMatched[i] = mInitialFrame.mvKeysUn[i].pt;
    vector<int> mvIniMatches;
    mvIniMatches.assign(mInitialFrame.mvKeys.size(), -1);
    for (int k = 0; k < 3; k++) {
      Frame& mCurrentFrame = frames[k];
      ORBmatcher matcher(0.9, true);  // Tracking.cc:327-328
      int nmatches;
      if (side == 0)
        nmatches = ref_search(mInitialFrame, mCurrentFrame, mvbPrevMatched, mvIniMatches, 100, 0.9f, true);
      else
        nmatches = matcher.SearchForInitialization(mInitialFrame, mCurrentFrame, mvbPrevMatched, mvIniMatches, 100);
      dump(f, side ? "D" : "H", k, nmatches, mvIniMatches, mvbPrevMatched);
    }
  }
  // the batched overload: two fresh initializers at once, against two single calls
  {
    vector<Frame*> vpF1(2, &mInitialFrame), vpF2 = {&frames[0], &frames[2]};
    vector<vector<cv::Point2f> > prev(2, vector<cv::Point2f>(mInitialFrame.mvKeysUn.size()));
    for (int p = 0; p < 2; p++)
      for (size_t i = 0; i < mInitialFrame.mvKeysUn.size(); i++) prev[p][i] = mInitialFrame.mvKeysUn[i].pt;
    vector<vector<cv::Point2f> > prevH = prev;
    vector<vector<int> > m(2), mH(2);
    ORBmatcher matcher(0.9, true);
    const vector<int> ret = matcher.SearchForInitialization(vpF1, vpF2, prev, m);  // default window 10
    for (int p = 0; p < 2; p++) {
      const int r = ref_search(*vpF1[p], *vpF2[p], prevH[p], mH[p], 10, 0.9f, true);
      dump(f, "H", 10 + p, r, mH[p], prevH[p]);
      dump(f, "D", 10 + p, ret[p], m[p], prev[p]);
    }
  }
  fclose(f);
  return 0;
}

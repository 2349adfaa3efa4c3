// kfwin_compat_main.cpp -- ORBmatcher::Fuse (both forms, and the batched
// form over the target keyframes of LocalMapping::SearchInNeighbors) and
// SearchBySim3 of cpp/orbslam2_compat.hpp on stand-in KeyFrame / MapPoint
// classes that carry the members the reference reads, next to a straight host
// loop written from src/ORBmatcher.cc:504-730 over the same classes.  Both
// run on their own copy of the same planted scene; Replace / AddObservation /
// AddMapPoint are recorded as events.  argv: seed, output file.  Output, per
// mode (FUSE, SCW, SIM3, BATCH) and side (H = host loop, D = compat header):
//   "<mode> <side> RET n", "<mode> <side> EV ...", "<mode> <side> MP kf idx id"
//   (the final GetMapPoint table), "<mode> <side> OUT i id" (vpReplacePoint /
//   vpMatches12).
#include "kfwin_mocks.hpp"

using namespace ORB_SLAM2;

// ---------------------------------------------------------------- host loops
static const int TH_LOW = 50, TH_HIGH = 100;

static int ref_best(KeyFrame* pKF, float u, float v, float radius, int level, const cv::Mat& dMP, int& bestIdx) {
  int bestDist = INT_MAX;
  bestIdx = -1;
  const vector<size_t> indices = pKF->GetFeaturesInArea(u, v, radius);
  for (auto idx : indices) {
    const cv::KeyPoint& kp = pKF->mvKeysUn[idx];
    if (kp.octave < level - 1 || kp.octave > level) continue;
    const cv::Mat& dKF = pKF->mDescriptors.row(idx);
    int dist = ORBmatcher::DescriptorDistance(dMP, dKF);
    if (dist < bestDist) {
      bestDist = dist;
      bestIdx = idx;
    }
  }
  return bestDist;
}

static bool ref_project(KeyFrame* pKF, const cv::Mat& Rcw, const cv::Mat& tcw, const cv::Mat& Ow, MapPoint* pMP,
                        float th, float& u, float& v, float& radius, int& level) {
  cv::Mat p3Dw = pMP->GetWorldPos();
  cv::Mat p3Dc = Rcw * p3Dw + tcw;
  if (p3Dc.at<float>(2) < 0.0f) return false;
  float invz = 1.0 / p3Dc.at<float>(2);
  float x = p3Dc.at<float>(0) * invz;
  float y = p3Dc.at<float>(1) * invz;
  u = pKF->fx * x + pKF->cx;
  v = pKF->fy * y + pKF->cy;
  if (!pKF->IsInImage(u, v)) return false;
  float dist = cv::norm(p3Dw - Ow);
  if (dist < pMP->GetMinDistanceInvariance() || dist > pMP->GetMaxDistanceInvariance()) return false;
  level = pMP->PredictScale(dist, pKF);
  radius = th * pKF->mvScaleFactors[level];
  return true;
}

static int ref_fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th) {
  cv::Mat Rcw = pKF->GetRotation();
  cv::Mat tcw = pKF->GetTranslation();
  cv::Mat Ow = pKF->GetCameraCenter();
  int nFused = 0;
  for (auto pMP : vpMapPoints) {
    if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
    float u, v, radius;
    int level, bestIdx;
    if (!ref_project(pKF, Rcw, tcw, Ow, pMP, th, u, v, radius, level)) continue;
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

static int ref_fuse_scw(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
                        vector<MapPoint*>& vpReplacePoint) {
  cv::Mat Rcw = Scw.rowRange(0, 3).colRange(0, 3);
  cv::Mat tcw = Scw.rowRange(0, 3).col(3);
  cv::Mat Ow = -Rcw.t() * tcw;
  int nFused = 0;
  for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
    MapPoint* pMP = vpPoints[iMP];
    if (!pMP || pMP->isBad() || pKF->GetMapPoint(pMP->GetIndexInKeyFrame(pKF))) continue;
    float u, v, radius;
    int level, bestIdx;
    if (!ref_project(pKF, Rcw, tcw, Ow, pMP, th, u, v, radius, level)) continue;
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

static int ref_sim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, const float& s12,
                    const cv::Mat& R12, const cv::Mat& t12, const float th) {
  const float& fx = pKF1->fx;
  const float& fy = pKF1->fy;
  const float& cx = pKF1->cx;
  const float& cy = pKF1->cy;
  cv::Mat R1w = pKF1->GetRotation();
  cv::Mat t1w = pKF1->GetTranslation();
  cv::Mat sR21 = (1.0 / s12) * R12.t();
  cv::Mat t21 = -sR21 * t12;
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
    cv::Mat p3Dw = pMP1->GetWorldPos();
    cv::Mat p3Dc1 = R1w * p3Dw + t1w;
    cv::Mat p3Dc2 = sR21 * p3Dc1 + t21;
    if (p3Dc2.at<float>(2) < 0.0f) continue;
    float invz = 1.0f / p3Dc2.at<float>(2);
    float x = p3Dc2.at<float>(0) * invz;
    float y = p3Dc2.at<float>(1) * invz;
    float u = fx * x + cx;
    float v = fy * y + cy;
    if (!pKF2->IsInImage(u, v)) continue;
    float dist = cv::norm(p3Dc2);
    if (dist < pMP1->GetMinDistanceInvariance() || dist > pMP1->GetMaxDistanceInvariance()) continue;
    int predictedLevel = pMP1->PredictScale(dist, pKF2);
    float radius = th * pKF2->mvScaleFactors[predictedLevel];
    const cv::Mat dMP1 = pMP1->GetDescriptor();
    int bestIdx2;
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

// ---------------------------------------------------------------- the scene
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 2654435761u + 88172645463325252ull) {}
  uint32_t next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return (uint32_t)(s >> 16);
  }
  double uni() { return (next() & 0xFFFFFF) / (double)0x1000000; }
  double uni(double a, double b) { return a + (b - a) * uni(); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Scene {
  vector<KeyFrame*> kfs;
  vector<MapPoint*> cand;      // the candidate list handed to Fuse
  vector<MapPoint*> all;       // every map point (owner)
  ~Scene() {
    for (auto k : kfs) delete k;
    for (auto m : all) delete m;
  }
};

static cv::Mat pose(double ay, double tx, double ty, double tz) {
  cv::Mat T(4, 4, CV_32F);
  const float c = (float)cos(ay), s = (float)sin(ay);
  const float v[16] = {c, 0, s, (float)tx, 0, 1, 0, (float)ty, -s, 0, c, (float)tz, 0, 0, 0, 1};
  for (int i = 0; i < 16; ++i) T.at<float>(i / 4, i % 4) = v[i];
  return T;
}

static void flip_bits(Rng& g, uint8_t* d, int k) {
  for (int i = 0; i < k; ++i) {
    const int b = g.below(256);
    d[b >> 3] ^= (uint8_t)(1 << (b & 7));
  }
}

// nkf keyframes looking at ncand candidate map points (seen from somewhere
// else: not in any of these keyframes, except a few planted ones) plus clutter.
// A keyframe has, for about 70 % of the candidates, a feature at the point's
// projection plus noise with its descriptor a few bits off, at the predicted
// octave; such a feature is free, or held by a resident map point with more or
// fewer observations than the candidate, now and then a bad one.  With
// resident_candidates a few candidates already sit in keyframe 0 (and can be
// the target of another candidate's Replace there).
static void build(Scene& S, uint64_t seed, int nkf, int ncand, int nclutter, bool resident_candidates = true) {
  Rng g(seed);
  long next_id = 1;
  vector<float> sf(8, 1.0f);
  for (int i = 1; i < 8; ++i) sf[i] = sf[i - 1] * 1.2f;
  for (int p = 0; p < nkf; ++p) {
    KeyFrame* kf = new KeyFrame;
    kf->id = p;
    kf->mvScaleFactors = sf;
    kf->Tcw = pose(g.uni(-0.08, 0.08), g.uni(-0.3, 0.3), g.uni(-0.1, 0.1), g.uni(-0.2, 0.2));
    S.kfs.push_back(kf);
  }
  vector<MapPoint*> pts;
  for (int i = 0; i < ncand; ++i) {
    MapPoint* mp = new MapPoint;
    mp->id = next_id++;
    mp->pos.create(3, 1, CV_32F);
    const double z = g.uni(4.0, 10.0);
    mp->pos.at<float>(0) = (float)(g.uni(-0.55, 0.55) * z);
    mp->pos.at<float>(1) = (float)(g.uni(-0.42, 0.42) * z);
    mp->pos.at<float>(2) = (float)z;
    mp->desc.create(1, 32, CV_8U);
    for (int b = 0; b < 32; ++b) mp->desc.ptr(0)[b] = (uint8_t)g.below(256);
    mp->mfMaxDistance = (float)(z * pow(1.2, g.below(8)) * g.uni(0.9, 1.0));
    mp->mfMinDistance = mp->mfMaxDistance / sf[7];
    mp->nObs = 2 + g.below(4);
    mp->bad = g.uni() < 0.04;
    S.all.push_back(mp);
    pts.push_back(mp);
  }
  for (KeyFrame* kf : S.kfs) {
    vector<cv::KeyPoint> keys;
    vector<vector<uint8_t> > descs;
    vector<MapPoint*> held;
    cv::Mat Rcw = kf->GetRotation(), tcw = kf->GetTranslation(), Ow = kf->GetCameraCenter();
    auto add = [&](float u, float v, int oct, const uint8_t* d, MapPoint* h) {
      keys.push_back(cv::KeyPoint(u, v, 31.0f, 0.0f, 0.0f, oct));
      descs.push_back(vector<uint8_t>(d, d + 32));
      held.push_back(h);
    };
    for (MapPoint* mp : pts) {
      if (g.uni() < 0.3) continue;
      cv::Mat pc = Rcw * mp->pos + tcw;
      const float z = pc.at<float>(2);
      if (z <= 0) continue;
      const float u = kf->fx * pc.at<float>(0) / z + kf->cx, v = kf->fy * pc.at<float>(1) / z + kf->cy;
      const float dist = (float)cv::norm(mp->pos - Ow);
      int lvl = mp->PredictScale(dist, kf);
      const int oct = g.uni() < 0.75 ? lvl : lvl > 0 && g.uni() < 0.7 ? lvl - 1 : (lvl + 2) % 8;
      uint8_t d[32];
      memcpy(d, mp->desc.ptr(0), 32);
      flip_bits(g, d, g.below(9));
      MapPoint* h = nullptr;
      const double r = g.uni();
      if (r < 0.5) {  // a resident map point holds the feature
        h = new MapPoint;
        h->id = next_id++;
        h->pos = mp->pos.clone();
        h->desc.create(1, 32, CV_8U);
        memcpy(h->desc.ptr(0), d, 32);
        h->mfMaxDistance = mp->mfMaxDistance;
        h->mfMinDistance = mp->mfMinDistance;
        h->nObs = g.below(7);
        h->bad = g.uni() < 0.1;
        S.all.push_back(h);
      }
      const float s = 0.7f * sf[oct];
      add(u + (float)g.uni(-s, s), v + (float)g.uni(-s, s), oct, d, h);
      if (g.uni() < 0.2) {  // an exact copy a few pixels away: a tie
        add(u + (float)g.uni(-s, s) + (g.uni() < 0.5 ? 2.0f : -2.0f), v + (float)g.uni(-s, s), oct, d, nullptr);
      }
    }
    for (int i = 0; i < nclutter; ++i) {
      uint8_t d[32];
      for (int b = 0; b < 32; ++b) d[b] = (uint8_t)g.below(256);
      add((float)g.uni(-6, 646), (float)g.uni(-6, 486), g.below(8), d, nullptr);
    }
    // shuffle so that index order is not planting order
    const int n = (int)keys.size();
    vector<int> perm(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(perm[i], perm[g.below(i + 1)]);
    kf->N = n;
    kf->mvKeysUn.resize(n);
    kf->mDescriptors.create(n, 32, CV_8U);
    kf->mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; ++i) {
      kf->mvKeysUn[i] = keys[perm[i]];
      memcpy(kf->mDescriptors.ptr(i), descs[perm[i]].data(), 32);
      MapPoint* h = held[perm[i]];
      if (h) {
        kf->mvpMapPoints[i] = h;
        h->obs[kf] = i;
        if (h->nObs < 1) h->nObs = 1;
      }
    }
    kf->AssignFeaturesToGrid();
  }
  // the candidate list: nulls, a duplicate now and then, and a few candidates
  // already in keyframe 0 (on a free feature)
  for (MapPoint* mp : pts) {
    if (g.uni() < 0.05) S.cand.push_back(nullptr);
    S.cand.push_back(mp);
    if (g.uni() < 0.08) S.cand.push_back(mp);
    if (g.uni() < 0.05 && resident_candidates) {
      KeyFrame* kf = S.kfs[0];
      for (int i = 0; i < kf->N; ++i)
        if (!kf->mvpMapPoints[i]) {
          kf->mvpMapPoints[i] = mp;
          mp->obs[kf] = i;
          break;
        }
    }
  }
}

static void dump(FILE* o, const char* mode, char side, int ret, Scene& S, const vector<MapPoint*>* out) {
  fprintf(o, "%s %c RET %d\n", mode, side, ret);
  for (const auto& e : g_events) fprintf(o, "%s %c EV %s\n", mode, side, e.c_str());
  g_events.clear();
  for (KeyFrame* kf : S.kfs)
    for (int i = 0; i < kf->N; ++i)
      if (kf->GetMapPoint(i)) fprintf(o, "%s %c MP %ld %d %ld\n", mode, side, kf->id, i, kf->GetMapPoint(i)->id);
  if (out)
    for (size_t i = 0; i < out->size(); ++i)
      if ((*out)[i]) fprintf(o, "%s %c OUT %zu %ld\n", mode, side, i, (*out)[i]->id);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint64_t seed = strtoull(argv[1], nullptr, 10);
  FILE* o = fopen(argv[2], "w");
  if (!o) return 2;
  try {
    ORBmatcher matcher(0.8, true);
    for (int side = 0; side < 2; ++side) {
      const char c = side ? 'D' : 'H';
      {  // Fuse(pKF, vpMapPoints, th)
        Scene S;
        build(S, seed, 1, 400, 300);
        KeyFrame* pKFi = S.kfs[0];
        const int n = side ? matcher.Fuse(pKFi, S.cand) : ref_fuse(pKFi, S.cand, 3.0);
        dump(o, "FUSE", c, n, S, nullptr);
      }
      {  // Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
        Scene S;
        build(S, seed + 1, 1, 400, 300);
        KeyFrame* pKF = S.kfs[0];
        cv::Mat Scw = pKF->Tcw.clone();
        vector<MapPoint*> vpReplacePoints(S.cand.size(), static_cast<MapPoint*>(nullptr));
        const int n = side ? matcher.Fuse(pKF, Scw, S.cand, 4, vpReplacePoints)
                           : ref_fuse_scw(pKF, Scw, S.cand, 4, vpReplacePoints);
        dump(o, "SCW", c, n, S, &vpReplacePoints);
      }
      {  // SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
        Scene S;
        build(S, seed + 2, 2, 400, 300);
        KeyFrame *pKF1 = S.kfs[0], *pKF2 = S.kfs[1];
        // KF1's map points are the searchers: give its free features the candidates
        size_t at = 0;
        for (int i = 0; i < pKF1->N && at < S.cand.size(); ++i)
          if (!pKF1->mvpMapPoints[i]) {
            while (at < S.cand.size() && !S.cand[at]) ++at;
            if (at < S.cand.size()) pKF1->mvpMapPoints[i] = S.cand[at++];
          }
        // T12 = T1w * Tw2 with a scale close to 1
        cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
        cv::Mat R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
        cv::Mat R12 = R1w * R2w.t();
        cv::Mat t12 = -R12 * t2w + t1w;
        const float s12 = 1.01f;
        vector<MapPoint*> vpMatches12(pKF1->N, static_cast<MapPoint*>(nullptr));
        for (int i = 0; i < pKF1->N; i += 9) vpMatches12[i] = pKF2->GetMapPoint(i % pKF2->N);
        const int n = side ? matcher.SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, 7.5)
                           : ref_sim3(pKF1, pKF2, vpMatches12, s12, R12, t12, 7.5);
        dump(o, "SIM3", c, n, S, &vpMatches12);
      }
      {  // the first loop of SearchInNeighbors: every target keyframe.  No
         // candidate is resident anywhere, so no Replace target is a later query
        Scene S;
        build(S, seed + 3, 5, 400, 250, false);
        int n = 0;
        if (side) {
          n = matcher.Fuse(S.kfs, S.cand);
        } else {
          for (KeyFrame* pKFi : S.kfs) n += ref_fuse(pKFi, S.cand, 3.0);
        }
        dump(o, "BATCH", c, n, S, nullptr);
      }
    }
  } catch (const cv::Exception& e) {
    fprintf(stderr, "cv::Exception %d: %s\n", e.code, e.what());
    fclose(o);
    return 1;
  }
  fclose(o);
  return 0;
}

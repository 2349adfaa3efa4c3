// KeyFrameDatabase of cpp/orbslam2_compat.hpp against a straight host loop
// written from src/KeyFrameDatabase.cc (per-word lists, the two Detect*
// members as they stand there, an L1 score as an ordered merge), on two
// copies of the same stand-in KeyFrame / Frame classes and covisibility
// graph, through one sequence of adds, loop queries, relocalisation queries
// and an erase.  After every step both sides print the returned candidates
// and the six members of every keyframe ("H ..." the host loop, "D ..." the
// compat class); the host loop also prints what the test's non-vacuity
// conditions need ("X ...").
//
//   bowdb_compat_main <seed> <out file> <vocabulary file to write> [host]
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <list>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "orbslam2_compat.hpp"

struct KeyFrame {
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
  long unsigned int mnLoopQuery = 0;
  int mnLoopWords = 0;
  float mLoopScore = 0.25f;  // planted: a stale read shows
  long unsigned int mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0.25f;
  std::vector<KeyFrame*> neigh;  // best covisibility first
  std::set<KeyFrame*> GetConnectedKeyFrames() const { return std::set<KeyFrame*>(neigh.begin(), neigh.end()); }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int N) const {
    return (int)neigh.size() < N ? neigh : std::vector<KeyFrame*>(neigh.begin(), neigh.begin() + N);
  }
};

struct Frame {
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
};

static FILE* g_out = nullptr;
static int g_step = 0;

// ----------------------------------------------------------------- host loop
static double ScoreL1(const DBoW2::BowVector& v1, const DBoW2::BowVector& v2) {
  DBoW2::BowVector::const_iterator a = v1.begin(), b = v2.begin();
  double score = 0;
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) {
      score += fabs(a->second - b->second) - fabs(a->second) - fabs(b->second);
      ++a;
      ++b;
    } else if (a->first < b->first) {
      a = v1.lower_bound(b->first);
    } else {
      b = v2.lower_bound(a->first);
    }
  }
  return -score / 2.0;
}

struct HostDatabase {
  std::vector<std::list<KeyFrame*> > mvInvertedFile;
  explicit HostDatabase(size_t nwords) : mvInvertedFile(nwords) {}

  void add(KeyFrame* pKF) {
    for (DBoW2::BowVector::const_iterator vit = pKF->mBowVec.begin(); vit != pKF->mBowVec.end(); vit++)
      mvInvertedFile[vit->first].push_back(pKF);
  }
  void erase(KeyFrame* pKF) {
    for (DBoW2::BowVector::const_iterator vit = pKF->mBowVec.begin(); vit != pKF->mBowVec.end(); vit++) {
      std::list<KeyFrame*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KeyFrame*>::iterator lit = lKFs.begin(); lit != lKFs.end(); lit++)
        if (pKF == *lit) {
          lKFs.erase(lit);
          break;
        }
    }
  }

  std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore) {
    std::set<KeyFrame*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::list<KeyFrame*> lKFsSharingWords;
    int connected_sharing = 0, stamped = 0;
    for (DBoW2::BowVector::const_iterator vit = pKF->mBowVec.begin(); vit != pKF->mBowVec.end(); vit++) {
      std::list<KeyFrame*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KeyFrame*>::iterator lit = lKFs.begin(); lit != lKFs.end(); lit++) {
        KeyFrame* pKFi = *lit;
        if (pKFi->mnLoopQuery != pKF->mnId) {
          pKFi->mnLoopWords = 0;
          if (!spConnectedKeyFrames.count(pKFi)) {
            pKFi->mnLoopQuery = pKF->mnId;
            lKFsSharingWords.push_back(pKFi);
          } else {
            ++connected_sharing;
          }
        } else if (!std::count(lKFsSharingWords.begin(), lKFsSharingWords.end(), pKFi)) {
          ++stamped;
        }
        pKFi->mnLoopWords++;
      }
    }
    fprintf(g_out, "X %d LOOP connected_sharing %d stamped_before %d\n", g_step, connected_sharing, stamped);
    if (lKFsSharingWords.empty()) return std::vector<KeyFrame*>();

    std::list<std::pair<float, KeyFrame*> > lScoreAndMatch;
    int maxCommonWords = 0;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++)
      if ((*lit)->mnLoopWords > maxCommonWords) maxCommonWords = (*lit)->mnLoopWords;
    int minCommonWords = maxCommonWords * 0.8f;
    int under = 0;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
      KeyFrame* pKFi = *lit;
      if (pKFi->mnLoopWords > minCommonWords) {
        float si = ScoreL1(pKF->mBowVec, pKFi->mBowVec);
        pKFi->mLoopScore = si;
        if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      } else {
        ++under;
      }
    }
    fprintf(g_out, "X %d GATE under %d of %d\n", g_step, under, (int)lKFsSharingWords.size());
    if (lScoreAndMatch.empty()) return std::vector<KeyFrame*>();

    std::list<std::pair<float, KeyFrame*> > lAccScoreAndMatch;
    float bestAccScore = minScore;
    int best_changed = 0;
    for (std::list<std::pair<float, KeyFrame*> >::iterator it = lScoreAndMatch.begin(); it != lScoreAndMatch.end();
         it++) {
      KeyFrame* pKFi = it->second;
      std::vector<KeyFrame*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = it->first;
      KeyFrame* pBestKF = pKFi;
      for (std::vector<KeyFrame*>::iterator vit = vpNeighs.begin(); vit != vpNeighs.end(); vit++) {
        KeyFrame* pKF2 = *vit;
        if (pKF2->mnLoopQuery == pKF->mnId && pKF2->mnLoopWords > minCommonWords) {
          accScore += pKF2->mLoopScore;
          if (pKF2->mLoopScore > bestScore) {
            pBestKF = pKF2;
            bestScore = pKF2->mLoopScore;
          }
        }
      }
      if (pBestKF != pKFi) ++best_changed;
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    fprintf(g_out, "X %d BEST changed %d\n", g_step, best_changed);
    return Retain(lAccScoreAndMatch, 0.75f * bestAccScore);
  }

  std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F) {
    std::list<KeyFrame*> lKFsSharingWords;
    for (DBoW2::BowVector::const_iterator vit = F->mBowVec.begin(); vit != F->mBowVec.end(); vit++) {
      std::list<KeyFrame*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KeyFrame*>::iterator lit = lKFs.begin(); lit != lKFs.end(); lit++) {
        KeyFrame* pKFi = *lit;
        if (pKFi->mnRelocQuery != F->mnId) {
          pKFi->mnRelocWords = 0;
          pKFi->mnRelocQuery = F->mnId;
          lKFsSharingWords.push_back(pKFi);
        }
        pKFi->mnRelocWords++;
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KeyFrame*>();
    int maxCommonWords = 0;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++)
      if ((*lit)->mnRelocWords > maxCommonWords) maxCommonWords = (*lit)->mnRelocWords;
    int minCommonWords = maxCommonWords * 0.8f;
    std::list<std::pair<float, KeyFrame*> > lScoreAndMatch;
    std::set<KeyFrame*> scored;
    for (std::list<KeyFrame*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
      KeyFrame* pKFi = *lit;
      if (pKFi->mnRelocWords > minCommonWords) {
        float si = ScoreL1(F->mBowVec, pKFi->mBowVec);
        pKFi->mRelocScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
        scored.insert(pKFi);
      }
    }
    fprintf(g_out, "X %d GATE under %d of %d\n", g_step, (int)(lKFsSharingWords.size() - scored.size()),
            (int)lKFsSharingWords.size());
    if (lScoreAndMatch.empty()) return std::vector<KeyFrame*>();
    std::list<std::pair<float, KeyFrame*> > lAccScoreAndMatch;
    float bestAccScore = 0;
    int best_changed = 0, stale = 0;
    for (std::list<std::pair<float, KeyFrame*> >::iterator it = lScoreAndMatch.begin(); it != lScoreAndMatch.end();
         it++) {
      KeyFrame* pKFi = it->second;
      std::vector<KeyFrame*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KeyFrame* pBestKF = pKFi;
      for (std::vector<KeyFrame*>::iterator vit = vpNeighs.begin(); vit != vpNeighs.end(); vit++) {
        KeyFrame* pKF2 = *vit;
        if (pKF2->mnRelocQuery != F->mnId) continue;
        const float before = accScore;
        accScore += pKF2->mRelocScore;
        if (!scored.count(pKF2) && accScore != before) ++stale;  // a score from an earlier query, or the planted one
        if (pKF2->mRelocScore > bestScore) {
          pBestKF = pKF2;
          bestScore = pKF2->mRelocScore;
        }
      }
      if (pBestKF != pKFi) ++best_changed;
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    fprintf(g_out, "X %d BEST changed %d\n", g_step, best_changed);
    fprintf(g_out, "X %d STALE changed %d\n", g_step, stale);
    return Retain(lAccScoreAndMatch, 0.75f * bestAccScore);
  }

  static std::vector<KeyFrame*> Retain(std::list<std::pair<float, KeyFrame*> >& lAccScoreAndMatch,
                                       float minScoreToRetain) {
    std::set<KeyFrame*> spAlreadyAddedKF;
    std::vector<KeyFrame*> vpCandidates;
    for (std::list<std::pair<float, KeyFrame*> >::iterator it = lAccScoreAndMatch.begin();
         it != lAccScoreAndMatch.end(); it++)
      if (it->first > minScoreToRetain) {
        KeyFrame* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    return vpCandidates;
  }
};

// ------------------------------------------------------------------ the scene
enum { NKF = 26, PLACES = 4, PLACE_WORDS = 40, UNIVERSE = 400 };

static DBoW2::BowVector MakeBow(std::mt19937& rng, int place, int from_place, int random) {
  std::map<unsigned int, double> m;
  while ((int)m.size() < from_place) m[(unsigned)(place * 100 + rng() % PLACE_WORDS)] = 1.0 + rng() % 1000;
  const size_t want = m.size() + random;
  while (m.size() < want) m[(unsigned)(rng() % UNIVERSE)] = 1.0 + rng() % 1000;
  double norm = 0;
  for (auto& e : m) norm += e.second;
  DBoW2::BowVector v;
  for (auto& e : m) v.insert(v.end(), std::make_pair(e.first, e.second / norm));  // L1-normalised
  return v;
}

static std::vector<KeyFrame> MakeGraph(unsigned seed) {
  std::mt19937 rng(seed);
  std::vector<KeyFrame> kfs(NKF);
  for (int i = 0; i < NKF; ++i) {
    kfs[i].mnId = 10 + i;
    kfs[i].mBowVec = MakeBow(rng, (i / 6) % PLACES, 22, 6);
  }
  const int order[4] = {1, -1, 2, -2};  // best covisibility first
  for (int i = 0; i < NKF; ++i)
    for (int d : order)
      if (i + d >= 0 && i + d < NKF) kfs[i].neigh.push_back(&kfs[i + d]);
  return kfs;
}

static void WriteVocabulary(const char* path) {  // k = 10, L = 3: 1000 words, L1 scoring
  FILE* f = fopen(path, "w");
  fprintf(f, "10 3 0 0\n");
  std::mt19937 rng(5);
  int id = 0;
  std::vector<int> level(1, 0);
  for (int L = 1; L <= 3; ++L) {
    std::vector<int> next;
    for (int p : level)
      for (int c = 0; c < 10; ++c) {
        fprintf(f, "%d %d", p, L == 3 ? 1 : 0);
        for (int b = 0; b < 32; ++b) fprintf(f, " %u", (unsigned)(rng() & 255));
        fprintf(f, " %g\n", L == 3 ? 1.0 : 0.0);
        next.push_back(++id);
      }
    level.swap(next);
  }
  fclose(f);
}

static unsigned Bits(float x) {
  unsigned u;
  memcpy(&u, &x, 4);
  return u;
}

static void Report(const char* side, const std::vector<KeyFrame*>& ret, const std::vector<KeyFrame>& kfs) {
  fprintf(g_out, "%s RET %d %d\n", side, g_step, (int)ret.size());
  for (size_t i = 0; i < ret.size(); ++i) fprintf(g_out, "%s C %d %d %lu\n", side, g_step, (int)i, ret[i]->mnId);
  for (const KeyFrame& k : kfs)
    fprintf(g_out, "%s K %d %lu %lu %d %08x %lu %d %08x\n", side, g_step, k.mnId, k.mnLoopQuery, k.mnLoopWords,
            Bits(k.mLoopScore), k.mnRelocQuery, k.mnRelocWords, Bits(k.mRelocScore));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const unsigned seed = (unsigned)atoi(argv[1]);
  g_out = fopen(argv[2], "w");
  if (!g_out) return 2;
  const bool both = !(argc > 4 && !strcmp(argv[4], "host"));  // "host": the host loop alone, no GPU
  std::unique_ptr<ORB_SLAM2::ORBVocabulary> voc;
  std::unique_ptr<ORB_SLAM2::KeyFrameDatabase<KeyFrame, Frame> > dev;
  if (both) {
    WriteVocabulary(argv[3]);
    voc.reset(new ORB_SLAM2::ORBVocabulary());
    if (!voc->loadFromTextFile(argv[3]) || voc->size() != 1000) return 3;
    dev.reset(new ORB_SLAM2::KeyFrameDatabase<KeyFrame, Frame>(*voc));
  }

  std::vector<KeyFrame> H = MakeGraph(seed), D = MakeGraph(seed);
  HostDatabase host(1000);
  std::mt19937 rng(seed + 1);
  std::vector<Frame> frames(3);
  for (int i = 0; i < 3; ++i) {
    frames[i].mnId = 100 + i;
    frames[i].mBowVec = MakeBow(rng, i == 2 ? 2 : 1, 24, 8);
  }

  // ORBVocabulary::score against the host merge, one by one and batched
  if (both) {
    std::vector<const DBoW2::BowVector*> many;
    for (const KeyFrame& k : H) many.push_back(&k.mBowVec);
    std::vector<double> s;
    voc->score(H[7].mBowVec, many, s);
    int differ = 0;
    for (size_t i = 0; i < many.size(); ++i) {
      const double want = ScoreL1(H[7].mBowVec, *many[i]);
      if (memcmp(&want, &s[i], 8) != 0) ++differ;
    }
    const double one = voc->score(H[7].mBowVec, H[8].mBowVec), want = ScoreL1(H[7].mBowVec, H[8].mBowVec);
    if (memcmp(&one, &want, 8) != 0) ++differ;
    fprintf(g_out, "X 0 SCORE differ %d\n", differ);
  }

  auto step_add = [&](int i) {
    host.add(&H[i]);
    if (both) dev->add(&D[i]);
  };
  auto step_loop = [&](int i, float minScore) {
    ++g_step;
    Report("H", host.DetectLoopCandidates(&H[i], minScore), H);
    if (both) Report("D", dev->DetectLoopCandidates(&D[i], minScore), D);
  };
  auto step_reloc = [&](int f) {
    ++g_step;
    Frame fh = frames[f], fd = frames[f];
    Report("H", host.DetectRelocalizationCandidates(&fh), H);
    if (both) Report("D", dev->DetectRelocalizationCandidates(&fd), D);
  };

  for (int i = 0; i < 20; ++i) step_add(i);
  step_loop(20, 0.02f);  // 1: (a) its neighbours 18, 19 are stored and share words
  step_loop(20, 0.02f);  // 2: (b) the same id again: everything is stamped, nothing returned
  step_add(20);
  step_add(21);
  step_loop(23, 0.02f);  // 3
  step_reloc(0);         // 4: (c) neighbours under the gate hold the planted score
  step_reloc(1);         // 5: ... and now scores of query 4
  host.erase(&H[9]);
  if (both) dev->erase(&D[9]);
  host.erase(&H[25]);  // never added: a no-op on both sides
  if (both) dev->erase(&D[25]);
  step_reloc(2);         // 6
  step_loop(12, 0.02f);  // 7: a query from the middle: neighbours on both sides excluded
  step_add(9);           // back again: behind everything in every list
  step_loop(24, 0.01f);  // 8
  step_reloc(0);         // 9: the id of step 4 again: stamped keyframes only count on
  fclose(g_out);
  return 0;
}

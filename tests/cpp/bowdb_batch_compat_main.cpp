// KeyFrameDatabase::DetectRelocalizationCandidates(const std::vector<FR*>&) of
// cpp/orbslam2_compat.hpp -- one batched query, then the host step frame after
// frame -- against the single form called frame after frame on a second copy
// of the same graph.  The stand-in KeyFrame / Frame classes, the covisibility
// graph, the BowVectors and the vocabulary file are those of
// bowdb_compat_main.cpp, included as it stands (its main renamed away).
// Both sides print the candidates of every frame and, at the end, the six
// members of every keyframe ("H ..." the single calls, "D ..." the batched
// one); "X ..." lines carry what the test's non-vacuity conditions need: a
// third copy takes the single calls in reverse order, which must leave other
// members behind (the frames' host steps read what earlier ones wrote).
//
//   bowdb_batch_compat_main <seed> <out file> <vocabulary file to write>
#define main bowdb_compat_sequence_main
#include "bowdb_compat_main.cpp"
#undef main

typedef ORB_SLAM2::KeyFrameDatabase<KeyFrame, Frame> Database;

static void ReportFrame(const char* side, int f, const std::vector<KeyFrame*>& ret) {
  fprintf(g_out, "%s RET %d %d\n", side, f, (int)ret.size());
  for (size_t i = 0; i < ret.size(); ++i) fprintf(g_out, "%s C %d %d %lu\n", side, f, (int)i, ret[i]->mnId);
}

static void ReportMembers(const char* side, const std::vector<KeyFrame>& kfs) {
  for (const KeyFrame& k : kfs)
    fprintf(g_out, "%s K %lu %lu %d %08x %lu %d %08x\n", side, k.mnId, k.mnLoopQuery, k.mnLoopWords,
            Bits(k.mLoopScore), k.mnRelocQuery, k.mnRelocWords, Bits(k.mRelocScore));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const unsigned seed = (unsigned)atoi(argv[1]);
  g_out = fopen(argv[2], "w");
  if (!g_out) return 2;
  WriteVocabulary(argv[3]);
  ORB_SLAM2::ORBVocabulary voc;
  if (!voc.loadFromTextFile(argv[3]) || voc.size() != 1000) return 3;

  enum { STORED = 24, NFRAMES = 4 };
  std::vector<KeyFrame> H = MakeGraph(seed), D = MakeGraph(seed), R = MakeGraph(seed);
  Database single(voc), batched(voc), reversed(voc);
  for (int i = 0; i < STORED; ++i) {
    single.add(&H[i]);
    batched.add(&D[i]);
    reversed.add(&R[i]);
  }
  std::mt19937 rng(seed + 1);
  std::vector<Frame> frames(NFRAMES);
  const int place[NFRAMES] = {1, 1, 2, 1};
  for (int i = 0; i < NFRAMES; ++i) {
    frames[i].mnId = 100 + i;
    frames[i].mBowVec = MakeBow(rng, place[i], 24, 8);
  }
  frames[3].mnId = frames[0].mnId;  // the first id again: its stamped keyframes only count on

  std::vector<Frame> fh = frames, fd = frames, fr = frames;
  int candidates = 0;
  for (int f = 0; f < NFRAMES; ++f) {
    const std::vector<KeyFrame*> ret = single.DetectRelocalizationCandidates(&fh[f]);
    candidates += (int)ret.size();
    ReportFrame("H", f, ret);
  }
  ReportMembers("H", H);

  std::vector<Frame*> list;
  for (int f = 0; f < NFRAMES; ++f) list.push_back(&fd[f]);
  const std::vector<std::vector<KeyFrame*> > rets = batched.DetectRelocalizationCandidates(list);
  if ((int)rets.size() != NFRAMES) return 4;
  for (int f = 0; f < NFRAMES; ++f) ReportFrame("D", f, rets[f]);
  ReportMembers("D", D);
  // an empty list, and a list of one
  if (!batched.DetectRelocalizationCandidates(std::vector<Frame*>()).empty()) return 5;

  for (int f = NFRAMES - 1; f >= 0; --f) reversed.DetectRelocalizationCandidates(&fr[f]);
  int differ = 0, stamped = 0, scored = 0;
  for (size_t i = 0; i < H.size(); ++i) {
    differ += H[i].mnRelocQuery != R[i].mnRelocQuery || H[i].mnRelocWords != R[i].mnRelocWords ||
              Bits(H[i].mRelocScore) != Bits(R[i].mRelocScore);
    stamped += H[i].mnRelocQuery != 0;
    scored += Bits(H[i].mRelocScore) != Bits(0.25f);
  }
  fprintf(g_out, "X candidates %d\n", candidates);
  fprintf(g_out, "X reversed_differ %d\n", differ);
  fprintf(g_out, "X stamped %d scored %d\n", stamped, scored);
  fclose(g_out);
  return 0;
}

// api_match.hip -- C ABI of the matcher: ORBmatcher::SearchByBoW(KF, KF)
// and DescriptorDistance drop-ins, and the batched frame-pair matcher.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/orbx.h"
#include "call_arena.h"
#include "match_fold_hash.h"
#include "match_internal.h"

namespace orbx {
__global__ void k_match_candidates(const MProblem*, const MNodePair*, int, int, uint2*, int4*,
                                   int2*);
template <int NW>
__global__ void k_match_cand_rows(const MProblem*, const MNodePair*, const uint4*, const uint32_t*,
                                  uint2*, int4*, int2*);
__global__ void k_match_gather2(const MProblem*, const MNodePair*, uint4*, uint32_t*);
typedef int v4i_ __attribute__((ext_vector_type(4)));
template <int NK, bool FOLD>
__global__ void k_match_expand2(const MProblem*, const MNodePair*, v4i_*, const MFoldPair*,
                                const uint32_t*);
template <int NK, int RT, bool PK, int CS, bool FOLD>
__global__ void k_match_cand_mfma(const MProblem*, const MNodePair*, const v4i_*, uint2*, int4*,
                                  int2*, const MFoldPair*, const uint32_t*);

__global__ void k_match_resolve(const MProblem*, const MNodePair*, int, int, const uint2*,
                                const int4*, int2*);
__global__ void k_match_resolve_spec(const MProblem*, const MNodePair*, int, const uint2*,
                                     const int4*, int2*, int);
__global__ void k_match_finalize(const MProblem*, const MNodePair*, const int4*, int2*, int*,
                                 const int*);
__global__ void k_match_setup(MProblem*, MNodePair*, MFoldPair*, int, const orbx_keypoint*,
                              const uint8_t*, const orbx_keypoint*, const uint8_t*, int, int, int,
                              const uint32_t*, int32_t*, int*, float, int, int*);
__global__ void k_match_select(MProblem*, MNodePair*, MFoldPair*, const orbx_keypoint*, const uint8_t*,
                               const int*, const orbx_keypoint*, const uint8_t*, const int*, int, int,
                               int, int, uint32_t*, uint32_t*, uint32_t*);
__global__ void k_hamming_pairs(const uint8_t*, const uint8_t*, const int32_t*, const int32_t*,
                                int, int32_t*);
}  // namespace orbx

using namespace orbx;

#ifndef ORBM_MFMA
#define ORBM_MFMA 1 /* 0: VALU distances everywhere (profiling variant) */
#endif

namespace {

// bytes 24..31 of every descriptor zero (orbx descriptors with the
// reference's pattern): the candidate kernel may skip dwords 6-7 exactly
bool upper_bytes_zero(const uint8_t* d, int n) {
  uint64_t acc = 0;
  for (int i = 0; i < n; ++i) {
    uint64_t w;
    memcpy(&w, d + (size_t)i * 32 + 24, 8);
    acc |= w;
  }
  return acc == 0;
}

int check_frame(const orbx_bow_frame* k) {
  if (!k || k->n < 0 || k->nnodes < 0) return ORBX_ERR_ARG;
  if (k->n > 0 && (!k->desc || !k->angle)) return ORBX_ERR_ARG;
  return check_feature_vector(k->n, k->nnodes, k->node_id, k->node_off, k->feat);
}

// launch_match's device scratch, rows = list1 entries, g2 = list2 positions
struct MatchScratch {
  uint4* gdesc2 = nullptr;   // g2 x 2: list2 descriptors in node order
  uint32_t* gval2 = nullptr; // g2: their validity, or nullptr (no masks)
  void* gx2 = nullptr;       // g2 x 256 B: list2 as +-1 bytes, or nullptr (no MFMA path)
  uint2* cand = nullptr;     // rows x ORBM_T
  int4* rowinfo = nullptr;   // rows
  int2* ev = nullptr;        // rows
  int* last = nullptr;       // per KF1 feature
  int* last_off = nullptr;   // per problem: its offset in last
  // folded lists (batched plan; MFoldPair), or nullptr: whole lists
  const MFoldPair* fps = nullptr;
  const uint32_t* fmap = nullptr;
};

// one launch's extent
struct MatchShape {
  int nprob, nnp, nrows, sequential, max_n1, max_n2, max_bitmap_n2;
  bool six_words;
};

void launch_match(const MProblem* d_probs, const MNodePair* d_nps, const MatchShape& sh,
                  const MatchScratch& sc, hipStream_t s, StageTimer* timer) {
  {
    int dev = 0;
    hipGetDevice(&dev);
    set_max_dynamic_lds((const void*)k_match_resolve_spec, dev);
    set_max_dynamic_lds((const void*)k_match_resolve, dev);
  }
  if (timer) timer->begin(ORBX_STAGE_MCAND, s);
  if (sh.nrows > 0 && sh.nnp > 0) {
    // Candidates.  Both callers (bow_search, orbm_plan_match_frames) always
    // pass gdesc2 and keep max_n2 <= ORBM_MAX_N2, so only the number of
    // node pairs picks the path: the gather kernels take one grid.y row per
    // node pair, and grid.y is bounded by 65535.
    if (sh.nnp <= 65535) {
      const bool mfma = ORBM_MFMA && sc.gx2 && !sc.gval2 && sh.max_n2 > 0;
      if (mfma) {
        // distances on the matrix cores (no validity masks on this path):
        // list2 gathered straight into +-1 bytes
        v4i_* gx2 = static_cast<v4i_*>(sc.gx2);
        // a launch of fewer workgroups than CUs (one long node pair, e.g. a
        // drop-in call) splits each row tile's list 4 ways over a
        // workgroup's waves (MC_CSPLIT_WGS: below this many 128-row
        // workgroups; lists of 8+ tiles)
        const bool csplit = (size_t)sh.nnp * (size_t)((sh.max_n1 + 128 * MC_RT - 1) / (128 * MC_RT)) < (size_t)MC_CSPLIT_WGS &&
                            sh.max_n2 >= 256;
        const dim3 g1((sh.max_n1 + 128 * MC_RT - 1) / (128 * MC_RT), sh.nnp), g4((sh.max_n1 + 31) / 32, sh.nnp);
#define MC_LAUNCH(NK, PK, FOLD)                                                                         \
  do {                                                                                                  \
    hipLaunchKernelGGL((k_match_expand2<NK, FOLD>),                                                     \
                       dim3((sh.max_n2 * ORBM_EXPAND_PER_POS(NK) + 255) / 256, sh.nnp), dim3(256), 0, s, \
                       d_probs, d_nps, gx2, sc.fps, sc.fmap);                                           \
    if (csplit)                                                                                         \
      hipLaunchKernelGGL((k_match_cand_mfma<NK, 1, PK, 4, FOLD>), g4, dim3(256), 0, s, d_probs, d_nps,  \
                         gx2, sc.cand, sc.rowinfo, sc.ev, sc.fps, sc.fmap);                             \
    else                                                                                                \
      hipLaunchKernelGGL((k_match_cand_mfma<NK, MC_RT, PK, 1, FOLD>), g1, dim3(256), 0, s, d_probs,     \
                         d_nps, gx2, sc.cand, sc.rowinfo, sc.ev, sc.fps, sc.fmap);                      \
  } while (0)
        // positions in the accumulator while they fit its 2^MC_PB(NK) slots;
        // folded lists (the batched plan, match_fold_ok) in that form only
        const bool pk = ORBM_FP4 && MC_PK && sh.max_n2 <= (sh.six_words ? 1 << 14 : 1 << 13);
        const bool fold = pk && sc.fps && sc.fmap;
        if (sh.six_words) {
          if (fold)
            MC_LAUNCH(6, ORBM_FP4 != 0, ORBM_FP4 != 0);
          else if (pk)
            MC_LAUNCH(6, ORBM_FP4 != 0, false);
          else
            MC_LAUNCH(6, false, false);
        } else {
          if (fold)
            MC_LAUNCH(8, ORBM_FP4 != 0, ORBM_FP4 != 0);
          else if (pk)
            MC_LAUNCH(8, ORBM_FP4 != 0, false);
          else
            MC_LAUNCH(8, false, false);
        }
#undef MC_LAUNCH
      } else {
        // list2 descriptors gathered into node order, then two rows per lane,
        // the 4 waves splitting the positions; descriptors stream through LDS
        if (sh.max_n2 > 0)
          hipLaunchKernelGGL(k_match_gather2, dim3((sh.max_n2 + 127) / 128, sh.nnp), dim3(256), 0, s, d_probs,
                             d_nps, sc.gdesc2, sc.gval2);
        if (sh.six_words)
          hipLaunchKernelGGL(k_match_cand_rows<6>, dim3((sh.max_n1 + 127) / 128, sh.nnp), dim3(256), 0, s,
                             d_probs, d_nps, sc.gdesc2, sc.gval2, sc.cand, sc.rowinfo, sc.ev);
        else
          hipLaunchKernelGGL(k_match_cand_rows<8>, dim3((sh.max_n1 + 127) / 128, sh.nnp), dim3(256), 0, s,
                             d_probs, d_nps, sc.gdesc2, sc.gval2, sc.cand, sc.rowinfo, sc.ev);
      }
    } else {
      // more node pairs than grid.y holds: one wavefront per row, a flat grid
      hipLaunchKernelGGL(k_match_candidates, dim3((sh.nrows + 3) / 4), dim3(256), 0, s, d_probs,
                         d_nps, sh.nnp, sh.nrows, sc.cand, sc.rowinfo, sc.ev);
    }
  }
  if (timer) timer->end(ORBX_STAGE_MCAND, s);
  if (timer) timer->begin(ORBX_STAGE_MRESOLVE, s);
  const int units = sh.sequential ? sh.nprob : sh.nnp;
  if (sh.nrows > 0 && units > 0 && !sh.sequential && sh.max_bitmap_n2 <= 16384) {
    // speculative 64-row chunks; LDS = vbMatched2 bitmap + claim table
    // (+ alignment to 8 B) + the chunk's candidate slots (64 lanes x ORBM_T)
    const int n2cap = std::max(sh.max_bitmap_n2, 32);
    const size_t lds = (size_t)((((n2cap + 31) / 32 + n2cap) + 1) & ~1) * 4 + (size_t)64 * ORBM_T * sizeof(uint2);
    hipLaunchKernelGGL(k_match_resolve_spec, dim3(units), dim3(64), lds, s, d_probs, d_nps, units,
                       sc.cand, sc.rowinfo, sc.ev, n2cap);
  } else if (sh.nrows > 0 && units > 0) {
    if (sh.max_bitmap_n2 > 16384) {
      const size_t lds = (size_t)((sh.max_bitmap_n2 + 31) / 32) * 4;
      hipLaunchKernelGGL(k_match_resolve, dim3(units), dim3(64), lds, s, d_probs, d_nps, units,
                         sh.sequential, sc.cand, sc.rowinfo, sc.ev);
    } else {
      hipLaunchKernelGGL(k_match_resolve, dim3((units + 3) / 4), dim3(256), 0, s, d_probs, d_nps,
                         units, sh.sequential, sc.cand, sc.rowinfo, sc.ev);
    }
  }
  if (timer) timer->end(ORBX_STAGE_MRESOLVE, s);
  if (timer) timer->begin(ORBX_STAGE_MFINAL, s);
  hipLaunchKernelGGL(k_match_finalize, dim3(sh.nprob), dim3(256), 0, s, d_probs, d_nps, sc.rowinfo,
                     sc.ev, sc.last, sc.last_off);
  if (timer) timer->end(ORBX_STAGE_MFINAL, s);
}

// the common nodes of two FeatureVectors as node pairs, ascending
// (ORBmatcher.cc:305-350), with the totals the arena and the launch need
struct NodePairs {
  std::vector<MNodePair> nps;
  int rows = 0, g2 = 0, max_n1 = 0, max_n2 = 0;
};

int node_pair_table(const orbx_bow_frame* kf1, const orbx_bow_frame* kf2, NodePairs& T) {
  return for_common_nodes(
      kf1->node_id, kf1->node_off, kf1->nnodes, kf2->node_id, kf2->node_off, kf2->nnodes,
      [&](uint32_t off1, uint32_t n1, uint32_t off2, uint32_t n2) {
        if (n2 > 0xFFFF) return ORBX_ERR_UNSUPPORTED; /* 16-bit list positions */
        const MNodePair np = {0, (int)off1, (int)n1, (int)off2, (int)n2, T.rows, T.g2};
        T.rows += np.n1;
        T.g2 += np.n2;
        T.max_n1 = std::max(T.max_n1, np.n1);
        T.max_n2 = std::max(T.max_n2, np.n2);
        T.nps.push_back(np);
        return ORBX_OK;
      });
}

// node pairs may run in parallel iff no KF2 feature appears in two of them
int needs_sequential(const orbx_bow_frame* kf2, const NodePairs& T) {
  std::vector<uint8_t> seen((size_t)kf2->n, 0);
  for (const MNodePair& np : T.nps)
    if (index_repeats(seen, kf2->feat + np.off2, (size_t)np.n2)) return 1;
  return 0;
}

// one search's arena: the two frames, the problem and node-pair tables, the
// results, launch_match's scratch
struct BowSlots {
  Slot<uint8_t> desc1, desc2, val1, val2, gx2;
  Slot<float> ang1, ang2;
  Slot<uint32_t> feat1, feat2, gval2;
  Slot<MProblem> prob;
  Slot<MNodePair> nps;
  Slot<int32_t> m12;
  Slot<int> loff, nm, last;
  Slot<uint2> cand;
  Slot<int4> rowinfo;
  Slot<int2> ev;
  Slot<uint4> gdesc2;

  BowSlots(CallArena& A, const orbx_bow_frame* kf1, const orbx_bow_frame* kf2, const NodePairs& T,
           int32_t* match12, int* nmatches) {
    const size_t n1 = (size_t)kf1->n, n2 = (size_t)kf2->n, rows = (size_t)T.rows, g2 = (size_t)T.g2;
    desc1 = A.in(kf1->desc, n1 * 32);
    desc2 = A.in(kf2->desc, n2 * 32);
    ang1 = A.in(kf1->angle, n1);
    ang2 = A.in(kf2->angle, n2);
    val1 = A.in_opt(kf1->valid, n1);
    val2 = A.in_opt(kf2->valid, n2);
    feat1 = A.in(kf1->feat, kf1->nnodes ? kf1->node_off[kf1->nnodes] : 0);
    feat2 = A.in(kf2->feat, kf2->nnodes ? kf2->node_off[kf2->nnodes] : 0);
    prob = A.in<MProblem>(1);
    nps = A.in(T.nps.data(), T.nps.size());
    loff = A.in<int>(1);
    m12 = A.out(match12, n1);
    nm = A.out(nmatches, 1);
    cand = A.scratch<uint2>(rows * ORBM_T);
    rowinfo = A.scratch<int4>(rows);
    ev = A.scratch<int2>(rows);
    last = A.scratch<int>(n1);
    gdesc2 = A.scratch<uint4>(g2 * 2);
    // validity masks take the VALU path, no masks the MFMA path's +-1 bytes
    if (kf2->valid) gval2 = A.scratch<uint32_t>(g2);
    else gx2 = A.scratch<uint8_t>(g2 * 256);
  }

  // the problem table's one entry and last's offset, built in staging
  void fill(const CallArena& A, const orbx_bow_frame* kf1, const orbx_bow_frame* kf2,
            const NodePairs& T, float nnratio, int check_ori, int sequential, int th_low) const {
    MProblem P = {};  // np_begin = row_begin = 0: the one problem owns every node pair and row
    P.desc1 = A.d(desc1);
    P.desc2 = A.d(desc2);
    P.ang1 = A.d(ang1);
    P.ang2 = A.d(ang2);
    P.valid1 = A.d(val1);
    P.valid2 = A.d(val2);
    P.feat1 = A.d(feat1);
    P.feat2 = A.d(feat2);
    P.match12 = A.d(m12);
    P.nmatches = A.d(nm);
    P.ang_stride = 1;
    P.n1 = kf1->n;
    P.n2 = kf2->n;
    P.np_end = (int)T.nps.size();
    P.row_end = T.rows;
    P.check_ori = check_ori ? 1 : 0;
    P.nnratio = nnratio;
    P.sequential = sequential;
    P.dcap = orbm_dcap(nnratio, th_low);
    P.th_low = th_low;
    *A.h(prob) = P;
    *A.h(loff) = 0;
  }

  MatchScratch scratch(const CallArena& A) const {
    return MatchScratch{A.d(gdesc2), A.d(gval2), A.d(gx2),  A.d(cand),
                        A.d(rowinfo), A.d(ev),   A.d(last), A.d(loff)};
  }
};

}  // namespace

// the KF-KF search (th_low = ORBM_TH_LOW) or upstream's KF-Frame search
// (th_low = ORBM_TH_LOW + 1, i.e. bestDist1 <= TH_LOW) of kf1's rows over
// kf2's candidates: match12 indexed by kf1 feature
static int bow_search(const orbx_bow_frame* kf1, const orbx_bow_frame* kf2, float nnratio,
                      int check_ori, int device, int th_low, int32_t* match12, int* nmatches) {
  if (!nmatches || (kf1 && kf1->n > 0 && !match12)) return ORBX_ERR_ARG;
  int rc = check_frame(kf1);
  if (rc) return rc;
  rc = check_frame(kf2);
  if (rc) return rc;
  if (kf2->n > ORBM_MAX_N2) return ORBX_ERR_UNSUPPORTED;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  NodePairs T;
  rc = node_pair_table(kf1, kf2, T);
  if (rc) return rc;
  const int sequential = needs_sequential(kf2, T);
  if (kf1->n == 0) {
    *nmatches = 0;
    return ORBX_OK;
  }
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  const BowSlots S(A, kf1, kf2, T, match12, nmatches);
  rc = A.commit();
  if (rc) return rc;
  S.fill(A, kf1, kf2, T, nnratio, check_ori, sequential, th_low);
  rc = A.upload();
  if (rc) return rc;
  const MatchShape sh = {1, (int)T.nps.size(), T.rows, sequential, T.max_n1, T.max_n2, kf2->n,
                         upper_bytes_zero(kf1->desc, kf1->n) && upper_bytes_zero(kf2->desc, kf2->n)};
  launch_match(A.d(S.prob), A.d(S.nps), sh, S.scratch(A), A.stream(), nullptr);
  return A.finish();
}

extern "C" int orbm_search_by_bow(const orbx_bow_frame* kf1, const orbx_bow_frame* kf2,
                                  float nnratio, int check_ori, int device, int32_t* match12,
                                  int* nmatches) {
  return bow_search(kf1, kf2, nnratio, check_ori, device, ORBM_TH_LOW, match12, nmatches);
}

// upstream ORB-SLAM2's SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
// (this reference keeps only its stub, ORBmatcher.cc:88-119): the KF's
// features are the rows (valid = a non-null, non-bad MapPoint), the Frame's
// every feature a candidate, a claimed Frame feature is skipped, bestDist1 <=
// TH_LOW; output indexed by Frame feature.  The same device search with
// th_low = TH_LOW + 1, its row -> candidate result inverted here.
extern "C" int orbm_search_by_bow_kf_frame(const orbx_bow_frame* kf, const orbx_bow_frame* frame,
                                           float nnratio, int check_ori, int device, int32_t* match_f,
                                           int* nmatches) {
  if (!nmatches || !frame || (frame->n > 0 && !match_f)) return ORBX_ERR_ARG;
  /* the sentinel scheme assumes a second-best of 256 (upstream's initial
   * bestDist2) passes the ratio test for every acceptable best */
  if (orbm_dcap(nnratio, ORBM_TH_LOW + 1) > 256) return ORBX_ERR_UNSUPPORTED;
  /* a KF feature listed under two nodes (never in a DBoW2 FeatureVector) would
   * leave one row per KF index in the row -> candidate result while nmatches
   * counts both: rejected */
  if (kf && kf->n > 0 && kf->nnodes > 0 && kf->node_off && kf->feat) {
    std::vector<uint8_t> seen((size_t)kf->n, 0);
    if (index_repeats(seen, kf->feat, kf->node_off[kf->nnodes])) return ORBX_ERR_ARG;
  }
  orbx_bow_frame fr = *frame;
  fr.valid = nullptr;  /* every Frame feature is a candidate */
  std::vector<int32_t> m(kf && kf->n > 0 ? (size_t)kf->n : 1, -1);
  const int rc = bow_search(kf, &fr, nnratio, check_ori, device, ORBM_TH_LOW + 1, m.data(), nmatches);
  if (rc) return rc;
  for (int i = 0; i < frame->n; ++i) match_f[i] = -1;
  for (int i = 0; kf && i < kf->n; ++i)
    if (m[i] >= 0) match_f[m[i]] = i;
  return ORBX_OK;
}

extern "C" int orbm_descriptor_distance_batch(const uint8_t* a, int na, const uint8_t* b, int nb,
                                              const int32_t* ia, const int32_t* ib, int npairs,
                                              int device, int32_t* dist) {
  if (npairs < 0 || (npairs > 0 && (!a || !b || !ia || !ib || !dist))) return ORBX_ERR_ARG;
  for (int i = 0; i < npairs; ++i)
    if (ia[i] < 0 || ia[i] >= na || ib[i] < 0 || ib[i] >= nb) return ORBX_ERR_ARG;
  if (npairs == 0) return ORBX_OK;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  const auto s_a = A.in(a, (size_t)na * 32), s_b = A.in(b, (size_t)nb * 32);
  const auto s_ia = A.in(ia, (size_t)npairs), s_ib = A.in(ib, (size_t)npairs);
  const auto s_d = A.out(dist, (size_t)npairs);
  int rc = A.commit();
  if (rc) return rc;
  rc = A.upload();
  if (rc) return rc;
  hipLaunchKernelGGL(k_hamming_pairs, dim3((npairs + 255) / 256), dim3(256), 0, A.stream(), A.d(s_a),
                     A.d(s_b), A.d(s_ia), A.d(s_ib), npairs, A.d(s_d));
  return A.finish();
}

// ---------------------------------------------------------------------------
// batched frame-pair matcher
// ---------------------------------------------------------------------------
struct orbm_plan {
  int device = 0, max_pairs = 0, kcap = 0, topn = 0;
  /* ORBM_PLAN_ZERO_TAIL (opt-in, orbm_plan_set_options): the caller
   * guarantees bytes 24..31 of every descriptor are zero, as they are for
   * orbx_plan_extract outputs (static_assert on the pattern in
   * kernels_extract.hip), and the candidate kernels skip dwords 6-7.  Off by
   * default: any other descriptor source gets all 8 dwords. */
  bool six_words = false;
  bool force_valu = false; /* ORBM_PLAN_VALU: popcount kernel instead of the MFMA path */
  bool no_fold = false;    /* ORBM_PLAN_NO_FOLD: whole lists (the kernels' FOLD = false forms) */
  int last_npairs = 0;     /* orbm_plan_fold_stats: the last call's pairs */
  DevBuf<MProblem> d_probs;
  DevBuf<MNodePair> d_nps;
  /* per list (2 per pair) topn dwords each: the selection, then MFoldPair's
   * tables (fmap), then k_match_select's entry states (fst); the pairs'
   * MFoldPair records behind them -- one allocation */
  DevBuf<uint32_t> d_sel;
  size_t lists() const { return (size_t)max_pairs * 2 * topn; }
  uint32_t* d_fmap() const { return (uint32_t*)d_sel + lists(); }
  uint32_t* d_fst() const { return (uint32_t*)d_sel + 2 * lists(); }
  MFoldPair* d_fps() const { return reinterpret_cast<MFoldPair*>((uint32_t*)d_sel + 3 * lists()); }
  /* launch_match's scratch (MatchScratch) */
  DevBuf<uint4> d_gdesc2;
  DevBuf<uint8_t> d_gx2;
  DevBuf<uint2> d_cand;
  DevBuf<int4> d_rowinfo;
  DevBuf<int2> d_ev;
  DevBuf<int> d_last, d_last_off;
  StageTimer timer;
  ~orbm_plan() { hipSetDevice(device); }

  /* no validity masks (gval2); the +-1 bytes unless the popcount path is forced */
  MatchScratch scratch() const {
    uint8_t* const gx2 = force_valu ? nullptr : d_gx2;
    const bool f = fold();
    return MatchScratch{d_gdesc2, nullptr, gx2, d_cand, d_rowinfo, d_ev, d_last, d_last_off,
                        f ? (const MFoldPair*)d_fps() : nullptr, f ? (const uint32_t*)d_fmap() : nullptr};
  }

  /* identical descriptors of a list folded: the MFMA path with positions in
   * the accumulator unless ORBM_PLAN_NO_FOLD -- launch_match's own conditions
   * for that path (at most 65535 node pairs, gx2, no validity arrays, list
   * length), so the tables are built exactly when the FOLD kernels run */
  bool fold() const {
    return !no_fold && !force_valu && ORBM_MFMA && ORBM_FP4 && MC_PK && max_pairs <= 65535 &&
           topn <= (six_words ? 1 << 14 : 1 << 13);
  }
};

extern "C" int orbm_plan_create(int max_pairs, int kcap, int topn, int device, orbm_plan** out) {
  if (!out || max_pairs < 1 || kcap < 1 || topn < 1 || topn > 0xFFFF || kcap > ORBM_MAX_N2)
    return ORBX_ERR_ARG;
  *out = nullptr;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  std::unique_ptr<orbm_plan> m(new orbm_plan());
  m->device = device;
  m->max_pairs = max_pairs;
  m->kcap = kcap;
  m->topn = topn;
  const size_t P = (size_t)max_pairs, rows = P * topn;
  if (m->d_probs.alloc(P) || m->d_nps.alloc(P) ||
      m->d_sel.alloc(3 * P * 2 * topn + P * sizeof(MFoldPair) / sizeof(uint32_t)) ||
      m->d_cand.alloc(rows * ORBM_T) || m->d_gdesc2.alloc(rows * 2) || m->d_gx2.alloc(rows * 256) ||
      m->d_rowinfo.alloc(rows) || m->d_ev.alloc(rows) || m->d_last.alloc(P * kcap) ||
      m->d_last_off.alloc(P))
    return ORBX_ERR_HIP;
  *out = m.release();
  return ORBX_OK;
}

extern "C" int orbm_plan_destroy(orbm_plan* m) {
  delete m;
  return ORBX_OK;
}

extern "C" int orbm_plan_set_options(orbm_plan* m, int flags) {
  if (!m || (flags & ~(ORBM_PLAN_ZERO_TAIL | ORBM_PLAN_VALU | ORBM_PLAN_NO_FOLD))) return ORBX_ERR_ARG;
  m->six_words = (flags & ORBM_PLAN_ZERO_TAIL) != 0;
  m->force_valu = (flags & ORBM_PLAN_VALU) != 0;
  m->no_fold = (flags & ORBM_PLAN_NO_FOLD) != 0;
  return ORBX_OK;
}

extern "C" int orbm_plan_fold_stats(orbm_plan* m, int64_t* out) {
  if (!m || !out) return ORBX_ERR_ARG;
  ORBX_TRY(hipSetDevice(m->device));
  out[0] = out[1] = out[2] = out[3] = 0;
  if (m->last_npairs < 1) return ORBX_OK;
  // the per-pair counts k_match_select left; summed here, no device counter
  std::vector<MNodePair> nps(m->last_npairs);
  std::vector<MFoldPair> fps(m->last_npairs);
  ORBX_TRY(hipDeviceSynchronize());  // that call's stream may be gone by now
  ORBX_TRY(hipMemcpy(nps.data(), m->d_nps, nps.size() * sizeof(MNodePair), hipMemcpyDeviceToHost));
  ORBX_TRY(hipMemcpy(fps.data(), m->d_fps(), fps.size() * sizeof(MFoldPair), hipMemcpyDeviceToHost));
  for (int p = 0; p < m->last_npairs; ++p) {
    out[0] += nps[p].n1;
    out[1] += nps[p].n1 - fps[p].n1u;
    out[2] += nps[p].n2;
    out[3] += nps[p].n2 - fps[p].n2u;
  }
  return ORBX_OK;
}

extern "C" int orbm_plan_set_timing(orbm_plan* m, int enable) {
  if (!m) return ORBX_ERR_ARG;
  hipSetDevice(m->device);
  m->timer.reset(enable != 0);
  return ORBX_OK;
}

extern "C" int orbm_plan_stage_times(orbm_plan* m, double* ms, int* launches, int n) {
  if (!m) return ORBX_ERR_ARG;
  hipSetDevice(m->device);
  return m->timer.collect(ms, launches, n);
}

extern "C" int orbm_plan_match_frames(orbm_plan* m, int npairs, const orbx_keypoint* kps_a,
                                      const uint8_t* desc_a, const int* count_a,
                                      const orbx_keypoint* kps_b, const uint8_t* desc_b,
                                      const int* count_b, float nnratio, int check_ori,
                                      int32_t* match12, int* nmatches, void* stream) {
  if (!m || npairs < 1 || npairs > m->max_pairs || !kps_a || !desc_a || !count_a || !kps_b ||
      !desc_b || !count_b || !match12 || !nmatches)
    return ORBX_ERR_ARG;
  ORBX_TRY(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  m->timer.begin(ORBX_STAGE_MSELECT, s);
  // side B = side A one frame back (a tracker's frame against its
  // predecessor, out of one buffer): npairs + 1 frames, each selected once
  const int shifted = kps_a == kps_b + m->kcap && desc_a == desc_b + (size_t)m->kcap * 32 &&
                      count_a == count_b + 1;
  const int hbits = m->fold() ? orbm_fold_hbits(m->topn) : 0;
  const size_t fold_lds = hbits ? sizeof(uint32_t) << hbits : 0;
  hipLaunchKernelGGL(k_match_setup, dim3((npairs + 63) / 64), dim3(64), 0, s, m->d_probs,
                     m->d_nps, m->d_fps(), npairs, kps_a, desc_a, kps_b, desc_b, m->kcap, m->topn,
                     shifted, m->d_sel, match12, nmatches, nnratio, check_ori ? 1 : 0, m->d_last_off);
  hipLaunchKernelGGL(k_match_select, shifted ? dim3(npairs + 1) : dim3(npairs, 2), dim3(256), fold_lds,
                     s, m->d_probs, m->d_nps, m->d_fps(), kps_a, desc_a, count_a, kps_b, desc_b, count_b,
                     m->kcap, m->topn, shifted, hbits, m->d_sel, m->d_fmap(), m->d_fst());
  m->last_npairs = npairs;
  m->timer.end(ORBX_STAGE_MSELECT, s);
  const MatchShape sh = {npairs, npairs, npairs * m->topn, 0, m->topn, m->topn, m->kcap, m->six_words};
  launch_match(m->d_probs, m->d_nps, sh, m->scratch(), s, &m->timer);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
}

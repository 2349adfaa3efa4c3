// api_tri.hip -- C ABI of ORBmatcher::SearchForTriangulation, batched over
// the neighbour keyframes of LocalMapping::CreateNewMapPoints.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/orbx.h"
#include "call_arena.h"
#include "tri_internal.h"

namespace orbx {
__global__ void k_tri_init(const TriProblem*, int);
__global__ void k_tri_search(const TriProblem*, const TriItem*, TriFrame, int);
__global__ void k_tri_finalize(const TriProblem*, int, int);
}  // namespace orbx

using namespace orbx;

namespace {

// kf2: the frame whose level_sigma2 CheckDistEpipolarLine indexes with
// kp2.octave (ORBmatcher.cc:84)
int check_tri_frame(const orbx_tri_frame* k, bool kf2) {
  if (!k || k->n < 0 || k->nnodes < 0) return ORBX_ERR_ARG;
  if (k->n > 0 && (!k->keys || !k->desc)) return ORBX_ERR_ARG;
  if (check_feature_vector(k->n, k->nnodes, k->node_id, k->node_off, k->feat)) return ORBX_ERR_ARG;
  if (kf2) {
    if (k->nlevels < 0 || (k->n > 0 && !k->level_sigma2)) return ORBX_ERR_ARG;
    for (int i = 0; i < k->n; ++i)
      if (k->keys[i].octave < 0 || k->keys[i].octave >= k->nlevels) return ORBX_ERR_ARG;
  }
  return ORBX_OK;
}

// one frame's inputs in the arena: declared by the constructor (kf2: with the
// level_sigma2 table), the keys converted in place and the device view taken
// once the arena is committed
struct FrameSlots {
  Slot<TriKey> key;
  Slot<uint8_t> desc, mp;
  Slot<uint32_t> feat;
  Slot<float> sigma2;

  FrameSlots(CallArena& A, const orbx_tri_frame* k, bool kf2) {
    key = A.in<TriKey>((size_t)k->n);
    desc = A.in(k->desc, (size_t)k->n * 32);
    mp = A.in_opt(k->has_mp, (size_t)k->n);
    feat = A.in(k->feat, k->nnodes ? k->node_off[k->nnodes] : 0);
    if (kf2) sigma2 = A.in(k->level_sigma2, (size_t)k->nlevels);
  }
  TriFrame fill(const CallArena& A, const orbx_tri_frame* k) const {
    TriKey* hk = A.h(key);
    for (int i = 0; i < k->n; ++i) {
      const orbx_keypoint& p = k->keys[i];
      hk[i] = TriKey{p.x, p.y, p.angle, p.octave};
    }
    return TriFrame{A.d(key), A.d(desc), A.d(mp), A.d(feat)};
  }
};

}  // namespace

extern "C" int orbm_search_for_triangulation(const orbx_tri_frame* kf1, int nkf2,
                                             const orbx_tri_frame* kf2, const float* F12,
                                             int only_stereo, int check_ori, int device,
                                             int32_t* match12, int* nmatches) {
  if (nkf2 < 0) return ORBX_ERR_ARG;
  int rc = check_tri_frame(kf1, false);
  if (rc) return rc;
  if (nkf2 > 0 && (!kf2 || !F12 || !nmatches || (kf1->n > 0 && !match12))) return ORBX_ERR_ARG;
  for (int p = 0; p < nkf2; ++p) {
    rc = check_tri_frame(kf2 + p, true);
    if (rc) return rc;
  }
  const uint32_t nf1 = kf1->nnodes ? kf1->node_off[kf1->nnodes] : 0;
  {
    /* a KF1 feature listed twice (never in a DBoW2 FeatureVector) would be one
     * match12 entry searched and counted twice (ORBmatcher.cc:431-432) */
    std::vector<uint8_t> seen((size_t)kf1->n, 0);
    if (index_repeats(seen, kf1->feat, nf1)) return ORBX_ERR_ARG;
  }
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  const size_t n1 = (size_t)kf1->n;
  // bOnlyStereo: `!bOnlyStereo && CheckDistEpipolarLine(..)` (:417) accepts
  // nothing in this reference, so there is nothing to launch
  if (only_stereo || n1 == 0 || nkf2 == 0) {
    for (size_t i = 0; i < n1 * (size_t)nkf2; ++i) match12[i] = -1;
    for (int p = 0; p < nkf2; ++p) nmatches[p] = 0;
    return ORBX_OK;
  }
  // the common nodes of every problem, ascending (:396-442), cut into items
  // of TRI_ROWS rows
  std::vector<TriItem> items;
  for (int p = 0; p < nkf2; ++p) {
    const auto cut = [&](uint32_t o1, uint32_t c1, uint32_t o2, uint32_t c2) {
      if (o1 > 0x7FFFFFFFu - c1 || o2 > 0x7FFFFFFFu - c2) return ORBX_ERR_UNSUPPORTED;
      for (uint32_t r = 0; r < c1 && c2 > 0; r += TRI_ROWS)
        items.push_back(
            TriItem{p, (int)(o1 + r), (int)std::min<uint32_t>(TRI_ROWS, c1 - r), (int)o2, (int)c2});
      return ORBX_OK;
    };
    rc = for_common_nodes(kf1->node_id, kf1->node_off, kf1->nnodes, kf2[p].node_id, kf2[p].node_off,
                          kf2[p].nnodes, cut);
    if (rc) return rc;
  }
  if (items.size() > 0x7FFFFFFFu || nkf2 > 65535) return ORBX_ERR_UNSUPPORTED; /* grid limits */
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  const FrameSlots s1(A, kf1, false);
  std::vector<FrameSlots> s2;
  for (int p = 0; p < nkf2; ++p) s2.emplace_back(A, kf2 + p, true);
  const auto s_prob = A.in<TriProblem>((size_t)nkf2);
  const auto s_items = A.in(items.data(), items.size());
  const auto s_m12 = A.out(match12, (size_t)nkf2 * n1);
  const auto s_nm = A.out(nmatches, (size_t)nkf2);
  const auto s_row = A.scratch<int2>((size_t)nkf2 * n1);
  const auto s_hist = A.scratch<int>((size_t)nkf2 * 32);
  rc = A.commit();
  if (rc) return rc;
  const TriFrame f1 = s1.fill(A, kf1);
  for (int p = 0; p < nkf2; ++p) {
    TriProblem P = {};
    P.kf2 = s2[p].fill(A, kf2 + p);
    P.sigma2 = A.d(s2[p].sigma2);
    memcpy(P.F, F12 + (size_t)p * 9, sizeof(P.F));
    P.row = A.d(s_row) + (size_t)p * n1;
    P.hist = A.d(s_hist) + (size_t)p * 32;
    P.match12 = A.d(s_m12) + (size_t)p * n1;
    P.nmatches = A.d(s_nm) + p;
    A.h(s_prob)[p] = P;
  }
  rc = A.upload();
  if (rc) return rc;
  const TriProblem* d_probs = A.d(s_prob);
  hipStream_t s = A.stream();
  hipLaunchKernelGGL(k_tri_init, dim3((unsigned)((n1 + 255) / 256), nkf2), dim3(256), 0, s, d_probs,
                     (int)n1);
  if (!items.empty())
    hipLaunchKernelGGL(k_tri_search, dim3((unsigned)items.size()), dim3(TRI_ROWS), 0, s, d_probs,
                       A.d(s_items), f1, check_ori ? 1 : 0);
  hipLaunchKernelGGL(k_tri_finalize, dim3(nkf2), dim3(256), 0, s, d_probs, (int)n1,
                     check_ori ? 1 : 0);
  return A.finish();
}

// api_tri.hip -- C ABI of ORBmatcher::SearchForTriangulation, batched over
// the neighbour keyframes of LocalMapping::CreateNewMapPoints.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/orbx.h"
#include "api_common.h"
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

// offsets of one frame's inputs in the arena
struct FrameOff {
  size_t key, desc, mp, feat, sigma2;
  uint32_t nf;
};

FrameOff carve_frame(Carve& C, const orbx_tri_frame* k, bool kf2) {
  FrameOff o;
  o.nf = k->nnodes ? k->node_off[k->nnodes] : 0;
  o.key = C.take((size_t)k->n * sizeof(TriKey));
  o.desc = C.take((size_t)k->n * 32);
  o.mp = k->has_mp ? C.take((size_t)k->n) : 0;
  o.feat = C.take((size_t)o.nf * 4);
  o.sigma2 = kf2 ? C.take((size_t)k->nlevels * 4) : 0;
  return o;
}

TriFrame fill_frame(uint8_t* h, uint8_t* d, const FrameOff& o, const orbx_tri_frame* k, bool kf2) {
  TriKey* hk = reinterpret_cast<TriKey*>(h + o.key);
  for (int i = 0; i < k->n; ++i) {
    const orbx_keypoint& p = k->keys[i];
    hk[i] = TriKey{p.x, p.y, p.angle, p.octave};
  }
  if (k->n) memcpy(h + o.desc, k->desc, (size_t)k->n * 32);
  if (k->has_mp && k->n) memcpy(h + o.mp, k->has_mp, (size_t)k->n);
  if (o.nf) memcpy(h + o.feat, k->feat, (size_t)o.nf * 4);
  if (kf2 && k->nlevels) memcpy(h + o.sigma2, k->level_sigma2, (size_t)k->nlevels * 4);
  TriFrame f;
  f.key = reinterpret_cast<const TriKey*>(d + o.key);
  f.desc = d + o.desc;
  f.has_mp = k->has_mp ? d + o.mp : nullptr;
  f.feat = reinterpret_cast<const uint32_t*>(d + o.feat);
  return f;
}

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
    std::vector<unsigned char> seen(kf1->n > 0 ? (size_t)kf1->n : 1, 0);
    for (uint32_t j = 0; j < nf1; ++j) {
      if (seen[kf1->feat[j]]) return ORBX_ERR_ARG;
      seen[kf1->feat[j]] = 1;
    }
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
  // the common nodes of every problem, ascending (:396-442: the iterator that
  // is behind jumps with lower_bound), cut into items of TRI_ROWS rows
  std::vector<TriItem> items;
  for (int p = 0; p < nkf2; ++p) {
    const orbx_tri_frame* k2 = kf2 + p;
    const uint32_t *b1 = kf1->node_id, *e1 = b1 + kf1->nnodes;
    const uint32_t *b2 = k2->node_id, *e2 = b2 + k2->nnodes;
    const uint32_t *f1 = b1, *f2 = b2;
    while (f1 != e1 && f2 != e2) {
      if (*f1 == *f2) {
        const uint32_t o1 = kf1->node_off[f1 - b1], c1 = kf1->node_off[f1 - b1 + 1] - o1;
        const uint32_t o2 = k2->node_off[f2 - b2], c2 = k2->node_off[f2 - b2 + 1] - o2;
        if (o1 > 0x7FFFFFFFu - c1 || o2 > 0x7FFFFFFFu - c2) return ORBX_ERR_UNSUPPORTED;
        for (uint32_t r = 0; r < c1 && c2 > 0; r += TRI_ROWS) {
          TriItem it;
          it.prob = p;
          it.off1 = (int)(o1 + r);
          it.n1 = (int)std::min<uint32_t>(TRI_ROWS, c1 - r);
          it.off2 = (int)o2;
          it.n2 = (int)c2;
          items.push_back(it);
        }
        ++f1;
        ++f2;
      } else if (*f1 < *f2) {
        f1 = std::lower_bound(f1, e1, *f2);
      } else {
        f2 = std::lower_bound(f2, e2, *f1);
      }
    }
  }
  if (items.size() > 0x7FFFFFFFu || nkf2 > 65535) return ORBX_ERR_UNSUPPORTED; /* grid limits */
  ORBX_TRY(hipSetDevice(device));
  WsLease L(device);
  CallWs* w = L.w;
  if (!w) return ORBX_ERR_HIP;
  hipStream_t s = w->stream;
  // one arena: inputs [0, in_end) go up in one copy from pinned staging,
  // outputs [in_end, out_end) come back in one copy, scratch after them
  Carve C;
  const FrameOff o1 = carve_frame(C, kf1, false);
  std::vector<FrameOff> o2((size_t)nkf2);
  for (int p = 0; p < nkf2; ++p) o2[p] = carve_frame(C, kf2 + p, true);
  const size_t o_prob = C.take((size_t)nkf2 * sizeof(TriProblem));
  const size_t o_items = C.take(items.size() * sizeof(TriItem));
  const size_t in_end = C.off;
  const size_t o_m12 = C.take((size_t)nkf2 * n1 * 4), o_nm = C.take((size_t)nkf2 * sizeof(int));
  const size_t out_end = C.off;
  const size_t o_row = C.take((size_t)nkf2 * n1 * sizeof(int2));
  const size_t o_hist = C.take((size_t)nkf2 * 32 * sizeof(int));
  rc = w->reserve(C.off, out_end);
  if (rc) return rc;
  uint8_t* d = w->d;
  uint8_t* h = w->h;
  const TriFrame f1 = fill_frame(h, d, o1, kf1, false);
  TriProblem* hp = reinterpret_cast<TriProblem*>(h + o_prob);
  for (int p = 0; p < nkf2; ++p) {
    TriProblem P;
    memset(&P, 0, sizeof(P));
    P.kf2 = fill_frame(h, d, o2[p], kf2 + p, true);
    P.sigma2 = reinterpret_cast<const float*>(d + o2[p].sigma2);
    memcpy(P.F, F12 + (size_t)p * 9, sizeof(P.F));
    P.row = reinterpret_cast<int2*>(d + o_row) + (size_t)p * n1;
    P.hist = reinterpret_cast<int*>(d + o_hist) + (size_t)p * 32;
    P.match12 = reinterpret_cast<int32_t*>(d + o_m12) + (size_t)p * n1;
    P.nmatches = reinterpret_cast<int*>(d + o_nm) + p;
    memcpy(hp + p, &P, sizeof(P));
  }
  if (!items.empty()) memcpy(h + o_items, items.data(), items.size() * sizeof(TriItem));
  rc = stage_in(d, h, in_end, s);
  if (rc) return rc;
  const TriProblem* d_probs = reinterpret_cast<const TriProblem*>(d + o_prob);
  hipLaunchKernelGGL(k_tri_init, dim3((unsigned)((n1 + 255) / 256), nkf2), dim3(256), 0, s, d_probs,
                     (int)n1);
  if (!items.empty())
    hipLaunchKernelGGL(k_tri_search, dim3((unsigned)items.size()), dim3(TRI_ROWS), 0, s, d_probs,
                       reinterpret_cast<const TriItem*>(d + o_items), f1, check_ori ? 1 : 0);
  hipLaunchKernelGGL(k_tri_finalize, dim3(nkf2), dim3(256), 0, s, d_probs, (int)n1,
                     check_ori ? 1 : 0);
  rc = finish_call(w, in_end, out_end);
  if (rc) return rc;
  memcpy(match12, h + o_m12, (size_t)nkf2 * n1 * 4);
  memcpy(nmatches, h + o_nm, (size_t)nkf2 * sizeof(int));
  return ORBX_OK;
}

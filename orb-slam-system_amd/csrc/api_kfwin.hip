// api_kfwin.hip -- C ABI of the keyframe window search shared by
// ORBmatcher::Fuse (both forms) and SearchBySim3, batched over the keyframes
// of LocalMapping::SearchInNeighbors.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/orbx.h"
#include "api_common.h"
#include "kfwin_internal.h"

namespace orbx {
__global__ void k_kfwin_grid(const KfwProblem*);
__global__ void k_kfwin_search(const KfwProblem*, const orbx_kf_query*, const int32_t*, const int32_t*,
                               const uint8_t*, int, int32_t*, int32_t*);
}  // namespace orbx

using namespace orbx;

extern "C" int orbm_keyframe_search(int nprob, const orbx_kf_frame* kf, const orbx_kf_query* q,
                                    const int32_t* qoff, const uint8_t* qdesc, int npool, int device,
                                    int32_t* best_idx, int32_t* best_dist) {
  if (nprob < 0 || npool < 0) return ORBX_ERR_ARG;
  if (nprob > 0 && (!kf || !qoff)) return ORBX_ERR_ARG;
  if (nprob > 0 && qoff[0] != 0) return ORBX_ERR_ARG;
  for (int p = 0; p < nprob; ++p) {
    if (qoff[p + 1] < qoff[p]) return ORBX_ERR_ARG;
    if (kf[p].n < 0 || (kf[p].n > 0 && (!kf[p].keys || !kf[p].desc))) return ORBX_ERR_ARG;
  }
  const int nq = nprob > 0 ? qoff[nprob] : 0;
  if (nq > 0 && (!q || !qdesc || !best_idx || !best_dist)) return ORBX_ERR_ARG;
  for (int j = 0; j < nq; ++j) {
    if (q[j].desc < 0 || q[j].desc >= npool) return ORBX_ERR_ARG;
    if (!isfinite(q[j].x) || !isfinite(q[j].y) || !isfinite(q[j].radius)) return ORBX_ERR_ARG;
  }
  for (int p = 0; p < nprob; ++p)
    if (kf[p].n > KFW_MAXN) return ORBX_ERR_UNSUPPORTED;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  if (nq == 0) return ORBX_OK;  // nothing to write
  ORBX_TRY(hipSetDevice(device));
  WsLease L(device);
  CallWs* w = L.w;
  if (!w) return ORBX_ERR_HIP;
  hipStream_t s = w->stream;
  // a keyframe without queries is neither uploaded nor gridded (its table
  // entry stays zeroed)
  const int qpb = KFW_BLOCK / KFW_G;
  const int nblk = (nq + qpb - 1) / qpb;
  // one arena: inputs [0, in_end) go up in one copy from pinned staging,
  // outputs [in_end, out_end) come back in one copy, scratch after them
  Carve C;
  std::vector<size_t> o_key((size_t)nprob), o_desc((size_t)nprob);
  for (int p = 0; p < nprob; ++p) {
    const size_t n = qoff[p + 1] > qoff[p] ? (size_t)kf[p].n : 0;
    o_key[p] = C.take(n * sizeof(KfwKey));
    o_desc[p] = C.take(n * 32);
  }
  const size_t o_prob = C.take((size_t)nprob * sizeof(KfwProblem));
  const size_t o_q = C.take((size_t)nq * sizeof(orbx_kf_query));
  const size_t o_qoff = C.take((size_t)(nprob + 1) * 4);
  const size_t o_blk = C.take((size_t)nblk * 4);
  const size_t o_pool = C.take((size_t)npool * 32);
  const size_t in_end = C.off;
  const size_t o_idx = C.take((size_t)nq * 4), o_dist = C.take((size_t)nq * 4);
  const size_t out_end = C.off;
  std::vector<size_t> o_off((size_t)nprob), o_rec((size_t)nprob);
  for (int p = 0; p < nprob; ++p) {
    const bool used = qoff[p + 1] > qoff[p];
    o_off[p] = used ? C.take((size_t)(KFW_CELLS + 1) * 4) : 0;
    o_rec[p] = used ? C.take((size_t)kf[p].n * sizeof(KfwRec)) : 0;
  }
  int rc = w->reserve(C.off, out_end);
  if (rc) return rc;
  uint8_t* d = w->d;
  uint8_t* h = w->h;
  KfwProblem* hp = reinterpret_cast<KfwProblem*>(h + o_prob);
  for (int p = 0; p < nprob; ++p) {
    KfwProblem P;
    memset(&P, 0, sizeof(P));
    if (qoff[p + 1] > qoff[p]) {
      const orbx_kf_frame& f = kf[p];
      KfwKey* hk = reinterpret_cast<KfwKey*>(h + o_key[p]);
      for (int i = 0; i < f.n; ++i) hk[i] = KfwKey{f.keys[i].x, f.keys[i].y, f.keys[i].octave};
      if (f.n) memcpy(h + o_desc[p], f.desc, (size_t)f.n * 32);
      P.n = f.n;
      P.minX = f.min_x;
      P.minY = f.min_y;
      P.wInv = f.grid_w_inv;
      P.hInv = f.grid_h_inv;
      P.key = reinterpret_cast<const KfwKey*>(d + o_key[p]);
      P.desc = d + o_desc[p];
      P.cell_off = reinterpret_cast<int*>(d + o_off[p]);
      P.rec = reinterpret_cast<KfwRec*>(d + o_rec[p]);
    }
    memcpy(hp + p, &P, sizeof(P));
  }
  memcpy(h + o_q, q, (size_t)nq * sizeof(orbx_kf_query));
  memcpy(h + o_qoff, qoff, (size_t)(nprob + 1) * 4);
  {
    // the problem of every search block's first query
    int32_t* hb = reinterpret_cast<int32_t*>(h + o_blk);
    int p = 0;
    for (int b = 0; b < nblk; ++b) {
      const int first = b * qpb;
      while (first >= qoff[p + 1]) ++p;
      hb[b] = p;
    }
  }
  if (npool) memcpy(h + o_pool, qdesc, (size_t)npool * 32);
  rc = stage_in(d, h, in_end, s);
  if (rc) return rc;
  const KfwProblem* d_probs = reinterpret_cast<const KfwProblem*>(d + o_prob);
  // one block per problem; the block of a problem without queries (a zeroed
  // table entry) returns at once
  hipLaunchKernelGGL(k_kfwin_grid, dim3((unsigned)nprob), dim3(1024), 0, s, d_probs);
  hipLaunchKernelGGL(k_kfwin_search, dim3((unsigned)nblk), dim3(KFW_BLOCK), 0, s, d_probs,
                     reinterpret_cast<const orbx_kf_query*>(d + o_q),
                     reinterpret_cast<const int32_t*>(d + o_qoff),
                     reinterpret_cast<const int32_t*>(d + o_blk), d + o_pool, nq,
                     reinterpret_cast<int32_t*>(d + o_idx), reinterpret_cast<int32_t*>(d + o_dist));
  rc = finish_call(w, in_end, out_end);
  if (rc) return rc;
  memcpy(best_idx, h + o_idx, (size_t)nq * 4);
  memcpy(best_dist, h + o_dist, (size_t)nq * 4);
  return ORBX_OK;
}

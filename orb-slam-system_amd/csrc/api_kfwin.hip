// api_kfwin.hip -- C ABI of the keyframe window search shared by
// ORBmatcher::Fuse (both forms) and SearchBySim3, batched over the keyframes
// of LocalMapping::SearchInNeighbors.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include <vector>

#include "../../include/orbx.h"
#include "call_arena.h"
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
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  // a keyframe without queries is neither uploaded nor gridded (its slots
  // stay absent and its table entry zeroed)
  const int qpb = KFW_BLOCK / KFW_G;
  const int nblk = (nq + qpb - 1) / qpb;
  struct KfSlots {
    Slot<KfwKey> key;
    Slot<uint8_t> desc;
    Slot<int> cell_off;
    Slot<KfwRec> rec;
  };
  std::vector<KfSlots> ks((size_t)nprob);
  for (int p = 0; p < nprob; ++p) {
    if (qoff[p + 1] == qoff[p]) continue;
    ks[p].key = A.in<KfwKey>((size_t)kf[p].n);
    ks[p].desc = A.in(kf[p].desc, (size_t)kf[p].n * 32);
  }
  const auto s_prob = A.in<KfwProblem>((size_t)nprob);
  const auto s_q = A.in(q, (size_t)nq);
  const auto s_qoff = A.in(qoff, (size_t)nprob + 1);
  const auto s_blk = A.in<int32_t>((size_t)nblk);
  const auto s_pool = A.in(qdesc, (size_t)npool * 32);
  const auto s_idx = A.out(best_idx, (size_t)nq), s_dist = A.out(best_dist, (size_t)nq);
  for (int p = 0; p < nprob; ++p) {
    if (qoff[p + 1] == qoff[p]) continue;
    ks[p].cell_off = A.scratch<int>(KFW_CELLS + 1);
    ks[p].rec = A.scratch<KfwRec>((size_t)kf[p].n);
  }
  int rc = A.commit();
  if (rc) return rc;
  for (int p = 0; p < nprob; ++p) {
    KfwProblem P = {};
    if (qoff[p + 1] > qoff[p]) {
      const orbx_kf_frame& f = kf[p];
      KfwKey* hk = A.h(ks[p].key);
      for (int i = 0; i < f.n; ++i) hk[i] = KfwKey{f.keys[i].x, f.keys[i].y, f.keys[i].octave};
      P.n = f.n;
      P.minX = f.min_x;
      P.minY = f.min_y;
      P.wInv = f.grid_w_inv;
      P.hInv = f.grid_h_inv;
      P.key = A.d(ks[p].key);
      P.desc = A.d(ks[p].desc);
      P.cell_off = A.d(ks[p].cell_off);
      P.rec = A.d(ks[p].rec);
    }
    A.h(s_prob)[p] = P;
  }
  {
    // the problem of every search block's first query
    int32_t* hb = A.h(s_blk);
    int p = 0;
    for (int b = 0; b < nblk; ++b) {
      const int first = b * qpb;
      while (first >= qoff[p + 1]) ++p;
      hb[b] = p;
    }
  }
  rc = A.upload();
  if (rc) return rc;
  // one block per problem; the block of a problem without queries (a zeroed
  // table entry) returns at once
  hipLaunchKernelGGL(k_kfwin_grid, dim3((unsigned)nprob), dim3(1024), 0, A.stream(), A.d(s_prob));
  hipLaunchKernelGGL(k_kfwin_search, dim3((unsigned)nblk), dim3(KFW_BLOCK), 0, A.stream(), A.d(s_prob),
                     A.d(s_q), A.d(s_qoff), A.d(s_blk), A.d(s_pool), nq, A.d(s_idx), A.d(s_dist));
  return A.finish();
}

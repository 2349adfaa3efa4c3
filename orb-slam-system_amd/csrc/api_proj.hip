// api_proj.hip -- C ABI of the frame grid + ORBmatcher::SearchByProjection
// (query form, src/ORBmatcher.cc:19-61,732-818,820-894).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "../../include/orbx.h"
#include "call_arena.h"
#include "proj_internal.h"
#include "proj_plan.h"

namespace orbx {  // kernels_proj.hip
__global__ void k_grid_build(const ProjProblem*);
__global__ void k_proj_cand(const ProjProblem*, int);
__global__ void k_proj_resolve(const ProjProblem*, int, float, int, int);
}  // namespace orbx

using namespace orbx;

ProjFrame orbx::proj_frame(const orbx_proj_frame* F) {
  ProjFrame PF;
  PF.n = F->n;
  PF.minX = F->min_x;
  PF.minY = F->min_y;
  PF.wInv = F->grid_w_inv;
  PF.hInv = F->grid_h_inv;
  return PF;
}

// the three launches over nprob problems (device table d_probs): grid per
// problem, candidates per (query, problem), the greedy walk per problem
void orbx::launch_proj(const ProjProblem* d_probs, int nprob, int max_n, int max_nq, int mode,
                       float nnratio, int th_dist, int check_ori, hipStream_t s) {
  int P = 1;
  while (P < max_n) P <<= 1;
  hipLaunchKernelGGL(k_grid_build, dim3((unsigned)nprob), dim3(1024), (size_t)P * 4, s, d_probs);
  if (max_nq > 0)
    hipLaunchKernelGGL(k_proj_cand, dim3((unsigned)((max_nq + 3) / 4), (unsigned)nprob), dim3(256), 0, s,
                       d_probs, mode);
  const size_t lds = (size_t)((max_n + 31) / 32) * 4 + (size_t)max_n;
  hipLaunchKernelGGL(k_proj_resolve, dim3((unsigned)nprob), dim3(64), lds, s, d_probs, mode, nnratio,
                     th_dist, check_ori);
}

extern "C" int orbm_search_by_projection(int mode, const orbx_proj_frame* F,
                                         const orbx_query_proj* q, const uint8_t* qdesc, int nq,
                                         float nnratio, int th_dist, int check_ori, int device,
                                         int32_t* match, int* nmatches) {
  if (!F || mode < 1 || mode > 3 || nq < 0 || F->n < 0 || !nmatches ||
      (nq > 0 && (!q || !qdesc)) || (F->n > 0 && (!F->keys || !F->desc || !match)))
    return ORBX_ERR_ARG;
  *nmatches = 0;
  const int n = F->n;
  if (n > PJ_MAXN) return ORBX_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) match[i] = -1;
  if (n == 0 || nq == 0) return ORBX_OK;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  set_max_dynamic_lds((const void*)k_grid_build, device);
  set_max_dynamic_lds((const void*)k_proj_resolve, device);
  const auto s_keys = A.in(F->keys, (size_t)n);
  const auto s_desc = A.in(F->desc, (size_t)n * 32);
  const auto s_ur = A.in_opt(F->uright, (size_t)n);
  const auto s_occ = A.in_opt(F->occupied, (size_t)n);
  const auto s_q = A.in(q, (size_t)nq);
  const auto s_qd = A.in(qdesc, (size_t)nq * 32);
  const auto s_prob = A.in<ProjProblem>(1);
  const auto s_match = A.out(match, (size_t)n);
  const auto s_nm = A.out(nmatches, 1);
  const auto s_off = A.scratch<int>(PG_CELLS + 1), s_feat = A.scratch<int>((size_t)n);
  const auto s_cand = A.scratch<uint32_t>((size_t)nq * PJ_T);
  const auto s_nc = A.scratch<int>((size_t)nq);
  const int rc = A.commit();
  if (rc) return rc;
  ProjProblem* hp = A.h(s_prob);
  hp->F = proj_frame(F);
  hp->keys = A.d(s_keys);
  hp->desc = A.d(s_desc);
  hp->uright = A.d(s_ur);
  hp->occupied = A.d(s_occ);
  hp->qs = A.d(s_q);
  hp->qdesc = A.d(s_qd);
  hp->nq = nq;
  hp->match = A.d(s_match);
  hp->nmatches = A.d(s_nm);
  hp->cell_off = A.d(s_off);
  hp->cell_feat = A.d(s_feat);
  hp->cand = A.d(s_cand);
  hp->ncand = A.d(s_nc);
  if (A.upload()) return ORBX_ERR_HIP;
  launch_proj(A.d(s_prob), 1, n, nq, mode, nnratio, th_dist, check_ori, A.stream());
  return A.finish();
}

// ---------------------------------------------------------------------------
// Batched device form: many SearchByProjection problems (frames, each with
// its query set) in one set of launches on device-resident inputs.
// ---------------------------------------------------------------------------
// struct orbm_proj_plan: proj_plan.h (shared with api_projbuild.hip)

extern "C" int orbm_proj_plan_create(int max_problems, int max_n, int max_nq, int device, orbm_proj_plan** out) {
  if (!out || max_problems < 1 || max_n < 1 || max_nq < 0) return ORBX_ERR_ARG;
  *out = nullptr;
  if (max_n > PJ_MAXN || max_problems > 65535) return ORBX_ERR_UNSUPPORTED;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  std::unique_ptr<orbm_proj_plan> p(new orbm_proj_plan());
  p->device = device;
  p->max_prob = max_problems;
  p->max_n = max_n;
  p->max_nq = max_nq;
  const size_t B = (size_t)max_problems;
  const size_t Q = B * (size_t)std::max(max_nq, 1);
  if (p->probs.alloc(B) || p->fence.create() || p->d_cell_off.alloc(B * (PG_CELLS + 1)) ||
      p->d_cell_feat.alloc(B * (size_t)max_n) || p->d_cand.alloc(Q * PJ_T) || p->d_ncand.alloc(Q) ||
      set_max_dynamic_lds((const void*)k_grid_build, device) ||
      set_max_dynamic_lds((const void*)k_proj_resolve, device))
    return ORBX_ERR_HIP;
  *out = p.release();
  return ORBX_OK;
}

extern "C" int orbm_proj_plan_destroy(orbm_proj_plan* p) {
  delete p;
  return ORBX_OK;
}

extern "C" int orbm_proj_plan_search(orbm_proj_plan* p, int mode, int nprob, const orbx_proj_problem* probs,
                                     float nnratio, int th_dist, int check_ori, void* stream) {
  if (!p || mode < 1 || mode > 3 || nprob < 0 || nprob > p->max_prob || (nprob > 0 && !probs))
    return ORBX_ERR_ARG;
  int max_n = 1, max_nq = 0;
  for (int i = 0; i < nprob; ++i) {
    const orbx_proj_problem& q = probs[i];
    if (!frame_ok(q.frame, p->max_n) || q.nq < 0 || q.nq > p->max_nq || !q.match || !q.nmatches ||
        (q.nq > 0 && (!q.q || !q.qdesc)))
      return ORBX_ERR_ARG;
    max_n = std::max(max_n, q.frame.n);
    max_nq = std::max(max_nq, q.nq);
  }
  if (nprob == 0) return ORBX_OK;
  ORBX_TRY(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  if (p->fence.begin(s)) return ORBX_ERR_HIP;
  for (int i = 0; i < nprob; ++i) {
    const orbx_proj_problem& q = probs[i];
    fill_search_row(p, i, q.frame, q.q, q.qdesc, q.nq, q.match, q.nmatches);
  }
  if (p->probs.upload((size_t)nprob, s) || p->fence.staged(s)) return ORBX_ERR_HIP;
  launch_proj(p->probs.dev(), nprob, max_n, max_nq, mode, nnratio, th_dist, check_ori, s);
  return p->fence.end(s);
}

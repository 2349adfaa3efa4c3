// api_kfbuild.hip -- C ABI of the device-side projection that feeds the
// keyframe window search (kernels_kfbuild.hip): the synchronous
// host-pointer form, and orbm_kf_plan with its search / project /
// project_search methods on device pointers.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/orbx.h"
#include "call_arena.h"
#include "kfbuild_internal.h"
#include "plan_table.h"
#include "projbuild_internal.h"

namespace orbx {
// kernels_kfbuild.hip
__global__ void k_kf_build_begin(const KfBuildProblem*, int);
__global__ void k_kf_build(const KfBuildProblem*, int, float);
// kernels_kfwin.hip
__global__ void k_kfwin_grid_kp(const KfwPlanProblem*);
__global__ void k_kfwin_search_plan(const KfwPlanProblem*);
}  // namespace orbx

using namespace orbx;

struct orbm_kf_plan {
  int device = 0, max_prob = 0, max_n = 0, max_nq = 0;
  PlanTable<KfBuildProblem> bprobs;  // the projection's problem table
  PlanTable<KfwPlanProblem> probs;   // the search's
  PlanFence fence;
  DevBuf<int> d_cell_off;    // max_prob x (KFW_CELLS + 1)
  DevBuf<KfwRec> d_rec;      // max_prob x max_n
  DevBuf<orbx_kf_query> d_q; // max_prob x max_nq: rows of a project_search call that names none
  PredictScaleCache thr_cache;
  ~orbm_kf_plan() { hipSetDevice(device); }
};

static bool form_ok(int form) { return form == ORBX_KF_FORM_FUSE || form == ORBX_KF_FORM_SIM3; }

// every array the forms read is present (npts > 0)
static bool points_ok(const orbx_kf_points& P) {
  return P.pos && P.min_dist_inv && P.max_dist_inv && P.max_dist;
}

static void launch_build(const KfBuildProblem* d_probs, int nprob, int max_npts, int form, float th, hipStream_t s) {
  hipLaunchKernelGGL(k_kf_build_begin, dim3((unsigned)((nprob + 63) / 64)), dim3(64), 0, s, d_probs, nprob);
  if (max_npts > 0)
    hipLaunchKernelGGL(k_kf_build, dim3((unsigned)((max_npts + KB_BLOCK - 1) / KB_BLOCK), (unsigned)nprob),
                       dim3(KB_BLOCK), 0, s, d_probs, form, th);
}

extern "C" int orbm_keyframe_project(int form, int nprob, const orbx_kf_camera* cameras,
                                     const orbx_kf_points* points, const int* npts, const int32_t* desc_base,
                                     float th, int device, orbx_kf_query* q, int32_t* level, int* n_live) {
  if (!form_ok(form) || nprob < 0 || nprob > 65535) return ORBX_ERR_ARG;
  if (nprob == 0) return ORBX_OK;
  if (!cameras || !points || !npts || !n_live) return ORBX_ERR_ARG;
  size_t total = 0;
  int max_npts = 0;
  for (int p = 0; p < nprob; ++p) {
    if (npts[p] < 0 || !predict_scale_args_ok(cameras[p].log_scale_factor, cameras[p].nlevels) ||
        (npts[p] > 0 && !points_ok(points[p])) || (desc_base && desc_base[p] < 0) ||
        (desc_base && (int64_t)desc_base[p] + npts[p] > INT32_MAX))
      return ORBX_ERR_ARG;
    total += (size_t)npts[p];
    max_npts = std::max(max_npts, npts[p]);
  }
  if (total > 0 && (!q || !level)) return ORBX_ERR_ARG;
  if (total == 0) {
    for (int p = 0; p < nprob; ++p) n_live[p] = 0;
    return ORBX_OK;
  }
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  struct In {
    Slot<float> pos, mind, maxd, maxdist;
    Slot<uint8_t> skip;
  };
  std::vector<In> in((size_t)nprob);
  const auto s_tab = A.in<KfBuildProblem>((size_t)nprob);
  for (int p = 0; p < nprob; ++p) {
    const orbx_kf_points& P = points[p];
    const size_t n = (size_t)npts[p];
    if (n == 0) continue;
    In& I = in[p];
    I.pos = A.in(P.pos, n * 3);
    I.mind = A.in(P.min_dist_inv, n);
    I.maxd = A.in(P.max_dist_inv, n);
    I.maxdist = A.in(P.max_dist, n);
    I.skip = A.in_opt(P.skip, n);
  }
  // outputs are copied out by hand: none is written when a radius is non-finite
  const auto s_q = A.out<orbx_kf_query>(nullptr, total);
  const auto s_level = A.out<int32_t>(nullptr, total);
  const auto s_cnt = A.out<int>(nullptr, (size_t)nprob * 2);
  const int rc = A.commit();
  if (rc) return rc;
  KfBuildProblem* tab = A.h(s_tab);
  size_t off = 0;
  for (int p = 0; p < nprob; ++p) {
    KfBuildProblem& B = tab[p];
    memset(&B, 0, sizeof(B));
    B.cam = cameras[p];
    predict_scale_thresholds_host(B.cam.log_scale_factor, B.cam.nlevels, B.thr);
    const In& I = in[p];
    B.pts.pos = A.d(I.pos);
    B.pts.min_dist_inv = A.d(I.mind);
    B.pts.max_dist_inv = A.d(I.maxd);
    B.pts.max_dist = A.d(I.maxdist);
    B.pts.skip = A.d(I.skip);
    B.npts = npts[p];
    B.desc_base = desc_base ? desc_base[p] : 0;
    B.q = A.d(s_q) + off;
    B.level = A.d(s_level) + off;
    B.n_live = A.d(s_cnt) + 2 * p;
    B.n_nonfinite = A.d(s_cnt) + 2 * p + 1;
    off += (size_t)npts[p];
  }
  if (A.upload()) return ORBX_ERR_HIP;
  launch_build(A.d(s_tab), nprob, max_npts, form, th, A.stream());
  const int rf = A.finish();
  if (rf) return rf;
  const int* cnt = A.h(s_cnt);
  for (int p = 0; p < nprob; ++p)
    if (cnt[2 * p + 1] != 0) return ORBX_ERR_ARG;
  memcpy(q, A.h(s_q), total * sizeof(orbx_kf_query));
  memcpy(level, A.h(s_level), total * sizeof(int32_t));
  for (int p = 0; p < nprob; ++p) n_live[p] = cnt[2 * p];
  return ORBX_OK;
}

extern "C" int orbm_kf_plan_create(int max_problems, int max_n, int max_queries, int device, orbm_kf_plan** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  if (max_problems < 1 || max_n < 1 || max_queries < 0) return ORBX_ERR_ARG;
  if (max_n > KFW_MAXN || max_problems > 65535) return ORBX_ERR_UNSUPPORTED;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  std::unique_ptr<orbm_kf_plan> p(new orbm_kf_plan());
  p->device = device;
  p->max_prob = max_problems;
  p->max_n = max_n;
  p->max_nq = max_queries;
  const size_t B = (size_t)max_problems, QS = (size_t)std::max(max_queries, 1);
  if (p->bprobs.alloc(B) || p->probs.alloc(B) || p->fence.create() || p->d_cell_off.alloc(B * (KFW_CELLS + 1)) ||
      p->d_rec.alloc(B * (size_t)max_n) || p->d_q.alloc(B * QS))
    return ORBX_ERR_HIP;  // the owners release what was acquired
  *out = p.release();
  return ORBX_OK;
}

extern "C" int orbm_kf_plan_destroy(orbm_kf_plan* p) {
  delete p;
  return ORBX_OK;
}

static int plan_run(orbm_kf_plan* p, int form, int nprob, const orbx_kf_problem* probs, float th, bool project,
                    bool search, void* stream) {
  if (!p || nprob < 0 || nprob > p->max_prob || (nprob > 0 && !probs) || (project && !form_ok(form)))
    return ORBX_ERR_ARG;
  int max_npts = 0;
  for (int i = 0; i < nprob; ++i) {
    const orbx_kf_problem& b = probs[i];
    if (b.npts < 0 || b.npts > p->max_nq) return ORBX_ERR_ARG;
    if (project) {
      if (!predict_scale_args_ok(b.camera.log_scale_factor, b.camera.nlevels) ||
          (b.npts > 0 && !points_ok(b.points)))
        return ORBX_ERR_ARG;
      if (!search && b.npts > 0 && (!b.q || !b.level)) return ORBX_ERR_ARG;
    }
    if (search) {
      const orbx_kf_frame& F = b.frame;
      if (F.n < 0 || F.n > p->max_n || (F.n > 0 && (!F.keys || !F.desc)) ||
          (b.npts > 0 && (!b.qdesc || !b.best_idx || !b.best_dist)) || (!project && b.npts > 0 && !b.q))
        return ORBX_ERR_ARG;
    }
    max_npts = std::max(max_npts, b.npts);
  }
  if (nprob == 0) return ORBX_OK;
  ORBX_TRY(hipSetDevice(p->device));
  const size_t QS = (size_t)std::max(p->max_nq, 1);
  hipStream_t s = (hipStream_t)stream;
  if (p->fence.begin(s)) return ORBX_ERR_HIP;
  for (int i = 0; i < nprob; ++i) {
    const orbx_kf_problem& b = probs[i];
    orbx_kf_query* rows = (project && search && !b.q) ? p->d_q + (size_t)i * QS : b.q;
    if (project) {
      KfBuildProblem& H = p->bprobs[i];
      H.cam = b.camera;
      p->thr_cache.fill(b.camera.log_scale_factor, b.camera.nlevels, H.thr);
      H.pts = b.points;
      H.npts = b.npts;
      H.desc_base = 0;
      H.q = rows;
      H.level = b.level;
      H.n_live = b.n_live;
      H.n_nonfinite = b.n_nonfinite;
    }
    if (search) {
      KfwPlanProblem& P = p->probs[i];
      memset(&P, 0, sizeof(P));
      if (b.npts > 0) {  // a problem without queries is not gridded (cell_off stays NULL)
        P.kf.n = b.frame.n;
        P.kf.minX = b.frame.min_x;
        P.kf.minY = b.frame.min_y;
        P.kf.wInv = b.frame.grid_w_inv;
        P.kf.hInv = b.frame.grid_h_inv;
        P.kf.key = reinterpret_cast<const KfwKey*>(b.frame.keys);  // read as orbx_keypoint rows
        P.kf.desc = b.frame.desc;
        P.kf.cell_off = p->d_cell_off + (size_t)i * (KFW_CELLS + 1);
        P.kf.rec = p->d_rec + (size_t)i * (size_t)p->max_n;
        P.qs = rows;
        P.qdesc = b.qdesc;
        P.nq = b.npts;
        P.best_idx = b.best_idx;
        P.best_dist = b.best_dist;
      }
    }
  }
  if ((project && p->bprobs.upload((size_t)nprob, s)) || (search && p->probs.upload((size_t)nprob, s)) ||
      p->fence.staged(s))
    return ORBX_ERR_HIP;
  if (project) launch_build(p->bprobs.dev(), nprob, max_npts, form, th, s);
  if (search && max_npts > 0) {
    const int qpb = KFW_BLOCK / KFW_G;
    hipLaunchKernelGGL(k_kfwin_grid_kp, dim3((unsigned)nprob), dim3(1024), 0, s, p->probs.dev());
    hipLaunchKernelGGL(k_kfwin_search_plan, dim3((unsigned)((max_npts + qpb - 1) / qpb), (unsigned)nprob),
                       dim3(KFW_BLOCK), 0, s, p->probs.dev());
  }
  return p->fence.end(s);
}

extern "C" int orbm_kf_plan_search(orbm_kf_plan* plan, int nprob, const orbx_kf_problem* problems, void* stream) {
  return plan_run(plan, 0, nprob, problems, 0.0f, false, true, stream);
}

extern "C" int orbm_kf_plan_project(orbm_kf_plan* plan, int form, int nprob, const orbx_kf_problem* problems,
                                    float th, void* stream) {
  return plan_run(plan, form, nprob, problems, th, true, false, stream);
}

extern "C" int orbm_kf_plan_project_search(orbm_kf_plan* plan, int form, int nprob,
                                           const orbx_kf_problem* problems, float th, void* stream) {
  return plan_run(plan, form, nprob, problems, th, true, true, stream);
}

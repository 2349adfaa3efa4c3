// api_projbuild.hip -- C ABI of the device-side projection that feeds the
// projection matchers (kernels_projbuild.hip): the PredictScale
// threshold tables, the synchronous host-pointer form and the plan's project /
// track methods.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/orbx.h"
#include "call_arena.h"
#include "proj_plan.h"
#include "projbuild_internal.h"

namespace orbx {  // kernels_projbuild.hip
__global__ void k_proj_build_begin(const ProjBuildProblem*, int);
__global__ void k_proj_build(const ProjBuildProblem*, int, ProjBuildParams);
}  // namespace orbx

using namespace orbx;

extern "C" int orbm_predict_scale_thresholds(float log_scale_factor, int nlevels, float* thr) {
  if (!predict_scale_args_ok(log_scale_factor, nlevels) || (nlevels > 1 && !thr)) return ORBX_ERR_ARG;
  predict_scale_thresholds_host(log_scale_factor, nlevels, thr);
  return ORBX_OK;
}

// the arrays `mode` reads are present (npts > 0)
static bool points_ok(int mode, const orbx_proj_points& P) {
  if (!P.pos) return false;
  if (mode == 1) return P.normal && P.min_dist_inv && P.max_dist_inv && P.max_dist;
  if (mode == 2) return P.octave && P.angle;
  return P.max_dist && P.angle;
}

static bool params_ok(int mode, const orbx_proj_params* prm) {
  if (!prm) return false;
  return mode != 2 || (prm->level_rule >= ORBX_LEVEL_RULE_NEITHER && prm->level_rule <= ORBX_LEVEL_RULE_BACKWARD);
}

static void launch_build(const ProjBuildProblem* d_probs, int nprob, int max_npts, int mode,
                         const orbx_proj_params* prm, hipStream_t s) {
  hipLaunchKernelGGL(k_proj_build_begin, dim3((unsigned)((nprob + 63) / 64)), dim3(64), 0, s, d_probs, nprob);
  if (max_npts > 0) {
    const ProjBuildParams kp = {prm->th, prm->viewing_cos_limit, prm->level_rule};
    hipLaunchKernelGGL(k_proj_build, dim3((unsigned)((max_npts + PB_BLOCK - 1) / PB_BLOCK), (unsigned)nprob),
                       dim3(PB_BLOCK), 0, s, d_probs, mode, kp);
  }
}

extern "C" int orbm_project_points(int mode, int nprob, const orbx_proj_camera* cameras,
                                   const orbx_proj_points* points, const int* npts,
                                   const orbx_proj_params* params, int device, orbx_query_proj* q,
                                   int32_t* level, float* view_cos, int* n_in_view) {
  if (mode < 1 || mode > 3 || nprob < 0 || nprob > 65535) return ORBX_ERR_ARG;
  if (nprob == 0) return ORBX_OK;
  if (!cameras || !points || !npts || !n_in_view || !params_ok(mode, params)) return ORBX_ERR_ARG;
  size_t total = 0;
  int max_npts = 0;
  for (int p = 0; p < nprob; ++p) {
    if (npts[p] < 0 || !predict_scale_args_ok(cameras[p].log_scale_factor, cameras[p].nlevels) ||
        (npts[p] > 0 && !points_ok(mode, points[p])))
      return ORBX_ERR_ARG;
    total += (size_t)npts[p];
    max_npts = std::max(max_npts, npts[p]);
  }
  if (total > 0 && (!q || !level)) return ORBX_ERR_ARG;
  if (total == 0) {
    for (int p = 0; p < nprob; ++p) n_in_view[p] = 0;
    return ORBX_OK;
  }
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  struct In {
    Slot<float> pos, normal, mind, maxd, maxdist, angle;
    Slot<int32_t> octave;
    Slot<uint8_t> skip;
  };
  std::vector<In> in((size_t)nprob);
  const auto s_tab = A.in<ProjBuildProblem>((size_t)nprob);
  for (int p = 0; p < nprob; ++p) {
    const orbx_proj_points& P = points[p];
    const size_t n = (size_t)npts[p];
    In& I = in[p];
    if (n == 0) continue;
    I.pos = A.in(P.pos, n * 3);
    if (mode == 1) {
      I.normal = A.in(P.normal, n * 3);
      I.mind = A.in(P.min_dist_inv, n);
      I.maxd = A.in(P.max_dist_inv, n);
    }
    if (mode != 2) I.maxdist = A.in(P.max_dist, n);
    if (mode == 2) I.octave = A.in(P.octave, n);
    if (mode != 1) I.angle = A.in(P.angle, n);
    I.skip = A.in_opt(P.skip, n);
  }
  // outputs are copied out by hand: none is written when a point is non-finite
  const auto s_q = A.out<orbx_query_proj>(nullptr, total);
  const auto s_level = A.out<int32_t>(nullptr, total);
  const auto s_vc = (mode == 1 && view_cos) ? A.out<float>(nullptr, total) : Slot<float>();
  const auto s_cnt = A.out<int>(nullptr, (size_t)nprob * 2);
  const int rc = A.commit();
  if (rc) return rc;
  ProjBuildProblem* tab = A.h(s_tab);
  size_t off = 0;
  for (int p = 0; p < nprob; ++p) {
    ProjBuildProblem& B = tab[p];
    memset(&B, 0, sizeof(B));
    B.cam = cameras[p];
    predict_scale_thresholds_host(B.cam.log_scale_factor, B.cam.nlevels, B.thr);
    const In& I = in[p];
    B.pts.pos = A.d(I.pos);
    B.pts.normal = A.d(I.normal);
    B.pts.min_dist_inv = A.d(I.mind);
    B.pts.max_dist_inv = A.d(I.maxd);
    B.pts.max_dist = A.d(I.maxdist);
    B.pts.octave = A.d(I.octave);
    B.pts.angle = A.d(I.angle);
    B.pts.skip = A.d(I.skip);
    B.npts = npts[p];
    B.q = A.d(s_q) + off;
    B.level = A.d(s_level) + off;
    B.view_cos = s_vc.present ? A.d(s_vc) + off : nullptr;
    B.n_in_view = A.d(s_cnt) + 2 * p;
    B.n_nonfinite = A.d(s_cnt) + 2 * p + 1;
    off += (size_t)npts[p];
  }
  if (A.upload()) return ORBX_ERR_HIP;
  launch_build(A.d(s_tab), nprob, max_npts, mode, params, A.stream());
  const int rf = A.finish();
  if (rf) return rf;
  const int* cnt = A.h(s_cnt);
  for (int p = 0; p < nprob; ++p)
    if (cnt[2 * p + 1] != 0) return ORBX_ERR_ARG;
  memcpy(q, A.h(s_q), total * sizeof(orbx_query_proj));
  memcpy(level, A.h(s_level), total * sizeof(int32_t));
  if (s_vc.present) memcpy(view_cos, A.h(s_vc), total * sizeof(float));
  for (int p = 0; p < nprob; ++p) n_in_view[p] = cnt[2 * p];
  return ORBX_OK;
}

static int plan_build(orbm_proj_plan* p, int mode, int nprob, const orbx_proj_build_problem* probs,
                      const orbx_proj_params* prm, bool track, float nnratio, int th_dist, int check_ori,
                      void* stream) {
  if (!p || mode < 1 || mode > 3 || nprob < 0 || nprob > p->max_prob || (nprob > 0 && !probs) ||
      (nprob > 0 && !params_ok(mode, prm)))
    return ORBX_ERR_ARG;
  int max_n = 1, max_npts = 0;
  for (int i = 0; i < nprob; ++i) {
    const orbx_proj_build_problem& b = probs[i];
    if (b.npts < 0 || !predict_scale_args_ok(b.camera.log_scale_factor, b.camera.nlevels) ||
        (b.npts > 0 && !points_ok(mode, b.points)))
      return ORBX_ERR_ARG;
    if (track) {
      if (b.npts > p->max_nq || !frame_ok(b.frame, p->max_n) || !b.match || !b.nmatches ||
          (b.npts > 0 && !b.qdesc))
        return ORBX_ERR_ARG;
      max_n = std::max(max_n, b.frame.n);
    } else if (b.npts > 0 && (!b.q || !b.level)) {
      return ORBX_ERR_ARG;
    }
    max_npts = std::max(max_npts, b.npts);
  }
  if (nprob == 0) return ORBX_OK;
  ORBX_TRY(hipSetDevice(p->device));
  const size_t B = (size_t)p->max_prob, QS = (size_t)std::max(p->max_nq, 1);
  // the first call's acquisitions; a call that fails leaves the plan holding what it held
  const bool first = !p->bprobs;
  if (first && p->bprobs.alloc(B)) return ORBX_ERR_HIP;
  if (track && !p->d_q && p->d_q.alloc(B * QS)) {
    if (first) p->bprobs.reset();
    return ORBX_ERR_HIP;
  }
  hipStream_t s = (hipStream_t)stream;
  if (p->fence.begin(s)) return ORBX_ERR_HIP;
  for (int i = 0; i < nprob; ++i) {
    const orbx_proj_build_problem& b = probs[i];
    ProjBuildProblem& H = p->bprobs[i];
    H.cam = b.camera;
    p->thr_cache.fill(b.camera.log_scale_factor, b.camera.nlevels, H.thr);
    H.pts = b.points;
    H.npts = b.npts;
    H.q = (track && !b.q) ? p->d_q + (size_t)i * QS : b.q;
    H.level = b.level;
    H.view_cos = b.view_cos;
    H.n_in_view = b.n_in_view;
    H.n_nonfinite = b.n_nonfinite;
    if (track) fill_search_row(p, i, b.frame, H.q, b.qdesc, b.npts, b.match, b.nmatches);
  }
  if (p->bprobs.upload((size_t)nprob, s) || (track && p->probs.upload((size_t)nprob, s)) || p->fence.staged(s))
    return ORBX_ERR_HIP;
  launch_build(p->bprobs.dev(), nprob, max_npts, mode, prm, s);
  if (track) launch_proj(p->probs.dev(), nprob, max_n, max_npts, mode, nnratio, th_dist, check_ori, s);
  return p->fence.end(s);
}

extern "C" int orbm_proj_plan_project(orbm_proj_plan* plan, int mode, int nprob,
                                      const orbx_proj_build_problem* problems,
                                      const orbx_proj_params* params, void* stream) {
  return plan_build(plan, mode, nprob, problems, params, false, 0.0f, 0, 0, stream);
}

extern "C" int orbm_proj_plan_track(orbm_proj_plan* plan, int mode, int nprob,
                                    const orbx_proj_build_problem* problems,
                                    const orbx_proj_params* params, float nnratio, int th_dist,
                                    int check_ori, void* stream) {
  return plan_build(plan, mode, nprob, problems, params, true, nnratio, th_dist, check_ori, stream);
}

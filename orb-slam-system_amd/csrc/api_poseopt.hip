// api_poseopt.hip -- C ABI of the batched pose-only optimisation
// (kernels_poseopt.hip): the synchronous host-pointer form on
// the call arena and the plan form on device pointers.
#include <hip/hip_runtime.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/orbx.h"
#include "call_arena.h"
#include "plan_table.h"
#include "poseopt_internal.h"

using namespace orbx;

struct orbm_pose_plan {
  int device = 0, max_prob = 0, max_n = 0;
  PlanTable<orbx_pose_problem> probs;
  PlanFence fence;
  ~orbm_pose_plan() { hipSetDevice(device); }
};

static void launch_pose(const orbx_pose_problem* d_probs, int nprob, hipStream_t s) {
  hipLaunchKernelGGL(k_pose_optimize, dim3((unsigned)nprob), dim3(PO_T), 0, s, d_probs);
}

// the per-feature checks the host form can make and the device form cannot
static bool features_ok(const orbx_pose_camera& c, const orbx_pose_obs& o) {
  if (!o.point_index && o.npos < o.n) return false;
  for (int i = 0; i < o.n; ++i) {
    bool present;
    if (o.point_index) {
      const int32_t idx = o.point_index[i];
      if (idx < -1 || idx >= o.npos) return false;
      present = idx >= 0;
    } else {
      present = !o.has_point || o.has_point[i] != 0;
    }
    if (present && (o.keys[i].octave < 0 || o.keys[i].octave >= c.nlevels)) return false;
  }
  return true;
}

extern "C" int orbm_pose_optimization(int nprob, const orbx_pose_camera* cameras, const orbx_pose_obs* obs,
                                      int device, float* Tcw_out, uint8_t* outlier, int* ninliers) {
  if (nprob < 0 || nprob > 65535) return ORBX_ERR_ARG;
  if (nprob == 0) return ORBX_OK;
  if (!cameras || !obs || !Tcw_out || !ninliers) return ORBX_ERR_ARG;
  size_t total = 0;
  for (int p = 0; p < nprob; ++p) {
    if (!pose_args_ok(cameras[p], obs[p], ORBX_POSE_MAX_N) || !features_ok(cameras[p], obs[p])) return ORBX_ERR_ARG;
    total += (size_t)obs[p].n;
  }
  if (total > 0 && !outlier) return ORBX_ERR_ARG;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  struct In {
    Slot<orbx_keypoint> keys;
    Slot<float> uright, pos;
    Slot<int32_t> index;
    Slot<uint8_t> has;
  };
  std::vector<In> in((size_t)nprob);
  const auto s_tab = A.in<orbx_pose_problem>((size_t)nprob);
  for (int p = 0; p < nprob; ++p) {
    const orbx_pose_obs& O = obs[p];
    const size_t n = (size_t)O.n;
    if (n == 0) continue;
    In& I = in[p];
    I.keys = A.in(O.keys, n);
    I.uright = A.in_opt(O.uright, n);
    I.pos = A.in(O.pos, (size_t)O.npos * 3);
    I.index = A.in_opt(O.point_index, n);
    if (!O.point_index) I.has = A.in_opt(O.has_point, n);
  }
  const auto s_T = A.out<float>(Tcw_out, (size_t)nprob * 16);
  const auto s_out = A.out<uint8_t>(outlier, total);
  const auto s_nin = A.out<int>(ninliers, (size_t)nprob);
  const auto s_status = A.out<int>(nullptr, (size_t)nprob);
  const int rc = A.commit();
  if (rc) return rc;
  orbx_pose_problem* tab = A.h(s_tab);
  size_t off = 0;
  for (int p = 0; p < nprob; ++p) {
    orbx_pose_problem& B = tab[p];
    memset(&B, 0, sizeof(B));
    const In& I = in[p];
    B.camera = cameras[p];
    B.obs.n = obs[p].n;
    B.obs.npos = obs[p].npos;
    B.obs.keys = A.d(I.keys);
    B.obs.uright = A.d(I.uright);
    B.obs.pos = A.d(I.pos);
    B.obs.point_index = A.d(I.index);
    B.obs.has_point = A.d(I.has);
    B.Tcw_out = A.d(s_T) + 16 * (size_t)p;
    B.outlier = A.d(s_out) + off;
    B.ninliers = A.d(s_nin) + p;
    B.status = A.d(s_status) + p;
    off += (size_t)obs[p].n;
  }
  if (A.upload()) return ORBX_ERR_HIP;
  launch_pose(A.d(s_tab), nprob, A.stream());
  return A.finish();
}

extern "C" int orbm_pose_plan_create(int max_problems, int max_n, int device, orbm_pose_plan** out) {
  if (!out) return ORBX_ERR_ARG;
  *out = nullptr;
  if (max_problems < 1 || max_n < 1) return ORBX_ERR_ARG;
  if (max_n > ORBX_POSE_MAX_N || max_problems > 65535) return ORBX_ERR_UNSUPPORTED;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  std::unique_ptr<orbm_pose_plan> p(new orbm_pose_plan());
  p->device = device;
  p->max_prob = max_problems;
  p->max_n = max_n;
  const size_t B = (size_t)max_problems;
  if (p->probs.alloc(B) || p->fence.create()) return ORBX_ERR_HIP;  // the owners release what was acquired
  *out = p.release();
  return ORBX_OK;
}

extern "C" int orbm_pose_plan_destroy(orbm_pose_plan* p) {
  delete p;
  return ORBX_OK;
}

extern "C" int orbm_pose_plan_optimize(orbm_pose_plan* p, int nprob, const orbx_pose_problem* probs, void* stream) {
  if (!p || nprob < 0 || nprob > p->max_prob || (nprob > 0 && !probs)) return ORBX_ERR_ARG;
  for (int i = 0; i < nprob; ++i) {
    const orbx_pose_problem& b = probs[i];
    if (!pose_args_ok(b.camera, b.obs, p->max_n) || !b.Tcw_out || !b.ninliers || !b.status ||
        (b.obs.n > 0 && !b.outlier))
      return ORBX_ERR_ARG;
  }
  if (nprob == 0) return ORBX_OK;
  ORBX_TRY(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  if (p->fence.begin(s)) return ORBX_ERR_HIP;
  memcpy(p->probs.host(), probs, (size_t)nprob * sizeof(orbx_pose_problem));
  if (p->probs.upload((size_t)nprob, s) || p->fence.staged(s)) return ORBX_ERR_HIP;
  launch_pose(p->probs.dev(), nprob, s);
  return p->fence.end(s);
}

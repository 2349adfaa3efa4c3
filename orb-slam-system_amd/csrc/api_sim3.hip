// api_sim3.hip -- C ABI of the batched Sim3Solver RANSAC (kernels_sim3.hip;
// DESIGN.md §22): the synchronous host-pointer form on the call arena.  The
// host checks every count and index; everything else runs on the device.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "../../include/orbx.h"
#include "api_common.h"
#include "call_arena.h"
#include "sim3_internal.h"

using namespace orbx;

static_assert(sizeof(orbx_sim3_result) == 29 * 4, "orbx_sim3_result layout");

static bool all_finite(const float* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!s3_finite(v[i])) return false;
  return true;
}

// :126: the solver returns before it reads anything
static bool inert(const orbx_sim3_problem& P) { return P.ncorr < P.min_inliers; }

// the checks of one problem that is not inert
static int problem_ok(const orbx_sim3_problem& P) {
  if (P.ncorr < 3) return ORBX_ERR_ARG;  // a triple needs three correspondences to draw from
  if (!P.pos1 || !P.pos2 || !P.sigma2_1 || !P.sigma2_2 || (P.nit > 0 && !P.triples)) return ORBX_ERR_ARG;
  const size_t n = (size_t)P.ncorr;
  if (!all_finite(P.pos1, 3 * n) || !all_finite(P.pos2, 3 * n)) return ORBX_ERR_ARG;
  if (!all_finite(P.Rcw1, 9) || !all_finite(P.tcw1, 3) || !all_finite(P.Rcw2, 9) || !all_finite(P.tcw2, 3))
    return ORBX_ERR_ARG;
  const float cams[8] = {P.fx1, P.fy1, P.cx1, P.cy1, P.fx2, P.fy2, P.cx2, P.cy2};
  if (!all_finite(cams, 8)) return ORBX_ERR_ARG;
  for (size_t i = 0; i < n; ++i)
    if (!s3_sigma2_ok(P.sigma2_1[i]) || !s3_sigma2_ok(P.sigma2_2[i])) return ORBX_ERR_ARG;
  for (size_t i = 0; i < (size_t)P.nit * 3; ++i)
    if (P.triples[i] < 0 || P.triples[i] >= P.ncorr) return ORBX_ERR_ARG;
  return ORBX_OK;
}

extern "C" int orbm_sim3_solve(int nprob, const orbx_sim3_problem* problems, int device, orbx_sim3_result* res,
                               uint8_t* inliers, const int32_t* inl_off) {
  if (nprob < 0) return ORBX_ERR_ARG;
  if (nprob == 0) return ORBX_OK;
  if (!problems || !res || !inliers || !inl_off) return ORBX_ERR_ARG;
  if (nprob > 65535) return ORBX_ERR_UNSUPPORTED;
  size_t total = 0;
  for (int p = 0; p < nprob; ++p) {
    const orbx_sim3_problem& P = problems[p];
    if (P.ncorr < 0 || P.nit < 0 || P.min_inliers < 0 || P.best_in < 0) return ORBX_ERR_ARG;
    if (P.ncorr > S3_MAXN || P.nit > S3_MAXIT) return ORBX_ERR_UNSUPPORTED;
    if (inl_off[p] < 0 || (int64_t)inl_off[p + 1] - inl_off[p] < P.ncorr) return ORBX_ERR_ARG;
    if (!inert(P)) {
      const int rc = problem_ok(P);
      if (rc) return rc;
    }
    total += (size_t)P.ncorr;
  }
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  struct In {
    Slot<float> pos1, pos2, sig1, sig2;
    Slot<int32_t> triples;
    Slot<S3Rec> corr;
    Slot<float> hyp;
  };
  std::vector<In> in((size_t)nprob);
  const auto s_tab = A.in<S3Problem>((size_t)nprob);
  for (int p = 0; p < nprob; ++p) {
    const orbx_sim3_problem& P = problems[p];
    if (inert(P)) continue;
    const size_t n = (size_t)P.ncorr;
    in[p].pos1 = A.in(P.pos1, 3 * n);
    in[p].pos2 = A.in(P.pos2, 3 * n);
    in[p].sig1 = A.in(P.sigma2_1, n);
    in[p].sig2 = A.in(P.sigma2_2, n);
    in[p].triples = A.in(P.triples, (size_t)P.nit * 3);
  }
  const auto s_res = A.out<orbx_sim3_result>(res, (size_t)nprob);
  const auto s_inl = A.out<uint8_t>(nullptr, total);  // packed; scattered to inl_off below
  for (int p = 0; p < nprob; ++p) {
    const orbx_sim3_problem& P = problems[p];
    if (inert(P)) continue;
    in[p].corr = A.scratch<S3Rec>((size_t)P.ncorr);
    in[p].hyp = A.scratch<float>((size_t)P.nit * S3_HYP);
  }
  const int rc = A.commit();
  if (rc) return rc;
  S3Problem* tab = A.h(s_tab);
  size_t off = 0;
  for (int p = 0; p < nprob; ++p) {
    const orbx_sim3_problem& P = problems[p];
    S3Problem& B = tab[p];
    memset(&B, 0, sizeof B);
    B.inl = A.d(s_inl) + off;
    B.res = A.d(s_res) + p;
    B.ncorr = P.ncorr;
    B.best_in = P.best_in;
    B.min_inliers = P.min_inliers;
    off += (size_t)P.ncorr;
    if (inert(P)) continue;  // nit stays 0: no iteration, it_hit = it_best = -1, the flags cleared
    B.pos1 = A.d(in[p].pos1);
    B.pos2 = A.d(in[p].pos2);
    B.sigma2_1 = A.d(in[p].sig1);
    B.sigma2_2 = A.d(in[p].sig2);
    B.triples = A.d(in[p].triples);
    B.corr = A.d(in[p].corr);
    B.hyp = A.d(in[p].hyp);
    memcpy(B.pose, P.Rcw1, sizeof(float) * 9);
    memcpy(B.pose + 9, P.tcw1, sizeof(float) * 3);
    memcpy(B.pose + 12, P.Rcw2, sizeof(float) * 9);
    memcpy(B.pose + 21, P.tcw2, sizeof(float) * 3);
    const float cams[8] = {P.fx1, P.fy1, P.cx1, P.cy1, P.fx2, P.fy2, P.cx2, P.cy2};
    memcpy(B.cams, cams, sizeof cams);
    B.nit = P.nit;
    B.fix_scale = P.fix_scale != 0;
  }
  if (A.upload()) return ORBX_ERR_HIP;
  launch_sim3(A.d(s_tab), nprob, A.stream());
  const int frc = A.finish();
  if (frc) return frc;
  const uint8_t* h = A.h(s_inl);
  off = 0;
  for (int p = 0; p < nprob; ++p) {
    memcpy(inliers + inl_off[p], h + off, (size_t)problems[p].ncorr);
    off += (size_t)problems[p].ncorr;
  }
  return ORBX_OK;
}

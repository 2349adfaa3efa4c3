// api_initransac.hip -- C ABI of the batched Initializer RANSAC
// (kernels_initransac.hip): the synchronous host-pointer form on
// the call arena.  The host builds mvMatches12 and runs Normalize (O(n),
// sequential float sums) in the reference's order; everything per hypothesis
// runs on the device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/orbx.h"
#include "api_common.h"
#include "call_arena.h"
#include "initransac_internal.h"

using namespace orbx;

static_assert(sizeof(orbx_keypoint) % sizeof(float) == 0, "keys are read with a float stride");
static_assert(sizeof(orbx_ransac_result) == 24 * 4, "orbx_ransac_result layout");

// the checks of one pair; *nmatch = the match list's length
static int pair_ok(const orbx_ransac_pair& P, int nit, int* nmatch) {
  if (P.n1 < 0 || P.n2 < 0 || !P.keys1 || !P.keys2 || !P.match12 || (nit > 0 && !P.sets)) return ORBX_ERR_ARG;
  if (P.n1 > IR_MAXN || P.n2 > IR_MAXN) return ORBX_ERR_UNSUPPORTED;
  for (int i = 0; i < P.n1; ++i)
    if (!isfinite(P.keys1[i].x) || !isfinite(P.keys1[i].y)) return ORBX_ERR_ARG;
  for (int i = 0; i < P.n2; ++i)
    if (!isfinite(P.keys2[i].x) || !isfinite(P.keys2[i].y)) return ORBX_ERR_ARG;
  int nm = 0;
  for (int i = 0; i < P.n1; ++i) {
    if (P.match12[i] >= P.n2) return ORBX_ERR_ARG;
    nm += P.match12[i] >= 0;
  }
  if (nm < 8) return ORBX_ERR_ARG;  // the draw of :49-63 would run its index vector empty
  for (size_t i = 0; i < (size_t)nit * 8; ++i)
    if (P.sets[i] < 0 || P.sets[i] >= nm) return ORBX_ERR_ARG;
  *nmatch = nm;
  return ORBX_OK;
}

extern "C" int orbm_initializer_ransac(int npair, const orbx_ransac_pair* pairs, int nit, float sigma, int device,
                                       orbx_ransac_result* res, uint8_t* inliers_H, uint8_t* inliers_F,
                                       const int32_t* inl_off) {
  if (npair < 0 || nit < 0) return ORBX_ERR_ARG;
  if (npair == 0) return ORBX_OK;
  if (!pairs || !res || !inliers_H || !inliers_F || !inl_off || !isfinite(sigma)) return ORBX_ERR_ARG;
  if (nit > IR_MAXIT || npair > 65535) return ORBX_ERR_UNSUPPORTED;
  std::vector<int> nmatch((size_t)npair);
  size_t total = 0;
  for (int p = 0; p < npair; ++p) {
    const int rc = pair_ok(pairs[p], nit, &nmatch[p]);
    if (rc) return rc;
    if (inl_off[p] < 0 || (int64_t)inl_off[p + 1] - inl_off[p] < nmatch[p]) return ORBX_ERR_ARG;
    total += (size_t)nmatch[p];
  }
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  struct In {
    Slot<IrRec> rec, recn;
    Slot<int32_t> sets;
  };
  std::vector<In> in((size_t)npair);
  const auto s_tab = A.in<IrProblem>((size_t)npair);
  for (int p = 0; p < npair; ++p) {
    in[p].rec = A.in<IrRec>((size_t)nmatch[p]);
    in[p].recn = A.in<IrRec>((size_t)nmatch[p]);
    in[p].sets = A.in(pairs[p].sets, (size_t)nit * 8);
  }
  const auto s_res = A.out<orbx_ransac_result>(res, (size_t)npair);
  const auto s_inlH = A.out<uint8_t>(nullptr, total);  // packed; scattered to inl_off below
  const auto s_inlF = A.out<uint8_t>(nullptr, total);
  const auto s_hyp = A.scratch<float>((size_t)npair * nit * IR_HYP);
  const auto s_score = A.scratch<float>((size_t)npair * nit * 2);
  const int rc = A.commit();
  if (rc) return rc;
  IrProblem* tab = A.h(s_tab);
  std::vector<float> pn1, pn2;
  const int kstride = (int)(sizeof(orbx_keypoint) / sizeof(float));
  size_t off = 0;
  for (int p = 0; p < npair; ++p) {
    const orbx_ransac_pair& P = pairs[p];
    IrProblem& B = tab[p];
    memset(&B, 0, sizeof B);
    pn1.resize((size_t)P.n1 * 2);
    pn2.resize((size_t)P.n2 * 2);
    float T2[9];
    ir_normalize(&P.keys1[0].x, kstride, P.n1, pn1.data(), B.T1);
    ir_normalize(&P.keys2[0].x, kstride, P.n2, pn2.data(), T2);
    ir_inv3(T2, B.T2inv);
    ir_transpose3(T2, B.T2t);
    IrRec* rec = A.h(in[p].rec);
    IrRec* recn = A.h(in[p].recn);
    for (int i = 0, k = 0; i < P.n1; ++i) {
      const int j = P.match12[i];
      if (j < 0) continue;
      rec[k] = {P.keys1[i].x, P.keys1[i].y, P.keys2[j].x, P.keys2[j].y};
      recn[k] = {pn1[2 * (size_t)i], pn1[2 * (size_t)i + 1], pn2[2 * (size_t)j], pn2[2 * (size_t)j + 1]};
      ++k;
    }
    B.rec = A.d(in[p].rec);
    B.recn = A.d(in[p].recn);
    B.sets = A.d(in[p].sets);
    B.hyp = A.d(s_hyp) + (size_t)p * nit * IR_HYP;
    B.score = A.d(s_score) + (size_t)p * nit * 2;
    B.inl_H = A.d(s_inlH) + off;
    B.inl_F = A.d(s_inlF) + off;
    B.res = A.d(s_res) + p;
    B.nmatch = nmatch[p];
    off += (size_t)nmatch[p];
  }
  if (A.upload()) return ORBX_ERR_HIP;
  launch_initransac(A.d(s_tab), npair, nit, ir_inv_sigma2(sigma), A.stream());
  const int frc = A.finish();
  if (frc) return frc;
  const uint8_t* hH = A.h(s_inlH);
  const uint8_t* hF = A.h(s_inlF);
  off = 0;
  for (int p = 0; p < npair; ++p) {
    memcpy(inliers_H + inl_off[p], hH + off, (size_t)nmatch[p]);
    memcpy(inliers_F + inl_off[p], hF + off, (size_t)nmatch[p]);
    off += (size_t)nmatch[p];
  }
  return ORBX_OK;
}

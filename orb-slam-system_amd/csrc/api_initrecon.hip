// api_initrecon.hip -- C ABI of the batched Initializer reconstruction
// (kernels_initrecon.hip): the synchronous host-pointer form on
// the call arena.  The host resolves the model (:73), counts N and compacts the
// inlier matches of the model used (:757-764 skips the others); everything per
// candidate and per match runs on the device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/orbx.h"
#include "api_common.h"
#include "call_arena.h"
#include "initrecon_internal.h"

using namespace orbx;

static_assert(sizeof(orbx_recon_result) == 33 * 4, "orbx_recon_result layout");

namespace {

struct Resolved {
  int model;    // ORBX_RECON_H or ORBX_RECON_F
  int present;  // its matrix exists
  int N;        // set flags of that model
  const uint8_t* flags;
};

// the checks of one pair
int pair_ok(const orbx_recon_pair& P, Resolved* out) {
  if (P.n1 < 0 || P.n2 < 0 || !P.keys1 || !P.keys2 || !P.match12 || !P.ransac) return ORBX_ERR_ARG;
  if (P.model != ORBX_RECON_H && P.model != ORBX_RECON_F && P.model != ORBX_RECON_AUTO) return ORBX_ERR_ARG;
  if (P.n1 > IR_MAXN || P.n2 > IR_MAXN) return ORBX_ERR_UNSUPPORTED;
  if (P.model == ORBX_RECON_AUTO && (!P.inliers_H || !P.inliers_F)) return ORBX_ERR_ARG;
  const int model = P.model == ORBX_RECON_AUTO ? (rc_choose_model(P.ransac->RH) ? ORBX_RECON_F : ORBX_RECON_H) : P.model;
  const uint8_t* flags = model == ORBX_RECON_H ? P.inliers_H : P.inliers_F;
  if (!flags) return ORBX_ERR_ARG;
  for (int e = 0; e < 9; ++e)
    if (!isfinite(P.K[e])) return ORBX_ERR_ARG;
  for (int i = 0; i < P.n1; ++i)
    if (!isfinite(P.keys1[i].x) || !isfinite(P.keys1[i].y)) return ORBX_ERR_ARG;
  for (int i = 0; i < P.n2; ++i)
    if (!isfinite(P.keys2[i].x) || !isfinite(P.keys2[i].y)) return ORBX_ERR_ARG;
  int nm = 0;
  for (int i = 0; i < P.n1; ++i) {
    if (P.match12[i] >= P.n2) return ORBX_ERR_ARG;
    nm += P.match12[i] >= 0;
  }
  if (P.ransac->nmatch != nm) return ORBX_ERR_ARG;
  int N = 0;
  for (int i = 0; i < nm; ++i) N += flags[i] != 0;
  out->model = model;
  out->present = (model == ORBX_RECON_H ? P.ransac->it_H : P.ransac->it_F) >= 0;
  out->N = N;
  out->flags = flags;
  return ORBX_OK;
}

}  // namespace

extern "C" int orbm_initializer_reconstruct(int npair, const orbx_recon_pair* pairs, float sigma, float min_parallax,
                                            int min_triangulated, int device, orbx_recon_result* res, float* P3D,
                                            uint8_t* triangulated, const int32_t* key_off) {
  if (npair < 0) return ORBX_ERR_ARG;
  if (npair == 0) return ORBX_OK;
  if (!pairs || !res || !P3D || !triangulated || !key_off || !isfinite(sigma) || !isfinite(min_parallax))
    return ORBX_ERR_ARG;
  if (npair > 65535) return ORBX_ERR_UNSUPPORTED;
  std::vector<Resolved> rv((size_t)npair);
  size_t total_n1 = 0, total_N = 0;
  int maxN = 0;
  for (int p = 0; p < npair; ++p) {
    const int rc = pair_ok(pairs[p], &rv[p]);
    if (rc) return rc;
    if (key_off[p] < 0 || (int64_t)key_off[p + 1] - key_off[p] < pairs[p].n1) return ORBX_ERR_ARG;
    total_n1 += (size_t)pairs[p].n1;
    total_N += (size_t)rv[p].N;
    if (rv[p].N > maxN) maxN = rv[p].N;
  }
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  struct In {
    Slot<IrRec> rec;
    Slot<int32_t> first;
  };
  std::vector<In> in((size_t)npair);
  const auto s_tab = A.in<RcProblem>((size_t)npair);
  for (int p = 0; p < npair; ++p) {
    in[p].rec = A.in<IrRec>((size_t)rv[p].N);
    in[p].first = A.in<int32_t>((size_t)rv[p].N);
  }
  const auto s_res = A.out<orbx_recon_result>(res, (size_t)npair);
  const auto s_p3d = A.out<float>(nullptr, total_n1 * 3);  // packed; scattered to key_off below
  const auto s_tri = A.out<uint8_t>(nullptr, total_n1);
  const auto s_cand = A.scratch<rc_cand>((size_t)npair * RC_MAXCAND);
  const auto s_stat = A.scratch<RcStat>((size_t)npair);
  const auto s_cos = A.scratch<float>(total_N * RC_MAXCAND);
  const auto s_code = A.scratch<uint8_t>(total_N * RC_MAXCAND);
  const int rc = A.commit();
  if (rc) return rc;
  RcProblem* tab = A.h(s_tab);
  size_t off1 = 0, offN = 0;
  for (int p = 0; p < npair; ++p) {
    const orbx_recon_pair& P = pairs[p];
    RcProblem& B = tab[p];
    memset(&B, 0, sizeof B);
    IrRec* rec = A.h(in[p].rec);
    int32_t* first = A.h(in[p].first);
    for (int i = 0, m = 0, k = 0; i < P.n1; ++i) {
      const int j = P.match12[i];
      if (j < 0) continue;
      if (rv[p].flags[m++]) {
        rec[k] = {P.keys1[i].x, P.keys1[i].y, P.keys2[j].x, P.keys2[j].y};
        first[k] = i;
        ++k;
      }
    }
    B.rec = A.d(in[p].rec);
    B.first = A.d(in[p].first);
    B.cand = A.d(s_cand) + (size_t)p * RC_MAXCAND;
    B.cosv = A.d(s_cos) + offN * RC_MAXCAND;
    B.code = A.d(s_code) + offN * RC_MAXCAND;
    B.stat = A.d(s_stat) + p;
    B.P3D = A.d(s_p3d) + off1 * 3;
    B.tri = A.d(s_tri) + off1;
    B.res = A.d(s_res) + p;
    B.N = rv[p].N;
    B.n1 = P.n1;
    B.model = rv[p].model;
    B.present = rv[p].present;
    const float* M = rv[p].model == ORBX_RECON_H ? P.ransac->H21 : P.ransac->F21;
    for (int e = 0; e < 9; ++e) {
      B.K[e] = P.K[e];
      B.M[e] = M[e];
    }
    off1 += (size_t)P.n1;
    offN += (size_t)rv[p].N;
  }
  if (A.upload()) return ORBX_ERR_HIP;
  launch_initrecon(A.d(s_tab), npair, maxN, rc_th2(sigma), min_parallax, min_triangulated, A.stream());
  const int frc = A.finish();
  if (frc) return frc;
  const float* hP = A.h(s_p3d);
  const uint8_t* hT = A.h(s_tri);
  off1 = 0;
  for (int p = 0; p < npair; ++p) {
    const size_t n1 = (size_t)pairs[p].n1;
    memcpy(P3D + 3 * (size_t)key_off[p], hP + 3 * off1, n1 * 3 * sizeof(float));
    memcpy(triangulated + key_off[p], hT + off1, n1);
    off1 += n1;
  }
  return ORBX_OK;
}

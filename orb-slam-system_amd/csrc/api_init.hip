// api_init.hip -- C ABI of ORBmatcher::SearchForInitialization
// (src/ORBmatcher.cc:197-276), batched over independent pairs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/orbx.h"
#include "call_arena.h"
#include "init_internal.h"

namespace orbx {
__global__ void k_grid_build(const ProjProblem*);  // kernels_proj.hip
__global__ void k_init_cand(const InitPair*, float, int);
__global__ void k_init_walk(const InitPair*, float, float, int);
}  // namespace orbx

using namespace orbx;

// the smallest bestDist2 that passes the ratio test for every bestDist <=
// TH_LOW, in the kernel's own arithmetic (:235); beyond TH_LOW so that no
// candidate at the cut or above can be an accepted best.  IN_NOCUT where no
// distance is that large (a small, negative or NaN ratio): nothing is pruned
static int cut_distance(float nnratio) {
  for (int d = IN_TH_LOW + 1; d <= 256; ++d)
    if ((float)IN_TH_LOW < (float)d * nnratio) return d;
  return IN_NOCUT;
}

// nrescan (npair, may be null): rows per pair whose walk step scanned the
// window again (tools/init_latency.py, tests)
extern "C" int orbm_search_for_initialization_stats(int npair, const orbx_init_pair* pairs, int window_size,
                                                    float nnratio, int check_ori, int device, int* nmatches,
                                                    int* nrescan) {
  if (npair < 0 || (npair > 0 && (!pairs || !nmatches))) return ORBX_ERR_ARG;
  int max_n1 = 0, max_n2 = 0;
  for (int p = 0; p < npair; ++p) {
    const orbx_init_pair& Q = pairs[p];
    if (Q.f1.n < 0 || Q.f2.n < 0) return ORBX_ERR_ARG;
    if (Q.f1.n > 0 && (!Q.f1.keys || !Q.f1.desc || !Q.prev_matched || !Q.match12)) return ORBX_ERR_ARG;
    if (Q.f2.n > 0 && (!Q.f2.keys || !Q.f2.desc)) return ORBX_ERR_ARG;
    for (int i = 0; i < 2 * Q.f1.n; ++i)
      if (!isfinite(Q.prev_matched[i])) return ORBX_ERR_ARG;
    for (int i = 0; i < Q.f2.n; ++i)
      if (!isfinite(Q.f2.keys[i].x) || !isfinite(Q.f2.keys[i].y)) return ORBX_ERR_ARG;
    if (check_ori) {  // !(..) also catches a NaN
      for (int i = 0; i < Q.f1.n; ++i)
        if (!(Q.f1.keys[i].angle >= 0.0f && Q.f1.keys[i].angle <= 360.0f)) return ORBX_ERR_ARG;
      for (int i = 0; i < Q.f2.n; ++i)
        if (!(Q.f2.keys[i].angle >= 0.0f && Q.f2.keys[i].angle <= 360.0f)) return ORBX_ERR_ARG;
    }
    max_n1 = std::max(max_n1, Q.f1.n);
    max_n2 = std::max(max_n2, Q.f2.n);
  }
  if (max_n1 > IN_MAXN || max_n2 > IN_MAXN) return ORBX_ERR_UNSUPPORTED;
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  if (npair == 0) return ORBX_OK;
  ORBX_TRY(hipSetDevice(device));
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  if (set_max_dynamic_lds((const void*)k_grid_build, device)) return ORBX_ERR_HIP;
  struct PairSlots {
    Slot<orbx_keypoint> keys1, keys2;
    Slot<uint8_t> desc1, desc2;
    Slot<float> prev_in, prev_out;
    Slot<int32_t> match_in, match_out;
    Slot<int> cell_off, cell_feat, nlow;
    Slot<uint32_t> cand;
  };
  std::vector<PairSlots> ps((size_t)npair);
  for (int p = 0; p < npair; ++p) {
    const orbx_init_pair& Q = pairs[p];
    const size_t n1 = (size_t)Q.f1.n, n2 = (size_t)Q.f2.n;
    ps[p].keys1 = A.in(Q.f1.keys, n1);
    ps[p].desc1 = A.in(Q.f1.desc, n1 * 32);
    ps[p].keys2 = A.in(Q.f2.keys, n2);
    ps[p].desc2 = A.in(Q.f2.desc, n2 * 32);
    ps[p].prev_in = A.in((const float*)Q.prev_matched, 2 * n1);
    ps[p].match_in = A.in((const int32_t*)Q.match12, n1);
  }
  const auto s_pair = A.in<InitPair>((size_t)npair);
  const auto s_grid = A.in<ProjProblem>((size_t)npair);
  // the outputs stay in the staging buffer until the error words are read:
  // a failed call writes nothing
  for (int p = 0; p < npair; ++p) {
    ps[p].prev_out = A.out<float>(nullptr, 2 * (size_t)pairs[p].f1.n);
    ps[p].match_out = A.out<int32_t>(nullptr, (size_t)pairs[p].f1.n);
  }
  const auto s_nm = A.out<int>(nullptr, (size_t)npair);
  const auto s_err = A.out<int>(nullptr, (size_t)npair);
  const auto s_resc = A.out<int>(nullptr, (size_t)npair);
  for (int p = 0; p < npair; ++p) {
    ps[p].cell_off = A.scratch<int>(PG_CELLS + 1);
    ps[p].cell_feat = A.scratch<int>((size_t)pairs[p].f2.n);
    ps[p].cand = A.scratch<uint32_t>((size_t)pairs[p].f1.n * IN_T);
    ps[p].nlow = A.scratch<int>((size_t)pairs[p].f1.n);
  }
  int rc = A.commit();
  if (rc) return rc;
  for (int p = 0; p < npair; ++p) {
    const orbx_init_pair& Q = pairs[p];
    InitPair P = {};
    P.F2.n = Q.f2.n;
    P.F2.minX = Q.f2.min_x;
    P.F2.minY = Q.f2.min_y;
    P.F2.wInv = Q.f2.grid_w_inv;
    P.F2.hInv = Q.f2.grid_h_inv;
    P.n1 = Q.f1.n;
    P.keys1 = A.d(ps[p].keys1);
    P.desc1 = A.d(ps[p].desc1);
    P.keys2 = A.d(ps[p].keys2);
    P.desc2 = A.d(ps[p].desc2);
    P.prev_in = A.d(ps[p].prev_in);
    P.match_in = A.d(ps[p].match_in);
    P.prev_out = A.d(ps[p].prev_out);
    P.match_out = A.d(ps[p].match_out);
    P.cell_off = A.d(ps[p].cell_off);
    P.cell_feat = A.d(ps[p].cell_feat);
    P.cand = A.d(ps[p].cand);
    P.nlow = A.d(ps[p].nlow);
    P.nmatches = A.d(s_nm) + p;
    P.err = A.d(s_err) + p;
    P.nrescan = A.d(s_resc) + p;
    A.h(s_pair)[p] = P;
    ProjProblem G = {};  // what k_grid_build reads
    G.F = P.F2;
    G.keys = P.keys2;
    G.cell_off = A.d(ps[p].cell_off);
    G.cell_feat = A.d(ps[p].cell_feat);
    A.h(s_grid)[p] = G;
  }
  rc = A.upload();
  if (rc) return rc;
  int P2 = 1;
  while (P2 < max_n2) P2 <<= 1;
  const float window = (float)window_size;  // GetFeaturesInArea takes const float& r
  hipLaunchKernelGGL(k_grid_build, dim3((unsigned)npair), dim3(1024), (size_t)P2 * 4, A.stream(), A.d(s_grid));
  if (max_n1 > 0) {
    const int rpb = IN_BLOCK / IN_G;
    hipLaunchKernelGGL(k_init_cand, dim3((unsigned)((max_n1 + rpb - 1) / rpb), (unsigned)npair),
                       dim3(IN_BLOCK), 0, A.stream(), A.d(s_pair), window, cut_distance(nnratio));
  }
  hipLaunchKernelGGL(k_init_walk, dim3((unsigned)npair), dim3(IN_BLOCK), 0, A.stream(), A.d(s_pair), window,
                     nnratio, check_ori ? 1 : 0);
  rc = A.finish();
  if (rc) return rc;
  for (int p = 0; p < npair; ++p)
    if (A.h(s_err)[p]) return ORBX_ERR_ARG;
  for (int p = 0; p < npair; ++p) {
    const size_t n1 = (size_t)pairs[p].f1.n;
    if (n1) {
      memcpy(pairs[p].prev_matched, A.h(ps[p].prev_out), 2 * n1 * sizeof(float));
      memcpy(pairs[p].match12, A.h(ps[p].match_out), n1 * sizeof(int32_t));
    }
    nmatches[p] = A.h(s_nm)[p];
    if (nrescan) nrescan[p] = A.h(s_resc)[p];
  }
  return ORBX_OK;
}

extern "C" int orbm_search_for_initialization(int npair, const orbx_init_pair* pairs, int window_size,
                                              float nnratio, int check_ori, int device, int* nmatches) {
  return orbm_search_for_initialization_stats(npair, pairs, window_size, nnratio, check_ori, device, nmatches,
                                              nullptr);
}

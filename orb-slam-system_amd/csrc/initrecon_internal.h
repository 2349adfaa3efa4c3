// initrecon_internal.h -- shared by kernels_initrecon.hip and
// api_initrecon.hip: the device problem table and the kernels.
#ifndef ORBX_INITRECON_INTERNAL_H
#define ORBX_INITRECON_INTERNAL_H

#include <hip/hip_runtime.h>

#include "../../include/orbx.h"
#include "initransac_internal.h"
#include "initrecon_math.h"

namespace orbx {

constexpr int RC_MAXCAND = 8;    // ReconstructH's candidates; ReconstructF uses the first 4 slots
constexpr int RC_CAND_W = 64;    // pairs per workgroup of the candidates kernel: one per lane
constexpr int RC_TILE = 128;     // inlier matches per workgroup of the CheckRT kernel: one per lane
constexpr int RC_SELECT_T = 256; // lanes of the select kernel = bins of its radix passes
constexpr int RC_DECIDE_T = 128; // lanes of the decide kernel: one retriangulation per lane

// what the candidates and select kernels leave for the decision
struct RcStat {
  int32_t ncand;  // 8, 4, or 0: ReconstructH's exit or an absent model
  int32_t nGood[RC_MAXCAND];
  float parallax[RC_MAXCAND];
};

struct RcProblem {
  const IrRec* rec;       // [N] the inlier matches' image coordinates, match-list order
  const int32_t* first;   // [N] their keys in frame 1, each < n1 (built on the host)
  rc_cand* cand;          // [RC_MAXCAND]
  float* cosv;            // [RC_MAXCAND][N] cosParallax of every inlier match
  uint8_t* code;          // [RC_MAXCAND][N] 0 not counted, 1 counted, 2 counted and triangulated
  RcStat* stat;
  float* P3D;             // [n1][3]
  uint8_t* tri;           // [n1]
  orbx_recon_result* res;
  int N, n1;
  int model;              // ORBX_RECON_H or ORBX_RECON_F: AUTO is resolved on the host
  int present;            // the model's matrix exists (it >= 0)
  float K[9], M[9];       // M: H21 or F21
};

// the four launches of one call on stream s (kernels_initrecon.hip): candidates,
// CheckRT records, nGood / parallax, the decision and the winner's points.
// npair >= 1; maxN = the largest N of the batch
void launch_initrecon(const RcProblem* d_probs, int npair, int maxN, float th2, float min_parallax,
                      int min_triangulated, hipStream_t s);

}  // namespace orbx

#endif

// poseopt_internal.h -- shared by kernels_poseopt.hip and api_poseopt.hip
// (DESIGN.md §19): the device problem table is the public orbx_pose_problem.
#ifndef ORBX_POSEOPT_INTERNAL_H
#define ORBX_POSEOPT_INTERNAL_H

#include <hip/hip_runtime.h>

#include "../../include/orbx.h"
#include "poseopt_math.h"

namespace orbx {

// one workgroup of PO_T lanes per problem; its LDS: the PO_NSUM x PO_T partial
// sums of a reduction, the solve's work space and x, three counters
constexpr int PO_LDS_BYTES = (PO_NSUM * PO_T + 42 + 6 + 2) * 8 + 16;

__global__ void k_pose_optimize(const orbx_pose_problem* probs);

// a camera / observation pair the forms accept (counts and required pointers;
// the per-feature checks are the host form's own)
inline bool pose_args_ok(const orbx_pose_camera& c, const orbx_pose_obs& o, int max_n) {
  if (o.n < 0 || o.n > max_n || c.nlevels < 1 || c.nlevels > ORBX_PROJ_MAX_LEVELS || o.npos < 0) return false;
  if (o.n > 0 && (!o.keys || !o.pos)) return false;
  return true;
}

}  // namespace orbx

#endif

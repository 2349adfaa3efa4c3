// kfbuild_internal.h -- device tables of the projection that feeds the keyframe
// window search (the statements of ORBmatcher::Fuse, src/ORBmatcher.cc:514-531
// and :582-599, and of SearchBySim3, :676-694), shared by kernels_kfbuild.hip,
// kernels_kfwin.hip and api_kfbuild.hip, and the plan's handle.
#ifndef ORBX_KFBUILD_INTERNAL_H
#define ORBX_KFBUILD_INTERNAL_H

#include <stdint.h>

#include "../../include/orbx.h"
#include "kfwin_internal.h"

namespace orbx {

#define KB_BLOCK 256

// one problem of k_kf_build: camera values, PredictScale thresholds, point
// arrays and outputs (device pointers).  Problem = blockIdx.y.
struct KfBuildProblem {
  orbx_kf_camera cam;
  float thr[ORBX_PROJ_MAX_LEVELS];  // nlevels - 1 used
  orbx_kf_points pts;
  int npts;
  int32_t desc_base;  // row i's desc = desc_base + i
  orbx_kf_query* q;
  int32_t* level;    // may be NULL
  int* n_live;       // may be NULL
  int* n_nonfinite;  // may be NULL
};

// one problem of the plan's search (k_kfwin_grid_kp, k_kfwin_search_plan):
// the keyframe's table with key = orbx_keypoint rows, and the problem's own
// queries, descriptor pool and results.  Problem = blockIdx.y.
struct KfwPlanProblem {
  KfwProblem kf;  // kf.key points at orbx_keypoint rows; cell_off NULL = nothing to search
  const orbx_kf_query* qs;
  const uint8_t* qdesc;  // nq x 32
  int nq;
  int32_t* best_idx;
  int32_t* best_dist;
};

}  // namespace orbx

#endif

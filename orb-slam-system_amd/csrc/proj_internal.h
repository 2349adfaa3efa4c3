// proj_internal.h -- device tables of the frame grid and the projection
// matchers (ORBmatcher::SearchByProjection, src/ORBmatcher.cc:19-61,732-894;
// Frame::AssignFeaturesToGrid / GetFeaturesInArea, src/Frame.cc:210-225,307-371),
// shared by kernels_proj.hip and api_proj.hip.
#ifndef ORBX_PROJ_INTERNAL_H
#define ORBX_PROJ_INTERNAL_H

#include <stdint.h>

#include "../../include/orbx.h"

namespace orbx {

#define PG_COLS 64 /* FRAME_GRID_COLS (include/Frame.h:18) */
#define PG_ROWS 48 /* FRAME_GRID_ROWS (include/Frame.h:17) */
#define PG_CELLS (PG_COLS * PG_ROWS)
#define PJ_T 8     /* candidates kept per query */
#define PJ_MAXN 8192

struct ProjFrame {
  int n;
  float minX, minY, wInv, hInv;
};

// one SearchByProjection call: the frame, its queries, outputs and grid /
// candidate scratch (device pointers).  The drop-in call launches one; the
// batched plan (orbm_proj_plan_search) launches many at once, problem =
// blockIdx.y (candidates) or blockIdx.x (grid, walk).
struct ProjProblem {
  ProjFrame F;
  const orbx_keypoint* keys;
  const uint8_t* desc;
  const float* uright;
  const uint8_t* occupied;
  const orbx_query_proj* qs;
  const uint8_t* qdesc;
  int nq;
  int32_t* match;
  int* nmatches;
  int* cell_off;   // PG_CELLS + 1
  int* cell_feat;  // n
  uint32_t* cand;  // nq x PJ_T
  int* ncand;      // nq
};

}  // namespace orbx

#endif

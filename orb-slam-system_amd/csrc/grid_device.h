// grid_device.h -- Frame::GetFeaturesInArea's cell bounds over the grid that
// k_grid_build (kernels_proj.hip) lays out, shared by the kernels that search
// it: kernels_proj.hip (SearchByProjection) and kernels_init.hip
// (SearchForInitialization).
#ifndef ORBX_GRID_DEVICE_H
#define ORBX_GRID_DEVICE_H

#include <hip/hip_runtime.h>

#include "proj_internal.h"

namespace orbx {

// GetFeaturesInArea cell bounds (src/Frame.cc:312-326); false = empty
__device__ __forceinline__ bool area_cells(const ProjFrame& F, float x, float y, float r,
                                           int* x0, int* x1, int* y0, int* y1) {
  const int mincx = (int)floorf((x - F.minX - r) * F.wInv);
  *x0 = mincx > 0 ? mincx : 0;
  if (*x0 >= PG_COLS) return false;
  const int maxcx = (int)ceilf((x - F.minX + r) * F.wInv);
  *x1 = maxcx < PG_COLS - 1 ? maxcx : PG_COLS - 1;
  if (*x1 < 0) return false;
  const int mincy = (int)floorf((y - F.minY - r) * F.hInv);
  *y0 = mincy > 0 ? mincy : 0;
  if (*y0 >= PG_ROWS) return false;
  const int maxcy = (int)ceilf((y - F.minY + r) * F.hInv);
  *y1 = maxcy < PG_ROWS - 1 ? maxcy : PG_ROWS - 1;
  if (*y1 < 0) return false;
  return true;
}

}  // namespace orbx

#endif

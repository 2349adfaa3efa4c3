// init_internal.h -- device tables of ORBmatcher::SearchForInitialization
// (src/ORBmatcher.cc:197-276), shared by kernels_init.hip and api_init.hip.
//
// One "pair" = one call of the member function: the rows of F1 search F2's
// frame grid (k_grid_build, kernels_proj.hip) around vbPrevMatched.  Per row
// k_init_cand keeps the IN_T smallest (distance, visiting rank) keys among the
// candidates below the cut distance and their number;
// k_init_walk, one workgroup per pair, then walks the rows in order.
#ifndef ORBX_INIT_INTERNAL_H
#define ORBX_INIT_INTERNAL_H

#include <stdint.h>

#include "../../include/orbx.h"
#include "proj_internal.h"

namespace orbx {

#define IN_T 8         /* candidates below the cut kept per row                   */
#define IN_G 16        /* lanes per row in k_init_cand                            */
#define IN_BLOCK 256   /* threads per block of both kernels                       */
#define IN_BATCH 256   /* rows whose lists the walk stages in LDS at a time       */
#define IN_MAXN 8192   /* features per frame: 16-bit indices, the walk's LDS      */
#define IN_TH_LOW 50   /* ORBmatcher::TH_LOW (src/ORBmatcher.cc:14)               */
#define IN_NOCUT 257   /* a cut above every distance: the pruning is off          */

struct InitPair {
  ProjFrame F2;  // f2.n and f2's grid constants
  int n1;
  const orbx_keypoint* keys1;  // n1 (octave, angle)
  const uint8_t* desc1;        // n1 x 32
  const orbx_keypoint* keys2;  // n2
  const uint8_t* desc2;        // n2 x 32
  const float* prev_in;        // 2 * n1
  const int32_t* match_in;     // n1
  float* prev_out;             // 2 * n1
  int32_t* match_out;          // n1
  const int* cell_off;         // PG_CELLS + 1
  const int* cell_feat;        // n2
  uint32_t* cand;              // n1 x IN_T: distance << 16 | f2 index, in (distance, rank) order
  int* nlow;                   // n1: candidates below the cut (the list is complete iff <= IN_T);
                               //     0 also where the closest one is beyond TH_LOW (nothing to walk)
  int* nmatches;               // 1
  int* err;                    // 1: a row ends the call holding an entry >= n2
  int* nrescan;                // 1: rows whose walk step scanned the window again
};

}  // namespace orbx

#endif

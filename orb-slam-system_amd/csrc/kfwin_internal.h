// kfwin_internal.h -- device tables of the keyframe window search shared by
// ORBmatcher::Fuse (both forms) and SearchBySim3 (src/ORBmatcher.cc:504-730):
// KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:549-588), the octave gate and
// the first strict minimum of DescriptorDistance.
//
// One "problem" = the queries of one call's map points in one keyframe.  The
// keyframe's features are written once in the grid's visiting order (ix, iy,
// index) as packed records; the cells (ix, y0..y1) of a query are then one
// contiguous run of records, read KFW_G at a time by the query's lane group.
#ifndef ORBX_KFWIN_INTERNAL_H
#define ORBX_KFWIN_INTERNAL_H

#include <stdint.h>

#ifndef KFW_G          /* tools/variant.sh may override it for the probe */
#define KFW_G 8        /* lanes per query (the measured run lengths) */
#endif
#define KFW_BLOCK 256  /* threads per search block = KFW_BLOCK / KFW_G queries    */
#define KFW_MAXN 8192  /* features per keyframe: the grid kernel's LDS sort       */
#define KFW_COLS 64    /* FRAME_GRID_COLS (include/Frame.h:18) */
#define KFW_ROWS 48    /* FRAME_GRID_ROWS (include/Frame.h:17) */
#define KFW_CELLS (KFW_COLS * KFW_ROWS)

/* the fields of mvKeysUn[i] the search reads, as uploaded (12 of the 28 bytes) */
struct KfwKey {
  float x, y;
  int32_t octave;
};

/* one feature in visiting order: 48 bytes, three 16-byte loads.  The octave
 * has a word of its own (the record is padded to 48 bytes anyway), so any
 * int32 octave is carried, not only 16 bits of it */
struct alignas(16) KfwRec {
  float x, y;
  int32_t index;
  int32_t octave;
  uint32_t d[8];
};

struct KfwProblem {
  int n;
  float minX, minY, wInv, hInv;
  const KfwKey* key;    /* n */
  const uint8_t* desc;  /* n x 32 */
  int* cell_off;        /* KFW_CELLS + 1: ix-major prefix of the cell sizes */
  KfwRec* rec;          /* n (the features inside the grid come first)     */
};

#endif

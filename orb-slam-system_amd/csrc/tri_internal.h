// tri_internal.h -- device tables of the SearchForTriangulation pipeline
// (src/ORBmatcher.cc:368-467).
//
// One "problem" = one SearchForTriangulation(KF1, KF2[p], F12[p]) call; KF1 is
// shared by every problem of a batch.  A common vocabulary node of a problem
// is cut into "items" of up to TRI_ROWS KF1 rows, each searched by one
// wavefront over the node's whole KF2 list.
#ifndef ORBX_TRI_INTERNAL_H
#define ORBX_TRI_INTERNAL_H

#include <stdint.h>

#define TRI_ROWS 64   /* KF1 rows per item: one lane each                       */
#define TRI_CHUNK 64  /* KF2 list entries staged in LDS at a time (one per lane) */

/* the fields of a keypoint the search reads (mvKeysUn[i].pt, .angle, .octave) */
struct alignas(16) TriKey {
  float x, y, angle;
  int32_t octave;
};

struct TriFrame {
  const TriKey* key;
  const uint8_t* desc;    /* n x 32 */
  const uint8_t* has_mp;  /* n, or nullptr */
  const uint32_t* feat;
};

struct TriProblem {
  TriFrame kf2;
  const float* sigma2;  /* kf2's mvLevelSigma2 */
  float F[9];           /* F12, row-major */
  int2* row;            /* [n1] per KF1 feature: (bestIdx2, mask of the rotation bins it touched) */
  int* hist;            /* [32] rotation events per bin (30 used) */
  int32_t* match12;     /* [n1] */
  int* nmatches;
};

struct TriItem {
  int prob;
  int off1, n1;  /* rows = kf1.feat[off1 .. off1+n1), n1 <= TRI_ROWS */
  int off2, n2;  /* list2 = kf2.feat[off2 .. off2+n2) */
};

#endif

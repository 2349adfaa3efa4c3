/* initsearch_ref.c -- CPU restatement of ORBmatcher::SearchForInitialization
 * (src/ORBmatcher.cc:197-276) and of what it calls: Frame::GetFeaturesInArea
 * (src/Frame.cc:307-358) over the grid Frame::AssignFeaturesToGrid fills
 * (src/Frame.cc:210-225, PosInGrid :362-372), DescriptorDistance (:896-908)
 * and ComputeThreeMaxima (:469-502).  Statement for statement, with real
 * per-cell lists filled in index order and real rotHist lists; the yardstick
 * of orbm_search_for_initialization.  Built by tests/initsearch_util.py with
 * gcc -O2 -ffp-contract=off. */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define GRID_COLS 64 /* FRAME_GRID_COLS */
#define GRID_ROWS 48 /* FRAME_GRID_ROWS */
#define TH_LOW 50
#define HISTO_LENGTH 30

typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} ini_keypoint; /* cv::KeyPoint == orbx_keypoint */

typedef struct {
  int n;
  const ini_keypoint* keys;
  const uint8_t* desc;
  float min_x, min_y, grid_w_inv, grid_h_inv;
} ini_frame; /* == orbx_kf_frame */

/* std::vector<int> / std::vector<size_t> */
typedef struct {
  int* v;
  int size, cap;
} int_list;

static void push_back(int_list* c, int i) {
  if (c->size == c->cap) {
    c->cap = c->cap ? 2 * c->cap : 4;
    c->v = (int*)realloc(c->v, (size_t)c->cap * sizeof(int));
  }
  c->v[c->size++] = i;
}

/* (int) of a float as the reference's x86 object converts it (cvttss2si): out
 * of int's range or NaN gives INT_MIN; in C the cast alone would be undefined */
static int f2i(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT_MIN; }
static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

typedef struct {
  int_list cell[GRID_COLS][GRID_ROWS]; /* mGrid */
  const ini_frame* f;
} ini_grid;

/* Frame::AssignFeaturesToGrid with PosInGrid */
static ini_grid* grid_create(const ini_frame* f) {
  ini_grid* g = (ini_grid*)calloc(1, sizeof(ini_grid));
  g->f = f;
  for (int i = 0; i < f->n; i++) {
    const ini_keypoint* kp = &f->keys[i];
    const int posX = f2i(roundf((kp->x - f->min_x) * f->grid_w_inv));
    const int posY = f2i(roundf((kp->y - f->min_y) * f->grid_h_inv));
    if (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) continue;
    push_back(&g->cell[posX][posY], i);
  }
  return g;
}

static void grid_free(ini_grid* g) {
  for (int ix = 0; ix < GRID_COLS; ix++)
    for (int iy = 0; iy < GRID_ROWS; iy++) free(g->cell[ix][iy].v);
  free(g);
}

/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) into vIndices */
static void get_features_in_area(const ini_grid* g, float x, float y, float r, int minLevel, int maxLevel,
                                 int_list* vIndices) {
  const ini_frame* f = g->f;
  vIndices->size = 0;

  const int nMinCellX = imax(0, f2i(floorf((x - f->min_x - r) * f->grid_w_inv)));
  if (nMinCellX >= GRID_COLS) return;

  const int nMaxCellX = imin(GRID_COLS - 1, f2i(ceilf((x - f->min_x + r) * f->grid_w_inv)));
  if (nMaxCellX < 0) return;

  const int nMinCellY = imax(0, f2i(floorf((y - f->min_y - r) * f->grid_h_inv)));
  if (nMinCellY >= GRID_ROWS) return;

  const int nMaxCellY = imin(GRID_ROWS - 1, f2i(ceilf((y - f->min_y + r) * f->grid_h_inv)));
  if (nMaxCellY < 0) return;

  const int bCheckLevels = (minLevel > 0) || (maxLevel >= 0);

  for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
    for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
      const int_list* vCell = &g->cell[ix][iy];
      if (vCell->size == 0) continue;

      for (int j = 0, jend = vCell->size; j < jend; j++) {
        const ini_keypoint* kpUn = &f->keys[vCell->v[j]];
        if (bCheckLevels) {
          if (kpUn->octave < minLevel) continue;
          if (maxLevel >= 0)
            if (kpUn->octave > maxLevel) continue;
        }

        const float distx = kpUn->x - x;
        const float disty = kpUn->y - y;

        if (fabsf(distx) < r && fabsf(disty) < r) push_back(vIndices, vCell->v[j]);
      }
    }
  }
}

/* ORBmatcher::DescriptorDistance */
int ini_descriptor_distance(const uint8_t* a, const uint8_t* b) {
  int dist = 0;
  for (int i = 0; i < 8; i++) {
    uint32_t pa, pb;
    memcpy(&pa, a + 4 * i, 4);
    memcpy(&pb, b + 4 * i, 4);
    unsigned int v = pa ^ pb;
    v = v - ((v >> 1) & 0x55555555);
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
    dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
  }
  return dist;
}

/* ORBmatcher::ComputeThreeMaxima */
static void compute_three_maxima(const int_list* histo, int L, int* ind1, int* ind2, int* ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int s = histo[i].size;
    if (s > max1) {
      max3 = max2;
      max2 = max1;
      max1 = s;
      *ind3 = *ind2;
      *ind2 = *ind1;
      *ind1 = i;
    } else if (s > max2) {
      max3 = max2;
      max2 = s;
      *ind3 = *ind2;
      *ind2 = i;
    } else if (s > max3) {
      max3 = s;
      *ind3 = i;
    }
  }
  if (max2 < 0.1f * (float)max1) {
    *ind2 = -1;
    *ind3 = -1;
  } else if (max3 < 0.1f * (float)max1) {
    *ind3 = -1;
  }
}

enum { ST_ACCEPTED, ST_DISPLACED, ST_FILTER_CHANGED, ST_RATIO_REJECTED, ST_ROT_REMOVED, ST_STALE, ST_NLOW, ST_N };

/* One call.  prev_matched (2 * f1->n) and match12 (f1->n, resized by the
 * caller and not cleared, :199) are in/out; *nmatches = the return value.
 * stats (may be NULL): ST_N ints per row -- accepted by this call; displaced
 * by a later row's steal; the filter dist < vMatchedDistance changed its
 * winner (the first strict minimum over all candidates is another feature than
 * the walk's best, or the walk has none); bestDist <= TH_LOW but the ratio
 * test rejected it; the rotation check removed it; a stale survivor (not
 * accepted by this call, still >= 0); candidates with distance < dcut.
 * Returns 0, or -1 where :272 would read past F2.mvKeysUn (that row's
 * prev_matched is then left alone). */
int ini_search(const ini_frame* F1, const ini_frame* F2, float* vbPrevMatched, int32_t* vnMatches12,
               int windowSize, float mfNNratio, int mbCheckOrientation, int dcut, int* nmatches_out,
               int32_t* stats) {
  int nmatches = 0;
  int rc = 0;
  const int n1 = F1->n, n2 = F2->n;
  ini_grid* g = grid_create(F2);
  int_list vIndices2 = {0, 0, 0};

  int_list rotHist[HISTO_LENGTH];
  memset(rotHist, 0, sizeof(rotHist));
  const float factor = 1.0f / HISTO_LENGTH;

  int* vMatchedDistance = (int*)malloc((size_t)(n2 > 0 ? n2 : 1) * sizeof(int));
  int* vnMatches21 = (int*)malloc((size_t)(n2 > 0 ? n2 : 1) * sizeof(int));
  for (int i = 0; i < n2; i++) {
    vMatchedDistance[i] = INT_MAX;
    vnMatches21[i] = -1;
  }
  if (stats) memset(stats, 0, (size_t)n1 * ST_N * sizeof(int32_t));

  for (int i1 = 0; i1 < n1; i1++) {
    const ini_keypoint* kp1 = &F1->keys[i1];
    if (kp1->octave > 0) continue;

    get_features_in_area(g, vbPrevMatched[2 * i1], vbPrevMatched[2 * i1 + 1], (float)windowSize, kp1->octave,
                         kp1->octave, &vIndices2);
    if (vIndices2.size == 0) continue;

    const uint8_t* d1 = F1->desc + (size_t)i1 * 32;
    int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
    int freeDist = INT_MAX, freeIdx = -1, nlow = 0; /* statistics only */

    for (int k = 0; k < vIndices2.size; k++) {
      const int i2 = vIndices2.v[k];
      const uint8_t* d2 = F2->desc + (size_t)i2 * 32;
      int dist = ini_descriptor_distance(d1, d2);

      if (dist < dcut) nlow++;
      if (dist < freeDist) {
        freeDist = dist;
        freeIdx = i2;
      }

      if (dist < vMatchedDistance[i2]) {
        if (dist < bestDist) {
          bestDist2 = bestDist;
          bestDist = dist;
          bestIdx2 = i2;
        } else if (dist < bestDist2) {
          bestDist2 = dist;
        }
      }
    }
    if (stats) {
      stats[ST_N * i1 + ST_NLOW] = nlow;
      stats[ST_N * i1 + ST_FILTER_CHANGED] = freeIdx != bestIdx2;
    }

    if (bestDist <= TH_LOW && bestDist < (float)bestDist2 * mfNNratio) {
      if (vnMatches21[bestIdx2] >= 0) {
        vnMatches12[vnMatches21[bestIdx2]] = -1;
        nmatches--;
        if (stats) stats[ST_N * vnMatches21[bestIdx2] + ST_DISPLACED] = 1;
      }
      vnMatches12[i1] = bestIdx2;
      vnMatches21[bestIdx2] = i1;
      vMatchedDistance[bestIdx2] = bestDist;
      nmatches++;
      if (stats) stats[ST_N * i1 + ST_ACCEPTED] = 1;

      if (mbCheckOrientation) {
        float rot = kp1->angle - F2->keys[bestIdx2].angle;
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        push_back(&rotHist[bin], i1);
      }
    } else if (stats && bestDist <= TH_LOW) {
      stats[ST_N * i1 + ST_RATIO_REJECTED] = 1;
    }
  }

  if (mbCheckOrientation) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    compute_three_maxima(rotHist, HISTO_LENGTH, &ind1, &ind2, &ind3);

    for (int i = 0; i < HISTO_LENGTH; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int j = 0; j < rotHist[i].size; j++) {
        const int idx1 = rotHist[i].v[j];
        if (vnMatches12[idx1] >= 0) {
          vnMatches12[idx1] = -1;
          nmatches--;
          if (stats) stats[ST_N * idx1 + ST_ROT_REMOVED] = 1;
        }
      }
    }
  }

  for (int i1 = 0; i1 < n1; i1++) {
    if (vnMatches12[i1] >= 0) {
      if (stats && !stats[ST_N * i1 + ST_ACCEPTED]) stats[ST_N * i1 + ST_STALE] = 1;
      if (vnMatches12[i1] >= n2) {
        rc = -1;
        continue;
      }
      vbPrevMatched[2 * i1] = F2->keys[vnMatches12[i1]].x;
      vbPrevMatched[2 * i1 + 1] = F2->keys[vnMatches12[i1]].y;
    }
  }

  for (int i = 0; i < HISTO_LENGTH; i++) free(rotHist[i].v);
  free(vIndices2.v);
  free(vMatchedDistance);
  free(vnMatches21);
  grid_free(g);
  *nmatches_out = nmatches;
  return rc;
}

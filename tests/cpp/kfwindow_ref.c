/* kfwindow_ref.c -- CPU restatement of the search ORBmatcher::Fuse (both
 * forms) and SearchBySim3 share (src/ORBmatcher.cc:532-551, :600-619,
 * :696-714): KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:549-588) over the
 * grid Frame::AssignFeaturesToGrid fills (src/Frame.cc:210-225, PosInGrid
 * :362-372; KeyFrame copies it, src/KeyFrame.cc:28-33), the octave gate and the
 * first strict minimum of DescriptorDistance.  Statement for statement, with
 * real per-cell lists filled in index order; the yardstick of
 * orbm_keyframe_search.  Built by tests/kfwindow_util.py with
 * gcc -O2 -ffp-contract=off. */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define GRID_COLS 64 /* FRAME_GRID_COLS */
#define GRID_ROWS 48 /* FRAME_GRID_ROWS */

typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} kfw_keypoint; /* cv::KeyPoint == orbx_keypoint */

typedef struct {
  float x, y, radius;
  int32_t level, desc;
} kfw_query; /* == orbx_kf_query */

typedef struct {
  int n;
  const kfw_keypoint* keys;
  const uint8_t* desc;
  float min_x, min_y, grid_w_inv, grid_h_inv;
} kfw_frame; /* == orbx_kf_frame */

/* std::vector<size_t> mGrid[ix][iy] */
typedef struct {
  int* v;
  int size, cap;
} cell_list;

typedef struct {
  cell_list cell[GRID_COLS][GRID_ROWS];
  kfw_frame f;
  int* indices; /* vIndices, reserve(N) */
} kfw_grid;

/* (int) of a float as the reference's x86 object converts it (cvttss2si): out
 * of int's range or NaN gives INT_MIN; in C the cast alone would be undefined */
static int f2i(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT_MIN; }

static void push_back(cell_list* c, int i) {
  if (c->size == c->cap) {
    c->cap = c->cap ? 2 * c->cap : 4;
    c->v = (int*)realloc(c->v, (size_t)c->cap * sizeof(int));
  }
  c->v[c->size++] = i;
}

/* Frame::AssignFeaturesToGrid with PosInGrid */
kfw_grid* kfw_grid_create(const kfw_frame* f) {
  kfw_grid* g = (kfw_grid*)calloc(1, sizeof(kfw_grid));
  g->f = *f;
  g->indices = (int*)malloc((size_t)(f->n > 0 ? f->n : 1) * sizeof(int));
  for (int i = 0; i < f->n; i++) {
    const kfw_keypoint* kp = &f->keys[i];
    const int posX = f2i(roundf((kp->x - f->min_x) * f->grid_w_inv));
    const int posY = f2i(roundf((kp->y - f->min_y) * f->grid_h_inv));
    if (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) continue;
    push_back(&g->cell[posX][posY], i);
  }
  return g;
}

void kfw_grid_free(kfw_grid* g) {
  if (!g) return;
  for (int ix = 0; ix < GRID_COLS; ix++)
    for (int iy = 0; iy < GRID_ROWS; iy++) free(g->cell[ix][iy].v);
  free(g->indices);
  free(g);
}

static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

/* KeyFrame::GetFeaturesInArea: fills g->indices, returns its size; *visited =
 * the cell entries walked */
static int features_in_area(kfw_grid* g, float x, float y, float r, int* visited) {
  const kfw_frame* f = &g->f;
  int n = 0;
  *visited = 0;

  const int nMinCellX = imax(0, f2i(floorf((x - f->min_x - r) * f->grid_w_inv)));
  if (nMinCellX >= GRID_COLS) return n;

  const int nMaxCellX = imin(GRID_COLS - 1, f2i(ceilf((x - f->min_x + r) * f->grid_w_inv)));
  if (nMaxCellX < 0) return n;

  const int nMinCellY = imax(0, f2i(floorf((y - f->min_y - r) * f->grid_h_inv)));
  if (nMinCellY >= GRID_ROWS) return n;

  const int nMaxCellY = imin(GRID_ROWS - 1, f2i(ceilf((y - f->min_y + r) * f->grid_h_inv)));
  if (nMaxCellY < 0) return n;

  for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
    for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
      const cell_list* vCell = &g->cell[ix][iy];
      for (int j = 0, jend = vCell->size; j < jend; j++) {
        const kfw_keypoint* kpUn = &f->keys[vCell->v[j]];
        const float distx = kpUn->x - x;
        const float disty = kpUn->y - y;
        ++*visited;
        if (fabsf(distx) < r && fabsf(disty) < r) g->indices[n++] = vCell->v[j];
      }
    }
  }
  return n;
}

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:896-908) */
int kfw_descriptor_distance(const uint8_t* a, const uint8_t* b) {
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

/* nq queries in the gridded keyframe.  stats (may be NULL) holds 5 ints per
 * query: cell entries visited, indices.size() (boxed), candidates past the
 * gate, gated candidates at the final best distance (>= 2: a tied minimum),
 * and whether one of the tied losers has a lower index than the winner */
void kfw_search_grid(kfw_grid* g, const kfw_query* q, int nq, const uint8_t* qdesc, int32_t* best_idx,
                     int32_t* best_dist, int32_t* stats) {
  const kfw_frame* f = &g->f;
  for (int i = 0; i < nq; i++) {
    const int level = q[i].level;
    int visited;
    const int nind = features_in_area(g, q[i].x, q[i].y, q[i].radius, &visited);
    const uint8_t* dMP = qdesc + (size_t)q[i].desc * 32;
    int bestDist = INT_MAX;
    int bestIdx = -1;
    int gated = 0;
    for (int k = 0; k < nind; k++) {
      const int idx = g->indices[k];
      const kfw_keypoint* kp = &f->keys[idx];
      if (level >= 0 && (kp->octave < level - 1 || kp->octave > level)) continue;
      ++gated;
      const int dist = kfw_descriptor_distance(dMP, f->desc + (size_t)idx * 32);
      if (dist < bestDist) {
        bestDist = dist;
        bestIdx = idx;
      }
    }
    best_idx[i] = bestIdx;
    best_dist[i] = bestDist;
    if (stats) {
      int at_best = 0, lower = 0;
      for (int k = 0; k < nind && bestIdx >= 0; k++) {
        const int idx = g->indices[k];
        const kfw_keypoint* kp = &f->keys[idx];
        if (level >= 0 && (kp->octave < level - 1 || kp->octave > level)) continue;
        if (kfw_descriptor_distance(dMP, f->desc + (size_t)idx * 32) == bestDist) {
          ++at_best;
          if (idx < bestIdx) lower = 1;
        }
      }
      stats[5 * i + 0] = visited;
      stats[5 * i + 1] = nind;
      stats[5 * i + 2] = gated;
      stats[5 * i + 3] = at_best;
      stats[5 * i + 4] = lower;
    }
  }
}

/* the cell of feature i as (ix, iy, position in the cell), or ix = -1 */
void kfw_grid_cell_of(const kfw_grid* g, int i, int32_t* out) {
  out[0] = out[1] = out[2] = -1;
  for (int ix = 0; ix < GRID_COLS; ix++)
    for (int iy = 0; iy < GRID_ROWS; iy++)
      for (int j = 0; j < g->cell[ix][iy].size; j++)
        if (g->cell[ix][iy].v[j] == i) {
          out[0] = ix;
          out[1] = iy;
          out[2] = j;
          return;
        }
}

/* one problem, grid included */
void kfw_search(const kfw_frame* f, const kfw_query* q, int nq, const uint8_t* qdesc, int32_t* best_idx,
                int32_t* best_dist, int32_t* stats) {
  kfw_grid* g = kfw_grid_create(f);
  kfw_search_grid(g, q, nq, qdesc, best_idx, best_dist, stats);
  kfw_grid_free(g);
}

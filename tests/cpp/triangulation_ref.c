/* triangulation_ref.c -- sequential CPU restatement of the reference's
 * ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:368-467),
 * CheckDistEpipolarLine (:71-85), ComputeThreeMaxima (:469-502) and
 * DescriptorDistance (:896-908), written line by line against them for the
 * tests (tests/test_triangulation*.py build it with
 * gcc -O2 -mfma -ffp-contract=off -shared and load it with ctypes).
 *
 * It is literal on purpose: rotHist is 30 growing vectors of idx1, walked
 * after ComputeThreeMaxima as the reference walks them, so that the device's
 * "event counts + per-row bin mask" formulation is checked against the
 * reference's form and not against itself.
 *
 * Floating point: the reference object is built -O3 -march=native with
 * contraction on; CheckDistEpipolarLine is not inlined, and its object code
 * fuses one product of every two-product sum into the add.
 * That form is written here with explicit fmaf under -ffp-contract=off.
 * tri_check_epipolar_written() is the same function in source order without
 * any fusing: the tests use it to show that a decision depends on the form. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TH_LOW 50       /* ORBmatcher.cc:14 */
#define HISTO_LENGTH 30 /* ORBmatcher.cc:15 */

/* cv::KeyPoint / orbx_keypoint */
typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} tri_keypoint;

/* layout of orbx_tri_frame (include/orbx.h) */
typedef struct {
  int n;
  const tri_keypoint* keys;
  const uint8_t* desc;
  const uint8_t* has_mp;
  int nnodes;
  const uint32_t* node_id;
  const uint32_t* node_off;
  const uint32_t* feat;
  const float* level_sigma2;
  int nlevels;
} tri_frame;

#define F(r, c) F12[3 * (r) + (c)]

/* :71-85 as the reference's object computes it.  sigma2 =
 * pKF2->mvLevelSigma2[kp2.octave] */
int tri_check_epipolar(float x1, float y1, float x2, float y2, const float* F12, float sigma2) {
  const float a = fmaf(x1, F(0, 0), y1 * F(1, 0)) + F(2, 0);  /* :72 */
  const float b = fmaf(x1, F(0, 1), y1 * F(1, 1)) + F(2, 1);  /* :73 */
  const float c = fmaf(y1, F(1, 2), x1 * F(0, 2)) + F(2, 2);  /* :74: the rounded product is x1*F(0,2) */
  const float den = fmaf(a, a, b * b);                        /* :77 */
  if (den == 0) return 0;                                     /* :79-81; a NaN den goes on */
  const float num = fmaf(b, y2, a * x2) + c;                  /* :76 */
  const float dsqr = (num * num) / den;                       /* :83 */
  return (double)dsqr < 3.84 * (double)sigma2;                /* :84: a double compare */
}

/* :71-85 in source order, every operation rounded (no contraction) */
int tri_check_epipolar_written(float x1, float y1, float x2, float y2, const float* F12,
                               float sigma2) {
  const float a = x1 * F(0, 0) + y1 * F(1, 0) + F(2, 0);
  const float b = x1 * F(0, 1) + y1 * F(1, 1) + F(2, 1);
  const float c = x1 * F(0, 2) + y1 * F(1, 2) + F(2, 2);
  const float num = a * x2 + b * y2 + c;
  const float den = a * a + b * b;
  if (den == 0) return 0;
  const float dsqr = num * num / den;
  return (double)dsqr < 3.84 * (double)sigma2;
}

/* :896-908 (the bit-twiddling popcount of 8 x 32 bits) */
int tri_descriptor_distance(const uint8_t* a, const uint8_t* b) {
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

/* a std::vector<int> */
typedef struct {
  int* v;
  int size, cap;
} ivec;

static void ivec_push(ivec* a, int x) {
  if (a->size == a->cap) {
    a->cap = a->cap ? 2 * a->cap : 16;
    a->v = (int*)realloc(a->v, (size_t)a->cap * sizeof(int));
  }
  a->v[a->size++] = x;
}

/* :469-502 */
static void compute_three_maxima(const ivec* histo, const int L, int* ind1, int* ind2, int* ind3) {
  int topIndices[3] = {-1, -1, -1};
  int topValues[3] = {0, 0, 0};
  for (int i = 0; i < L; ++i) {
    const int value = histo[i].size;
    for (int j = 0; j < 3; ++j) { /* insertInTop */
      if (value > topValues[j]) {
        for (int k = 2; k > j; --k) {
          topValues[k] = topValues[k - 1];
          topIndices[k] = topIndices[k - 1];
        }
        topValues[j] = value;
        topIndices[j] = i;
        break;
      }
    }
  }
  *ind1 = topIndices[0];
  *ind2 = topIndices[1];
  *ind3 = topIndices[2];
  if (topValues[1] < 0.1f * topValues[0]) {
    *ind2 = -1;
    *ind3 = -1;
  } else if (topValues[2] < 0.1f * topValues[0]) {
    *ind3 = -1;
  }
}

/* ComputeThreeMaxima alone, on bin sizes (for its own test) */
void tri_three_maxima(const int* sizes, int L, int* ind) {
  ivec* h = (ivec*)calloc((size_t)L, sizeof(ivec));
  for (int i = 0; i < L; ++i) h[i].size = sizes[i];
  compute_three_maxima(h, L, &ind[0], &ind[1], &ind[2]);
  free(h);
}

/* std::map::lower_bound over the ascending node ids */
static int lower_bound_node(const uint32_t* id, int from, int n, uint32_t key) {
  while (from < n && id[from] < key) ++from;
  return from;
}

/* :368-467.  match12[kf1->n]: the index in kf2, -1, or -2 where the rotation
 * check reset a match (the reference writes -1 there; the C ABI tells the two
 * apart).  contracted = 0 takes tri_check_epipolar_written instead (what the
 * search would give without the object's fusing).  stats (may be NULL):
 *   [0] rows that accepted two or more candidates,
 *   [1] epipolar decisions that differ between the two forms,
 *   [2] epipolar evaluations, [3] of them accepted.
 * Returns nmatches. */
int tri_search(const tri_frame* pKF1, const tri_frame* pKF2, const float* F12, int bOnlyStereo,
               int mbCheckOrientation, int contracted, int32_t* vMatches12, int* stats) {
  int nmatches = 0;
  int st[4] = {0, 0, 0, 0};
  char* wasReset = (char*)calloc(pKF1->n > 0 ? (size_t)pKF1->n : 1, 1);
  for (int i = 0; i < pKF1->n; i++) vMatches12[i] = -1; /* :383 */

  ivec rotHist[HISTO_LENGTH]; /* :385-388 */
  memset(rotHist, 0, sizeof(rotHist));
  const float factor = 1.0f / HISTO_LENGTH; /* :389 */

  int f1it = 0, f2it = 0; /* :391-394 */
  const int f1end = pKF1->nnodes, f2end = pKF2->nnodes;

  while (f1it != f1end && f2it != f2end) { /* :396 */
    if (pKF1->node_id[f1it] == pKF2->node_id[f2it]) {
      for (uint32_t i1 = pKF1->node_off[f1it]; i1 < pKF1->node_off[f1it + 1]; i1++) { /* :398 */
        const uint32_t idx1 = pKF1->feat[i1];
        /* :399-400: a pointer test; mvuRight only matters with bOnlyStereo,
         * where nothing is accepted anyway (:417) */
        if (pKF1->has_mp && pKF1->has_mp[idx1]) continue;
        const tri_keypoint* kp1 = &pKF1->keys[idx1];
        const uint8_t* d1 = pKF1->desc + (size_t)idx1 * 32;
        int bestDist = TH_LOW; /* :405 */
        int bestIdx2 = -1;
        int accepted = 0;
        for (uint32_t i2 = pKF2->node_off[f2it]; i2 < pKF2->node_off[f2it + 1]; i2++) { /* :408 */
          const uint32_t idx2 = pKF2->feat[i2];
          if (pKF2->has_mp && pKF2->has_mp[idx2]) continue; /* :409; vbMatched2 is never set */
          const uint8_t* d2 = pKF2->desc + (size_t)idx2 * 32;
          const int dist = tri_descriptor_distance(d1, d2); /* :412 */
          if (dist > TH_LOW || dist > bestDist) continue;   /* :414 */
          const tri_keypoint* kp2 = &pKF2->keys[idx2];
          if (bOnlyStereo) continue; /* :417 `!bOnlyStereo &&` */
          const float s2 = pKF2->level_sigma2[kp2->octave];
          const int ok = tri_check_epipolar(kp1->x, kp1->y, kp2->x, kp2->y, F12, s2);
          const int okw = tri_check_epipolar_written(kp1->x, kp1->y, kp2->x, kp2->y, F12, s2);
          st[2]++;
          st[1] += ok != okw;
          if (contracted ? ok : okw) {
            st[3]++;
            bestIdx2 = (int)idx2; /* :418-419 */
            bestDist = dist;
            accepted++;
            if (mbCheckOrientation) { /* :420-426 */
              float rot = kp1->angle - kp2->angle;
              if (rot < 0.0) rot += 360.0f;
              const int bin = (int)roundf(rot * factor) % HISTO_LENGTH;
              /* outside [0, 30) the reference indexes rotHist out of range;
               * angles in [0, 360) never get there */
              if (bin >= 0 && bin < HISTO_LENGTH) ivec_push(&rotHist[bin], (int)idx1);
            }
          }
        }
        st[0] += accepted >= 2;
        if (bestIdx2 >= 0) { /* :430-433 */
          vMatches12[idx1] = bestIdx2;
          nmatches++;
        }
      }
      ++f1it; /* :435-436 */
      ++f2it;
    } else if (pKF1->node_id[f1it] < pKF2->node_id[f2it]) { /* :437-438 */
      f1it = lower_bound_node(pKF1->node_id, f1it, f1end, pKF2->node_id[f2it]);
    } else { /* :440 */
      f2it = lower_bound_node(pKF2->node_id, f2it, f2end, pKF1->node_id[f1it]);
    }
  }

  if (mbCheckOrientation) { /* :444-458 */
    int ind1 = -1, ind2 = -1, ind3 = -1;
    compute_three_maxima(rotHist, HISTO_LENGTH, &ind1, &ind2, &ind3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
      if (i != ind1 && i != ind2 && i != ind3) {
        for (int j = 0; j < rotHist[i].size; j++) {
          const int idx = rotHist[i].v[j];
          if (vMatches12[idx] >= 0) {
            vMatches12[idx] = -1;
            wasReset[idx] = 1;
            nmatches--;
          }
        }
      }
    }
  }
  for (int i = 0; i < pKF1->n; i++)
    if (wasReset[i]) vMatches12[i] = -2;
  for (int i = 0; i < HISTO_LENGTH; i++) free(rotHist[i].v);
  free(wasReset);
  if (stats) memcpy(stats, st, sizeof(st));
  return nmatches;
}

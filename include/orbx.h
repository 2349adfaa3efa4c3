/* orbx.h -- C ABI of the MI355X-native ORB front end (liborbx.so).
 *
 * Drop-in boundary for the reference's hot path:
 *   ORB_SLAM2::ORBextractor   /root/reference/include/ORBextractor.h:25-91
 *   ORB_SLAM2::ORBmatcher     /root/reference/include/ORBmatcher.h:16-81
 *   ORBVocabulary::score and ORB_SLAM2::KeyFrameDatabase's word walk
 *                             include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc
 *                             (orbv_score, orbv_db_*: place recognition)
 * Plain C: POD structs, raw pointers, explicit sizes, int status codes, no
 * exceptions across the boundary, no torch types.  Every compute entry point
 * runs hand-written HIP kernels on a gfx950 device; there is no CPU path.
 *
 * Threading: an orbx_extractor / orbx_plan owns its own HIP stream and
 * scratch and may be used from one thread at a time; distinct instances may
 * run concurrently (the reference runs left/right extractors on two threads,
 * /root/reference/src/Frame.cc:58-61).  Matcher calls are re-entrant.
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): plan option flags 2 and 4 retired (ORBX_ERR_ARG), flags 8 / 16,
 * orbx_proj_problem and the orbm_proj_plan_* / orbm_search_by_bow_kf_frame
 * entry points added (round 5).  orbx_tri_frame and
 * orbm_search_for_triangulation, and orbx_kf_frame / orbx_kf_query and
 * orbm_keyframe_search, and orbx_init_pair and
 * orbm_search_for_initialization, and the debug entry points
 * orbx_debug_live_resources / orbx_debug_fail_acquire, and orbv_score and the
 * orbv_db_* keyframe database with its batched queries
 * (orbv_db_query_batch / orbv_db_query_batch_device), and the device-side projection
 * (orbx_proj_camera / orbx_proj_points / orbx_proj_params / orbx_proj_build_problem,
 * orbm_predict_scale_thresholds, orbm_project_points, orbm_proj_plan_project / _track), and
 * the keyframe form of it (orbx_kf_camera / orbx_kf_points / orbx_kf_problem,
 * orbm_keyframe_project and the orbm_kf_plan_* entry points), are
 * additive (no existing struct or entry point changes), so the version stays 2. */
#define ORBX_ABI_VERSION 2

/* status codes */
enum {
  ORBX_OK = 0,
  ORBX_ERR_ARG = -1,         /* bad argument / image type                               */
  ORBX_ERR_CELL_ROI = -2,    /* strict cell guard: a FAST cell has negative extent; the
                                reference throws cv::Exception from cv::Mat(m, Rect) at
                                src/ORBextractor.cc:328 (1920x1080)      */
  ORBX_ERR_LEVEL_SIZE = -3,  /* a pyramid level has <= 32 rows (reference divides by 0 at
                                src/ORBextractor.cc:230) or < 32 cols                     */
  ORBX_ERR_QUADTREE = -4,    /* DistributeOctTree would never terminate */
  ORBX_ERR_CAPACITY = -5,    /* caller buffer too small (*n holds the required count)     */
  ORBX_ERR_UNSUPPORTED = -6, /* a configuration beyond the kernels' static limits: a level
                                ratio > ~2.3 other than exactly 2, or a level-0 size
                                outside the FAST key packing -- supported are
                                (w-32 <= 4095 and h-32 <= 4095), (w-32 <= 8191 and
                                h-32 <= 2047) or (w-32 <= 2047 and h-32 <= 8191), so
                                e.g. 4200x2100 is refused; ...                        */
  ORBX_ERR_HIP = -7,         /* HIP runtime error                                         */
  ORBX_ERR_NO_DEVICE = -8,   /* no gfx950 device / bad device ordinal                     */
};

/* ORBextractor constructor arguments (ORBextractor.h:31-32) + switches. */
typedef struct {
  int nfeatures;
  float scale_factor;
  int nlevels;
  int ini_th_fast;
  int min_th_fast;
  int cell_guard; /* 0 = strict (reference: throw on negative-extent FAST cells),
                     1 = empty (such cells yield no corners; == upstream ORB-SLAM2 guards) */
} orbx_params;

/* Layout-identical to cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle,
 * response, octave, class_id. */
typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} orbx_keypoint;

int orbx_abi_version(void);
const char* orbx_status_string(int status);
/* number of visible gfx950 devices (0 on a host without GPU) */
int orbx_device_count(void);

/* ---------------------------------------------------------------------------
 * Level geometry and constant tables (host-only, no device needed).
 * Mirrors ORBextractor::ORBextractor (src/ORBextractor.cc:116-170),
 * GetScaleFactors() & co. (ORBextractor.h:43-63) and ComputePyramid sizes
 * (src/ORBextractor.cc:501-502).
 * ------------------------------------------------------------------------- */
int orbx_tables(const orbx_params* p, float* scale, float* inv_scale, float* sigma2,
                float* inv_sigma2, int* features_per_level, int* umax16);

typedef struct {
  int nlevels;
  int width[32], height[32];
  int alias[32];          /* level whose pixels this level shares (level 1 == level 0:
                             mvScaleFactor[1] == 1)                    */
  int ncols[32], nrows[32], wcell[32], hcell[32]; /* FAST cell grid (:308-314)        */
  int ncells_bad[32];     /* cells with negative extent (strict guard -> error)       */
  int features[32];       /* mnFeaturesPerLevel                                        */
  int nini[32];           /* DistributeOctTree initial nodes (:230)                    */
  int kcap_level[32];     /* max keypoints a level can emit                            */
  int kcap;               /* max keypoints per frame (sum of kcap_level)               */
  long long pixels;       /* sum of level pixel counts                                 */
  long long bytes_pyr_fast; /* algorithmic bytes of pyramid + FAST per frame */
} orbx_geometry;

int orbx_geometry_compute(const orbx_params* p, int width, int height, orbx_geometry* g);

/* Resize coefficient tables for level l (l >= 1, non-alias): xofs[w_l],
 * alpha[2*w_l], yofs[h_l], beta[2*h_l] (INTER_RESIZE_COEF_BITS = 11). */
int orbx_resize_tables(const orbx_params* p, int width, int height, int level, int32_t* xofs,
                       int16_t* alpha, int32_t* yofs, int16_t* beta);

/* ---------------------------------------------------------------------------
 * ORBextractor drop-in: host image in, host keypoints/descriptors out.
 * Replaces ORBextractor::operator() (src/ORBextractor.cc:442-495).
 * ------------------------------------------------------------------------- */
typedef struct orbx_extractor orbx_extractor;

int orbx_extractor_create(const orbx_params* p, int device, orbx_extractor** out);
int orbx_extractor_destroy(orbx_extractor* e);

/* Capacity needed for a w x h image (upper bound of the keypoint count). */
int orbx_extractor_capacity(orbx_extractor* e, int width, int height, int* kcap);

/* operator()(image, mask, keypoints, descriptors): img is CV_8UC1 rows of
 * `stride` bytes.  On success *n = K; kps[0..K) and desc[0..K*32) hold the
 * level-major keypoints (level coordinates * mvScaleFactor) and descriptors.
 * K == 0 leaves kps/desc untouched (reference :460-463).  cap < K returns
 * ORBX_ERR_CAPACITY with *n = K.  Synchronous. */
int orbx_extract(orbx_extractor* e, const uint8_t* img, int width, int height, size_t stride,
                 orbx_keypoint* kps, int cap, uint8_t* desc, int* n);

/* mvImagePyramid[level] of the last orbx_extract (copied D2H on demand). */
int orbx_extractor_level(orbx_extractor* e, int level, uint8_t* dst, size_t dst_stride,
                         int* width, int* height);

/* Options of an extractor (default 0; persistent across calls):
 * ORBX_EXTRACTOR_PYRAMID_TO_HOST  every orbx_extract also brings the whole
 *     pyramid back (the reference refills mvImagePyramid on each call,
 *     src/ORBextractor.cc:497-515, read by Frame::ComputeStereoMatches): one
 *     D2H of the level buffer on a second stream, overlapped with the rest
 *     of the extraction; read it with orbx_extractor_level_host;
 * ORBX_EXTRACTOR_PINNED_H2D  upload the caller's image through the
 *     extractor's pinned staging buffer (host copy in row chunks overlapped
 *     with the DMA) instead of straight from its pageable rows (measurement
 *     option: slower at 1080p). */
#define ORBX_EXTRACTOR_PYRAMID_TO_HOST 1
#define ORBX_EXTRACTOR_PINNED_H2D 2
int orbx_extractor_set_options(orbx_extractor* e, int flags);

/* Host view of mvImagePyramid[level] after an orbx_extract with
 * ORBX_EXTRACTOR_PYRAMID_TO_HOST: *data / *stride point into extractor-owned
 * pinned memory, valid until the next orbx_extract or destroy of `e` (levels
 * whose size equals the previous level's -- level 1 with the reference's
 * scale table -- share its pixels, as cv::resize copies them). */
int orbx_extractor_level_host(orbx_extractor* e, int level, const uint8_t** data, size_t* stride,
                              int* width, int* height);

/* Call statistics of an extractor since creation: calls of orbx_extract and
 * the calls that needed a second D2H round trip for their results (always 0
 * since round 6: one kernel writes exactly the frame's rows into the pinned
 * staging; kept for ABI compatibility). */
int orbx_extractor_stats(orbx_extractor* e, long long* calls, long long* refetches);

/* ---------------------------------------------------------------------------
 * Batched device-resident extraction (the throughput path; bench.py).
 * ------------------------------------------------------------------------- */
typedef struct orbx_plan orbx_plan;

int orbx_plan_create(const orbx_params* p, int width, int height, int max_batch, int device,
                     orbx_plan** out);
int orbx_plan_destroy(orbx_plan* plan);
int orbx_plan_geometry(const orbx_plan* plan, orbx_geometry* g);

/* d_frames: nframes images, frame i at d_frames + i*frame_stride, rows of
 * row_stride bytes (device memory; any byte alignment -- 16-B aligned rows
 * take the fastest staging path; no byte outside a frame's row_stride x
 * height bytes is read; row_stride < 2^24, else ORBX_ERR_UNSUPPORTED: the
 * kernels form row offsets with 24-bit multiplies).  Outputs (device memory):
 *   d_kps  [nframes][kcap], d_desc [nframes][kcap][32], d_counts [nframes].
 * Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 * Device-side failures (quadtree stuck) are latched; read them with
 * orbx_plan_check(). */
int orbx_plan_extract(orbx_plan* plan, const uint8_t* d_frames, int nframes, size_t frame_stride,
                      size_t row_stride, orbx_keypoint* d_kps, uint8_t* d_desc, int* d_counts,
                      void* stream);
/* synchronises `stream`, returns and clears the latched device error */
int orbx_plan_check(orbx_plan* plan, void* stream);
/* Debug counters since the last call (then reset; synchronises the plan's
 * stream): FAST strips whose corner list overflowed into the strength-map
 * scan (see orbx_debug_set_fast_ccap). */
int orbx_plan_debug_counters(orbx_plan* plan, int* fast_overflow_strips);
/* A second debug counter, read and reset the same way: FAST strips that took
 * the dense post-pass (row masks, all four waves) since the last call.  With
 * automatic options those are the strips with more than 64 corners (or more
 * than the corner list holds); strips with 1..64 corners are finished by one
 * wave in registers and empty strips only clear their cells' counts, and
 * neither is counted.  With ORBX_PLAN_FAST_DENSE it counts every strip. */
int orbx_plan_fast_dense_strips(orbx_plan* plan, int* fast_dense_strips);
/* Testing only: plans created after this call give the FAST kernels a
 * corner list of `ccap` entries (<= 1024) in one launch group, so the
 * strength-map overflow path runs on ordinary frames; ccap < 0 restores the
 * planner's own length.  Process-global; results are unchanged either way. */
int orbx_debug_set_fast_ccap(int ccap);
/* Debugging: the device buffers, pinned host buffers, streams and events
 * (counts[0..3]) that the handles of this library hold at the moment, over
 * the whole process.  A handle that was destroyed has given all of its own
 * back.  The per-call workspaces of the synchronous entry points are pooled
 * for the life of the process and are not counted. */
int orbx_debug_live_resources(int counts[4]);
/* Testing only: from now on the `nth` acquisition of such a resource on the
 * calling thread fails (the entry point returns ORBX_ERR_HIP) without a call
 * into the HIP runtime; the ones before and after it proceed.  nth <= 0
 * disarms. */
int orbx_debug_fail_acquire(int nth);

/* Kernel-path options of a plan (default 0 = automatic; persistent).  Every
 * path gives bit-identical results; they differ in speed only.
 *   ORBX_PLAN_PYR_TILES    the pyramid by k_pyramid (2-D tiles of the level
 *                          chain, halo recompute) -- the one pyramid path;
 *   ORBX_PLAN_BRIEF_PATCH  descriptors blur each keypoint's 43 x 48 patch
 *                          (k_orient_brief);
 *   ORBX_PLAN_BRIEF_LEVEL  every unique level is blurred once (k_blur) and
 *                          the descriptors sample it (k_orient_brief_lb);
 *   ORBX_PLAN_FAST_DENSE   every FAST strip takes the dense post-pass, as
 *                          before the per-strip choice (DESIGN.md §4 round 7;
 *                          for A/B timing and tests);
 *   ORBX_PLAN_NO_TWINS     a keypoint that wins the quadtree both in a level
 *                          and in a level aliasing it (level 1 of the
 *                          reference's scale table is level 0's image) is
 *                          computed once per level, as before DESIGN.md §4
 *                          round 10; by default it is computed once and
 *                          written to both rows (for A/B timing and tests).
 * Automatic (0): the tile pyramid, and the level blur when nfeatures x 43 x
 * 48 exceeds ORBX_LB_RATIO x the unique level pixels.
 * The round-4 row-streaming pyramid and fused pyramid + FAST kernels (flags
 * 2 and 4) measured 1.1x / 2.6x the tile path's time and were retired; their
 * flags, like any other unknown bit or both BRIEF flags at once, return
 * ORBX_ERR_ARG (options unchanged). */
#define ORBX_PLAN_PYR_TILES 1
#define ORBX_PLAN_BRIEF_PATCH 8
#define ORBX_PLAN_BRIEF_LEVEL 16
#define ORBX_PLAN_FAST_DENSE 64
#define ORBX_PLAN_NO_TWINS 128
int orbx_plan_set_options(orbx_plan* plan, int flags);

/* mvImagePyramid[level] of frame `frame` of the last orbx_plan_extract on
 * this plan, copied to host rows of dst_stride bytes (synchronises `stream`,
 * which must be the stream of that extraction or ordered after it; NULL =
 * the default stream).  Level 0 (and levels aliasing it) are the caller's
 * frame and are not held by the plan: ORBX_ERR_ARG.  With dst != NULL,
 * `frame` must be below the frame count of the plan's last orbx_plan_extract
 * (ORBX_ERR_ARG before any extraction); dst == NULL only reports the size. */
int orbx_plan_level(orbx_plan* plan, int frame, int level, uint8_t* dst, size_t dst_stride,
                    int* width, int* height, void* stream);

/* Per-stage device timing (HIP events around every launch of a stage). */
int orbx_stage_count(void);
const char* orbx_stage_name(int stage);
int orbx_plan_set_timing(orbx_plan* plan, int enable); /* also resets the accumulators   */
/* after the stream is synchronised: total ms and launch count per stage */
int orbx_plan_stage_times(orbx_plan* plan, double* ms, int* launches, int nstages);

/* Device synthetic frames (same bytes as orbx/synth.py): kind 0 rects, 3 pan,
 * 1 noise, 2 flat; frame i gets seed 0x5EED0000 + first_idx + i. */
int orbx_synth_frames(uint8_t* d_frames, int width, int height, size_t frame_stride, int nframes,
                      int first_idx, int kind, void* stream);

/* Self-test of the rotated-BRIEF sin/cos (device memory): sc[2i], sc[2i+1] =
 * the (sin, cos) k_orient_brief uses for angle x[i] -- glibc sincosf
 * (ORBextractor.cc:58-59) wherever it moves a BRIEF sample (orbx_sincos.h). */
int orbx_selftest_sincos(const float* d_x, int n, float* d_sc, void* stream);
/* Same (sin, cos) for the n consecutive float bit patterns first_bits ..
 * first_bits + n - 1, lane-parallel, into host memory sc[2n] (synchronous):
 * the exhaustive device check of every reachable BRIEF angle. */
int orbx_selftest_sincos_range(uint32_t first_bits, int n, float* sc, int device);

/* ---------------------------------------------------------------------------
 * ORBmatcher drop-in.
 * ------------------------------------------------------------------------- */
/* One KeyFrame's matcher inputs.  DBoW2::FeatureVector
 * (Thirdparty/DBoW2/DBoW2/FeatureVector.h:21-22) flattened: node_id[nnodes]
 * ascending & unique, node j holds feat[node_off[j] .. node_off[j+1]).
 * valid[i] != 0 <=> GetMapPointMatches()[i] && !isBad() (NULL = all valid).
 * angle[i] = mvKeysUn[i].angle. */
typedef struct {
  int n;
  const uint8_t* desc; /* n x 32 */
  const float* angle;  /* n */
  const uint8_t* valid;
  int nnodes;
  const uint32_t* node_id;
  const uint32_t* node_off; /* nnodes + 1 */
  const uint32_t* feat;
} orbx_bow_frame;

/* ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)
 * (src/ORBmatcher.cc:278-366).  Host inputs; match12[n1] = matched index in
 * kf2 (vpMatches12[i] = vpMapPoints2[match12[i]]), -1 where the reference
 * never writes vpMatches12[i] (it only resize()s the caller's vector, :289),
 * or -2 where it matched and the rotation check reset it to nullptr (:359).
 * Synchronous. */
int orbm_search_by_bow(const orbx_bow_frame* kf1, const orbx_bow_frame* kf2, float nnratio,
                       int check_ori, int device, int32_t* match12, int* nmatches);

/* SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) in upstream ORB-SLAM2's
 * form (SURVEY.md §5 switch bow_kf_frame=full; this reference ships only the
 * stub of src/ORBmatcher.cc:88-119, which the compat header keeps as the
 * default).  kf: the KeyFrame (valid[i] = its MapPoint i is non-null and not
 * bad, angles of mvKeysUn); frame: the Frame (mvKeys angles; its valid is
 * ignored: every Frame feature is a candidate).  Per KF row in node order:
 * best / second over the node's unclaimed Frame features, accepted when
 * best <= TH_LOW (50) and best < nnratio * second; the rotation check as the
 * KF-KF form.  match_f[frame->n] = the KF feature whose MapPoint the Frame
 * feature received (vpMapPointMatches[i] = vpMapPointsKF[match_f[i]]), -1 for
 * none (vpMapPointMatches starts as F.N nulls).  Synchronous.
 * ORBX_ERR_UNSUPPORTED for nnratio <= 50/256 (no second-best could pass). */
int orbm_search_by_bow_kf_frame(const orbx_bow_frame* kf, const orbx_bow_frame* frame, float nnratio,
                                int check_ori, int device, int32_t* match_f, int* nmatches);

/* One KeyFrame's inputs to SearchForTriangulation: keys = mvKeysUn (pt, angle
 * and octave are read), desc = mDescriptors, has_mp[i] != 0 <=>
 * GetMapPoint(i) != NULL (a pointer test only, no isBad(); NULL = no feature
 * has one), the FeatureVector flattened as in orbx_bow_frame, and
 * level_sigma2[nlevels] = mvLevelSigma2. */
typedef struct {
  int n;
  const orbx_keypoint* keys; /* n */
  const uint8_t* desc;       /* n x 32 */
  const uint8_t* has_mp;     /* n, or NULL */
  int nnodes;
  const uint32_t* node_id;  /* ascending, unique */
  const uint32_t* node_off; /* nnodes + 1 */
  const uint32_t* feat;
  const float* level_sigma2; /* nlevels */
  int nlevels;
} orbx_tri_frame;

/* ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:368-467 with
 * CheckDistEpipolarLine, :71-85) of kf1 against nkf2 neighbour keyframes in
 * one batch: problem p searches kf1's rows over kf2[p] under F12 + 9 * p (3x3
 * row-major, CV_32F).  nkf2 = 1 is the reference's call; nkf2 > 1 is the
 * neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:
 * 177-191) as one upload, one set of launches and one download.  Per row of a
 * common vocabulary node (a KF1 feature without a MapPoint): over the node's
 * KF2 features without a MapPoint, in list order, a candidate with Hamming
 * distance <= the best so far (50 at first; ties accepted, so the later
 * candidate wins) that passes the epipolar test becomes the best; with
 * check_ori (mbCheckOrientation) every such acceptance enters the rotation
 * histogram, and a row with any acceptance outside the three kept bins is
 * reset.  match12[p * kf1->n + i] = the index in kf2[p], -1 for none, or -2
 * where the rotation check reset a match (as orbm_search_by_bow);
 * nmatches[p] = the entries >= 0 (vMatchedPairs = those rows in ascending i).
 * only_stereo != 0 (bOnlyStereo) gives no match at all: in this reference the
 * `!bOnlyStereo &&` of :417 rejects every candidate (mvuRight and the epipole
 * of :373-379 are therefore not inputs).  Only kf2[p]'s level_sigma2 is read
 * (kf1's may be NULL).  Host pointers; synchronous.
 * ORBX_ERR_ARG where the reference would index out of range or count a row
 * twice: a feat index >= n, a kf2 octave outside [0, nlevels), a kf1 feature
 * listed twice in feat, node_id not ascending, nkf2 < 0.  nkf2 == 0, n == 0
 * and no common node are valid (no matches). */
int orbm_search_for_triangulation(const orbx_tri_frame* kf1, int nkf2, const orbx_tri_frame* kf2,
                                  const float* F12, int only_stereo, int check_ori, int device,
                                  int32_t* match12, int* nmatches);

/* One query of the keyframe window search below: the arguments of
 * KeyFrame::GetFeaturesInArea and the octave gate of the loop after it. */
typedef struct {
  float x, y;      /* the u, v handed to KeyFrame::GetFeaturesInArea            */
  float radius;    /* th * mvScaleFactors[level], already multiplied            */
  int32_t level;   /* PredictScale(): candidates need level-1 <= octave <= level;
                      < 0 = no octave gate                                      */
  int32_t desc;    /* row of the call's descriptor pool                         */
} orbx_kf_query;

typedef struct {
  int n;
  const orbx_keypoint* keys;   /* mvKeysUn (pt and octave are read) */
  const uint8_t* desc;         /* mDescriptors, n x 32              */
  float min_x, min_y, grid_w_inv, grid_h_inv;  /* mnMinX, mnMinY, mfGridElement{Width,Height}Inv */
} orbx_kf_frame;

/* The search that ORBmatcher::Fuse(KF, vpMapPoints, th), Fuse(KF, Scw, ..)
 * and SearchBySim3 share (src/ORBmatcher.cc:532-551, :600-619, :696-714),
 * batched: problem p searches queries q[qoff[p] .. qoff[p+1]) in kf[p]; a
 * query's descriptor is qdesc + 32 * q.desc, a pool of npool rows shared by
 * every problem (in LocalMapping::SearchInNeighbors, src/LocalMapping.cc:
 * 235-293, one map point's descriptor goes up once however many keyframes it
 * is projected into).  One upload, one set of launches, one download.
 * Per query j: KeyFrame::GetFeaturesInArea(x, y, radius) (src/KeyFrame.cc:
 * 549-588: the 64 x 48 grid filled by PosInGrid's round() in index order, a
 * feature outside the grid in no cell, the floor / ceil cell bounds with their
 * clamps and early returns, cells visited ix then iy then the cell's list,
 * the strict box test fabs(dx) < r && fabs(dy) < r), then over its result the
 * gate level - 1 <= octave <= level and the first strict minimum of
 * DescriptorDistance.  best_idx[j] = that feature's index or -1, best_dist[j]
 * = its distance or INT_MAX (also where features were found but none passed
 * the gate).  Ties go to the candidate visited first, which need not be the
 * lowest index.  No threshold is applied (TH_LOW for Fuse, TH_HIGH for
 * SearchBySim3 are the caller's), nothing is claimed: queries do not interact
 * and several may return the same feature.  A float outside int's range
 * converts to INT_MIN, as in the reference's x86 object.
 * Host pointers; synchronous.  ORBX_ERR_ARG for nprob < 0, a qoff that does
 * not start at 0 or decreases, a desc outside [0, npool), a non-finite x, y
 * or radius (the reference would convert a NaN to int); ORBX_ERR_UNSUPPORTED
 * for n > 8192.  nprob == 0, n == 0 and a problem without queries are valid. */
int orbm_keyframe_search(int nprob, const orbx_kf_frame* kf, const orbx_kf_query* q,
                         const int32_t* qoff /* nprob + 1 */, const uint8_t* qdesc, int npool,
                         int device, int32_t* best_idx, int32_t* best_dist);

/* One ORBmatcher::SearchForInitialization call (src/ORBmatcher.cc:197-276):
 * F1 = the initial frame, F2 = the current one. */
typedef struct {
  orbx_kf_frame f1, f2;   /* mvKeysUn (pt, octave, angle), mDescriptors; grid constants of f2 only */
  float* prev_matched;    /* in/out, 2 * f1.n: vbPrevMatched (x, y)                                */
  int32_t* match12;       /* in/out, f1.n: vnMatches12 as the previous call left it                 */
} orbx_init_pair;

/* ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:197-276), the
 * monocular bootstrap of Tracking::MonocularInitialization, batched: npair
 * independent pairs (streams bootstrapping at once) in one upload, one set of
 * launches and one download; npair = 1 is the member function.
 * Per pair, for i1 ascending: a row with f1 octave > 0 is skipped; a row with
 * a negative octave is not, and searches every octave of f2.  Candidates are
 * Frame::GetFeaturesInArea(prev_matched[i1], (float)window_size, octave,
 * octave) on f2 (src/Frame.cc:307-358: the 64 x 48 grid filled by PosInGrid's
 * round() in index order, the floor / ceil cell bounds with their clamps and
 * early returns, cells visited ix then iy then the cell's list, the level
 * gate, the strict box test).  Over them in visiting order only candidates
 * closer than their feature's current holder (dist < vMatchedDistance[i2])
 * take part: best = the first strict minimum, second best = the second
 * smallest distance as a multiset (it may equal best).  Accepted when best <=
 * TH_LOW (50) and best < (float)second * nnratio; an accepted row takes the
 * feature away from its holder (the holder's match12 becomes -1).  With
 * check_ori the accepted rows, displaced ones included, vote in the 30-bin
 * rotation histogram (bin = round(rot / 30), 30 wraps to 0) and rows outside
 * the three fullest bins that still hold a match are reset to -1 (not the -2
 * of orbm_search_by_bow: match12 feeds the next call).
 * match12 is not cleared (the reference's resize(n, -1) keeps the caller's
 * entries): a row not accepted by this call keeps its value, nmatches[p]
 * counts this call's matches only, and prev_matched[i1] = f2.keys[match12[i1]]
 * .pt for every row >= 0, the kept ones included.
 * Host pointers; synchronous; safe from several threads.  ORBX_ERR_ARG for
 * npair < 0, a null pointer where a count is positive, a non-finite coordinate
 * in prev_matched or f2.keys, with check_ori a key angle outside [0, 360] or
 * non-finite (the bin would leave the histogram), and a row that ends the call
 * holding an entry >= f2.n (the reference reads out of range there; found on
 * the device, reported after the download).  ORBX_ERR_UNSUPPORTED for f1.n or
 * f2.n > 8192.  On any error no output is written.  npair == 0, n == 0 and a
 * pair without level-0 rows are valid. */
int orbm_search_for_initialization(int npair, const orbx_init_pair* pairs, int window_size,
                                   float nnratio, int check_ori, int device, int* nmatches /* npair */);
/* the same call; nrescan (npair, may be NULL) receives per pair the number of
 * rows whose step of the ordered walk had to scan its window a second time
 * (DESIGN.md §15): a diagnostic for tools and tests. */
int orbm_search_for_initialization_stats(int npair, const orbx_init_pair* pairs, int window_size,
                                         float nnratio, int check_ori, int device, int* nmatches,
                                         int* nrescan);

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:896-908), batched on the
 * device: dist[i] = Hamming(a + 32*ia[i], b + 32*ib[i]); host pointers. */
int orbm_descriptor_distance_batch(const uint8_t* a, int na, const uint8_t* b, int nb,
                                   const int32_t* ia, const int32_t* ib, int npairs, int device,
                                   int32_t* dist);

/* Batched device matcher over extractor outputs (bench "extract+match",
 * BASELINE config 4): pair p matches frame A_p against frame B_p, each
 * reduced to its top `topn` keypoints by (response desc, index asc) and
 * placed in ONE vocabulary node in ascending index order (brute force).
 * match12 rows are indexed by keypoint index of frame A (cap kcap), value =
 * keypoint index in frame B, -1 for no match, or -2 where a match was found
 * and the rotation check (check_ori) reset it (as orbm_search_by_bow; test
 * `< 0` for "no match").  Frame p of side A is d_kps_a + p*kcap,
 * d_desc_a + p*kcap*32, d_count_a[p] (side B likewise), i.e. the layout of
 * orbx_plan_extract outputs; d_match12 is [npairs][kcap], d_nmatches
 * [npairs].  Asynchronous on `stream`.  Descriptors are arbitrary 32-byte
 * rows unless the caller opts in to ORBM_PLAN_ZERO_TAIL. */
typedef struct orbm_plan orbm_plan;
int orbm_plan_create(int max_pairs, int kcap, int topn, int device, orbm_plan** out);
int orbm_plan_destroy(orbm_plan* mp);
int orbm_plan_match_frames(orbm_plan* mp, int npairs, const orbx_keypoint* d_kps_a,
                           const uint8_t* d_desc_a, const int* d_count_a,
                           const orbx_keypoint* d_kps_b, const uint8_t* d_desc_b,
                           const int* d_count_b, float nnratio, int check_ori,
                           int32_t* d_match12, int* d_nmatches, void* stream);
int orbm_plan_set_timing(orbm_plan* mp, int enable);
int orbm_plan_stage_times(orbm_plan* mp, double* ms, int* launches, int nstages);
/* Options of orbm_plan_match_frames (default 0):
 * ORBM_PLAN_ZERO_TAIL  the caller guarantees bytes 24..31 of every descriptor
 *                      are zero -- true of orbx_plan_extract outputs (the
 *                      reference's 728-entry BRIEF pattern leaves them 0) --
 *                      so the distance kernels skip those two dwords;
 * ORBM_PLAN_VALU       distances by xor/popcount on the VALU instead of the
 *                      i8 MFMA formulation (same results; for testing);
 * ORBM_PLAN_NO_FOLD    every selected keypoint gets a distance row and column
 *                      of its own.  By default selected keypoints of a frame
 *                      with byte-identical descriptors (a keypoint kept in
 *                      level 0 and in its alias level 1) are computed once, in
 *                      pairs, and both get the result: the same matches, about
 *                      half the distance work on extractor outputs.  Lists
 *                      beyond 8192 keypoints (16384 with ORBM_PLAN_ZERO_TAIL)
 *                      and ORBM_PLAN_VALU run unfolded.
 * If side B is side A one frame back (d_kps_b + kcap == d_kps_a,
 * d_desc_b + kcap*32 == d_desc_a, d_count_b + 1 == d_count_a: a frame against
 * its predecessor out of one buffer of npairs + 1 frames), every frame is
 * selected once; the result is the same. */
#define ORBM_PLAN_ZERO_TAIL 1
#define ORBM_PLAN_VALU 2
#define ORBM_PLAN_NO_FOLD 4
int orbm_plan_set_options(orbm_plan* mp, int flags);
/* Folding counters of the plan's last orbm_plan_match_frames call, summed over
 * its pairs (waits for the device): out[0] selected keypoints of the
 * A sides, out[1] those among them computed as another's copy (followers),
 * out[2] / out[3] the same for the B sides.  0 followers when unfolded. */
int orbm_plan_fold_stats(orbm_plan* mp, int64_t out[4]);

/* ---------------------------------------------------------------------------
 * Stereo matcher: Frame::ComputeStereoMatches (src/Frame.cc:446-620), the
 * consumer of the extractors' mvImagePyramid.
 * ------------------------------------------------------------------------- */
/* Drop-in on host keypoints: kps_l/desc_l (mvKeys / mDescriptors) and
 * kps_r/desc_r (mvKeysRight / mDescriptorsRight) of a rectified pair whose
 * images were the last orbx_extract of `left` and `right` (their pyramids are
 * read on the device).  mb = baseline, mbf = baseline * fx (the reference
 * reads the member mb before assigning it at Frame.cc:94; callers pass
 * mbf / fx).  Outputs uright[nl] (mvuRight) and depth[nl] (mvDepth), -1 =
 * no match; *nmatches = stereo matches kept by the median filter.
 * ORBX_ERR_ARG where the reference would index out of range or throw. */
int orbx_stereo_match(orbx_extractor* left, orbx_extractor* right, const orbx_keypoint* kps_l,
                      const uint8_t* desc_l, int nl, const orbx_keypoint* kps_r,
                      const uint8_t* desc_r, int nr, float mb, float mbf, float* uright,
                      float* depth, int* nmatches);

/* Batched device path: nframes rectified pairs.  `left` / `right` are the
 * plans whose last orbx_plan_extract consumed d_frames_l / d_frames_r (their
 * device pyramids are read); keypoint arrays are the orbx_plan_extract
 * outputs ([nframes][kcap], counts [nframes]).  d_uright / d_depth are
 * [nframes][kcap], d_nmatches [nframes].  Asynchronous on `stream`;
 * orbs_plan_check() synchronises and reports latched range errors. */
typedef struct orbs_plan orbs_plan;
int orbs_plan_create(const orbx_plan* geometry, int max_batch, orbs_plan** out);
int orbs_plan_destroy(orbs_plan* sp);
int orbs_plan_match(orbs_plan* sp, int nframes, const orbx_plan* left, const orbx_plan* right,
                    const uint8_t* d_frames_l, const uint8_t* d_frames_r, size_t frame_stride,
                    size_t row_stride, const orbx_keypoint* d_kps_l, const uint8_t* d_desc_l,
                    const int* d_count_l, const orbx_keypoint* d_kps_r, const uint8_t* d_desc_r,
                    const int* d_count_r, float mb, float mbf, float* d_uright, float* d_depth,
                    int* d_nmatches, void* stream);
int orbs_plan_check(orbs_plan* sp, void* stream);
int orbs_plan_set_timing(orbs_plan* sp, int enable);
int orbs_plan_stage_times(orbs_plan* sp, double* ms, int* launches, int nstages);

/* ---------------------------------------------------------------------------
 * DBoW2 vocabulary transform: the producer of the
 * FeatureVectors SearchByBoW consumes (Frame::ComputeBoW / KeyFrame::ComputeBoW,
 * src/Frame.cc:375-382, src/KeyFrame.cc:39-48, levelsup = 4).
 *   TemplatedVocabulary<FORB::TDescriptor, FORB>
 *     loadFromTextFile     Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424
 *     transform(features, BowVector&, FeatureVector&, levelsup)          :1126-1191
 *     transform(feature, word, weight, nid, levelsup)                    :1222-1259
 * ------------------------------------------------------------------------- */
typedef struct orbv_vocab orbv_vocab;
/* Text vocabulary (ORBvoc.txt format): "k L scoring weighting" then one node
 * per line "parent isLeaf d0..d31 weight".  ORBX_ERR_ARG for a rejected
 * header (:1356-1360) or a parent that does not precede its child. */
int orbv_vocab_load_text(const char* path, int device, orbv_vocab** out);
/* The same from node records (record r = node r+1 in file order). */
int orbv_vocab_create(int k, int L, int scoring, int weighting, int nrec, const int32_t* parent,
                      const int32_t* is_leaf, const uint8_t* desc, const double* weight,
                      int device, orbv_vocab** out);
int orbv_vocab_destroy(orbv_vocab* v);
int orbv_vocab_info(const orbv_vocab* v, int* k, int* L, int* scoring, int* weighting,
                    int* nnodes, int* nwords);
/* transform(features, BowVector&, FeatureVector&, levelsup) on host
 * descriptors desc[n][32].  BowVector: bow_word[nbow] ascending with
 * bow_value[nbow] (WordValue = double, normalised as the scoring requires);
 * FeatureVector (DBoW2::FeatureVector, FeatureVector.h:21-22) as CSR:
 * fv_node[nfv] ascending, features fv_feat[fv_off[j] .. fv_off[j+1]) in
 * ascending index order -- exactly the orbx_bow_frame layout.  Outputs hold
 * n entries (fv_off n + 1).  ORBX_ERR_ARG where the reference would read an
 * uninitialised NodeId (a leaf above the levelsup level); at most 8192
 * descriptors per call (ORBX_ERR_UNSUPPORTED beyond). */
int orbv_transform(orbv_vocab* v, const uint8_t* desc, int n, int levelsup, uint32_t* bow_word,
                   double* bow_value, int* nbow, uint32_t* fv_node, uint32_t* fv_off,
                   uint32_t* fv_feat, int* nfv);
/* Batched device form over orbx_plan_extract outputs: d_desc [nframes][kcap][32],
 * d_counts [nframes]; outputs [nframes][kcap] (d_fv_off [nframes][kcap+1]) and
 * counts [nframes].  Asynchronous on `stream`; orbv_check() synchronises and
 * reports the latched unset-NodeId error. */
int orbv_transform_batch(orbv_vocab* v, int nframes, const uint8_t* d_desc, const int* d_counts,
                         int kcap, int levelsup, uint32_t* d_bow_word, double* d_bow_value,
                         int* d_nbow, uint32_t* d_fv_node, uint32_t* d_fv_off, uint32_t* d_fv_feat,
                         int* d_nfv, void* stream);
int orbv_check(orbv_vocab* v, void* stream);

/* ---------------------------------------------------------------------------
 * Place recognition: the two consumers of the BowVector.
 *   TemplatedVocabulary::score(a, b)     TemplatedVocabulary.h:1199-1203,
 *                                        Thirdparty/DBoW2/DBoW2/ScoringObject.cpp
 *   KeyFrameDatabase add / erase / clear and the word walk of
 *   DetectLoopCandidates / DetectRelocalizationCandidates
 *                                        src/KeyFrameDatabase.cc:56-85,179-203
 * BowVectors in the layout orbv_transform emits: word[n] strictly ascending
 * and below the vocabulary's nwords (else ORBX_ERR_ARG), value[n] finite
 * doubles (not necessarily normalised); more than 8192 words in one vector:
 * ORBX_ERR_UNSUPPORTED.  Scores are bit-equal to ScoringObject.cpp for the
 * vocabulary's scoring L1_NORM (0), L2_NORM (1), CHI_SQUARE (2) and
 * DOT_PRODUCT (5); KL (3) and BHATTACHARYYA (4): ORBX_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
/* TemplatedVocabulary::score of one vector against nvec vectors (CSR: vector j is
 * b_word/b_value[b_off[j] .. b_off[j+1])), with the vocabulary's scoring. Host buffers,
 * synchronous. */
int orbv_score(const orbv_vocab* v, const uint32_t* a_word, const double* a_value, int na,
               const uint32_t* b_off, const uint32_t* b_word, const double* b_value, int nvec,
               double* score);

/* The keyframe database: the stored BowVectors live on the device.  The
 * vocabulary is read at creation only (scoring, nwords).  One host thread
 * calls a given orbv_db at a time (the reference holds mMutex). */
typedef struct orbv_db orbv_db;
/* reserve_words: initial capacity of the device word store (0 = default); it grows on demand */
int orbv_db_create(const orbv_vocab* v, size_t reserve_words, int device, orbv_db** out);
int orbv_db_destroy(orbv_db* db);
/* ORBX_ERR_ARG for a kf_id already present */
int orbv_db_add(orbv_db* db, uint64_t kf_id, const uint32_t* word, const double* value, int n);
int orbv_db_erase(orbv_db* db, uint64_t kf_id);   /* an absent id is a no-op, as in the reference */
int orbv_db_clear(orbv_db* db);
int orbv_db_size(const orbv_db* db, int* nkf);
/* Every stored keyframe that shares at least one word with the query, in the order the reference's
 * lKFsSharingWords would hold them if nothing were excluded; per entry its id, the number of
 * common words, and score(query, keyframe). cap entries; ORBX_ERR_CAPACITY with *nsharing = the
 * required count.  n == 0 or an empty database: ORBX_OK with *nsharing = 0. */
int orbv_db_query(orbv_db* db, const uint32_t* word, const double* value, int n, int cap,
                  uint64_t* kf_id, int32_t* ncommon, double* score, int* nsharing);

#define ORBV_QUERY_GATED 1  /* keep only entries with ncommon > (int)(maxCommonWords * 0.8f) */

/* nq queries in CSR form: query q is q_word/q_value[q_off[q] .. q_off[q+1]), q_off[0] == 0.
 * Result in CSR form: query q's entries are [out_off[q], out_off[q+1]) of kf_id / ncommon / score,
 * each segment exactly what orbv_db_query returns for that query (same ids, order, counts,
 * score bits).  With ORBV_QUERY_GATED the segment is that list with the entries whose
 * ncommon <= (int)(max ncommon of the segment * 0.8f) removed, order kept:
 * KeyFrameDatabase.cc:207-233 with nothing excluded.
 * cap = entries the three arrays hold in total.  ORBX_ERR_CAPACITY: out_off[] is filled with the
 * required offsets (out_off[nq] = required total) and no entry is written.  out_off (nq + 1
 * entries) is always required and filled; nq == 0, empty queries and an empty database give
 * ORBX_OK with empty segments.  ORBX_ERR_ARG for unknown flag bits, q_off[0] != 0, a descending
 * q_off or words not strictly ascending below nwords; ORBX_ERR_UNSUPPORTED for a query of more
 * than 8192 words or nq * (slots in the store) >= 2^31.  Synchronous, host buffers. */
int orbv_db_query_batch(orbv_db* db, int nq, const uint32_t* q_off, const uint32_t* q_word,
                        const double* q_value, int flags, int cap, uint32_t* out_off,
                        uint64_t* kf_id, int32_t* ncommon, double* score);

/* The same on device buffers, asynchronous on `stream`.
 * Queries: [nq][qstride] with d_n[nq], the layout of orbv_transform_batch's d_bow_word /
 * d_bow_value / d_nbow with qstride = kcap (qstride > 8192: ORBX_ERR_UNSUPPORTED).
 * d_n[q] < 0 counts as 0; d_n[q] > qstride gives d_nsharing[q] = -1 and nothing written for q.
 * The words are taken as orbv_transform_batch emits them (strictly ascending, below nwords) and
 * are NOT checked: other words give a wrong list, never an access out of range.
 * Outputs: [nq][cap], and d_nsharing[nq] = the full count.  Entries beyond cap are not written.
 * For L2_NORM d_score holds the sum s before the scoring's closing step, which the caller
 * applies: score = s >= 1 ? 1.0 : 1.0 - sqrt(1.0 - s) (the host forms apply it themselves).
 * The call leaves work in flight that reads the store and the handle's scratch: a later call of
 * this form on another stream waits for it on the device, every other orbv_db_* call on the
 * host.  The caller keeps its buffers alive until `stream` has run the work. */
int orbv_db_query_batch_device(orbv_db* db, int nq, const uint32_t* d_word, const double* d_value,
                               const int* d_n, int qstride, int flags, int cap, uint64_t* d_kf_id,
                               int32_t* d_ncommon, double* d_score, int* d_nsharing, void* stream);

/* ---------------------------------------------------------------------------
 * Projection matchers: the frame grid
 * (Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea,
 * src/Frame.cc:210-225,307-371, 64 x 48 cells) and the windowed Hamming
 * search of ORBmatcher::SearchByProjection.  Query form: per query the
 * arguments the reference hands to GetFeaturesInArea plus the gates' inputs.
 * The caller may project itself, or have the rows built on the device from
 * map points and a pose (orbm_project_points / orbm_proj_plan_project /
 * orbm_proj_plan_track below).
 * ------------------------------------------------------------------------- */
typedef struct {
  float x, y;                    /* mTrackProjX/Y (mode 1) or the projection u, v       */
  float radius;                  /* the r argument of GetFeaturesInArea (already scaled)  */
  int32_t min_level, max_level;  /* its level bounds (-1 = the defaults)                 */
  float xr;                      /* mode 1: mTrackProjXR (stereo gate, :39-43)           */
  float angle;                   /* modes 2/3: angle of the source keypoint             */
} orbx_query_proj;

typedef struct {
  int n;
  const orbx_keypoint* keys;  /* mvKeysUn                                              */
  const uint8_t* desc;        /* mDescriptors, n x 32                                   */
  const float* uright;        /* mvuRight (mode 1 stereo gate), NULL = monocular        */
  const uint8_t* occupied;    /* mode 1: mvpMapPoints[i] && Observations() > 0;
                                 modes 2/3: mvpMapPoints[i] != NULL; NULL = none        */
  float min_x, min_y;         /* mnMinX, mnMinY                                         */
  float grid_w_inv, grid_h_inv; /* mfGridElementWidthInv / HeightInv                    */
} orbx_proj_frame;

/* mode 1: SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:19-61):
 *         best/second over unoccupied candidates, accept best <= TH_HIGH and
 *         best <= nnratio * second (th_dist and check_ori unused).
 * mode 2: SearchByProjection(Frame& Current, const Frame& Last, th, bMono) (:732-818):
 *         accept best <= th_dist (TH_HIGH); rotation check if check_ori.
 * mode 3: SearchByProjection(Frame&, KeyFrame*, set<MapPoint*>&, th, ORBdist) (:820-894):
 *         accept best <= th_dist (ORBdist); rotation check if check_ori.
 * Queries are walked in order (each takes its best unoccupied candidate,
 * later queries skip it).  match[i] = the query that took feature i, or -1.
 * At most 8192 features.  Synchronous; host buffers. */
int orbm_search_by_projection(int mode, const orbx_proj_frame* frame, const orbx_query_proj* q,
                              const uint8_t* qdesc, int nq, float nnratio, int th_dist,
                              int check_ori, int device, int32_t* match, int* nmatches);

/* Batched device form of orbm_search_by_projection: nprob independent
 * problems (e.g. the current frames of many streams, each with its projected
 * map points) searched in one set of launches -- the grid of every frame, a
 * wavefront per (query, problem), the greedy walk of every problem in
 * parallel.  Every pointer of a problem is DEVICE memory (frame.keys / desc
 * / uright / occupied, q, qdesc; outputs match[frame.n] and *nmatches);
 * asynchronous on `stream`.  Same results as orbm_search_by_projection on
 * each problem.  A plan holds the scratch for max_problems problems of at
 * most max_n features (<= 8192) and max_nq queries; one host thread calls a
 * plan at a time (the problem table is staged in pinned memory; a call
 * waits on the host for the previous call's table upload, not for its
 * kernels).  Calls may use different streams: each call's stream waits on
 * the device for the previous call's kernels before it reuses the plan's
 * scratch. */
typedef struct {
  orbx_proj_frame frame;
  const orbx_query_proj* q;
  const uint8_t* qdesc;
  int nq;
  int32_t* match;
  int* nmatches;
} orbx_proj_problem;
typedef struct orbm_proj_plan orbm_proj_plan;
int orbm_proj_plan_create(int max_problems, int max_n, int max_nq, int device, orbm_proj_plan** out);
int orbm_proj_plan_destroy(orbm_proj_plan* plan);
int orbm_proj_plan_search(orbm_proj_plan* plan, int mode, int nprob, const orbx_proj_problem* probs,
                          float nnratio, int th_dist, int check_ori, void* stream);

/* ---------------------------------------------------------------------------
 * Device-side projection for the three SearchByProjection forms: map points
 * and a pose in, orbx_query_proj rows out.
 *   mode 1: Frame::isInFrustum (src/Frame.cc:249-305) + the radius / levels of
 *           SearchByProjection(Frame&, vector<MapPoint*>&, th) (:19-28,67-69)
 *   mode 2: the projection of the last-frame form (:750-774)
 *   mode 3: the projection of the keyframe form (:832-848)
 * Point i writes query row i; there is no compaction.  Where the reference
 * executes `continue` / `return false`, the row is inert: x = y = 0,
 * radius = -1, min_level = max_level = -1, xr = angle = 0 and level[i] = -1.
 * An inert row fails the matcher's strict box test for every feature, so it
 * takes nothing and match[] of a search over these rows names the map point.
 * The one deviation: a point the reference would hand to GetFeaturesInArea
 * with a NaN / infinite u or v (it converts them to int), and a mode-2 octave
 * outside [0, nlevels), is written inert and counted in n_nonfinite.
 * ------------------------------------------------------------------------- */
#define ORBX_PROJ_MAX_LEVELS 32
typedef struct {
  float Rcw[9], tcw[3];        /* rows 0..2 of mTcw: rotation (row-major), translation      */
  float ow[3];                 /* camera centre: mOw (mode 1), twc (modes 2, 3); computed
                                  by the caller once per frame                              */
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY                       */
  int nlevels;                 /* mnScaleLevels, 1 .. ORBX_PROJ_MAX_LEVELS                  */
  float scale_factors[ORBX_PROJ_MAX_LEVELS]; /* mvScaleFactors, nlevels used                */
  float log_scale_factor;      /* mfLogScaleFactor: finite, > 0                             */
} orbx_proj_camera;

/* map points of one problem, npts entries per array; the arrays a mode does
 * not read may be NULL */
typedef struct {
  const float* pos;           /* [npts][3] GetWorldPos()                                    */
  const float* normal;        /* mode 1: [npts][3] GetNormal()                              */
  const float* min_dist_inv;  /* mode 1: GetMinDistanceInvariance()                         */
  const float* max_dist_inv;  /* mode 1: GetMaxDistanceInvariance()                         */
  const float* max_dist;      /* modes 1, 3: the raw mfMaxDistance PredictScale divides
                                 (not the x1.2 value)                                       */
  const int32_t* octave;      /* mode 2: LastFrame.mvKeys[i].octave                         */
  const float* angle;         /* mode 2: LastFrame.mvKeys[i].angle; mode 3: pKF->mvKeys[i]  */
  const uint8_t* skip;        /* NULL = none; 1 where the reference skips the point before
                                 projecting -- mode 1: mnLastFrameSeen == id or isBad();
                                 mode 2: null or outlier; mode 3: null, bad or already found */
} orbx_proj_points;

enum { ORBX_LEVEL_RULE_NEITHER = 0, ORBX_LEVEL_RULE_FORWARD = 1, ORBX_LEVEL_RULE_BACKWARD = 2 };
typedef struct {
  float th;                /* the th argument of the reference call                          */
  float viewing_cos_limit; /* mode 1: isInFrustum's second argument                          */
  int level_rule;          /* mode 2: bForward / bBackward, evaluated by the caller          */
} orbx_proj_params;

/* thr[L], L = 0 .. nlevels - 2: the smallest positive float ratio for which
 * MapPoint::PredictScale (src/MapPoint.cc:364-373: logf, divide, ceil,
 * truncate, clamp) gives a level above L under this host's logf; +inf where no
 * finite ratio does.  The kernels count thresholds instead of taking a
 * logarithm.  ORBX_ERR_ARG for nlevels outside 1 .. ORBX_PROJ_MAX_LEVELS and a
 * log_scale_factor that is not finite, is <= 0, or so small that
 * logf(FLT_MAX) / log_scale_factor reaches 2^31. */
int orbm_predict_scale_thresholds(float log_scale_factor, int nlevels, float* thr);

/* nprob problems (problem p: cameras[p], points[p], npts[p]; `params` is
 * shared) in one launch.  Host pointers; synchronous.  Outputs are
 * concatenated in problem order: q, level and view_cos (mode 1: mTrackViewCos
 * of the live rows, 0 for inert ones; may be NULL) hold sum(npts) entries,
 * n_in_view[p] = live rows of problem p (nToMatch).  nprob == 0 and
 * npts[p] == 0 are valid.  ORBX_ERR_ARG for a bad mode / count / camera, a
 * NULL array the mode reads, and where any problem counts a non-finite point;
 * no output is written then. */
int orbm_project_points(int mode, int nprob, const orbx_proj_camera* cameras,
                        const orbx_proj_points* points, const int* npts,
                        const orbx_proj_params* params, int device, orbx_query_proj* q,
                        int32_t* level, float* view_cos, int* n_in_view);

/* The same on device pointers, as methods of orbm_proj_plan (which stages the
 * problem table and keeps the threshold tables): `camera` holds values, every
 * pointer of `points` and every output is DEVICE memory.
 * orbm_proj_plan_project: q[npts] and level[npts] are required, view_cos,
 *   n_in_view and n_nonfinite (one int each) may be NULL; frame, qdesc, match
 *   and nmatches are not read.
 * orbm_proj_plan_track: projection followed by orbm_proj_plan_search's search
 *   on the same stream with nq = npts and qdesc = the map points' descriptors
 *   [npts][32]; match[frame.n] holds map-point indices.  q and level may be
 *   NULL (the rows then stay in the plan's scratch).  npts <= max_nq and
 *   frame.n <= max_n of the plan.
 * Asynchronous on `stream`; n_nonfinite is left for the caller to read.  The
 * one-host-thread and cross-stream rules of orbm_proj_plan_search hold. */
typedef struct {
  orbx_proj_camera camera;
  orbx_proj_points points;
  int npts;
  orbx_query_proj* q;
  int32_t* level;
  float* view_cos;
  int* n_in_view;
  int* n_nonfinite;
  orbx_proj_frame frame; /* track only, as in orbx_proj_problem */
  const uint8_t* qdesc;
  int32_t* match;
  int* nmatches;
} orbx_proj_build_problem;
int orbm_proj_plan_project(orbm_proj_plan* plan, int mode, int nprob,
                           const orbx_proj_build_problem* problems,
                           const orbx_proj_params* params, void* stream);
int orbm_proj_plan_track(orbm_proj_plan* plan, int mode, int nprob,
                         const orbx_proj_build_problem* problems,
                         const orbx_proj_params* params, float nnratio, int th_dist,
                         int check_ori, void* stream);

/* ---------------------------------------------------------------------------
 * Device-side projection for ORBmatcher::Fuse (both forms) and SearchBySim3:
 * map points and a pose in, orbx_kf_query rows out, and the
 * device-pointer plan form of orbm_keyframe_search's search.
 *   ORBX_KF_FORM_FUSE: p3Dc = Rcw * p + tcw; dist = |p - ow|; fx fy cx cy of
 *           the target keyframe (src/ORBmatcher.cc:514-531, :582-599; for the
 *           Scw form Rcw / tcw are rows 0..2 of Scw as they stand)
 *   ORBX_KF_FORM_SIM3: p3Dc2 = sR21 * (Rcw * p + tcw) + t21 with Rcw / tcw =
 *           R1w / t1w of pKF1; dist = |p3Dc2|; fx fy cx cy of pKF1, bounds
 *           and scale tables of pKF2 (:639-642, :676-694); ow is not read
 * Then, for both: Z < 0 rejects; invz = 1 / Z; x = X * invz; u = fma(x, fx,
 * cx) (fused, as the reference's object has it); KeyFrame::IsInImage (u >=
 * min_x && u < max_x && v >= min_y && v < max_y); dist outside [min_dist_inv,
 * max_dist_inv] rejects; level = PredictScale(dist); radius = th *
 * scale_factors[level].
 * Point i writes query row i and level[i]; there is no compaction.  Where the
 * reference executes `continue`, the row is inert: x = y = 0, radius = -1,
 * level = -1, desc = the row's own pool index, and level[i] = -1.  The search's
 * strict box test rejects every feature for it, so an inert row returns
 * -1 / INT_MAX; queries never interact, so it changes no other row.
 * The one deviation: a live row whose radius is not finite is written inert
 * and counted in n_nonfinite.
 * ------------------------------------------------------------------------- */
enum { ORBX_KF_FORM_FUSE = 1, ORBX_KF_FORM_SIM3 = 2 };
typedef struct {
  float Rcw[9], tcw[3];        /* rotation (row-major) and translation: pKF (FUSE), pKF1 (SIM3) */
  float ow[3];                 /* FUSE: camera centre, computed by the caller                */
  float sR21[9], t21[3];       /* SIM3: (1 / s12) * R12^T and -sR21 * t12, by the caller     */
  float fx, fy, cx, cy;
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY of the searched keyframe */
  int nlevels;                 /* mnScaleLevels, 1 .. ORBX_PROJ_MAX_LEVELS                   */
  float scale_factors[ORBX_PROJ_MAX_LEVELS]; /* mvScaleFactors, nlevels used                 */
  float log_scale_factor;      /* mfLogScaleFactor: finite, > 0                              */
} orbx_kf_camera;

/* map points of one problem, npts entries per array */
typedef struct {
  const float* pos;           /* [npts][3] GetWorldPos()                                     */
  const float* min_dist_inv;  /* GetMinDistanceInvariance()                                  */
  const float* max_dist_inv;  /* GetMaxDistanceInvariance()                                  */
  const float* max_dist;      /* the raw mfMaxDistance PredictScale divides                  */
  const uint8_t* skip;        /* NULL = none; 1 where the reference skips the point before it
                                 projects -- Fuse: null, bad, IsInKeyFrame / GetMapPoint(
                                 GetIndexInKeyFrame); SearchBySim3: null, already matched, bad */
} orbx_kf_points;

/* nprob problems (problem p: cameras[p], points[p], npts[p]; th is shared) in
 * one launch.  Host pointers; synchronous.  q and level hold sum(npts) entries
 * in problem order, n_live[p] = the live rows of problem p.  q[..].desc =
 * desc_base[p] + i (i when desc_base is NULL), so the rows go straight into
 * orbm_keyframe_search with qoff = the prefix of npts, over a descriptor pool
 * that is shared (every desc_base[p] = 0: one point set, many keyframes) or
 * per problem (desc_base = that prefix).  nprob == 0 and npts[p] == 0 are
 * valid.  ORBX_ERR_ARG for a bad form / count / camera, a negative desc_base,
 * a NULL array, and where any problem counts a non-finite radius; no output
 * is written then. */
int orbm_keyframe_project(int form, int nprob, const orbx_kf_camera* cameras,
                          const orbx_kf_points* points, const int* npts, const int32_t* desc_base,
                          float th, int device, orbx_kf_query* q, int32_t* level, int* n_live);

/* The same, and orbm_keyframe_search's search, on device pointers and
 * asynchronous on `stream`.  A plan holds the scratch (grids, feature records,
 * staged problem tables, query rows, PredictScale threshold tables) for
 * max_problems problems of at most max_n features (<= 8192) and max_queries
 * points; everything is allocated by _create.  One host thread calls a plan at
 * a time; a call waits on the host for the previous call's table upload only,
 * and its stream waits on the device for the previous call's kernels before it
 * reuses the scratch.
 * One problem: `camera` holds values; every pointer is DEVICE memory.  Point
 * arrays and qdesc of different problems may alias (one point set, many
 * keyframes).  Row i's descriptor is qdesc + 32 * q[i].desc; the rows the
 * projection writes have desc = i.
 * orbm_kf_plan_search: q[npts] is given (x, y, radius, level, desc in
 *   [0, npts); a desc outside it returns -1 / INT_MAX); best_idx[npts] and
 *   best_dist[npts] are written as orbm_keyframe_search writes them.  camera,
 *   points, level, n_live and n_nonfinite are not read.
 * orbm_kf_plan_project: q[npts] and level[npts] are written; n_live and
 *   n_nonfinite (one int each) may be NULL; frame, qdesc, best_* are not read.
 * orbm_kf_plan_project_search: both on one stream; q and level may be NULL
 *   (the rows then stay in the plan's scratch). */
typedef struct {
  orbx_kf_camera camera;
  orbx_kf_points points;
  int npts;
  const uint8_t* qdesc;  /* [npts][32] */
  orbx_kf_frame frame;   /* keys: orbx_keypoint rows on the device */
  orbx_kf_query* q;
  int32_t* level;
  int* n_live;
  int* n_nonfinite;
  int32_t* best_idx;
  int32_t* best_dist;
} orbx_kf_problem;
typedef struct orbm_kf_plan orbm_kf_plan;
int orbm_kf_plan_create(int max_problems, int max_n, int max_queries, int device, orbm_kf_plan** out);
int orbm_kf_plan_destroy(orbm_kf_plan* plan);
int orbm_kf_plan_search(orbm_kf_plan* plan, int nprob, const orbx_kf_problem* problems, void* stream);
int orbm_kf_plan_project(orbm_kf_plan* plan, int form, int nprob, const orbx_kf_problem* problems,
                         float th, void* stream);
int orbm_kf_plan_project_search(orbm_kf_plan* plan, int form, int nprob,
                                const orbx_kf_problem* problems, float th, void* stream);

/* ---------------------------------------------------------------------------
 * Optimizer::PoseOptimization (src/Optimizer.cc:220-432), batched (DESIGN.md
 * §19): the four rounds of g2o's Levenberg loop over one 6-DoF vertex and the
 * frame's unary reprojection edges, one launch for all problems.  Sums over
 * edges are taken in the fixed device order of DESIGN §19, not in edge order.
 * ------------------------------------------------------------------------- */
typedef struct {
  float Tcw[12];               /* rows 0..2 of mTcw */
  float fx, fy, cx, cy, mbf;
  int nlevels;                 /* 1 .. ORBX_PROJ_MAX_LEVELS */
  float inv_level_sigma2[ORBX_PROJ_MAX_LEVELS];   /* mvInvLevelSigma2 */
} orbx_pose_camera;

typedef struct {
  int n;                       /* Frame::N, <= 8192 */
  const orbx_keypoint* keys;   /* mvKeysUn: pt and octave are read */
  const float* uright;         /* mvuRight; NULL = all monocular */
  const float* pos;            /* world positions, [n][3] or a pool */
  const int32_t* point_index;  /* NULL: feature i uses pos[i] where has_point[i];
                                  else pos[point_index[i]], -1 = no point.  This is
                                  orbm_proj_plan_track's match[] as it stands */
  const uint8_t* has_point;    /* read only when point_index is NULL; NULL = all */
  int npos;                    /* pool size, bounds point_index */
} orbx_pose_obs;

#define ORBX_POSE_MAX_N 8192
/* Host pointers; synchronous.  Tcw_out[p] = the 4x4 pose (row-major),
 * outlier = mvbOutlier of every problem, concatenated (sum of n; 0 where a
 * feature has no point), ninliers[p] = the return value.  Where the reference
 * returns 0 (fewer than 3 correspondences) ninliers[p] = 0 and Tcw_out[p] is
 * the input pose.  nprob == 0 and n == 0 are valid.  ORBX_ERR_ARG, with no
 * output written, for a bad count (nprob, n, npos, nlevels), an octave outside
 * [0, nlevels), a point_index outside [-1, npos), npos < n without
 * point_index, or a required pointer that is NULL. */
int orbm_pose_optimization(int nprob, const orbx_pose_camera* cameras, const orbx_pose_obs* obs,
                           int device, float* Tcw_out, uint8_t* outlier, int* ninliers);

/* The same on device memory, asynchronous on `stream`: every pointer of obs and
 * the four outputs are device pointers; the problem table itself is host
 * memory, staged by the call.  Tcw_out[16], outlier[obs.n], ninliers (one int)
 * and status (one int) are written per problem.  A feature with a bad octave or
 * point index cannot be refused here: it is taken as having no point and
 * counted in *status (0 = none).  One host thread per plan; calls on different
 * streams are ordered by the plan as orbm_proj_plan_search's are.  It may
 * follow orbm_proj_plan_track on the same stream with point_index = match. */
typedef struct {
  orbx_pose_camera camera;
  orbx_pose_obs obs;
  float* Tcw_out;
  uint8_t* outlier;
  int* ninliers;
  int* status;
} orbx_pose_problem;
typedef struct orbm_pose_plan orbm_pose_plan;
int orbm_pose_plan_create(int max_problems, int max_n, int device, orbm_pose_plan** out);
int orbm_pose_plan_destroy(orbm_pose_plan* plan);
int orbm_pose_plan_optimize(orbm_pose_plan* plan, int nprob, const orbx_pose_problem* problems, void* stream);

/* ---------------------------------------------------------------------------
 * Initializer::FindHomography / FindFundamental (src/Initializer.cc:80-404),
 * batched over frame pairs: nit RANSAC hypotheses of each
 * model per pair (8-point DLT, symmetric transfer / epipolar score of every
 * match), the winners, their inlier flags and RH = SH / (SH + SF), which is
 * Initialize (:16-72) up to the choice of the model.  ReconstructH / ReconstructF
 * stay with the caller.  The SVD, the 3x3 products and the inverses are this
 * library's own fixed forms ("unpinned"), not OpenCV's.
 * ------------------------------------------------------------------------- */
typedef struct {
  int n1, n2;
  const orbx_keypoint* keys1;  /* mvKeysUn of the reference frame (pt read) */
  const orbx_keypoint* keys2;  /* mvKeysUn of the current frame */
  const int32_t* match12;      /* n1, as orbm_search_for_initialization leaves it */
  const int32_t* sets;         /* nit * 8, indices into the match list (mvSets) */
} orbx_ransac_pair;

typedef struct {
  float H21[9], F21[9];        /* row-major; zeros where the winner is absent */
  float SH, SF, RH;
  int32_t it_H, it_F;          /* winning iteration, -1 for none */
  int32_t nmatch;
} orbx_ransac_result;

/* Host pointers; synchronous; safe from several threads.  The match list
 * (mvMatches12) of a pair holds the rows with match12[i] >= 0 in ascending i;
 * inliers_H / inliers_F receive one flag per entry of it, nmatch of them, at
 * inl_off[p] (inl_off has npair + 1 entries; bytes past nmatch are not
 * written).  A model none of whose hypotheses scores above 0 has it = -1, a
 * zero matrix, score 0 and all flags 0; RH is NaN for 0 / 0.  npair == 0 and
 * nit == 0 are valid.  ORBX_ERR_ARG, with no output written, for npair < 0,
 * nit < 0, a required pointer that is NULL, a non-finite key coordinate or
 * sigma, a match12 entry >= n2, a set index outside [0, nmatch), fewer than 8
 * matches in a pair, or inl_off[p + 1] - inl_off[p] < nmatch;
 * ORBX_ERR_UNSUPPORTED for n1 or n2 > 8192, nit > 4096 or npair > 65535. */
int orbm_initializer_ransac(int npair, const orbx_ransac_pair* pairs, int nit, float sigma, int device,
                            orbx_ransac_result* res,
                            uint8_t* inliers_H, uint8_t* inliers_F, const int32_t* inl_off /* npair + 1 */);

/* ---------------------------------------------------------------------------
 * Initializer::ReconstructH / ReconstructF (src/Initializer.cc:406-864),
 * batched over frame pairs: the 8 or 4 pose candidates of the
 * chosen model, CheckRT of every inlier match under each (Triangulate, the
 * depth, reprojection and parallax tests), the reference's decision, R21, t21
 * and the winner's points.  Together with orbm_initializer_ransac this is
 * Initialize (:16-77) from the match list on.  The SVD, the determinant, the
 * norms, the products and acos are this library's own fixed forms (DESIGN §21,
 * "unpinned"), not OpenCV's or libm's.
 * ------------------------------------------------------------------------- */
#define ORBX_RECON_H 0    /* ReconstructH from ransac->H21 and inliers_H */
#define ORBX_RECON_F 1    /* ReconstructF from ransac->F21 and inliers_F */
#define ORBX_RECON_AUTO 2 /* H when ransac->RH > 0.40 (:73), else F */

typedef struct {
  int n1, n2;
  const orbx_keypoint* keys1;        /* as in orbx_ransac_pair */
  const orbx_keypoint* keys2;
  const int32_t* match12;            /* n1 */
  float K[9];                        /* row-major calibration matrix (mK) */
  int32_t model;                     /* ORBX_RECON_* */
  const orbx_ransac_result* ransac;  /* one record, as orbm_initializer_ransac left it */
  const uint8_t* inliers_H;          /* ransac->nmatch flags each, match-list order; */
  const uint8_t* inliers_F;          /* under a forced model the other may be NULL */
} orbx_recon_pair;

typedef struct {
  int32_t ok;                        /* the reference's return value */
  int32_t model_used;                /* ORBX_RECON_H or ORBX_RECON_F */
  float R21[9], t21[3];              /* row-major; zeros when !ok */
  int32_t best;                      /* the winning candidate; ReconstructH's bestSolutionIdx
                                        even when it then fails; -1 for none */
  int32_t ncand;                     /* 8 (H), 4 (F), 0 (ReconstructH's singular-value exit or
                                        an absent model) */
  int32_t nGood[8];                  /* CheckRT's return per candidate; 0 past ncand */
  float parallax[8];                 /* CheckRT's parallax in degrees; 0 past ncand */
  int32_t n_inliers;                 /* N: the set flags of the model used */
} orbx_recon_result;

/* Host pointers; synchronous; safe from several threads.  P3D receives n1 rows
 * of 3 floats per pair at 3 * key_off[p] and triangulated n1 flags at
 * key_off[p], both indexed by the key of frame 1 as vP3D / vbTriangulated are
 * (key_off has npair + 1 entries; rows past n1 are not written): the point and
 * flag of every match the winning candidate counts, zeros for a key that is
 * unmatched, no inlier or not counted.  sigma: the Initializer's (th2 = 4 sigma^2);
 * min_parallax in degrees and min_triangulated as Initialize passes them (1.0,
 * 50).  When ok == 0, R21, t21 and the pair's P3D rows and flags are zero and
 * the diagnostics (best, ncand, nGood, parallax, n_inliers) are still filled; a
 * model whose matrix is absent (it_H / it_F < 0) gives ok = 0 with ncand = 0.
 * npair == 0 is valid.  ORBX_ERR_ARG, with no output written, for npair < 0, a
 * required pointer that is NULL (under ORBX_RECON_AUTO both flag arrays are
 * required), a non-finite entry of K, sigma, min_parallax or key coordinate, a
 * match12 entry >= n2, a model outside ORBX_RECON_*, ransac->nmatch different
 * from the count of match12[i] >= 0, or key_off[p] < 0 or key_off[p + 1] -
 * key_off[p] < n1; ORBX_ERR_UNSUPPORTED for n1 or n2 > 8192 or npair > 65535. */
int orbm_initializer_reconstruct(int npair, const orbx_recon_pair* pairs, float sigma, float min_parallax,
                                 int min_triangulated, int device, orbx_recon_result* res, float* P3D,
                                 uint8_t* triangulated, const int32_t* key_off /* npair + 1 */);

/* ---------------------------------------------------------------------------
 * Sim3Solver (src/Sim3Solver.cc), batched: the constructor's
 * per-correspondence values (camera coordinates, image points, the two error
 * bounds) and iterate's RANSAC loop -- Horn's closed form on three point pairs
 * per hypothesis, both reprojections of every correspondence, and the
 * reference's sequential choice of the best and of the returning iteration --
 * for any number of solvers in one launch.  One problem is one solver: one
 * (current keyframe, candidate) pair after the constructor's filtering
 * (:44-59), which stays with the caller, as does the rand() draw (:143-157).
 * cv::eigen of the 4x4, atan2, cv::Rodrigues with its sin and cos, the centroid,
 * the 3x3 products, Mat::dot / cv::norm and the scaled products are this
 * library's own fixed forms ("unpinned"), not OpenCV's or libm's;
 * Project, FromCameraToImage, the truncated bound and the comparison are
 * pinned from the reference's object.
 * ------------------------------------------------------------------------- */
typedef struct {
  int ncorr;                  /* N: correspondences kept by the constructor, <= 8192        */
  const float* pos1;          /* [ncorr][3] GetWorldPos() of pMP1                            */
  const float* pos2;          /* [ncorr][3] GetWorldPos() of pMP2                            */
  const float* sigma2_1;      /* [ncorr] pKF1->mvLevelSigma2[kp1.octave]                     */
  const float* sigma2_2;      /* [ncorr] pKF2->mvLevelSigma2[kp2.octave]                     */
  float Rcw1[9], tcw1[3];     /* pKF1->GetRotation() (row-major), GetTranslation()           */
  float Rcw2[9], tcw2[3];     /* pKF2                                                        */
  float fx1, fy1, cx1, cy1;   /* pKF1->mK                                                    */
  float fx2, fy2, cx2, cy2;   /* pKF2->mK                                                    */
  int nit;                    /* hypotheses this call evaluates, <= 4096                     */
  const int32_t* triples;     /* [nit][3] indices into the correspondences; an index may
                                 repeat within a triple                                      */
  int min_inliers;            /* mRansacMinInliers                                           */
  int fix_scale;              /* mbFixScale                                                  */
  int best_in;                /* mnBestInliers on entry: 0 for a fresh solver, n_best of the
                                 previous call to continue it                                */
} orbx_sim3_problem;

typedef struct {
  int32_t it_hit;             /* the iteration at which iterate returns a transformation
                                 (:172), -1 for none                                         */
  int32_t it_best;            /* the iteration whose state mBest* holds on return; -1 when no
                                 iteration reached best_in                                   */
  int32_t n_best;             /* mnBestInliers on return (best_in when it_best is -1)        */
  int32_t ncorr;
  float R12[9], t12[3], s12;  /* GetEstimatedRotation / Translation / Scale; zeros when
                                 it_best is -1                                               */
  float sR21[9], t21[3];      /* rows 0..2 of mT21i of that iteration: orbx_kf_camera's sR21
                                 and t21 as they stand                                       */
} orbx_sim3_result;

/* Host pointers; synchronous; safe from several threads.  With c_i the inlier
 * count of iteration i and m_i = max(best_in, c_j for j < i): it_hit is the
 * first i with c_i >= m_i and c_i > min_inliers; it_best is the last i <= it_hit
 * (<= nit - 1 without a hit) with c_i >= m_i -- what the reference's sequential
 * loop leaves (>=, so later ties replace; a count of 0 passes while best_in is
 * 0, and a degenerate hypothesis is then reported as it is, NaNs included).
 * inliers receives mvbBestInliers, ncorr bytes at inl_off[p] (inl_off has nprob
 * + 1 entries; bytes past ncorr are not written); all 0 when it_best is -1.
 * ncorr < min_inliers is valid and inert (:126): it_hit = it_best = -1 and none
 * of the problem's arrays is read.  nprob == 0 and nit == 0 are valid.
 * ORBX_ERR_ARG, with no output written, for a negative count (nprob, ncorr,
 * nit, min_inliers, best_in), a required pointer that is NULL, ncorr < 3 in a
 * problem that is not inert, a triple index outside [0, ncorr), a non-finite
 * position, pose or camera entry, a sigma2 that is not finite, is negative or
 * has 9.210 * sigma2 >= 2^31, inl_off[p] < 0 or inl_off[p + 1] - inl_off[p] <
 * ncorr; ORBX_ERR_UNSUPPORTED for ncorr > 8192, nit > 4096 or nprob > 65535. */
int orbm_sim3_solve(int nprob, const orbx_sim3_problem* problems, int device, orbx_sim3_result* res,
                    uint8_t* inliers, const int32_t* inl_off /* nprob + 1 */);

/* ---------------------------------------------------------------------------
 * SURVEY.md §8f rank 4.
 * ------------------------------------------------------------------------- */
/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:222-271), batched
 * over map points: map point m's observation descriptors (mObservations order,
 * non-bad keyframes) are rows off[m] .. off[m+1]) of desc; best[m] = the row
 * (relative to off[m]) with the smallest median distance, the first on ties,
 * -1 for no observation. */
int orbm_compute_distinctive_descriptors(const uint8_t* desc, const int32_t* off, int nmp,
                                         int device, int32_t* best);
/* Frame::UndistortKeyPoints (src/Frame.cc:384-414): K = mK (3x3 row-major,
 * CV_32F), dist = mDistCoef, ndist = 0 .. 14 in OpenCV's order: k1 k2 p1 p2
 * [k3 [k4 k5 k6 [s1 s2 s3 s4 [tauX tauY]]]], missing ones 0.  k1 == 0
 * copies the keypoints (:386-390); otherwise cv::undistortPoints(.., K, D,
 * noArray(), K) (OpenCV 3.4: double, 5 iterations).  The tilt model is not
 * implemented: a non-zero tauX or tauY is ORBX_ERR_UNSUPPORTED (checked after
 * the k1 == 0 copy, before any device work).  out may equal kps. */
int orbx_undistort_keypoints(const orbx_keypoint* kps, int n, const float* K, const float* dist,
                             int ndist, int device, orbx_keypoint* out);

/* Multi-GPU boundary frame (bench/orbx.dist): one frame of
 * orbx_plan_extract outputs (kcap keypoint rows, kcap descriptor rows, the
 * count) as one contiguous record of orbx_boundary_record_bytes(kcap) bytes
 * [kps | desc | count | pad], the unit of the RCCL all-gather.  Device
 * pointers (kps/desc 4-B aligned), asynchronous on `stream`, one launch. */
size_t orbx_boundary_record_bytes(int kcap);
int orbx_boundary_pack(const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_count,
                       int kcap, uint8_t* d_record, void* stream);
int orbx_boundary_unpack(const uint8_t* d_record, int kcap, orbx_keypoint* d_kps, uint8_t* d_desc,
                         int* d_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */

// plan_internal.h -- host-side state of an extraction plan, of the stereo
// plan and of the ORBextractor drop-in, shared by the C-ABI translation units
// (the stereo matcher reads the device pyramid the extractor left behind, and
// the extractor owns the stereo plan of its orbx_stereo_match calls).  The
// handles hold their GPU resources in owners (owned.h): destroying one is
// `delete`, and its destructor only selects the device first.
#ifndef ORBX_PLAN_INTERNAL_H
#define ORBX_PLAN_INTERNAL_H

#include <hip/hip_runtime.h>

#include <memory>

#include "../../include/orbx.h"
#include "api_common.h"
#include "geometry.h"

struct orbx_plan {
  orbx::Plan P;
  int device = 0, max_batch = 0;
  orbx::Stream stream;
  orbx::DevBuf<LevelInfo> d_lv;
  orbx::DevBuf<CellInfo> d_cells;
  orbx::DevBuf<StripInfo> d_strips;
  int fs_tpitch = 0;
  /* k_fast_strips launches: strips [begin, end) of the (height-partitioned)
   * strip table with their tile rows, cells, corner-list entries and LDS */
  struct FsGroup {
    int begin = 0, end = 0, tmaxh = 7, mcells = 1, ccap = 0;
    size_t lds = 0;
  };
  FsGroup fs_grp[2];
  int fs_ngrp = 1;
  orbx::DevBuf<int32_t> d_xofs, d_xofs1, d_yofs;
  orbx::DevBuf<int32_t> d_pyr_xs, d_pyr_ys, d_pyr_bo;
  orbx::DevBuf<uint32_t> d_pyr_blob;
  orbx::DevBuf<int16_t> d_alpha, d_beta;
  orbx::DevBuf<uint8_t> d_pyr, d_blur;
  orbx::DevBuf<uint32_t> d_slots, d_ccount, d_qkeys, d_qout;
  orbx::DevBuf<uint32_t> d_qperm; /* per level: k_orient_brief's processing order (k_quadtree); then the twin tables below */
  orbx::DevBuf<int32_t> d_qnode;
  /* twin rows (LevelInfo::twin; plans with an alias level), parts of d_qperm's
   * allocation, not owned: the winners' key indices (qperm's layout), the
   * pairs' winner bitmaps with their rank prefixes, and per level whether its
   * bitmap is there */
  uint32_t *d_qkidx = nullptr, *d_twscr = nullptr;
  int* d_twvalid = nullptr;
  size_t tw_stride = 0;
  orbx::DevBuf<int> d_lcount, d_err;
  orbx::DevBuf<int> d_fs_cnt; /* k_fast_strips' striped debug counters (FS_CNT_LINES x FS_CNT_STRIDE) */
  long long fs_dense_total = 0, fs_ovf_total = 0; /* their sums since each was last read */
  orbx::PinnedBuf<int> h_err; /* pinned: orbx_plan_check reads the error word without a blocking copy */
  size_t pyr_stride = 0, blur_stride = 0, slot_stride = 0, qk_stride = 0, qout_stride = 0;
  size_t qt_lds = 0;
  size_t qt_lds_wide = 0; /* k_quadtree_wide (single-frame calls): + a second child array */
  BriefArgs bargs;
  BlurArgs blargs;  /* level-blur mode: k_blur's tiles */
  int lb_auto = 0;  /* the planner's BRIEF blur choice: 1 = level blur (k_blur + k_orient_brief_lb) */
  LevelArgs largs;
  orbx::StageTimer timer;
  int dbg = 0; /* ORBX_DEBUG_STOP: kernel phase early-exit for profiling only */
  int ob_div = 0; /* ORBX_DEBUG_OBDIV: k_orient_brief grid divisor, profiling only */
  /* ORBX_DEBUG_LDSPAD=pyr,fast,brief: extra dynamic LDS per workgroup
   * (occupancy probes: room for other streams' kernels), profiling only */
  int pad_pyr = 0, pad_fast = 0, pad_brief = 0;
  int fs_ccap = 0; /* FAST per-strip corner list entries (FS_CCAP; orbx_debug_set_fast_ccap fixes a lower one) */
  bool ccap_fixed_dbg = false; /* orbx_debug_set_fast_ccap: one launch group, that list length */
  int chunk = 0;  /* frames per extraction pass (0 = the whole batch in one pass) */
  hipEvent_t ev_after_pyr = nullptr; /* not owned: the extractor's ev_pyr, recorded after the pyramid launch when set (orbx_extract) */
  int overlap = 0; /* FAST on level 0 beside the pyramid on s_aux */
  orbx::Stream s_aux;
  orbx::Event ev_aux0, ev_aux1;
  int options = 0; /* ORBX_PLAN_* (include/orbx.h) */
  int nextracted = 0; /* frames of the last orbx_plan_extract (orbx_plan_level bound) */
  int uses_lb() const {
    return (options & ORBX_PLAN_BRIEF_LEVEL) ? 1 : (options & ORBX_PLAN_BRIEF_PATCH) ? 0 : lb_auto;
  }
  ~orbx_plan() { hipSetDevice(device); }
};

/* the stereo matcher's plan (api_stereo.hip) */
struct orbs_plan {
  int device = 0, max_batch = 0, waves = 4;
  int sm_div = 0; /* ORBX_DEBUG_SMDIV: k_stereo_match keypoints per wave, profiling only */
  orbx_params params;
  int W = 0, H = 0;
  StereoArgs args;
  orbx::DevBuf<int> d_rowoff;
  orbx::DevBuf<uint2> d_rows; /* CSR entries {iR | octave << 16, x} (kernels_stereo.hip) */
  orbx::DevBuf<int> d_sad;
  orbx::DevBuf<int> d_err;
  /* host drop-in (orbx_stereo_match) staging, batch 1 */
  orbx::DevBuf<orbx_keypoint> d_kl, d_kr;
  orbx::DevBuf<uint8_t> d_dl, d_dr;
  orbx::DevBuf<int> d_cnt; /* [2]: left, right */
  orbx::DevBuf<float> d_ur, d_dep;
  orbx::DevBuf<int> d_nm;
  orbx::Stream stream;
  orbx::StageTimer timer;
  ~orbs_plan() { hipSetDevice(device); }
};

/* everything an extractor holds for the current image size: a new size
 * replaces it whole */
struct orbx_sized {
  std::unique_ptr<orbx_plan> plan;
  int W = 0, H = 0;
  orbx::DevBuf<uint8_t> d_img;
  orbx::DevBuf<orbx_keypoint> d_kps;
  orbx::DevBuf<uint8_t> d_desc;
  orbx::DevBuf<int> d_count;
  /* pinned result staging: [count, error word | kps rows | desc rows] (64-B
   * header, kcap rows each), written by k_pack_results through d_res */
  orbx::PinnedBuf<uint8_t> h_res;
  uint8_t* d_res = nullptr;  /* not owned: h_res's device address */
  int last_k = 0; /* keypoints of the previous call */
  bool have_frame = false;
  orbx::PinnedBuf<uint8_t> h_img;  /* pinned staging of the caller's image (= host level 0) */
  orbx::PinnedBuf<uint8_t> h_pyr;  /* pinned host copy of the level buffer (PYRAMID_TO_HOST) */
  size_t pyr_bytes = 0;
  orbx::Stream s_copy; /* pyramid D2H, overlapped with FAST .. BRIEF */
  orbx::Event ev_pyr;
  bool host_pyr = false;     /* the last call filled h_img / h_pyr */
  std::unique_ptr<orbs_plan> stereo; /* orbx_stereo_match's plan, made on its first call */
};

struct orbx_extractor : orbx_sized {
  orbx_params params;
  int device = 0;
  int flags = 0;             /* ORBX_EXTRACTOR_* */
  long long n_calls = 0, n_refetch = 0; /* n_refetch: always 0 (k_pack_results writes exactly K rows) */
  void release_sized() {
    hipSetDevice(device);
    static_cast<orbx_sized&>(*this) = orbx_sized();
  }
  ~orbx_extractor() { hipSetDevice(device); }
};

#endif

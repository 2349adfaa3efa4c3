// projbuild_internal.h -- device table of the projection that feeds the
// projection matchers (Frame::isInFrustum, src/Frame.cc:249-305; the
// projections of ORBmatcher::SearchByProjection, src/ORBmatcher.cc:750-774,
// 832-848; MapPoint::PredictScale, src/MapPoint.cc:364-373), shared by
// kernels_projbuild.hip and api_projbuild.hip, and the host's threshold
// builder.
#ifndef ORBX_PROJBUILD_INTERNAL_H
#define ORBX_PROJBUILD_INTERNAL_H

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/orbx.h"

namespace orbx {

#define PB_BLOCK 256

// one problem: camera values, PredictScale thresholds, point arrays and
// outputs (device pointers).  Problem = blockIdx.y.
struct ProjBuildProblem {
  orbx_proj_camera cam;
  float thr[ORBX_PROJ_MAX_LEVELS];  // nlevels - 1 used
  orbx_proj_points pts;
  int npts;
  orbx_query_proj* q;
  int32_t* level;    // may be NULL
  float* view_cos;   // may be NULL
  int* n_in_view;    // may be NULL
  int* n_nonfinite;  // may be NULL
};

struct ProjBuildParams {
  float th, viewing_cos_limit;
  int level_rule;
};

// MapPoint::PredictScale from the ratio on, as MapPoint.cc.o has it: logf,
// vdivss, vroundss (ceil), vcvttss2si (NaN / out of range -> INT_MIN),
// min(.., nlevels - 1), max(0, ..)
inline int predict_scale_level_host(float ratio, float log_scale_factor, int nlevels) {
  const float c = ceilf(logf(ratio) / log_scale_factor);
  const int s = (c >= -2147483648.0f && c < 2147483648.0f) ? (int)c : INT32_MIN;
  const int m = s < nlevels - 1 ? s : nlevels - 1;
  return m > 0 ? m : 0;
}

inline bool predict_scale_args_ok(float log_scale_factor, int nlevels) {
  if (nlevels < 1 || nlevels > ORBX_PROJ_MAX_LEVELS) return false;
  if (!isfinite(log_scale_factor) || !(log_scale_factor > 0)) return false;
  return logf(FLT_MAX) / log_scale_factor < 2147483648.0f;
}

// thr[L] = the smallest positive float whose level exceeds L (bisection over
// the bit patterns: the level is monotone in the ratio), +inf where none does
inline void predict_scale_thresholds_host(float log_scale_factor, int nlevels, float* thr) {
  auto level_of = [&](uint32_t bits) {
    float r;
    memcpy(&r, &bits, 4);
    return predict_scale_level_host(r, log_scale_factor, nlevels);
  };
  for (int L = 0; L + 1 < nlevels; ++L) {
    uint32_t lo = 1u, hi = 0x7F7FFFFFu, out;
    if (level_of(hi) <= L) {
      out = 0x7F800000u;
    } else if (level_of(lo) > L) {
      out = lo;
    } else {
      while (hi - lo > 1) {  // level(lo) <= L < level(hi)
        const uint32_t mid = lo + (hi - lo) / 2;
        if (level_of(mid) > L) hi = mid;
        else lo = mid;
      }
      out = hi;
    }
    memcpy(&thr[L], &out, 4);
  }
}

// the threshold tables of the (log_scale_factor, nlevels) pairs a plan has
// met, each built on first use; 16 entries, cleared when full
struct PredictScaleCache {
  struct Entry {
    float lsf;
    int nlevels;
    float thr[ORBX_PROJ_MAX_LEVELS];
  };
  Entry entries[16];
  int n = 0;

  // a problem row's thr: the nlevels - 1 thresholds, zeros behind them.  lsf
  // is matched by bit pattern
  void fill(float lsf, int nlevels, float (&thr)[ORBX_PROJ_MAX_LEVELS]) {
    const Entry* hit = nullptr;
    for (int i = 0; i < n && !hit; ++i)
      if (entries[i].nlevels == nlevels && memcmp(&entries[i].lsf, &lsf, 4) == 0) hit = &entries[i];
    if (!hit) {
      if (n == 16) n = 0;
      Entry& e = entries[n++];
      e.lsf = lsf;
      e.nlevels = nlevels;
      predict_scale_thresholds_host(lsf, nlevels, e.thr);
      hit = &e;
    }
    memset(thr, 0, sizeof(thr));
    memcpy(thr, hit->thr, sizeof(float) * (size_t)(nlevels - 1));
  }
};

}  // namespace orbx

#endif

// kernels_projbuild.hip -- gfx950 kernel that builds the projection matchers'
// query rows from map points and a pose:
//   mode 1  Frame::isInFrustum (src/Frame.cc:249-305) + the radius and levels
//           of SearchByProjection(Frame&, vector<MapPoint*>&, th) (:26-28,67-69)
//   mode 2  the projection of SearchByProjection(Current, Last) (:756-774)
//   mode 3  the projection of SearchByProjection(Current, KeyFrame*) (:836-848)
//   MapPoint::PredictScale (src/MapPoint.cc:364-373) by threshold count
// One thread per (problem, point); point i writes row i, an inert row where
// the reference skips the point.  The library builds with -ffp-contract=off:
// a fused operation appears only where the reference's object has one, as
// __builtin_fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbx.h"
#include "projbuild_device.h"
#include "projbuild_internal.h"

namespace orbx {

__global__ __launch_bounds__(64) void k_proj_build_begin(const ProjBuildProblem* __restrict__ probs, int nprob) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= nprob) return;
  if (probs[p].n_in_view) *probs[p].n_in_view = 0;
  if (probs[p].n_nonfinite) *probs[p].n_nonfinite = 0;
}

__global__ __launch_bounds__(PB_BLOCK) void k_proj_build(const ProjBuildProblem* __restrict__ probs, int mode,
                                                         ProjBuildParams prm) {
  const ProjBuildProblem& PP = probs[blockIdx.y];
  const int npts = PP.npts;
  const int i = blockIdx.x * PB_BLOCK + threadIdx.x;
  if (blockIdx.x * PB_BLOCK >= npts) return;  // the whole block: uniform
  const orbx_proj_camera& C = PP.cam;
  const bool valid = i < npts;
  bool live = false, nonfinite = false;
  orbx_query_proj Q;
  Q.x = 0.0f;
  Q.y = 0.0f;
  Q.radius = -1.0f;
  Q.min_level = -1;
  Q.max_level = -1;
  Q.xr = 0.0f;
  Q.angle = 0.0f;
  int level = -1;
  float vcos = 0.0f;
  if (valid && !(PP.pts.skip && PP.pts.skip[i])) {
    const float* __restrict__ pos = PP.pts.pos + (size_t)i * 3;
    const float p0 = pos[0], p1 = pos[1], p2 = pos[2];
    const float X = pb_row(C.Rcw + 0, p0, p1, p2, C.tcw[0]);
    const float Y = pb_row(C.Rcw + 3, p0, p1, p2, C.tcw[1]);
    const float Z = pb_row(C.Rcw + 6, p0, p1, p2, C.tcw[2]);
    float u = 0.0f, v = 0.0f;
    if (mode == 1) {
      do {
        if (Z < 0.0f) break;  // Frame.cc:263 (PcZ == 0 passes)
        const float invz = 1.0f / Z;
        u = __builtin_fmaf(C.fx * X, invz, C.cx);  // :268-269, contracted
        v = __builtin_fmaf(C.fy * Y, invz, C.cy);
        if (u < C.min_x || u > C.max_x) break;
        if (v < C.min_y || v > C.max_y) break;
        const float o0 = p0 - C.ow[0], o1 = p1 - C.ow[1], o2 = p2 - C.ow[2];
        const float dist = pb_norm(o0, o1, o2);
        if (dist < PP.pts.min_dist_inv[i] || dist > PP.pts.max_dist_inv[i]) break;
        const float* __restrict__ nrm = PP.pts.normal + (size_t)i * 3;
        float vc = (float)(pb_dot(o0, o1, o2, nrm[0], nrm[1], nrm[2]) / (double)dist);
        if (vc != vc) vc = __uint_as_float(0xFFC00000u);  // 0 / 0 as x86 produces it
        if (vc < prm.viewing_cos_limit) break;
        level = pb_predict(PP.thr, C.nlevels, PP.pts.max_dist[i] / dist);
        // ORBmatcher.cc:27-28,67-69: viewCos > 0.998 and th != 1.0 in double
        const float r = ((double)vc > 0.998 ? 2.5f : 4.0f) * (prm.th != 1.0f ? prm.th : 1.0f);
        Q.radius = r * C.scale_factors[level];
        Q.min_level = level - 1;
        Q.max_level = level;
        Q.xr = __builtin_fmaf(-invz, C.mbf, u);  // :299, contracted
        vcos = vc;
        live = true;
      } while (0);
    } else if (mode == 2) {
      do {
        if (Z <= 0.0f) break;  // ORBmatcher.cc:758
        u = C.fx * X / Z + C.cx;  // :760-761: vmulss, vdivss, vaddss
        v = C.fy * Y / Z + C.cy;
        if (u < C.min_x || u > C.max_x || v < C.min_y || v > C.max_y) break;
        const int oct = PP.pts.octave[i];
        if (oct < 0 || oct >= C.nlevels) {  // the reference would index mvScaleFactors outside
          nonfinite = true;
          break;
        }
        level = oct;
        Q.radius = prm.th * C.scale_factors[oct];
        if (prm.level_rule == ORBX_LEVEL_RULE_FORWARD) {
          Q.min_level = oct;
          Q.max_level = -1;
        } else if (prm.level_rule == ORBX_LEVEL_RULE_BACKWARD) {
          Q.min_level = 0;
          Q.max_level = oct;
        } else {
          Q.min_level = oct - 1;
          Q.max_level = oct + 1;
        }
        Q.angle = PP.pts.angle[i];
        live = true;
      } while (0);
    } else {
      do {
        const float invz = 1.0f / Z;  // :838 (1.0 / z narrowed to vdivss); no depth test
        u = __builtin_fmaf(C.fx * X, invz, C.cx);  // :839-840: vmulss, vfmadd213ss
        v = __builtin_fmaf(C.fy * Y, invz, C.cy);
        if (u < C.min_x || u > C.max_x || v < C.min_y || v > C.max_y) break;
        const float dist = pb_norm(p0 - C.ow[0], p1 - C.ow[1], p2 - C.ow[2]);
        level = pb_predict(PP.thr, C.nlevels, PP.pts.max_dist[i] / dist);
        Q.radius = prm.th * C.scale_factors[level];
        Q.min_level = level - 1;
        Q.max_level = level + 1;
        Q.angle = PP.pts.angle[i];
        live = true;
      } while (0);
    }
    if (live && !(pb_finite(u) && pb_finite(v))) {  // the reference converts them to int
      live = false;
      nonfinite = true;
    }
    if (live) {
      Q.x = u;
      Q.y = v;
    } else {
      Q.radius = -1.0f;
      Q.min_level = -1;
      Q.max_level = -1;
      Q.xr = 0.0f;
      Q.angle = 0.0f;
      level = -1;
      vcos = 0.0f;
    }
  }
  if (valid) {
    PP.q[i] = Q;
    if (PP.level) PP.level[i] = level;
    if (mode == 1 && PP.view_cos) PP.view_cos[i] = vcos;
  }
  const int nl = __popcll(__ballot(live)), nn = __popcll(__ballot(nonfinite));
  if ((threadIdx.x & 63) == 0) {
    if (nl && PP.n_in_view) atomicAdd(PP.n_in_view, nl);
    if (nn && PP.n_nonfinite) atomicAdd(PP.n_nonfinite, nn);
  }
}

}  // namespace orbx

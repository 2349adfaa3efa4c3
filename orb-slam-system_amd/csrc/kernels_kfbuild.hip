// kernels_kfbuild.hip -- gfx950 kernel that builds the keyframe window search's
// query rows from map points and a pose:
//   ORBX_KF_FORM_FUSE  the projection of ORBmatcher::Fuse(KeyFrame*, vector&, th)
//                      and Fuse(KeyFrame*, Scw, ..) (src/ORBmatcher.cc:514-531,
//                      :582-599)
//   ORBX_KF_FORM_SIM3  the projection of SearchBySim3 (:676-694)
//   KeyFrame::IsInImage (src/KeyFrame.cc:590-593) and MapPoint::PredictScale
//   (src/MapPoint.cc:353-362, the KeyFrame* overload) by threshold count
// One thread per (problem, point); point i writes row i, an inert row where
// the reference skips the point.  The library builds with -ffp-contract=off:
// a fused operation appears only where the reference's object has one, as
// __builtin_fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbx.h"
#include "kfbuild_internal.h"
#include "projbuild_device.h"

namespace orbx {

__global__ __launch_bounds__(64) void k_kf_build_begin(const KfBuildProblem* __restrict__ probs, int nprob) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= nprob) return;
  if (probs[p].n_live) *probs[p].n_live = 0;
  if (probs[p].n_nonfinite) *probs[p].n_nonfinite = 0;
}

__global__ __launch_bounds__(KB_BLOCK) void k_kf_build(const KfBuildProblem* __restrict__ probs, int form, float th) {
  const KfBuildProblem& PP = probs[blockIdx.y];
  const int npts = PP.npts;
  const int i = blockIdx.x * KB_BLOCK + threadIdx.x;
  if (blockIdx.x * KB_BLOCK >= npts) return;  // the whole block: uniform
  const orbx_kf_camera& C = PP.cam;
  const bool valid = i < npts;
  bool live = false, nonfinite = false;
  orbx_kf_query Q;
  Q.x = 0.0f;
  Q.y = 0.0f;
  Q.radius = -1.0f;
  Q.level = -1;
  Q.desc = PP.desc_base + i;
  if (valid && !(PP.pts.skip && PP.pts.skip[i])) {
    const float* __restrict__ pos = PP.pts.pos + (size_t)i * 3;
    const float p0 = pos[0], p1 = pos[1], p2 = pos[2];
    float X = pb_row(C.Rcw + 0, p0, p1, p2, C.tcw[0]);
    float Y = pb_row(C.Rcw + 3, p0, p1, p2, C.tcw[1]);
    float Z = pb_row(C.Rcw + 6, p0, p1, p2, C.tcw[2]);
    if (form == ORBX_KF_FORM_SIM3) {  // p3Dc2 = sR21 * p3Dc1 + t21 (:678)
      const float a = X, b = Y, c = Z;
      X = pb_row(C.sR21 + 0, a, b, c, C.t21[0]);
      Y = pb_row(C.sR21 + 3, a, b, c, C.t21[1]);
      Z = pb_row(C.sR21 + 6, a, b, c, C.t21[2]);
    }
    do {
      if (Z < 0.0f) break;  // :517 (Z == +-0 passes and fails IsInImage below)
      const float invz = 1.0f / Z;  // :519 (1.0 / z narrowed to vdivss)
      const float x = X * invz, y = Y * invz;
      const float u = __builtin_fmaf(x, C.fx, C.cx);  // :522-523: vfmadd132ss
      const float v = __builtin_fmaf(y, C.fy, C.cy);
      if (!(u >= C.min_x && u < C.max_x && v >= C.min_y && v < C.max_y)) break;  // KeyFrame.cc:592
      const float dist = form == ORBX_KF_FORM_SIM3 ? pb_norm(X, Y, Z)  // :690
                                                   : pb_norm(p0 - C.ow[0], p1 - C.ow[1], p2 - C.ow[2]);  // :527
      if (dist < PP.pts.min_dist_inv[i] || dist > PP.pts.max_dist_inv[i]) break;
      const int lv = pb_predict(PP.thr, C.nlevels, PP.pts.max_dist[i] / dist);
      const float radius = th * C.scale_factors[lv];
      if (!pb_finite(radius)) {
        nonfinite = true;
        break;
      }
      Q.x = u;
      Q.y = v;
      Q.radius = radius;
      Q.level = lv;
      live = true;
    } while (0);
  }
  if (valid) {
    PP.q[i] = Q;
    if (PP.level) PP.level[i] = Q.level;
  }
  const int nl = __popcll(__ballot(live)), nn = __popcll(__ballot(nonfinite));
  if ((threadIdx.x & 63) == 0) {
    if (nl && PP.n_live) atomicAdd(PP.n_live, nl);
    if (nn && PP.n_nonfinite) atomicAdd(PP.n_nonfinite, nn);
  }
}

}  // namespace orbx

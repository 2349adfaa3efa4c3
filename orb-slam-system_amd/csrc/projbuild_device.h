// projbuild_device.h -- the device arithmetic the query-building kernels share
// (kernels_projbuild.hip; kernels_kfbuild.hip, §18): a row of
// cv::Mat R * P + t, cv::norm of a 3-vector and MapPoint::PredictScale by
// threshold count.  The library builds with -ffp-contract=off; nothing here
// fuses.
#ifndef ORBX_PROJBUILD_DEVICE_H
#define ORBX_PROJBUILD_DEVICE_H

#include <hip/hip_runtime.h>

namespace orbx {

// one row of cv::Mat Rcw * P + tcw (OpenCV 3.4 without FMA: the products
// summed left to right in binary32, then the addition)
__device__ __forceinline__ float pb_row(const float* __restrict__ r, float p0, float p1, float p2, float t) {
  float s = r[0] * p0;
  s = s + r[1] * p1;
  s = s + r[2] * p2;
  return s + t;
}

// cv::Mat::dot / cv::norm's sum of a 3-vector: sequential in double
__device__ __forceinline__ double pb_dot(float a0, float a1, float a2, float b0, float b1, float b2) {
  double s = (double)a0 * (double)b0;
  s = s + (double)a1 * (double)b1;
  s = s + (double)a2 * (double)b2;
  return s;
}

// Correctly rounded double square root, whatever the rounding of the device
// library's sqrt() (taken as within one ulp; the library declares
// __ocml_sqrt_rte_f64 but ships no body for it).  For adjacent doubles c < d
// the root lies below their midpoint iff s <= c * d: s - c * d is a multiple
// of (d - c)^2 and the midpoint's square exceeds c * d by a quarter of that,
// and the sign of s - c * d is exact in one fma.  s > 0 finite and far from
// the subnormals here (a sum of squares of binary32 values).
__device__ __forceinline__ double pb_sqrt_rn(double s) {
  const double y = sqrt(s);
  if (!(s > 0.0) || !(s < __builtin_inf())) return y;
  const double ym = __longlong_as_double(__double_as_longlong(y) - 1);
  const double yp = __longlong_as_double(__double_as_longlong(y) + 1);
  if (__builtin_fma(ym, y, -s) >= 0.0) return ym;
  if (__builtin_fma(y, yp, -s) >= 0.0) return y;
  return yp;
}

__device__ __forceinline__ float pb_norm(float a0, float a1, float a2) {
  return (float)pb_sqrt_rn(pb_dot(a0, a1, a2, a0, a1, a2));
}

// MapPoint::PredictScale: the number of thresholds a finite ratio reaches;
// 0 for NaN, +-inf, zero and negative ratios (thr > 0)
__device__ __forceinline__ int pb_predict(const float* __restrict__ thr, int nlevels, float ratio) {
  int level = 0;
  if (ratio < __builtin_inff())
    for (int L = 0; L + 1 < nlevels; ++L) level += ratio >= thr[L] ? 1 : 0;
  return level;
}

__device__ __forceinline__ bool pb_finite(float v) { return fabsf(v) < __builtin_inff(); }

}  // namespace orbx

#endif

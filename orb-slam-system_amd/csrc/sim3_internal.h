// sim3_internal.h -- shared by kernels_sim3.hip and api_sim3.hip (DESIGN.md
// §22): the device problem table and the kernel.
#ifndef ORBX_SIM3_INTERNAL_H
#define ORBX_SIM3_INTERNAL_H

#include <hip/hip_runtime.h>

#include "../../include/orbx.h"
#include "sim3_math.h"

namespace orbx {

constexpr int S3_MAXN = 8192;   // correspondences per problem
constexpr int S3_MAXIT = 4096;  // hypotheses per problem and call
constexpr int S3_T = 256;       // lanes of the workgroup: one problem per workgroup
constexpr int S3_TF = 24;       // floats of (T12, T21) as CheckInliers reads them: sR12 t12 sR21 t21

// the constructor's values of one correspondence, read as three 16-byte words
struct alignas(16) S3Rec {
  s3_corr c;
};
static_assert(sizeof(S3Rec) == 48, "S3Rec layout");
static_assert(sizeof(s3_hyp) == S3_HYP * sizeof(float), "s3_hyp layout");

struct S3Problem {
  const float* pos1;       // [ncorr][3]
  const float* pos2;
  const float* sigma2_1;   // [ncorr]
  const float* sigma2_2;
  const int32_t* triples;  // [nit][3], checked on the host
  S3Rec* corr;             // [ncorr] scratch
  float* hyp;              // [S3_HYP][nit] scratch, element-major
  uint8_t* inl;            // [ncorr]
  orbx_sim3_result* res;
  float pose[24];          // Rcw1 tcw1 Rcw2 tcw2
  float cams[8];           // fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2
  int ncorr, nit;          // nit = 0 for an inert problem
  int min_inliers, fix_scale, best_in;
};

// the one launch of a call on stream s (kernels_sim3.hip); nprob >= 1
void launch_sim3(const S3Problem* d_probs, int nprob, hipStream_t s);

}  // namespace orbx

#endif

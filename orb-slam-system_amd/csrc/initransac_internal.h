// initransac_internal.h -- shared by kernels_initransac.hip and
// api_initransac.hip: the device problem table and the kernels.
#ifndef ORBX_INITRANSAC_INTERNAL_H
#define ORBX_INITRANSAC_INTERNAL_H

#include <hip/hip_runtime.h>

#include "../../include/orbx.h"
#include "initransac_math.h"

namespace orbx {

constexpr int IR_MAXN = 8192;    // keys per frame
constexpr int IR_MAXIT = 4096;   // hypotheses per model
constexpr int IR_W = 64;         // hypotheses per workgroup: one per lane of one wavefront
constexpr int IR_SELECT_T = 256; // lanes of the select kernel
constexpr int IR_SCORE_T = 512;  // lanes of the score kernel: IR_SCORE_SUB wavefronts over the same 64 hypotheses
constexpr int IR_SCORE_SUB = IR_SCORE_T / IR_W;
constexpr int IR_TILE = 32;      // matches per tile of the score kernel (a multiple of IR_SCORE_SUB)
constexpr int IR_HYP = 27;       // floats per iteration: H21i, H12i, F21i

// one entry of mvMatches12: the two keys' pt (mvKeys1 / mvKeys2), or their
// normalised points (vPn1 / vPn2)
struct alignas(16) IrRec {
  float u1, v1, u2, v2;
};

struct IrProblem {
  const IrRec* rec;     // [nmatch] image coordinates, match-list order
  const IrRec* recn;    // [nmatch] normalised
  const int32_t* sets;  // [nit][8] indices into the match list (checked on the host)
  float* hyp;           // [IR_HYP][nit]: element-major, so that a wavefront's lanes read neighbours
  float* score;         // [2][nit]: H, F
  uint8_t* inl_H;       // [nmatch]
  uint8_t* inl_F;
  orbx_ransac_result* res;
  int nmatch;
  float T1[9], T2inv[9], T2t[9];
};

// the four launches of one call on stream s (kernels_initransac.hip): the
// hypotheses of both models, their scores, then the winners, flags and RH.
// npair >= 1; nit == 0 launches the last only
void launch_initransac(const IrProblem* d_probs, int npair, int nit, float inv_sigma2, hipStream_t s);

}  // namespace orbx

#endif

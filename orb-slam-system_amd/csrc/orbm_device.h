// orbm_device.h -- device helpers shared by the kernels of the ORBmatcher
// family (kernels_match / tri / proj / bow / kfwin / stereo / misc): the
// 256-bit DescriptorDistance (src/ORBmatcher.cc:896-908) in its two spellings
// and ComputeThreeMaxima (:469-502).
//
// Not shared on purpose: the rotation-bin arithmetic.  kernels_match wraps
// bin == 30 to 0, kernels_tri takes % 30 and drops out-of-range bins,
// kernels_proj takes % 30 -- each mirrors a different function of the reference.
#ifndef ORBX_ORBM_DEVICE_H
#define ORBX_ORBM_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_internal.h"

namespace orbx {

// __popc spelling: the compiler's add3 trees.  Which spelling a site uses was
// measured per site; ham256 below is the other one.
__device__ __forceinline__ int ham256_popc(uint4 a0, uint4 a1, uint4 b0, uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
// (b0, b1 by reference: by value, the copies shifted the register allocation
// of k_match_resolve, whose loads used to sit inside the helper)
__device__ __forceinline__ int ham256_popc(const uint32_t d1[8], const uint4& b0, const uint4& b1) {
  return __popc(d1[0] ^ b0.x) + __popc(d1[1] ^ b0.y) + __popc(d1[2] ^ b0.z) + __popc(d1[3] ^ b0.w) +
         __popc(d1[4] ^ b1.x) + __popc(d1[5] ^ b1.y) + __popc(d1[6] ^ b1.z) + __popc(d1[7] ^ b1.w);
}
// two descriptor rows (32 bytes each, 32-byte aligned)
__device__ __forceinline__ int ham256_popc(const void* a, const void* b) {
  const uint4* pa = reinterpret_cast<const uint4*>(a);
  const uint4* pb = reinterpret_cast<const uint4*>(b);
  return ham256_popc(pa[0], pa[1], pb[0], pb[1]);
}

// 256-bit Hamming distance as one accumulate chain: v_bcnt_u32_b32 adds its
// second operand, so 8 xor + 8 bcnt (the compiler's add3 trees cost 3 more)
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}
// V: uint4 or an ext_vector_type(4) of uint32_t (both have .x .. .w)
template <typename V>
__device__ __forceinline__ uint32_t ham256(uint4 a0, uint4 a1, V b0, V b1) {
  uint32_t d = bcnt_acc(a0.x ^ b0.x, 0u);
  d = bcnt_acc(a0.y ^ b0.y, d);
  d = bcnt_acc(a0.z ^ b0.z, d);
  d = bcnt_acc(a0.w ^ b0.w, d);
  d = bcnt_acc(a1.x ^ b1.x, d);
  d = bcnt_acc(a1.y ^ b1.y, d);
  d = bcnt_acc(a1.z ^ b1.z, d);
  return bcnt_acc(a1.w ^ b1.w, d);
}

// ComputeThreeMaxima (ORBmatcher.cc:469-502) over the ORBM_HISTO bins of
// hist, one thread: ind = the three fullest bins, -1 for one below a tenth of
// the fullest (or never filled).  k_match_finalize and k_tri_finalize call
// it from one thread; k_proj_resolve keeps its own register-only ladder
// (this body's indexed ti / tv arrays live in scratch)
__device__ __forceinline__ void three_maxima(const int* hist, int ind[3]) {
  int ti[3] = {-1, -1, -1}, tv[3] = {0, 0, 0};
  int hv[ORBM_HISTO];  // every bin read up front (independent loads)
#pragma unroll
  for (int i = 0; i < ORBM_HISTO; ++i) hv[i] = hist[i];
#pragma unroll
  for (int i = 0; i < ORBM_HISTO; ++i) {
    const int v = hv[i];
    for (int jj = 0; jj < 3; ++jj) {
      if (v > tv[jj]) {
        for (int k = 2; k > jj; --k) { tv[k] = tv[k - 1]; ti[k] = ti[k - 1]; }
        tv[jj] = v;
        ti[jj] = i;
        break;
      }
    }
  }
  if (tv[1] < 0.1f * tv[0]) { ti[1] = -1; ti[2] = -1; }
  else if (tv[2] < 0.1f * tv[0]) { ti[2] = -1; }
  ind[0] = ti[0]; ind[1] = ti[1]; ind[2] = ti[2];
}

// bit b set iff bin b is one of ind
__device__ __forceinline__ uint32_t kept_bins_mask(const int ind[3]) {
  return (ind[0] >= 0 ? 1u << ind[0] : 0u) | (ind[1] >= 0 ? 1u << ind[1] : 0u) |
         (ind[2] >= 0 ? 1u << ind[2] : 0u);
}

}  // namespace orbx

#endif

// api_misc.hip -- C ABI of SURVEY.md §8f rank 4: distinctive descriptors and
// keypoint undistortion.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/orbx.h"
#include "call_arena.h"

namespace orbx {
struct UndistortArgs {
  double fx, fy, cx, cy, ifx, ify;
  double k[14];
};
__global__ void k_distinctive(const uint8_t*, const int32_t*, int, int32_t*);
__global__ void k_undistort(const orbx_keypoint*, int, const UndistortArgs, orbx_keypoint*);
__global__ void k_boundary_copy(const uint8_t*, size_t, const uint8_t*, size_t, const uint8_t*, size_t,
                                uint8_t*, int, uint8_t*, uint8_t*, uint8_t*);
}  // namespace orbx

using namespace orbx;

static int select_device(int device) {
  if (check_device(device)) return ORBX_ERR_NO_DEVICE;
  return hipSetDevice(device) == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
}

extern "C" int orbm_compute_distinctive_descriptors(const uint8_t* desc, const int32_t* off,
                                                    int nmp, int device, int32_t* best) {
  if (nmp < 0 || (nmp > 0 && (!off || !best))) return ORBX_ERR_ARG;
  if (nmp == 0) return ORBX_OK;
  const int total = off[nmp];
  if (off[0] != 0 || total < 0 || (total > 0 && !desc)) return ORBX_ERR_ARG;
  for (int m = 0; m < nmp; ++m)
    if (off[m + 1] < off[m] || off[m + 1] - off[m] > (1 << 20)) return ORBX_ERR_ARG;
  int rc = select_device(device);
  if (rc) return rc;
  CallArena A(device);
  if (!A.ok()) return ORBX_ERR_HIP;
  const auto s_desc = A.in(desc, (size_t)total * 32);
  const auto s_off = A.in(off, (size_t)nmp + 1);
  const auto s_best = A.out(best, (size_t)nmp);
  rc = A.commit();
  if (rc) return rc;
  if (A.upload()) return ORBX_ERR_HIP;
  hipLaunchKernelGGL(k_distinctive, dim3((nmp + 3) / 4), dim3(256), 0, A.stream(), A.d(s_desc),
                     A.d(s_off), nmp, A.d(s_best));
  return A.finish();
}

extern "C" int orbx_undistort_keypoints(const orbx_keypoint* kps, int n, const float* K,
                                        const float* dist, int ndist, int device,
                                        orbx_keypoint* out) {
  if (n < 0 || !K || (ndist > 0 && !dist) || ndist < 0 || ndist > 14 || (n > 0 && (!kps || !out)))
    return ORBX_ERR_ARG;
  if (n == 0) return ORBX_OK;
  if (ndist == 0 || dist[0] == 0.0f) { /* mvKeysUn = mvKeys (:386-390) */
    memmove(out, kps, n * sizeof(orbx_keypoint));
    return ORBX_OK;
  }
  /* tauX, tauY: cvUndistortPointsInternal applies the inverse tilt matrix when
   * either is non-zero; that is not restated here */
  for (int j = 12; j < ndist; ++j)
    if (dist[j] != 0.0f) return ORBX_ERR_UNSUPPORTED;
  int rc = select_device(device);
  if (rc) return rc;
  UndistortArgs A;
  memset(&A, 0, sizeof(A));
  A.fx = K[0];
  A.fy = K[4];
  A.cx = K[2];
  A.cy = K[5];
  A.ifx = 1. / A.fx;
  A.ify = 1. / A.fy;
  for (int j = 0; j < ndist; ++j) A.k[j] = dist[j];
  CallArena ar(device);
  if (!ar.ok()) return ORBX_ERR_HIP;
  const auto s_in = ar.in(kps, (size_t)n);
  const auto s_out = ar.out(out, (size_t)n);
  rc = ar.commit();
  if (rc) return rc;
  if (ar.upload()) return ORBX_ERR_HIP;
  hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, ar.stream(), ar.d(s_in), n, A,
                     ar.d(s_out));
  return ar.finish();
}

extern "C" size_t orbx_boundary_record_bytes(int kcap) {
  return kcap > 0 ? (size_t)kcap * (sizeof(orbx_keypoint) + 32) + 16 : 0;
}

static int boundary_copy(int kcap, const void* a, const void* b, const void* c, void* rec, int unpack,
                         void* oa, void* ob, void* oc, void* stream) {
  if (kcap < 1) return ORBX_ERR_ARG;
  const size_t na = (size_t)kcap * sizeof(orbx_keypoint), nb = (size_t)kcap * 32, nc = 4;
  const size_t n = na + nb + nc;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 4095) / 4096, 1024);
  hipLaunchKernelGGL(k_boundary_copy, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)a, na, (const uint8_t*)b, nb, (const uint8_t*)c, nc,
                     (uint8_t*)rec, unpack, (uint8_t*)oa, (uint8_t*)ob, (uint8_t*)oc);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_HIP;
}

extern "C" int orbx_boundary_pack(const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                  const int* d_count, int kcap, uint8_t* d_record, void* stream) {
  if (!d_kps || !d_desc || !d_count || !d_record) return ORBX_ERR_ARG;
  return boundary_copy(kcap, d_kps, d_desc, d_count, d_record, 0, nullptr, nullptr, nullptr, stream);
}

extern "C" int orbx_boundary_unpack(const uint8_t* d_record, int kcap, orbx_keypoint* d_kps,
                                    uint8_t* d_desc, int* d_count, void* stream) {
  if (!d_kps || !d_desc || !d_count || !d_record) return ORBX_ERR_ARG;
  return boundary_copy(kcap, d_record, nullptr, nullptr, nullptr, 1, d_kps, d_desc, d_count, stream);
}

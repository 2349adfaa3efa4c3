// kernels_poseopt.hip -- Optimizer::PoseOptimization on the device (DESIGN.md
// §19): one workgroup of PO_T lanes per problem runs the whole four-round
// procedure.  Lanes stride over the feature slots in f64 (poseopt_math.h, the
// arithmetic the CPU restatement shares); the PO_NSUM partial sums are reduced
// through LDS in the documented order; lane 0 solves the 6x6 system in LDS;
// every lane then forms exp(x) * estimate for itself, so all control flow is
// uniform across the workgroup and every barrier is reached by all lanes.
#include <hip/hip_runtime.h>

#include "poseopt_internal.h"

namespace orbx {

namespace {

struct PoLds {
  double part[PO_NSUM * PO_T];
  double work[42];
  double x[6];
  int ok;
  int cnt[3];
};
static_assert(sizeof(PoLds) <= (size_t)PO_LDS_BYTES, "PO_LDS_BYTES");

// feature i's edge; false where it has none (no point, or a bad octave / index,
// which *invalid reports)
__device__ inline bool load_edge(const orbx_pose_problem& P, int i, po_edge* e, bool* invalid) {
  const orbx_pose_obs& O = P.obs;
  *invalid = false;
  int idx = i;
  if (O.point_index) {
    idx = O.point_index[i];
    if (idx < -1 || idx >= O.npos) {
      *invalid = true;
      return false;
    }
    if (idx < 0) return false;
  } else {
    if (O.has_point && O.has_point[i] == 0) return false;
    if (idx >= O.npos) {
      *invalid = true;
      return false;
    }
  }
  const orbx_keypoint k = O.keys[i];
  if (k.octave < 0 || k.octave >= P.camera.nlevels) {
    *invalid = true;
    return false;
  }
  const float ur = O.uright ? O.uright[i] : -1.0f;
  e->stereo = !(ur < 0);
  e->obs[0] = (double)k.x;
  e->obs[1] = (double)k.y;
  e->obs[2] = (double)ur;
  e->w = (double)P.camera.inv_level_sigma2[k.octave];
  const float* X = O.pos + 3 * (size_t)idx;
  e->X[0] = (double)X[0];
  e->X[1] = (double)X[1];
  e->X[2] = (double)X[2];
  return true;
}

// the halving tree over the PO_T partial sums of K quantities, part[k][t] =
// acc[k] of lane t; every lane returns with out[k] = the total.  Uniform.
template <int K>
__device__ inline void reduce(PoLds& L, const double* acc, double* out) {
  const int t = (int)threadIdx.x;
  __syncthreads();  // the previous reduction's totals have been read
#pragma unroll
  for (int k = 0; k < K; ++k) L.part[k * PO_T + t] = acc[k];
  __syncthreads();
  for (int s = PO_T / 2; s >= 1; s >>= 1) {
    for (int w = t; w < K * s; w += PO_T) {
      const int k = w / s, j = w - k * s;
      L.part[k * PO_T + j] = L.part[k * PO_T + j] + L.part[k * PO_T + j + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = L.part[k * PO_T];
}

struct Huber {
  double delta_mono, delta_stereo;
  float dsqr_mono, dsqr_stereo;
};

}  // namespace

__global__ __launch_bounds__(PO_T) void k_pose_optimize(const orbx_pose_problem* probs) {
  __shared__ PoLds L;
  const orbx_pose_problem& P = probs[blockIdx.x];
  const int t = (int)threadIdx.x;
  const int n = P.obs.n;
  uint8_t* outlier = P.outlier;

  if (t < 3) L.cnt[t] = 0;
  if (t < 6) L.x[t] = 0.0;
  __syncthreads();
  // the edge set (Optimizer.cc:261-341): flags cleared, correspondences counted
  int mine = 0, bad = 0;
  for (int i = t; i < n; i += PO_T) {
    po_edge e;
    bool invalid;
    mine += load_edge(P, i, &e, &invalid) ? 1 : 0;
    bad += invalid ? 1 : 0;
    outlier[i] = 0;
  }
  if (mine) atomicAdd(&L.cnt[0], mine);
  if (bad) atomicAdd(&L.cnt[1], bad);
  __syncthreads();
  const int ninit = L.cnt[0];
  if (t == 0) *P.status = L.cnt[1];
  if (ninit < 3) {  // :345-346
    if (t < 16) P.Tcw_out[t] = t < 12 ? P.camera.Tcw[t] : (t == 15 ? 1.0f : 0.0f);
    if (t == 0) *P.ninliers = 0;
    return;
  }

  po_cam K;
  K.fx = (double)P.camera.fx;
  K.fy = (double)P.camera.fy;
  K.cx = (double)P.camera.cx;
  K.cy = (double)P.camera.cy;
  K.bf = (double)P.camera.mbf;
  Huber hub;
  {
    const float dm = (float)sqrt(5.991), ds = (float)sqrt(7.815);  // :254-255
    hub.delta_mono = (double)dm;
    hub.delta_stereo = (double)ds;
    hub.dsqr_mono = (float)(hub.delta_mono * hub.delta_mono);
    hub.dsqr_stereo = (float)(hub.delta_stereo * hub.delta_stereo);
  }
  const float chi2Mono = 5.991, chi2Stereo = 7.815;

  po_pose pose0, est, err_pose;
  po_from_tcw(P.camera.Tcw, &pose0);
  est = pose0;
  int robust = 1, nBad = 0;

  for (int it = 0; it < 4; ++it) {
    est = pose0;  // :358
    err_pose = est;
    if (ninit - nBad > 0) {
      // SparseOptimizer::optimize(10) over OptimizationAlgorithmLevenberg::solve
      double lambda = 0.0, ni = 2.0;
      int nbadlm = 0;
      for (int iteration = 0; iteration < 10; ++iteration) {
        double S[PO_NSUM];
        {
          double acc[PO_NSUM];
#pragma unroll
          for (int k = 0; k < PO_NSUM; ++k) acc[k] = 0.0;
          for (int i = t; i < n; i += PO_T) {
            po_edge e;
            bool invalid;
            if (!load_edge(P, i, &e, &invalid) || outlier[i]) continue;
            po_edge_accumulate(&K, &est, &e, robust, e.stereo ? hub.delta_stereo : hub.delta_mono,
                               e.stereo ? hub.dsqr_stereo : hub.dsqr_mono, acc);
          }
          reduce<PO_NSUM>(L, acc, S);
        }
        err_pose = est;
        double currentChi = S[27];
        double tempChi = currentChi;
        const double iniChi = currentChi;
        if (iteration == 0) {  // computeLambdaInit, _tau = 1e-5
          double maxDiagonal = 0.;
          const double dg[6] = {S[0], S[6], S[11], S[15], S[18], S[20]};
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            const double a = dg[j] < 0 ? -dg[j] : dg[j];
            maxDiagonal = (a < maxDiagonal) ? maxDiagonal : a;
          }
          lambda = 1e-5 * maxDiagonal;
          ni = 2;
          nbadlm = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
          const po_pose backup = est;
          // lane 0 solves (H + lambda I) x = b in LDS; a failed solve leaves x as it was
          if (t == 0) {
            double T0[PO_NSUM];
#pragma unroll
            for (int k = 0; k < PO_NSUM; ++k) T0[k] = S[k];
            L.ok = po_solve(T0, lambda, L.work, L.x);
          }
          __syncthreads();
          const int ok2 = L.ok;
          double x[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) x[j] = L.x[j];
          po_pose dT, trial;
          po_exp(x, &dT);
          po_mul(&dT, &est, &trial);
          est = trial;
          {
            double a = 0.0, tot;
            for (int i = t; i < n; i += PO_T) {
              po_edge e;
              bool invalid;
              if (!load_edge(P, i, &e, &invalid) || outlier[i]) continue;
              a = a + po_edge_robust_chi2(&K, &est, &e, robust, e.stereo ? hub.delta_stereo : hub.delta_mono,
                                          e.stereo ? hub.dsqr_stereo : hub.dsqr_mono);
            }
            reduce<1>(L, &a, &tot);
            tempChi = tot;
          }
          err_pose = est;
          if (!ok2) tempChi = PO_DBL_MAX;
          rho = (currentChi - tempChi);
          double scale = 0.;
#pragma unroll
          for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + (-S[21 + j]));
          scale += 1e-3;
          rho /= scale;
          if (rho > 0 && tempChi - tempChi == 0) {
            const double c = 2 * rho - 1;
            double alpha = 1. - c * c * c;
            alpha = (2. / 3. < alpha) ? 2. / 3. : alpha;
            const double scaleFactor = (1. / 3. < alpha) ? alpha : 1. / 3.;
            lambda *= scaleFactor;
            ni = 2;
            currentChi = tempChi;
          } else {
            lambda *= ni;
            ni *= 2;
            est = backup;
          }
          qmax++;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi)
          nbadlm++;
        else
          nbadlm = 0;
        if (nbadlm >= 3) break;
      }
    }
    // :363-419: each lane classifies its own slots, so the flags need no fence
    if (t == 0) L.cnt[2] = 0;
    __syncthreads();
    int nb = 0;
    for (int i = t; i < n; i += PO_T) {
      po_edge e;
      bool invalid;
      if (!load_edge(P, i, &e, &invalid)) continue;
      const float chi2 = (float)po_edge_chi2(&K, outlier[i] ? &est : &err_pose, &e);
      const bool out = chi2 > (e.stereo ? chi2Stereo : chi2Mono);
      outlier[i] = out ? 1 : 0;
      nb += out ? 1 : 0;
    }
    if (nb) atomicAdd(&L.cnt[2], nb);
    __syncthreads();
    nBad = L.cnt[2];
    __syncthreads();
    if (it == 2) robust = 0;
    if (ninit < 10) break;
  }
  if (t == 0) {
    float M[16];
    po_to_tcw(&est, M);
#pragma unroll
    for (int i = 0; i < 16; ++i) P.Tcw_out[i] = M[i];
    *P.ninliers = ninit - nBad;
  }
}

}  // namespace orbx

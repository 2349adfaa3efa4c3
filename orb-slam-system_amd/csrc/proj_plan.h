// proj_plan.h -- the batched projection matcher's handle (orbm_proj_plan),
// shared by api_proj.hip (create / destroy / search) and api_projbuild.hip
// (project / track).  Host only.
#ifndef ORBX_PROJ_PLAN_H
#define ORBX_PROJ_PLAN_H

#include <vector>

#include "api_common.h"
#include "proj_internal.h"
#include "projbuild_internal.h"

// PredictScale thresholds of one (log_scale_factor, nlevels), kept per plan
struct ProjThrEntry {
  float lsf;
  int nlevels;
  float thr[ORBX_PROJ_MAX_LEVELS];
};

struct orbm_proj_plan {
  int device = 0, max_prob = 0, max_n = 0, max_nq = 0;
  orbx::DevBuf<orbx::ProjProblem> d_probs;
  orbx::PinnedBuf<orbx::ProjProblem> h_probs;  // pinned staging of the problem table
  orbx::Event ev;                              // the last table upload (h_probs reusable after it)
  orbx::Event ev_done;                         // the last call's kernels (its grid / candidate scratch free after it)
  orbx::DevBuf<int> d_cell_off, d_cell_feat;
  orbx::DevBuf<uint32_t> d_cand;
  orbx::DevBuf<int> d_ncand;
  // project / track (allocated by their first call): the projection's problem
  // table with its staging, and the query rows of a track call that names none
  orbx::DevBuf<orbx::ProjBuildProblem> d_bprobs;
  orbx::PinnedBuf<orbx::ProjBuildProblem> h_bprobs;
  orbx::DevBuf<orbx_query_proj> d_q;
  std::vector<ProjThrEntry> thr_cache;
  ~orbm_proj_plan() { hipSetDevice(device); }
};

namespace orbx {
// api_proj.hip: grid, candidates and walk of nprob problems
void launch_proj(const ProjProblem* d_probs, int nprob, int max_n, int max_nq, int mode, float nnratio,
                 int th_dist, int check_ori, hipStream_t s);
ProjFrame proj_frame(const orbx_proj_frame* F);
}  // namespace orbx

#endif

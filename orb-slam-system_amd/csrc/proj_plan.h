// proj_plan.h -- the batched projection matcher's handle (orbm_proj_plan),
// shared by api_proj.hip (create / destroy / search) and api_projbuild.hip
// (project / track).  Host only.
#ifndef ORBX_PROJ_PLAN_H
#define ORBX_PROJ_PLAN_H

#include <algorithm>

#include "plan_table.h"
#include "proj_internal.h"
#include "projbuild_internal.h"

struct orbm_proj_plan {
  int device = 0, max_prob = 0, max_n = 0, max_nq = 0;
  orbx::PlanTable<orbx::ProjProblem> probs;  // the search's problem table
  orbx::PlanFence fence;
  orbx::DevBuf<int> d_cell_off, d_cell_feat;  // per problem: PG_CELLS + 1, max_n
  orbx::DevBuf<uint32_t> d_cand;              // per problem: max(max_nq, 1) x PJ_T
  orbx::DevBuf<int> d_ncand;                  // per problem: max(max_nq, 1)
  // project / track (allocated by their first call): the projection's problem
  // table, and the query rows of a track call that names none
  orbx::PlanTable<orbx::ProjBuildProblem> bprobs;
  orbx::DevBuf<orbx_query_proj> d_q;
  orbx::PredictScaleCache thr_cache;
  ~orbm_proj_plan() { hipSetDevice(device); }
};

namespace orbx {
// api_proj.hip: grid, candidates and walk of nprob problems
void launch_proj(const ProjProblem* d_probs, int nprob, int max_n, int max_nq, int mode, float nnratio,
                 int th_dist, int check_ori, hipStream_t s);
ProjFrame proj_frame(const orbx_proj_frame* F);

// a plan problem's frame: at most max_n keypoints, with their arrays
inline bool frame_ok(const orbx_proj_frame& F, int max_n) {
  return F.n >= 0 && F.n <= max_n && (F.n == 0 || (F.keys && F.desc));
}

// row i of the plan's search table: frame F matched against the nq queries
// qs / qdesc, on the plan's scratch of problem i
inline void fill_search_row(orbm_proj_plan* p, int i, const orbx_proj_frame& F, const orbx_query_proj* qs,
                            const uint8_t* qdesc, int nq, int32_t* match, int* nmatches) {
  const size_t QS = (size_t)std::max(p->max_nq, 1);
  ProjProblem& P = p->probs[i];
  P.F = proj_frame(&F);
  P.keys = F.keys;
  P.desc = F.desc;
  P.uright = F.uright;
  P.occupied = F.occupied;
  P.qs = qs;
  P.qdesc = qdesc;
  P.nq = nq;
  P.match = match;
  P.nmatches = nmatches;
  P.cell_off = p->d_cell_off + (size_t)i * (PG_CELLS + 1);
  P.cell_feat = p->d_cell_feat + (size_t)i * p->max_n;
  P.cand = p->d_cand + (size_t)i * QS * PJ_T;
  P.ncand = p->d_ncand + (size_t)i * QS;
}
}  // namespace orbx

#endif

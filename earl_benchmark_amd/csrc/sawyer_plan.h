// sawyer_plan.h -- what the Sawyer door / peg MPPI planner (include/earl_physics.h, "MPPI planning": earl_sawyer_plan_mppi, earl_sawyer_plan_candidates) computes per
// element, for the two kernels of sawyer_plan.hip and for the host twins of tabletop_host.cpp: the argument block, the argument rules and the reweighting's sum of one
// branch.  The clipped row, the candidate of one (branch, step, env) and its place in memory are sawyer_shoot.h's, shared with the CEM planner.  The dimension-free
// pieces of the contract -- plan_clip, plan_best / plan_best_merge, plan_weight, plan_new_mean and the noise counter's word 0 (kPlanDraw) -- ARE tabletop_plan.h's:
// items 1, 4, 5 and 7 are the tabletop's verbatim.  What differs is item 2 (FOUR action dimensions out of one Philox block, the gripper clipped like x, y, z) and where
// the candidates live: in memory, [K, H, n, 4], because the rollout that scores them reads them there.
#pragma once
#include "sawyer_shoot.h"

namespace earl {

struct SawyerPlanArgs {
  const float* mean;       // [H, n, 4]: the plan entering this iteration
  float* plan;             // [H, n, 4]: the plan leaving it; may be `mean`
  float* act;              // [K, H, n, 4]: the candidates (16-byte aligned)
  const double* ret;       // [K, n]
  double* ret0;            // NULL or [n]: this iteration's row of ret0
  double* best_ret;        // NULL or [n]  (the caller passes these two on the last iteration only)
  int32_t* best_k;         // NULL or [n]
  double inv_temperature;
  uint64_t seed;
  float sigma[4];
  uint32_t noise_counter;
  uint32_t word0;          // kPlanDraw | j
  int32_t env_offset, n, K, H;
};

// the block of one call before its per-iteration words (mean after the first iteration, plan, act, ret, ret0, best_*, word0) are set
inline SawyerPlanArgs sawyer_plan_args(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* pp, const float* mean) {
  SawyerPlanArgs p{};
  p.mean = mean;
  p.inv_temperature = pp->inv_temperature;
  p.seed = cfg->seed;
  for (int d = 0; d < 4; ++d) p.sigma[d] = pp->sigma[d];
  p.noise_counter = pp->noise_counter;
  p.env_offset = cfg->env_offset;
  p.n = cfg->n;
  p.K = pp->K;
  p.H = pp->H;
  return p;
}

// The argument rules the three calls share, in the header's order (the model / state side of earl_sawyer_plan_mppi is earl_sawyer_branch_rollout's own check).
// Mppi: `out` = plan, the iteration range is params'; Candidates: `out` = act_out, j the iteration, no temperature; Update (the host twin of the update kernel):
// `out` = plan, j the iteration, no sigma.
enum class SawyerPlanCall { Mppi, Candidates, Update };
inline int check_sawyer_plan(SawyerPlanCall call, const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* p, int32_t j, const float* mean, const void* out) {
  using hostside::fail;
  if (!cfg) return fail(EARL_ERR_ARG, "cfg is NULL");
  if (cfg->n < 0) return fail(EARL_ERR_ARG, "n = %d < 0", cfg->n);
  if (!p) return fail(EARL_ERR_ARG, "params is NULL");
  if (!mean || !out) return fail(EARL_ERR_ARG, call == SawyerPlanCall::Candidates ? "mean/act_out is NULL" : "mean/plan is NULL");
  if (p->K < 1 || p->K > EARL_SAWYER_PLAN_MAX_K) return fail(EARL_ERR_ARG, "K = %d: 1 .. %d", p->K, EARL_SAWYER_PLAN_MAX_K);
  if (p->H < 1 || p->H > 65536) return fail(EARL_ERR_ARG, "H = %d: 1 .. 65536", p->H);
  if (call == SawyerPlanCall::Mppi) {
    if (p->iterations < 1 || p->iteration0 < 0 || (long long)p->iteration0 + p->iterations > 256)
      return fail(EARL_ERR_ARG, "iterations = %d from iteration0 = %d: at least one, inside 0 .. 255", p->iterations, p->iteration0);
  } else if (j < 0 || j > 255) {
    return fail(EARL_ERR_ARG, "iteration %d: 0 .. 255", j);
  }
  if (call != SawyerPlanCall::Candidates && (!std::isfinite(p->inv_temperature) || !(p->inv_temperature > 0)))
    return fail(EARL_ERR_ARG, "inv_temperature = %g: finite and > 0", p->inv_temperature);
  if (call != SawyerPlanCall::Update)
    for (int d = 0; d < 4; ++d)
      if (!std::isfinite(p->sigma[d]) || !(p->sigma[d] >= 0)) return fail(EARL_ERR_ARG, "sigma[%d] = %g: finite and >= 0", d, (double)p->sigma[d]);
  if ((long long)p->K * cfg->n > 0x7fffffffll) return fail(EARL_ERR_ARG, "K n = %lld virtual envs: at most 2^31 - 1", (long long)p->K * cfg->n);
  if (call != SawyerPlanCall::Candidates && out != (const void*)mean) {
    const uintptr_t a = (uintptr_t)mean, b = (uintptr_t)out, bytes = (uintptr_t)p->H * (uintptr_t)cfg->n * 16u;
    if (a < b + bytes && b < a + bytes) return fail(EARL_ERR_ARG, "plan overlaps mean without being the same array");
  }
  return EARL_OK;
}

// item 5: a branch's candidate c of (env, step), READ back from the candidates, added with its weight to the four sums around the clipped row m
__device__ __forceinline__ void splan_accumulate(const float (&c)[4], const float (&m)[4], int32_t W, int64_t (&A)[4]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) A[d] += (int64_t)W * shoot_delta(c[d], m[d]);
}

}  // namespace earl

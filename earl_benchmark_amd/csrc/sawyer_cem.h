// sawyer_cem.h -- what the Sawyer door / peg CEM planner (include/earl_physics.h, "CEM planning on the door and the peg": earl_sawyer_plan_cem,
// earl_sawyer_cem_candidates, earl_sawyer_cem_update) computes per element, for the two kernels of sawyer_cem.hip and for the host twins of tabletop_host.cpp: the
// argument block, the argument rules, the clamped std of one (step, env), and an elite's share of the two integer moments.  The clipped row, the candidate of one
// (branch, step, env) -- its scale here the clamped std -- and its place in memory are sawyer_shoot.h's, shared with the MPPI planner.  The dimension-free pieces of the
// contract ARE the tabletop's, unedited: plan_clip, plan_best / plan_best_merge (tabletop_plan.h), cem_sclamp, cem_key, cem_before, cem_new_mean, cem_new_std and
// the noise counter's word 0, kCemDraw (tabletop_cem.h).  What differs is FOUR action dimensions out of one Philox block and where the candidates live: in memory,
// [K, H, n, 4], so item 5 reads an elite's candidate back instead of making it again.  The elite selection itself is cem_select.h's (device) or a sort (host).
#pragma once
#include "sawyer_shoot.h"
#include "tabletop_cem.h"

namespace earl {

struct SawyerCemArgs {
  const float* mean;       // [H, n, 4]: the plan entering this iteration
  const float* std_in;     // NULL (every row sclamp(sigma)) or [H, n, 4]: the std entering this iteration
  float* plan;             // [H, n, 4]: the plan leaving it; may be `mean`
  float* std_out;          // [H, n, 4]: the std leaving it; may be `std_in`
  const float* act;        // [K, H, n, 4]: the candidates (16-byte aligned)
  const double* ret;       // [K, n]
  double* ret0;            // NULL or [n]: this iteration's row of ret0
  double* best_ret;        // NULL or [n]  (earl_sawyer_plan_cem passes these three on the last iteration only)
  int32_t* best_k;         // NULL or [n]
  uint8_t* elite;          // NULL or [K, n]
  uint64_t seed;
  float sigma[4];
  uint32_t noise_counter;
  uint32_t word0;          // kCemDraw | j
  int32_t env_offset, n, K, H, E;
  float alpha, std_min, std_max;
};

// the block of one call before its per-iteration words (mean / std_in after the first iteration, plan, std_out, act, ret, ret0, best_*, elite, word0) are set
inline SawyerCemArgs sawyer_cem_args(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* c, const float* mean, const float* std_in) {
  SawyerCemArgs p{};
  p.mean = mean;
  p.std_in = std_in;
  p.seed = cfg->seed;
  for (int d = 0; d < 4; ++d) p.sigma[d] = c->sigma[d];
  p.noise_counter = c->noise_counter;
  p.env_offset = cfg->env_offset;
  p.n = cfg->n;
  p.K = c->K;
  p.H = c->H;
  p.E = c->elites;
  p.alpha = c->alpha;
  p.std_min = c->std_min;
  p.std_max = c->std_max;
  return p;
}

// The argument rules the three calls share, in the header's order (the model / state side of earl_sawyer_plan_cem is earl_sawyer_branch_rollout's own check).
// Cem: the iteration range is params'; Candidates: `plan` = act_out, j the iteration, no elites, no alpha, no std output; Update: j the iteration, no sigma rule
// beyond the planner's.
enum class SawyerCemCall { Cem, Candidates, Update };
inline int check_sawyer_cem(SawyerCemCall call, const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* c, int32_t j, const float* mean, const float* std0,
                            const void* plan, const float* std_out) {
  using hostside::fail;
  const bool cand = call == SawyerCemCall::Candidates;
  if (!cfg) return fail(EARL_ERR_ARG, "cfg is NULL");
  if (cfg->n < 0) return fail(EARL_ERR_ARG, "n = %d < 0", cfg->n);
  if (!c) return fail(EARL_ERR_ARG, "params is NULL");
  if (!mean || !plan) return fail(EARL_ERR_ARG, cand ? "mean/act_out is NULL" : "mean/plan is NULL");
  if (c->K < 1 || c->K > EARL_SAWYER_PLAN_MAX_K) return fail(EARL_ERR_ARG, "K = %d: 1 .. %d", c->K, EARL_SAWYER_PLAN_MAX_K);
  if (c->H < 1 || c->H > 65536) return fail(EARL_ERR_ARG, "H = %d: 1 .. 65536", c->H);
  if (call == SawyerCemCall::Cem) {
    if (c->iterations < 1 || c->iteration0 < 0 || (long long)c->iteration0 + c->iterations > 256)
      return fail(EARL_ERR_ARG, "iterations = %d from iteration0 = %d: at least one, inside 0 .. 255", c->iterations, c->iteration0);
  } else if (j < 0 || j > 255) {
    return fail(EARL_ERR_ARG, "iteration %d: 0 .. 255", j);
  }
  for (int d = 0; d < 4; ++d)
    if (!std::isfinite(c->sigma[d]) || !(c->sigma[d] >= 0)) return fail(EARL_ERR_ARG, "sigma[%d] = %g: finite and >= 0", d, (double)c->sigma[d]);
  if ((long long)c->K * cfg->n > 0x7fffffffll) return fail(EARL_ERR_ARG, "K n = %lld virtual envs: at most 2^31 - 1", (long long)c->K * cfg->n);
  if (!cand) {
    const int emax = c->K < EARL_SAWYER_CEM_MAX_E ? c->K : EARL_SAWYER_CEM_MAX_E;
    if (c->elites < 1 || c->elites > emax)
      return fail(EARL_ERR_ARG, "elites = %d: 1 .. min(K, %d) = %d (the moments of more elites leave int64)", c->elites, EARL_SAWYER_CEM_MAX_E, emax);
    if (!std::isfinite(c->alpha) || !(c->alpha >= 0.0f && c->alpha < 1.0f)) return fail(EARL_ERR_ARG, "alpha = %g: finite, 0 <= alpha < 1", (double)c->alpha);
  }
  if (!std::isfinite(c->std_min) || !std::isfinite(c->std_max) || !(c->std_min >= 0.0f && c->std_min <= c->std_max))
    return fail(EARL_ERR_ARG, "std_min = %g, std_max = %g: finite, 0 <= std_min <= std_max", (double)c->std_min, (double)c->std_max);
  if (!cand && !std_out) return fail(EARL_ERR_ARG, "std is NULL: it is the workspace between iterations and a result");
  const uintptr_t bytes = (uintptr_t)c->H * (uintptr_t)cfg->n * 16u;
  const void* arr[4] = {mean, cand ? nullptr : plan, std0, std_out};   // allowed to coincide: (mean, plan) and (std0, std)
  for (int x = 0; x < 4; ++x)
    for (int y = x + 1; y < 4; ++y) {
      if (!arr[x] || !arr[y]) continue;
      const uintptr_t a = (uintptr_t)arr[x], b = (uintptr_t)arr[y];
      const bool pair = (x == 0 && y == 1) || (x == 2 && y == 3);
      if (pair && a == b) continue;
      if (a < b + bytes && b < a + bytes) return fail(EARL_ERR_ARG, "mean, std0, plan and std overlap beyond plan == mean and std == std0");
    }
  return EARL_OK;
}

// item 1: row t of env i of the std entering, all four words clamped (the plan's row is sawyer_shoot.h's shoot_mean)
__device__ __forceinline__ void scem_std(const SawyerCemArgs& p, int i, int t, float (&s)[4]) {
  if (p.std_in) {
    const float* sp = p.std_in + ((size_t)t * p.n + i) * 4;
#pragma unroll
    for (int d = 0; d < 4; ++d) s[d] = cem_sclamp(sp[d], p.std_min, p.std_max);
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d) s[d] = cem_sclamp(p.sigma[d], p.std_min, p.std_max);
  }
}

// item 5: an elite's candidate c of (env, step), READ back from the candidates, added to the two moments around the clipped row m
__device__ __forceinline__ void scem_accumulate(const float (&c)[4], const float (&m)[4], int64_t (&A1)[4], int64_t (&A2)[4]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int64_t D = shoot_delta(c[d], m[d]);
    A1[d] += D;
    A2[d] += D * D;
  }
}

}  // namespace earl

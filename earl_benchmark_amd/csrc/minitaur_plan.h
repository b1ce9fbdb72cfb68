// minitaur_plan.h -- what the minitaur's MPPI planner (include/earl_physics.h, "MPPI planning on the minitaur": earl_minitaur_plan_mppi, earl_minitaur_plan_candidates)
// computes per element, for the two kernels of minitaur_plan.hip and, under -DEARL_HOST_BUILD, for the host twins of tabletop_host.cpp: the argument block, the argument
// rules, the clipped row, the candidate of one (branch, step, env) and its place in memory, the reweighting's sums of one branch -- and, host side, the ONE statement of
// the planner's workspace block.  The dimension-free pieces of the contract ARE tabletop_plan.h's (plan_clip, plan_best / plan_best_merge, plan_weight, plan_new_mean,
// kPlanDraw, the quantile) and sawyer_shoot.h's (shoot_delta, shoot_for_each_candidate, wave_sum, block_best), as they stand.  What differs from the Sawyer planner is
// item 2: EIGHT action dimensions out of two Philox blocks, the first of them the Sawyer planner's.
#pragma once
#include "minitaur_branch_ws.h"
#include "sawyer_shoot.h"

namespace earl {

struct MinitaurPlanArgs {
  const float* mean;       // [H, n, 8]: the plan entering this iteration
  float* plan;             // [H, n, 8]: the plan leaving it; may be `mean`
  float* act;              // [K, H, n, 8]: the candidates (16-byte aligned)
  const double* ret;       // [K, n]
  double* ret0;            // NULL or [n]: this iteration's row of ret0
  double* best_ret;        // NULL or [n]  (the caller passes these two on the last iteration only)
  int32_t* best_k;         // NULL or [n]
  double inv_temperature;
  uint64_t seed;
  float sigma[8];
  uint32_t noise_counter;
  uint32_t word0;          // kPlanDraw | j
  int32_t env_offset, n, K, H;
};

// the block of one call before its per-iteration words (mean after the first iteration, plan, act, ret, ret0, best_*, word0) are set
inline MinitaurPlanArgs minitaur_plan_args(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* pp, const float* mean) {
  MinitaurPlanArgs p{};
  p.mean = mean;
  p.inv_temperature = pp->inv_temperature;
  p.seed = cfg->seed;
  for (int d = 0; d < 8; ++d) p.sigma[d] = pp->sigma[d];
  p.noise_counter = pp->noise_counter;
  p.env_offset = cfg->env_offset;
  p.n = cfg->n;
  p.K = pp->K;
  p.H = pp->H;
  return p;
}

// The argument rules the three calls share, in the header's order (the model / state side of earl_minitaur_plan_mppi is earl_minitaur_branch_rollout's own check).
// Mppi: `out` = plan, the iteration range is params'; Candidates: `out` = act_out, j the iteration, no temperature; Update (the host twin of the update kernel):
// `out` = plan, j the iteration, no sigma.
enum class MinitaurPlanCall { Mppi, Candidates, Update };
inline int check_minitaur_plan(MinitaurPlanCall call, const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* p, int32_t j, const float* mean, const void* out) {
  using hostside::fail;
  if (!cfg) return fail(EARL_ERR_ARG, "cfg is NULL");
  if (cfg->n < 0) return fail(EARL_ERR_ARG, "n = %d < 0", cfg->n);
  if (!p) return fail(EARL_ERR_ARG, "params is NULL");
  if (!mean || !out) return fail(EARL_ERR_ARG, call == MinitaurPlanCall::Candidates ? "mean/act_out is NULL" : "mean/plan is NULL");
  if (p->K < 1 || p->K > EARL_MINITAUR_PLAN_MAX_K) return fail(EARL_ERR_ARG, "K = %d: 1 .. %d", p->K, EARL_MINITAUR_PLAN_MAX_K);
  if (p->H < 1 || p->H > 65536) return fail(EARL_ERR_ARG, "H = %d: 1 .. 65536", p->H);
  if (call == MinitaurPlanCall::Mppi) {
    if (p->iterations < 1 || p->iteration0 < 0 || (long long)p->iteration0 + p->iterations > 256)
      return fail(EARL_ERR_ARG, "iterations = %d from iteration0 = %d: at least one, inside 0 .. 255", p->iterations, p->iteration0);
  } else if (j < 0 || j > 255) {
    return fail(EARL_ERR_ARG, "iteration %d: 0 .. 255", j);
  }
  if (call != MinitaurPlanCall::Candidates && (!std::isfinite(p->inv_temperature) || !(p->inv_temperature > 0)))
    return fail(EARL_ERR_ARG, "inv_temperature = %g: finite and > 0", p->inv_temperature);
  if (call != MinitaurPlanCall::Update)
    for (int d = 0; d < 8; ++d)
      if (!std::isfinite(p->sigma[d]) || !(p->sigma[d] >= 0)) return fail(EARL_ERR_ARG, "sigma[%d] = %g: finite and >= 0", d, (double)p->sigma[d]);
  if ((long long)p->K * cfg->n > 0x7fffffffll) return fail(EARL_ERR_ARG, "K n = %lld virtual envs: at most 2^31 - 1", (long long)p->K * cfg->n);
  if (call != MinitaurPlanCall::Candidates && out != (const void*)mean) {
    const uintptr_t a = (uintptr_t)mean, b = (uintptr_t)out, bytes = (uintptr_t)p->H * (uintptr_t)cfg->n * 32u;
    if (a < b + bytes && b < a + bytes) return fail(EARL_ERR_ARG, "plan overlaps mean without being the same array");
  }
  return EARL_OK;
}

// item 1: row t of env i of the plan entering, all eight words clipped
__device__ __forceinline__ void mtplan_mean(const float* mean, int n, int i, int t, float (&m)[8]) {
  const float* mp = mean + ((size_t)t * n + i) * 8;
#pragma unroll
  for (int d = 0; d < 8; ++d) m[d] = plan_clip(mp[d]);
}

// where candidate k of (step t, env i) lives in a [K, H, n, 8] array
__device__ __forceinline__ size_t mtplan_act_index(int H, int n, int i, int k, int t) { return (((size_t)k * H + t) * n + i) * 8; }

// item 2: candidate k of (step t, the env with global id gid) around the clipped row m -- the row itself for k == 0, else two Philox blocks and eight quantiles, each
// times its sigma: the Sawyer planner's block (shoot_candidate) for dimensions 0 .. 3, the block with bit 31 of word 2 set for 4 .. 7 (k < 2^15, t < 2^16: the bit is free)
__device__ __forceinline__ void mtplan_candidate(uint32_t word0, uint32_t gid, uint32_t k, uint32_t t, uint32_t noise_counter, uint64_t seed, const float (&sigma)[8],
                                                 const float (&m)[8], float (&c)[8]) {
  if (k == 0) {
#pragma unroll
    for (int d = 0; d < 8; ++d) c[d] = m[d];
    return;
  }
  const U4 b0 = philox4x32_10(U4{word0, gid, (k << 16) | t, noise_counter}, (uint32_t)seed, (uint32_t)(seed >> 32));
  const U4 b1 = philox4x32_10(U4{word0, gid, 0x80000000u | (k << 16) | t, noise_counter}, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t w[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
  for (int d = 0; d < 8; ++d) c[d] = plan_clip(fmaf(sigma[d], normal_quantile_f32(w[d] >> 8), m[d]));
}

// item 5: a branch's candidate c of (env, step), READ back from the candidates, added with its weight to the eight sums around the clipped row m
__device__ __forceinline__ void mtplan_accumulate(const float (&c)[8], const float (&m)[8], int32_t W, int64_t (&A)[8]) {
#pragma unroll
  for (int d = 0; d < 8; ++d) A[d] += (int64_t)W * shoot_delta(c[d], m[d]);
}

// The block of a planner call, from its 8-byte aligned base: the branch launch's workspace (minitaur_branch_ws.h) rounded up to 8 bytes (`branch`), then the [K, H, n, 8]
// candidates at the next 16-byte ADDRESS (8 bytes of slack).  need: 0 without a virtual env.  The ONLY statement of the block: the size function, the refusal and the
// driver's carve read it
struct MinitaurPlanLayout {
  int64_t branch, need;
};
inline int minitaur_plan_layout(int32_t K, int32_t H, int32_t n, MinitaurPlanLayout* L) {
  if (K < 0 || H < 0 || n < 0 || (int64_t)K * n > 0x7fffffffll) return EARL_ERR_ARG;
  const int64_t V = (int64_t)K * n;
  L->branch = (minitaur_branch_layout(V).bytes + 7) / 8 * 8;
  L->need = V == 0 ? 0 : L->branch + 8 + V * H * 32;
  return EARL_OK;
}
inline float* minitaur_plan_candidates_at(void* base, const MinitaurPlanLayout& L) {
  return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(base) + (uintptr_t)L.branch + 15) & ~(uintptr_t)15);
}

}  // namespace earl

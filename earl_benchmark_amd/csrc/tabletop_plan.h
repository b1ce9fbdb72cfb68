// tabletop_plan.h -- what the tabletop planners run per lane on top of tabletop_step.h's wrapped step: the branch launch's argument block and body, and the whole MPPI
// contract (PlanArgs, plan_clip .. plan_new_mean, plan_score_body, plan_candidates_body; PlanValueArgs for the `_value` calls: their sum and network are tabletop_value.h's).
// Included by the units that plan (tabletop_branch.hip, tabletop_plan.hip, tabletop_plan_value.hip, tabletop_mpc.h) and the host twin; all others stop at tabletop_step.h.
#pragma once
#include "tabletop_step.h"
#include "policy_math.h"   // exp_f32, normal_quantile_f32: the planner's noise and weights (plan_* below)
#include "tabletop_value.h"   // the discounted score with a terminal value (plan_score_body<.., true>)

namespace earl {

// earl_tabletop[3]_branch_rollout: K candidate action sequences per env, scored from the CURRENT state.  `a` is the rollout's argument block (T = the horizon
// H of a branch, `out` unused, `st` read and never written); the rest is what a branch adds.
struct BranchArgs {
  KArgs a;
  long long act_branch_stride;  // floats between the [H, n, 3] blocks of consecutive branches; 0 = one block for all
  earl_episode_summary sum;     // rows [K, n]; any pointer may be NULL
  float* last_obs;              // NULL or [K, n, NOBS]: the row out->obs[H-1] of the equivalent rollout
};

// Branch k of env i: rollout_body's loop (same loads, same prefetch, same wrapped_step, same counters) with the per-step stores replaced by the three
// reducers of earl_episode_summary held in registers, and without store_lane -- the state is where it was when the launch ends.
template <int NOBJ, bool GENERAL>
__device__ __forceinline__ void branch_body(const BranchArgs& b, int i, int k) {
  const KArgs& a = b.a;
  const int n = a.cfg.n;
  Lane<NOBJ> L;
  load_lane<NOBJ>(a, i, L);
  float g[Dims<NOBJ>::NG];
  load_goal<NOBJ>(a.st.goal_table, L.goal_idx, g);
  const float* act = a.act + (size_t)k * (size_t)b.act_branch_stride;
  double ret = 0.0;
  bool succ_last = false;
  int first = -1;
  float o[Dims<NOBJ>::NOBS] = {};
  constexpr int PF = 8;  // as rollout_body: the actions are state-independent
  for (int t0 = 0; t0 < a.T; t0 += PF) {
    float av[PF][3];
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int t = t0 + j < a.T ? t0 + j : a.T - 1;
      const float* ap = act + ((size_t)t * n + i) * 3;
      av[j][0] = ap[0];
      av[j][1] = ap[1];
      av[j][2] = ap[2];
    }
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int t = t0 + j;
      if (t < a.T) {
        float reward;
        bool done, succ;
        wrapped_step<NOBJ, GENERAL>(a, i, a.cfg.counter + (uint64_t)t, L, g, av[j][0], av[j][1], av[j][2], o, reward, done, succ);
        ret += (double)reward;
        succ_last = succ;
        if (succ && first < 0) first = t;
      }
    }
  }
  const size_t row = (size_t)k * n + i;
  if (b.sum.ret) b.sum.ret[row] = ret;
  if (b.sum.success_last) b.sum.success_last[row] = succ_last;
  if (b.sum.first_success) b.sum.first_success[row] = first;
  if (b.last_obs) store_obs<NOBJ>(b.last_obs + row * Dims<NOBJ>::NOBS, o);
}

// earl_tabletop[3]_plan_mppi / earl_tabletop_plan_candidates (include/earl_tabletop.h, "MPPI planning": the numbered items cited below are its contract).  One
// iteration is two launches: plan_score_body per (branch, env) -- branch_body's loop with the action loads replaced by the candidate made on the spot -- and the
// update, per (env, step), which makes every candidate AGAIN from the same counters.  The functions below are everything either launch computes; the kernels
// (tabletop_plan.hip) and the host twin (tabletop_host.cpp) only decide who calls them for which (k, env, t).
constexpr uint32_t kPlanDraw = 0x504C4E00u;   // word 0 of the noise counter, | the iteration index (the env's draws: 0 .. 2048; kGaussDraw: 0x504F4C00)

struct PlanArgs {
  KArgs a;                 // the branch launch's block: T = the horizon H of a plan, `act` and `out` unused, `st` read and never written
  const float* mean;       // [H, n, 3]: the plan entering this iteration
  float* plan;             // [H, n, 3]: the plan leaving it; may be `mean`
  double* ret;             // [K, n]
  double* ret0;            // NULL or [n]: this iteration's row of ret0
  double* best_ret;        // NULL or [n]  (the caller passes these two on the last iteration only)
  int32_t* best_k;         // NULL or [n]
  double inv_temperature;
  float sigma[3];
  uint32_t noise_counter;
  uint32_t word0;          // kPlanDraw | j
  int32_t K;
};

// the argument block of one call before its per-iteration words (mean after the first iteration, plan, ret, ret0, best_*, word0) are set; st == NULL: earl_tabletop_plan_candidates
inline PlanArgs plan_args(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, const float* mean, const Thresholds& th) {
  PlanArgs p{};
  p.a = KArgs{*cfg, st ? *st : earl_tabletop_state{}, earl_tabletop_out{nullptr, nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr, nullptr, nullptr, pp->H, th};
  p.mean = mean;
  p.inv_temperature = pp->inv_temperature;
  for (int d = 0; d < 3; ++d) p.sigma[d] = pp->sigma[d];
  p.noise_counter = pp->noise_counter;
  p.K = pp->K;
  return p;
}

// earl_tabletop[3]_plan_mppi_value: the planner's block followed by the discount and the value network.  A derived struct, so that every function above and below
// takes it as the PlanArgs it starts with and the value-free launches pass what they always passed
struct PlanValueArgs : PlanArgs {
  ValueArgs v;
};

#ifndef EARL_HOST_BUILD
// the update launch of one iteration (tabletop_plan.hip: ublocks workgroups of kBranchBlock * kPlanUpdateSteps lanes on `stream`), for the units that score
void plan_update_launch(const PlanArgs& p, unsigned tiles, unsigned ublocks, earl_stream_t stream);
#endif

// item 1 (and the clip of item 2 and 5): min(max(x, -1), 1) as two compare-and-selects, NaN -> -1
__device__ __forceinline__ float plan_clip(float x) {
  const float y = x > -1.0f ? x : -1.0f;
  return y < 1.0f ? y : 1.0f;
}

__device__ __forceinline__ void plan_mean(const PlanArgs& p, int i, int t, float (&m)[3]) {
  const float* mp = p.mean + ((size_t)t * p.a.cfg.n + i) * 3;
  m[0] = plan_clip(mp[0]);
  m[1] = plan_clip(mp[1]);
  m[2] = plan_clip(mp[2]);
}

// item 2, k >= 1: one Philox block and three quantiles
__device__ __forceinline__ void plan_candidate(const PlanArgs& p, int i, uint32_t k, uint32_t t, const float (&m)[3], float (&c)[3]) {
  const U4 b = philox4x32_10(U4{p.word0, (uint32_t)(p.a.cfg.env_offset + i), (k << 16) | t, p.noise_counter}, (uint32_t)p.a.cfg.seed,
                             (uint32_t)(p.a.cfg.seed >> 32));
  c[0] = plan_clip(fmaf(p.sigma[0], normal_quantile_f32(b.x >> 8), m[0]));
  c[1] = plan_clip(fmaf(p.sigma[1], normal_quantile_f32(b.y >> 8), m[1]));
  c[2] = plan_clip(fmaf(p.sigma[2], normal_quantile_f32(b.z >> 8), m[2]));
}

// item 3: branch k of env i.  branch_body's loop (same state loads, same wrapped_step, same counters, eight steps of the mean in flight) with the candidate of
// the step made in registers; one word stored.  VALUE (the `_value` entry points; v != NULL): item 3 as tabletop_value.h states it -- the discounted sum, and the value
// network on the last step's row (what branch_body stores as last_obs).  That row is made AGAIN after the loop from the state the last step left (its auto-reset is
// left out: the copy is thrown away), so that no observation stays live through the loop's register peak.
template <int NOBJ, bool GENERAL, bool VALUE = false>
__device__ __forceinline__ void plan_score_body(const PlanArgs& p, int i, int k, const ValueArgs* v = nullptr) {
  const KArgs& a = p.a;
  Lane<NOBJ> L;
  load_lane<NOBJ>(a, i, L);
  float g[Dims<NOBJ>::NG];
  load_goal<NOBJ>(a.st.goal_table, L.goal_idx, g);
  double ret = 0.0;
  [[maybe_unused]] double disc = 1.0;
  float o[Dims<NOBJ>::NOBS];
  constexpr int PF = 8;
  for (int t0 = 0; t0 < a.T; t0 += PF) {
    float mv[PF][3];
#pragma unroll
    for (int j = 0; j < PF; ++j) plan_mean(p, i, t0 + j < a.T ? t0 + j : a.T - 1, mv[j]);
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int t = t0 + j;
      if (t < a.T) {
        float c[3] = {mv[j][0], mv[j][1], mv[j][2]};
        if (k > 0) plan_candidate(p, i, (uint32_t)k, (uint32_t)t, mv[j], c);
        float reward;
        bool done, succ;
        if constexpr (VALUE) {
          wrapped_step<NOBJ, GENERAL>(a, i, a.cfg.counter + (uint64_t)t, L, g, c[0], c[1], c[2], o, reward, done, succ, nullptr, t + 1 < a.T);
          value_accumulate(ret, disc, reward, v->discount);
        } else {
          wrapped_step<NOBJ, GENERAL>(a, i, a.cfg.counter + (uint64_t)t, L, g, c[0], c[1], c[2], o, reward, done, succ);
          ret += (double)reward;
        }
      }
    }
  }
  if constexpr (VALUE) {
    if (v->net.params) {
      float ov[Dims<NOBJ>::NOBS];
      make_obs<NOBJ>(L.e, g, ov);
      ret = value_terminal<Dims<NOBJ>::NOBS>(*v, ov, ret, disc);
    }
  }
  p.ret[(size_t)k * a.cfg.n + i] = ret;
  if (k == 0 && p.ret0) p.ret0[i] = ret;
}

// item 4.  beta and best_k: plan_best over k ASCENDING from (-Inf, 0); plan_best_merge joins two such results over disjoint sets of k in any order.
__device__ __forceinline__ void plan_best(double r, int k, double& beta, int& bk) {
  if (r > beta) { beta = r; bk = k; }
}
__device__ __forceinline__ void plan_best_merge(double r, int k, double& beta, int& bk) {
  if (r > beta || (r == beta && k < bk)) { beta = r; bk = k; }
}
__device__ __forceinline__ int32_t plan_weight(double r, double beta, double inv_temperature) {
  const float x = (float)((r - beta) * inv_temperature);
  if (!(x == x)) return 0;                                        // item 7: a NaN return, or Inf - Inf
  return (int32_t)__builtin_rint((double)exp_f32(x) * 16777216.0);   // x <= 0: 0 .. 2^24
}

// item 5: branch k >= 1 added to the three sums of (env i, step t), and the new mean out of a sum
__device__ __forceinline__ void plan_accumulate(const PlanArgs& p, int i, uint32_t k, uint32_t t, const float (&m)[3], int32_t W, int64_t (&A)[3]) {
  float c[3];
  plan_candidate(p, i, k, t, m, c);
#pragma unroll
  for (int d = 0; d < 3; ++d) A[d] += (int64_t)W * (int64_t)(int32_t)__builtin_rint((double)(c[d] - m[d]) * 1048576.0);   // |D| <= 2^21
}
__device__ __forceinline__ float plan_new_mean(float m, int64_t A, int64_t S) {
  if (S == 0) return m;                                           // item 7
  return plan_clip(m + (float)((double)A / ((double)S * 1048576.0)));
}

// earl_tabletop_plan_candidates: the candidates of (branch k, env i) written out, act_out [K, H, n, 3]
__device__ __forceinline__ void plan_candidates_body(const PlanArgs& p, int i, int k, float* __restrict__ act_out) {
  const int n = p.a.cfg.n;
  for (int t = 0; t < p.a.T; ++t) {
    float m[3];
    plan_mean(p, i, t, m);
    float c[3] = {m[0], m[1], m[2]};
    if (k > 0) plan_candidate(p, i, (uint32_t)k, (uint32_t)t, m, c);
    float* dst = act_out + (((size_t)k * p.a.T + t) * n + i) * 3;
    dst[0] = c[0];
    dst[1] = c[1];
    dst[2] = c[2];
  }
}

}  // namespace earl

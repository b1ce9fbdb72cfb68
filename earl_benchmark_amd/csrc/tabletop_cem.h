// tabletop_cem.h -- the cross-entropy planner of earl_tabletop[3]_plan_cem / earl_tabletop_cem_candidates / earl_tabletop[3]_mpc_rollout_cem (include/earl_tabletop.h,
// "CEM planning": the numbered items cited below are its contract): what a lane runs on top of tabletop_plan.h's plan_clip, plan_mean and plan_best*, tabletop_step.h's
// wrapped step and tabletop_value.h's discounted score.  Shared by the gfx950 kernels (tabletop_cem.hip, tabletop_cem_mpc.hip) and the host twin (tabletop_host.cpp);
// the kernels and the twin only decide who calls these functions for which (k, env, t).  What differs from MPPI: a noise scale per (step, env, dim) (cem_std,
// cem_candidate), the elites by a total order (cem_before), and an update of two integer moments over the elites alone (cem_accumulate, cem_new_mean, cem_new_std).
#pragma once
#include "tabletop_mpc.h"   // copy_lane, mpc_act, check_mpc: the receding-horizon loop's; tabletop_plan.h and tabletop_hostside.h through it

namespace earl {

constexpr uint32_t kCemDraw = 0x43454D00u;   // word 0 of the noise counter, | the iteration index (the envs: 0 .. 2048; kGaussDraw 0x504F4C00; kPlanDraw 0x504C4E00)

struct CemArgs {
  PlanArgs p;              // plan_args(): a.T = H, mean / plan / ret / ret0 / best_*, sigma, noise_counter, word0 = kCemDraw | j, K; inv_temperature unused
  const float* std_in;     // NULL (every row sclamp(sigma)) or [H, n, 3]: the std entering this iteration
  float* std_out;          // [H, n, 3]: the std leaving it; may be std_in
  ValueArgs v;             // the `pv` block (VALUE instantiations only)
  int32_t E;
  float alpha, std_min, std_max;
};

// earl_tabletop[3]_mpc_rollout_cem: the loop's block (mpc_act reads x) followed by what CEM adds
struct CemMpcArgs {
  MpcArgs x;
  int32_t E;
  float alpha, std_min, std_max;
};

// item 1: (y = x > std_min ? x : std_min; y < std_max ? y : std_max), NaN -> std_min
__device__ __forceinline__ float cem_sclamp(float x, float lo, float hi) {
  const float y = x > lo ? x : lo;
  return y < hi ? y : hi;
}

__device__ __forceinline__ void cem_std(const CemArgs& c, int i, int t, float (&s)[3]) {
  if (c.std_in) {
    const float* sp = c.std_in + ((size_t)t * c.p.a.cfg.n + i) * 3;
    s[0] = cem_sclamp(sp[0], c.std_min, c.std_max);
    s[1] = cem_sclamp(sp[1], c.std_min, c.std_max);
    s[2] = cem_sclamp(sp[2], c.std_min, c.std_max);
  } else {
    s[0] = cem_sclamp(c.p.sigma[0], c.std_min, c.std_max);
    s[1] = cem_sclamp(c.p.sigma[1], c.std_min, c.std_max);
    s[2] = cem_sclamp(c.p.sigma[2], c.std_min, c.std_max);
  }
}

// item 2, k >= 1: plan_candidate with the row's own std.  cem_noise: the three quantiles of the block alone, for the caller that fetches the std after them
__device__ __forceinline__ void cem_noise(const PlanArgs& p, int i, uint32_t k, uint32_t t, float (&eps)[3]) {
  const U4 b = philox4x32_10(U4{p.word0, (uint32_t)(p.a.cfg.env_offset + i), (k << 16) | t, p.noise_counter}, (uint32_t)p.a.cfg.seed,
                             (uint32_t)(p.a.cfg.seed >> 32));
  eps[0] = normal_quantile_f32(b.x >> 8);
  eps[1] = normal_quantile_f32(b.y >> 8);
  eps[2] = normal_quantile_f32(b.z >> 8);
}
__device__ __forceinline__ void cem_candidate(const PlanArgs& p, int i, uint32_t k, uint32_t t, const float (&m)[3], const float (&s)[3], float (&c)[3]) {
  float eps[3];
  cem_noise(p, i, k, t, eps);
  c[0] = plan_clip(fmaf(s[0], eps[0], m[0]));
  c[1] = plan_clip(fmaf(s[1], eps[1], m[1]));
  c[2] = plan_clip(fmaf(s[2], eps[2], m[2]));
}

// item 3: one look-ahead step of a branch and what follows the last one, for cem_score_body and cem_mpc_score
template <int NOBJ, bool GENERAL, bool VALUE>
__device__ __forceinline__ void cem_step(const KArgs& a, int i, uint64_t counter, bool more, Lane<NOBJ>& L, float (&g)[Dims<NOBJ>::NG], const float (&c)[3],
                                         float (&o)[Dims<NOBJ>::NOBS], double& ret, double& disc, const ValueArgs& v) {
  float reward;
  bool done, succ;
  if constexpr (VALUE) {   // (the last step without its auto-reset, the row made again after the loop: plan_score_body)
    wrapped_step<NOBJ, GENERAL>(a, i, counter, L, g, c[0], c[1], c[2], o, reward, done, succ, nullptr, more);
    value_accumulate(ret, disc, reward, v.discount);
  } else {
    wrapped_step<NOBJ, GENERAL>(a, i, counter, L, g, c[0], c[1], c[2], o, reward, done, succ);
    ret += (double)reward;
  }
}
template <int NOBJ, bool VALUE>
__device__ __forceinline__ double cem_terminal(const Lane<NOBJ>& L, const float (&g)[Dims<NOBJ>::NG], double ret, double disc, const ValueArgs& v) {
  if constexpr (VALUE) {
    if (v.net.params) {
      float ov[Dims<NOBJ>::NOBS];
      make_obs<NOBJ>(L.e, g, ov);
      ret = value_terminal<Dims<NOBJ>::NOBS>(v, ov, ret, disc);
    }
  }
  return ret;
}

// item 3: branch k of env i -- plan_score_body with the 12 B of the row's std prefetched beside the 12 B of its mean
template <int NOBJ, bool GENERAL, bool VALUE>
__device__ __forceinline__ void cem_score_body(const CemArgs& c, int i, int k) {
  const PlanArgs& p = c.p;
  const KArgs& a = p.a;
  Lane<NOBJ> L;
  load_lane<NOBJ>(a, i, L);
  float g[Dims<NOBJ>::NG];
  load_goal<NOBJ>(a.st.goal_table, L.goal_idx, g);
  double ret = 0.0, disc = 1.0;
  float o[Dims<NOBJ>::NOBS];
  constexpr int PF = 8;
  for (int t0 = 0; t0 < a.T; t0 += PF) {
    float mv[PF][3], sv[PF][3];
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int t = t0 + j < a.T ? t0 + j : a.T - 1;
      plan_mean(p, i, t, mv[j]);
      cem_std(c, i, t, sv[j]);
    }
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int t = t0 + j;
      if (t < a.T) {
        float cv[3] = {mv[j][0], mv[j][1], mv[j][2]};
        if (k > 0) cem_candidate(p, i, (uint32_t)k, (uint32_t)t, mv[j], sv[j], cv);
        cem_step<NOBJ, GENERAL, VALUE>(a, i, a.cfg.counter + (uint64_t)t, t + 1 < a.T, L, g, cv, o, ret, disc, c.v);
      }
    }
  }
  ret = cem_terminal<NOBJ, VALUE>(L, g, ret, disc, c.v);
  p.ret[(size_t)k * a.cfg.n + i] = ret;
  if (k == 0 && p.ret0) p.ret0[i] = ret;
}

// the value-free score from the state (L, g) of the receding-horizon loop, on a copy: row(t, m, s) hands out the clipped mean and the clamped std of look-ahead step t
template <int NOBJ, bool GENERAL, class Row>
__device__ __forceinline__ double cem_mpc_score(const PlanArgs& q, int i, int k, uint64_t counter, const Lane<NOBJ>& L, const float (&g)[Dims<NOBJ>::NG], Row&& row) {
  Lane<NOBJ> B;
  copy_lane<NOBJ>(B, L);
  float gb[Dims<NOBJ>::NG];
#pragma unroll
  for (int j = 0; j < Dims<NOBJ>::NG; ++j) gb[j] = g[j];
  double ret = 0.0, disc = 1.0;
  float o[Dims<NOBJ>::NOBS];
  for (int t = 0; t < q.a.T; ++t) {
    float c[3];
    if (k > 0) {   // (the row is read after the quantiles: nothing of it is live through them)
      float eps[3], m[3], s[3];
      cem_noise(q, i, (uint32_t)k, (uint32_t)t, eps);
      row(t, m, s);
#pragma unroll
      for (int d = 0; d < 3; ++d) c[d] = plan_clip(fmaf(s[d], eps[d], m[d]));
    } else {
      float s[3];
      row(t, c, s);
    }
    cem_step<NOBJ, GENERAL, false>(q.a, i, counter + (uint64_t)t, true, B, gb, c, o, ret, disc, ValueArgs{});
  }
  return ret;
}

// item 4: whether branch ka (return a) stands before branch kb (return b) in the total order; rank_k = the number of branches before k
__device__ __forceinline__ bool cem_before(double a, int ka, double b, int kb) {
  const bool na = !(a == a), nb = !(b == b);
  if (na != nb) return nb;
  if (!na && a != b) return a > b;
  return ka < kb;
}
__device__ __forceinline__ bool cem_elite(double r, int rank, int E) { return rank < E && r == r; }
// the same order on integers, for the pass that compares one return against many: cem_before(a, ka, b, kb) == (cem_key(a) > cem_key(b) || (cem_key(a) == cem_key(b) &&
// ka < kb)).  The usual order-preserving image of a float64 (sign flipped for positives, all bits for negatives) with -0 folded into +0 and every NaN at 0, below -Inf
__device__ __forceinline__ uint64_t cem_key(double r) {
  if (!(r == r)) return 0ull;
  const uint64_t b = __builtin_bit_cast(uint64_t, r + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// item 5: elite k >= 1 added to the two moments of (env i, step t), and the new mean and std out of them
__device__ __forceinline__ void cem_accumulate(const PlanArgs& p, int i, uint32_t k, uint32_t t, const float (&m)[3], const float (&s)[3], int64_t (&A1)[3],
                                               int64_t (&A2)[3]) {
  float c[3];
  cem_candidate(p, i, k, t, m, s, c);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int64_t D = (int64_t)(int32_t)__builtin_rint((double)(c[d] - m[d]) * 1048576.0);   // |D| <= 2^21
    A1[d] += D;
    A2[d] += D * D;
  }
}
__device__ __forceinline__ float cem_new_mean(float m, int64_t A1, int32_t Ne, float alpha) {
  if (Ne == 0) return m;
  const float e = m + (float)((double)A1 / ((double)Ne * 1048576.0));
  return plan_clip(fmaf(alpha, m - e, e));
}
__device__ __forceinline__ float cem_new_std(float s, int64_t A1, int64_t A2, int32_t Ne, float alpha, float lo, float hi) {
  if (Ne == 0) return s;
  const int64_t V = (int64_t)Ne * A2 - A1 * A1;
  const float e = __builtin_sqrtf((float)((double)V / ((double)Ne * (double)Ne * 1099511627776.0)));
  return cem_sclamp(fmaf(alpha, s - e, e), lo, hi);
}

// earl_tabletop_cem_candidates: the candidates of (branch k, env i) written out, act_out [K, H, n, 3]
__device__ __forceinline__ void cem_candidates_body(const CemArgs& c, int i, int k, float* __restrict__ act_out) {
  const int n = c.p.a.cfg.n;
  for (int t = 0; t < c.p.a.T; ++t) {
    float m[3], s[3];
    plan_mean(c.p, i, t, m);
    cem_std(c, i, t, s);
    float cv[3] = {m[0], m[1], m[2]};
    if (k > 0) cem_candidate(c.p, i, (uint32_t)k, (uint32_t)t, m, s, cv);
    float* dst = act_out + (((size_t)k * c.p.a.T + t) * n + i) * 3;
    dst[0] = cv[0];
    dst[1] = cv[1];
    dst[2] = cv[2];
  }
}

namespace hostside {

constexpr int kCemMaxK = EARL_CEM_MAX_K;

// the MPPI block the shared rules (check_plan, check_mpc, plan_args) read, out of a CEM block; the temperature is a constant they accept
inline earl_plan_params cem_plan_params(const earl_cem_params* c) {
  earl_plan_params p{};
  p.K = c->K;
  p.H = c->H;
  p.iterations = c->iterations;
  p.iteration0 = c->iteration0;
  for (int d = 0; d < 3; ++d) p.sigma[d] = c->sigma[d];
  p.noise_counter = c->noise_counter;
  p.inv_temperature = 1.0;
  return p;
}

// the ranges of earl_cem_params beyond what check_plan tests; `update`: the calls that select elites (not earl_tabletop_cem_candidates, which reads neither)
inline int check_cem_params(const earl_cem_params* c, bool update) {
  if (c->K > kCemMaxK) return fail(EARL_ERR_ARG, "K = %d > %d: the elite masks of an update workgroup stay in LDS", c->K, kCemMaxK);
  if (update && (c->elites < 1 || c->elites > c->K)) return fail(EARL_ERR_ARG, "elites = %d: 1 .. K = %d", c->elites, c->K);
  if (update && (!std::isfinite(c->alpha) || !(c->alpha >= 0.0f && c->alpha < 1.0f))) return fail(EARL_ERR_ARG, "alpha = %g: finite, 0 <= alpha < 1", (double)c->alpha);
  if (!std::isfinite(c->std_min) || !std::isfinite(c->std_max) || !(c->std_min >= 0.0f && c->std_min <= c->std_max))
    return fail(EARL_ERR_ARG, "std_min = %g, std_max = %g: finite, 0 <= std_min <= std_max", (double)c->std_min, (double)c->std_max);
  return EARL_OK;
}

// The argument rules of earl_tabletop[3]_plan_cem and of earl_tabletop_cem_candidates (st == NULL, j = the iteration, `plan` = act_out, no std output) and of their
// host twins: MPPI's (check_plan) and the header's own.  pv: NULL or the `_value` block's rules.
inline int check_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int nobj, int obs_dim, const earl_cem_params* c, const earl_plan_value* pv, int32_t j,
                     const float* mean, const float* std0, const void* plan, const float* std_out, const double* ret, long long* blocks, long long* ublocks) {
  *blocks = *ublocks = 0;
  if (!c) return fail(EARL_ERR_ARG, "params is NULL");
  const earl_plan_params pp = cem_plan_params(c);
  long long nb, ub;
  if (int rc = check_plan(cfg, st, nobj, &pp, j, mean, plan, ret, &nb, &ub)) return rc;
  if (int rc = check_cem_params(c, st != nullptr)) return rc;
  if (st) {
    if (pv)
      if (int rc = check_plan_value(pv, obs_dim)) return rc;
    if (!std_out) return fail(EARL_ERR_ARG, "std is NULL: it is the workspace between iterations and a result");
  }
  const uintptr_t bytes = (uintptr_t)c->H * (uintptr_t)cfg->n * 12u;
  const void* arr[4] = {mean, st ? plan : nullptr, std0, std_out};   // allowed to coincide: (mean, plan) and (std0, std)
  for (int x = 0; x < 4; ++x)
    for (int y = x + 1; y < 4; ++y) {
      if (!arr[x] || !arr[y]) continue;
      const uintptr_t a = (uintptr_t)arr[x], b = (uintptr_t)arr[y];
      const bool pair = (x == 0 && y == 1) || (x == 2 && y == 3);
      if (pair && a == b) continue;
      if (a < b + bytes && b < a + bytes) return fail(EARL_ERR_ARG, "mean, std0, plan and std overlap beyond plan == mean and std == std0");
    }
  *blocks = nb;
  *ublocks = ub;
  return EARL_OK;
}

inline CemArgs cem_args(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* c, const earl_plan_value* pv, const float* mean,
                        const float* std0, const Thresholds& th) {
  CemArgs x{};
  const earl_plan_params pp = cem_plan_params(c);
  x.p = plan_args(cfg, st, &pp, mean, th);
  x.std_in = std0;
  x.v = pv ? value_args(pv) : ValueArgs{1.0, earl_mlp_policy{}};
  x.E = c->elites;
  x.alpha = c->alpha;
  x.std_min = c->std_min;
  x.std_max = c->std_max;
  return x;
}

// the rules of earl_tabletop[3]_mpc_rollout_cem and of its twin: check_mpc's with the CEM block, and the block's own.  *lanes = the workgroup's size (0: nothing to do)
inline int check_cem_mpc(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int nobj, const earl_cem_params* c, const earl_plan_value* pv, int32_t T,
                         const earl_tabletop_out* out, const earl_mpc_out* mpc, int* lanes) {
  *lanes = 0;
  if (!c) return fail(EARL_ERR_ARG, "params is NULL");
  const earl_plan_params pp = cem_plan_params(c);
  int wg;
  if (int rc = check_mpc(cfg, st, nobj, &pp, T, out, mpc, &wg)) return rc;
  if (int rc = check_cem_params(c, true)) return rc;
  // the three-object auto-reset kernel with the value network inside spills 12 bytes per lane at 128 VGPRs under 1024-lane workgroups: refused, not shipped
  if (pv) return fail(EARL_ERR_ARG, "pv != NULL: the receding-horizon CEM loop has no value build (compose earl_tabletop[3]_plan_cem and the one-step rollout)");
  *lanes = wg;
  return EARL_OK;
}

inline CemMpcArgs cem_mpc_args(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* c, int32_t T,
                               const earl_tabletop_out* out, const earl_mpc_out* mpc) {
  CemMpcArgs x{};
  const earl_plan_params pp = cem_plan_params(c);
  x.x = mpc_args(cfg, st, &pp, T, out, mpc);
  x.E = c->elites;
  x.alpha = c->alpha;
  x.std_min = c->std_min;
  x.std_max = c->std_max;
  return x;
}

}  // namespace hostside
}  // namespace earl

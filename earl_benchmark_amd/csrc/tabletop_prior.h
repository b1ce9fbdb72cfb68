// tabletop_prior.h -- the policy-prior branches of earl_tabletop[3]_plan_mppi_prior (include/earl_tabletop.h, "MPPI with policy-prior branches"): what a lane that owns
// one PRIOR (branch, env) runs on top of tabletop_plan.h's planner, and what the update reads back.  Shared by the gfx950 kernels (tabletop_prior.hip) and the host twin
// (tabletop_host.cpp, the same text under -DEARL_HOST_BUILD).
//
// prior_forward      u = pi(o) on the lane's OWN observation row, in registers: tabletop_value.h's scheme (its chains, its weight pointer, its multiply-add) with
//                    THREE outputs.  Every lane of a wave reads the same W_jk through the constant address space, so a wave-uniform address is a scalar load; four
//                    chains at a time share every x_k; the last hidden layer is streamed into three accumulators, j ascending -- the contract's order -- and never
//                    stored; the first layer of a two-hidden-layer net is held in kPriorMaxH1 registers as value_forward holds it.
// prior_candidate    item 2 for 1 <= k <= P: the SAME Philox block as plan_candidate (same word 0, no new draw id), around u instead of the mean.
// prior_score_body   plan_score_body's loop (same state loads, same wrapped_step, same counters) with prior_forward on the row `o` before each step and one 12-byte
//                    store per step into prior->act.  Unlike the value network the policy runs INSIDE the look-ahead loop, so the row stays live through it: with
//                    VALUE the terminal value is taken on that row (what plan_score_body makes again after its loop: the same row by wrapped_step's contract).
//                    The mean is not read: a prior branch does not depend on it.
// prior_accumulate   item 5 for k <= P: the candidate read back from prior->act.
#pragma once
#include "tabletop_hostside.h"
#include "tabletop_plan.h"

namespace earl {

constexpr int kPriorMaxH1 = EARL_PLAN_PRIOR_MAX_H1;   // the widest first hidden layer of a two-hidden-layer prior (held in registers through the network)
static_assert(kPriorMaxH1 == 16, "prior_forward holds one tile of 16");

// what a `_prior` launch carries beside the planner's block and the value block.  P == 0: net and act unused
struct PriorArgs {
  earl_mlp_policy net;
  float sigma[3];
  int32_t P;
  float* act;   // [P, H, n, 3]
};
struct PlanPriorArgs : PlanValueArgs {
  PriorArgs pr;
};

template <int NOBS>
__device__ __forceinline__ void prior_forward(const earl_mlp_policy& net, const float (&x)[NOBS], float (&u)[3]) {
#pragma clang fp contract(off)
  const value_wptr W0 = (value_wptr)(uintptr_t)net.params;   // [H1][NOBS]
  const int H1 = net.dims[1], hact = net.hidden_act;
  const value_wptr b0 = W0 + (size_t)H1 * NOBS;
  float a0, a1, a2;
  if (net.n_layers == 2) {                            // NOBS -> H1 -> 3: nothing held
    const value_wptr Wo0 = b0 + H1, Wo1 = Wo0 + H1, Wo2 = Wo1 + H1;   // [3][H1]
    a0 = Wo2[H1];
    a1 = Wo2[H1 + 1];
    a2 = Wo2[H1 + 2];
#pragma unroll 1
    for (int j = 0; j < H1; j += 4) {
      float r0 = b0[j], r1 = b0[j + 1], r2 = b0[j + 2], r3 = b0[j + 3];
      const value_wptr w = W0 + (size_t)j * NOBS;
      value_chains<0, NOBS>(x, w, w + NOBS, w + 2 * NOBS, w + 3 * NOBS, r0, r1, r2, r3);
      const float h[4] = {policy_act(r0, hact), policy_act(r1, hact), policy_act(r2, hact), policy_act(r3, hact)};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        a0 = __builtin_fmaf(h[c], Wo0[j + c], a0);
        a1 = __builtin_fmaf(h[c], Wo1[j + c], a1);
        a2 = __builtin_fmaf(h[c], Wo2[j + c], a2);
      }
    }
  } else {                                            // NOBS -> H1 (= 16) -> H2 -> 3: h1 held, the second hidden layer streamed
    float h1[kPriorMaxH1];
#pragma unroll
    for (int c = 0; c < 16; ++c) h1[c] = 0.0f;
#pragma unroll 1
    for (int j = 0; j < 16; j += 4) {                 // (the rotation of value_forward: no register array indexed by the runtime j)
      float r0 = b0[j], r1 = b0[j + 1], r2 = b0[j + 2], r3 = b0[j + 3];
      const value_wptr w = W0 + (size_t)j * NOBS;
      value_chains<0, NOBS>(x, w, w + NOBS, w + 2 * NOBS, w + 3 * NOBS, r0, r1, r2, r3);
#pragma unroll
      for (int c = 0; c < 12; ++c) h1[c] = h1[c + 4];
      h1[12] = policy_act(r0, hact);
      h1[13] = policy_act(r1, hact);
      h1[14] = policy_act(r2, hact);
      h1[15] = policy_act(r3, hact);
    }
    const int H2 = net.dims[2];
    const value_wptr W1 = b0 + H1;                    // [H2][H1]
    const value_wptr b1 = W1 + (size_t)H2 * H1;
    const value_wptr Wo0 = b1 + H2, Wo1 = Wo0 + H2, Wo2 = Wo1 + H2;   // [3][H2]
    a0 = Wo2[H2];
    a1 = Wo2[H2 + 1];
    a2 = Wo2[H2 + 2];
#pragma unroll 1
    for (int j = 0; j < H2; j += 2) {
      float r0 = b1[j], r1 = b1[j + 1];
      const value_wptr w0 = W1 + (size_t)j * H1, w1 = w0 + H1;
      value_chains2<0, 16>(h1, w0, w1, r0, r1);
      const float h[2] = {policy_act(r0, hact), policy_act(r1, hact)};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        a0 = __builtin_fmaf(h[c], Wo0[j + c], a0);
        a1 = __builtin_fmaf(h[c], Wo1[j + c], a1);
        a2 = __builtin_fmaf(h[c], Wo2[j + c], a2);
      }
    }
  }
  u[0] = policy_act(a0, net.out_act);
  u[1] = policy_act(a1, net.out_act);
  u[2] = policy_act(a2, net.out_act);
}

// item 2, 1 <= k <= P: plan_candidate's Philox block and quantiles around the policy's action; a NaN of u clips to -1
__device__ __forceinline__ void prior_candidate(const PlanPriorArgs& p, int i, uint32_t k, uint32_t t, const float (&u)[3], float (&c)[3]) {
  const U4 b = philox4x32_10(U4{p.word0, (uint32_t)(p.a.cfg.env_offset + i), (k << 16) | t, p.noise_counter}, (uint32_t)p.a.cfg.seed,
                             (uint32_t)(p.a.cfg.seed >> 32));
  c[0] = plan_clip(fmaf(p.pr.sigma[0], normal_quantile_f32(b.x >> 8), u[0]));
  c[1] = plan_clip(fmaf(p.pr.sigma[1], normal_quantile_f32(b.y >> 8), u[1]));
  c[2] = plan_clip(fmaf(p.pr.sigma[2], normal_quantile_f32(b.z >> 8), u[2]));
}

__device__ __forceinline__ float* prior_row(const PlanPriorArgs& p, int i, uint32_t k, uint32_t t) {
  return p.pr.act + (((size_t)(k - 1) * (size_t)p.a.T + t) * (size_t)p.a.cfg.n + (size_t)i) * 3;
}

// item 3 of prior branch k (1 <= k <= P) of env i
template <int NOBJ, bool GENERAL, bool VALUE>
__device__ __forceinline__ void prior_score_body(const PlanPriorArgs& p, int i, int k) {
  const KArgs& a = p.a;
  Lane<NOBJ> L;
  load_lane<NOBJ>(a, i, L);
  float g[Dims<NOBJ>::NG];
  load_goal<NOBJ>(a.st.goal_table, L.goal_idx, g);
  double ret = 0.0;
  [[maybe_unused]] double disc = 1.0;
  float o[Dims<NOBJ>::NOBS];
  make_obs<NOBJ>(L.e, g, o);                          // x_0: _get_obs() of the incoming state
#pragma unroll 1
  for (int t = 0; t < a.T; ++t) {
    float u[3], c[3];
    prior_forward<Dims<NOBJ>::NOBS>(p.pr.net, o, u);
    prior_candidate(p, i, (uint32_t)k, (uint32_t)t, u, c);
    float* dst = prior_row(p, i, (uint32_t)k, (uint32_t)t);
    dst[0] = c[0];
    dst[1] = c[1];
    dst[2] = c[2];
    float reward;
    bool done, succ;
    wrapped_step<NOBJ, GENERAL>(a, i, a.cfg.counter + (uint64_t)t, L, g, c[0], c[1], c[2], o, reward, done, succ);
    if constexpr (VALUE) value_accumulate(ret, disc, reward, p.v.discount);
    else ret += (double)reward;
  }
  if constexpr (VALUE) ret = value_terminal<Dims<NOBJ>::NOBS>(p.v, o, ret, disc);
  p.ret[(size_t)k * a.cfg.n + i] = ret;
}

// item 5, 1 <= k <= P: the candidate read back
__device__ __forceinline__ void prior_accumulate(const PlanPriorArgs& p, int i, uint32_t k, uint32_t t, const float (&m)[3], int32_t W, int64_t (&A)[3]) {
  const float* c = prior_row(p, i, k, t);
#pragma unroll
  for (int d = 0; d < 3; ++d) A[d] += (int64_t)W * (int64_t)(int32_t)__builtin_rint((double)(c[d] - m[d]) * 1048576.0);   // |D| <= 2^21: both in [-1, 1]
}

namespace hostside {

// What earl_tabletop[3]_plan_mppi_prior and its twin refuse beyond check_plan / check_plan_value (called after them: cfg and pp are valid)
inline int check_plan_prior(const earl_tabletop_cfg* cfg, const earl_plan_params* pp, const earl_plan_prior* pr, int obs_dim, const float* mean, const float* plan,
                            const double* ret) {
  if (!pr) return fail(EARL_ERR_ARG, "prior block is NULL (earl_tabletop[3]_plan_mppi is the call without one)");
  if (pr->branches < 0 || pr->branches >= pp->K) return fail(EARL_ERR_ARG, "prior branches = %d: 0 .. K - 1 = %d (branch 0 is the plan itself)", pr->branches, pp->K - 1);
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(pr->sigma[d]) || !(pr->sigma[d] >= 0)) return fail(EARL_ERR_ARG, "prior sigma[%d] = %g: finite and >= 0", d, (double)pr->sigma[d]);
  if (pr->branches == 0) return EARL_OK;
  if (!pr->policy || !pr->act) return fail(EARL_ERR_ARG, "prior policy/act is NULL with %d prior branches", pr->branches);
  if (int rc = contract::check_policy(*pr->policy, obs_dim, 3, nullptr, 0, g_err)) return rc;
  if (pr->policy->n_layers == 3 && pr->policy->dims[1] > kPriorMaxH1)
    return fail(EARL_ERR_ARG, "prior policy: first hidden width %d of two > %d (a lane holds that layer in registers)", pr->policy->dims[1], kPriorMaxH1);
  const uintptr_t rows = (uintptr_t)pp->H * (uintptr_t)cfg->n * 12u, a = (uintptr_t)pr->act, ab = rows * (uintptr_t)pr->branches;
  const uintptr_t other[3] = {(uintptr_t)mean, (uintptr_t)plan, (uintptr_t)ret}, bytes[3] = {rows, rows, (uintptr_t)pp->K * (uintptr_t)cfg->n * 8u};
  for (int e = 0; e < 3; ++e)
    if (a < other[e] + bytes[e] && other[e] < a + ab) return fail(EARL_ERR_ARG, "prior act overlaps %s", e == 0 ? "mean" : e == 1 ? "plan" : "ret");
  return EARL_OK;
}

inline PriorArgs prior_args(const earl_plan_prior* pr) {
  PriorArgs x{};
  if (pr->branches > 0) x.net = *pr->policy;
  for (int d = 0; d < 3; ++d) x.sigma[d] = pr->sigma[d];
  x.P = pr->branches;
  x.act = pr->act;
  return x;
}

}  // namespace hostside
}  // namespace earl

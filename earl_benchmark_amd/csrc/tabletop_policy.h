// tabletop_policy.h -- the closed-loop tabletop rollout: a float32 MLP policy 12 -> hidden (-> hidden) -> 3 evaluated between the env steps of ONE
// launch (include/earl_tabletop.h: earl_tabletop_policy_rollout).  Shared by the gfx950 kernel (tabletop_policy.hip) and its host twin
// (tabletop_host.cpp, -DEARL_HOST_BUILD); the per-env step is tabletop_step.h's wrapped_step<1, GENERAL>, not restated here.  The same kernel with a
// Gaussian head (12 -> hidden (-> hidden) -> 6, actions sampled inside the launch: earl_tabletop_policy_rollout_gaussian) is instantiated in
// tabletop_policy_gaussian.hip; its sampling contract follows the deterministic one below.  Both heads for a POPULATION of policies (every 16-env workgroup its own
// member's parameters) with per-episode summaries (earl_tabletop_population_rollout) are instantiated in tabletop_policy_population.hip; the kernel body the
// three units share is tabletop_policy_kernel.inc.  The THREE-object env's closed loop (20 -> hidden (-> hidden) -> 3 or 6, one policy or a population, summaries:
// earl_tabletop3_policy_rollout) is the same body with NOBJ = 3, instantiated in tabletop3_policy.hip; the env's side below (policy_episode_begin, policy_env_step) and the host
// twin's loops take the object count as a template argument.  The agent pair's env side (pair_env_step and its neighbours) takes it too, and so does its kernel, one text
// for both envs (tabletop_pair_kernel.h): earl_tabletop_pair_rollout is its NOBJ = 1 in tabletop_policy_pair.hip, earl_tabletop3_pair_rollout its NOBJ = 3 in tabletop3_pair.hip.
//
// The policy arithmetic is a contract, stated here once for both builds:
//   pre-activation   acc = b_j;  for k = 0 .. K-1 ascending:  acc = fmaf(x_k, W_jk, acc)     (float32, one rounding per fused multiply-add)
//   ReLU             acc > 0 ? acc : +0                                                     (= fmaxf(acc, 0) with -0 -> +0 and NaN -> 0 pinned)
//   tanh             tanh_f32 (policy_math.h, with the Gaussian head's arithmetic)
// On gfx950 the chain is v_mfma_f32_16x16x4_f32: per output element bit for bit a k-ordered fmaf chain, C input = the bias.  The host states the loops.
// Held on the device by tests/test_policy_widths_gpu.py: every instantiation (NT2 x GENERAL x head x POP, and the pair's) and every hidden width 16 .. 256 at
// every layer position against the host twin bit for bit, the wide shapes also against an exact integer reference (the lane maps).
#pragma once
#include "policy_check.h"
#include "policy_math.h"
#include "tabletop_hostside.h"
#include "tabletop_step.h"

namespace earl {

constexpr int kPolicyEnvsPerWg = 16;   // the M of 16x16x4

// ------------------------------------------------------------------------------------------------
// arguments
// ------------------------------------------------------------------------------------------------
struct PolicyArgs {
  KArgs k;              // cfg / state / outputs / thresholds; k.T = steps per episode; k.act unused
  earl_mlp_policy p;
  float* act_out;
  int32_t episodes;
  int32_t reset_first;
};
struct GaussianPolicyArgs : PolicyArgs {   // the deterministic kernels keep PolicyArgs as their kernel argument
  earl_gaussian_head head;
};
template <bool GAUSS>
struct PolicyArgsOf { using type = PolicyArgs; };
template <>
struct PolicyArgsOf<true> { using type = GaussianPolicyArgs; };
// earl_tabletop_population_rollout: both heads take this one (head unused without GAUSS).  pop.envs_per_policy == 0 = one policy (pop was NULL)
struct PopulationArgs : GaussianPolicyArgs {
  earl_policy_population pop;
  earl_episode_summary sum;
};
// earl_tabletop_pair_rollout / earl_tabletop3_pair_rollout: both heads take this one (head unused without one).  p.params is [2, pair.param_stride]
struct PairArgs : GaussianPolicyArgs {
  earl_agent_pair pair;
};
// the widest second hidden layer of an agent pair: two weight sets share the 512 registers of one wave per SIMD (tabletop_pair_kernel.h has the table)
constexpr int kPairMaxH2 = EARL_PAIR_MAX_H2;
// the per-episode summary of one env, kept in registers over the T steps (earl_episode_summary)
struct EpisodeSum {
  double ret;
  int32_t first;
  bool last;
};
__host__ __device__ __forceinline__ void episode_sum_begin(EpisodeSum& s) { s.ret = 0.0; s.first = -1; s.last = false; }
__host__ __device__ __forceinline__ void episode_sum_step(EpisodeSum& s, int t, float reward, bool succ) {
  s.ret += (double)reward;
  if (succ && s.first < 0) s.first = t;
  s.last = succ;
}
__host__ __device__ __forceinline__ void episode_sum_store(const earl_episode_summary& d, size_t row, const EpisodeSum& s) {
  if (d.ret) d.ret[row] = s.ret;
  if (d.success_last) d.success_last[row] = s.last;
  if (d.first_success) d.first_success[row] = s.first;
}

namespace hostside {

// the deterministic entry point (h == NULL: a 3-wide last layer) or the Gaussian head's (6-wide, then the head's rules): the env's checks, the policy's
// (policy_check.h), the launch's own.  nobj = 3: the three-object env's (earl_tabletop3_policy_rollout), 20 observations wide
inline int check_policy(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, const earl_gaussian_head* h, int32_t episodes, int32_t T,
                        int32_t reset_first, const earl_tabletop_out* out, int nobj = 1) {
  static_assert(sizeof g_err >= contract::kErrLen, "policy_check.h writes its messages into g_err");
  if (int rc = check_common(cfg, st, nobj)) return rc;
  if (!p || !out) return fail(EARL_ERR_ARG, "policy/out is NULL");
  if (int rc = contract::check_policy(*p, nobj == 3 ? EARL_TABLETOP3_OBS_DIM : EARL_TABLETOP_OBS_DIM, EARL_TABLETOP_ACT_DIM, h, 0, g_err)) return rc;
  if (T < 1) return fail(EARL_ERR_ARG, "T = %d < 1", T);
  if (episodes < 1) return fail(EARL_ERR_ARG, "episodes = %d < 1", episodes);
  if (reset_first != 0 && reset_first != 1) return fail(EARL_ERR_ARG, "reset_first = %d", reset_first);
  if (!reset_first && episodes != 1) return fail(EARL_ERR_ARG, "episodes = %d without reset_first: a continuing rollout is one episode", episodes);
  return EARL_OK;
}

// the Gaussian-head entry points: the head is not optional
inline int check_policy_gaussian(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, const earl_gaussian_head* h,
                                 int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out) {
  if (!h) return fail(EARL_ERR_ARG, "head is NULL");
  return check_policy(cfg, st, p, h, episodes, T, reset_first, out);
}

// earl_tabletop_population_rollout: the checks of the head's single-policy entry point, then the population's (one member per 16-env workgroup, any stride)
inline int check_population(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, const earl_policy_population* pop,
                            const earl_gaussian_head* h, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, int nobj = 1) {
  if (int rc = check_policy(cfg, st, p, h, episodes, T, reset_first, out, nobj)) return rc;
  return pop ? contract::check_population(*p, *pop, cfg->env_offset, cfg->n, kPolicyEnvsPerWg, 1, g_err) : EARL_OK;
}

inline PopulationArgs population_args(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, const earl_policy_population* pop,
                                      const earl_gaussian_head* h, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out,
                                      const earl_episode_summary* sum, const Thresholds& th) {
  PopulationArgs a;
  static_cast<PolicyArgs&>(a) = PolicyArgs{KArgs{*cfg, *st, *out, nullptr, nullptr, nullptr, nullptr, T, th}, *p, act_out, episodes, reset_first};
  a.head = h ? *h : contract::default_head();
  a.pop = pop ? *pop : earl_policy_population{1, 0, 0};
  a.sum = sum ? *sum : earl_episode_summary{nullptr, nullptr, nullptr};
  return a;
}

// earl_tabletop_pair_rollout (nobj = 3: earl_tabletop3_pair_rollout): the checks of the head's single-policy entry point, then the pair's (any stride) and the register
// budget of two weight sets
inline int check_pair(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, const earl_agent_pair* pair, const earl_gaussian_head* h,
                      int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, int nobj = 1) {
  if (int rc = check_policy(cfg, st, p, h, episodes, T, reset_first, out, nobj)) return rc;
  if (int rc = contract::check_pair(*p, pair, cfg->goal_change_frequency, 1, g_err)) return rc;
  if (p->n_layers == 3 && p->dims[2] > kPairMaxH2)
    return fail(EARL_ERR_ARG, "pair: second hidden width %d > EARL_PAIR_MAX_H2 = %d (two weight sets in one wave's registers)", p->dims[2], kPairMaxH2);
  return EARL_OK;
}

inline PairArgs pair_args(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, const earl_agent_pair* pair, const earl_gaussian_head* h,
                          int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out, const Thresholds& th,
                          [[maybe_unused]] int nobj = 1) {      // (nobj: not read -- PairArgs has no width of its own; taken so that the call reads as check_pair's)
  PairArgs a;
  static_cast<PolicyArgs&>(a) = PolicyArgs{KArgs{*cfg, *st, *out, nullptr, nullptr, nullptr, nullptr, T, th}, *p, act_out, episodes, reset_first};
  a.head = h ? *h : contract::default_head();
  a.pair = *pair;
  return a;
}

}  // namespace hostside

// the member of a population that the env with global id `gid` runs, as an offset into policy->params
__host__ __device__ __forceinline__ size_t population_param_offset(const earl_policy_population& pop, int gid) {
  return pop.envs_per_policy > 0 ? (size_t)(gid / pop.envs_per_policy) * (size_t)pop.param_stride : 0;
}

// the env's side of one closed-loop launch, shared by the kernel's env lanes and the host loop: what happens to ONE env before episode e's first step
// (reset_body's reset on register state, or nothing) and the observation the first action is computed from
template <bool GENERAL, int NOBJ>
__device__ __forceinline__ void policy_episode_begin(const PolicyArgs& a, int i, int e, Lane<NOBJ>& L, float (&g)[Dims<NOBJ>::NG], float (&o)[Dims<NOBJ>::NOBS]) {
  if (a.reset_first) {                              // reset_body: Philox counter of episode e's reset = cfg.counter + e (T + 1)
    L.goal_idx = reset_env<NOBJ>(L.e, a.k.cfg, a.k.cfg.counter + (uint64_t)e * (uint64_t)(a.k.T + 1), i, a.k.st.goal_table, nullptr, a.k.th);
    L.steps = 0;
    L.sgc = 0;
    L.resets += 1;
    load_goal<NOBJ>(a.k.st.goal_table, L.goal_idx, g);
  }
  make_obs<NOBJ>(L.e, g, o);
}

// the Philox counter of step t of episode e: what wrapped_step gets, and what keys the Gaussian head's draw of that step
__device__ __forceinline__ uint64_t policy_step_counter(const PolicyArgs& a, int e, int t) {
  return a.k.cfg.counter + (uint64_t)e * (uint64_t)(a.k.T + 1) + (uint64_t)(a.reset_first ? 1 : 0) + (uint64_t)t;
}

// one closed-loop step of one env given the policy's action (a0, a1, a2): act_out, wrapped_step, outputs
template <bool GENERAL, int NOBJ>
__device__ __forceinline__ void policy_env_step(const PolicyArgs& a, int i, int e, int t, Lane<NOBJ>& L, float (&g)[Dims<NOBJ>::NG], float a0, float a1, float a2,
                                                float (&o)[Dims<NOBJ>::NOBS], float& reward, bool& succ) {
  const size_t row = ((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)i;
  if (a.act_out) {
    float* ap = a.act_out + row * 3;
    ap[0] = a0; ap[1] = a1; ap[2] = a2;
  }
  const uint64_t counter = policy_step_counter(a, e, t);
  bool done;
  wrapped_step<NOBJ, GENERAL>(a.k, i, counter, L, g, a0, a1, a2, o, reward, done, succ);
  if (a.k.out.obs) store_obs<NOBJ>(a.k.out.obs + row * Dims<NOBJ>::NOBS, o);
  if (a.k.out.reward) a.k.out.reward[row] = reward;
  if (a.k.out.done) a.k.out.done[row] = done;
  if (a.k.out.success) a.k.out.success[row] = succ;
}
template <bool GENERAL, int NOBJ>
__device__ __forceinline__ void policy_env_step(const PolicyArgs& a, int i, int e, int t, Lane<NOBJ>& L, float (&g)[Dims<NOBJ>::NG], float a0, float a1, float a2,
                                                float (&o)[Dims<NOBJ>::NOBS]) {
  float reward;
  bool succ;
  policy_env_step<GENERAL>(a, i, e, t, L, g, a0, a1, a2, o, reward, succ);
}

// ------------------------------------------------------------------------------------------------
// The agent pair (include/earl_tabletop.h: earl_tabletop_pair_rollout; NOBJ = 3: earl_tabletop3_pair_rollout), the env's side, shared by the kernel's env lanes
// (tabletop_pair_kernel.h) and the host loop: the phase state of one env and what a step does to it.  The order of pair_env_step IS the contract of record's items 3 .. 6.
// ------------------------------------------------------------------------------------------------
struct PairLane {
  int phase;   // 0 forward, 1 reset
  int sip;     // steps in phase
  int fs, bs;  // forward / reset phases of this episode that ended by success
};

// the goal in force: the reset agent's row if there is one, otherwise the env's stored task goal.  NOBJ = 3 (earl_tabletop3_pair_rollout): a 10-wide row
template <int NOBJ = 1>
__device__ __forceinline__ void pair_goal(const PairArgs& a, const Lane<NOBJ>& L, int phase, float (&g)[Dims<NOBJ>::NG]) {
  if (phase && a.pair.backward_goal) {
#pragma unroll
    for (int k = 0; k < Dims<NOBJ>::NG; ++k) g[k] = (float)a.pair.backward_goal[k];
  } else {
    load_goal<NOBJ>(a.k.st.goal_table, L.goal_idx, g);
  }
}

template <int NOBJ = 1>
__device__ __forceinline__ void pair_load(const PairArgs& a, int i, const Lane<NOBJ>& L, PairLane& P, float (&g)[Dims<NOBJ>::NG]) {
  P.phase = a.pair.phase[i] != 0;
  P.sip = a.pair.steps_in_phase[i];
  P.fs = 0;
  P.bs = 0;
  pair_goal<NOBJ>(a, L, P.phase, g);
}

// episode e's begin: policy_episode_begin, and a reset puts the env into the forward phase
template <int NOBJ = 1>
__device__ __forceinline__ void pair_episode_begin(const PairArgs& a, int i, int e, Lane<NOBJ>& L, PairLane& P, float (&g)[Dims<NOBJ>::NG],
                                                   float (&o)[Dims<NOBJ>::NOBS]) {
  if (a.reset_first) {
    P.phase = 0;
    P.sip = 0;
  }
  P.fs = 0;
  P.bs = 0;
  policy_episode_begin<true>(a, i, e, L, g, o);
}

template <int NOBJ = 1>      // (not used: the counters have no width; a template like its neighbours so that a caller names the object count throughout)
__device__ __forceinline__ void pair_episode_end(const PairArgs& a, int i, int e, const PairLane& P) {
  const size_t row = (size_t)e * (size_t)a.k.cfg.n + (size_t)i;
  if (a.pair.forward_success) a.pair.forward_success[row] = P.fs;
  if (a.pair.backward_success) a.pair.backward_success[row] = P.bs;
}

template <int NOBJ = 1>
__device__ __forceinline__ void pair_store(const PairArgs& a, int i, const Lane<NOBJ>& L, const PairLane& P) {
  store_lane<NOBJ>(a.k, i, L);
  a.k.st.goal_idx[i] = L.goal_idx;                  // (store_lane writes it under lifelong / reset only)
  a.pair.phase[i] = (int8_t)P.phase;
  a.pair.steps_in_phase[i] = P.sip;
}

// one closed-loop step of one env given ITS agent's action: agent_out, act_out, wrapped_step, the handover, outputs
template <int NOBJ = 1>
__device__ __forceinline__ void pair_env_step(const PairArgs& a, int i, int e, int t, Lane<NOBJ>& L, PairLane& P, float (&g)[Dims<NOBJ>::NG], float a0, float a1,
                                              float a2, float (&o)[Dims<NOBJ>::NOBS]) {
  constexpr int NG = Dims<NOBJ>::NG, NOBS = Dims<NOBJ>::NOBS;      // the goal slots of the observation: o[NOBS - NG ..] = o[NQ + 2 ..]
  const size_t row = ((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)i;
  if (a.pair.agent_out) a.pair.agent_out[row] = (int8_t)P.phase;
  if (a.act_out) {
    float* ap = a.act_out + row * 3;
    ap[0] = a0; ap[1] = a1; ap[2] = a2;
  }
  const uint64_t counter = policy_step_counter(a, e, t);
  const int resets = L.resets;
  float reward;
  bool done, succ;
  wrapped_step<NOBJ, true>(a.k, i, counter, L, g, a0, a1, a2, o, reward, done, succ);
  if (L.resets != resets) {                         // auto-reset: back to the forward agent (g is the new task goal already), nothing else
    P.phase = 0;
    P.sip = 0;
  } else {
    P.sip += 1;
    const bool by_success = a.pair.switch_on_success && succ;
    if (by_success || P.sip >= (P.phase ? a.pair.switch_every[1] : a.pair.switch_every[0])) {
      if (by_success) {
        if (P.phase) P.bs += 1;
        else P.fs += 1;
      }
      P.phase ^= 1;
      P.sip = 0;
      if (P.phase == 0) L.goal_idx = sample_goal(a.k.cfg, counter, i, nullptr);      // the draw the lifelong switch makes
      if (P.phase == 0 || a.pair.backward_goal) {
        pair_goal<NOBJ>(a, L, P.phase, g);
#pragma unroll
        for (int k = 0; k < NG; ++k) o[NOBS - NG + k] = g[k];                          // obs re-read with the new goal
      }
    }
  }
  if (a.k.out.obs) store_obs<NOBJ>(a.k.out.obs + row * NOBS, o);
  if (a.k.out.reward) a.k.out.reward[row] = reward;
  if (a.k.out.done) a.k.out.done[row] = done;
  if (a.k.out.success) a.k.out.success[row] = succ;
}

#ifdef EARL_HOST_BUILD
// ------------------------------------------------------------------------------------------------
// host twin: the MLP as the plain loops of the contract, one env at a time
// ------------------------------------------------------------------------------------------------
inline void mlp_layers(const earl_mlp_policy& p, const float* params, const float* x, float* act, int last_act) {      // x: the p.dims[0] inputs
  float h[2][kPolicyMaxWidth];
  const float* in = x;
  const float* w = params;
  for (int l = 0; l < p.n_layers; ++l) {
    const int K = p.dims[l], N = p.dims[l + 1];
    const float* b = w + (size_t)N * K;
    const int kind = l + 1 < p.n_layers ? p.hidden_act : last_act;
    float* dst = l + 1 < p.n_layers ? h[l & 1] : act;
    for (int j = 0; j < N; ++j) {
      float acc = b[j];
      for (int k = 0; k < K; ++k) acc = fmaf(in[k], w[(size_t)j * K + k], acc);
      dst[j] = policy_act(acc, kind);
    }
    in = dst;
    w = b + N;
  }
}
inline void mlp_forward(const earl_mlp_policy& p, const float* params, const float* x, float (&act)[3]) { mlp_layers(p, params, x, act, p.out_act); }

// `params`: the parameters this env runs (a population: its member's); `sum`: NULL or the per-episode summary arrays
template <bool GENERAL, int NOBJ = 1>
inline void policy_rollout_env(const PolicyArgs& a, int i, const float* params, const earl_episode_summary* sum = nullptr) {
  Lane<NOBJ> L;
  load_lane<NOBJ>(a.k, i, L);
  float g[Dims<NOBJ>::NG], o[Dims<NOBJ>::NOBS];
  load_goal<NOBJ>(a.k.st.goal_table, L.goal_idx, g);
  for (int e = 0; e < a.episodes; ++e) {
    policy_episode_begin<GENERAL>(a, i, e, L, g, o);
    EpisodeSum es;
    episode_sum_begin(es);
    for (int t = 0; t < a.k.T; ++t) {
      float act[3], reward;
      bool succ;
      mlp_forward(a.p, params, o, act);
      policy_env_step<GENERAL>(a, i, e, t, L, g, act[0], act[1], act[2], o, reward, succ);
      episode_sum_step(es, t, reward, succ);
    }
    if (sum) episode_sum_store(*sum, (size_t)e * (size_t)a.k.cfg.n + (size_t)i, es);
  }
  store_lane<NOBJ>(a.k, i, L);
}

// the Gaussian head: the 6-wide last layer without activation, then the contract's head per dimension
template <bool GENERAL, int NOBJ = 1>
inline void gaussian_rollout_env(const GaussianPolicyArgs& a, int i, const float* params, const earl_episode_summary* sum = nullptr) {
  Lane<NOBJ> L;
  load_lane<NOBJ>(a.k, i, L);
  float g[Dims<NOBJ>::NG], o[Dims<NOBJ>::NOBS];
  load_goal<NOBJ>(a.k.st.goal_table, L.goal_idx, g);
  for (int e = 0; e < a.episodes; ++e) {
    policy_episode_begin<GENERAL>(a, i, e, L, g, o);
    EpisodeSum es;
    episode_sum_begin(es);
    for (int t = 0; t < a.k.T; ++t) {
      float y[6], act[3], reward;
      bool succ;
      mlp_layers(a.p, params, o, y, EARL_ACT_NONE);
      const U4 b = draw_block(a.k.cfg, policy_step_counter(a, e, t), i, kGaussDraw);
      const uint32_t word[3] = {b.x, b.y, b.z};
      const size_t row = ((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)i;
      for (int d = 0; d < 3; ++d) {
        const float eps = normal_quantile_f32(word[d] >> 8);
        act[d] = gaussian_head_action(a.head, a.p.out_act, y[d], y[3 + d], eps);
        if (a.head.eps_out) a.head.eps_out[row * 3 + d] = eps;
      }
      policy_env_step<GENERAL>(a, i, e, t, L, g, act[0], act[1], act[2], o, reward, succ);
      episode_sum_step(es, t, reward, succ);
    }
    if (sum) episode_sum_store(*sum, (size_t)e * (size_t)a.k.cfg.n + (size_t)i, es);
  }
  store_lane<NOBJ>(a.k, i, L);
}

// the agent pair: per step the network of the env's phase, the head's draw (phase-independent), pair_env_step
template <int NOBJ = 1>
inline void pair_rollout_env(const PairArgs& a, int i, bool gauss) {
  Lane<NOBJ> L;
  load_lane<NOBJ>(a.k, i, L);
  PairLane P;
  float g[Dims<NOBJ>::NG], o[Dims<NOBJ>::NOBS];
  pair_load<NOBJ>(a, i, L, P, g);
  for (int e = 0; e < a.episodes; ++e) {
    pair_episode_begin<NOBJ>(a, i, e, L, P, g, o);
    for (int t = 0; t < a.k.T; ++t) {
      const float* params = a.p.params + (size_t)P.phase * (size_t)a.pair.param_stride;
      float act[3];
      if (gauss) {
        float y[6];
        mlp_layers(a.p, params, o, y, EARL_ACT_NONE);
        const U4 b = draw_block(a.k.cfg, policy_step_counter(a, e, t), i, kGaussDraw);
        const uint32_t word[3] = {b.x, b.y, b.z};
        const size_t row = ((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)i;
        for (int d = 0; d < 3; ++d) {
          const float eps = normal_quantile_f32(word[d] >> 8);
          act[d] = gaussian_head_action(a.head, a.p.out_act, y[d], y[3 + d], eps);
          if (a.head.eps_out) a.head.eps_out[row * 3 + d] = eps;
        }
      } else {
        mlp_forward(a.p, params, o, act);
      }
      pair_env_step<NOBJ>(a, i, e, t, L, P, g, act[0], act[1], act[2], o);
    }
    pair_episode_end<NOBJ>(a, i, e, P);
  }
  pair_store<NOBJ>(a, i, L, P);
}

#else
// ------------------------------------------------------------------------------------------------
// gfx950 kernel.  One workgroup = 16 envs (the M of v_mfma_f32_16x16x4_f32) x four waves.
//   env step        lanes 0..15 of wave 0, one lane per env, state in registers for the whole launch (as rollout_body)
//   layer 0         12 -> H1:  A = the 16 observation rows (LDS), B = W0 tiles in registers; N-tile `tl` belongs to wave tl & 3
//   hidden layer    H1 -> H2 (NT2 > 0 only): A = the 16 x H1 activations (LDS), B = the wave's NT2 tiles of W1 in registers, H1 / 4 k-steps per tile, the
//                   tiles of a wave interleaved so that consecutive MFMAs do not depend on one another
//   output layer    Hlast -> 3 (padded to one 16-wide tile) on wave 0: ONE accumulator, Hlast / 4 dependent MFMAs -- the serial part
// Weights are loaded ONCE, in the B-operand lane map (lane l of k-step s holds B[k = 4 s + (l >> 4)][j = l & 15] = W[n0 + j][k]); every register
// array is indexed by unrolled constants only.  The A operand of k-step s is A[i = l & 15][k = 4 s + (l >> 4)]: activations are kept in LDS as
// [row][k & 3][k >> 2] so that a lane's operands of four consecutive k-steps are one 16-byte read.  C/D: column l & 15, rows 4 (l >> 4) + r.
// K is never padded (12 and the hidden widths are multiples of 4); only the output's N = 3 is (zero columns, results dropped).
// ------------------------------------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kPolX = 0;                                             // LDS floats: observation rows [16][12] (NOBJ = 3: [16][20], every image below 128 floats later: XS in the body)
constexpr int kPolH1 = 16 * 12;                                      // hidden activations [16][H1]
constexpr int kPolH2 = kPolH1 + 16 * kPolicyMaxWidth;                // [16][H2]
constexpr int kPolAct = kPolH2 + 16 * kPolicyMaxWidth;               // actions [16][4]
constexpr int kPolWo = kPolAct + 16 * 4;                              // output-layer weights [3][4][HL / 4] (the NT2 = 4 instantiation only)
constexpr int kPolLds = kPolWo + 3 * kPolicyMaxWidth;
// with a Gaussian head (GAUSS): the output tile has 6 live columns, the action rows are [16][8] (0..2 mean -> action, 3..5 raw log_std) and the
// output-layer weights, where they live in LDS, are [6][4][HL / 4]
constexpr int kPolWoG = kPolAct + 16 * 8;
constexpr int kPolEpsG = kPolWoG + 6 * kPolicyMaxWidth;            // the step's draws [16][4]
constexpr int kPolLdsG = kPolEpsG + 16 * 4;

// EARL_POLICY_STAMPS = diagnostic build only (tools/build_policy_stamped.sh, tools/prof_policy.py; never in libearl_hip.so): s_memtime stamps of wave 0 of
// workgroup 0 at the end of each phase of a step, summed over the launch: [0] observation -> LDS + barrier, [1] layer 0 + barrier, [2] hidden layer +
// barrier, [3] output layer + barrier (GAUSS: wave 1 makes the step's draws meanwhile), [4] env step (action read, tanh, wrapped_step, stores), [5] GAUSS only:
// the head on lanes 0..47 of wave 0 + the wavefront fence.  Each unit that instantiates the kernel has its own copy of the sums and its own reader
// (earl_debug_read_policy_profile: 5 words; earl_debug_read_policy_gaussian_profile: 6; earl_debug_read_policy_pair_profile: 6, [0] with the phase ballot).
#ifdef EARL_POLICY_STAMPS
static __device__ unsigned long long g_policy_prof[8];
__device__ __forceinline__ unsigned long long pol_clock() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define POL_STAMP(k) do { const unsigned long long now_ = pol_clock(); prof[k] += now_ - last_; last_ = now_; } while (0)
#else
#define POL_STAMP(k)
#endif

// where element (row, k) of a [16][K] activation image lives
__device__ __forceinline__ int pol_idx(int row, int k, int K) { return row * K + (k & 3) * (K >> 2) + (k >> 2); }

// GAUSS (tabletop_policy_gaussian.hip only): the head runs one lane per (env, dimension), lane 16 d + env of a wave's lanes 0..47.
//   draws   wave 1, WHILE wave 0 runs the output layer (the draw depends on the step's counter only, not on the network): the Philox block of the step,
//           eps = normal_quantile_f32, eps -> LDS and eps_out.  The output layer's barrier publishes it.
//   head    wave 0, after that barrier: log_std map, sigma, u, out_act; the action is written over the mean in the action row, and the env lanes, same
//           wave, read the row after a wavefront fence.  No workgroup barrier is added, and the three serial tanh_f32 leave the env lane.
//
// POP (policy_population_kernel, instantiated in tabletop_policy_population.hip only; argument PopulationArgs): a population of policies and per-episode summaries.
//   addressing  workgroups are aligned to GLOBAL env ids: workgroup b owns global ids 16 (floor(env_offset / 16) + b) .. + 15, its lanes whose local index falls
//               outside [0, n) idle like the ragged last workgroup's.  envs_per_policy being a multiple of 16, a workgroup never straddles two members
//   weights     the prologue's bases gain member * param_stride: wave-uniform scalar arithmetic, once
//   summaries   on the env lanes, in registers over the T steps, stored once per episode: no atomics, no LDS, no barrier
//   (the body both kernels share is tabletop_policy_kernel.inc)

template <int NT2, bool GENERAL, bool GAUSS = false>
__global__ __launch_bounds__(256) void policy_rollout_kernel(const typename PolicyArgsOf<GAUSS>::type a) {
  constexpr bool POP = false;
  constexpr int NOBJ = 1;
#include "tabletop_policy_kernel.inc"
}
template <int NT2, bool GENERAL, bool GAUSS>
__global__ __launch_bounds__(256) void policy_population_kernel(const PopulationArgs a) {
  constexpr bool POP = true;
  constexpr int NOBJ = 1;
#include "tabletop_policy_kernel.inc"
}
#endif  // EARL_HOST_BUILD

}  // namespace earl

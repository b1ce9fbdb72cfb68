// tabletop_host.cpp -- the `_cpu` entry points of include/earl_tabletop.h (BASELINE configs[0]: "1 env, CPU ... plumbing, no GPU"):
// the SAME per-env functions the gfx950 kernels run (tabletop_device.h, tabletop_step.h, philox.h; the planners' tabletop_plan.h, tabletop_value.h, tabletop_mpc.h, tabletop_cem.h, tabletop_prior.h;
// the policies' tabletop_policy.h), compiled for the host by g++ (-DEARL_HOST_BUILD: earl_rt.h -> host_shim.h) with -ffp-contract=off, one OpenMP iteration per env
// where a kernel has one lane per env.  This file owns only the walks: for_each_env, rollout_tiles, for_each_branch_tile (the branch-shaped launches' (branch, tile)
// range), update_env (one env's MPPI reweighting) and cem_update_env (one env's CEM refit), each for its planner and its receding-horizon loop; no arithmetic of an env or
// a planner is stated here.  Also the two host twins of the Sawyer door / peg planner (sawyer_plan.h: the candidates and the reweighting; the Sawyer stepper has no host build)
// and the two of its CEM planner (sawyer_cem.h: the candidates and the refit, the elites by a sort under cem_before).
// Host pointers, no stream, no HIP runtime.  This library is loaded only when a caller ASKS for device='cpu'; nothing falls back to it,
// and nothing here touches oracle/ (the oracle is the checker of both builds).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "tabletop_hostside.h"
#include "tabletop_plan.h"
#include "tabletop_mpc.h"
#include "tabletop_cem.h"
#include "tabletop_prior.h"
#include "tabletop_policy.h"
#include "sawyer_plan.h"   // the door / peg planner's candidates and reweighting (earl_sawyer_plan_candidates_cpu, earl_sawyer_plan_update_cpu)
#include "minitaur_plan.h" // the minitaur planner's, eight action dimensions (earl_minitaur_plan_candidates_cpu, earl_minitaur_plan_update_cpu)
#include "sawyer_cem.h"    // its CEM planner's candidates and refit (earl_sawyer_cem_candidates_cpu, earl_sawyer_cem_update_cpu)
#include "sawyer_value.h"  // the terminal value of both (earl_sawyer_value_terminal_cpu)
#include "../../include/earl_physics.h"

#ifdef _OPENMP
#include <omp.h>
#endif

using namespace earl;
using namespace earl::hostside;

namespace {

// envs per OpenMP chunk.  A thread walks its envs one after the other, each through all T steps (the kernels' loop order: state in registers), so the
// rows [t, i] a chunk writes must stay cache-resident across its envs: 16 envs x 200 steps x 66 B = 211 KB
constexpr int kChunk = 16;

template <class F>
inline void for_each_env(int n, F&& f) {
#pragma omp parallel for schedule(static, kChunk) if (n >= 4 * kChunk)
  for (int i = 0; i < n; ++i) f(i);
}

// The fused rollout on the host: a TILE of kTile consecutive envs keeps its state in a small array (the kernels keep it in registers) and walks the T steps time-major,
// so that every step writes kTile consecutive rows of each output -- the kernels' row order, contiguous in memory -- instead of one row per env per step scattered
// T * n * 66 bytes apart (rollout_body's loop order, made for a lane that owns one env).  Same wrapped_step, same counters: the same bits.
constexpr int kTile = 64;
template <int NOBJ, bool GENERAL>
void rollout_tiles(const KArgs& a) {
  const int n = a.cfg.n, tiles = (n + kTile - 1) / kTile;
#pragma omp parallel for schedule(static) if (tiles >= 4)
  for (int tile = 0; tile < tiles; ++tile) {
    const int i0 = tile * kTile, m = n - i0 < kTile ? n - i0 : kTile;
    Lane<NOBJ> L[kTile];
    float g[kTile][Dims<NOBJ>::NG];
    for (int k = 0; k < m; ++k) {
      load_lane<NOBJ>(a, i0 + k, L[k]);
      load_goal<NOBJ>(a.st.goal_table, L[k].goal_idx, g[k]);
    }
    for (int t = 0; t < a.T; ++t) {
      const float* ap = a.act + ((size_t)t * n + i0) * 3;
      const size_t row0 = (size_t)t * n + i0;
      for (int k = 0; k < m; ++k) {
        float o[Dims<NOBJ>::NOBS];
        float reward;
        bool done, succ;
        wrapped_step<NOBJ, GENERAL>(a, i0 + k, a.cfg.counter + (uint64_t)t, L[k], g[k], ap[3 * k], ap[3 * k + 1], ap[3 * k + 2], o, reward, done, succ);
        const size_t row = row0 + k;
        if (a.out.obs) store_obs<NOBJ>(a.out.obs + row * Dims<NOBJ>::NOBS, o);
        if (a.out.reward) a.out.reward[row] = reward;
        if (a.out.done) a.out.done[row] = done;
        if (a.out.success) a.out.success[row] = succ;
      }
    }
    for (int k = 0; k < m; ++k) store_lane<NOBJ>(a, i0 + k, L[k]);
  }
}

template <int NOBJ>
int do_step(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const float* act, const int32_t* ngi, const earl_tabletop_out* out) {
  if (int rc = check_common(cfg, st, NOBJ)) return rc;
  if (!act || !out) return fail(EARL_ERR_ARG, "act/out is NULL");
  if (cfg->n == 0) return EARL_OK;
  const KArgs a{*cfg, *st, *out, act, ngi, nullptr, nullptr, 1, thresholds()};
  if (is_general(cfg)) for_each_env(cfg->n, [&](int i) { step_body<NOBJ, true>(a, i); });
  else for_each_env(cfg->n, [&](int i) { step_body<NOBJ, false>(a, i); });
  return EARL_OK;
}

template <int NOBJ>
int do_reset(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const uint8_t* mask, const int32_t* ngi, float* obs) {
  if (int rc = check_common(cfg, st, NOBJ)) return rc;
  if (cfg->n == 0) return EARL_OK;
  const KArgs a{*cfg, *st, earl_tabletop_out{nullptr, nullptr, nullptr, nullptr, nullptr}, nullptr, ngi, mask, obs, 0, thresholds()};
  for_each_env(cfg->n, [&](int i) { reset_body<NOBJ>(a, i); });
  return EARL_OK;
}

template <int NOBJ>
int do_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T, const float* act, const earl_tabletop_out* out, bool reset_first) {
  if (int rc = check_common(cfg, st, NOBJ)) return rc;
  if (!act || !out) return fail(EARL_ERR_ARG, "act/out is NULL");
  if (T < 0) return fail(EARL_ERR_ARG, "T = %d < 0", T);
  if (cfg->n == 0) return EARL_OK;
  earl_tabletop_cfg c2 = *cfg;
  if (reset_first) {                       // reset with counter cfg->counter, the steps with the next ones (earl_tabletop_reset_rollout)
    if (int rc = do_reset<NOBJ>(cfg, st, nullptr, nullptr, nullptr)) return rc;
    c2.counter += 1;
  }
  if (T == 0) return EARL_OK;
  const KArgs a{c2, *st, *out, act, nullptr, nullptr, nullptr, T, thresholds()};
  if (is_general(cfg)) rollout_tiles<NOBJ, true>(a);
  else rollout_tiles<NOBJ, false>(a);
  return EARL_OK;
}

// The evaluation episodes on the host: the plain loop over the reset and the rollout above, episode e at counter + e * (T + 1)
template <int NOBJ>
int do_eval(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T, const float* act, int64_t act_episode_stride,
            const earl_tabletop_out* out) {
  if (episodes < 0) return fail(EARL_ERR_ARG, "episodes = %d < 0", episodes);
  if (act_episode_stride < 0) return fail(EARL_ERR_ARG, "negative action stride");
  if (int rc = check_common(cfg, st, NOBJ)) return rc;
  if (!act || !out) return fail(EARL_ERR_ARG, "act/out is NULL");
  if (T < 0) return fail(EARL_ERR_ARG, "T = %d < 0", T);
  for (int32_t e = 0; e < episodes; ++e) {
    earl_tabletop_cfg c = *cfg;
    c.counter += (uint64_t)e * (uint64_t)(T + 1);
    const size_t rows = (size_t)e * (size_t)T * (size_t)cfg->n;
    const earl_tabletop_out o{out->obs ? out->obs + rows * Dims<NOBJ>::NOBS : nullptr, out->reward ? out->reward + rows : nullptr, out->done ? out->done + rows : nullptr,
                              out->success ? out->success + rows : nullptr, nullptr};
    if (int rc = do_rollout<NOBJ>(&c, st, T, act + (size_t)e * (size_t)act_episode_stride, &o, true)) return rc;
  }
  return EARL_OK;
}

// The (branch, tile of kTile envs) walk of the branch-shaped launches (branch, score, candidates) on the host, stated once: one OpenMP iteration per workgroup of
// the device's flattened 1-D grid of `blocks` = K * tiles, f(i, k) for every live env i of the tile.
template <class F>
inline void for_each_branch_tile(long long blocks, int K, int n, F&& f) {
  static_assert(kTile == kBranchBlock, "a tile of the twin is a workgroup of the device launch");
  const long long tiles = blocks / K;
#pragma omp parallel for schedule(static) if (blocks >= 4)
  for (long long j = 0; j < blocks; ++j) {
    const int k = (int)(j / tiles);
    const long long i0 = (j - k * tiles) * kTile;
    const int m = n - i0 < kTile ? (int)(n - i0) : kTile;
    for (int i = (int)i0; i < (int)i0 + m; ++i) f(i, k);
  }
}

// One reweighting of ONE env (items 4-5 of the planner's contract), stated once for the planner and the receding-horizon loop: beta / best_k over the K returns in
// ascending k, the weights once per k, then per plan row the integer sums in ascending k (branch 0 is the mean and adds nothing; W == 0 is skipped) and plan_new_mean.
// ret(k) = return k; row(t, m) = the CLIPPED row t of the plan entering; put(t, d, v) = word d of row t of the plan leaving; acc(k, t, m, W, A) = item 5 of branch
// k >= 1 (plan_accumulate wherever the candidate is made again; the `_prior` twin reads its prior branches back).  -> (beta, best_k)
template <class Ret, class Row, class Put, class Acc>
inline std::pair<double, int> update_env_with(const PlanArgs& p, Ret&& ret, Row&& row, Put&& put, Acc&& acc) {
  double beta = -INFINITY;
  int bk = 0;
  for (int k = 0; k < p.K; ++k) plan_best(ret(k), k, beta, bk);
  std::vector<int32_t> Wk(p.K);                            // once per (k, env), as the update kernel shares them through LDS
  for (int k = 0; k < p.K; ++k) Wk[k] = plan_weight(ret(k), beta, p.inv_temperature);
  for (int t = 0; t < p.a.T; ++t) {
    float m[3];
    row(t, m);
    int64_t A[3] = {0, 0, 0}, S = 0;
    for (int k = 0; k < p.K; ++k) {
      const int32_t W = Wk[k];
      S += W;
      if (W != 0 && k > 0) acc(k, t, m, W, A);
    }
    for (int d = 0; d < 3; ++d) put(t, d, plan_new_mean(m[d], A[d], S));
  }
  return {beta, bk};
}
template <class Ret, class Row, class Put>
inline std::pair<double, int> update_env(const PlanArgs& p, int i, Ret&& ret, Row&& row, Put&& put) {
  return update_env_with(p, ret, row, put,
                    [&](int k, int t, const float (&m)[3], int32_t W, int64_t (&A)[3]) { plan_accumulate(p, i, (uint32_t)k, (uint32_t)t, m, W, A); });
}

// The branch launch on the host: each env of each (branch, tile) through branch_body, the function the kernel runs.
template <int NOBJ>
int do_branch(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t stride,
              const earl_episode_summary* summary, float* last_obs) {
  long long blocks;
  if (int rc = check_branch(cfg, st, NOBJ, K, H, act, stride, summary, last_obs, &blocks)) return rc;
  if (blocks == 0) return EARL_OK;
  const BranchArgs b{KArgs{*cfg, *st, earl_tabletop_out{nullptr, nullptr, nullptr, nullptr, nullptr}, act, nullptr, nullptr, nullptr, H, thresholds()},
                     (long long)stride, summary ? *summary : earl_episode_summary{nullptr, nullptr, nullptr}, last_obs};
  const bool general = is_general(cfg);
  for_each_branch_tile(blocks, K, cfg->n, [&](int i, int k) {
    if (general) branch_body<NOBJ, true>(b, i, k);
    else branch_body<NOBJ, false>(b, i, k);
  });
  return EARL_OK;
}

// The planner on the host (include/earl_tabletop.h, "MPPI planning"): per iteration the score pass over the device's (branch, 64 envs) workgroups, then update_env
// per env -- tabletop_plan.h's plan_* functions, the ones the kernels run.  VALUE: the `_value` twins (the score of tabletop_value.h, as plan_score_kernel<.., true>).
template <int NOBJ, bool VALUE>
int do_plan(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, const earl_plan_value* pv, const float* mean, float* plan,
            double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  long long blocks, ublocks;
  if (int rc = check_plan(cfg, st, NOBJ, pp, 0, mean, plan, ret, &blocks, &ublocks)) return rc;
  if constexpr (VALUE)
    if (int rc = check_plan_value(pv, Dims<NOBJ>::NOBS)) return rc;
  if (blocks == 0) return EARL_OK;
  PlanValueArgs p{};
  static_cast<PlanArgs&>(p) = plan_args(cfg, st, pp, mean, thresholds());
  if constexpr (VALUE) p.v = value_args(pv);
  p.plan = plan;
  p.ret = ret;
  const int n = cfg->n, K = pp->K;
  const bool general = is_general(cfg);
  for (int it = 0; it < pp->iterations; ++it) {
    const bool last = it + 1 == pp->iterations;
    p.mean = it ? plan : mean;
    p.word0 = kPlanDraw | (uint32_t)(pp->iteration0 + it);
    p.ret0 = ret0 ? ret0 + (size_t)it * n : nullptr;
    for_each_branch_tile(blocks, K, n, [&](int i, int k) {
      if (general) plan_score_body<NOBJ, true, VALUE>(p, i, k, &p.v);
      else plan_score_body<NOBJ, false, VALUE>(p, i, k, &p.v);
    });
    for_each_env(n, [&](int i) {
      const auto [beta, bk] = update_env(p, i, [&](int k) { return ret[(size_t)k * n + i]; }, [&](int t, float (&m)[3]) { plan_mean(p, i, t, m); },
                                         [&](int t, int d, float v) { plan[((size_t)t * n + i) * 3 + d] = v; });
      if (last && best_ret) best_ret[i] = beta;
      if (last && best_k) best_k[i] = bk;
    });
  }
  return EARL_OK;
}

// The planner with policy-prior branches on the host (include/earl_tabletop.h, "MPPI with policy-prior branches"): do_plan's walk; a (branch, tile) of 1 <= k <= P runs
// tabletop_prior.h's prior_score_body, every other one plan_score_body, and update_env reads the prior branches back through prior_accumulate -- the device's three launches
template <int NOBJ, bool VALUE>
int do_plan_prior_v(const PlanPriorArgs& p0, const earl_plan_params* pp, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                    long long blocks) {
  PlanPriorArgs p = p0;
  const int n = p.a.cfg.n, K = pp->K, P = p.pr.P;
  const bool general = is_general(&p.a.cfg);
  for (int it = 0; it < pp->iterations; ++it) {
    const bool last = it + 1 == pp->iterations;
    p.mean = it ? plan : mean;
    p.word0 = kPlanDraw | (uint32_t)(pp->iteration0 + it);
    p.ret0 = ret0 ? ret0 + (size_t)it * n : nullptr;
    for_each_branch_tile(blocks, K, n, [&](int i, int k) {
      if (k >= 1 && k <= P) {
        if (general) prior_score_body<NOBJ, true, VALUE>(p, i, k);
        else prior_score_body<NOBJ, false, VALUE>(p, i, k);
      } else {
        if (general) plan_score_body<NOBJ, true, VALUE>(p, i, k, &p.v);
        else plan_score_body<NOBJ, false, VALUE>(p, i, k, &p.v);
      }
    });
    for_each_env(n, [&](int i) {
      const auto [beta, bk] = update_env_with(
          p, [&](int k) { return ret[(size_t)k * n + i]; }, [&](int t, float (&m)[3]) { plan_mean(p, i, t, m); },
          [&](int t, int d, float v) { plan[((size_t)t * n + i) * 3 + d] = v; },
          [&](int k, int t, const float (&m)[3], int32_t W, int64_t (&A)[3]) {
            if (k <= P) prior_accumulate(p, i, (uint32_t)k, (uint32_t)t, m, W, A);
            else plan_accumulate(p, i, (uint32_t)k, (uint32_t)t, m, W, A);
          });
      if (last && best_ret) best_ret[i] = beta;
      if (last && best_k) best_k[i] = bk;
    });
  }
  return EARL_OK;
}

template <int NOBJ>
int do_plan_prior(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, const earl_plan_value* pv, const earl_plan_prior* prior,
                  const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  long long blocks, ublocks;
  if (int rc = check_plan(cfg, st, NOBJ, pp, 0, mean, plan, ret, &blocks, &ublocks)) return rc;
  if (pv)
    if (int rc = check_plan_value(pv, Dims<NOBJ>::NOBS)) return rc;
  if (int rc = check_plan_prior(cfg, pp, prior, Dims<NOBJ>::NOBS, mean, plan, ret)) return rc;
  if (blocks == 0) return EARL_OK;
  PlanPriorArgs p{};
  static_cast<PlanArgs&>(p) = plan_args(cfg, st, pp, mean, thresholds());
  if (pv) p.v = value_args(pv);
  p.pr = prior_args(prior);
  p.plan = plan;
  p.ret = ret;
  return pv ? do_plan_prior_v<NOBJ, true>(p, pp, mean, plan, ret, ret0, best_ret, best_k, blocks)
            : do_plan_prior_v<NOBJ, false>(p, pp, mean, plan, ret, ret0, best_ret, best_k, blocks);
}

// The receding-horizon loop on the host (include/earl_tabletop.h, "receding-horizon MPPI control"): one OpenMP iteration per env -- the device's workgroup -- holds
// the env and its plan for all T steps; per iteration the K scores in ascending k (mpc_score, the kernel's) and update_env on the env's own plan; then the real
// step (mpc_act, the kernel's) and the shift.
template <int NOBJ, bool GENERAL, bool VALUE>
void mpc_env(const MpcValueArgs& x, int i) {
  const KArgs& a = x.p.a;
  const int n = a.cfg.n, H = a.T, K = x.p.K;
  std::vector<float> P((size_t)H * 3);
  for (int e = 0; e < H * 3; ++e) P[e] = x.m.plan[((size_t)(e / 3) * n + i) * 3 + e % 3];
  std::vector<double> ret(K);
  Lane<NOBJ> L;
  load_lane<NOBJ>(a, i, L);
  float g[Dims<NOBJ>::NG];
  load_goal<NOBJ>(a.st.goal_table, L.goal_idx, g);
  PlanArgs q = x.p;
  auto row = [&](int t, float (&m)[3]) {
    for (int d = 0; d < 3; ++d) m[d] = plan_clip(P[(size_t)t * 3 + d]);
  };
  for (int s = 0; s < x.T; ++s) {
    const uint64_t counter = a.cfg.counter + (uint64_t)s;
    q.noise_counter = x.p.noise_counter + (uint32_t)s;
    for (int it = 0; it < x.iterations; ++it) {
      q.word0 = kPlanDraw | (uint32_t)(x.iteration0 + it);
      for (int k = 0; k < K; ++k) ret[k] = mpc_score<NOBJ, GENERAL, VALUE>(q, i, k, counter, L, g, row, &x.v);
      if (x.m.ret0) x.m.ret0[((size_t)s * x.iterations + it) * n + i] = ret[0];
      const double beta = update_env(q, i, [&](int k) { return ret[k]; }, row, [&](int t, int d, float v) { P[(size_t)t * 3 + d] = v; }).first;
      if (it + 1 == x.iterations && x.m.best_ret) x.m.best_ret[(size_t)s * n + i] = beta;
    }
    const float act[3] = {P[0], P[1], P[2]};
    const bool done = mpc_act<NOBJ, GENERAL>(x, i, s, counter, L, g, act, true);
    if (GENERAL && done && a.cfg.auto_reset) std::fill(P.begin(), P.end(), 0.0f);
    else std::copy(P.begin() + 3, P.end(), P.begin());   // (the shift; the last row stays, repeated)
  }
  for (int e = 0; e < H * 3; ++e) x.m.plan[((size_t)(e / 3) * n + i) * 3 + e % 3] = P[e];
  store_lane<NOBJ>(a, i, L);
}

template <int NOBJ, bool VALUE>
int do_mpc(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, const earl_plan_value* pv, int32_t T, const earl_tabletop_out* out,
           const earl_mpc_out* mpc) {
  int lanes;
  if (int rc = check_mpc(cfg, st, NOBJ, pp, T, out, mpc, &lanes)) return rc;
  if constexpr (VALUE)
    if (int rc = check_plan_value(pv, Dims<NOBJ>::NOBS)) return rc;
  if (lanes == 0) return EARL_OK;
  MpcValueArgs x{};
  static_cast<MpcArgs&>(x) = mpc_args(cfg, st, pp, T, out, mpc);
  if constexpr (VALUE) x.v = value_args(pv);
  const bool general = is_general(cfg);
  const int n = cfg->n;
#pragma omp parallel for schedule(dynamic, 1) if (n >= 4)
  for (int i = 0; i < n; ++i) {
    if (general) mpc_env<NOBJ, true, VALUE>(x, i);
    else mpc_env<NOBJ, false, VALUE>(x, i);
  }
  return EARL_OK;
}


// One CEM refit of ONE env (items 4-5 of the CEM contract), stated once for the planner and the receding-horizon loop: beta / best_k and the ranks over the K returns,
// the elites in ascending k, then per plan row the two integer moments over the elites (branch 0 adds nothing) and cem_new_mean / cem_new_std.
// ret(k) = return k; row(t, m, s) = the clipped mean and clamped std of row t entering; put(t, d, mean', std').  -> (beta, best_k)
template <class Ret, class Row, class Put>
inline std::pair<double, int> cem_update_env(const PlanArgs& p, int i, int E, float alpha, float lo, float hi, Ret&& ret, Row&& row, Put&& put) {
  double beta = -INFINITY;
  int bk = 0;
  std::vector<int> elite;
  for (int k = 0; k < p.K; ++k) {
    const double r = ret(k);
    plan_best(r, k, beta, bk);
    int rank = 0;
    for (int k2 = 0; k2 < p.K; ++k2) rank += cem_before(ret(k2), k2, r, k) ? 1 : 0;
    if (cem_elite(r, rank, E)) elite.push_back(k);
  }
  const int32_t Ne = (int32_t)elite.size();
  for (int t = 0; t < p.a.T; ++t) {
    float m[3], s[3];
    row(t, m, s);
    int64_t A1[3] = {0, 0, 0}, A2[3] = {0, 0, 0};
    for (int k : elite)
      if (k > 0) cem_accumulate(p, i, (uint32_t)k, (uint32_t)t, m, s, A1, A2);
    for (int d = 0; d < 3; ++d) put(t, d, cem_new_mean(m[d], A1[d], Ne, alpha), cem_new_std(s[d], A1[d], A2[d], Ne, alpha, lo, hi));
  }
  return {beta, bk};
}

// The CEM planner on the host (include/earl_tabletop.h, "CEM planning"): do_plan's walk with tabletop_cem.h's functions, the ones the kernels run
template <int NOBJ>
int do_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* cp, const earl_plan_value* pv, const float* mean, const float* std0,
           float* plan, float* std_out, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  long long blocks, ublocks;
  if (int rc = check_cem(cfg, st, NOBJ, Dims<NOBJ>::NOBS, cp, pv, 0, mean, std0, plan, std_out, ret, &blocks, &ublocks)) return rc;
  if (blocks == 0) return EARL_OK;
  CemArgs c = cem_args(cfg, st, cp, pv, mean, std0, thresholds());
  c.p.plan = plan;
  c.p.ret = ret;
  c.std_out = std_out;
  const int n = cfg->n, K = cp->K;
  const bool general = is_general(cfg), value = pv != nullptr;
  for (int it = 0; it < cp->iterations; ++it) {
    const bool last = it + 1 == cp->iterations;
    c.p.mean = it ? plan : mean;
    c.std_in = it ? std_out : std0;
    c.p.word0 = kCemDraw | (uint32_t)(cp->iteration0 + it);
    c.p.ret0 = ret0 ? ret0 + (size_t)it * n : nullptr;
    for_each_branch_tile(blocks, K, n, [&](int i, int k) {
      if (general) value ? cem_score_body<NOBJ, true, true>(c, i, k) : cem_score_body<NOBJ, true, false>(c, i, k);
      else value ? cem_score_body<NOBJ, false, true>(c, i, k) : cem_score_body<NOBJ, false, false>(c, i, k);
    });
    for_each_env(n, [&](int i) {
      const auto [beta, bk] = cem_update_env(
          c.p, i, c.E, c.alpha, c.std_min, c.std_max, [&](int k) { return ret[(size_t)k * n + i]; },
          [&](int t, float (&m)[3], float (&s)[3]) {
            plan_mean(c.p, i, t, m);
            cem_std(c, i, t, s);
          },
          [&](int t, int d, float mv, float sv) {
            plan[((size_t)t * n + i) * 3 + d] = mv;
            std_out[((size_t)t * n + i) * 3 + d] = sv;
          });
      if (last && best_ret) best_ret[i] = beta;
      if (last && best_k) best_k[i] = bk;
    });
  }
  return EARL_OK;
}

// The receding-horizon CEM loop on the host: mpc_env with the CEM score and refit; the std starts from sclamp(sigma) at every real step
template <int NOBJ, bool GENERAL>
void cem_mpc_env(const CemMpcArgs& c, int i) {
  const MpcArgs& x = c.x;
  const KArgs& a = x.p.a;
  const int n = a.cfg.n, H = a.T, K = x.p.K;
  std::vector<float> P((size_t)H * 3), S((size_t)H * 3);
  for (int e = 0; e < H * 3; ++e) P[e] = x.m.plan[((size_t)(e / 3) * n + i) * 3 + e % 3];
  std::vector<double> ret(K);
  Lane<NOBJ> L;
  load_lane<NOBJ>(a, i, L);
  float g[Dims<NOBJ>::NG];
  load_goal<NOBJ>(a.st.goal_table, L.goal_idx, g);
  PlanArgs q = x.p;
  auto row = [&](int t, float (&m)[3], float (&s)[3]) {
    for (int d = 0; d < 3; ++d) {
      m[d] = plan_clip(P[(size_t)t * 3 + d]);
      s[d] = S[(size_t)t * 3 + d];
    }
  };
  for (int s = 0; s < x.T; ++s) {
    const uint64_t counter = a.cfg.counter + (uint64_t)s;
    q.noise_counter = x.p.noise_counter + (uint32_t)s;
    for (int e = 0; e < H * 3; ++e) S[e] = cem_sclamp(x.p.sigma[e % 3], c.std_min, c.std_max);
    for (int it = 0; it < x.iterations; ++it) {
      q.word0 = kCemDraw | (uint32_t)(x.iteration0 + it);
      for (int k = 0; k < K; ++k) ret[k] = cem_mpc_score<NOBJ, GENERAL>(q, i, k, counter, L, g, row);
      if (x.m.ret0) x.m.ret0[((size_t)s * x.iterations + it) * n + i] = ret[0];
      const double beta = cem_update_env(q, i, c.E, c.alpha, c.std_min, c.std_max, [&](int k) { return ret[k]; }, row, [&](int t, int d, float mv, float sv) {
                            P[(size_t)t * 3 + d] = mv;
                            S[(size_t)t * 3 + d] = sv;
                          }).first;
      if (it + 1 == x.iterations && x.m.best_ret) x.m.best_ret[(size_t)s * n + i] = beta;
    }
    const float act[3] = {P[0], P[1], P[2]};
    const bool done = mpc_act<NOBJ, GENERAL>(x, i, s, counter, L, g, act, true);
    if (GENERAL && done && a.cfg.auto_reset) std::fill(P.begin(), P.end(), 0.0f);
    else std::copy(P.begin() + 3, P.end(), P.begin());   // (the shift; the last row stays, repeated)
  }
  for (int e = 0; e < H * 3; ++e) x.m.plan[((size_t)(e / 3) * n + i) * 3 + e % 3] = P[e];
  store_lane<NOBJ>(a, i, L);
}

template <int NOBJ>
int do_cem_mpc(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* cp, const earl_plan_value* pv, int32_t T, const earl_tabletop_out* out,
               const earl_mpc_out* mpc) {
  int lanes;
  if (int rc = check_cem_mpc(cfg, st, NOBJ, cp, pv, T, out, mpc, &lanes)) return rc;
  if (lanes == 0) return EARL_OK;
  const CemMpcArgs c = cem_mpc_args(cfg, st, cp, T, out, mpc);
  const bool general = is_general(cfg);
  const int n = cfg->n;
#pragma omp parallel for schedule(dynamic, 1) if (n >= 4)
  for (int i = 0; i < n; ++i) {
    if (general) cem_mpc_env<NOBJ, true>(c, i);
    else cem_mpc_env<NOBJ, false>(c, i);
  }
  return EARL_OK;
}

// The candidates walk of both Sawyer planners, one row of n envs per (k, t): row(i, t, m, scale) gives the clipped row and the scale of the noise around it
template <class Row>
void sawyer_candidates_walk(const earl_sawyer_cfg* cfg, int K, int H, uint32_t word0, uint32_t noise_counter, float* act_out, Row row) {
  const int n = cfg->n;
  const long long rows = (long long)K * H;
#pragma omp parallel for schedule(static) if (rows * n >= 4096)
  for (long long kt = 0; kt < rows; ++kt) {
    const int k = (int)(kt / H), t = (int)(kt - (long long)k * H);
    for (int i = 0; i < n; ++i) {
      float m[4], scale[4], c[4];
      row(i, t, m, scale);
      shoot_candidate(word0, (uint32_t)(cfg->env_offset + i), (uint32_t)k, (uint32_t)t, noise_counter, cfg->seed, scale, m, c);
      float* dst = act_out + shoot_act_index(H, n, i, k, t);
      for (int d = 0; d < 4; ++d) dst[d] = c[d];
    }
  }
}

}  // namespace

extern "C" {

int earl_tabletop_plan_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                               const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_cem<1>(cfg, st, params, pv, mean, std0, plan, std, ret, ret0, best_ret, best_k);
}
int earl_tabletop3_plan_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                                const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_cem<3>(cfg, st, params, pv, mean, std0, plan, std, ret, ret0, best_ret, best_k);
}
int earl_tabletop_cem_candidates_cpu(const earl_tabletop_cfg* cfg, const earl_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out) {
  long long blocks, ublocks;
  if (int rc = check_cem(cfg, nullptr, 1, 0, params, nullptr, j, mean, std, act_out, nullptr, nullptr, &blocks, &ublocks)) return rc;
  if (blocks == 0) return EARL_OK;
  CemArgs c = cem_args(cfg, nullptr, params, nullptr, mean, std, thresholds());
  c.p.word0 = kCemDraw | (uint32_t)j;
  for_each_branch_tile(blocks, params->K, cfg->n, [&](int i, int k) { cem_candidates_body(c, i, k, act_out); });
  return EARL_OK;
}
int earl_tabletop_mpc_rollout_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                      const earl_tabletop_out* out, const earl_mpc_out* mpc) {
  return do_cem_mpc<1>(cfg, st, params, pv, T, out, mpc);
}
int earl_tabletop3_mpc_rollout_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                       const earl_tabletop_out* out, const earl_mpc_out* mpc) {
  return do_cem_mpc<3>(cfg, st, params, pv, T, out, mpc);
}
int earl_tabletop_mpc_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                                  const earl_mpc_out* mpc) {
  return do_mpc<1, false>(cfg, st, params, nullptr, T, out, mpc);
}
int earl_tabletop3_mpc_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                                   const earl_mpc_out* mpc) {
  return do_mpc<3, false>(cfg, st, params, nullptr, T, out, mpc);
}
int earl_tabletop_mpc_rollout_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                        const earl_tabletop_out* out, const earl_mpc_out* mpc) {
  return do_mpc<1, true>(cfg, st, params, pv, T, out, mpc);
}
int earl_tabletop3_mpc_rollout_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                         const earl_tabletop_out* out, const earl_mpc_out* mpc) {
  return do_mpc<3, true>(cfg, st, params, pv, T, out, mpc);
}
int earl_tabletop_plan_mppi_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan,
                                double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_plan<1, false>(cfg, st, params, nullptr, mean, plan, ret, ret0, best_ret, best_k);
}
int earl_tabletop3_plan_mppi_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan,
                                 double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_plan<3, false>(cfg, st, params, nullptr, mean, plan, ret, ret0, best_ret, best_k);
}
int earl_tabletop_plan_mppi_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                      const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_plan<1, true>(cfg, st, params, pv, mean, plan, ret, ret0, best_ret, best_k);
}
int earl_tabletop3_plan_mppi_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                       const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_plan<3, true>(cfg, st, params, pv, mean, plan, ret, ret0, best_ret, best_k);
}
int earl_tabletop_plan_mppi_prior_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                      const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_plan_prior<1>(cfg, st, params, pv, prior, mean, plan, ret, ret0, best_ret, best_k);
}
int earl_tabletop3_plan_mppi_prior_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                       const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k) {
  return do_plan_prior<3>(cfg, st, params, pv, prior, mean, plan, ret, ret0, best_ret, best_k);
}
int earl_tabletop_plan_candidates_cpu(const earl_tabletop_cfg* cfg, const earl_plan_params* params, int32_t j, const float* mean, float* act_out) {
  long long blocks, ublocks;
  if (int rc = check_plan(cfg, nullptr, 1, params, j, mean, act_out, nullptr, &blocks, &ublocks)) return rc;
  if (blocks == 0) return EARL_OK;
  PlanArgs p = plan_args(cfg, nullptr, params, mean, thresholds());
  p.word0 = kPlanDraw | (uint32_t)j;
  for_each_branch_tile(blocks, params->K, cfg->n, [&](int i, int k) { plan_candidates_body(p, i, k, act_out); });
  return EARL_OK;
}

int earl_tabletop_branch_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                     const earl_episode_summary* summary, float* last_obs) {
  return do_branch<1>(cfg, st, K, H, act, act_branch_stride, summary, last_obs);
}
int earl_tabletop3_branch_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                      const earl_episode_summary* summary, float* last_obs) {
  return do_branch<3>(cfg, st, K, H, act, act_branch_stride, summary, last_obs);
}

int earl_tabletop_step_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const float* act, const int32_t* next_goal_idx,
                           const earl_tabletop_out* out) {
  return do_step<1>(cfg, st, act, next_goal_idx, out);
}
int earl_tabletop_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T, const float* act, const earl_tabletop_out* out) {
  return do_rollout<1>(cfg, st, T, act, out, false);
}
int earl_tabletop_reset_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T, const float* act, const earl_tabletop_out* out) {
  return do_rollout<1>(cfg, st, T, act, out, true);
}
int earl_tabletop_eval_episodes_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T, const float* act,
                                    int64_t act_episode_stride, const earl_tabletop_out* out) {
  return do_eval<1>(cfg, st, episodes, T, act, act_episode_stride, out);
}
int earl_tabletop_policy_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, int32_t episodes, int32_t T,
                                     int32_t reset_first, const earl_tabletop_out* out, float* act_out) {
  if (int rc = check_policy(cfg, st, policy, nullptr, episodes, T, reset_first, out)) return rc;
  if (cfg->n == 0) return EARL_OK;
  const PolicyArgs a{KArgs{*cfg, *st, *out, nullptr, nullptr, nullptr, nullptr, T, thresholds()}, *policy, act_out, episodes, reset_first};
  if (is_general(cfg)) for_each_env(cfg->n, [&](int i) { policy_rollout_env<true>(a, i, a.p.params); });
  else for_each_env(cfg->n, [&](int i) { policy_rollout_env<false>(a, i, a.p.params); });
  return EARL_OK;
}
int earl_tabletop_policy_rollout_gaussian_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                              const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                              const earl_tabletop_out* out, float* act_out) {
  if (int rc = check_policy_gaussian(cfg, st, policy, head, episodes, T, reset_first, out)) return rc;
  if (cfg->n == 0) return EARL_OK;
  GaussianPolicyArgs a;
  static_cast<PolicyArgs&>(a) = PolicyArgs{KArgs{*cfg, *st, *out, nullptr, nullptr, nullptr, nullptr, T, thresholds()}, *policy, act_out, episodes, reset_first};
  a.head = *head;
  if (is_general(cfg)) for_each_env(cfg->n, [&](int i) { gaussian_rollout_env<true>(a, i, a.p.params); });
  else for_each_env(cfg->n, [&](int i) { gaussian_rollout_env<false>(a, i, a.p.params); });
  return EARL_OK;
}
int earl_tabletop_population_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                         const earl_policy_population* pop, const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                         const earl_tabletop_out* out, float* act_out, const earl_episode_summary* summary) {
  if (int rc = check_population(cfg, st, policy, pop, head, episodes, T, reset_first, out)) return rc;
  if (cfg->n == 0) return EARL_OK;
  const PopulationArgs a = population_args(cfg, st, policy, pop, head, episodes, T, reset_first, out, act_out, summary, thresholds());
  const bool general = is_general(cfg);
  for_each_env(cfg->n, [&](int i) {                       // the env with global id env_offset + i runs its member's parameters
    const float* params = a.p.params + population_param_offset(a.pop, a.k.cfg.env_offset + i);
    if (head) general ? gaussian_rollout_env<true>(a, i, params, &a.sum) : gaussian_rollout_env<false>(a, i, params, &a.sum);
    else general ? policy_rollout_env<true>(a, i, params, &a.sum) : policy_rollout_env<false>(a, i, params, &a.sum);
  });
  return EARL_OK;
}
int earl_tabletop_pair_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                   const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out) {
  if (int rc = check_pair(cfg, st, policy, pair, head, episodes, T, reset_first, out)) return rc;
  if (cfg->n == 0) return EARL_OK;
  const PairArgs a = pair_args(cfg, st, policy, pair, head, episodes, T, reset_first, out, act_out, thresholds());
  for_each_env(cfg->n, [&](int i) { pair_rollout_env(a, i, head != nullptr); });
  return EARL_OK;
}
int earl_tabletop_reset_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const uint8_t* mask, const int32_t* next_goal_idx, float* obs) {
  return do_reset<1>(cfg, st, mask, next_goal_idx, obs);
}
int earl_tabletop_observe_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_tabletop_out* out) {
  if (int rc = check_common(cfg, st, 1)) return rc;
  if (!out) return fail(EARL_ERR_ARG, "out is NULL");
  const KArgs a{*cfg, *st, *out, nullptr, nullptr, nullptr, nullptr, 0, thresholds()};
  for_each_env(cfg->n, [&](int i) { observe_body(a, i); });
  return EARL_OK;
}
int earl_tabletop_reward_cpu(int32_t n, const float* obs, int32_t reward_type, int32_t wide_init, float* reward, uint8_t* success) {
  if (n < 0 || !obs) return fail(EARL_ERR_ARG, "bad n/obs");
  if (reward_type != EARL_REWARD_SPARSE && reward_type != EARL_REWARD_DENSE) return fail(EARL_ERR_ARG, "reward_type = %d", reward_type);
  const Thresholds th = thresholds();
  for_each_env(n, [&](int i) { reward_body<1>(i, obs, reward_type, wide_init, reward, success, th); });
  return EARL_OK;
}
int earl_tabletop_valid_init_cpu(int32_t n, const double* cand, uint8_t* valid) {
  if (n < 0 || !cand || !valid) return fail(EARL_ERR_ARG, "bad n/cand/valid");
  const Thresholds th = thresholds();
  for_each_env(n, [&](int i) { valid_init_body(i, cand, valid, th); });
  return EARL_OK;
}

int earl_tabletop3_step_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const float* act, const earl_tabletop_out* out) {
  return do_step<3>(cfg, st, act, nullptr, out);
}
int earl_tabletop3_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T, const float* act, const earl_tabletop_out* out) {
  return do_rollout<3>(cfg, st, T, act, out, false);
}
int earl_tabletop3_reset_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const uint8_t* mask, float* obs) {
  return do_reset<3>(cfg, st, mask, nullptr, obs);
}
int earl_tabletop3_eval_episodes_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T, const float* act,
                                     int64_t act_episode_stride, const earl_tabletop_out* out) {
  return do_eval<3>(cfg, st, episodes, T, act, act_episode_stride, out);
}
// host twin of earl_tabletop3_policy_rollout: the single-object loops (tabletop_policy.h) on Lane<3> and the 20-wide observation
int earl_tabletop3_policy_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_policy_population* pop,
                                      const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out,
                                      const earl_episode_summary* summary) {
  if (int rc = check_population(cfg, st, policy, pop, head, episodes, T, reset_first, out, 3)) return rc;
  if (cfg->n == 0) return EARL_OK;
  const PopulationArgs a = population_args(cfg, st, policy, pop, head, episodes, T, reset_first, out, act_out, summary, thresholds());
  const bool general = cfg->auto_reset != 0;
  for_each_env(cfg->n, [&](int i) {
    const float* params = a.p.params + population_param_offset(a.pop, a.k.cfg.env_offset + i);
    if (head) general ? gaussian_rollout_env<true, 3>(a, i, params, &a.sum) : gaussian_rollout_env<false, 3>(a, i, params, &a.sum);
    else general ? policy_rollout_env<true, 3>(a, i, params, &a.sum) : policy_rollout_env<false, 3>(a, i, params, &a.sum);
  });
  return EARL_OK;
}
// host twin of earl_tabletop3_pair_rollout: pair_rollout_env (tabletop_policy.h) on Lane<3>, the 20-wide observation and the 10-wide goal row
int earl_tabletop3_pair_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                    const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out) {
  if (int rc = check_pair(cfg, st, policy, pair, head, episodes, T, reset_first, out, 3)) return rc;
  if (cfg->n == 0) return EARL_OK;
  const PairArgs a = pair_args(cfg, st, policy, pair, head, episodes, T, reset_first, out, act_out, thresholds(), 3);
  for_each_env(cfg->n, [&](int i) { pair_rollout_env<3>(a, i, head != nullptr); });
  return EARL_OK;
}
int earl_tabletop3_reward_cpu(int32_t n, const float* obs, int32_t reward_type, float* reward, uint8_t* success) {
  if (n < 0 || !obs) return fail(EARL_ERR_ARG, "bad n/obs");
  if (reward_type != EARL_REWARD_SPARSE && reward_type != EARL_REWARD_DENSE) return fail(EARL_ERR_ARG, "reward_type = %d", reward_type);
  const Thresholds th = thresholds();
  for_each_env(n, [&](int i) { reward_body<3>(i, obs, reward_type, 0, reward, success, th); });
  return EARL_OK;
}

// include/earl_physics.h: the policy contract as plain loops, any input / action width (the oracle of the Sawyer rollout's in-kernel policy)
int32_t earl_mlp_policy_forward_cpu(const earl_mlp_policy* p, const earl_gaussian_head* h, int32_t n, const float* obs, const float* eps, float* actions) {
  if (!p || !p->params || !obs || !actions || n < 0) return fail(EARL_ERR_ARG, "policy/params/obs/actions is NULL or n < 0");
  if (int rc = contract::check_form(*p, g_err, contract::kBf16Params)) return rc;
  for (int l = 0; l < p->n_layers; ++l)                    // (its own width rule: any width 1..256 at every position, the input included)
    if (p->dims[l] < 1 || p->dims[l] > kPolicyMaxWidth) return fail(EARL_ERR_ARG, "policy dims[%d] = %d: 1..256", l, p->dims[l]);
  const int NL = p->dims[p->n_layers];
  if (NL < 1 || NL > kPolicyMaxWidth || (h && NL % 2)) return fail(EARL_ERR_ARG, "policy output width %d", NL);
  if (h && contract::check_head(*h, g_err)) return EARL_ERR_ARG;
  const int A = h ? NL / 2 : NL;
  earl_gaussian_head head = h ? *h : contract::default_head();
  if (!eps) head.mode = EARL_HEAD_MEAN;
  for_each_env(n, [&](int i) {
    float buf[2][kPolicyMaxWidth];
    const float* in = obs + (size_t)i * p->dims[0];
    // parameter e of the packing order: the float32 itself, or (EARL_PRECISION_BF16) the stored uint16_t widened exactly, u << 16
    const uint16_t* const stored = reinterpret_cast<const uint16_t*>(p->params);
    const bool bf16 = p->precision == EARL_PRECISION_BF16;
    auto param = [&](size_t e) {
      if (!bf16) return p->params[e];
      return __builtin_bit_cast(float, (uint32_t)stored[e] << 16);
    };
    size_t w = 0;
    for (int l = 0; l < p->n_layers; ++l) {
      const int K = p->dims[l], N = p->dims[l + 1];
      const size_t b = w + (size_t)N * K;
      float* dst = buf[l & 1];
      for (int j = 0; j < N; ++j) {
        float acc = param(b + j);
        for (int k = 0; k < K; ++k) acc = fmaf(in[k], param(w + (size_t)j * K + k), acc);
        dst[j] = l + 1 < p->n_layers ? policy_act(acc, p->hidden_act) : acc;
      }
      in = dst;
      w = b + N;
    }
    for (int d = 0; d < A; ++d)
      actions[(size_t)i * A + d] = h ? gaussian_head_action(head, p->out_act, in[d], in[A + d], eps ? eps[(size_t)i * A + d] : 0.0f) : policy_act(in[d], p->out_act);
  });
  return EARL_OK;
}
// include/earl_physics.h, "discount and a terminal value on the door and the peg": the value kernel's work on given rows -- sawyer_value.h's per-element functions
// around the loops above
int32_t earl_sawyer_value_terminal_cpu(const earl_plan_value* pv, int32_t H, int32_t rows, const double* last_obs, double* ret) {
  if (!pv || !last_obs || !ret || rows < 0 || H < 0) return fail(EARL_ERR_ARG, "pv/last_obs/ret is NULL, or rows or H < 0");
  if (int rc = check_sawyer_value(pv, g_err, 0)) return rc;
  if (!pv->value || rows == 0) return EARL_OK;
  const double d_H = svalue_discount(pv->discount, H);
  std::vector<float> x((size_t)rows * 14), V((size_t)rows);
  for (size_t e = 0; e < x.size(); ++e) x[e] = svalue_row(last_obs[e]);
  if (int rc = earl_mlp_policy_forward_cpu(pv->value, nullptr, rows, x.data(), nullptr, V.data())) return rc;
  for_each_env(rows, [&](int i) {
    bool nan_row = false;
    for (int c = 0; c < 14; ++c) nan_row = nan_row || last_obs[(size_t)i * 14 + c] != last_obs[(size_t)i * 14 + c];
    ret[i] = svalue_terminal(ret[i], d_H, V[i], nan_row);
  });
  return EARL_OK;
}
// include/earl_physics.h, "policy-prior branches on the door and the peg": the action rows of prior branch k for GIVEN observation rows -- the float32 rounding, the
// loops above, then the planner's noise function (sawyer_shoot.h: shoot_candidate around u, with the prior's sigma; k >= 1 always, branch 0 being the plan).  cem != 0: the
// block CEM's branch k would have drawn (tabletop_cem.h: kCemDraw).  No host stepper: the rows are the caller's
int32_t earl_sawyer_prior_actions_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_prior* prior, int32_t H, int32_t k, int32_t j, uint32_t noise_counter, int32_t cem,
                                      const double* obs, float* act) {
  if (!cfg || !prior || !prior->policy || !obs || !act) return fail(EARL_ERR_ARG, "cfg/prior/policy/obs/act is NULL");
  if (cfg->n < 0 || H < 0 || H > 65536 || k < 1 || k >= EARL_SAWYER_PLAN_MAX_K || j < 0 || j > 255)
    return fail(EARL_ERR_ARG, "n = %d, H = %d, k = %d, j = %d: n >= 0, H in 0 .. 65536, k in 1 .. %d, j in 0 .. 255", cfg->n, H, k, j, EARL_SAWYER_PLAN_MAX_K - 1);
  if (int rc = contract::check_policy(*prior->policy, 14, 4, nullptr, 0, g_err)) return rc;
  for (int d = 0; d < 4; ++d)
    if (!std::isfinite(prior->sigma[d]) || !(prior->sigma[d] >= 0)) return fail(EARL_ERR_ARG, "prior->sigma[%d] = %g: finite and >= 0", d, (double)prior->sigma[d]);
  const size_t rows = (size_t)H * (size_t)cfg->n;
  if (rows == 0) return EARL_OK;
  std::vector<float> x(rows * 14), u(rows * 4);
  for (size_t e = 0; e < x.size(); ++e) x[e] = svalue_row(obs[e]);
  if (int rc = earl_mlp_policy_forward_cpu(prior->policy, nullptr, (int32_t)rows, x.data(), nullptr, u.data())) return rc;
  const uint32_t word0 = (cem ? kCemDraw : kPlanDraw) | (uint32_t)j;
  for (int t = 0; t < H; ++t)
    for (int i = 0; i < cfg->n; ++i) {
      const size_t r = ((size_t)t * cfg->n + i) * 4;
      const float m[4] = {u[r], u[r + 1], u[r + 2], u[r + 3]};
      float c[4];
      shoot_candidate(word0, (uint32_t)(cfg->env_offset + i), (uint32_t)k, (uint32_t)t, noise_counter, cfg->seed, prior->sigma, m, c);
      for (int d = 0; d < 4; ++d) act[r + d] = c[d];
    }
  return EARL_OK;
}
// the contract's scalar functions (csrc/policy_math.h), for callers that restate a policy on the host
float earl_tanh_f32(float x) { return tanh_f32(x); }
float earl_exp_f32(float x) { return exp_f32(x); }
float earl_normal_quantile_f32(uint32_t k24) { return normal_quantile_f32(k24 & 0xFFFFFFu); }

// include/earl_physics.h: the Sawyer planner's own arithmetic as plain loops over sawyer_shoot.h's and sawyer_plan.h's per-element functions -- the candidates kernel's (the
// walk above) and the update kernel's, one env at a time with k ascending (integer sums: the kernel's split over lanes gives the same bits).  No host stepper: the returns
// of the update are the caller's.
int32_t earl_sawyer_plan_candidates_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, float* act_out) {
  if (int rc = check_sawyer_plan(SawyerPlanCall::Candidates, cfg, params, j, mean, act_out)) return rc;
  if (cfg->n == 0) return EARL_OK;
  sawyer_candidates_walk(cfg, params->K, params->H, kPlanDraw | (uint32_t)j, params->noise_counter, act_out, [&](int i, int t, float (&m)[4], float (&scale)[4]) {
    shoot_mean(mean, cfg->n, i, t, m);
    for (int d = 0; d < 4; ++d) scale[d] = params->sigma[d];
  });
  return EARL_OK;
}
int32_t earl_sawyer_plan_update_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, const float* act, const double* ret,
                                    float* plan, double* ret0_row, double* best_ret, int32_t* best_k) {
  if (int rc = check_sawyer_plan(SawyerPlanCall::Update, cfg, params, j, mean, plan)) return rc;
  if (!act || !ret) return fail(EARL_ERR_ARG, "act/ret is NULL");
  SawyerPlanArgs p = sawyer_plan_args(cfg, params, mean);
  p.plan = plan;
  p.ret = ret;
  const int n = p.n, K = p.K;
  for_each_env(n, [&](int i) {
    double beta = -INFINITY;
    int bk = 0;
    for (int k = 0; k < K; ++k) plan_best(ret[(size_t)k * n + i], k, beta, bk);
    std::vector<int32_t> Wk(K);
    for (int k = 0; k < K; ++k) Wk[k] = plan_weight(ret[(size_t)k * n + i], beta, p.inv_temperature);
    for (int t = 0; t < p.H; ++t) {
      float m[4];
      shoot_mean(p.mean, n, i, t, m);
      int64_t A[4] = {0, 0, 0, 0}, S = 0;
      for (int k = 0; k < K; ++k) {
        const int32_t W = Wk[k];
        S += W;
        if (W != 0 && k > 0) {
          const float* src = act + shoot_act_index(p.H, n, i, k, t);
          const float c[4] = {src[0], src[1], src[2], src[3]};
          splan_accumulate(c, m, W, A);
        }
      }
      for (int d = 0; d < 4; ++d) plan[((size_t)t * n + i) * 4 + d] = plan_new_mean(m[d], A[d], S);
    }
    if (ret0_row) ret0_row[i] = ret[i];
    if (best_ret) best_ret[i] = beta;
    if (best_k) best_k[i] = bk;
  });
  return EARL_OK;
}

// include/earl_physics.h, "MPPI planning on the minitaur": the same two walks over minitaur_plan.h's per-element functions, eight action dimensions
int32_t earl_minitaur_plan_candidates_cpu(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* params, int32_t j, const float* mean, float* act_out) {
  if (int rc = check_minitaur_plan(MinitaurPlanCall::Candidates, cfg, params, j, mean, act_out)) return rc;
  const int n = cfg->n, K = params->K, H = params->H;
  if (n == 0) return EARL_OK;
  float sigma[8];
  for (int d = 0; d < 8; ++d) sigma[d] = params->sigma[d];
  const uint32_t word0 = kPlanDraw | (uint32_t)j;
  const long long rows = (long long)K * H;
#pragma omp parallel for schedule(static) if (rows * n >= 4096)
  for (long long kt = 0; kt < rows; ++kt) {
    const int k = (int)(kt / H), t = (int)(kt - (long long)k * H);
    for (int i = 0; i < n; ++i) {
      float m[8], c[8];
      mtplan_mean(mean, n, i, t, m);
      mtplan_candidate(word0, (uint32_t)(cfg->env_offset + i), (uint32_t)k, (uint32_t)t, params->noise_counter, cfg->seed, sigma, m, c);
      float* dst = act_out + mtplan_act_index(H, n, i, k, t);
      for (int d = 0; d < 8; ++d) dst[d] = c[d];
    }
  }
  return EARL_OK;
}
int32_t earl_minitaur_plan_update_cpu(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* params, int32_t j, const float* mean, const float* act, const double* ret,
                                      float* plan, double* ret0_row, double* best_ret, int32_t* best_k) {
  if (int rc = check_minitaur_plan(MinitaurPlanCall::Update, cfg, params, j, mean, plan)) return rc;
  if (!act || !ret) return fail(EARL_ERR_ARG, "act/ret is NULL");
  MinitaurPlanArgs p = minitaur_plan_args(cfg, params, mean);
  const int n = p.n, K = p.K;
  for_each_env(n, [&](int i) {
    double beta = -INFINITY;
    int bk = 0;
    for (int k = 0; k < K; ++k) plan_best(ret[(size_t)k * n + i], k, beta, bk);
    std::vector<int32_t> Wk(K);
    for (int k = 0; k < K; ++k) Wk[k] = plan_weight(ret[(size_t)k * n + i], beta, p.inv_temperature);
    for (int t = 0; t < p.H; ++t) {
      float m[8];
      mtplan_mean(p.mean, n, i, t, m);
      int64_t A[8] = {0, 0, 0, 0, 0, 0, 0, 0}, S = 0;
      for (int k = 0; k < K; ++k) {
        const int32_t W = Wk[k];
        S += W;
        if (W != 0 && k > 0) {
          const float* src = act + mtplan_act_index(p.H, n, i, k, t);
          const float c[8] = {src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7]};
          mtplan_accumulate(c, m, W, A);
        }
      }
      for (int d = 0; d < 8; ++d) plan[((size_t)t * n + i) * 8 + d] = plan_new_mean(m[d], A[d], S);
    }
    if (ret0_row) ret0_row[i] = ret[i];
    if (best_ret) best_ret[i] = beta;
    if (best_k) best_k[i] = bk;
  });
  return EARL_OK;
}

// include/earl_physics.h, "CEM planning on the door and the peg": the same two walks over sawyer_shoot.h's and sawyer_cem.h's per-element functions.  The elites of an
// env are the first E of a sort under cem_before (the order of item 4 itself, where the kernel runs a radix select over its keys) that are not NaN; the moments are
// integer sums, so the order in which the elites are added gives the same bits as the kernel's split over lanes.
int32_t earl_sawyer_cem_candidates_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out) {
  if (int rc = check_sawyer_cem(SawyerCemCall::Candidates, cfg, params, j, mean, std, act_out, nullptr)) return rc;
  if (cfg->n == 0) return EARL_OK;
  const SawyerCemArgs p = sawyer_cem_args(cfg, params, mean, std);
  sawyer_candidates_walk(cfg, p.K, p.H, kCemDraw | (uint32_t)j, p.noise_counter, act_out, [&](int i, int t, float (&m)[4], float (&scale)[4]) {
    shoot_mean(mean, p.n, i, t, m);
    scem_std(p, i, t, scale);
  });
  return EARL_OK;
}
int32_t earl_sawyer_cem_update_cpu(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std_in, const float* act,
                                   const double* ret, float* plan, float* std, double* ret0_row, double* best_ret, int32_t* best_k, uint8_t* elite) {
  if (int rc = check_sawyer_cem(SawyerCemCall::Update, cfg, params, j, mean, std_in, plan, std)) return rc;
  if (!act || !ret) return fail(EARL_ERR_ARG, "act/ret is NULL");
  SawyerCemArgs p = sawyer_cem_args(cfg, params, mean, std_in);
  const int n = p.n, K = p.K;
  for_each_env(n, [&](int i) {
    double beta = -INFINITY;
    int bk = 0;
    std::vector<int> order(K);
    for (int k = 0; k < K; ++k) {
      plan_best(ret[(size_t)k * n + i], k, beta, bk);
      order[k] = k;
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return cem_before(ret[(size_t)a * n + i], a, ret[(size_t)b * n + i], b); });
    int32_t Ne = 0;
    while (Ne < p.E && cem_elite(ret[(size_t)order[Ne] * n + i], Ne, p.E)) ++Ne;      // (the NaNs stand last: the first of them ends the elites)
    if (elite) {
      for (int k = 0; k < K; ++k) elite[(size_t)k * n + i] = 0;
      for (int e = 0; e < Ne; ++e) elite[(size_t)order[e] * n + i] = 1;
    }
    for (int t = 0; t < p.H; ++t) {
      float m[4], s[4];
      shoot_mean(p.mean, n, i, t, m);
      scem_std(p, i, t, s);
      int64_t A1[4] = {0, 0, 0, 0}, A2[4] = {0, 0, 0, 0};
      for (int e = 0; e < Ne; ++e) {
        const int k = order[e];
        if (k > 0) {
          const float* src = act + shoot_act_index(p.H, n, i, k, t);
          const float c[4] = {src[0], src[1], src[2], src[3]};
          scem_accumulate(c, m, A1, A2);
        }
      }
      for (int d = 0; d < 4; ++d) {
        plan[((size_t)t * n + i) * 4 + d] = cem_new_mean(m[d], A1[d], Ne, p.alpha);
        std[((size_t)t * n + i) * 4 + d] = cem_new_std(s[d], A1[d], A2[d], Ne, p.alpha, p.std_min, p.std_max);
      }
    }
    if (ret0_row) ret0_row[i] = ret[i];
    if (best_ret) best_ret[i] = beta;
    if (best_k) best_k[i] = bk;
  });
  return EARL_OK;
}

int earl_host_set_threads(int n) {
#ifdef _OPENMP
  if (n > 0) omp_set_num_threads(n);
  return omp_get_max_threads();
#else
  (void)n;
  return 1;
#endif
}
const char* earl_host_version(void) { return "earl-host 0.1 (csrc/tabletop_device.h compiled for the host)"; }
const char* earl_host_last_error(void) { return g_err; }

}  // extern "C"

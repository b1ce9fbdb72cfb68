// tabletop_mpc.h -- earl_tabletop[3]_mpc_rollout (include/earl_tabletop.h, "receding-horizon MPPI control"): what the gfx950 kernel (tabletop_mpc.hip: one
// workgroup per env, one lane per branch) and the host twin (tabletop_host.cpp: one OpenMP iteration per env, the branches in ascending k) share.  The arithmetic
// is tabletop_step.h's wrapped_step and tabletop_plan.h's plan_clip, plan_candidate, plan_best / plan_best_merge, plan_weight, plan_accumulate, plan_new_mean.  This
// file owns the loop's argument blocks and argument rules, mpc_score and mpc_act: they only say which plan rows, counters and output rows those functions are called
// with; the plan lives with the caller (LDS / a host array) behind `row(t, m)`, which hands out the CLIPPED row t of the plan entering the iteration.
#pragma once
#include "tabletop_hostside.h"
#include "tabletop_plan.h"

namespace earl {

struct MpcArgs {
  PlanArgs p;              // plan_args(): a.T = H, a.st the state (read at entry, written at exit); a.out = the rollout's rows [T, n]; mean / plan / ret unused
  earl_mpc_out m;
  int32_t T;
  int32_t iterations;
  int32_t iteration0;
};

// earl_tabletop[3]_mpc_rollout_value: the loop's block followed by the discount and the value network (as PlanValueArgs after PlanArgs)
struct MpcValueArgs : MpcArgs {
  ValueArgs v;
};

// the env word by word (the struct's padding stays where it is: a whole-struct copy out of LDS goes through private memory)
template <int NOBJ>
__device__ __forceinline__ void copy_lane(Lane<NOBJ>& dst, const Lane<NOBJ>& src) {
#pragma unroll
  for (int j = 0; j < Dims<NOBJ>::NQ; ++j) dst.e.q[j] = src.e.q[j];
  dst.e.attached = src.e.attached;
  dst.goal_idx = src.goal_idx;
  dst.steps = src.steps;
  dst.sgc = src.sgc;
  dst.lret = src.lret;
  dst.resets = src.resets;
}

// the return of branch k of env i from the state (L, g) -- plan_score_body's loop on a COPY of the registers the real env lives in, look-ahead step t at `counter` + t.
// VALUE (v != NULL): the discounted sum and the value network on the last row, as plan_score_body<.., true>
template <int NOBJ, bool GENERAL, bool VALUE = false, class Row>
__device__ __forceinline__ double mpc_score(const PlanArgs& q, int i, int k, uint64_t counter, const Lane<NOBJ>& L, const float (&g)[Dims<NOBJ>::NG], Row&& row,
                                            const ValueArgs* v = nullptr) {
  Lane<NOBJ> B;
  copy_lane<NOBJ>(B, L);
  float gb[Dims<NOBJ>::NG];
#pragma unroll
  for (int j = 0; j < Dims<NOBJ>::NG; ++j) gb[j] = g[j];
  double ret = 0.0;
  [[maybe_unused]] double disc = 1.0;
  float o[Dims<NOBJ>::NOBS];
  for (int t = 0; t < q.a.T; ++t) {
    float m[3];
    row(t, m);
    float c[3] = {m[0], m[1], m[2]};
    if (k > 0) plan_candidate(q, i, (uint32_t)k, (uint32_t)t, m, c);
    float reward;
    bool done, succ;
    if constexpr (VALUE) {   // (the last step without its auto-reset, the row made again after the loop: plan_score_body)
      wrapped_step<NOBJ, GENERAL>(q.a, i, counter + (uint64_t)t, B, gb, c[0], c[1], c[2], o, reward, done, succ, nullptr, t + 1 < q.a.T);
      value_accumulate(ret, disc, reward, v->discount);
    } else {
      wrapped_step<NOBJ, GENERAL>(q.a, i, counter + (uint64_t)t, B, gb, c[0], c[1], c[2], o, reward, done, succ);
      ret += (double)reward;
    }
  }
  if constexpr (VALUE) {
    if (v->net.params) {
      float ov[Dims<NOBJ>::NOBS];
      make_obs<NOBJ>(B.e, gb, ov);
      ret = value_terminal<Dims<NOBJ>::NOBS>(*v, ov, ret, disc);
    }
  }
  return ret;
}

// real step s of env i with the action a: rollout_body's step at `counter`, its row stored by the caller that passes store = true.  -> done
template <int NOBJ, bool GENERAL>
__device__ __forceinline__ bool mpc_act(const MpcArgs& x, int i, int s, uint64_t counter, Lane<NOBJ>& L, float (&g)[Dims<NOBJ>::NG], const float (&a)[3], bool store) {
  const KArgs& k = x.p.a;
  float o[Dims<NOBJ>::NOBS];
  float reward;
  bool done, succ;
  wrapped_step<NOBJ, GENERAL>(k, i, counter, L, g, a[0], a[1], a[2], o, reward, done, succ);
  if (store) {
    const size_t row = (size_t)s * k.cfg.n + i;
    if (k.out.obs) store_obs<NOBJ>(k.out.obs + row * Dims<NOBJ>::NOBS, o);
    if (k.out.reward) k.out.reward[row] = reward;
    if (k.out.done) k.out.done[row] = done;
    if (k.out.success) k.out.success[row] = succ;
    if (x.m.act) {
      float* dst = x.m.act + row * 3;
      dst[0] = a[0];
      dst[1] = a[1];
      dst[2] = a[2];
    }
  }
  return done;
}

namespace hostside {

// The argument rules of earl_tabletop[3]_mpc_rollout and of its host twin, in the header's order.  *lanes = the workgroup's size (0: nothing to do).
constexpr int kMpcMaxK = EARL_MPC_MAX_K, kMpcMaxH = EARL_MPC_MAX_H;
inline int check_mpc(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int nobj, const earl_plan_params* p, int32_t T, const earl_tabletop_out* out,
                     const earl_mpc_out* mpc, int* lanes) {
  *lanes = 0;
  if (!cfg || !st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  if (!mpc || !mpc->plan) return fail(EARL_ERR_ARG, "mpc / mpc->plan is NULL: the plan is the warm start and the result");
  long long blocks, ublocks;   // the planner's rules with the plan as mean and plan; its `ret` workspace does not exist here (any non-NULL address passes its test)
  if (int rc = check_plan(cfg, st, nobj, p, 0, mpc->plan, mpc->plan, reinterpret_cast<const double*>(mpc->plan), &blocks, &ublocks)) return rc;
  if (!out || (!out->obs && !out->reward && !out->done && !out->success)) return fail(EARL_ERR_ARG, "out is NULL or holds no pointer");
  if (T < 0) return fail(EARL_ERR_ARG, "T = %d < 0", T);
  if (p->K > kMpcMaxK) return fail(EARL_ERR_ARG, "K = %d > %d: one branch per lane of one workgroup", p->K, kMpcMaxK);
  if (p->H > kMpcMaxH) return fail(EARL_ERR_ARG, "H = %d > %d: the plan stays in LDS", p->H, kMpcMaxH);
  const int wg = (p->K + kBranchBlock - 1) / kBranchBlock * kBranchBlock;
  if ((long long)cfg->n * wg > 0xffffffffll) return fail(EARL_ERR_ARG, "n = %d workgroups of %d lanes do not fit one launch (2^32 - 1 lanes)", cfg->n, wg);
  if (T > 0 && cfg->n > 0) *lanes = wg;
  return EARL_OK;
}

inline MpcArgs mpc_args(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, int32_t T, const earl_tabletop_out* out,
                        const earl_mpc_out* mpc) {
  MpcArgs x{};
  x.p = plan_args(cfg, st, pp, nullptr, thresholds());
  x.p.a.out = earl_tabletop_out{out->obs, out->reward, out->done, out->success, nullptr};
  x.m = *mpc;
  x.T = T;
  x.iterations = pp->iterations;
  x.iteration0 = pp->iteration0;
  return x;
}

}  // namespace hostside
}  // namespace earl

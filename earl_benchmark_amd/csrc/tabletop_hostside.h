// tabletop_hostside.h -- host-side helpers of the tabletop entry points shared by libearl_hip.so (tabletop.hip) and libearl_host.so
// (tabletop_host.cpp): the exact comparison thresholds (IEEE sqrt on the host), argument validation, the thread-local error message.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "tabletop_device.h"
#include "policy_check.h"   // contract::check_policy: the value network of the `_value` planner calls (check_plan_value below)

namespace earl {
struct ValueArgs;   // tabletop_value.h: complete wherever value_args (below) is called; not included here, so that the units that never plan do not depend on it
namespace hostside {

inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

// smallest double s with sqrt(s) >= c  (so that  sqrt(d2) < c  <=>  d2 < s)
inline double lt_threshold_f64(double c) {
  double s = c * c;
  while (std::sqrt(s) >= c) s = std::nextafter(s, 0.0);
  while (std::sqrt(s) < c) s = std::nextafter(s, INFINITY);
  return s;
}
// largest float s with (double)sqrtf(s) <= c  (so that  (double)sqrtf(x) <= c  <=>  x <= s)
inline float le_threshold_f32(double c) {
  float s = (float)(c * c);
  while ((double)std::sqrt(s) <= c) s = std::nextafterf(s, INFINITY);
  while ((double)std::sqrt(s) > c) s = std::nextafterf(s, 0.0f);
  return s;
}
inline const Thresholds& thresholds() {
  static const Thresholds th = {lt_threshold_f64(0.4), lt_threshold_f64(1.0), le_threshold_f32(0.2), le_threshold_f32(0.4)};
  return th;
}

// smallest float x with rescale_action(x) > 0: the grip test `rescaled a[2] > 0` (:144) on the RAW action.
// rescale is monotone, so a bisection over the (ordered) non-negative float bit patterns finds it exactly.
inline float grip_threshold() {
  static const float thr = [] {
    auto rescaled_positive = [](float x) {
      const double c = x < -1.0f ? -1.0 : (x > 1.0f ? 1.0 : (double)x);
      volatile double v = -0.2 + ((c + 1.) * 0.5) * (0.2 - -0.2);
      return v > 0;
    };
    uint32_t lo = 0u, hi = 0x3f800000u;  // +0.0f (not positive) .. 1.0f (positive)
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      float f;
      memcpy(&f, &mid, 4);
      if (rescaled_positive(f)) hi = mid; else lo = mid;
    }
    float f;
    memcpy(&f, &hi, 4);
    return f;
  }();
  return thr;
}

inline int check_common(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int nobj) {
  if (!cfg || !st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  if (cfg->n < 0) return fail(EARL_ERR_ARG, "n = %d < 0", cfg->n);
  if (!st->qpos || !st->attached || !st->goal_idx || !st->goal_table || !st->steps_since_reset || !st->num_interventions)
    return fail(EARL_ERR_ARG, "state has a NULL array");
  if (cfg->n_goals < 1 || cfg->n_sample_goals < 1 || cfg->n_sample_goals > cfg->n_goals)
    return fail(EARL_ERR_ARG, "bad goal table sizes n_goals=%d n_sample_goals=%d", cfg->n_goals, cfg->n_sample_goals);
  if (cfg->reward_type != EARL_REWARD_SPARSE && cfg->reward_type != EARL_REWARD_DENSE)
    return fail(EARL_ERR_ARG, "reward_type = %d", cfg->reward_type);
  if (cfg->goal_change_frequency < 0 || cfg->horizon < 0) return fail(EARL_ERR_ARG, "negative horizon/frequency");
  if (cfg->goal_change_frequency > 0 && (!st->steps_since_goal_change || !st->lifelong_return))
    return fail(EARL_ERR_ARG, "lifelong mode needs steps_since_goal_change and lifelong_return");
  if (nobj == 3 && (cfg->wide_init || cfg->goal_change_frequency))
    return fail(EARL_ERR_ARG, "3-object variant: wide_init / lifelong do not exist in the reference class");
  return EARL_OK;
}

// GENERAL of the kernels and the host loops: lifelong goal switching or the auto-reset is on (wrapped_step, tabletop_step.h)
inline bool is_general(const earl_tabletop_cfg* cfg) { return cfg->goal_change_frequency > 0 || cfg->auto_reset; }

// The argument rules of earl_tabletop[3]_branch_rollout and of its host twin (include/earl_tabletop.h), in the header's order.  The device launch is a 1-D grid
// of K * ceil(n / kBranchBlock) workgroups of kBranchBlock lanes; the twin refuses the grids the device refuses.  *blocks = that count (0: nothing to do).
constexpr int kBranchBlock = 64;
inline int check_branch(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int nobj, int32_t K, int32_t H, const float* act, int64_t stride,
                        const earl_episode_summary* summary, const float* last_obs, long long* blocks) {
  *blocks = 0;
  if (int rc = check_common(cfg, st, nobj)) return rc;
  if (!act) return fail(EARL_ERR_ARG, "act is NULL");
  if (K < 0) return fail(EARL_ERR_ARG, "K = %d < 0", K);
  if (H < 0) return fail(EARL_ERR_ARG, "H = %d < 0", H);
  if (stride < 0) return fail(EARL_ERR_ARG, "negative action stride");
  if (stride != 0 && stride < (int64_t)H * cfg->n * 3) return fail(EARL_ERR_ARG, "action stride %lld is neither 0 nor >= H * n * 3 = %lld", (long long)stride, (long long)H * cfg->n * 3);
  if (!summary && !last_obs) return fail(EARL_ERR_ARG, "summary and last_obs are both NULL");
  const long long tiles = ((long long)cfg->n + kBranchBlock - 1) / kBranchBlock, nb = tiles * K;
  if (nb > 0x7fffffffll || nb * kBranchBlock > 0xffffffffll)
    return fail(EARL_ERR_ARG, "K = %d branches of %lld workgroups do not fit one launch (2^31 - 1 workgroups, 2^32 - 1 lanes)", K, tiles);
  if (H > 0) *blocks = nb;
  return EARL_OK;
}

// The argument rules of earl_tabletop[3]_plan_mppi, of earl_tabletop_plan_candidates (st == NULL, j = the iteration: no env state, no iteration range, no
// temperature, `out` = act_out) and of their host twins, in the header's order.  *blocks = the score launch's workgroups, *ublocks = the update launch's
// (kPlanUpdateSteps waves of kBranchBlock envs each); both 0 when n == 0.
constexpr int kPlanUpdateSteps = EARL_PLAN_UPDATE_STEPS;
inline int check_plan(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int nobj, const earl_plan_params* p, int32_t j, const float* mean, const void* out,
                      const double* ret, long long* blocks, long long* ublocks) {
  *blocks = *ublocks = 0;
  if (st) {
    if (int rc = check_common(cfg, st, nobj)) return rc;
  } else {
    if (!cfg) return fail(EARL_ERR_ARG, "cfg is NULL");
    if (cfg->n < 0) return fail(EARL_ERR_ARG, "n = %d < 0", cfg->n);
  }
  if (!p) return fail(EARL_ERR_ARG, "params is NULL");
  if (!mean || !out) return fail(EARL_ERR_ARG, st ? "mean/plan is NULL" : "mean/act_out is NULL");
  if (st && !ret) return fail(EARL_ERR_ARG, "ret is NULL: it is the workspace between the score and the update launch");
  if (p->K < 1 || p->K > 65536) return fail(EARL_ERR_ARG, "K = %d: 1 .. 65536", p->K);
  if (p->H < 1 || p->H > 65536) return fail(EARL_ERR_ARG, "H = %d: 1 .. 65536", p->H);
  if (st) {
    if (p->iterations < 1 || p->iteration0 < 0 || (long long)p->iteration0 + p->iterations > 256)
      return fail(EARL_ERR_ARG, "iterations = %d from iteration0 = %d: at least one, inside 0 .. 255", p->iterations, p->iteration0);
    if (!std::isfinite(p->inv_temperature) || !(p->inv_temperature > 0)) return fail(EARL_ERR_ARG, "inv_temperature = %g: finite and > 0", p->inv_temperature);
  } else if (j < 0 || j > 255) {
    return fail(EARL_ERR_ARG, "iteration %d: 0 .. 255", j);
  }
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(p->sigma[d]) || !(p->sigma[d] >= 0)) return fail(EARL_ERR_ARG, "sigma[%d] = %g: finite and >= 0", d, (double)p->sigma[d]);
  const long long tiles = ((long long)cfg->n + kBranchBlock - 1) / kBranchBlock, nb = tiles * p->K;
  const long long ub = tiles * ((p->H + kPlanUpdateSteps - 1) / kPlanUpdateSteps);
  if (nb > 0x7fffffffll || nb * kBranchBlock > 0xffffffffll)
    return fail(EARL_ERR_ARG, "K = %d branches of %lld workgroups do not fit one launch (2^31 - 1 workgroups, 2^32 - 1 lanes)", p->K, tiles);
  if (st && (ub > 0x7fffffffll || ub * kBranchBlock * kPlanUpdateSteps > 0xffffffffll))
    return fail(EARL_ERR_ARG, "H = %d steps of %lld env tiles do not fit the update launch (2^31 - 1 workgroups, 2^32 - 1 lanes)", p->H, tiles);
  if (st && out != (const void*)mean) {
    const uintptr_t a = (uintptr_t)mean, b = (uintptr_t)out, bytes = (uintptr_t)p->H * (uintptr_t)cfg->n * 12u;
    if (a < b + bytes && b < a + bytes) return fail(EARL_ERR_ARG, "plan overlaps mean without being the same array");
  }
  *blocks = nb;
  *ublocks = ub;
  return EARL_OK;
}

// What earl_tabletop[3]_plan_mppi_value and earl_tabletop[3]_mpc_rollout_value (and their host twins) refuse beyond check_plan / check_mpc: the discount, and the value
// network obs_dim -> hidden (-> hidden) -> 1 under the policy contract (policy_check.h) with the lane's register budget on its first hidden layer.
constexpr int kPlanValueMaxH1 = EARL_PLAN_VALUE_MAX_H1;
inline int check_plan_value(const earl_plan_value* pv, int obs_dim) {
  if (!pv) return fail(EARL_ERR_ARG, "value block is NULL (discount = 1 and value = NULL is the value-free call)");
  if (!(pv->discount > 0.0 && pv->discount <= 1.0)) return fail(EARL_ERR_ARG, "discount = %g: 0 < discount <= 1", pv->discount);   // (NaN fails both comparisons)
  if (!pv->value) return EARL_OK;
  if (int rc = contract::check_policy(*pv->value, obs_dim, 1, nullptr, 0, g_err)) return rc;
  if (pv->value->n_layers == 3 && pv->value->dims[1] > kPlanValueMaxH1)
    return fail(EARL_ERR_ARG, "value network: first hidden width %d of two > %d (a lane holds that layer in registers)", pv->value->dims[1], kPlanValueMaxH1);
  return EARL_OK;
}

// the checked block of a `_value` call as the launch carries it; value == NULL: no terminal term
template <class V = ValueArgs> inline V value_args(const earl_plan_value* pv) { return V{pv->discount, pv->value ? *pv->value : earl_mlp_policy{}}; }

}  // namespace hostside
}  // namespace earl

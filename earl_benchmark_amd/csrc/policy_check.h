// policy_check.h -- the host-side contract of a closed-loop launch's policy arguments (earl_mlp_policy, earl_gaussian_head, earl_policy_population, earl_agent_pair),
// stated once for every entry point that takes them: the tabletop's four (tabletop_policy.h, both libraries), the Sawyer door / peg's four (physics.hip), the
// minitaur's (physics_mt.hip), the kitchen's (physics_kitchen.hip) and earl_mlp_policy_forward_cpu (tabletop_host.cpp).  Host only; it needs the ABI structs and kPolicyMaxWidth and nothing of any env.
// What differs between the callers is an argument: the widths, the rules below, the population's group size, the stride multiple.  Every check returns EARL_OK or
// EARL_ERR_ARG; `err` is NULL (the physics entry points return the bare code) or kErrLen bytes that receive the message (the tabletop's thread-local g_err).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "policy_math.h"

namespace earl {
namespace contract {

constexpr size_t kErrLen = 512;

inline int refuse(char* err, const char* fmt, ...) {
  if (err) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, kErrLen, fmt, ap);
    va_end(ap);
  }
  return EARL_ERR_ARG;
}

// what an entry point asks of a policy beyond the common rules: params 16-byte aligned (the stepper units read the weight rows in 16-byte pieces); out_act tanh
// (the minitaur: the reference env raises on an action outside +-(1 + 0.01) and a kernel cannot); precision may be EARL_PRECISION_BF16 (the stepper entry points, whose
// weights are read from memory at every step, and earl_mlp_policy_forward_cpu: params then holds uint16_t bf16 values, 16-byte aligned whatever the other rules say, and
// every stride counts those elements and is a multiple of 8 of them.  Not the tabletop's: its weights sit in registers for the whole launch, so a narrower stored
// format buys nothing there)
enum : unsigned { kParamsAligned16 = 1u, kBoundedOutput = 2u, kBf16Params = 4u };

// elements of the stored type in a 16-byte piece: what every stride of a launch whose rows are read in such pieces is a multiple of
inline int stride_multiple(const earl_mlp_policy& p) { return p.precision == EARL_PRECISION_BF16 ? 8 : 4; }

// the head of a launch without one (the kernels' argument structs always carry a head)
inline earl_gaussian_head default_head() { return earl_gaussian_head{EARL_HEAD_MEAN, EARL_LOGSTD_CLAMP, 0.0f, 0.0f, nullptr}; }

// parameters (elements of the stored type) of one policy in the packing order W_0, b_0, W_1, b_1, ...  (after check_form: n_layers is 2 or 3)
inline int64_t mlp_param_count(const earl_mlp_policy& p) {
  int64_t count = 0;
  for (int l = 0; l < p.n_layers; ++l) count += (int64_t)p.dims[l + 1] * (p.dims[l] + 1);
  return count;
}

// precision, layer count and activations: what holds whatever the widths are
inline int check_form(const earl_mlp_policy& p, char* err, unsigned rules = 0) {
  if (p.precision == EARL_PRECISION_BF16 && !(rules & kBf16Params))
    return refuse(err, "policy precision = %d (bf16): the stepper envs and earl_mlp_policy_forward_cpu take it; this entry point takes 0 (fp32) only", p.precision);
  if (p.precision != 0 && p.precision != EARL_PRECISION_BF16) return refuse(err, "policy precision = %d: 0 (fp32) or %d (bf16)", p.precision, EARL_PRECISION_BF16);
  if (p.precision == EARL_PRECISION_BF16 && ((uintptr_t)p.params & 15)) return refuse(err, "policy params (bf16) is not 16-byte aligned");
  if (p.n_layers != 2 && p.n_layers != 3) return refuse(err, "policy n_layers = %d: 2 (one hidden layer) or 3 (two)", p.n_layers);
  if (p.hidden_act != EARL_ACT_RELU && p.hidden_act != EARL_ACT_TANH) return refuse(err, "policy hidden_act = %d", p.hidden_act);
  if (p.out_act != EARL_ACT_NONE && p.out_act != EARL_ACT_TANH) return refuse(err, "policy out_act = %d", p.out_act);
  return EARL_OK;
}

inline int check_head(const earl_gaussian_head& h, char* err) {
  if (h.mode != EARL_HEAD_MEAN && h.mode != EARL_HEAD_SAMPLE) return refuse(err, "head mode = %d", h.mode);
  if (h.log_std_map != EARL_LOGSTD_CLAMP && h.log_std_map != EARL_LOGSTD_TANH) return refuse(err, "head log_std_map = %d", h.log_std_map);
  if (!(h.log_std_min >= -20.0f && h.log_std_max <= 4.0f && h.log_std_min <= h.log_std_max))       // (NaN fails every comparison)
    return refuse(err, "head log_std bounds [%g, %g]: finite, min <= max, inside [-20, 4]", (double)h.log_std_min, (double)h.log_std_max);
  return EARL_OK;
}

// one policy obs_dim -> hidden (-> hidden) -> act_dim of an in-kernel launch; head: NULL, or the Gaussian head of a last layer 2 act_dim wide (mean, raw log_std)
inline int check_policy(const earl_mlp_policy& p, int obs_dim, int act_dim, const earl_gaussian_head* head, unsigned rules, char* err) {
  if (!p.params) return refuse(err, "policy params is NULL");
  if ((rules & kParamsAligned16) && ((uintptr_t)p.params & 15)) return refuse(err, "policy params is not 16-byte aligned");
  if (int rc = check_form(p, err, rules)) return rc;
  const int out_dim = head ? 2 * act_dim : act_dim;
  if (p.dims[0] != obs_dim || p.dims[p.n_layers] != out_dim)
    return refuse(err, "policy dims: input %d, output %d (want %d and %d)", p.dims[0], p.dims[p.n_layers], obs_dim, out_dim);
  for (int l = 1; l < p.n_layers; ++l)
    if (p.dims[l] < 16 || p.dims[l] > kPolicyMaxWidth || p.dims[l] % 16) return refuse(err, "policy hidden width %d: a multiple of 16 in 16..256", p.dims[l]);
  if (p.n_layers == 2 && p.dims[3] != 0) return refuse(err, "policy dims[3] = %d is unused and must be 0", p.dims[3]);
  if ((rules & kBoundedOutput) && p.out_act != EARL_ACT_TANH) return refuse(err, "policy out_act = %d: this env takes bounded policies only (EARL_ACT_TANH)", p.out_act);
  return head ? check_head(*head, err) : EARL_OK;
}

// a population of checked policies over the envs with global ids env_offset .. env_offset + n - 1: `group` envs share their weights' loads (16 everywhere today), and
// the rows of params are a multiple of `stride_multiple` elements apart (4 floats / 8 bf16 values where a member's rows are read in 16-byte pieces)
inline int check_population(const earl_mlp_policy& p, const earl_policy_population& pop, int32_t env_offset, int32_t n, int group, int stride_multiple, char* err) {
  if (pop.n_policies < 1) return refuse(err, "population n_policies = %d < 1", pop.n_policies);
  if (pop.envs_per_policy < group || pop.envs_per_policy % group)
    return refuse(err, "population envs_per_policy = %d: a multiple of %d, >= %d", pop.envs_per_policy, group, group);
  const int64_t count = mlp_param_count(p);
  if (pop.param_stride < count) return refuse(err, "population param_stride = %lld < %lld parameters of one policy", (long long)pop.param_stride, (long long)count);
  if (pop.param_stride % stride_multiple) return refuse(err, "population param_stride = %lld: a multiple of %d", (long long)pop.param_stride, stride_multiple);
  if (env_offset < 0) return refuse(err, "population: env_offset = %d < 0", env_offset);
  const int64_t last = (int64_t)env_offset + n - 1;
  if (n > 0 && last / pop.envs_per_policy >= pop.n_policies)
    return refuse(err, "population: global env id %lld runs policy %lld of %d", (long long)last, (long long)(last / pop.envs_per_policy), pop.n_policies);
  return EARL_OK;
}

// the forward / reset pair of a checked policy; goal_change_frequency: the env's (the pair IS the lifelong mechanism)
inline int check_pair(const earl_mlp_policy& p, const earl_agent_pair* pair, int32_t goal_change_frequency, int stride_multiple, char* err) {
  if (!pair) return refuse(err, "pair is NULL");
  if (!pair->phase || !pair->steps_in_phase) return refuse(err, "pair phase/steps_in_phase is NULL");
  for (int k = 0; k < 2; ++k)
    if (pair->switch_every[k] < 1) return refuse(err, "pair switch_every[%d] = %d < 1", k, pair->switch_every[k]);
  if (pair->switch_on_success != 0 && pair->switch_on_success != 1) return refuse(err, "pair switch_on_success = %d", pair->switch_on_success);
  const int64_t count = mlp_param_count(p);
  if (pair->param_stride < count) return refuse(err, "pair param_stride = %lld < %lld parameters of one agent", (long long)pair->param_stride, (long long)count);
  if (pair->param_stride % stride_multiple) return refuse(err, "pair param_stride = %lld: a multiple of %d", (long long)pair->param_stride, stride_multiple);
  if (goal_change_frequency > 0)
    return refuse(err, "pair: goal_change_frequency = %d > 0 (the pair is the lifelong mechanism: the two clocks would fight over the same draw)", goal_change_frequency);
  return EARL_OK;
}

// a population of PAIRS (earl_sawyer_agents_rollout): params is [P, 2, pair->param_stride], so a member's two rows fit between two members' starts
inline int check_pair_population(const earl_policy_population& pop, const earl_agent_pair& pair, char* err) {
  if (pop.param_stride < 2 * pair.param_stride)
    return refuse(err, "population param_stride = %lld < 2 x pair param_stride = %lld (a member is a forward and a reset row)", (long long)pop.param_stride,
                  (long long)(2 * pair.param_stride));
  return EARL_OK;
}

// the reset agent's table of backward goals next to a checked pair; n_goal_rows: the env's forward goal table (0: the forward goal could not be restored).
// A template: the struct is include/earl_physics.h's, which only the stepper units see
template <class Goals>
inline int check_backward_goals(const Goals& goals, const earl_agent_pair& pair, int32_t n_goal_rows, char* err) {
  if (!goals.table) return refuse(err, "backward goals: table is NULL");
  if (goals.n_rows < 1) return refuse(err, "backward goals: n_rows = %d < 1", goals.n_rows);
  if (pair.backward_goal) return refuse(err, "backward goals: a table AND pair backward_goal (one of them)");
  if (n_goal_rows == 0) return refuse(err, "backward goals: the env has no goal table (the forward goal could not be restored)");
  return EARL_OK;
}

// The whole contract of a closed-loop launch of a stepper env (Sawyer, minitaur, kitchen), in the order the entry points applied it: the policy obs_dim -> .. ->
// act_dim under `rules` with its head; the population (NULL: one policy) over the global ids env_offset .. env_offset + n - 1; the pair (NULL: none) with the env's
// goal_change_frequency, its population and its table of backward goals (NULL: none).  n_forward_rows: the rows of the forward goal table the launch can draw from; a
// pair with a backward goal -- one row or a table -- needs one at least (the forward goal could not be restored).  Everywhere: groups of 16 envs share their weights'
// loads, and every stride is a multiple of 4 floats -- of 8 bf16 values -- (the rows are read in 16-byte pieces)
template <class Goals>
inline int check_closed_loop(const earl_mlp_policy& p, int obs_dim, int act_dim, unsigned rules, const earl_gaussian_head* head, const earl_policy_population* pop,
                             int32_t env_offset, int32_t n, const earl_agent_pair* pair, int32_t goal_change_frequency, const Goals* goals, int32_t n_forward_rows,
                             char* err) {
  if (int rc = check_policy(p, obs_dim, act_dim, head, rules, err)) return rc;
  if (pop)
    if (int rc = check_population(p, *pop, env_offset, n, 16, stride_multiple(p), err)) return rc;
  if (!pair) return EARL_OK;
  if (int rc = check_pair(p, pair, goal_change_frequency, stride_multiple(p), err)) return rc;
  if (pair->backward_goal && n_forward_rows < 1) return refuse(err, "pair backward_goal: the env has no forward goal table (the forward goal could not be restored)");
  if (pop)
    if (int rc = check_pair_population(*pop, *pair, err)) return rc;
  return goals ? check_backward_goals(*goals, *pair, n_forward_rows, err) : EARL_OK;
}

}  // namespace contract
}  // namespace earl

// physics_kitchen.hip -- fifth build of the articulated-body stepper: the KITCHEN (BASELINE configs[3]).
//
// The stepper (physics_stepper.h) instantiated for nv = 23 (32 lanes per env, arm block + fixtures solver, joint couplings, dry friction, springs, force-limited actuators) plus the kitchen env
// kernels (physics_env_kitchen.h: the per-step kernels, the fused rollout, the fused rollout with an MLP policy inside) and the entry points earl_kitchen_step / earl_kitchen_rollout /
// earl_kitchen_policy_rollout / earl_kitchen_population_rollout; earl_physics_step / _forward of the
// main unit forward nv = 23 here.  A translation unit of its own (round 5): the main unit's compile time was 50 s with it.
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_kitchen.h"
}  // namespace

#include "physics_launch.h"

// the rules of an env's cfg / st that every entry point has; fused: the rollout kernels', which hold the attachment rows in 32 lanes and read the mocap orientation themselves
static bool kitchen_args_ok(const earl_kitchen_cfg* cfg, const earl_kitchen_state* st, bool fused) {
  if (cfg->n < 0 || cfg->n_att < 10 || cfg->frame_skip < 0 || (fused && (cfg->n_att > 32 || !cfg->mocap_quat_dev))) return false;
  if (!st->qpos || !st->qvel || !st->mocap_pos || !st->goal || !st->last_qp_robot || !st->att_xpos || !st->steps_since_reset || !st->last_obs) return false;
  for (int k = 0; k < 8; ++k) if (cfg->site_att[k] < 0 || cfg->site_att[k] >= cfg->n_att) return false;
  return true;
}
// the launch form of a fused rollout, for the plain and the closed-loop entry point alike: solo_mode's value, by default promoted to the multi-wave forms
static int kitchen_solo(int n) {
  const int solo = solo_mode(n);
  if (g_solo < 0 && solo == 2) return 3;   // one env per workgroup: four waves per env (rows | mass matrix | bias forces | collision, then one wave's active set)
  return g_solo < 0 && solo == 1 && n <= 2 * cu_count() ? 4 : solo;      // 4: at most two envs per CU: two envs per workgroup, two waves per env
}

extern "C" {

void earl_unit_kitchen_physics(const void* pargs, int integrate, void* stream) {
  const PArgs& a = *static_cast<const PArgs*>(pargs);
  const hipStream_t st = (hipStream_t)stream;
  if (integrate) physics_kernel<23, 32, true><<<grid_for<23, 32>(a.n), block_for<23>(), 0, st>>>(a);     // 32 lanes per env: two envs per wave
  else physics_kernel<23, 32, false><<<grid_for<23, 32>(a.n), block_for<23>(), 0, st>>>(a);
}
int earl_kitchen_step(const void* model, const earl_collision_model* col, const earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                      const earl_kitchen_state* st, const float* action, const earl_kitchen_out* out, earl_stream_t stream) {
  if (!model || !params || !cfg || !st || !action || !out || !kitchen_args_ok(cfg, st, false)) return EARL_ERR_ARG;
  if (!st->action64 || !st->ctrl9 || !st->qpos_bak || !st->qvel_bak || !st->sites || !st->bad || !st->mocap_bak || !st->att_bak || (cfg->sensor_noise && !st->noise)) return EARL_ERR_ARG;
  if (!out->obs || !out->reward || !out->done || !out->success) return EARL_ERR_ARG;
  const int n = cfg->n;
  if (n == 0) return EARL_OK;
  const hipStream_t hs = (hipStream_t)stream;
  if (int rc = check_cone(col, false, hs, "kitchen_step")) return rc;
  KitchenArgs k{*cfg, *st, *out, action, cfg->n_att};
  kitchen_pre_kernel<<<(n * 23 + 255) / 256, 256, 0, hs>>>(k);
  // KitchenV0.step up to do_simulation: mocap target, the nine position targets (csrc/glue.hip)
  if (int rc = earl_kitchen_action(n, params, st->action64, st->mocap_pos, st->last_qp_robot, st->ctrl9, stream)) return rc;
  // do_simulation: ctrl[i] = targets[i] for i < nu = 2, frame_skip timesteps (adept_envs/mujoco_env.py:148-157)
  PArgs a{model, col, n, cfg->frame_skip, st->qpos, st->qvel, st->mocap_pos, cfg->mocap_quat_dev, st->ctrl9, st->att_xpos, nullptr, nullptr, 9, 0};
  earl_unit_kitchen_physics(&a, 1, stream);
  kitchen_guard_kernel<<<(n + 255) / 256, 256, 0, hs>>>(k);
  // Robot.get_obs + KitchenV0._get_obs: sensor noise from Philox draws keyed by the global env id
  if (cfg->sensor_noise)
    if (int rc = earl_philox_uniform(n, 46, cfg->seed, cfg->counter, cfg->env_offset, 0x4B00u, -1.0, 1.0, st->noise, stream)) return rc;
  if (int rc = earl_kitchen_obs(n, params, st->qpos, st->goal, cfg->sensor_noise ? st->noise : nullptr, out->obs, stream)) return rc;
  if (int rc = earl_kitchen_reward(n, out->obs, st->mocap_pos, st->sites, out->reward, out->success, stream)) return rc;
  kitchen_finish_kernel<<<(n + 255) / 256, 256, 0, hs>>>(k);
  return launched("kitchen_step");
}

int earl_kitchen_rollout_clocked(const void* model, const earl_collision_model* col, const earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                 const earl_kitchen_state* st, const float* action, int32_t T, const uint64_t* clock, const earl_kitchen_out* out, earl_stream_t stream) {
  if (!model || !params || !cfg || !st || !action || !out || T < 0 || !kitchen_args_ok(cfg, st, true)) return EARL_ERR_ARG;
  if (!out->obs || !out->reward || !out->done || !out->success) return EARL_ERR_ARG;
  if (cfg->n == 0 || T == 0) return EARL_OK;
  if (int rc = check_cone(col, false, (hipStream_t)stream, "kitchen_rollout")) return rc;
  KitchenRolloutArgs k{model, col, *params, *cfg, *st, *out, action, T, kitchen_solo(cfg->n), clock};
  if (k.solo == 3) kitchen_rollout_kernel<1><<<cfg->n, block_for<23>(), 0, (hipStream_t)stream>>>(k);
  else if (k.solo == 4) kitchen_rollout_kernel<2><<<(cfg->n + 1) / 2, block_for<23>(), 0, (hipStream_t)stream>>>(k);
  else kitchen_rollout_kernel<0><<<solo_grid(cfg->n, k.solo, Lim<23>::WPB), block_for<23>(), 0, (hipStream_t)stream>>>(k);
  return launched("kitchen_rollout");
}
// include/earl_physics.h: T closed-loop env steps in one launch, the policy evaluated by the 32 lanes that own the env -- one policy or a population's member per env,
// every [T] output optional, per-env episode summaries.  The launch forms are earl_kitchen_rollout_clocked's, chosen here by the same rule; the kernels are
// instantiated in physics_kitchen_policy.hip
// (the body of the closed-loop entry points: a population, summaries, an agent pair with its backward goals and the forward table, each there or not)
static int kitchen_closed_loop(const void* model, const earl_collision_model* col, const earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                               const earl_kitchen_state* st, const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_agent_pair* pair, bool paired,
                               const earl_backward_goals* goals, const double* forward_goals, int32_t n_forward_goals, const earl_gaussian_head* head,
                               const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_kitchen_out* out,
                               const earl_episode_summary* summary, earl_stream_t stream) {
  if (!model || !params || !cfg || !st || !policy || !obs0 || !out || T < 0 || !kitchen_args_ok(cfg, st, true)) return EARL_ERR_ARG;
  // the policy's contract (policy_check.h).  The reference clips the action silently, so an unbounded output is taken (unlike the minitaur's).  A population: groups
  // of 16 envs, every member's rows read in 16-byte pieces
  // (the kitchen has no lifelong switch of its own: goal_change_frequency 0; its forward goals come with the call)
  if (paired && (!pair || n_forward_goals < 0)) return EARL_ERR_ARG;
  const bool forward = paired && forward_goals && n_forward_goals >= 1;
  if (earl::contract::check_closed_loop(*policy, 46, 9, earl::contract::kParamsAligned16 | earl::contract::kBf16Params, head, pop, cfg->env_offset, cfg->n, paired ? pair : nullptr, 0, goals,
                                        forward ? n_forward_goals : 0, nullptr))
    return EARL_ERR_ARG;
  if (cfg->n == 0 || T == 0) return EARL_OK;
  if (int rc = check_cone(col, false, (hipStream_t)stream, "kitchen_policy_rollout")) return rc;
  KitchenPolicyArgs k;
  static_cast<KitchenRolloutArgs&>(k) = KitchenRolloutArgs{model, col, *params, *cfg, *st, *out, nullptr, T, kitchen_solo(cfg->n), clock};
  fill_closed_loop(k, *policy, head, obs0, actions, pop, summary, paired ? pair : nullptr, goals, forward ? forward_goals : nullptr, forward ? n_forward_goals : 0);
  if (policy->precision == EARL_PRECISION_BF16) earl_unit_kitchen_bf16_policy_rollout(&k, stream);      // physics_kitchen_policy_bf16.hip: parameters stored as bf16
  else earl_unit_kitchen_policy_rollout(&k, stream);      // physics_kitchen_policy.hip holds the kernels
  return launched("kitchen_policy_rollout");
}
int earl_kitchen_population_rollout(const void* model, const earl_collision_model* col, const earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                    const earl_kitchen_state* st, const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_gaussian_head* head,
                                    const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_kitchen_out* out,
                                    const earl_episode_summary* summary, earl_stream_t stream) {
  return kitchen_closed_loop(model, col, params, cfg, st, policy, pop, nullptr, false, nullptr, nullptr, 0, head, obs0, T, clock, actions, out, summary, stream);
}
// include/earl_physics.h: the forward / reset agent pair inside the same launch -- a population of pairs, a table of backward goals, the forward table and summaries
int earl_kitchen_agents_rollout(const void* model, const earl_collision_model* col, const earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                const earl_kitchen_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_policy_population* pop,
                                const earl_backward_goals* goals, const double* forward_goals, int32_t n_forward_goals, const earl_gaussian_head* head, const double* obs0,
                                int32_t T, const uint64_t* clock, float* actions, const earl_kitchen_out* out, const earl_episode_summary* summary, earl_stream_t stream) {
  return kitchen_closed_loop(model, col, params, cfg, st, policy, pop, pair, true, goals, forward_goals, n_forward_goals, head, obs0, T, clock, actions, out, summary,
                             stream);
}
// one policy, every [T] row kept: the population entry point without a population and without a summary (the same launch, bit for bit)
int earl_kitchen_policy_rollout(const void* model, const earl_collision_model* col, const earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                                const earl_kitchen_state* st, const earl_mlp_policy* policy, const earl_gaussian_head* head, const double* obs0, int32_t T,
                                const uint64_t* clock, float* actions, const earl_kitchen_out* out, earl_stream_t stream) {
  if (!actions || !out || !out->obs || !out->reward || !out->done || !out->success) return EARL_ERR_ARG;
  return earl_kitchen_population_rollout(model, col, params, cfg, st, policy, nullptr, head, obs0, T, clock, actions, out, nullptr, stream);
}
int earl_kitchen_rollout(const void* model, const earl_collision_model* col, const earl_kitchen_params* params, const earl_kitchen_cfg* cfg,
                         const earl_kitchen_state* st, const float* action, int32_t T, const earl_kitchen_out* out, earl_stream_t stream) {
  return earl_kitchen_rollout_clocked(model, col, params, cfg, st, action, T, nullptr, out, stream);
}

int earl_debug_set_solo(int mode) {          // -1 = by batch size, 0 = two envs per wave, 1 = one env per wave, 2 = one env per workgroup (one wave), 3 = one env per workgroup, four waves, 4 = two envs per workgroup, two waves each (kitchen launches)
  const int prev = g_solo;
  if (mode >= -1 && mode <= 4) g_solo = mode;
  return prev;
}
#ifdef EARL_PHYS_PROF
int earl_debug_set_prof_wave_kitchen(int block, int thread) { return prof_set_wave(block, thread); }     // (tools/prof_kitchen_phases.py)
int earl_debug_read_wave_cycles_kitchen(unsigned long long* out) { return prof_read_wave_cycles(out); }
int earl_debug_read_phys_profile_kitchen(unsigned long long* out, int reset) { return prof_read_phases(out, reset); }
#endif

}  // extern "C"

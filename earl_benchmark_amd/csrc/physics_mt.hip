// physics_mt.hip -- third build of the articulated-body stepper: the MINITAUR (BASELINE configs[4]).
//
// The stepper (physics_stepper.h) instantiated for nv = 22 (Lim<22>: a floating root body + 16 hinges in ONE tree, 32 lanes per env, dense lane-cooperative in-LDS
// factorisations, connect constraints for the four knee closures, the motor model's torques handed in per timestep, no mocap weld, no joint damping)
// plus the env kernel (minitaur_kernel: reset incl. its settle steps, fused T-step rollout) and the entry points earl_minitaur_rollout /
// earl_minitaur_reset.  A translation unit of its own so that the three builds compile side by side.
#include "minitaur_device.h"
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"
#include "minitaur_branch_ws.h"
#include "tabletop_hostside.h"   // fail: the thread-local message behind earl_last_error

namespace {
#include "minitaur_stepper.h"
#include "physics_env_minitaur.h"
}  // namespace

#include "physics_launch.h"
// the branch launch (physics_mt_branch.hip): earl_minitaur_branch_rollout hands it the MinitaurBranchArgs it filled -- first to the replicate kernel (src_state: the env's
// own earl_minitaur_state, whose [n] rows become the workspace's [K n]), then to the rollout kernel of the form chosen
extern "C" __attribute__((visibility("hidden"))) int earl_unit_mt_branch_replicate(const void* minitaur_branch_args, const void* src_state, void* stream);
extern "C" __attribute__((visibility("hidden"))) int earl_unit_mt_branch_rollout(const void* minitaur_branch_args, int duo, void* stream);

namespace {

int g_mt_stepper = 1;     // earl_debug_set_minitaur_stepper: 1 = the tree-structured timestep (minitaur_stepper.h), 0 = the generic substep<22>
int g_mt_duo = EARL_MT_DUO_DEFAULT;   // earl_debug_set_minitaur_duo: 1 = the two-waves-per-SIMD rollout (minitaur_duo_kernel), 0 = the one-wave kernel, -1 = by batch size

// minitaur rollout, packed launches: the one-wave kernel holds 8 envs per CU, the two-wave kernel 16 at 1.6 x the time per round (measured: 4096 x 1000 in 174 ms = two rounds of
// 87 against one round of 139): whichever needs less time for the batch's rounds
bool mt_use_duo(int n) {
  const int cus = cu_count();
  const long rounds_one = (n + 8L * cus - 1) / (8L * cus), rounds_two = (n + 16L * cus - 1) / (16L * cus);
  return 16 * rounds_two < 10 * rounds_one;
}

// the launch form of a rollout, for the plain and the closed-loop entry point alike.  Duo: two waves per SIMD by role (minitaur_duo_kernel, 16 envs per workgroup of eight waves)
enum class MtForm { Generic, Duo, Tree };      // for batches that fill the chip's wave slots in the packed form anyway; Generic: substep<22>, the comparison build (no policy form)
MtForm minitaur_form(int n, int solo, int num_substeps) {
  if (!g_mt_stepper) return MtForm::Generic;
  return solo == 0 && num_substeps > 0 && (g_mt_duo > 0 || (g_mt_duo < 0 && mt_use_duo(n))) ? MtForm::Duo : MtForm::Tree;      // (num_substeps = 0: nothing to split)
}
// the rules of an env's cfg / st that every entry point has
bool minitaur_args_ok(const earl_minitaur_cfg* cfg, const earl_minitaur_state* st) {
  if (cfg->n < 0 || !cfg->goal_table || cfg->n_goals < 1) return false;
  if (!st->qpos || !st->qvel || !st->goal || !st->motor_param || !st->observed_torque || !st->overheat || !st->motor_enabled) return false;
  return cfg->goal_change_frequency <= 0 || st->steps_since_goal_change;   // (NULL is allowed without goal switching only: the reset clears the counter the rollout reads)
}

}  // namespace

extern "C" {

int earl_minitaur_rollout_clocked(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                  const float* action, int32_t T, const uint64_t* clock, const earl_minitaur_out* out, earl_stream_t stream) {
  if (!model24 || !cfg || !st || !out || !action || T < 0 || !minitaur_args_ok(cfg, st)) return EARL_ERR_ARG;
  if (!out->obs || !out->reward || !out->done || !out->success || cfg->num_substeps < 0) return EARL_ERR_ARG;
  if (cfg->n == 0 || T == 0) return EARL_OK;
  if (int rc = check_cone(col, false, (hipStream_t)stream, "minitaur_rollout")) return rc;
  MinitaurArgs a{model24, col, *cfg, *st, *out, action, T, nullptr, nullptr, solo_mode(cfg->n), clock};
  const MtForm form = minitaur_form(cfg->n, a.solo, cfg->num_substeps);
  if (form == MtForm::Duo) {
    minitaur_duo_kernel<<<(unsigned)((cfg->n + 16 * MT_DUO_PAIRS / 4 - 1) / (4 * MT_DUO_PAIRS)), 128 * MT_DUO_PAIRS, 0, (hipStream_t)stream>>>(a);
    return launched("minitaur_rollout (two waves per SIMD)");
  }
  if (form == MtForm::Tree) minitaur_kernel<false, true><<<solo_grid(cfg->n, a.solo, EARL_MT_WPB), 64 * EARL_MT_WPB, 0, (hipStream_t)stream>>>(a);
  else minitaur_kernel<false, false><<<solo_grid(cfg->n, a.solo, Lim<22>::WPB), block_for<22>(), 0, (hipStream_t)stream>>>(a);
  return launched("minitaur_rollout");
}
// include/earl_physics.h: T closed-loop env steps in one launch, the policy evaluated by the 32 lanes that own the env -- one policy or a population's member per env,
// every [T] output optional, per-env episode summaries.  The launch forms are earl_minitaur_rollout_clocked's, by the same rule (minitaur_form)
// (the body of the closed-loop entry points: a population, summaries, an agent pair and its table of backward goals, each there or not)
static int minitaur_closed_loop(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_agent_pair* pair, bool paired, const earl_backward_goals* goals,
                                const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_minitaur_out* out,
                                const earl_episode_summary* summary, earl_stream_t stream) {
  if (!model24 || !cfg || !st || !out || !policy || !obs0 || T < 0 || !minitaur_args_ok(cfg, st) || cfg->num_substeps < 0) return EARL_ERR_ARG;
  if (!out->obs && !st->last_obs) return EARL_ERR_ARG;    // (without out->obs the env's row of last_obs is the one observation row the launch keeps)
  // the policy's contract (policy_check.h).  The reference env raises on an action outside +-(1 + 0.01); a kernel cannot, and the open-loop replay of the returned
  // actions must not either: bounded policies only.  A population: groups of 16 envs, every member's rows read in 16-byte pieces
  // (the pair's handover IS the goal switch of autonomous RL: goal_change_frequency > 0 is refused with a pair -- both would draw with index 0xFFFE at the same step)
  if (paired && !pair) return EARL_ERR_ARG;
  if (earl::contract::check_closed_loop(*policy, 32, 8, earl::contract::kParamsAligned16 | earl::contract::kBoundedOutput | earl::contract::kBf16Params, head, pop, cfg->env_offset, cfg->n,
                                        paired ? pair : nullptr, cfg->goal_change_frequency, goals, cfg->n_goals, nullptr))
    return EARL_ERR_ARG;
  if (!g_mt_stepper) return EARL_ERR_ARG;                 // (earl_debug_set_minitaur_stepper(0): no policy form)
  if (cfg->n == 0 || T == 0) return EARL_OK;
  if (int rc = check_cone(col, false, (hipStream_t)stream, "minitaur_policy_rollout")) return rc;
  MinitaurPolicyArgs a;
  static_cast<MinitaurArgs&>(a) = MinitaurArgs{model24, col, *cfg, *st, *out, nullptr, T, nullptr, nullptr, solo_mode(cfg->n), clock};
  fill_closed_loop(a, *policy, head, obs0, actions, pop, summary, paired ? pair : nullptr, goals, nullptr, 0);      // (the forward goals are cfg->goal_table's)
  const bool duo = minitaur_form(cfg->n, a.solo, cfg->num_substeps) == MtForm::Duo;
  if (policy->precision == EARL_PRECISION_BF16) return earl_unit_mt_bf16_policy_rollout(&a, duo ? 1 : 0, stream);      // physics_mt_bf16.hip: the same two kernels, parameters stored as bf16
  if (duo) {
    minitaur_policy_duo_kernel<<<(unsigned)((cfg->n + 16 * MT_DUO_PAIRS / 4 - 1) / (4 * MT_DUO_PAIRS)), 128 * MT_DUO_PAIRS, 0, (hipStream_t)stream>>>(a);
    return launched("minitaur_policy_rollout (two waves per SIMD)");
  }
  minitaur_policy_kernel<false, true><<<solo_grid(cfg->n, a.solo, EARL_MT_WPB), 64 * EARL_MT_WPB, 0, (hipStream_t)stream>>>(a);
  return launched("minitaur_policy_rollout");
}
int earl_minitaur_population_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                     const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_gaussian_head* head, const double* obs0, int32_t T,
                                     const uint64_t* clock, float* actions, const earl_minitaur_out* out, const earl_episode_summary* summary, earl_stream_t stream) {
  return minitaur_closed_loop(model24, col, cfg, st, policy, pop, nullptr, false, nullptr, head, obs0, T, clock, actions, out, summary, stream);
}
// include/earl_physics.h: the forward / reset agent pair inside the same launch -- a population of pairs, a table of backward goals and summaries, each NULL or given
int earl_minitaur_agents_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                 const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_policy_population* pop, const earl_backward_goals* goals,
                                 const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_minitaur_out* out,
                                 const earl_episode_summary* summary, earl_stream_t stream) {
  return minitaur_closed_loop(model24, col, cfg, st, policy, pop, pair, true, goals, head, obs0, T, clock, actions, out, summary, stream);
}
// one policy, every [T] row kept: the population entry point without a population and without a summary (the same launch, bit for bit)
int earl_minitaur_policy_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                 const earl_mlp_policy* policy, const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions,
                                 const earl_minitaur_out* out, earl_stream_t stream) {
  if (!actions || !out || !out->obs || !out->reward || !out->done || !out->success) return EARL_ERR_ARG;
  return earl_minitaur_population_rollout(model24, col, cfg, st, policy, nullptr, head, obs0, T, clock, actions, out, nullptr, stream);
}
// include/earl_physics.h: K action plans per env scored from the current state in ONE launch over K n virtual envs (kernels: physics_mt_branch.hip).  The workspace
// block is minitaur_branch_ws.h's
int earl_minitaur_branch_ws_bytes(int32_t K, int32_t n, int64_t* bytes) {
  if (!bytes || K < 0 || n < 0 || (int64_t)K * n > INT32_MAX) return EARL_ERR_ARG;
  *bytes = earl::minitaur_branch_layout((int64_t)K * n).bytes;
  return EARL_OK;
}
int earl_minitaur_branch_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                                 int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_minitaur_branch_ws* ws,
                                 const earl_episode_summary* summary, double* last_obs, int32_t* fail_count, earl_stream_t stream) {
  using earl::hostside::fail;
  if (!model24 || !cfg || !st) return fail(EARL_ERR_ARG, "minitaur_branch_rollout: model / cfg / st is NULL");
  if (!minitaur_args_ok(cfg, st) || cfg->num_substeps < 0)
    return fail(EARL_ERR_ARG, "minitaur_branch_rollout: cfg / st as earl_minitaur_rollout_clocked refuses them (n = %d, a NULL state row, goal switching without its counter, no goal table)", cfg->n);
  if (!act || !ws) return fail(EARL_ERR_ARG, "minitaur_branch_rollout: act / ws is NULL");
  if (K < 0 || H < 0) return fail(EARL_ERR_ARG, "minitaur_branch_rollout: K = %d, H = %d: both >= 0", K, H);
  const int n = cfg->n;
  if (act_branch_stride < 0 || (act_branch_stride != 0 && act_branch_stride < (int64_t)H * n * 8))
    return fail(EARL_ERR_ARG, "minitaur_branch_rollout: action stride %lld is neither 0 nor >= H * n * 8 = %lld", (long long)act_branch_stride, (long long)H * n * 8);
  if (!(summary && (summary->ret || summary->success_last || summary->first_success)) && !last_obs && !fail_count)
    return fail(EARL_ERR_ARG, "minitaur_branch_rollout: all five outputs are NULL");      // (nothing to compute)
  const int64_t V = (int64_t)K * n;
  if (V > INT32_MAX) return fail(EARL_ERR_ARG, "minitaur_branch_rollout: K n = %lld virtual envs: at most 2^31 - 1", (long long)V);
  const earl::MinitaurBranchLayout L = earl::minitaur_branch_layout(V);
  if (V > 0 && (!ws->base || (reinterpret_cast<uintptr_t>(ws->base) & 7) != 0 || ws->bytes < L.bytes))
    return fail(EARL_ERR_ARG, "minitaur_branch_rollout: ws: base %p (8-byte aligned), %lld bytes of the %lld needed", ws->base, (long long)ws->bytes, (long long)L.bytes);
  if (!g_mt_stepper) return fail(EARL_ERR_ARG, "minitaur_branch_rollout: earl_debug_set_minitaur_stepper(0) has no branch form");      // (as it has no policy form)
  if (V == 0 || H == 0) return EARL_OK;
  if (int rc = check_cone(col, false, (hipStream_t)stream, "minitaur_branch_rollout")) return rc;
  char* const base = static_cast<char*>(ws->base);
  earl_minitaur_state vs{};                               // the virtual envs' state: the workspace's rows (steps_since_reset: NULL, a branch keeps none)
  vs.qpos = reinterpret_cast<double*>(base + L.qpos);
  vs.qvel = reinterpret_cast<double*>(base + L.qvel);
  vs.goal = reinterpret_cast<double*>(base + L.goal);
  vs.motor_param = reinterpret_cast<double*>(base + L.motor_param);
  vs.observed_torque = reinterpret_cast<double*>(base + L.observed_torque);
  vs.overheat = reinterpret_cast<int32_t*>(base + L.overheat);
  vs.motor_enabled = reinterpret_cast<uint8_t*>(base + L.motor_enabled);
  vs.steps_since_goal_change = cfg->goal_change_frequency > 0 ? reinterpret_cast<int32_t*>(base + L.sgc) : nullptr;
  vs.fail_count = fail_count;                                   // (the replicate kernel clears it, a rolled-back step counts into it)
  vs.last_obs = last_obs ? last_obs : reinterpret_cast<double*>(base + L.last_obs);      // the one carried row: step by step it IS the observation of the newest stable step
  MinitaurBranchArgs a{};
  static_cast<MinitaurArgs&>(a) = MinitaurArgs{model24, col, *cfg, vs, earl_minitaur_out{nullptr, nullptr, nullptr, nullptr, nullptr}, act, H, nullptr, nullptr, solo_mode((int)V), clock};
  a.cfg.n = (int)V;
  a.n_env = n;
  a.act_stride = act_branch_stride;
  a.br_ret = summary ? summary->ret : nullptr;
  a.br_last = summary ? summary->success_last : nullptr;
  a.br_first = summary ? summary->first_success : nullptr;
  if (int rc = earl_unit_mt_branch_replicate(&a, st, stream)) return rc;
  return earl_unit_mt_branch_rollout(&a, minitaur_form((int)V, a.solo, cfg->num_substeps) == MtForm::Duo ? 1 : 0, stream);
}
int earl_minitaur_rollout(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                          const float* action, int32_t T, const earl_minitaur_out* out, earl_stream_t stream) {
  return earl_minitaur_rollout_clocked(model24, col, cfg, st, action, T, nullptr, out, stream);
}
int earl_minitaur_reset(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                        const uint8_t* mask, double* obs, earl_stream_t stream) {
  if (!model24 || !cfg || !st || !minitaur_args_ok(cfg, st) || !cfg->reset_qpos || cfg->settle_steps < 0) return EARL_ERR_ARG;
  if (cfg->n == 0) return EARL_OK;
  if (int rc = check_cone(col, false, (hipStream_t)stream, "minitaur_reset")) return rc;
  MinitaurArgs a{model24, col, *cfg, *st, earl_minitaur_out{nullptr, nullptr, nullptr, nullptr, nullptr}, nullptr, 0, mask, obs, solo_mode(cfg->n), nullptr};
  if (g_mt_stepper) minitaur_kernel<true, true><<<solo_grid(cfg->n, a.solo, EARL_MT_WPB), 64 * EARL_MT_WPB, 0, (hipStream_t)stream>>>(a);
  else minitaur_kernel<true, false><<<solo_grid(cfg->n, a.solo, Lim<22>::WPB), block_for<22>(), 0, (hipStream_t)stream>>>(a);
  return launched("minitaur_reset");
}
int earl_minitaur_cfg_size(void) { return (int)sizeof(earl_minitaur_cfg); }
int earl_debug_set_solo_mt(int mode) {       // this unit's copy of the small-batch switch (earl_debug_set_solo): the minitaur launches
  const int prev = g_solo;
  if (mode >= -1 && mode <= 2) g_solo = mode;
  return prev;
}
int earl_debug_set_minitaur_stepper(int tree) {          // 1 (default): minitaur_stepper.h, 0: the generic substep<22> (comparison / measurement)
  if (tree != 0 && tree != 1) return EARL_ERR_ARG;
  g_mt_stepper = tree;
  return EARL_OK;
}
int earl_debug_set_minitaur_duo(int mode) {              // 1: the two-waves-per-SIMD rollout kernel for every packed launch, 0: never, -1: by batch size (default).  Returns the previous setting
  const int prev = g_mt_duo;
  if (mode >= -1 && mode <= 1) g_mt_duo = mode;
  return prev;
}
#ifdef EARL_MT_DEBUG
int earl_debug_read_mt_dbg(int* out_i, double* out_d) {
  if (hipMemcpyFromSymbol(out_i, HIP_SYMBOL(g_mt_dbg), sizeof(int) * 4096 * 8 * 32) != hipSuccess) return EARL_ERR_LAUNCH;
  if (hipMemcpyFromSymbol(out_d, HIP_SYMBOL(g_mt_dbg_al), sizeof(double) * 4096 * 8 * 32) != hipSuccess) return EARL_ERR_LAUNCH;
  if (hipMemcpyFromSymbol(out_d + 4096 * 8 * 32, HIP_SYMBOL(g_mt_dbg_x), sizeof(double) * 5 * 4096 * 8 * 32) != hipSuccess) return EARL_ERR_LAUNCH;
  return hipMemcpyFromSymbol(out_d + 6 * 4096 * 8 * 32, HIP_SYMBOL(g_mt_dbg_ph), sizeof(double) * 8 * 4096 * 8 * 32) == hipSuccess ? EARL_OK : EARL_ERR_LAUNCH;
}
#endif
#ifdef EARL_PHYS_PROF
int earl_debug_set_prof_wave_mt(int block, int thread) { return prof_set_wave(block, thread); }     // (minitaur_duo_kernel: thread 0 = a first-half wave, thread 256 = its partner)
int earl_debug_read_wave_cycles_mt(unsigned long long* out) { return prof_read_wave_cycles(out); }
int earl_debug_read_phys_profile_mt(unsigned long long* out, int reset) { return prof_read_phases(out, reset); }     // (tools/prof_minitaur.py)
#endif

}  // extern "C"

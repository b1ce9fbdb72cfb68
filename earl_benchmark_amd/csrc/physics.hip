// physics.hip -- the main unit of the articulated-body stepper (physics_stepper.h): the Sawyer door (nv = 10) and peg (nv = 15) at 16 lanes per env, the
// stepper's own entry points earl_physics_step / _forward (nv = 23 forwarded to physics_kitchen.hip, 64 lanes per env to physics_l64.hip), the Sawyer env's
// entry points (the door's eight-wave rollout forwarded to physics_w8.hip), the collision-table cone cache of all units, and the size queries and debug switches.
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"
#include "sawyer_prior.h"

#include <mutex>
#include <unordered_map>

namespace {
#include "physics_env_sawyer.h"

// compute_reward / is_successful on given observations (sawyer_door.py:141-177), one lane per row
__global__ void sawyer_door_reward_kernel(const int n, const double* __restrict__ obs, const earl_sawyer_cfg cfg, float* __restrict__ reward,
                                          uint8_t* __restrict__ success) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* o = obs + (size_t)i * 14;
  double r; bool ok;
  door_reward(cfg, ld3(o), ld3(o + 4), ld3(o + 11), r, ok);
  if (reward) reward[i] = (float)r;
  if (success) success[i] = ok ? 1 : 0;
}

// SawyerDoorV2.evaluate_state's info dict (sawyer_door.py:127-139) of given observation rows: every entry is a function of the observation (and of the
// reward type), so the rollout kernel need not carry it; one lane per row
__global__ void sawyer_door_info_kernel(const int n, const double* __restrict__ obs, const earl_sawyer_cfg cfg, const uint8_t* __restrict__ status, double* __restrict__ info) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* o = obs + (size_t)i * 14;
  double r, row[EARL_SAWYER_INFO]; bool ok;
  double* mine = info + (size_t)i * EARL_SAWYER_INFO;
  // a goal-switch row of a lifelong rollout (cfg.goal_change_frequency > 0: only then has the rollout kernel written the marker, for every row): the target its reward used
  // (the row's goal block holds the NEW goal).  Without goal switching the slot is output only.
  const V3 target = (cfg.goal_change_frequency > 0 && mine[7] == 1.0) ? ld3(mine) : ld3(o + 11);
  door_reward(cfg, ld3(o), ld3(o + 4), target, r, ok, row);
  const bool rolled_back = status && status[i] != 0;
#pragma unroll
  for (int k = 0; k < EARL_SAWYER_INFO; ++k) info[(size_t)i * EARL_SAWYER_INFO + k] = rolled_back ? 0.0 : row[k];
}
}  // namespace

#include "physics_launch.h"

namespace {

#ifndef EARL_PEG_SLICE
#define EARL_PEG_SLICE 10   // env steps per work item (tools/bench_peg_schedule.py: 5 and 10: 43.1 ms, 20: 44.3, 40: 47.0, 100: 50.9, one group per wave: 54.8) of the peg's time-sliced schedule (a slice is ~1 ms; claiming one costs a scan of the queue: microseconds)
#endif
int g_peg_sliced = 1;     // earl_debug_set_peg_schedule
int g_door_variant = 0;   // earl_debug_set_door_variant: 0 = by batch size, 1 = four single-wave workgroups per CU, 2 = one eight-wave workgroup per CU
int g_lpe = 16;   // lanes per env (earl_debug_set_physics_lanes): 16 = four envs per wavefront, 64 = one wavefront per env
int g_prior_fused = 1;   // earl_debug_set_sawyer_prior_launches: 1 = the prior branches of earl_sawyer_branch_rollout_prior inside ONE launch over all K n virtual envs (default), 0 = a launch of their own behind the plain one

template <int NV, bool INTEGRATE>
void launch_physics(const PArgs& a, hipStream_t st) {
  if constexpr (NV > 16) earl_unit_kitchen_physics(&a, INTEGRATE ? 1 : 0, st);      // (physics_kitchen.hip: 32 lanes per env)
  else if (g_lpe == 64) earl_unit_l64_physics(&a, NV, INTEGRATE ? 1 : 0, st);
  else physics_kernel<NV, 16, INTEGRATE><<<grid_for<NV, 16>(a.n), block_for<NV>(), 0, st>>>(a);
}

enum SawyerUse { kObserve, kReset, kStep };      // the rules of an env's cfg / st by what the entry point does: read the state | write what a rollout will read | step (nv, out given)
bool sawyer_args_ok(SawyerUse use, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st, int32_t nv = 0, const earl_sawyer_out* out = nullptr) {
  if (cfg->n < 0 || !st->qpos || !st->qvel || !st->mocap_pos || !st->goal) return false;
  if (use == kObserve) return true;
  if (cfg->goal_change_frequency > 0 && !st->steps_since_goal_change) return false;   // (NULL is allowed without goal switching only: the reset clears the counter the rollout reads)
  if (cfg->n_goal_rows > 0 && !cfg->goal_table) return false;
  const bool dense_peg = cfg->obj_kind >= 1 && cfg->reward_type != 0;      // its reward reads what the reset keeps in obj_init, and the pad / grasp attachments
  if (dense_peg && !st->obj_init) return false;
  if (use == kReset) return true;
  if (cfg->frame_skip < 0 || cfg->att_hand < 0 || cfg->att_right < 0 || cfg->att_left < 0 || cfg->att_obj < 0) return false;
  if (dense_peg && (cfg->att_grasp < 0 || cfg->att_lpad < 0 || cfg->att_rpad < 0)) return false;
  return !(nv == 15 && cfg->obj_kind >= 1 && out->info && !st->obj_init);     // (so does the peg's info dict: without it the rows were left unwritten)
}
// the launch form of a rollout of nv = 10 / 15, for the plain and the closed-loop entry point alike
enum class SawyerForm { L64, DoorSliced, DoorW8, Door, PegSliced, Peg };
int peg_slice() { return g_peg_sliced >= 2 ? g_peg_sliced : EARL_PEG_SLICE; }
SawyerForm sawyer_form(int32_t nv, int n, int32_t T, const earl_sawyer_state* st, bool policy) {
  if (g_lpe == 64) return SawyerForm::L64;                // (measurement builds: no policy form, the closed-loop entry point refuses them)
  if (nv == 10) {
    // variant 3 (measurement: the one-wave build under the peg's work queue, tools/bench_variant.py) has no policy kernel, so the closed loop reads it as 0, by batch
    // size -- on purpose unlike the plain entry point, where 3 stays on the one-wave build at every batch size, also where the queue cannot run (no sched, T = 1)
    const int v = policy && g_door_variant == 3 ? 0 : g_door_variant;
    if (v == 3 && st->sched && T > 1) return SawyerForm::DoorSliced;
    return v == 2 || (v == 0 && n > 4096) ? SawyerForm::DoorW8 : SawyerForm::Door;      // eight waves per CU: wins from two rounds of 4096 envs on
  }
  // more workgroups than the GPU holds at once (one four-wave workgroup = 16 envs per CU): time-sliced schedule, one persistent workgroup per CU
  return st->sched && g_peg_sliced && grid_for<15, 16>(n) > cu_count() && T > 1 ? SawyerForm::PegSliced : SawyerForm::Peg;
}

std::mutex g_cone_mu;
std::unordered_map<const void*, int> g_cone_seen;
}  // namespace
extern "C" __attribute__((visibility("hidden"))) int earl_unit_table_cone(const void* col, void* stream) {
  std::lock_guard<std::mutex> lock(g_cone_mu);
  const auto it = g_cone_seen.find(col);
  if (it != g_cone_seen.end()) return it->second;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) { (void)hipGetLastError(); return -1; }
  if (cs != hipStreamCaptureStatusNone) return -1;
  int cone = -1;
  if (hipMemcpy(&cone, &static_cast<const earl_collision_model*>(col)->cone, sizeof cone, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -1; }
  g_cone_seen[col] = cone;
  return cone;
}

extern "C" {

// include/earl_physics.h: the owner of a device collision table announces that the block is freed / rewritten (NULL: every table)
int earl_physics_forget_table(const void* col) {
  std::lock_guard<std::mutex> lock(g_cone_mu);
  if (!col) { const int k = (int)g_cone_seen.size(); g_cone_seen.clear(); return k; }
  return (int)g_cone_seen.erase(col);
}
int earl_physics_step(const void* model, const earl_collision_model* col, int32_t nv, int32_t n, int32_t nsub, double* qpos, double* qvel,
                      const double* mocap_pos, const double* mocap_quat, const double* ctrl, double* att_xpos,
                      earl_stream_t stream) {
  if (!model || n < 0 || nsub < 0 || !qpos || !qvel || !mocap_pos || !mocap_quat || !ctrl) return EARL_ERR_ARG;
  if (n == 0 || nsub == 0) return EARL_OK;
  if (nv != 10 && nv != 15 && nv != 23) return EARL_ERR_ARG;
  if (int rc = check_cone(col, nv <= 16, (hipStream_t)stream, "physics_step")) return rc;
  PArgs a{model, col, n, nsub, qpos, qvel, mocap_pos, mocap_quat, ctrl, att_xpos, nullptr, nullptr, 0, 4};
  if (nv == 10) launch_physics<10, true>(a, (hipStream_t)stream);
  else if (nv == 15) launch_physics<15, true>(a, (hipStream_t)stream);
  else if (nv == 23) launch_physics<23, true>(a, (hipStream_t)stream);
  else return EARL_ERR_ARG;
  return launched("physics_step");
}

int earl_physics_forward(const void* model, const earl_collision_model* col, int32_t nv, int32_t n, const double* qpos, const double* qvel,
                         const double* mocap_pos, const double* mocap_quat, const double* ctrl, double* qacc,
                         double* efc_force, double* att_xpos, earl_stream_t stream) {
  if (!model || n < 0 || !qpos || !qvel || !mocap_pos || !mocap_quat || !ctrl || !qacc) return EARL_ERR_ARG;
  if (n == 0) return EARL_OK;
  if (nv != 10 && nv != 15 && nv != 23) return EARL_ERR_ARG;
  if (int rc = check_cone(col, nv <= 16, (hipStream_t)stream, "physics_forward")) return rc;
  PArgs a{model, col, n, 1, const_cast<double*>(qpos), const_cast<double*>(qvel), mocap_pos, mocap_quat, ctrl, att_xpos, qacc, efc_force, 0, 4};
  if (nv == 10) launch_physics<10, false>(a, (hipStream_t)stream);
  else if (nv == 15) launch_physics<15, false>(a, (hipStream_t)stream);
  else if (nv == 23) launch_physics<23, false>(a, (hipStream_t)stream);
  else return EARL_ERR_ARG;
  return launched("physics_forward");
}

int earl_sawyer_rollout_clocked(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                const float* action, int32_t T, const uint64_t* clock, const earl_sawyer_out* out, earl_stream_t stream) {
  if (!model || !cfg || !st || !out || !action || T < 0 || !out->obs || !sawyer_args_ok(kStep, cfg, st, nv, out)) return EARL_ERR_ARG;
  if (cfg->n == 0 || T == 0) return EARL_OK;
  if (nv != 10 && nv != 15) return EARL_ERR_ARG;
  if (int rc = check_cone(col, true, (hipStream_t)stream, "sawyer_rollout")) return rc;
  SawyerArgs a{model, col, *cfg, *st, action, T, *out, nullptr, nullptr, nullptr, nullptr, 0, 0, clock};
  switch (sawyer_form(nv, cfg->n, T, st, false)) {
    case SawyerForm::DoorSliced: a.slice = peg_slice(); sawyer_rollout_kernel<10, 16, true><<<4 * cu_count(), block_for<10>(), 0, (hipStream_t)stream>>>(a);
      return launched("sawyer_rollout (door, time-sliced)");
    case SawyerForm::DoorW8: return earl_unit_w8_sawyer_rollout(&a, stream);
    case SawyerForm::L64: earl_unit_l64_sawyer_rollout(&a, nv, stream); break;
    case SawyerForm::Door: sawyer_rollout_kernel<10, 16><<<grid_for<10, 16>(cfg->n), block_for<10>(), 0, (hipStream_t)stream>>>(a); break;
    case SawyerForm::PegSliced: a.slice = peg_slice(); sawyer_rollout_kernel<15, 16, true><<<cu_count(), block_for<15>(), 0, (hipStream_t)stream>>>(a); break;
    case SawyerForm::Peg: sawyer_rollout_kernel<15, 16><<<grid_for<15, 16>(cfg->n), block_for<15>(), 0, (hipStream_t)stream>>>(a); break;
  }
  return launched("sawyer_rollout");
}
int earl_sawyer_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                        const float* action, int32_t T, const earl_sawyer_out* out, earl_stream_t stream) {
  return earl_sawyer_rollout_clocked(model, col, nv, cfg, st, action, T, nullptr, out, stream);
}

// include/earl_physics.h: T closed-loop env steps in one launch of the rollout kernel, the policy evaluated by the wave that owns the env -- one policy or a
// population's member per env, every [T] output optional, per-env episode summaries.  The launch forms are earl_sawyer_rollout's, by the same rule (sawyer_form)
// (the body of the closed-loop entry points: a population, summaries, an agent pair and its table of backward goals, each there or not)
static int sawyer_closed_loop(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                              const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_agent_pair* pair, bool paired, const earl_backward_goals* goals,
                              const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_sawyer_out* out,
                              const earl_episode_summary* summary, earl_stream_t stream) {
  if (!model || !cfg || !st || !out || !policy || !obs0 || T < 1 || (nv != 10 && nv != 15) || !sawyer_args_ok(kStep, cfg, st, nv, out)) return EARL_ERR_ARG;      // (T = 0 is an error here)
  if (!out->obs && !st->last_obs) return EARL_ERR_ARG;    // (without out->obs the env's row of last_obs is the one observation row the launch keeps)
  // the policy's contract (policy_check.h); the weight rows are read in 16-byte pieces, so params is aligned and every stride a multiple of 4 floats (8 bf16 values)
  if (paired && !pair) return EARL_ERR_ARG;
  if (earl::contract::check_closed_loop(*policy, 14, 4, earl::contract::kParamsAligned16 | earl::contract::kBf16Params, head, pop, cfg->env_offset, cfg->n, paired ? pair : nullptr,
                                        cfg->goal_change_frequency, goals, cfg->n_goal_rows, nullptr))
    return EARL_ERR_ARG;
  if (g_lpe == 64) return EARL_ERR_ARG;                   // (the 64-lane measurement builds: no policy form)
  if (cfg->n == 0) return EARL_OK;
  if (int rc = check_cone(col, true, (hipStream_t)stream, "sawyer_policy_rollout")) return rc;
  SawyerPolicyArgs a;
  static_cast<SawyerArgs&>(a) = SawyerArgs{model, col, *cfg, *st, nullptr, T, *out, nullptr, nullptr, nullptr, nullptr, 0, 0, clock};
  fill_closed_loop(a, *policy, head, obs0, actions, pop, summary, paired ? pair : nullptr, goals, nullptr, 0);      // (the forward goals are cfg->goal_table's)
  const SawyerForm form = sawyer_form(nv, cfg->n, T, st, true);
  if (policy->precision == EARL_PRECISION_BF16) {         // the same forms with the parameters stored as bf16: the kernels of physics_bf16.hip / physics_w8_bf16.hip
    if (form == SawyerForm::DoorW8) return earl_unit_w8_bf16_sawyer_policy_rollout(&a, stream);
    if (form != SawyerForm::Door && form != SawyerForm::PegSliced && form != SawyerForm::Peg) return EARL_ERR_ARG;
    if (form == SawyerForm::PegSliced) a.slice = peg_slice();
    return earl_unit_bf16_sawyer_policy_rollout(&a, nv, form == SawyerForm::PegSliced ? 1 : 0, stream);
  }
  switch (form) {
    case SawyerForm::DoorW8: return earl_unit_w8_sawyer_policy_rollout(&a, stream);
    case SawyerForm::Door: sawyer_policy_rollout_kernel<10, 16><<<grid_for<10, 16>(cfg->n), block_for<10>(), 0, (hipStream_t)stream>>>(a); break;
    case SawyerForm::PegSliced: a.slice = peg_slice(); sawyer_policy_rollout_kernel<15, 16, true><<<cu_count(), block_for<15>(), 0, (hipStream_t)stream>>>(a); break;
    case SawyerForm::Peg: sawyer_policy_rollout_kernel<15, 16><<<grid_for<15, 16>(cfg->n), block_for<15>(), 0, (hipStream_t)stream>>>(a); break;
    default: return EARL_ERR_ARG;                           // (L64 was refused above; the closed loop never gets DoorSliced)
  }
  return launched("sawyer_policy_rollout");
}
int earl_sawyer_population_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                   const earl_mlp_policy* policy, const earl_policy_population* pop, const earl_gaussian_head* head, const double* obs0, int32_t T,
                                   const uint64_t* clock, float* actions, const earl_sawyer_out* out, const earl_episode_summary* summary, earl_stream_t stream) {
  return sawyer_closed_loop(model, col, nv, cfg, st, policy, pop, nullptr, false, nullptr, head, obs0, T, clock, actions, out, summary, stream);
}
// the forward / reset agent pair in its general form: a population of pairs, a table of backward goals and summaries, each NULL or given
int earl_sawyer_agents_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_policy_population* pop, const earl_backward_goals* goals,
                               const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions, const earl_sawyer_out* out,
                               const earl_episode_summary* summary, earl_stream_t stream) {
  return sawyer_closed_loop(model, col, nv, cfg, st, policy, pop, pair, true, goals, head, obs0, T, clock, actions, out, summary, stream);
}
// the forward / reset agent pair: the same launch with the phase state machine switched on (no population, no table, no summary)
int earl_sawyer_pair_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                             const earl_mlp_policy* policy, const earl_agent_pair* pair, const earl_gaussian_head* head, const double* obs0, int32_t T,
                             const uint64_t* clock, float* actions, const earl_sawyer_out* out, earl_stream_t stream) {
  return earl_sawyer_agents_rollout(model, col, nv, cfg, st, policy, pair, nullptr, nullptr, head, obs0, T, clock, actions, out, nullptr, stream);
}
// one policy, every [T] row kept: the population entry point without a population and without a summary (the same launch, bit for bit)
int earl_sawyer_policy_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_mlp_policy* policy, const earl_gaussian_head* head, const double* obs0, int32_t T, const uint64_t* clock, float* actions,
                               const earl_sawyer_out* out, earl_stream_t stream) {
  if (!actions || !out || !out->obs) return EARL_ERR_ARG;
  return earl_sawyer_population_rollout(model, col, nv, cfg, st, policy, nullptr, head, obs0, T, clock, actions, out, nullptr, stream);
}

// include/earl_physics.h: K action plans per env scored from the current state in ONE launch over K n virtual envs (kernels: physics_branch.hip, physics_branch_w8.hip).
// The workspace block, carved here: [V, nv + 1] qpos (rows of the model's nq), [V, nv] qvel, [V, 3] mocap_pos, [V, 7] goal, [V, 14] carried observation rows (unused when
// the caller's last_obs takes them), then int32 [V] goal-switch counters and [2 ceil(V / 4)] work queue; V = K n
static int64_t sawyer_branch_bytes(int32_t nv, int64_t V) { return V * (int64_t)((nv + 1 + nv + 3 + 7 + 14) * sizeof(double) + sizeof(int32_t)) + 2 * ((V + 3) / 4) * (int64_t)sizeof(int32_t); }
int earl_sawyer_branch_ws_bytes(int32_t nv, int32_t K, int32_t n, int64_t* bytes) {
  if (!bytes || (nv != 10 && nv != 15) || K < 0 || n < 0 || (int64_t)K * n > INT32_MAX) return EARL_ERR_ARG;
  *bytes = sawyer_branch_bytes(nv, (int64_t)K * n);
  return EARL_OK;
}
// the body of earl_sawyer_branch_rollout.  gamma NULL: the plain sum, the kernels of physics_branch.hip / physics_branch_w8.hip.  gamma given
// (earl_sawyer_branch_rollout_value with discount != 1, sawyer_value.hip): the discounted sum, the same kernel text built with EARL_BRANCH_DISCOUNT
// (physics_branch_value.hip / physics_branch_value_w8.hip), `disc` the [K n] words of the caller's block that carry d_t; same checks, same forms, same replicate kernel.
// pr NULL: ONE launch over all K n virtual envs, as ever.  pr given (earl_sawyer_branch_rollout_prior with P = pr->prior->branches >= 1, sawyer_value.hip; `disc` is then
// required, the prior kernels being built with the discounted sum): by default still ONE launch, of sawyer_prior_rollout_kernel (physics_branch_prior.hip /
// physics_branch_prior_w8.hip), in which the branches in front of K - P load their action; under earl_debug_set_sawyer_prior_launches(2) TWO launches on the caller's stream
// over two contiguous ranges of v = k n + i -- the plain (or discounted) kernels over the first (K - P) n, then the prior kernel over the last P n, every row pointer
// advanced here.  Each range has its replicate launch, its form by its own count of virtual envs and its own work queue (a queue's progress words end at T: the second
// launch cannot reuse the first's).  The one-launch shape measured 1.5 - 1.9 x faster where K n fits one round of waves; the shapes give the same bits
static int sawyer_branch_launch(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                                const earl_episode_summary* summary, double* last_obs, int32_t* fail, const double* gamma, double* disc, const earl::SawyerPriorLaunch* pr,
                                earl_stream_t stream) {
  const earl_sawyer_out none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (!model || !cfg || !st || !act || !ws || K < 0 || H < 0 || (nv != 10 && nv != 15) || !sawyer_args_ok(kStep, cfg, st, nv, &none)) return EARL_ERR_ARG;
  const int n = cfg->n;
  if (act_branch_stride < 0 || (act_branch_stride != 0 && act_branch_stride < (int64_t)H * n * 4)) return EARL_ERR_ARG;
  if (!(summary && (summary->ret || summary->success_last || summary->first_success)) && !last_obs && !fail) return EARL_ERR_ARG;      // (nothing to compute)
  const int64_t V = (int64_t)K * n;
  if (V > INT32_MAX) return EARL_ERR_ARG;
  if (V > 0 && (!ws->base || (reinterpret_cast<uintptr_t>(ws->base) & 7) != 0 || ws->bytes < sawyer_branch_bytes(nv, V))) return EARL_ERR_ARG;
  if (g_lpe == 64) return EARL_ERR_ARG;                   // (the 64-lane measurement builds: no branch form)
  const int P = pr ? pr->prior->branches : 0;
  if (pr && (P < 1 || P >= K || !disc || !pr->sched || (act_branch_stride == 0 && H > 0))) return EARL_ERR_ARG;      // (checked by the entry point: sawyer_value.hip)
  if (V == 0 || H == 0) return EARL_OK;
  if (int rc = check_cone(col, true, (hipStream_t)stream, "sawyer_branch_rollout")) return rc;
  // the carve of the whole call's block, whatever the ranges: [V, nv + 1] qpos, [V, nv] qvel, [V, 3] mocap_pos, [V, 7] goal, [V, 14] rows, then the int32 words
  double* const base = static_cast<double*>(ws->base);
  int32_t* const words = reinterpret_cast<int32_t*>(base + V * (int64_t)(nv + 1 + nv + 3 + 7 + 14));
  // one launch over the virtual envs v0 .. v0 + Vr - 1 (whole branches: v0 a multiple of n, so v % n is the env inside the range too), `prior`: by the policy
  const int64_t k_first = K - P;                          // the call's first prior branch
  auto run = [&](const int64_t v0, const int64_t Vr, int32_t* const sched, const bool prior) -> int {
    double* d = base;
    earl_sawyer_state vs{};                               // the virtual envs' state: the workspace's rows (steps_since_reset, last_obs, fail_count: NULL, a branch keeps none)
    vs.qpos = d + v0 * (nv + 1); d += V * (nv + 1);       // (rows of the model's nq <= nv + 1: a range's rows start where rows of nv + 1 would, and stay inside the block)
    vs.qvel = d + v0 * nv; d += V * nv;
    vs.mocap_pos = d + v0 * 3; d += V * 3;
    vs.goal = d + v0 * 7; d += V * 7;
    double* const rows = d + v0 * 14;
    vs.steps_since_goal_change = cfg->goal_change_frequency > 0 ? words + v0 : nullptr;
    vs.obj_init = st->obj_init;                           // (read only, indexed by the env: v % n)
    SawyerBranchPriorArgs a{};                            // (the plain kernels read its base, the SawyerBranchArgs; the discounted ones the SawyerBranchValueArgs)
    a.gamma = gamma ? *gamma : 1.0;
    a.br_disc = disc ? disc + v0 : nullptr;
    static_cast<SawyerArgs&>(a) = SawyerArgs{model, col, *cfg, vs, act + (v0 / n) * act_branch_stride, H, none, nullptr, nullptr, nullptr, nullptr, 0, 0, clock};
    a.cfg.n = (int)Vr;
    a.n_env = n;
    a.act_stride = act_branch_stride;
    a.obs_row = last_obs ? last_obs + v0 * 14 : rows;
    a.br_ret = summary && summary->ret ? summary->ret + v0 : nullptr;
    a.br_last = summary && summary->success_last ? summary->success_last + v0 : nullptr;
    a.br_first = summary && summary->first_success ? summary->first_success + v0 : nullptr;
    a.br_fail = fail ? fail + v0 : nullptr;
    if (prior) {
      a.pol = *pr->prior->policy;
      a.obs0 = pr->prior->obs0;
      a.prior_act = pr->prior->act;
      for (int k = 0; k < 4; ++k) a.sigma[k] = pr->prior->sigma[k];
      a.word0 = pr->word0;
      a.noise_counter = pr->noise_counter;
      a.k0 = (int)(k_first - v0 / n);
      a.kbase = (int)(v0 / n);
    }
    // the form by the number of virtual envs of THIS launch, with the closed loop's reading of the door variants; the queue is always there, so the peg's time-sliced form is sawyer_form's to choose
    a.st.sched = sched;
    const SawyerForm form = sawyer_form(nv, (int)Vr, H, &a.st, true);
    if (form == SawyerForm::PegSliced) a.slice = peg_slice();
    else a.st.sched = nullptr;                            // (the replicate kernel clears the queue only where it is used)
    if (int rc = earl_unit_branch_replicate(static_cast<const SawyerBranchArgs*>(&a), st, nv, stream)) return rc;
    if (prior)
      switch (form) {
        case SawyerForm::DoorW8: return earl_unit_branch_prior_w8_sawyer_rollout(&a, stream);
        case SawyerForm::Door: case SawyerForm::Peg: return earl_unit_branch_prior_sawyer_rollout(&a, nv, 0, stream);
        case SawyerForm::PegSliced: return earl_unit_branch_prior_sawyer_rollout(&a, nv, 1, stream);
        default: return EARL_ERR_ARG;
      }
    if (gamma)
      switch (form) {
        case SawyerForm::DoorW8: return earl_unit_branch_value_w8_sawyer_rollout(static_cast<const SawyerBranchValueArgs*>(&a), stream);
        case SawyerForm::Door: case SawyerForm::Peg: return earl_unit_branch_value_sawyer_rollout(static_cast<const SawyerBranchValueArgs*>(&a), nv, 0, stream);
        case SawyerForm::PegSliced: return earl_unit_branch_value_sawyer_rollout(static_cast<const SawyerBranchValueArgs*>(&a), nv, 1, stream);
        default: return EARL_ERR_ARG;
      }
    switch (form) {
      case SawyerForm::DoorW8: return earl_unit_branch_w8_sawyer_rollout(static_cast<const SawyerBranchArgs*>(&a), stream);
      case SawyerForm::Door: case SawyerForm::Peg: return earl_unit_branch_sawyer_rollout(static_cast<const SawyerBranchArgs*>(&a), nv, 0, stream);
      case SawyerForm::PegSliced: return earl_unit_branch_sawyer_rollout(static_cast<const SawyerBranchArgs*>(&a), nv, 1, stream);
      default: return EARL_ERR_ARG;                       // (L64 was refused above; the policy reading never gives DoorSliced)
    }
  };
  if (!pr) return run(0, V, words + V, false);
  if (g_prior_fused) return run(0, V, words + V, true);   // ONE launch over all K n: the branches in front of K - P load their action inside the prior kernel
  const int64_t V1 = (int64_t)(K - P) * n;
  if (int rc = run(0, V1, words + V, false)) return rc;
  return run(V1, V - V1, pr->sched, true);
}
int earl_sawyer_branch_rollout(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                               const earl_episode_summary* summary, double* last_obs, int32_t* fail, earl_stream_t stream) {
  return sawyer_branch_launch(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, ws, summary, last_obs, fail, nullptr, nullptr, nullptr, stream);
}
// for sawyer_value.hip (declared there: it includes no stepper header): the launch above with the discounted sum, and where the [K n, 14] carried observation rows of
// a branch workspace start -- the rows the launch used when the caller gave no last_obs (the carve in sawyer_branch_launch: qpos, qvel, mocap_pos and goal rows before them)
__attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_discounted(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg,
                                                                             const earl_sawyer_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                                                             const uint64_t* clock, const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary,
                                                                             double* last_obs, int32_t* fail, double gamma, double* disc, earl_stream_t stream) {
  if (!disc) return EARL_ERR_ARG;
  return sawyer_branch_launch(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, ws, summary, last_obs, fail, &gamma, disc, nullptr, stream);
}
// ... and with the last pr->prior->branches branches run by the policy (earl_sawyer_branch_rollout_prior, sawyer_value.hip, which owns the checks of `pr`): gamma == 1.0
// runs the first range through the plain kernels, as the value-free call would; the prior kernels take gamma as it is.  The candidates are written, hence float*
__attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg,
                                                                        const earl_sawyer_state* st, int32_t K, int32_t H, float* act, int64_t act_branch_stride,
                                                                        const uint64_t* clock, const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary,
                                                                        double* last_obs, int32_t* fail, double gamma, double* disc, const earl::SawyerPriorLaunch* pr,
                                                                        earl_stream_t stream) {
  if (!disc || !pr || !pr->prior) return EARL_ERR_ARG;
  return sawyer_branch_launch(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, ws, summary, last_obs, fail, gamma == 1.0 ? nullptr : &gamma, disc, pr, stream);
}
__attribute__((visibility("hidden"))) double* earl_unit_sawyer_branch_rows(int32_t nv, int64_t V, void* base) {
  return static_cast<double*>(base) + V * (int64_t)(nv + 1 + nv + 3 + 7);
}

int earl_sawyer_reset(const earl_link_model* model, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                      const double* reset_qpos, const double* reset_qvel, const uint8_t* mask, double* obs,
                      earl_stream_t stream) {
  if (!model || !cfg || !st || !reset_qpos || !reset_qvel || !sawyer_args_ok(kReset, cfg, st)) return EARL_ERR_ARG;
  if (cfg->obj_dof < 0 || cfg->obj_dof >= nv || cfg->obj_kind < 0 || cfg->obj_kind > 2) return EARL_ERR_ARG;
  if (cfg->obj_kind >= 1 && cfg->obj_dof + 6 > nv) return EARL_ERR_ARG;
  if (cfg->obj_kind == 2 && (cfg->n_wide <= 0 || !cfg->wide_table)) return EARL_ERR_ARG;
  if (cfg->n == 0) return EARL_OK;
  SawyerArgs a{model, nullptr, *cfg, *st, nullptr, 0, earl_sawyer_out{nullptr, nullptr, nullptr, nullptr, nullptr}, reset_qpos, reset_qvel, mask, obs, 0, 0, nullptr};
  if (nv == 10) sawyer_reset_kernel<10, 16><<<grid_for<10, 16>(cfg->n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15) sawyer_reset_kernel<15, 16><<<grid_for<15, 16>(cfg->n), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else return EARL_ERR_ARG;
  return launched("sawyer_reset");
}

int earl_sawyer_observe(const earl_link_model* model, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st, double* obs,
                        earl_stream_t stream) {
  if (!model || !cfg || !st || !obs || !sawyer_args_ok(kObserve, cfg, st)) return EARL_ERR_ARG;
  if (cfg->n == 0) return EARL_OK;
  SawyerArgs a{model, nullptr, *cfg, *st, nullptr, 0, earl_sawyer_out{nullptr, nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr, nullptr, obs, 1, 0, nullptr};
  if (nv == 10) sawyer_reset_kernel<10, 16><<<grid_for<10, 16>(cfg->n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15) sawyer_reset_kernel<15, 16><<<grid_for<15, 16>(cfg->n), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else return EARL_ERR_ARG;
  return launched("sawyer_observe");
}

int earl_sawyer_door_reward(const earl_sawyer_cfg* cfg, int32_t n, const double* obs, float* reward, uint8_t* success,
                            earl_stream_t stream) {
  if (!cfg || n < 0 || !obs) return EARL_ERR_ARG;
  if (n == 0) return EARL_OK;
  sawyer_door_reward_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(n, obs, *cfg, reward, success);
  return launched("sawyer_door_reward");
}

int earl_sawyer_door_info(const earl_sawyer_cfg* cfg, int32_t n, const double* obs, const uint8_t* status, double* info, earl_stream_t stream) {
  if (!cfg || n < 0 || !obs || !info) return EARL_ERR_ARG;
  if (n == 0) return EARL_OK;
  sawyer_door_info_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(n, obs, *cfg, status, info);
  return launched("sawyer_door_info");
}

int earl_debug_set_physics_lanes(int lanes_per_env) {
  if (lanes_per_env != 16 && lanes_per_env != 64) return EARL_ERR_ARG;
  g_lpe = lanes_per_env;
  return EARL_OK;
}

#ifdef EARL_PHYS_PROF
int earl_debug_set_prof_wave(int block, int thread) { return prof_set_wave(block, thread); }     // the wave whose phases the profiling build clocks (default: workgroup 0, thread 0)
int earl_debug_read_wave_cycles(unsigned long long* out) { return prof_read_wave_cycles(out); }
int earl_debug_read_phys_profile(unsigned long long* out, int reset) { return prof_read_phases(out, reset); }
#endif

int earl_physics_model_size(void) { return (int)sizeof(earl_link_model); }
int earl_physics_model24_size(void) { return (int)sizeof(earl_link_model24); }
int earl_collision_model_size(void) { return (int)sizeof(earl_collision_model); }
int earl_sawyer_cfg_size(void) { return (int)sizeof(earl_sawyer_cfg); }

int earl_debug_set_peg_schedule(int sliced) {          // 0: one group per wave; 1: time-sliced, EARL_PEG_SLICE env steps per item; k >= 2: time-sliced, k env steps per item
  if (sliced < 0) return EARL_ERR_ARG;
  g_peg_sliced = sliced;
  return EARL_OK;
}
int earl_debug_set_sawyer_prior_launches(int launches) {      // 1 (default): the prior branches inside ONE launch over all K n virtual envs; 2: a launch of their own behind the plain one
  if (launches != 1 && launches != 2) return EARL_ERR_ARG;
  g_prior_fused = launches == 1;
  return EARL_OK;
}
int earl_debug_set_door_variant(int v) {
  if (v < 0 || v > 3) return EARL_ERR_ARG;
  g_door_variant = v;
  return EARL_OK;
}

}  // extern "C"

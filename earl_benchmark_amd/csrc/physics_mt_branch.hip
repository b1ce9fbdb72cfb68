// physics_mt_branch.hip -- the minitaur BRANCH launch (include/earl_physics.h: earl_minitaur_branch_rollout): K candidate action sequences per env scored from the current
// state in one launch of the rollout kernel over K n virtual envs, the state left as it is.  The kernels are the third inclusion of physics_env_minitaur_rollout.inc /
// physics_env_minitaur_duo.inc (minitaur_branch_kernel<false, true>, minitaur_branch_duo_kernel: BRANCH = true), instantiated here only.
//
// A translation unit of its own, the project's idiom for a second build (physics_mt_bf16.hip, physics_branch.hip): physics_mt.hip compiles to what it compiled to
// before -- no new device function in it --, and the units compile side by side.  Entry point, argument checks and the choice of the launch form: physics_mt.hip.
//
// What a branch mutates lives in the caller's workspace, [K n] rows indexed by the virtual env v = k n + i (minitaur_branch_ws.h): last stable qpos / qvel, the goal, the
// eight motors' overheat counters, enabled flags and observed torques, the goal-switch counter, the one carried observation row.  minitaur_branch_replicate_kernel fills
// them from the env's [n] rows in front of the rollout kernel (stream order), so that the rollout kernel's state pointers are simply the workspace's: its step loop
// loads, stores and rolls back exactly as the plain kernel's does, and holds nothing more across a timestep.
#define EARL_MT_BRANCH 1
#include "minitaur_device.h"
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "minitaur_stepper.h"
#include "physics_env_minitaur.h"

// [n] rows of `src` -> [K n] rows of a.st (a MinitaurBranchArgs' state: the workspace's), 128 threads per virtual env: thread c copies one element of the rows
// (qpos | qvel | goal | motor_param | observed_torque | the carried observation row | overheat | motor_enabled | the goal-switch counter | the count of rolled-back steps).
// The carried row starts as the env's row of last_obs -- what a step 0 that diverges re-emits --, NaN without one; the count of rolled-back steps (the caller's `fail`,
// a.st.fail_count) starts at 0.
__global__ __launch_bounds__(256) void minitaur_branch_replicate_kernel(const MinitaurBranchArgs a, const earl_minitaur_state src) {
  const int V = a.cfg.n, n = a.n_env;
  const long long v_ = (long long)blockIdx.x * 2 + (threadIdx.x >> 7);
  if (v_ >= V) return;
  const size_t v = (size_t)v_, i = (size_t)(v_ % n);
  int c = threadIdx.x & 127;
  if (c < 23) { a.st.qpos[v * 23 + c] = src.qpos[i * 23 + c]; return; }
  c -= 23;
  if (c < 22) { a.st.qvel[v * 22 + c] = src.qvel[i * 22 + c]; return; }
  c -= 22;
  if (c < 2) { a.st.goal[v * 2 + c] = src.goal[i * 2 + c]; return; }
  c -= 2;
  if (c < 6) { a.st.motor_param[v * 6 + c] = src.motor_param[i * 6 + c]; return; }
  c -= 6;
  if (c < 8) { a.st.observed_torque[v * 8 + c] = src.observed_torque[i * 8 + c]; return; }
  c -= 8;
  if (c < 32) { a.st.last_obs[v * 32 + c] = src.last_obs ? src.last_obs[i * 32 + c] : __builtin_nan(""); return; }
  c -= 32;
  if (c < 8) { a.st.overheat[v * 8 + c] = src.overheat[i * 8 + c]; return; }
  c -= 8;
  if (c < 8) { a.st.motor_enabled[v * 8 + c] = src.motor_enabled[i * 8 + c]; return; }
  c -= 8;
  if (c == 0 && a.st.steps_since_goal_change) a.st.steps_since_goal_change[v] = src.steps_since_goal_change[i];
  if (c == 1 && a.st.fail_count) a.st.fail_count[v] = 0;
}
static_assert(23 + 22 + 2 + 6 + 8 + 32 + 8 + 8 + 2 <= 128, "one thread per element of a virtual env's rows");
}  // namespace

#include "physics_launch.h"

extern "C" {

int earl_unit_mt_branch_replicate(const void* minitaur_branch_args, const void* src_state, void* stream) {
  const MinitaurBranchArgs& a = *static_cast<const MinitaurBranchArgs*>(minitaur_branch_args);
  minitaur_branch_replicate_kernel<<<(unsigned)((a.cfg.n + 1) / 2), 256, 0, (hipStream_t)stream>>>(a, *static_cast<const earl_minitaur_state*>(src_state));
  return launched("minitaur_branch_replicate");
}

// duo != 0: the two-waves-per-SIMD kernel; otherwise the one-wave kernel in the shape a.solo says (the forms as earl_minitaur_branch_rollout chose them, by K n)
int earl_unit_mt_branch_rollout(const void* minitaur_branch_args, int duo, void* stream) {
  const MinitaurBranchArgs& a = *static_cast<const MinitaurBranchArgs*>(minitaur_branch_args);
  const int V = a.cfg.n;
  if (duo) {
    minitaur_branch_duo_kernel<<<(unsigned)((V + 16 * MT_DUO_PAIRS / 4 - 1) / (4 * MT_DUO_PAIRS)), 128 * MT_DUO_PAIRS, 0, (hipStream_t)stream>>>(a);
    return launched("minitaur_branch_rollout (two waves per SIMD)");
  }
  minitaur_branch_kernel<false, true><<<solo_grid(V, a.solo, EARL_MT_WPB), 64 * EARL_MT_WPB, 0, (hipStream_t)stream>>>(a);
  return launched("minitaur_branch_rollout");
}

}  // extern "C"

// physics_branch.hip -- the Sawyer door / peg BRANCH launch (include/earl_physics.h: earl_sawyer_branch_rollout): K candidate action sequences per env scored from the
// current state in one launch of the rollout kernel over K n virtual envs, the state left as it is.  The kernel is the third inclusion of
// physics_env_sawyer_rollout.inc (sawyer_branch_rollout_kernel: BRANCH = true), instantiated here and in physics_branch_w8.hip only.
//
// A translation unit of its own, the project's idiom for a second build (physics_w8.hip, physics_bf16.hip): physics.hip and physics_w8.hip compile to what they
// compiled to before -- no new device function in them --, and the units compile side by side.  Entry point and argument checks: physics.hip.
//
// What a branch mutates lives in the caller's workspace, [K n] rows indexed by the virtual env v = k n + i: last stable qpos / qvel / mocap_pos, the goal row, the
// goal-switch counter, the one carried observation row, the work queue of the time-sliced peg form.  sawyer_branch_replicate_kernel fills them from the env's [n] rows
// in front of the rollout kernel (stream order), so that the rollout kernel's state pointers are simply the workspace's: its step loop loads, stores and rolls back
// exactly as the plain kernel's does, and holds nothing more across a timestep.
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_sawyer.h"

// [n] rows of `src` -> [K n] rows of `dst` (a SawyerBranchArgs' st), one 64-lane row of threads per virtual env: lane c copies one element of the row
// (qpos | qvel | mocap_pos | goal | the carried observation row | the goal-switch counter).  The carried row starts as the env's row of last_obs -- what a step 0 that
// diverges re-emits --, NaN without one.  Workgroup b also clears entries b and G + b of the work queue (G = gridDim.x = ceil(K n / 4) groups: progress, then lock).
__global__ __launch_bounds__(256) void sawyer_branch_replicate_kernel(const SawyerBranchArgs a, const earl_sawyer_state src, const int nv) {
  const int V = a.cfg.n, n = a.n_env;
  const int nq = static_cast<const earl_link_model*>(a.m)->nq;
  if (threadIdx.x == 0 && a.st.sched) { a.st.sched[blockIdx.x] = 0; a.st.sched[gridDim.x + blockIdx.x] = 0; }
  const long long v_ = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v_ >= V) return;
  const size_t v = (size_t)v_, i = (size_t)(v_ % n);
  int c = threadIdx.x & 63;
  if (c < nq) { a.st.qpos[v * nq + c] = src.qpos[i * nq + c]; return; }
  c -= nq;
  if (c < nv) { a.st.qvel[v * nv + c] = src.qvel[i * nv + c]; return; }
  c -= nv;
  if (c < 3) { a.st.mocap_pos[v * 3 + c] = src.mocap_pos[i * 3 + c]; return; }
  c -= 3;
  if (c < 7) { a.st.goal[v * 7 + c] = src.goal[i * 7 + c]; return; }
  c -= 7;
  if (c < 14) { a.obs_row[v * 14 + c] = src.last_obs ? src.last_obs[i * 14 + c] : __builtin_nan(""); return; }
  c -= 14;
  if (c == 0 && a.st.steps_since_goal_change) a.st.steps_since_goal_change[v] = src.steps_since_goal_change[i];
}
static_assert(EARL_MAXV + 1 + EARL_MAXV + 3 + 7 + 14 + 1 <= 64, "one lane per element of a virtual env's rows");
}  // namespace

#include "physics_launch.h"

extern "C" {

int earl_unit_branch_replicate(const void* sawyer_branch_args, const void* src_state, int nv, void* stream) {
  const SawyerBranchArgs& a = *static_cast<const SawyerBranchArgs*>(sawyer_branch_args);
  sawyer_branch_replicate_kernel<<<(a.cfg.n + 3) / 4, 256, 0, (hipStream_t)stream>>>(a, *static_cast<const earl_sawyer_state*>(src_state), nv);
  return launched("sawyer_branch_replicate");
}

// form as earl_sawyer_branch_rollout chose it: 0 = one group per wave (door: the one-wave build), 1 = the peg's time-sliced schedule (a.slice set, the queue cleared
// by the replicate kernel)
int earl_unit_branch_sawyer_rollout(const void* sawyer_branch_args, int nv, int sliced, void* stream) {
  const SawyerBranchArgs& a = *static_cast<const SawyerBranchArgs*>(sawyer_branch_args);
  const int V = a.cfg.n;
  if (nv == 10 && !sliced) sawyer_branch_rollout_kernel<10, 16><<<grid_for<10, 16>(V), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15 && sliced) sawyer_branch_rollout_kernel<15, 16, true><<<cu_count(), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15) sawyer_branch_rollout_kernel<15, 16><<<grid_for<15, 16>(V), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else return EARL_ERR_ARG;
  return launched("sawyer_branch_rollout");
}

}  // extern "C"

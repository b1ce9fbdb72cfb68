// minitaur_branch_ws.h -- the ONE statement of the workspace block of earl_minitaur_branch_rollout (include/earl_physics.h), read by the entry point (physics_mt.hip), by the
// replicate kernel's launch (physics_mt_branch.hip) and by the planner's layout (minitaur_plan.h), host side only.
// Per virtual env v = k n + i, V = K n of them, everything a branch mutates: float64 rows [V, 23] qpos, [V, 22] qvel, [V, 2] goal, [V, 6] motor_param (read only, copied
// so that the kernel's state pointers are simply the block's), [V, 8] observed_torque, [V, 32] the one carried observation row (unused when the caller's last_obs takes
// it); then int32 [V, 8] overheat counters and [V] goal-switch counters; then uint8 [V, 8] motor_enabled.  Offsets in bytes from the 8-byte aligned base.
#pragma once
#include <cstdint>

namespace earl {

struct MinitaurBranchLayout {
  int64_t qpos, qvel, goal, motor_param, observed_torque, last_obs, overheat, sgc, motor_enabled, bytes;
};
inline MinitaurBranchLayout minitaur_branch_layout(int64_t V) {
  MinitaurBranchLayout L;
  int64_t o = 0;
  L.qpos = o; o += V * 23 * 8;
  L.qvel = o; o += V * 22 * 8;
  L.goal = o; o += V * 2 * 8;
  L.motor_param = o; o += V * 6 * 8;
  L.observed_torque = o; o += V * 8 * 8;
  L.last_obs = o; o += V * 32 * 8;
  L.overheat = o; o += V * 8 * 4;
  L.sgc = o; o += V * 4;
  L.motor_enabled = o; o += V * 8;
  L.bytes = o;
  return L;
}

}  // namespace earl

// physics_branch_value.hip -- the Sawyer door / peg branch launch (physics_branch.hip) with the DISCOUNTED sum of earl_sawyer_branch_rollout_value (include/earl_physics.h,
// "discount and a terminal value on the door and the peg"): sawyer_branch_rollout_kernel compiled with EARL_BRANCH_DISCOUNT, so that sawyer_branch_summary keeps
// ret = sum_t d_t r_t with d_t beside it in the workspace (physics_env_sawyer.h: SawyerBranchValueArgs).  Reached with discount != 1 only; discount == 1 runs the
// kernels of physics_branch.hip.
//
// A translation unit of its own, the project's idiom for a second build: physics_branch.hip and physics_branch_w8.hip compile to what they compiled to before.  The
// replicate kernel is physics_branch.hip's (it reads the base of the argument block, which is the same here).  Entry point and argument checks: sawyer_value.hip and
// physics.hip.  The terminal value is a kernel of its own behind this one (sawyer_value.hip).
#define EARL_BRANCH_DISCOUNT 1
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_sawyer.h"
}  // namespace

#include "physics_launch.h"

extern "C" {

// form as physics.hip chose it: 0 = one group per wave, 1 = the peg's time-sliced schedule (a.slice set, the queue cleared by the replicate kernel)
int earl_unit_branch_value_sawyer_rollout(const void* sawyer_branch_value_args, int nv, int sliced, void* stream) {
  const SawyerBranchValueArgs& a = *static_cast<const SawyerBranchValueArgs*>(sawyer_branch_value_args);
  const int V = a.cfg.n;
  if (nv == 10 && !sliced) sawyer_branch_rollout_kernel<10, 16><<<grid_for<10, 16>(V), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15 && sliced) sawyer_branch_rollout_kernel<15, 16, true><<<cu_count(), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15) sawyer_branch_rollout_kernel<15, 16><<<grid_for<15, 16>(V), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else return EARL_ERR_ARG;
  return launched("sawyer_branch_rollout (discounted)");
}

}  // extern "C"

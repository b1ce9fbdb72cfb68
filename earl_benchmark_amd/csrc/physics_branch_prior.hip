// physics_branch_prior.hip -- the Sawyer door / peg branch launch whose actions are a POLICY's (include/earl_physics.h, "policy-prior branches on the door and the peg":
// earl_sawyer_branch_rollout_prior, earl_sawyer_plan_mppi_prior, earl_sawyer_plan_cem_prior): sawyer_prior_rollout_kernel, the fourth inclusion of
// physics_env_sawyer_rollout.inc -- the branch inclusion compiled with EARL_BRANCH_PRIOR, so that the action of env step t is the policy's on the row the virtual env
// carries plus the planner's noise (physics_env_sawyer.h: sawyer_prior_action), stored where a plain branch would load it.  By default ONE launch covers all K n
// virtual envs of a call -- the branches in front of K - P load their action here as they would in physics_branch.hip, and a wave without a prior branch never enters the
// policy phase --; under earl_debug_set_sawyer_prior_launches(2) it covers the LAST P branches only, behind a launch of the untouched kernels over the first K - P.
//
// Built with the discounted sum only: gamma == 1 gives the plain sum's bits (1.0 * r_t and d * 1.0 are exact), so one build serves both.  A translation unit of its own,
// the project's idiom for a second build: every other unit compiles to what it compiled to before.  The replicate kernel is physics_branch.hip's (it reads the base of the
// argument block).  Entry points and argument checks: sawyer_value.hip and physics.hip.
#define EARL_BRANCH_DISCOUNT 1
#define EARL_BRANCH_PRIOR 1
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_sawyer.h"
}  // namespace

#include "physics_launch.h"

extern "C" {

// form as physics.hip chose it by the launch's own count of virtual envs: 0 = one group per wave, 1 = the peg's time-sliced schedule (a.slice set, the launch's own queue
// cleared by its replicate launch)
int earl_unit_branch_prior_sawyer_rollout(const void* sawyer_branch_prior_args, int nv, int sliced, void* stream) {
  const SawyerBranchPriorArgs& a = *static_cast<const SawyerBranchPriorArgs*>(sawyer_branch_prior_args);
  const int V = a.cfg.n;
  if (nv == 10 && !sliced) sawyer_prior_rollout_kernel<10, 16><<<grid_for<10, 16>(V), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15 && sliced) sawyer_prior_rollout_kernel<15, 16, true><<<cu_count(), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15) sawyer_prior_rollout_kernel<15, 16><<<grid_for<15, 16>(V), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else return EARL_ERR_ARG;
  return launched("sawyer_prior_rollout");
}

}  // extern "C"

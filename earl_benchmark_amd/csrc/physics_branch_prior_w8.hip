// physics_branch_prior_w8.hip -- the door's prior-branch launch (physics_branch_prior.hip) in the EIGHT-wave build of physics_branch_w8.hip: the same defines, the same
// stepper, for a prior launch of more than 4096 virtual envs.  physics.hip picks it by the launch's count of virtual envs with sawyer_form's rule.
#define EARL_DOOR_WPB 8
#define EARL_DOOR_PACKED 1
#define EARL_DOOR_COOP 0
#define EARL_NO_PREFETCH 1
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

int earl_unit_branch_prior_w8_sawyer_rollout(const void* sawyer_branch_prior_args, void* stream) {
  const SawyerBranchPriorArgs& a = *static_cast<const SawyerBranchPriorArgs*>(sawyer_branch_prior_args);
  sawyer_prior_rollout_kernel<10, 16><<<grid_for<10, 16>(a.cfg.n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  return launched("sawyer_prior_rollout (door, 8 waves per CU)");
}

}  // extern "C"

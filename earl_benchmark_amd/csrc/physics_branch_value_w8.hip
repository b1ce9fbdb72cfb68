// physics_branch_value_w8.hip -- the door's discounted branch launch (physics_branch_value.hip) in the EIGHT-wave build of physics_branch_w8.hip: the same defines, the
// same stepper, for a launch of more than 4096 virtual envs.  physics.hip picks it by K n with sawyer_form's rule.
#define EARL_DOOR_WPB 8
#define EARL_DOOR_PACKED 1
#define EARL_DOOR_COOP 0
#define EARL_NO_PREFETCH 1
#define EARL_BRANCH_DISCOUNT 1
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_sawyer.h"
}  // namespace

#include "physics_launch.h"

extern "C" {

int earl_unit_branch_value_w8_sawyer_rollout(const void* sawyer_branch_value_args, void* stream) {
  const SawyerBranchValueArgs& a = *static_cast<const SawyerBranchValueArgs*>(sawyer_branch_value_args);
  sawyer_branch_rollout_kernel<10, 16><<<grid_for<10, 16>(a.cfg.n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  return launched("sawyer_branch_rollout (discounted; door, 8 waves per CU)");
}

}  // extern "C"

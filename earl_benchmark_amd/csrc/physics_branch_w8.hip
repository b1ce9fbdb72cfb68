// physics_branch_w8.hip -- the door's branch launch (physics_branch.hip) in the EIGHT-wave build of physics_w8.hip: the same defines, the same stepper, so a branch
// of a launch of more than 4096 virtual envs walks through the bits the eight-wave rollout walks through (tests/test_sawyer_full_gpu.py holds that build to the
// one-wave build's bits).  earl_sawyer_branch_rollout picks it by K n with sawyer_form's rule.
#define EARL_DOOR_WPB 8
#define EARL_DOOR_PACKED 1
#define EARL_DOOR_COOP 0
#define EARL_NO_PREFETCH 1
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_sawyer.h"
}  // namespace

#include "physics_launch.h"

extern "C" {

int earl_unit_branch_w8_sawyer_rollout(const void* sawyer_branch_args, void* stream) {
  const SawyerBranchArgs& a = *static_cast<const SawyerBranchArgs*>(sawyer_branch_args);
  sawyer_branch_rollout_kernel<10, 16><<<grid_for<10, 16>(a.cfg.n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  return launched("sawyer_branch_rollout (door, 8 waves per CU)");
}

}  // extern "C"

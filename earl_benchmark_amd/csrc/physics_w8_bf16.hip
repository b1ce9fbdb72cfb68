// physics_w8_bf16.hip -- the door's eight-wave rollout with the policy inside (physics_w8.hip's build settings), its parameters STORED as bf16: see physics_bf16.hip.
// The settings below are physics_w8.hip's, which says why each is what it is; only the policy kernel is instantiated here.
#define EARL_POLICY_BF16 1
#define EARL_DOOR_WPB 8
#define EARL_DOOR_PACKED 1
#define EARL_DOOR_COOP 0
#define EARL_NO_PREFETCH 1
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
namespace bf16 {
#include "physics_env_sawyer.h"
}  // namespace bf16
using namespace bf16;
}  // namespace

#include "physics_launch.h"

extern "C" {

int earl_unit_w8_bf16_sawyer_policy_rollout(const void* sawyer_policy_args, void* stream) {
  const SawyerPolicyArgs& a = *static_cast<const SawyerPolicyArgs*>(sawyer_policy_args);
  bf16::sawyer_policy_rollout_kernel<10, 16><<<grid_for<10, 16>(a.cfg.n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  return launched("sawyer_policy_rollout (door, 8 waves per CU, bf16 parameters)");
}

}  // extern "C"

// physics_bf16.hip -- the Sawyer door / peg rollout with the policy inside, its parameters STORED as bf16 (earl_mlp_policy.precision == EARL_PRECISION_BF16): the same
// kernel text as physics.hip's sawyer_policy_rollout_kernel<10 | 15, 16, sliced>, compiled with EARL_POLICY_BF16, which switches the element type of the weight path
// (policy_lane_group.h: pol_elem, pol_layer; policy_closed_loop.h: cl_policy_weights).  A stored value widens exactly to float32 and enters the same fmaf chains in
// the same order: a launch returns the bits of the float32 launch fed with the widened values.
//
// A translation unit of its own, the project's idiom for a second build (physics_w8.hip, physics_kitchen_policy.hip): physics.hip compiles to what it compiled to
// before -- no runtime branch inside sawyer_policy_action, no new template parameter in a kernel's name -- and the units compile side by side.  Only the policy kernels
// are instantiated here; the namespace bf16 tells them from the float32 kernels of the same name in a kernel trace.  Entry point and argument checks: physics.hip.
#define EARL_POLICY_BF16 1
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

// form as sawyer_closed_loop chose it: 0 = one group per wave (door: the one-wave build), 1 = the peg's time-sliced schedule (a.slice set)
int earl_unit_bf16_sawyer_policy_rollout(const void* sawyer_policy_args, int nv, int sliced, void* stream) {
  const SawyerPolicyArgs& a = *static_cast<const SawyerPolicyArgs*>(sawyer_policy_args);
  const int n = a.cfg.n;
  if (nv == 10 && !sliced) bf16::sawyer_policy_rollout_kernel<10, 16><<<grid_for<10, 16>(n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15 && sliced) bf16::sawyer_policy_rollout_kernel<15, 16, true><<<cu_count(), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15) bf16::sawyer_policy_rollout_kernel<15, 16><<<grid_for<15, 16>(n), block_for<15>(), 0, (hipStream_t)stream>>>(a);
  else return EARL_ERR_ARG;
  return launched("sawyer_policy_rollout (bf16 parameters)");
}

}  // extern "C"

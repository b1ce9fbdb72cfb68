// physics_kitchen_policy_bf16.hip -- the kitchen's fused rollout with the policy inside (kitchen_policy_rollout_kernel<0 | 1 | 2>), its parameters STORED as bf16
// (earl_mlp_policy.precision == EARL_PRECISION_BF16): physics_kitchen_policy.hip's kernel text compiled with EARL_POLICY_BF16.  Why a unit of its own, and what the
// define switches: physics_bf16.hip.  Entry point, argument checks and the choice of the launch form: physics_kitchen.hip.
#define EARL_POLICY_BF16 1
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
namespace bf16 {
#include "physics_env_kitchen.h"
}  // namespace bf16
using namespace bf16;
}  // namespace

#include "physics_launch.h"

extern "C" {

// k.solo as kitchen_closed_loop chose it (earl_unit_kitchen_policy_rollout)
void earl_unit_kitchen_bf16_policy_rollout(const void* kitchen_policy_args, void* stream) {
  const KitchenPolicyArgs& k = *static_cast<const KitchenPolicyArgs*>(kitchen_policy_args);
  const int n = k.cfg.n;
  if (k.solo == 3) bf16::kitchen_policy_rollout_kernel<1><<<n, block_for<23>(), 0, (hipStream_t)stream>>>(k);
  else if (k.solo == 4) bf16::kitchen_policy_rollout_kernel<2><<<(n + 1) / 2, block_for<23>(), 0, (hipStream_t)stream>>>(k);
  else bf16::kitchen_policy_rollout_kernel<0><<<solo_grid(n, k.solo, Lim<23>::WPB), block_for<23>(), 0, (hipStream_t)stream>>>(k);
}

}  // extern "C"

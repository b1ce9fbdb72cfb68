// physics_kitchen_policy.hip -- the kitchen's fused rollout with an MLP policy inside (kitchen_policy_rollout_kernel<0 | 1 | 2>, physics_env_kitchen.h): the kernels behind
// earl_kitchen_policy_rollout, whose entry point (argument checks, launch form) is physics_kitchen.hip's.
//
// A translation unit of its own so that physics_kitchen.hip compiles to what it compiled to before: in one module with the plain kitchen_rollout_kernel<1 | 2> the second
// instantiation of the same body changes the inliner's decisions for the lambdas of the split timestep (a local function with one call site is inlined at any size) and
// with them the plain kernels' schedule and register assignment.  Here the plain kernels stay byte-identical, and the two units compile side by side.
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_kitchen.h"
}  // namespace

#include "physics_launch.h"

extern "C" {

// k.solo as earl_kitchen_policy_rollout chose it: 0 / 1 / 2 the one-wave kernel in its three shapes, 3 four waves per env, 4 two waves per env
void earl_unit_kitchen_policy_rollout(const void* kitchen_policy_args, void* stream) {
  const KitchenPolicyArgs& k = *static_cast<const KitchenPolicyArgs*>(kitchen_policy_args);
  const int n = k.cfg.n;
  if (k.solo == 3) kitchen_policy_rollout_kernel<1><<<n, block_for<23>(), 0, (hipStream_t)stream>>>(k);
  else if (k.solo == 4) kitchen_policy_rollout_kernel<2><<<(n + 1) / 2, block_for<23>(), 0, (hipStream_t)stream>>>(k);
  else kitchen_policy_rollout_kernel<0><<<solo_grid(n, k.solo, Lim<23>::WPB), block_for<23>(), 0, (hipStream_t)stream>>>(k);
}

}  // extern "C"

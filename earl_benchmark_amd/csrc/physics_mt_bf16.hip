// physics_mt_bf16.hip -- the minitaur's two rollout kernels with the policy inside (minitaur_policy_kernel<false, true>, minitaur_policy_duo_kernel), its parameters
// STORED as bf16 (earl_mlp_policy.precision == EARL_PRECISION_BF16): physics_mt.hip's kernel text compiled with EARL_POLICY_BF16.  Why a unit of its own, and what the
// define switches: physics_bf16.hip.  Entry point, argument checks and the choice of the launch form: physics_mt.hip.
#define EARL_POLICY_BF16 1
#include "minitaur_device.h"
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
namespace bf16 {
#include "minitaur_stepper.h"
#include "physics_env_minitaur.h"
}  // namespace bf16
using namespace bf16;
}  // namespace

#include "physics_launch.h"

extern "C" {

// duo != 0: the two-waves-per-SIMD kernel; otherwise the one-wave kernel in the shape a.solo says
int earl_unit_mt_bf16_policy_rollout(const void* minitaur_policy_args, int duo, void* stream) {
  const MinitaurPolicyArgs& a = *static_cast<const MinitaurPolicyArgs*>(minitaur_policy_args);
  const int n = a.cfg.n;
  if (duo) {
    bf16::minitaur_policy_duo_kernel<<<(unsigned)((n + 16 * MT_DUO_PAIRS / 4 - 1) / (4 * MT_DUO_PAIRS)), 128 * MT_DUO_PAIRS, 0, (hipStream_t)stream>>>(a);
    return launched("minitaur_policy_rollout (two waves per SIMD, bf16 parameters)");
  }
  bf16::minitaur_policy_kernel<false, true><<<solo_grid(n, a.solo, EARL_MT_WPB), 64 * EARL_MT_WPB, 0, (hipStream_t)stream>>>(a);
  return launched("minitaur_policy_rollout (bf16 parameters)");
}

}  // extern "C"

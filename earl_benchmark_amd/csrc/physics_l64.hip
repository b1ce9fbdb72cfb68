// physics_l64.hip -- fourth build of the articulated-body stepper: the ONE-WAVEFRONT-PER-ENV (64 lanes) instantiations of the nv = 10 / 15 kernels
// (physics_kernel<10 | 15, 64, *>, sawyer_rollout_kernel<10 | 15, 64>): the measurement / test switch earl_debug_set_physics_lanes(64), which the parity tests use to show
// that results do not depend on the lane layout.  A translation unit of its own (round 5) so that the main unit does not carry them: a third of its compile time.
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_sawyer.h"
}  // namespace

#include "physics_launch.h"

extern "C" {

void earl_unit_l64_physics(const void* pargs, int nv, int integrate, void* stream) {
  const PArgs& a = *static_cast<const PArgs*>(pargs);
  const hipStream_t st = (hipStream_t)stream;
  if (nv == 10 && integrate) physics_kernel<10, 64, true><<<grid_for<10, 64>(a.n), block_for<10>(), 0, st>>>(a);
  else if (nv == 10) physics_kernel<10, 64, false><<<grid_for<10, 64>(a.n), block_for<10>(), 0, st>>>(a);
  else if (nv == 15 && integrate) physics_kernel<15, 64, true><<<grid_for<15, 64>(a.n), block_for<15>(), 0, st>>>(a);
  else if (nv == 15) physics_kernel<15, 64, false><<<grid_for<15, 64>(a.n), block_for<15>(), 0, st>>>(a);
}
void earl_unit_l64_sawyer_rollout(const void* sawyer_args, int nv, void* stream) {
  const SawyerArgs& a = *static_cast<const SawyerArgs*>(sawyer_args);
  if (nv == 10) sawyer_rollout_kernel<10, 64><<<grid_for<10, 64>(a.cfg.n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  else if (nv == 15) sawyer_rollout_kernel<15, 64><<<grid_for<15, 64>(a.cfg.n), block_for<15>(), 0, (hipStream_t)stream>>>(a);
}

}  // extern "C"

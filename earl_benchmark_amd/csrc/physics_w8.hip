// physics_w8.hip -- second build of the Sawyer-door rollout kernel: EIGHT wavefronts per CU.
//
// The door model's env block was cut to 4.4 KB (packed mass matrix and Hessian, the weld Jacobian aliased with the Hessian, 8-word contact
// records), so an eight-wave workgroup (32 envs + ONE copy of the model / block tables = 155 KB) fits a CU's 160 KB of LDS: two waves per SIMD
// hide each other's LDS round trips and dependent-issue stalls (one wave per SIMD issues on 55 % of its cycles).  The
// price is the 256-register cap of two waves per SIMD (204 B of scratch per lane, none of it touched inside the timestep loop).  N = 8192 is then ONE round of
// 256 workgroups instead of two rounds of 1024 single-wave ones.  Same source, same arithmetic, bit-identical outputs
// (tests/test_sawyer_full_gpu.py); earl_sawyer_rollout picks it for batches of more than 4096 envs.
#define EARL_DOOR_WPB 8
#define EARL_DOOR_PACKED 1
#define EARL_DOOR_COOP 0        // register-resident factorisation, as in the single-wave build.  (The lane-cooperative in-LDS form was the faster one
                                // while this build still reloaded spilled values inside the timestep -- 73.1 against 77.4 ms; with those gone it is the
                                // slower one: 60.3 against 57.5 ms.)
#define EARL_NO_PREFETCH 1      // no prefetch of the first near block's pair record: the second wave hides that latency, the 22 registers are worth more
#include "physics_stepper.h"
#include "policy_check.h"
#include "policy_math.h"

namespace {
#include "physics_env_sawyer.h"
}  // namespace

#include "physics_launch.h"

extern "C" {

int earl_unit_w8_sawyer_rollout(const void* sawyer_args, void* stream) {
  const SawyerArgs& a = *static_cast<const SawyerArgs*>(sawyer_args);
  sawyer_rollout_kernel<10, 16><<<grid_for<10, 16>(a.cfg.n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  return launched("sawyer_rollout (door, 8 waves per CU)");
}
int earl_unit_w8_sawyer_policy_rollout(const void* sawyer_policy_args, void* stream) {
  const SawyerPolicyArgs& a = *static_cast<const SawyerPolicyArgs*>(sawyer_policy_args);
  sawyer_policy_rollout_kernel<10, 16><<<grid_for<10, 16>(a.cfg.n), block_for<10>(), 0, (hipStream_t)stream>>>(a);
  return launched("sawyer_policy_rollout (door, 8 waves per CU)");
}
int earl_sawyer_rollout_door_w8(const earl_link_model* model, const earl_collision_model* col, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                const float* action, int32_t T, const earl_sawyer_out* out, earl_stream_t stream) {
  SawyerArgs a{model, col, *cfg, *st, action, T, *out, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr};
  return earl_unit_w8_sawyer_rollout(&a, stream);
}

#ifdef EARL_PHYS_PROF
int earl_debug_set_prof_wave_w8(int block, int thread) { return prof_set_wave(block, thread); }     // (eight-wave workgroups: thread = 64 x the wave)
int earl_debug_read_wave_cycles_w8(unsigned long long* out) { return prof_read_wave_cycles(out); }
int earl_debug_read_phys_profile_w8(unsigned long long* out, int reset) { return prof_read_phases(out, reset); }
#endif

}  // extern "C"

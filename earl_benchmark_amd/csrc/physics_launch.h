// physics_launch.h -- host helpers of the stepper units (physics.hip, physics_w8.hip, physics_l64.hip, physics_kitchen.hip, physics_kitchen_policy.hip, physics_mt.hip and the four *_bf16.hip):
// launch checks, the calls from one unit into another, launch geometry and the profiling build's hooks.  Included after physics_stepper.h and the
// unit's env kernels; what sits in the anonymous namespace here is the including unit's own copy.
#pragma once

// cone word of a device collision table, cached per address (defined in the main unit; -1 = unknown); see check_cone
extern "C" __attribute__((visibility("hidden"))) int earl_unit_table_cone(const void* col, void* stream);
// the 64-lanes-per-env instantiations live in physics_l64.hip (argument structs by address: same source, same layout in both units); not exported from the library
extern "C" __attribute__((visibility("hidden"))) void earl_unit_l64_physics(const void* pargs, int nv, int integrate, void* stream);
extern "C" __attribute__((visibility("hidden"))) void earl_unit_l64_sawyer_rollout(const void* sawyer_args, int nv, void* stream);
extern "C" __attribute__((visibility("hidden"))) void earl_unit_kitchen_physics(const void* pargs, int integrate, void* stream);      // physics_kitchen.hip: nv = 23
// the kitchen rollout with the policy inside (physics_kitchen_policy.hip): earl_kitchen_policy_rollout hands it its KitchenPolicyArgs, launch form chosen (solo)
extern "C" __attribute__((visibility("hidden"))) void earl_unit_kitchen_policy_rollout(const void* kitchen_policy_args, void* stream);
// the door's eight-wave rollout (physics_w8.hip): earl_sawyer_rollout(_clocked) hands it its argument struct (the clock included); earl_sawyer_rollout_door_w8 is
// exported like the other entry points
extern "C" __attribute__((visibility("hidden"))) int earl_unit_w8_sawyer_rollout(const void* sawyer_args, void* stream);
// the same hand-over for the rollout with the policy inside (earl_sawyer_policy_rollout; the argument is a SawyerPolicyArgs)
extern "C" __attribute__((visibility("hidden"))) int earl_unit_w8_sawyer_policy_rollout(const void* sawyer_policy_args, void* stream);
// the units compiled with EARL_POLICY_BF16 (policy parameters stored as bf16: physics_bf16.hip, physics_w8_bf16.hip, physics_mt_bf16.hip,
// physics_kitchen_policy_bf16.hip): the closed-loop entry points hand them the argument struct they filled, launch form chosen, when policy->precision says so
extern "C" __attribute__((visibility("hidden"))) int earl_unit_bf16_sawyer_policy_rollout(const void* sawyer_policy_args, int nv, int sliced, void* stream);
extern "C" __attribute__((visibility("hidden"))) int earl_unit_w8_bf16_sawyer_policy_rollout(const void* sawyer_policy_args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int earl_unit_mt_bf16_policy_rollout(const void* minitaur_policy_args, int duo, void* stream);
extern "C" __attribute__((visibility("hidden"))) void earl_unit_kitchen_bf16_policy_rollout(const void* kitchen_policy_args, void* stream);
// the branch launch (physics_branch.hip, physics_branch_w8.hip): earl_sawyer_branch_rollout hands them the SawyerBranchArgs it filled -- first to the replicate kernel
// (src_state: the env's own earl_sawyer_state, whose [n] rows become the workspace's [K n]; it also clears the work queue), then to the rollout kernel of the form chosen
extern "C" __attribute__((visibility("hidden"))) int earl_unit_branch_replicate(const void* sawyer_branch_args, const void* src_state, int nv, void* stream);
extern "C" __attribute__((visibility("hidden"))) int earl_unit_branch_sawyer_rollout(const void* sawyer_branch_args, int nv, int sliced, void* stream);
extern "C" __attribute__((visibility("hidden"))) int earl_unit_branch_w8_sawyer_rollout(const void* sawyer_branch_args, void* stream);
// the same launch with the discounted sum (physics_branch_value.hip, physics_branch_value_w8.hip): the argument is a SawyerBranchValueArgs; the replicate kernel is the one above
extern "C" __attribute__((visibility("hidden"))) int earl_unit_branch_value_sawyer_rollout(const void* sawyer_branch_value_args, int nv, int sliced, void* stream);
extern "C" __attribute__((visibility("hidden"))) int earl_unit_branch_value_w8_sawyer_rollout(const void* sawyer_branch_value_args, void* stream);
// the branch launch whose actions are a policy's (physics_branch_prior.hip, physics_branch_prior_w8.hip): the argument is a SawyerBranchPriorArgs over all K n virtual envs
// of a call, or over the last P branches with its rows advanced by physics.hip; the replicate kernel is the one above
extern "C" __attribute__((visibility("hidden"))) int earl_unit_branch_prior_sawyer_rollout(const void* sawyer_branch_prior_args, int nv, int sliced, void* stream);
extern "C" __attribute__((visibility("hidden"))) int earl_unit_branch_prior_w8_sawyer_rollout(const void* sawyer_branch_prior_args, void* stream);
extern "C" int earl_sawyer_rollout_door_w8(const earl_link_model* model, const earl_collision_model* col, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                           const float* action, int32_t T, const earl_sawyer_out* out, earl_stream_t stream);

namespace {

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "earl_physics: %s: %s\n", what, hipGetErrorString(e));
    return EARL_ERR_LAUNCH;
  }
  return EARL_OK;
}

// The kernels compile the friction cone per model size (Lim<NV>::ELLIPTIC) and the two cones lay the contact arrays out differently, so a collision table
// compiled for the other cone must be refused (include/earl_physics.h: earl_collision_model.cone).  `col` is a DEVICE table: its cone word is copied to the
// host once per device address (4 bytes, a blocking copy -- never while the stream is being captured into a graph: the check is then skipped for an address
// not yet seen) and remembered in ONE cache for all translation units (earl_unit_table_cone, main unit) until its owner announces that the block is gone:
// earl_physics_forget_table (the Python front end calls it when a DeviceModel is freed -- a caching allocator hands the block to the next table, which may be of
// the other cone: ADVICE r05).
int check_cone(const earl_collision_model* col, const bool want_elliptic, hipStream_t st, const char* what) {
  if (!col) return EARL_OK;
  const int cone = earl_unit_table_cone(col, st);
  if (cone < 0) return EARL_OK;            // (unknown: a capture in progress, or not a device table -- the launch reports that)
  if (cone != (want_elliptic ? 1 : 0)) {
    fprintf(stderr, "earl_physics: %s: the collision table is compiled for the %s friction cone, this model size runs the %s one (earl_collision_model.cone)\n", what,
            cone == 1 ? "elliptic" : "pyramidal", want_elliptic ? "elliptic" : "pyramidal");
    return EARL_ERR_ARG;
  }
  return EARL_OK;
}

// compute units of the current device (256 if the query fails)
int cu_count() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}

// Small batches of the 32-lanes-per-env kernels (kitchen, minitaur): an env is a serial chain of T x frame_skip timesteps walked by one wave, so a batch that leaves
// wave slots empty gains nothing from them -- except by giving every env a wave (solo 1: up to 4 x CUs envs) or a whole CU (solo 2: up to CUs envs) to itself.
// earl_debug_set_solo: -1 = by batch size (default), 0 / 1 / 2 = forced (measurement, tests); the kitchen's fused rollout runs its one-env-per-workgroup launches with
// all FOUR waves on the env (solo 3: by default, or forced; 2 forces the one-wave form)
int g_solo = -1;
int solo_mode(int n) {
  if (g_solo >= 0) return g_solo;
  const int cus = cu_count();
  return n <= cus ? 2 : (n <= 4 * cus ? 1 : 0);
}
int solo_grid(int n, int solo, int wpb) { return solo == 2 ? n : (solo == 1 ? (n + wpb - 1) / wpb : (n + 2 * wpb - 1) / (2 * wpb)); }

// launch geometry: Lim<NV>::WPB wavefronts per workgroup, 64 / LPE envs per wavefront
template <int NV, int LPE> int grid_for(int n) { constexpr int epb = (64 / LPE) * Lim<NV>::WPB; return (n + epb - 1) / epb; }
template <int NV> constexpr int block_for() { return 64 * Lim<NV>::WPB; }

#ifdef EARL_PHYS_PROF
// Phase timing (physics_stepper.h): every unit has its own device counters, so each unit's exported hooks (earl_debug_set_prof_wave*, earl_debug_read_wave_cycles*,
// earl_debug_read_phys_profile*) call these.  Templates so that only a unit that instantiates them refers to the counters from host code: a host reference makes
// g_prof_sel a variable the host may write, and physics_l64.hip, which has no hooks, keeps it the constant 0 in its kernels.
template <int = 0> int prof_set_wave(int block, int thread) {     // the wave whose phases are clocked (default: workgroup 0, thread 0)
  const int v[2] = {block, thread};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_prof_sel), v, sizeof(v)) == hipSuccess ? EARL_OK : EARL_ERR_LAUNCH;
}
template <int = 0> int prof_read_wave_cycles(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_cycles), sizeof(unsigned long long) * 4096) == hipSuccess ? EARL_OK : EARL_ERR_LAUNCH;
}
template <int = 0> int prof_read_phases(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phys_prof), sizeof(unsigned long long) * 32) != hipSuccess) return EARL_ERR_LAUNCH;
  if (reset) {
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phys_prof), z, sizeof(z)) != hipSuccess) return EARL_ERR_LAUNCH;
  }
  return EARL_OK;
}
#endif

}  // namespace

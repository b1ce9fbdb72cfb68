// physics_env_kitchen.h -- the kitchen env kernels: the small per-step kernels around the stepper and the fused rollout
// Included by physics_kitchen.hip, inside the anonymous namespace, after the stepper (physics_stepper.h): split out in round 5 so that a change to one env's kernels
// recompiles only the translation units that hold them (csrc/Makefile lists the headers per unit).

// ------------------------------------------------------------------------------------------------ kitchen env step (include/earl_physics.h)
// small per-env kernels around the stepper; the numpy glue of the reference (action scaling, observation noise, reward) stays in csrc/glue.hip
struct KitchenArgs {
  earl_kitchen_cfg cfg;
  earl_kitchen_state st;
  earl_kitchen_out out;
  const float* action;
  int n_att;
};
// before the stepper: the float32 action promoted to float64 (np.clip keeps float32; the reference's scaling then promotes), the state saved
__global__ void kitchen_pre_kernel(const KitchenArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.cfg.n * 23) return;
  const int e = i / 23, j = i % 23;
  a.st.qpos_bak[i] = a.st.qpos[i];
  a.st.qvel_bak[i] = a.st.qvel[i];
  if (j < 9) a.st.action64[e * 9 + j] = (double)a.action[e * 9 + j];
  if (j < 3) a.st.mocap_bak[e * 3 + j] = a.st.mocap_pos[e * 3 + j];      // (before earl_kitchen_action moves the target)
  for (int k = j; k < a.n_att * 3; k += 23) a.st.att_bak[(size_t)e * a.n_att * 3 + k] = a.st.att_xpos[(size_t)e * a.n_att * 3 + k];
}
// after the stepper: failure guard (roll a diverged env back), the eight task sites gathered for the reward
__global__ void kitchen_guard_kernel(const KitchenArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.cfg.n) return;
  bool bad = false;
  for (int j = 0; j < 23; ++j) bad = bad || !(fabs(a.st.qpos[e * 23 + j]) < EARL_BAD_VALUE) || !(fabs(a.st.qvel[e * 23 + j]) < EARL_BAD_VALUE);
  if (bad) {
    // rolled back: state, the mocap target the diverged step was pulled towards, the attachment positions (possibly NaN) the stepper left
    for (int j = 0; j < 23; ++j) { a.st.qpos[e * 23 + j] = a.st.qpos_bak[e * 23 + j]; a.st.qvel[e * 23 + j] = a.st.qvel_bak[e * 23 + j]; }
    for (int j = 0; j < 3; ++j) a.st.mocap_pos[e * 3 + j] = a.st.mocap_bak[e * 3 + j];
    for (int k = 0; k < a.n_att * 3; ++k) a.st.att_xpos[(size_t)e * a.n_att * 3 + k] = a.st.att_bak[(size_t)e * a.n_att * 3 + k];
    if (a.st.fail_count) a.st.fail_count[e] += 1;
  }
  if (a.out.status) a.out.status[e] = bad ? EARL_STEP_DIVERGED : 0;
  a.st.bad[e] = bad ? 1 : 0;
  for (int k = 0; k < 8; ++k)
    for (int c = 0; c < 3; ++c) a.st.sites[(e * 8 + k) * 3 + c] = a.st.att_xpos[(e * a.n_att + a.cfg.site_att[k]) * 3 + c];
}
// last: the observation / reward / flags of the step (a rolled-back env returns its last stable observation, reward 0), wrapper bookkeeping
__global__ void kitchen_finish_kernel(const KitchenArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.cfg.n) return;
  const bool bad = a.st.bad[e] != 0;
  for (int k = 0; k < 46; ++k) {
    const double v = bad ? a.st.last_obs[e * 46 + k] : a.out.obs[e * 46 + k];
    a.out.obs[e * 46 + k] = v;
    a.st.last_obs[e * 46 + k] = v;
    if (k < 9 && !bad) a.st.last_qp_robot[e * 9 + k] = v;          // the newest cached (noisy) robot joint readings
  }
  if (bad) { a.out.reward[e] = 0.0; a.out.success[e] = 0; }
  const int steps = a.st.steps_since_reset[e] + 1;
  a.st.steps_since_reset[e] = steps;
  a.out.done[e] = (a.cfg.horizon > 0 && steps >= a.cfg.horizon) ? 1 : 0;
}
// The whole env step of earl_kitchen_step, T times, in ONE launch: a wave walks its two envs through action glue -> 40 timesteps -> failure guard ->
// observation (Philox noise) -> reward -> bookkeeping without ever meeting the other waves.  A launch of the stepper lasts as long as its slowest
// wave -- the one env with a finger on a fixture -- and between the launches of consecutive env steps every other wave waited for it; here the
// waves drift apart and only the sum over the rollout counts.  Same arithmetic as the per-step kernels above and csrc/glue.hip (expression by
// expression: kitchen_action_kernel, kitchen_obs_kernel, uniform_kernel, kitchen_reward_kernel, kitchen_guard / finish): bit-identical outputs.
struct KitchenRolloutArgs {
  const void* m;
  const earl_collision_model* col;
  earl_kitchen_params p;
  earl_kitchen_cfg cfg;
  earl_kitchen_state st;
  earl_kitchen_out out;          // rows [T, n, ...]
  const float* action;           // [T, n, 9]
  int T;
  int solo;                      // small batches (round 5): 1 = ONE env per wave -- the wave's second 32-lane group shadows the first one's env (same state, same actions, same
                                 // branches; stores nothing), so the env's chain of timesteps is not held up by a wave-mate on a longer path; 2 = also one wave per workgroup
                                 // (waves 1-3 leave after the tables are staged): every env has a CU's LDS and issue slots to itself.  Same numbers as the packed launch.
  const uint64_t* clock;         // earl_kitchen_rollout_clocked: DEVICE words, [0] added to cfg.counter (NULL = zero); read where the noise is drawn, once per env step
};
__device__ __forceinline__ double kit_norm_diff(const double* a, const double* b, const int n) {     // glue.hip norm_diff
  double d = 0.0;
  for (int i = 0; i < n; ++i) {
    const double x = a[i] - b[i];
    d = fma(x, x, d);
  }
  return sqrt(d);
}

// ------------------------------------------------------------------------------------------------ the policy phase of the policy kernels (earl_kitchen_policy_rollout)
// The rollout's arguments (action unused) plus the policy.  A struct of its own so that the plain kernels' argument stays what it was
#include "policy_closed_loop.h"
struct KitchenPolicyArgs : ClosedLoopArgs<KitchenRolloutArgs> {};      // pol.dims[0] = 46, pol.dims[n_layers] = 9 (18 with the head); goal rows of 23
static_assert(std::is_standard_layout<KitchenRolloutArgs>::value && std::is_trivially_copyable<KitchenPolicyArgs>::value, "the policy phase reads KitchenPolicyArgs as laid out in the kernel-argument segment");
// A float32 MLP 46 -> H1 (-> H2) -> 9 | 18 evaluated by the 32 lanes of an env between two env steps: element k of a layer on lane k & 31 in register k >> 5.  The input
// layer is pol_layer<32, false> (rows of 46 floats = 184 bytes are no whole 16-byte pieces; its second k-tile holds 14 elements), every later one pol_layer<32, true>
// (hidden widths are multiples of 16 and params is 16-byte aligned, so every later row starts on a 16-byte boundary).
// -> the action's element `sub` on lanes 0 .. 8 of the group, as stored in act_out.
// `seen`: the env's row of 46 doubles the policy sees (NULL at step 0: the env's row of obs0); `row` = t n + env.  A group that is not live (an idle group of the last
// wave / workgroup, a solo launch's shadow) computes on zeros and stores nothing: the row of the env an idle group shadows is written by another wave, and a read of it
// would race with that wave; the shadow of a solo launch takes the live group's action from its own wave afterwards (kit_step_action).
// A population: `gid` picks the member, gid / pop_G.  A group that is not live comes with the id of the env it shadows (the kernel clamps `env` to n - 1, a solo shadow has
// its wave-mate's), so the rows it reads are those of a member that exists: no id at or beyond env_offset + n is ever formed.  (The helper waves of the several-wave forms
// never get here.)
// The policy's kernel arguments are read HERE, through the kernel-argument pointer the caller passed through an empty asm: read as `a.pol...` they would be loaded once at
// kernel entry and held in scalar registers across every timestep (see sawyer_policy_action).  Nothing of the policy lives across a timestep.
__device__ __noinline__ float kitchen_policy_action(const uint64_t ka_bits, const uint64_t ev, const uint32_t gid, const uint64_t seed, const double* __restrict__ seen, const int env,
                                                    const size_t row, const int sub, const bool live) {
#pragma clang fp contract(off)
  const EARL_KARG KitchenPolicyArgs* ka = cl_kernarg<KitchenPolicyArgs>(ka_bits);
  const int n_layers = ka->pol.n_layers, d1 = ka->pol.dims[1], d2 = ka->pol.dims[2], d3 = ka->pol.dims[3];
  const int hidden_act = ka->pol.hidden_act, out_act = ka->pol.out_act;
  if (!seen) seen = ka->obs0 + (size_t)env * 46;       // step 0
  float h[8];
  // each double rounded once to float32; lane `sub` reads the elements lane `sub` stored (sub and sub + 32)
  h[0] = live ? (float)seen[sub] : 0.f;
  h[1] = (live && sub + 32 < 46) ? (float)seen[sub + 32] : 0.f;
#pragma unroll
  for (int i = 2; i < 8; ++i) h[i] = 0.f;
  const pol_elem* w = cl_policy_weights(ka, gid, env, row, sub == 0 && live);      // (the member's rows, the network of the pair's phase)
  pol_layer<32, false>(w, w + (size_t)d1 * 46, 46, d1, hidden_act, sub, h);
  w += (size_t)d1 * (46 + 1);
  if (n_layers == 3) {
    pol_layer<32, true>(w, w + (size_t)d2 * d1, d1, d2, hidden_act, sub, h);
    w += (size_t)d2 * (d1 + 1);
  }
  const int KL = n_layers == 3 ? d2 : d1, NL = n_layers == 3 ? d3 : d2;
  pol_layer<32, true>(w, w + (size_t)NL * KL, KL, NL, EARL_ACT_NONE, sub, h);       // lane j < NL holds output j
  const int d = sub < 9 ? sub : 8;                     // this lane's action dimension (lanes 9 .. 31 repeat dimension 8 and store nothing)
  float u;
  if (ka->gauss) {
    // lanes 0 .. 8 are the head's nine dimensions: mean on the lane itself, raw log_std nine lanes up
    const float mean = __shfl(h[0], d, 32), raw = __shfl(h[0], d + 9, 32);
    // THREE Philox blocks per (env, env step), counter words {kGaussDraw + b, global id, ev}: ev = the step's sensor-noise counter (cfg.counter plus the clock word of a
    // graph-captured launch, plus t), whose draw indices are 0x4B00 + j: the streams are disjoint.  Words x, y, z, w of block b serve action dimensions 4 b .. 4 b + 3;
    // block 2 uses x only.
    const int c = d & 3;
    const earl::U4 b = earl::philox4x32_10(earl::U4{earl::kGaussDraw + (uint32_t)(d >> 2), gid, (uint32_t)ev, (uint32_t)(ev >> 32)}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float eps = earl::normal_quantile_f32((c == 0 ? b.x : (c == 1 ? b.y : (c == 2 ? b.z : b.w))) >> 8);
    u = earl::gaussian_head_action(earl_gaussian_head{ka->head.mode, ka->head.log_std_map, ka->head.log_std_min, ka->head.log_std_max, nullptr}, out_act, mean, raw, eps);
    float* eps_out = ka->head.eps_out;
    if (sub < 9 && live && eps_out) eps_out[row * 9 + sub] = eps;
  } else {
    u = earl::policy_act(h[0], out_act);
  }
  float* act_out = ka->act_out;
  if (sub < 9 && live && act_out) act_out[row * 9 + sub] = u;
  return u;
}
// the action component `kk` of env step t as this lane's double, before the env step's own [-1, 1] clip, computed by the policy.  `A` is the policy kernel's argument
// struct (a template so that the plain kernels, which name this call in a discarded statement, never instantiate it)
template <class A>
__device__ __forceinline__ double kit_policy_step(const A& a, const int t, const int n, const int env, const int sub, const int grp, const int kk, const bool live) {
#pragma clang fp contract(off)
  const size_t row = (size_t)t * n + env;
  // what the policy sees: the row this env emitted last, exactly as it stands in out.obs (sensor noise included, a rolled-back step's repeated row), each double
  // rounded to float32; at step 0 the caller's obs0.  Lane `sub` reads the elements lane `sub` wrote (the observation loop and the rollback both store elements
  // sub and sub + 32 from lane `sub`), after the agent-scope fence that ends every env step.
  // (out.obs == NULL, earl_kitchen_population_rollout: the env's row of st.last_obs, which holds the same bits: the observation loop writes both, the rollback leaves it)
  const double* seen = t > 0 ? (a.out.obs ? a.out.obs + (row - n) * 46 : a.st.last_obs + (size_t)env * 46) : nullptr;
  const uint64_t ev = a.cfg.counter + (a.clock ? a.clock[0] : 0) + (uint64_t)t;      // the step's sensor-noise counter (read per step, like the noise's)
  // (offset 0 of the kernel-argument segment is the kernel's one argument, the KitchenPolicyArgs)
  const float u = kitchen_policy_action((uint64_t)cl_kernarg<KitchenPolicyArgs>(), ev, (uint32_t)(a.cfg.env_offset + env), a.cfg.seed, seen, env, row, sub, live);
  // the env step consumes the float32 values stored in act_out: lanes 0 .. 8 of the live group hold them.  The second group of a one-env-per-wave launch (solo >= 1)
  // is the first one's shadow and steps with the bits of the live group's action (wave-wide shuffle; the choice is wave-uniform)
  return (double)__shfl(u, a.solo >= 1 ? kk : grp * 32 + kk, 64);
}
// The agent pair's handover after env step t (include/earl_physics.h, earl_kitchen_agents_rollout, items 5 and 6), worked out by the 32 lanes of the env's owner wave
// from the same words: the step's success flag from lane 0 of the live group, phase and steps_in_phase from HBM, where that lane stores them again -- nothing of the
// pair lives across a timestep.  The pair's kernel arguments are read through the kernel-argument segment here, where they are used (see kitchen_policy_action on why).
// The goal in force IS the env's row of st.goal, which the observation loop reads at every step: a handover that changes it stores the new row there and patches entries
// 23 .. 45 of the row the env emitted at this step (row t of out.obs if given, and the env's row of st.last_obs), each entry by the lane that emitted it; this step's
// reward was computed before, from the row as emitted.  Called by the policy kernels only; `a`'s own members are KitchenRolloutArgs'
template <class A>
__device__ __forceinline__ void kit_pair_handover(const A& a, const int t, const int env, const size_t row, const int sub, const int grp, const bool live, const bool failed,
                                                  const uint8_t suc) {
#pragma clang fp contract(off)
  const EARL_KARG KitchenPolicyArgs* ka = cl_kernarg<KitchenPolicyArgs>();
  // (the second group of a one-env-per-wave launch is the first one's shadow and takes the live group's flag: the same branches)
  const bool success = __shfl((int)((!failed && suc) ? 1 : 0), a.solo >= 1 ? 0 : grp * 32, 64) != 0;
  // ev: the step's sensor-noise counter (the noise draws with 0x4B00 + j, the head with 0x504F4C00 + b)
  cl_pair_handover(ka, t, env, row, sub == 0 && live, success, (uint32_t)(a.cfg.env_offset + env), a.cfg.seed, a.cfg.counter, a.clock, ka->pair_fwd, ka->pair_fwd_rows,
                   [&](const double* table, const int gi) {
                     if (!live) return;
                     for (int k = sub; k < 46; k += 32) {
                       if (k < 23) continue;
                       const double gv = table[(size_t)gi * 23 + (k - 23)];
                       a.st.goal[(size_t)env * 23 + (k - 23)] = gv;
                       if (a.out.obs) a.out.obs[row * 46 + k] = gv;
                       a.st.last_obs[(size_t)env * 46 + k] = gv;
                     }
                   });
}
// DUO (solo == 3, round 5): the FOUR waves of the workgroup, one per SIMD, work on its one env (substep's ROLE 1 - 4).  Per timestep all run the kinematics; then, side by
// side: wave 0 (B, owns the env) the constraint rows, wave 1 (A) the mass matrix into wave 0's LDS block, wave 2 the bias forces, wave 3 the bounding tests and the collision
// phases (contact records into wave 0's block); barrier X; wave 1 builds the equality Hessian in wave 0's block while wave 0 does the contact rows and its right-hand side;
// barrier Y; wave 0 iterates on the active set while wave 1 factorises for the integration (K10's arm block and fixture scalars: barrier Z); wave 0 integrates; barrier 2;
// waves 1 - 3 copy the new state.  Barrier 0, once per env step, keeps them off the state while wave 0
// does the env step's bookkeeping and hands over the step's actuator targets.  Waves 1 - 3 keep no env state of their own and store nothing outside LDS.
// DUO == 2 (solo == 4: batches of at most TWO envs per CU): two envs per workgroup, two waves each -- waves 0 / 2 own an env and run its collision phases too (ROLE 6), waves
// 1 / 3 do its mass matrix, bias forces, equality Hessian and K10's factor (ROLE 5); the same barriers, shared by the workgroup's two envs.
template <int DUO>
__global__ __launch_bounds__(64 * Lim<23>::WPB) void kitchen_rollout_kernel(const KitchenRolloutArgs a) {
#include "physics_env_kitchen_rollout.inc"
}
// The same kernel with the policy inside (earl_kitchen_policy_rollout), all three launch forms.  `a` must stay the kernel's ONLY argument: the policy phase reads
// a.pol / a.head / a.gauss / a.obs0 / a.act_out through the kernel-argument segment pointer.  The helper waves of the several-wave forms (DUO 1, 2) take no part in the
// policy phase: the owner wave computes the action where the plain kernel loads it, before barrier 0, where they wait as they do in the plain kernel.
template <int DUO>
__global__ __launch_bounds__(64 * Lim<23>::WPB) void kitchen_policy_rollout_kernel(const KitchenPolicyArgs a) {
#include "physics_env_kitchen_rollout.inc"
}

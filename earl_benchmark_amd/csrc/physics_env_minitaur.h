// physics_env_minitaur.h -- the minitaur env kernel: reset incl. its settle steps and the fused rollout, on the tree-structured timestep of minitaur_stepper.h or the generic one
// Included by physics_mt.hip, inside the anonymous namespace, after the stepper (physics_stepper.h): split out in round 5 so that a change to one env's kernels
// recompiles only the translation units that hold them (csrc/Makefile lists the headers per unit).

// ------------------------------------------------------------------------------------------------ minitaur env (include/earl_physics.h; physics_mt.hip)
// One launch = T env steps (or the reset incl. its settle steps) of every env: 32 lanes per env, two envs per wave; lanes 0-7 of a group are also
// the eight MOTORS (Minitaur.ApplyAction per timestep: velocity-limited command, DC-motor model, overheat protection -- csrc/minitaur_device.h),
// whose counters and flags live in those lanes' registers between timesteps.  Reference of every expression: oracle/minitaur_oracle.py.
struct MinitaurArgs {
  const void* m;
  const earl_collision_model* col;
  earl_minitaur_cfg cfg;
  earl_minitaur_state st;
  earl_minitaur_out out;
  const float* action; int T;
  const uint8_t* mask; double* reset_obs;
  int solo;                      // as KitchenRolloutArgs::solo
  const uint64_t* clock;         // earl_minitaur_rollout_clocked: DEVICE words, [1] added to cfg.step_counter (NULL = zero); read where a goal-switch draw is made
};
__device__ __forceinline__ double mt_draw(const earl_minitaur_cfg& cfg, const uint32_t stream, const int env, const uint64_t counter) {
  const earl::U4 b = earl::philox4x32_10(earl::U4{stream, (uint32_t)(cfg.env_offset + env), (uint32_t)counter, (uint32_t)(counter >> 32)},
                                         (uint32_t)cfg.seed, (uint32_t)(cfg.seed >> 32));
  return earl::u01(b.x, b.y);
}
// ARROW: the timestep written on the model's tree (minitaur_stepper.h: substep_mt, the product path) or the generic substep<22> above (kept for
// comparison: earl_debug_set_minitaur_stepper(0); same numbers to rounding)
#ifndef EARL_MT_WPB
#define EARL_MT_WPB 4            // wavefronts per workgroup of the tree-structured kernels
#endif
#ifndef EARL_MT_BLOCKS
#define EARL_MT_BLOCKS 1         // ... and workgroups per CU the register budget is set for (2 = two waves per SIMD, 256 registers each: spills 1.4 KB per lane and runs 1.5 x slower, tools/bench_mt_variant.py)
#endif
#ifndef EARL_MT_DUO_DEFAULT
#define EARL_MT_DUO_DEFAULT -1   // g_mt_duo at start-up: -1 = the launcher picks the rollout kernel by batch size (mt_use_duo), 0 = always the one-wave kernel, 1 = the two-waves-per-SIMD
                                 // kernel (minitaur_duo_kernel below) for every packed launch.  The two kernels return the same bits (tests/test_minitaur_gpu.py), so the choice is
                                 // about speed only: 16 resident envs per CU against 8, a round of the two-wave kernel taking 1.6 x a round of the one-wave kernel
#endif
template <bool ARROW> constexpr int mt_wpb() { return ARROW ? EARL_MT_WPB : Lim<22>::WPB; }

// ------------------------------------------------------------------------------------------------ the policy phase of the two policy kernels (earl_minitaur_policy_rollout)
// The rollout's arguments (action unused) plus the policy.  A struct of its own so that the plain kernels' argument stays what it was
#include "policy_closed_loop.h"
struct MinitaurPolicyArgs : ClosedLoopArgs<MinitaurArgs> {};      // pol.dims[0] = 32, pol.dims[n_layers] = 8 (16 with the head); goal rows of 2
static_assert(std::is_standard_layout<MinitaurArgs>::value && std::is_trivially_copyable<MinitaurPolicyArgs>::value, "the policy phase reads MinitaurPolicyArgs as laid out in the kernel-argument segment");
// ------------------------------------------------------------------------------------------------ the branch launch (earl_minitaur_branch_rollout; kernels: physics_mt_branch.hip)
// The rollout's arguments over K n_env VIRTUAL envs v = k n_env + i: cfg.n is their number, `st` the [K n_env] rows of the caller's workspace (filled by
// minitaur_branch_replicate_kernel in front of the rollout kernel; st.last_obs the one carried observation row, st.fail_count the caller's `fail`, st.steps_since_reset
// NULL), every pointer of `out` NULL, `action` the [K, H, n_env, 8] candidates.  The fields below are read through the kernel-argument segment where they are used
// (policy_closed_loop.h on why)
struct MinitaurBranchArgs : MinitaurArgs {
  int n_env;                     // the env's own n: the env of v is v % n_env, its branch v / n_env
  int64_t act_stride;            // floats between consecutive branches' [H, n_env, 8] blocks (0: every branch replays one block)
  double* br_ret;                // earl_episode_summary of the launch, each NULL or [K n_env]
  uint8_t* br_last;
  int32_t* br_first;
};
static_assert(std::is_trivially_copyable<MinitaurBranchArgs>::value, "the branch pieces read MinitaurBranchArgs as laid out in the kernel-argument segment");
// the virtual env's episode summary after env step t, by lane 0: cl_episode_summary's three words, each its definition applied to the step's reward and success (a
// rolled-back step: 0 and 0)
__device__ __forceinline__ void mt_branch_summary(const int t, const int v, const double r_t, const uint8_t s_t) {
  const EARL_KARG MinitaurBranchArgs* ka = cl_kernarg<MinitaurBranchArgs>();
  double* const br_ret = ka->br_ret;
  uint8_t* const br_last = ka->br_last;
  int32_t* const br_first = ka->br_first;
  if (br_ret) br_ret[v] = (t > 0 ? br_ret[v] : 0.0) + r_t;            // sum over t ascending of (double)reward_t
  if (br_last) br_last[v] = s_t;                                      // (the one of step H - 1 stays)
  if (br_first) {
    const int32_t f = t > 0 ? br_first[v] : -1;
    br_first[v] = (f < 0 && s_t) ? t : f;
  }
}
// the env whose id a draw of `env` uses: `env` itself, or -- BRANCH, `env` a virtual env -- the env it is a branch of
template <bool BRANCH>
__device__ __forceinline__ int mt_draw_env(const int env) {
  if constexpr (BRANCH) return env % cl_kernarg<MinitaurBranchArgs>()->n_env;
  else return env;
}
// A float32 MLP 32 -> H1 (-> H2) -> 8 | 16 evaluated by the 32 lanes of an env between two env steps (pol_layer<32, true>: element k of a layer on lane k & 31 in register
// k >> 5; K = 32 makes the input layer a vector layer too).  -> the action's element `sub` on lanes 0 .. 7 of the group, as stored in act_out.
// `seen`: the env's row of 32 doubles the policy sees (NULL at step 0: the env's row of obs0); `row` = t n + env.  A group that is not live (an idle group of the last
// wave / workgroup, a solo launch's shadow) computes on zeros and stores nothing: the row of the env it shadows is written by other lanes -- of another wave in the packed
// forms -- and a read of it would race with them; what such a group simulates is never stored.
// A population: `gid` picks the member, gid / pop_G.  A group that is not live comes with the id of the env it shadows (the callers clamp `env` to n - 1, a solo shadow has
// its wave-mate's), so the rows it reads are those of a member that exists: no id at or beyond env_offset + n is ever formed.
// The policy's kernel arguments are read HERE, through the kernel-argument pointer the caller passed through an empty asm: read as `a.pol...` they would be loaded once at
// kernel entry and held in scalar registers across every timestep (see sawyer_policy_action).  Nothing of the policy lives across a timestep.
__device__ __noinline__ float minitaur_policy_action(const uint64_t ka_bits, const uint64_t ev, const uint32_t gid, const uint64_t seed, const double* __restrict__ seen, const int env,
                                                     const size_t row, const int sub, const bool live) {
#pragma clang fp contract(off)
  const EARL_KARG MinitaurPolicyArgs* ka = cl_kernarg<MinitaurPolicyArgs>(ka_bits);
  const int n_layers = ka->pol.n_layers, d1 = ka->pol.dims[1], d2 = ka->pol.dims[2], d3 = ka->pol.dims[3];
  const int hidden_act = ka->pol.hidden_act, out_act = ka->pol.out_act;
  if (!seen) seen = ka->obs0 + (size_t)env * 32;       // step 0
  float h[8];
  h[0] = live ? (float)seen[sub] : 0.f;
#pragma unroll
  for (int i = 1; i < 8; ++i) h[i] = 0.f;
  const pol_elem* w = cl_policy_weights(ka, gid, env, row, sub == 0 && live);      // (the member's rows, the network of the pair's phase)
  pol_layer<32, true>(w, w + (size_t)d1 * 32, 32, d1, hidden_act, sub, h);
  w += (size_t)d1 * (32 + 1);
  if (n_layers == 3) {
    pol_layer<32, true>(w, w + (size_t)d2 * d1, d1, d2, hidden_act, sub, h);
    w += (size_t)d2 * (d1 + 1);
  }
  const int KL = n_layers == 3 ? d2 : d1, NL = n_layers == 3 ? d3 : d2;
  pol_layer<32, true>(w, w + (size_t)NL * KL, KL, NL, EARL_ACT_NONE, sub, h);       // lane j < NL holds output j
  float u;
  if (ka->gauss) {
    // lanes 0..7 are the head's eight dimensions: mean on the lane itself, raw log_std eight lanes up
    const float raw = __shfl(h[0], (sub & 7) + 8, 32);
    // TWO Philox blocks per (env, env step), counter words {kGaussDraw + b, global id, ev}: ev = the host's step counter plus the clock word of a graph-captured launch,
    // plus t -- the goal-switch draw's of the same step, whose draw index is 0xFFFE (the reset's are 0x4D00 .. 0x4D06): the streams are disjoint.  Words x, y, z, w of
    // block b serve action dimensions 4 b .. 4 b + 3.
    const int d = sub & 3;
    const earl::U4 b = earl::philox4x32_10(earl::U4{earl::kGaussDraw + (uint32_t)((sub >> 2) & 1), gid, (uint32_t)ev, (uint32_t)(ev >> 32)}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float eps = earl::normal_quantile_f32((d == 0 ? b.x : (d == 1 ? b.y : (d == 2 ? b.z : b.w))) >> 8);
    u = earl::gaussian_head_action(earl_gaussian_head{ka->head.mode, ka->head.log_std_map, ka->head.log_std_min, ka->head.log_std_max, nullptr}, out_act, h[0], raw, eps);
    float* eps_out = ka->head.eps_out;
    if (sub < 8 && live && eps_out) eps_out[row * 8 + sub] = eps;
  } else {
    u = earl::policy_act(h[0], out_act);
  }
  float* act_out = ka->act_out;
  if (sub < 8 && live && act_out) act_out[row * 8 + sub] = u;
  return u;
}
// the action of env step t, as eight clipped doubles on every lane of the group: given (the plain kernels) or computed here (POLICY).  `A` is the kernel's argument struct
template <bool POLICY, class A>
__device__ __forceinline__ void mt_step_action(const A& a, const int t, const int n, const int env, const int sub, const bool live, double (&a64)[8]) {
#pragma clang fp contract(off)
  const size_t row = (size_t)t * n + env;
  if constexpr (std::is_same<A, MinitaurBranchArgs>::value) {
    // the branch launch: `env` is the virtual env v, its action row (k, t, i) of the [K, H, n_env, 8] candidates
    const EARL_KARG MinitaurBranchArgs* ka = cl_kernarg<MinitaurBranchArgs>();
    const int n_env = ka->n_env, k = env / n_env, i = env - k * n_env;
    const float* ap = a.action + (size_t)k * (size_t)ka->act_stride + ((size_t)t * n_env + i) * 8;
#pragma unroll
    for (int d = 0; d < 8; ++d) a64[d] = earl::mt_clipd((double)ap[d], -1.01, 1.01);
  } else if constexpr (POLICY) {
    // what the policy sees: the row this env emitted last, exactly as it stands in out.obs (a rolled-back step's repeated row, the goal entries a goal switch patched),
    // each double rounded to float32; at step 0 the caller's obs0.  Lane `sub` reads the element lane `sub` wrote (observe, the rollback and the goal switch all store
    // element `sub` from lane `sub`), after the agent-scope fence that ends every env step.
    // (out.obs == NULL, earl_minitaur_population_rollout: the env's row of st.last_obs, the one observation row such a launch keeps)
    const double* seen = t > 0 ? (a.out.obs ? a.out.obs + (row - n) * 32 : a.st.last_obs + (size_t)env * 32) : nullptr;
    const uint64_t ev = a.cfg.step_counter + (a.clock ? a.clock[1] : 0) + (uint64_t)t;      // (read per step, like the goal switch's)
    // (offset 0 of the kernel-argument segment is the kernel's one argument, the MinitaurPolicyArgs)
    const float u = minitaur_policy_action((uint64_t)cl_kernarg<MinitaurPolicyArgs>(), ev, (uint32_t)(a.cfg.env_offset + env), a.cfg.seed, seen, env, row, sub, live);
    // the env step consumes the float32 values stored in act_out: lanes 0 .. 7 hold them
#pragma unroll
    for (int k = 0; k < 8; ++k) a64[k] = earl::mt_clipd((double)__shfl(u, k, 32), -1.01, 1.01);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) a64[k] = earl::mt_clipd((double)a.action[row * 8 + k], -1.01, 1.01);      // (the front end raises beyond the reference's bound)
  }
}
// The agent pair's handover after env step t (include/earl_physics.h, earl_minitaur_agents_rollout, items 5 and 6), worked out by all 32 lanes of the env from the same
// words: the step's success flag from lane 0, phase and steps_in_phase from HBM, where lane 0 stores them again -- nothing of the pair lives across a timestep.  The
// pair's kernel arguments are read through the kernel-argument segment here, where they are used (see minitaur_policy_action on why).  A handover that changes the goal
// leaves the new one in goal0 / goal1 and in the env's row of st.goal, and patches entries 30 / 31 of the row the env emitted at this step, as the lifelong switch does
// (which a pair launch never runs: goal_change_frequency > 0 is refused).  Called by the policy kernels only; `a`'s own members are MinitaurArgs'
template <class A>
__device__ __forceinline__ void mt_pair_handover(const A& a, const int t, const int env, const size_t row, const int sub, const bool live, const bool failed, const uint8_t suc,
                                                 double& goal0, double& goal1) {
#pragma clang fp contract(off)
  const bool success = __shfl((int)((!failed && suc) ? 1 : 0), 0, 32) != 0;
  // entering the forward phase: the lifelong switch's draw for this step (0xFFFE, cfg.goal_table), with its counter words
  cl_pair_handover(cl_kernarg<MinitaurPolicyArgs>(), t, env, row, sub == 0 && live, success, (uint32_t)(a.cfg.env_offset + env), a.cfg.seed, a.cfg.step_counter,
                   a.clock ? a.clock + 1 : nullptr, a.cfg.goal_table, a.cfg.n_goals, [&](const double* table, const int gi) {
                     goal0 = table[2 * gi]; goal1 = table[2 * gi + 1];
                     if (live && sub >= 30) (a.out.obs ? a.out.obs + row * 32 : a.st.last_obs + (size_t)env * 32)[sub] = sub == 30 ? goal0 : goal1;
                     if (live && sub == 0) { a.st.goal[(size_t)env * 2] = goal0; a.st.goal[(size_t)env * 2 + 1] = goal1; }
                   });
}
#ifndef EARL_MT_BRANCH             // (physics_mt_branch.hip holds the branch kernels only)
template <bool RESET, bool ARROW>
__global__ __launch_bounds__(64 * mt_wpb<ARROW>(), ARROW ? EARL_MT_BLOCKS : 1) void minitaur_kernel(const MinitaurArgs a) {
#include "physics_env_minitaur_rollout.inc"
}
// The same kernel with the policy inside (earl_minitaur_policy_rollout; instantiated at <false, true> only: all three launch shapes of the tree-structured rollout).
// `a` must stay the kernel's ONLY argument: the policy phase reads a.pol / a.head / a.gauss / a.obs0 / a.act_out through the kernel-argument segment pointer
template <bool RESET, bool ARROW>
__global__ __launch_bounds__(64 * mt_wpb<ARROW>(), ARROW ? EARL_MT_BLOCKS : 1) void minitaur_policy_kernel(const MinitaurPolicyArgs a) {
#include "physics_env_minitaur_rollout.inc"
  static_assert(!RESET && ARROW, "the policy form derives from minitaur_kernel<false, true>");
}
#else
// The branch form (earl_minitaur_branch_rollout), the body's third inclusion: BRANCH = true.  It takes the policy form's arms -- no [T] row, the summaries on lane 0, the
// carried row handled as the population launch handles st.last_obs -- with the action loaded at (k, t, i) and every draw made with the ENV's id.  `a` must stay the
// kernel's ONLY argument: the branch fields are read through the kernel-argument segment pointer
template <bool RESET, bool ARROW>
__global__ __launch_bounds__(64 * mt_wpb<ARROW>(), ARROW ? EARL_MT_BLOCKS : 1) void minitaur_branch_kernel(const MinitaurBranchArgs a) {
#include "physics_env_minitaur_rollout.inc"
  static_assert(!RESET && ARROW, "the branch form derives from minitaur_kernel<false, true>");
}
#endif

// ------------------------------------------------------------------------------------------------ two waves per SIMD by ROLE (round 6)
// The one-wave kernel above needs all 512 registers of a SIMD lane (256 + 256 accumulation registers used as spill space): one wave per SIMD, the vector ALU issuing in
// half of its cycles.  Capped at 256 registers it spills 1.2 KB per lane and runs 1.7 x slower (profiles/r06_minitaur_two_waves_per_simd.txt).  What does fit 256 registers is
// HALF a timestep: the dynamics half (frames, bounding and pair tests, mass matrix, bias forces, closure rows: substep_mt<.., 1>) and the solver half (active-set passes: substep_mt<.., 2>; the integration runs at the head of the first-half wave's next visit) are each other's only long-lived register state.  So a workgroup is EIGHT waves, two per SIMD: waves 0 - 3 run first halves, waves
// 4 - 7 second halves, wave p and wave p + 4 work as a pair on TWO env pairs (four envs) alternately -- while A runs the first half of timestep k of env pair X, B runs the
// second half of timestep k of env pair Y (whose first half A finished in the slot before); one barrier of the PAIR per slot (a flag each in LDS).  16 envs per CU: 4096 envs are ONE round of the
// chip instead of two.  An env's per-step state (motor counters, command, goal, wrapper counters) lives in its LDS block (SharedMTData::ev) between the visits of wave A,
// which also runs everything around the timesteps (action fetch and leg model, motor model, observation, reward, state rows).  Same expressions as the one-wave kernel.
constexpr int MT_DUO_PAIRS = 4;
#if !defined(EARL_POLICY_BF16) && !defined(EARL_MT_BRANCH)      // (physics_mt_bf16.hip holds the policy kernels only, physics_mt_branch.hip the branch kernels)
__global__ __launch_bounds__(128 * MT_DUO_PAIRS, 1) void minitaur_duo_kernel(const MinitaurArgs a) {
#include "physics_env_minitaur_duo.inc"
}
#endif
// The two-wave kernel with the policy inside: wave A computes env step t's action where the plain kernel loads it (k == 0, after finish_step(t - 1)).  `a` must stay the ONLY argument
#ifndef EARL_MT_BRANCH
__global__ __launch_bounds__(128 * MT_DUO_PAIRS, 1) void minitaur_policy_duo_kernel(const MinitaurPolicyArgs a) {
#include "physics_env_minitaur_duo.inc"
}
#else
// ... and the branch form of the two-wave kernel.  `a` must stay the ONLY argument
__global__ __launch_bounds__(128 * MT_DUO_PAIRS, 1) void minitaur_branch_duo_kernel(const MinitaurBranchArgs a) {
#include "physics_env_minitaur_duo.inc"
}
#endif

// physics_env_sawyer.h -- the Sawyer door / peg env kernels: fused rollout (optionally time-sliced), reset / observe; the reward / info kernels of given observations are in physics.hip
// Included by physics.hip, physics_w8.hip and physics_l64.hip, inside the anonymous namespace, after the stepper (physics_stepper.h): split out in round 5 so that a change to one env's kernels
// recompiles only the translation units that hold them (csrc/Makefile lists the headers per unit).

// ------------------------------------------------------------------------------------------------ Sawyer env kernels
struct SawyerArgs {
  const void* m;
  const earl_collision_model* col;
  earl_sawyer_cfg cfg;
  earl_sawyer_state st;
  const float* action; int T;
  earl_sawyer_out out;
  const double* reset_qpos; const double* reset_qvel; const uint8_t* mask; double* reset_obs;
  int observe_only;
  int slice;                     // SLICED rollout: env steps per work item (0: one item = the whole rollout of a group)
  const uint64_t* clock;         // earl_sawyer_rollout_clocked: DEVICE words added to cfg.counter / cfg.step_counter (NULL = zero); [1] is read where a goal-switch draw is made
};
// earl_sawyer_policy_rollout: the rollout's arguments (action unused) plus the policy.  A struct of its own so that the plain kernels' argument stays what it was
#include "policy_closed_loop.h"
struct SawyerPolicyArgs : ClosedLoopArgs<SawyerArgs> {};      // pol.dims[0] = 14, pol.dims[n_layers] = 4 (8 with the head); goal rows of 7
// earl_sawyer_branch_rollout: the rollout's arguments over the K n VIRTUAL envs of the launch -- cfg.n = K n, st = the [K n] rows of the caller's workspace (st.obj_init:
// the env's own [n] rows; steps_since_reset, last_obs, fail_count NULL), every pointer of `out` NULL -- plus what a branch reads and keeps.  A struct of its own, like
// SawyerPolicyArgs and for its reason; the fields below are read through the kernel-argument segment where they are used (policy_closed_loop.h)
struct SawyerBranchArgs : SawyerArgs {
  int n_env;                     // the env's n: virtual env v is branch k = v / n_env of env i = v % n_env
  int64_t act_stride;            // floats between two branches' [T, n_env, 4] blocks of `action` (0: one block for all)
  double* obs_row;               // [K n, 14] the one observation row a virtual env keeps: the caller's last_obs output, or the workspace's rows
  double* br_ret;                // the branch's episode summary and its count of rolled-back steps, each NULL or [K n]: kept as cl_episode_summary keeps a summary
  uint8_t* br_last;
  int32_t* br_first;
  int32_t* br_fail;
};
// earl_sawyer_branch_rollout_value with discount != 1: the branch block followed by gamma and the branch's running discount.  A derived struct once more, so that
// the plain branch kernels' argument -- and with it their code objects -- stays what it was.  d_t goes THROUGH THE WORKSPACE beside br_ret (br_disc, [K n] words of the
// caller's block: after env step t the word holds d_{t+1}), because nothing of a branch may live across a timestep and in the time-sliced form another wave takes
// the next slice; recomputing d_t from t at every step would cost t multiplications per step.  The bits are the recurrence's either way.
struct SawyerBranchValueArgs : SawyerBranchArgs {
  double gamma;                  // 0 < gamma < 1 (gamma == 1 runs the plain branch kernels)
  double* br_disc;               // [K n]
};
// EARL_BRANCH_DISCOUNT: the compile-time flag of sawyer_branch_rollout_kernel, set by physics_branch_value.hip and physics_branch_value_w8.hip only (a define, like
// EARL_DOOR_WPB: the kernel keeps its name and its template parameters, so the units without the define compile to what they compiled to before)
#ifndef EARL_BRANCH_DISCOUNT
#define EARL_BRANCH_DISCOUNT 0
#endif
constexpr bool kBranchDiscount = EARL_BRANCH_DISCOUNT != 0;
using SawyerBranchKernelArgs = std::conditional<kBranchDiscount, SawyerBranchValueArgs, SawyerBranchArgs>::type;
// earl_sawyer_branch_rollout_prior (include/earl_physics.h, "policy-prior branches on the door and the peg"): the discounted block followed by the policy of the prior
// branches and their noise.  A derived struct once more.  Virtual env v of the launch is branch kbase + v / n_env of the call; the launch's branches from k0 on are the
// policy's (their block of `action` is written here, not read), those before it load their action as a plain branch does.  Two launch shapes use it (physics.hip):
// ONE launch over all K n virtual envs (kbase = 0, k0 = K - P), or a launch over the last P n only, every row pointer advanced on the host (kbase = K - P, k0 = 0).
struct SawyerBranchPriorArgs : SawyerBranchValueArgs {
  earl_mlp_policy pol;           // 14 -> H1 (-> H2) -> 4, float32, one network
  const double* obs0;            // [n_env, 14]: what the policy sees at step 0
  float* prior_act;              // NULL or [P, T, n_env, 4]: the action rows once more (act_stride is the candidates' own)
  float sigma[4];
  uint32_t word0;                // the planner's draw word | the iteration (kPlanDraw | j, kCemDraw | j)
  uint32_t noise_counter;
  int k0;                        // the launch's first prior branch
  int kbase;                     // the call's index of the launch's branch 0 (the noise words are keyed by the call's k)
};
// EARL_BRANCH_PRIOR: set by physics_branch_prior.hip and physics_branch_prior_w8.hip only (with EARL_BRANCH_DISCOUNT: gamma == 1 gives the plain sum's bits, 1.0 * r_t
// and d * 1.0 being exact); it switches the branch pieces of the rollout body to the policy phase below and defines the fourth kernel, sawyer_prior_rollout_kernel
#ifndef EARL_BRANCH_PRIOR
#define EARL_BRANCH_PRIOR 0
#endif
constexpr bool kBranchPrior = EARL_BRANCH_PRIOR != 0;
static_assert(!kBranchPrior || kBranchDiscount, "the prior kernels are built with the discounted sum");

// Work queue of the time-sliced rollout (earl_sawyer_state.sched: progress[G] then lock[G], zero on entry).  An env group's state is in HBM after every env
// step (the failure guard's "last stable state"), so ANY wave can take the group's next slice of env steps; a wave claims the unlocked group that has come
// LEAST far.  The groups whose envs are in contact -- the slow chains a statically scheduled launch waits for at the end of its second round -- are then
// re-claimed the moment they are released and run without a break from the start, while the fast groups share the other wave slots: the launch tends to
// total work / wave slots instead of (typical wave) + (slowest wave).  Results do not depend on the schedule: an env's arithmetic is its own.
// `home`: where this wave starts looking among groups that have come equally far (its own index in the launch x 2): at the start every group stands at 0, and
// a thousand waves going for group 0 at once would fight over every lock in turn
__device__ __forceinline__ int sched_claim(int32_t* sched, const int G, const int T, const int lane, const int home, int& t0) {
  int32_t* progress = sched;
  int32_t* lock = sched + G;
  for (;;) {
    unsigned long long best = ~0ull;
    for (int gi = lane; gi < G; gi += 64) {
      const int p = __hip_atomic_load(progress + gi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int l = __hip_atomic_load(lock + gi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int rot = gi >= home ? gi - home : gi - home + G;                 // distance from `home`, going up and around
      const unsigned long long key = ((unsigned long long)(unsigned int)p << 32) | (unsigned int)rot;
      best = (l == 0 && p < T && key < best) ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off);
      best = o < best ? o : best;
    }
    if (best == ~0ull) return -1;                       // every unfinished group is in some wave's hands: nothing to do for this one
    const int rot_ = (int)(best & 0xFFFFFFFFull);
    const int gi = rot_ + home < G ? rot_ + home : rot_ + home - G;
    int ok = 0;
    if (lane == 0) ok = atomicCAS(lock + gi, 0, 1) == 0 ? 1 : 0;
    ok = __shfl(ok, 0);
    if (!ok) continue;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the rows the previous holder of this group wrote
    const int p = __hip_atomic_load(progress + gi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= T) {                                       // (finished between the scan and the lock)
      if (lane == 0) __hip_atomic_store(lock + gi, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    t0 = p;
    return gi;
  }
}
__device__ __forceinline__ void sched_release(int32_t* sched, const int G, const int g, const int t1, const int lane) {
  fence();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");     // state rows, output rows, goal rows of this slice -> visible to the next holder
  if (lane == 0) {
    __hip_atomic_store(sched + g, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(sched + G + g, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// metaworld reward_utils.tolerance(x, bounds=(0, hi), margin, sigmoid='gaussian') [UPSTREAM, dm_control semantics; unpinned]
__device__ __forceinline__ double tolerance_gaussian(double x, double hi, double margin) {
#pragma clang fp contract(off)
  if (0.0 <= x && x <= hi) return 1.0;
  if (margin == 0) return 0.0;
  const double d = (x < 0.0 ? -x : x - hi) / margin;
  const double scale = sqrt(-2.0 * log(0.1));
  return exp(-0.5 * (d * scale) * (d * scale));
}

// reward + success of one observation row (sawyer_door.py:141-177)
__device__ __forceinline__ void door_reward(const earl_sawyer_cfg& cfg, const V3 tcp, const V3 obj, const V3 target, double& r, bool& ok, double* info = nullptr) {
#pragma clang fp contract(off)
  const V3 d = vsub(obj, target);
  const double obj_to_target = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);     // np.linalg.norm in f64
  ok = obj_to_target <= cfg.success_radius;
  r = ok ? 1.0 : 0.0;
  if (cfg.reward_type != 0 || info) {
    const V3 e = vsub(tcp, obj);
    const V3 oi = vsub(ld3(cfg.obj_init_pos), target), hi = vsub(ld3(cfg.hand_init_pos), obj);
    const double in_place = tolerance_gaussian(obj_to_target, 0.05, sqrt(oi.x * oi.x + oi.y * oi.y + oi.z * oi.z));
    const double hand_in_place = tolerance_gaussian(sqrt(e.x * e.x + e.y * e.y + e.z * e.z), 0.25 * 0.05, sqrt(hi.x * hi.x + hi.y * hi.y + hi.z * hi.z) + 0.1);
    if (cfg.reward_type != 0) {
      r = 3 * hand_in_place + 6 * in_place;
      if (obj_to_target < 0.05) r = 10;
    }
    if (info) {
      // SawyerDoorV2.evaluate_state (sawyer_door.py:127-139); compute_reward returns [reward, obj_to_target, hand_in_place] (:171), so the dict's
      // 'in_place_reward' is the hand's term
      info[EARL_INFO_SUCCESS] = obj_to_target <= 0.08 ? 1.0 : 0.0;
      info[EARL_INFO_NEAR_OBJECT] = 0.0; info[EARL_INFO_GRASP_SUCCESS] = 1.0; info[EARL_INFO_GRASP_REWARD] = 1.0;
      info[EARL_INFO_IN_PLACE_REWARD] = hand_in_place; info[EARL_INFO_OBJ_TO_TARGET] = obj_to_target; info[EARL_INFO_UNSCALED_REWARD] = r;
      info[7] = 0.0;
    }
  }
}

// ---- metaworld reward_utils / SawyerXYZEnv._gripper_caging_reward [UPSTREAM metaworld, not in the reference tree; UNPINNED]:
// restated as in oracle/sawyer_oracle.py (tolerance_long_tail, rect_prism_tolerance, hamacher_product, gripper_caging_reward)
__device__ __forceinline__ double tol_long_tail(double x, double lo, double hi, double margin) {
#pragma clang fp contract(off)
  if (lo <= x && x <= hi) return 1.0;
  if (margin == 0) return 0.0;
  const double d = (x < lo ? lo - x : x - hi) / margin;
  const double scale = sqrt(1 / 0.1 - 1);
  return 1 / ((d * scale) * (d * scale) + 1);
}
__device__ __forceinline__ bool in_rng(double a, double b, double c) { return c >= b ? (b <= a && a <= c) : (c <= a && a <= b); }
__device__ __forceinline__ double rect_prism_tol(const V3 cur, const double* zero, const double* one) {
#pragma clang fp contract(off)
  if (in_rng(cur.x, zero[0], one[0]) && in_rng(cur.y, zero[1], one[1]) && in_rng(cur.z, zero[2], one[2]))
    return (cur.x - zero[0]) / (one[0] - zero[0]) * ((cur.y - zero[1]) / (one[1] - zero[1])) * ((cur.z - zero[2]) / (one[2] - zero[2]));
  return 1.0;
}
__device__ __forceinline__ double hamacher(double a, double b) {
#pragma clang fp contract(off)
  const double den = a + b - (a * b);
  return den > 0 ? (a * b) / den : 0.0;
}
// SawyerPegV2.compute_reward, reward_type 'dense' (sawyer_peg.py:231-299); head = obs[4:7] (site pegHead), tcp = obs[:3] (hand)
// dense = false: reward_type 'sparse' (sawyer_peg.py:284-285: object_grasped = 0 unless lifted); the terms are still worked out, for the info dict (terms[]:
// tcp_to_obj, obj_to_target (axis-scaled), object_grasped, in_place; may be NULL)
__device__ __forceinline__ double peg_dense_reward(const earl_sawyer_cfg& cfg, const V3 tcp, const double tcp_opened, const V3 head, const V3 grasp,
                                                   const V3 lpad, const V3 rpad, const V3 tcpc, const V3 target, const double* __restrict__ oi,
                                                   const double effort, const bool dense = true, double* terms = nullptr) {
#pragma clang fp contract(off)
  const V3 obj = grasp;                                   // obs[4:7] - pegHead + pegGrasp with obs[4:7] == pegHead
  const V3 e = vsub(obj, tcp);
  const double tcp_to_obj = sqrt(e.x * e.x + e.y * e.y + e.z * e.z);
  const V3 ht{(head.x - target.x) * 1.0, (head.y - target.y) * 2.0, (head.z - target.z) * 2.0};
  const double obj_to_target = sqrt(ht.x * ht.x + ht.y * ht.y + ht.z * ht.z);
  const V3 hi{(oi[3] - target.x) * 1.0, (oi[4] - target.y) * 2.0, (oi[5] - target.z) * 2.0};
  double in_place = tol_long_tail(obj_to_target, 0.0, 0.05, sqrt(hi.x * hi.x + hi.y * hi.y + hi.z * hi.z));
  const double box1 = rect_prism_tol(head, cfg.box_corners[0], cfg.box_corners[1]), box2 = rect_prism_tol(head, cfg.box_corners[2], cfg.box_corners[3]);
  in_place = hamacher(in_place, hamacher(box2, box1));
  const bool lifted = tcp_to_obj < 0.08 && tcp_opened > 0 && obj.z - 0.01 > oi[2];
  double grasped = 1.0;
  if (!lifted && !dense) grasped = 0.0;
  if (!lifted && dense) {
    // _gripper_caging_reward(action, obj, obj_radius 0.0075, pad_success_thresh 0.03, object_reach_radius 0.01, xz_thresh 0.005, high_density)
    const double pl = fabs(lpad.y - obj.y), pr = fabs(rpad.y - obj.y);
    const double ml = fabs(fabs(lpad.y - oi[1]) - 0.03), mr = fabs(fabs(rpad.y - oi[1]) - 0.03);
    const double caging_y = hamacher(tol_long_tail(pl, 0.0075, 0.03, ml), tol_long_tail(pr, 0.0075, 0.03, mr));
    const double ix = oi[0] - cfg.init_tcp[0], iz = oi[2] - cfg.init_tcp[2];
    const double dx = tcpc.x - obj.x, dz = tcpc.z - obj.z;
    const double caging_xz = tol_long_tail(sqrt(dx * dx + dz * dz), 0.0, 0.005, sqrt(ix * ix + iz * iz) - 0.005);
    const double closed = fmin(fmax(0.0, effort), 1.0) / 1.0;
    const double caging = hamacher(caging_y, caging_xz);
    const double gripping = caging > 0.97 ? closed : 0.0;
    grasped = (hamacher(caging, gripping) + caging) / 2;
  }
  double r = hamacher(grasped, in_place);
  if (lifted) r += 1.0 + 5 * in_place;
  if (obj_to_target <= 0.05) r = 10.0;
  if (terms) { terms[0] = tcp_to_obj; terms[1] = obj_to_target; terms[2] = grasped; terms[3] = in_place; }
  return r;
}

// any lane of this env's LPE-lane group (the whole wavefront calls it)

// obs[14] + reward + flags of one env from the kinematics in LDS (sawyer_door.py:86-94, :141-177); the whole group calls it
template <int NV>
__device__ __forceinline__ void sawyer_emit(Shared<NV>& s, const typename ModelOf<NV>::T& m, const earl_sawyer_cfg& cfg, const int sub, const bool live,
                                            const double* __restrict__ goal, double* __restrict__ obs, float* reward, uint8_t* success,
                                            const double* __restrict__ obj_init = nullptr, const double effort = 0.0, double* __restrict__ obs2 = nullptr,
                                            double* __restrict__ info = nullptr) {
#pragma clang fp contract(off)
  // (compiled into the peg model's kernels only: in the door kernel this code cost 35 more AGPR spills and 10 % of its throughput.  The door's info dict is a
  // function of the observation alone: earl_sawyer_door_info works it out from the emitted rows.)
  const bool peg_terms = NV >= 15 && cfg.obj_kind >= 1 && obj_init != nullptr && (cfg.reward_type != 0 || info != nullptr);
  const bool peg_dense = peg_terms && cfg.reward_type != 0;
  if (sub < (peg_terms ? 7 : 4)) {
    const int k = sub == 0 ? cfg.att_hand : (sub == 1 ? cfg.att_right : (sub == 2 ? cfg.att_left : (sub == 3 ? cfg.att_obj :
                  (sub == 4 ? cfg.att_grasp : (sub == 5 ? cfg.att_lpad : cfg.att_rpad)))));
    const V3 p = attachment<NV>(s, m, k);
    s.emit.att[sub][0] = p.x; s.emit.att[sub][1] = p.y; s.emit.att[sub][2] = p.z;
  }
  fence();
  if (sub < 14 && live && (obs || obs2)) {
    double v;
    if (sub < 3) v = s.emit.att[0][sub];
    else if (sub == 3) {
      const V3 d = vsub(ld3(s.emit.att[1]), ld3(s.emit.att[2]));
      v = fmin(fmax(sqrt(d.x * d.x + d.y * d.y + d.z * d.z) / 0.1, 0.0), 1.0);
    } else if (sub < 7) v = s.emit.att[3][sub - 4];
    else v = goal[sub - 7];
    if (obs) obs[sub] = v;
    if (obs2) obs2[sub] = v;
  }
  if (sub == 0 && live) {
    double r; bool ok;
    door_reward(cfg, ld3(s.emit.att[0]), ld3(s.emit.att[3]), ld3(goal + 4), r, ok);
    if constexpr (NV >= 15) if (peg_terms) {
      const V3 rr = ld3(s.emit.att[1]), ll = ld3(s.emit.att[2]), dg = vsub(rr, ll);
      const double opened = fmin(fmax(sqrt(dg.x * dg.x + dg.y * dg.y + dg.z * dg.z) / 0.1, 0.0), 1.0);      // obs[3]
      double terms[4];
      const double rd = peg_dense_reward(cfg, ld3(s.emit.att[0]), opened, ld3(s.emit.att[3]), ld3(s.emit.att[4]), ld3(s.emit.att[5]), ld3(s.emit.att[6]),
                                         scl(add(rr, ll), 0.5), ld3(goal + 4), obj_init, effort, peg_dense, terms);
      if (peg_dense) r = rd;
      if (info) {
        // SawyerPegV2.evaluate_state (sawyer_peg.py:165-184): tcp_to_obj to the pegGrasp site, obj = the observation's pegHead, TARGET_RADIUS 0.05
        const double headz = s.emit.att[3][2];
        info[EARL_INFO_SUCCESS] = terms[1] <= 0.05 ? 1.0 : 0.0;
        info[EARL_INFO_NEAR_OBJECT] = terms[0] <= 0.03 ? 1.0 : 0.0;
        info[EARL_INFO_GRASP_SUCCESS] = (terms[0] < 0.02 && opened > 0 && headz - 0.01 > obj_init[2]) ? 1.0 : 0.0;
        info[EARL_INFO_GRASP_REWARD] = terms[2]; info[EARL_INFO_IN_PLACE_REWARD] = terms[3]; info[EARL_INFO_OBJ_TO_TARGET] = terms[1];
        info[EARL_INFO_UNSCALED_REWARD] = r; info[7] = 0.0;
      }
    }
    if (reward) *reward = (float)r;
    if (success) *success = ok ? 1 : 0;
  }
  fence();
}


// ------------------------------------------------------------------------------------------------ the policy phase of sawyer_policy_rollout_kernel
// A float32 MLP 14 -> H1 (-> H2) -> 4 | 8 evaluated by the 16 lanes of an env between two env steps, under the contract of policy_math.h / tabletop_policy.h.  The layer
// itself -- activations in registers, element k on lane k & 15 in register k >> 4, x_k by a width-16 __shfl, four fmaf chains per lane, weight rows in 16-byte pieces --
// is pol_layer<16, ..> of policy_lane_group.h, shared with the minitaur and the kitchen (32 lanes per env).

// the action of env step t of one env, on all 16 lanes of its group: observation (element `sub` on lane `sub`, 0 beyond 13) -> MLP -> head -> float4.
// `row` = t n + env; a group that is not live computes on zeros and writes nothing.
// The policy's kernel arguments are read HERE, through the kernel-argument pointer the caller passed through an empty asm (the register-pinning recipe of DESIGN 2, on
// scalar registers): read as `a.pol...` they are loaded once at kernel entry and held in some twenty scalar registers across the whole env-step loop -- through substep, where the
// scalar file is full already; the extra scalar spills took vector registers away and the stepper's own constants went to scratch, reloaded inside the timestep loop.
__device__ __noinline__ float4 sawyer_policy_action(const uint64_t ka_bits, const uint64_t ev, const uint32_t gid, const uint64_t seed, const double* __restrict__ seen, const int env,
                                                       const size_t row, const int sub, const bool live) {
#pragma clang fp contract(off)
  const EARL_KARG SawyerPolicyArgs* ka = cl_kernarg<SawyerPolicyArgs>(ka_bits);
  const int n_layers = ka->pol.n_layers, d0 = ka->pol.dims[0], d1 = ka->pol.dims[1], d2 = ka->pol.dims[2], d3 = ka->pol.dims[3];
  const int hidden_act = ka->pol.hidden_act, out_act = ka->pol.out_act;
  if (!seen) seen = ka->obs0 + (size_t)env * 14;       // step 0
  float h[16];
  h[0] = (sub < 14 && live) ? (float)seen[sub] : 0.f;
#pragma unroll
  for (int i = 1; i < 16; ++i) h[i] = 0.f;
  const pol_elem* w = cl_policy_weights(ka, gid, env, row, sub == 0 && live);      // (the member's rows, the network of the pair's phase)
  pol_layer<16, false>(w, w + (size_t)d1 * d0, d0, d1, hidden_act, sub, h);
  w += (size_t)d1 * (d0 + 1);
  if (n_layers == 3) {
    pol_layer<16, true>(w, w + (size_t)d2 * d1, d1, d2, hidden_act, sub, h);
    w += (size_t)d2 * (d1 + 1);
  }
  const int KL = n_layers == 3 ? d2 : d1, NL = n_layers == 3 ? d3 : d2;
  pol_layer<16, true>(w, w + (size_t)NL * KL, KL, NL, EARL_ACT_NONE, sub, h);       // lane j < NL holds output j
  float u;
  if (ka->gauss) {
    // lanes 0..3 are the head's four dimensions: mean on the lane itself, raw log_std four lanes up
    const float raw = __shfl(h[0], (sub & 3) + 4, 16);
    // ONE Philox block per (env, env step), keyed like the goal-switch draw of the same step: ev = the host's step counter plus the clock word of a graph-captured
    // launch, plus t.  The draw index earl::kGaussDraw = 0x504F4C00 keeps the stream disjoint from every other draw made with these counter words: the reset's
    // (indices 0 .. 31, 0xFFF0 .. 0xFFF2, 0xFFFF) and the goal switch's (0xFFFE).  Words x, y, z, w serve action dimensions 0 .. 3.
    const earl::U4 b = earl::philox4x32_10(earl::U4{earl::kGaussDraw, gid, (uint32_t)ev, (uint32_t)(ev >> 32)}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int d = sub & 3;
    const float eps = earl::normal_quantile_f32((d == 0 ? b.x : (d == 1 ? b.y : (d == 2 ? b.z : b.w))) >> 8);
    u = earl::gaussian_head_action(earl_gaussian_head{ka->head.mode, ka->head.log_std_map, ka->head.log_std_min, ka->head.log_std_max, nullptr}, out_act, h[0], raw, eps);
    float* eps_out = ka->head.eps_out;
    if (sub < 4 && live && eps_out) eps_out[row * 4 + sub] = eps;
  } else {
    u = earl::policy_act(h[0], out_act);
  }
  float* act_out = ka->act_out;
  if (sub < 4 && live && act_out) act_out[row * 4 + sub] = u;
  return float4{__shfl(u, 0, 16), __shfl(u, 1, 16), __shfl(u, 2, 16), __shfl(u, 3, 16)};
}

// the action of env step t: given (the plain rollout) or computed here (POLICY).  `A` is the kernel's argument struct
template <bool POLICY, class A>
__device__ __forceinline__ float4 sawyer_step_action(const A& a, const int t, const int n, const int env, const int sub, const bool live) {
  if constexpr (POLICY) {
    // what the policy sees: the row this env emitted last, exactly as it stands in out.obs (a rolled-back step's repeated row, the goal block a goal switch
    // patched), each double rounded to float32; at step 0 the caller's obs0.  Lane `sub` reads the element lane `sub` wrote (sawyer_emit, the rollback and the
    // goal switch all write element `sub` from lane `sub`), so inside a wave's run of env steps this is the lane's own store in program order; the first step of
    // a time slice reads a row another wave wrote, ordered by sched_release's release fence and sched_claim's acquire fence exactly as the qpos / qvel rows are.
    // Without out.obs (earl_sawyer_population_rollout) the env's row of st.last_obs is the one observation row the launch keeps: written, patched and read like the row of out.obs.
    const double* seen = t > 0 ? (a.out.obs ? a.out.obs + ((size_t)(t - 1) * n + env) * 14 : a.st.last_obs + (size_t)env * 14) : nullptr;
    const uint64_t ev = a.cfg.step_counter + (a.clock ? a.clock[1] : 0) + (uint64_t)t;      // (read per step, like the goal switch's: see there)
    // (offset 0 of the kernel-argument segment is the kernel's one argument, the SawyerPolicyArgs: see sawyer_policy_rollout_kernel)
    return sawyer_policy_action((uint64_t)cl_kernarg<SawyerPolicyArgs>(), ev, (uint32_t)(a.cfg.env_offset + env), a.cfg.seed, seen, env, (size_t)t * n + env, sub, live);
  } else {
    return *reinterpret_cast<const float4*>(a.action + ((size_t)t * n + env) * 4);
  }
}

// ------------------------------------------------------------------------------------------------ the pieces of sawyer_branch_rollout_kernel (BRANCH)
// Every SawyerBranchArgs field is read through the kernel-argument segment here, where it is used (policy_closed_loop.h on why): nothing of a branch's bookkeeping
// lives across a timestep.
// the env a virtual env is a branch of: i = v % n_env
__device__ __forceinline__ int sawyer_branch_env(const int v) { return v % cl_kernarg<SawyerBranchArgs>()->n_env; }
// the action of env step t of virtual env v: row (t, i) of branch v / n_env's block
__device__ __forceinline__ float4 sawyer_branch_action(const int t, const int v) {
  const EARL_KARG SawyerBranchArgs* ka = cl_kernarg<SawyerBranchArgs>();
  const int n = ka->n_env, k = v / n, i = v - k * n;
  return *reinterpret_cast<const float4*>(ka->action + (size_t)k * (size_t)ka->act_stride + ((size_t)t * n + i) * 4);
}
// the virtual env's summary and rolled-back steps after env step t, by lane 0 of the live env: cl_episode_summary's three words, each its definition applied to the
// step's reward and success as a rollout would have stored them (a rolled-back step: 0 and 0), and the number of such steps; step 0 initialises all four.
// DISCOUNT (earl_sawyer_branch_rollout_value, discount != 1): ret is the discounted sum of include/earl_physics.h -- term = d_t * r_t; ret = ret + term;
// d_{t+1} = d_t * gamma, three float64 roundings with contraction off (value_accumulate of tabletop_value.h, mirrored), d_0 = 1 and d_{t+1} kept in br_disc[v];
// a rolled-back step adds 0 and still advances d.  gamma and br_disc are read through the kernel-argument segment here, like the other fields
template <bool DISCOUNT>
__device__ __forceinline__ void sawyer_branch_summary(const int t, const int v, const double r_t, const uint8_t s_t, const bool failed) {
  const EARL_KARG SawyerBranchArgs* ka = cl_kernarg<SawyerBranchArgs>();
  double* const ret = ka->br_ret;
  uint8_t* const last = ka->br_last;
  int32_t* const first = ka->br_first;
  int32_t* const fail = ka->br_fail;
  if constexpr (DISCOUNT) {
#pragma clang fp contract(off)
    const EARL_KARG SawyerBranchValueArgs* kv = cl_kernarg<SawyerBranchValueArgs>();
    double* const disc = kv->br_disc;
    if (ret) {
      const double d = t > 0 ? disc[v] : 1.0;
      const double term = d * r_t;
      ret[v] = (t > 0 ? ret[v] : 0.0) + term;
      disc[v] = d * kv->gamma;
    }
  } else
  if (ret) ret[v] = (t > 0 ? ret[v] : 0.0) + r_t;                      // sum over t ascending of (double)reward_t
  if (last) last[v] = s_t;                                             // (the one of step T - 1 stays)
  if (first) {
    const int32_t f = t > 0 ? first[v] : -1;
    first[v] = (f < 0 && s_t) ? t : f;
  }
  if (fail) fail[v] = (t > 0 ? fail[v] : 0) + (failed ? 1 : 0);
}

#ifndef EARL_WAVES_PER_EU
#define EARL_WAVES_PER_EU 1
#endif
// the policy phase and the kernel of the prior branches (the units built with EARL_BRANCH_PRIOR only): a file of their own, which holds the FOURTH inclusion of the rollout body
#if EARL_BRANCH_PRIOR
#include "physics_env_sawyer_prior.inc"
#endif
// SLICED: the launch's work is a queue of (env group, slice of a.slice env steps) items (sched_claim above) taken by persistent waves, instead of one
// whole rollout of one group per wave
template <int NV, int LPE, bool SLICED = false>
__global__ __launch_bounds__(64 * Lim<NV>::WPB, EARL_WAVES_PER_EU) void sawyer_rollout_kernel(const SawyerArgs a) {
  constexpr bool POLICY = false;
  constexpr bool BRANCH = false;
#include "physics_env_sawyer_rollout.inc"
}
// The same rollout with the policy inside (earl_sawyer_policy_rollout): 16 lanes per env only (the policy phase is laid out over an env's 16 lanes)
// `a` must stay the kernel's ONLY argument: the policy phase reads a.pol / a.head / a.gauss / a.obs0 / a.act_out through the kernel-argument segment pointer cast to
// SawyerPolicyArgs* (sawyer_step_action, sawyer_policy_action), which is `a` only while `a` sits at offset 0 of the segment
static_assert(std::is_standard_layout<SawyerArgs>::value && std::is_trivially_copyable<SawyerPolicyArgs>::value, "the policy phase reads SawyerPolicyArgs as laid out in the kernel-argument segment");
template <int NV, int LPE, bool SLICED = false>
__global__ __launch_bounds__(64 * Lim<NV>::WPB, EARL_WAVES_PER_EU) void sawyer_policy_rollout_kernel(const SawyerPolicyArgs a) {
  static_assert(LPE == 16, "the policy phase is laid out over 16 lanes per env");
  constexpr bool POLICY = true;
  constexpr bool BRANCH = false;
#include "physics_env_sawyer_rollout.inc"
}
// The same rollout over the K n virtual envs of a branch launch (earl_sawyer_branch_rollout; instantiated in physics_branch.hip and physics_branch_w8.hip only): every
// action given, no [T] row written, the state rows the workspace's.  `a` must stay the kernel's ONLY argument, as for the policy kernel: the branch's fields are read
// through the kernel-argument segment pointer cast to SawyerBranchArgs*
static_assert(std::is_trivially_copyable<SawyerBranchArgs>::value, "the branch pieces read SawyerBranchArgs as laid out in the kernel-argument segment");
// (under EARL_BRANCH_DISCOUNT the argument is the SawyerBranchValueArgs and sawyer_branch_summary<true> keeps the discounted sum: the same text otherwise)
static_assert(std::is_trivially_copyable<SawyerBranchValueArgs>::value, "the discounted summary reads SawyerBranchValueArgs as laid out in the kernel-argument segment");
template <int NV, int LPE, bool SLICED = false>
__global__ __launch_bounds__(64 * Lim<NV>::WPB, EARL_WAVES_PER_EU) void sawyer_branch_rollout_kernel(const SawyerBranchKernelArgs a) {
  static_assert(LPE == 16, "the branch launch has the 16-lane forms only");
  constexpr bool POLICY = false;
  constexpr bool BRANCH = true;
#include "physics_env_sawyer_rollout.inc"
}

// reset (masked) / observe: both end with the kinematics of the current state and the observation
template <int NV, int LPE>
__global__ __launch_bounds__(64 * Lim<NV>::WPB) void sawyer_reset_kernel(const SawyerArgs a) {
  constexpr int EPW = 64 / LPE, WPB = Lim<NV>::WPB;
  __shared__ alignas(16) typename ModelOf<NV>::T m;
  __shared__ alignas(16) BlkTable<Lim<NV>::MB, Lim<NV>::KBT> bt;
  __shared__ alignas(16) Shared<NV> sh[EPW * WPB];
  stage_blocks(bt, a.col);
  stage_kb<NV>(bt, a.m, a.col);
  stage_model(m, a.m);
  const earl_sawyer_cfg& cfg = a.cfg;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = lane % LPE, grp = lane / LPE;
  const int env_raw = (blockIdx.x * WPB + wave) * EPW + grp;
  const int env = env_raw < cfg.n ? env_raw : cfg.n - 1;
  Shared<NV>& s = sh[wave * EPW + grp];
  const bool resetting = !a.observe_only && env_raw < cfg.n && (!a.mask || a.mask[env]);
  const bool live = env_raw < cfg.n && (a.observe_only || resetting);
  if constexpr (Lim<NV>::TS < Lim<NV>::NT) {            // (the forward pass below reads the whole mass matrix; K5 leaves the entries between the trees alone)
    for (int k = sub; k < (int)(sizeof(s.M.v) / sizeof(double)); k += LPE) s.M.v[k] = 0.0;
  }
  if (sub < 3) s.mocap[sub] = a.st.mocap_pos[(size_t)env * 3 + sub];
  if (resetting) {
    const uint32_t gid = (uint32_t)(cfg.env_offset + env), c0 = (uint32_t)cfg.counter, c1 = (uint32_t)(cfg.counter >> 32);
    const uint32_t k0 = (uint32_t)cfg.seed, k1 = (uint32_t)(cfg.seed >> 32);
    load_state<NV>(s, m, a.reset_qpos, a.reset_qvel, sub);
    fence();
    if (cfg.obj_kind == 0) {
      const earl::U4 b = earl::philox4x32_10(earl::U4{0u, gid, c0, c1}, k0, k1);
      // np.random.uniform(lo, hi) = lo + (hi - lo) * u   (sawyer_door.py:116-118)
      double angle;
      {
#pragma clang fp contract(off)
        angle = cfg.obj_init_angle + (cfg.angle_noise[0] + (cfg.angle_noise[1] - cfg.angle_noise[0]) * earl::u01(b.x, b.y));
      }
      if (sub == cfg.obj_dof) { s.qp[sub] = angle; s.qv[sub] = 0.0; }
    } else {
      // sawyer_peg.py:199-212 / :221-223: xyz ~ U(obj_low, obj_high), redrawn while the xy distance to the hole block is < 0.1;
      // _set_obj_xyz [UPSTREAM]: qpos[9:12] <- xyz, qvel[9:15] <- 0 (the orientation is left as it is)
      double px = 0, py = 0, pz = 0;
      bool wide = false;
      if (cfg.obj_kind == 2 && cfg.n_wide > 0 && cfg.wide_table) {
        // wide_init (sawyer_peg.py:200-209): np.random.uniform() < 0.5 keeps the default draw below; otherwise a row of the wide table
        // (shifted by +0.1 in x: "- np.array([-0.1, 0, 0])") plus U(-0.02, 0.02)^3
#pragma clang fp contract(off)
        const earl::U4 c0_ = earl::philox4x32_10(earl::U4{0xFFF0u, gid, c0, c1}, k0, k1);
        const earl::U4 c1_ = earl::philox4x32_10(earl::U4{0xFFF1u, gid, c0, c1}, k0, k1);
        wide = !(earl::u01(c0_.x, c0_.y) < 0.5);
        int wr = (int)(earl::u01(c0_.z, c0_.w) * (double)cfg.n_wide);
        wr = wr < cfg.n_wide ? wr : cfg.n_wide - 1;
        const double lo = -cfg.wide_noise, hi = cfg.wide_noise;
        px = (cfg.wide_table[wr * 3 + 0] + cfg.wide_shift[0]) + (lo + (hi - lo) * earl::u01(c1_.x, c1_.y));
        py = (cfg.wide_table[wr * 3 + 1] + cfg.wide_shift[1]) + (lo + (hi - lo) * earl::u01(c1_.z, c1_.w));
        const earl::U4 c2_ = earl::philox4x32_10(earl::U4{0xFFF2u, gid, c0, c1}, k0, k1);
        pz = (cfg.wide_table[wr * 3 + 2] + cfg.wide_shift[2]) + (lo + (hi - lo) * earl::u01(c2_.x, c2_.y));
      }
      for (uint32_t attempt = 0; attempt < 16u && !wide; ++attempt) {
#pragma clang fp contract(off)
        const earl::U4 b0 = earl::philox4x32_10(earl::U4{2u * attempt, gid, c0, c1}, k0, k1);
        const earl::U4 b1 = earl::philox4x32_10(earl::U4{2u * attempt + 1u, gid, c0, c1}, k0, k1);
        px = cfg.obj_low[0] + (cfg.obj_high[0] - cfg.obj_low[0]) * earl::u01(b0.x, b0.y);
        py = cfg.obj_low[1] + (cfg.obj_high[1] - cfg.obj_low[1]) * earl::u01(b0.z, b0.w);
        pz = cfg.obj_low[2] + (cfg.obj_high[2] - cfg.obj_low[2]) * earl::u01(b1.x, b1.y);
        const double dx = px - cfg.obj_reject_xy[0], dy = py - cfg.obj_reject_xy[1];
        if (!(sqrt(dx * dx + dy * dy) < cfg.obj_reject_radius)) break;
      }
      const int k = sub - cfg.obj_dof;
      if (k >= 0 && k < 6 && sub < NV) {
        if (k < 3) s.qp[sub] = k == 0 ? px : (k == 1 ? py : pz);
        s.qv[sub] = 0.0;
      }
    }
    if (cfg.n_goal_rows > 0 && cfg.goal_table && sub < 7) {
      // get_next_goal with reset_at_goal (sawyer_peg.py:149-152): np.random.randint(0, rows) -> own Philox draw
      const earl::U4 b = earl::philox4x32_10(earl::U4{0xFFFFu, gid, c0, c1}, k0, k1);
      int row = (int)(earl::u01(b.x, b.y) * (double)cfg.n_goal_rows);
      row = row < cfg.n_goal_rows ? row : cfg.n_goal_rows - 1;
      a.st.goal[(size_t)env * 7 + sub] = cfg.goal_table[(size_t)row * 7 + sub];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");    // the observation below reads the goal row back through global memory
    fence();
    store_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
    if (sub < 3) { s.mocap[sub] = cfg.hand_init_pos[sub]; a.st.mocap_pos[(size_t)env * 3 + sub] = cfg.hand_init_pos[sub]; }
    if (sub == 0 && a.st.steps_since_reset) a.st.steps_since_reset[env] = 0;
    if (sub == 0 && a.st.steps_since_goal_change) a.st.steps_since_goal_change[env] = 0;     // LifelongWrapper.reset (lifelong_wrapper.py:25-28)
  } else {
    load_state<NV>(s, m, a.st.qpos + (size_t)env * m.nq, a.st.qvel + (size_t)env * NV, sub);
  }
  fence();
  const bool keep = resetting && ((cfg.obj_kind >= 1 && a.st.obj_init) || a.st.last_obs);     // uniform enough: decided per lane, used per lane below
  if (!a.reset_obs && !__any(keep)) return;
  // set_state -> sim.forward(): kinematics of the state just written
  const Q4 mq = ldq(cfg.mocap_quat);                     // as given, NOT normalised (include/earl_physics.h)
  const double ctrl[EARL_MAXACT] = {0, 0, 0, 0};
  substep<NV, LPE, false>(s, m, bt, nullptr, sub, grp, mq, ctrl, false, nullptr, nullptr);
  sawyer_emit<NV>(s, m, cfg, sub, live, a.st.goal + (size_t)env * 7, a.reset_obs ? a.reset_obs + (size_t)env * 14 : nullptr, nullptr, nullptr, nullptr, 0.0,
                  (resetting && a.st.last_obs) ? a.st.last_obs + (size_t)env * 14 : nullptr);
  // reset_model keeps obj_init_pos and the pegHead site of the freshly placed peg for the dense reward (sawyer_peg.py:213-215)
  if (resetting && cfg.obj_kind >= 1 && a.st.obj_init && sub < 6) {
    double* oi = a.st.obj_init + (size_t)env * 6;
    oi[sub] = sub < 3 ? s.qp[cfg.obj_dof + sub] : s.emit.att[3][sub - 3];
  }
}

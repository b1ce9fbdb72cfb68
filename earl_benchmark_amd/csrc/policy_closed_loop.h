// policy_closed_loop.h -- what the closed-loop launches of the stepper envs (Sawyer door / peg, minitaur, kitchen) share: the kernel arguments a policy kernel takes
// beyond its plain kernel's (ClosedLoopArgs), the host-side fill of them from the public structs, and the device pieces that are the same code in every env: the
// kernel-argument pointer, the weight rows of an env, the episode-summary update and the agent pair's handover.
// Included inside the anonymous namespace of the stepper units, after policy_math.h and policy_check.h (host) and the stepper (include/earl_physics.h).
#pragma once
#include "policy_lane_group.h"

// The plain kernel's arguments plus the policy: the ONE argument of a policy kernel.  A struct of its own so that the plain kernels' argument -- and machine code --
// stays what it was: new fields go HERE, never into `Plain`.  O = the env's observation width, A its action width, G its goal width.
template <class Plain>
struct ClosedLoopArgs : Plain {
  earl_mlp_policy pol;           // dims[0] = O, dims[n_layers] = A (2 A with the head)
  earl_gaussian_head head;       // read when gauss != 0
  int gauss;
  const double* obs0;            // [n, O]: what the policy sees at step 0
  float* act_out;                // NULL or [T, n, A]: the actions as the policy produced them (the open-loop entry points fed with it walk through the same bits)
  // a population (earl_policy_population)
  int pop_G;                     // envs per member (0: one policy); the env with global id g reads its parameters at pol.params + (g / pop_G) pop_stride
  int64_t pop_stride;            // elements of the stored type between consecutive members (whole 16-byte pieces: a multiple of 4 floats, of 8 bf16 values)
  // earl_episode_summary of the launch, each NULL or [n]: lane 0 of the env keeps its three words up to date in HBM after every env step (step 0 initialises them), so
  // a time slice handed to another wave finds them where it finds qpos
  double* sum_ret;
  uint8_t* sum_last;
  int32_t* sum_first;
  // the forward / reset agent pair (pair_phase == NULL: no pair, and nothing below is read).  The env's phase word travels through HBM like the summary words: lane 0
  // stores it after the handover decision, an agent-scope fence follows, and all lanes of the env read it back where the next action is computed
  int8_t* pair_phase;            // [n] 0 forward, anything else reset; the network of the phase starts at pol.params (+ the member's offset) + phase * pair_stride
  int32_t* pair_sip;             // [n] steps the env has spent in its phase
  int64_t pair_stride;           // elements between the two agents' rows (a multiple of 4 floats, of 8 bf16 values)
  const double* pair_goal;       // NULL or the table [pair_goal_rows, G] of backward goals: entering the reset phase, a drawn row of it becomes the env's st.goal row
  const double* pair_fwd;        // NULL or the table [pair_fwd_rows, G] of forward goals: entering the forward phase, likewise (the kitchen; the Sawyer and the minitaur
                                 // draw from their cfg's goal table and leave this NULL / 0)
  int pair_goal_rows;            // (1 for pair->backward_goal, the table of one row; 0 with pair_goal == NULL)
  int pair_fwd_rows;
  int pair_se[2];                // switch_every
  int pair_sos;                  // switch_on_success
  int8_t* pair_agent;            // NULL or [T, n]
  int32_t* pair_fs;              // NULL or [n]: forward phases that ended by success (step 0 of the launch starts them at 0)
  int32_t* pair_bs;              // NULL or [n]: reset phases that ended by success
  int32_t* pair_row;             // NULL or [n]: earl_backward_goals.row, the table row the env's reset goal came from, stored at every entry into the reset phase
  int32_t* pair_row_out;         // NULL or [T, n]: earl_backward_goals.row_out, the row drawn at env step t, -1 at a step without a draw
};

// host: the fields above from the public structs of one launch (pop, summary, pair, goals, forward_goals: NULL = none; `a`'s Plain part is the caller's)
template <class Plain>
void fill_closed_loop(ClosedLoopArgs<Plain>& a, const earl_mlp_policy& policy, const earl_gaussian_head* head, const double* obs0, float* actions,
                      const earl_policy_population* pop, const earl_episode_summary* summary, const earl_agent_pair* pair, const earl_backward_goals* goals,
                      const double* forward_goals, int32_t n_forward_goals) {
  a.pol = policy;
  a.head = head ? *head : earl::contract::default_head();
  a.gauss = head ? 1 : 0;
  a.obs0 = obs0;
  a.act_out = actions;
  a.pop_G = pop ? pop->envs_per_policy : 0;
  a.pop_stride = pop ? pop->param_stride : 0;
  a.sum_ret = summary ? summary->ret : nullptr;
  a.sum_last = summary ? summary->success_last : nullptr;
  a.sum_first = summary ? summary->first_success : nullptr;
  a.pair_phase = pair ? pair->phase : nullptr;
  a.pair_sip = pair ? pair->steps_in_phase : nullptr;
  a.pair_stride = pair ? pair->param_stride : 0;
  a.pair_goal = !pair ? nullptr : (goals ? goals->table : pair->backward_goal);      // (the ONE fixed row: the table of one row)
  a.pair_goal_rows = !pair ? 0 : (goals ? goals->n_rows : (pair->backward_goal ? 1 : 0));
  a.pair_fwd = pair ? forward_goals : nullptr;
  a.pair_fwd_rows = pair ? n_forward_goals : 0;
  a.pair_se[0] = pair ? pair->switch_every[0] : 0;
  a.pair_se[1] = pair ? pair->switch_every[1] : 0;
  a.pair_sos = pair ? pair->switch_on_success : 0;
  a.pair_agent = pair ? pair->agent_out : nullptr;
  a.pair_fs = pair ? pair->forward_success : nullptr;
  a.pair_bs = pair ? pair->backward_success : nullptr;
  a.pair_row = pair && goals ? goals->row : nullptr;
  a.pair_row_out = pair && goals ? goals->row_out : nullptr;
}

// ------------------------------------------------------------------------------------------------ device: the pieces every env's policy phase is made of
// Every closed-loop field is read through the kernel-argument segment WHERE IT IS USED (`ka->...`), never as `a....`: read as a member of the kernel's argument it is
// loaded once at kernel entry and held in scalar registers across every timestep -- through the stepper, where the scalar file is full already.  Nothing of
// the policy, the summary or the pair lives across a timestep.

// the kernel's own kernel-argument pointer as a pointer to its one argument, the policy struct KA at offset 0 of the segment; passed through an empty asm so that no
// load through it is hoisted out of the env-step loop
template <class KA>
__device__ __forceinline__ const EARL_KARG KA* cl_kernarg() {
  const EARL_KARG void* p = (const EARL_KARG void*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return (const EARL_KARG KA*)p;
}
// ... and inside a called function (where the builtin is null): from the bits the caller handed over, made wave-uniform again so that the reads are scalar loads
template <class KA>
__device__ __forceinline__ const EARL_KARG KA* cl_kernarg(const uint64_t bits) {
  return (const EARL_KARG KA*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bits >> 32)) << 32) |
                               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bits));
}

// the weight rows of env `env` (global id `gid`): a population's member from the GLOBAL id alone (a wave whose envs belong to two members walks two sets of rows:
// correct, only slower); an agent pair's network of the env's phase, the word lane 0 stored after the last handover decision (a group that is not live reads the word of
// the env it shadows).  `lane0`: lane 0 of a live env, which leaves the phase in pair_agent[row].  Both strides count elements of the stored type (pol_elem)
template <class KA>
__device__ __forceinline__ const pol_elem* cl_policy_weights(const EARL_KARG KA* ka, const uint32_t gid, const int env, const size_t row, const bool lane0) {
#ifdef EARL_POLICY_BF16
  const pol_elem* w = reinterpret_cast<const pol_elem*>(ka->pol.params);      // (precision == EARL_PRECISION_BF16: the field keeps its type, the elements are 2 bytes)
#else
  const float* w = ka->pol.params;
#endif
  const int pop_G = ka->pop_G;
  if (pop_G > 0) w += (size_t)(gid / (uint32_t)pop_G) * (size_t)ka->pop_stride;
  const int8_t* pair_phase = ka->pair_phase;
  if (pair_phase) {
    const int ph = pair_phase[env] != 0 ? 1 : 0;
    if (ph) w += (size_t)ka->pair_stride;
    int8_t* agent_out = ka->pair_agent;
    if (lane0 && agent_out) agent_out[row] = (int8_t)ph;
  }
  return w;
}

// the env's episode summary after env step t, by lane 0 of the live env: each word is its definition applied to the step's reward and success as stored in their rows
// (a rolled-back step: 0 and 0)
template <class KA>
__device__ __forceinline__ void cl_episode_summary(const EARL_KARG KA* ka, const int t, const int env, const double r_t, const uint8_t s_t) {
  double* const sum_ret = ka->sum_ret;
  uint8_t* const sum_last = ka->sum_last;
  int32_t* const sum_first = ka->sum_first;
  if (sum_ret) sum_ret[env] = (t > 0 ? sum_ret[env] : 0.0) + r_t;      // sum over t ascending of (double)reward_t
  if (sum_last) sum_last[env] = s_t;                                   // (the one of step T - 1 stays)
  if (sum_first) {
    const int32_t f = t > 0 ? sum_first[env] : -1;
    sum_first[env] = (f < 0 && s_t) ? t : f;
  }
}

// The pair's state machine after env step t (include/earl_physics.h, earl_*_agents_rollout, item 5), the decision: worked out by all lanes of the env from the same
// words -- `success`, the step's success flag of a step that was not rolled back, as lane 0 of the env has it (the caller shuffles); phase and steps_in_phase from HBM.
// -> is the phase over; `ph` / `sip`: phase and steps_in_phase as they stand after this step, which the caller's lane 0 stores again.  `lane0` counts the phases that
// ended by success.  Call with ka->pair_phase != NULL only
template <class KA>
__device__ __forceinline__ bool cl_pair_decide(const EARL_KARG KA* ka, const int t, const int env, const bool lane0, const bool success, int& ph, int& sip) {
  const bool by_s = ka->pair_sos != 0 && success;
  ph = ka->pair_phase[env] != 0 ? 1 : 0;
  sip = ka->pair_sip[env] + 1;                             // (a rolled-back step counts, with success 0)
  const bool over = by_s || sip >= (ph ? ka->pair_se[1] : ka->pair_se[0]);
  if (lane0) {
    int32_t* const fs = ka->pair_fs;
    int32_t* const bs = ka->pair_bs;
    if (fs) fs[env] = (t > 0 ? fs[env] : 0) + ((by_s && ph == 0) ? 1 : 0);      // (a step where the clock ran out as well counts as ended by success)
    if (bs) bs[env] = (t > 0 ? bs[env] : 0) + ((by_s && ph != 0) ? 1 : 0);
  }
  if (over) { ph ^= 1; sip = 0; }
  return over;
}

// ... and the whole handover of the envs whose draw is the pair's own (minitaur, kitchen; the Sawyer merges its draw with the lifelong switch's: see its rollout body).
// Entering the reset phase: a row of the backward table, if there is one (draw index 0xFFFD); entering the forward phase: a row of `fwd` [fwd_rows, G] (0xFFFE, the
// lifelong switch's index).  Counter words {index, gid, ev}, ev = counter + the launch's clock word (*clock, NULL = 0) + t, key `seed`; u01 and clamp as every goal
// draw's.  `store(table, gi)`: the env makes row gi of `table` its goal (all lanes of the env call it).  row / row_out: -1 at every step of a live env, the drawn row on a
// step that enters the reset phase.  Lane 0 stores phase and steps_in_phase last
template <class KA, class Store>
__device__ __forceinline__ void cl_pair_handover(const EARL_KARG KA* ka, const int t, const int env, const size_t row, const bool lane0, const bool success, const uint32_t gid,
                                                 const uint64_t seed, const uint64_t counter, const uint64_t* clock, const double* fwd, const int fwd_rows, Store store) {
#pragma clang fp contract(off)
  int8_t* const pair_phase = ka->pair_phase;
  if (!pair_phase) return;                               // (wave-uniform)
  int ph, sip;
  const bool over = cl_pair_decide(ka, t, env, lane0, success, ph, sip);
  int32_t* const row_at = ka->pair_row_out;
  if (lane0 && row_at) row_at[row] = -1;                 // overwritten below by the same lane on a step that draws
  if (over) {
    const double* const table = ph ? ka->pair_goal : fwd;
    if (table) {
      const int rows = ph ? ka->pair_goal_rows : fwd_rows;
      const uint64_t ev = counter + (clock ? *clock : 0) + (uint64_t)t;
      const earl::U4 b = earl::philox4x32_10(earl::U4{ph ? 0xFFFDu : 0xFFFEu, gid, (uint32_t)ev, (uint32_t)(ev >> 32)}, (uint32_t)seed, (uint32_t)(seed >> 32));
      int gi = (int)(earl::u01(b.x, b.y) * (double)rows);
      gi = gi < rows ? gi : rows - 1;
      store(table, gi);
      if (lane0 && ph) {
        int32_t* const row_of = ka->pair_row;
        if (row_of) row_of[env] = gi;
        if (row_at) row_at[row] = gi;
      }
    }
  }
  if (lane0) { pair_phase[env] = (int8_t)ph; ka->pair_sip[env] = sip; }
}

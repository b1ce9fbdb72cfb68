/* earl_tabletop.h -- C ABI of the MI355X-native tabletop_manipulation step()/reset() hot path.
 *
 * The reference (architsharma97/earl_benchmark) has NO FFI for this path: the env is an ordinary
 * Python object.  Each entry point below therefore cites the Python call it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) owned by the caller; the library allocates nothing,
 *     never synchronises, and enqueues on the caller's HIP stream (earl_stream_t == hipStream_t);
 *   - one row per env; a "shard" is a contiguous range of `n` envs whose global ids are
 *     env_offset .. env_offset+n-1 (RNG streams are keyed by the GLOBAL id, so results do not
 *     depend on how envs are sharded over GPUs);
 *   - functions return EARL_OK (0) or a negative EARL_ERR_* code; they never throw.
 *     earl_last_error() returns a thread-local message for the last failure;
 *   - distinct state buffers may be driven concurrently from different threads/streams.
 *
 * Numerics (tested bit-exact against oracle/ and the golden vectors in tests/golden/):
 *   state is fp64, observations are the fp32 rounding of the state, discrete outputs (attached
 *   flag, done, success, sparse reward) are bit-exact, the dense reward is within 1e-6 relative.
 */
#ifndef EARL_TABLETOP_H
#define EARL_TABLETOP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* earl_stream_t; /* a hipStream_t; NULL = the default stream */

enum { EARL_OK = 0, EARL_ERR_ARG = -1, EARL_ERR_LAUNCH = -2, EARL_ERR_NODEVICE = -3 };
enum { EARL_REWARD_SPARSE = 0, EARL_REWARD_DENSE = 1 };

#define EARL_TABLETOP_OBS_DIM 12  /* qpos[4], attached flag x2, goal[6]: tabletop_manipulation.py:55-60 */
#define EARL_TABLETOP_ACT_DIM 3   /* dx, dy, grip:                     tabletop_manipulation.py:128-132 */
#define EARL_TABLETOP3_OBS_DIM 20 /* qpos[8], flag x2, goal[10]:       tabletop_manipulation_3obj.py:45-50 */

/* Static configuration of one batched env (constructor arguments of the reference's classes). */
typedef struct earl_tabletop_cfg {
  int32_t n;             /* envs in this shard */
  int32_t env_offset;    /* global id of row 0 */
  int32_t reward_type;   /* EARL_REWARD_*:      TabletopManipulation(reward_type=...)  tabletop_manipulation.py:26 */
  int32_t wide_init;     /* wide_init_distr: object-only success test (:201-202) + rejection-sampled reset (:114-117) */
  int32_t reset_at_goal; /* reset_at_goal (:109-111) */
  int32_t horizon;       /* PersistentStateWrapper(episode_horizon)  wrappers/persistent_state_wrapper.py:10-13 */
  int32_t goal_change_frequency; /* LifelongWrapper(goal_change_frequency), 0 = not lifelong  wrappers/lifelong_wrapper.py:18-23 */
  int32_t auto_reset;    /* batched-only extension: 1 = an env whose done fired is reset in the same launch
                            (outputs of that step are still the terminal ones); 0 = reference behaviour */
  int32_t n_goals;       /* rows of state.goal_table */
  int32_t n_sample_goals;/* get_next_goal() draws uniformly from rows 0..n_sample_goals-1 (:62-76; 4 tasks) */
  uint64_t seed;         /* Philox4x32-10 key */
  uint64_t counter;      /* Philox counter word: the caller passes a fresh value on every call that may draw */
} earl_tabletop_cfg;

/* Persistent per-env state (all arrays have cfg.n rows). */
typedef struct earl_tabletop_state {
  double* qpos;                     /* [n,4] gripper x,y then mug x,y  (sim.data.qpos[:4], fp64 like MuJoCo) */
  int8_t* attached;                 /* [n]  -1 free, 0 holding the mug (attached_object, :42) */
  int32_t* goal_idx;                /* [n]  row of goal_table currently set as self.goal */
  const double* goal_table;         /* [n_goals,6] rows 0..3 = goal_states-derived goals (:12-16, :62-76); the
                                       caller may append rows for reset_goal(goal) with arbitrary goals (:78-81) */
  int32_t* steps_since_reset;       /* [n]  PersistentStateWrapper._steps_since_reset */
  int32_t* num_interventions;       /* [n]  PersistentStateWrapper._num_interventions */
  int32_t* steps_since_goal_change; /* [n]  LifelongWrapper, may be NULL when goal_change_frequency == 0 */
  double* lifelong_return;          /* [n]  LifelongWrapper._lifelong_return, may be NULL likewise */
  const uint64_t* counter_base;     /* may be NULL.  Device word ADDED to cfg.counter by earl_tabletop_step / earl_tabletop3_step (only): the Philox counter of a
                                       step launch captured into a HIP graph is a kernel argument frozen at capture time; with the base in device memory the
                                       captured launch of step t (cfg.counter = t) draws with base + t, and the host refreshes the one word before each replay
                                       -- lifelong goal switching and auto-reset inside a captured step loop (envs/tabletop.py StepGraph) */
} earl_tabletop_state;

/* Outputs of one step (rows = envs) or of one rollout (rows = [T, n]). */
typedef struct earl_tabletop_out {
  float* obs;       /* [.., 12] */
  float* reward;    /* [..] */
  uint8_t* done;    /* [..] 0/1: horizon reached (the env itself never terminates, :137) */
  uint8_t* success; /* [..] 0/1: is_successful(next_obs) (:197-204) */
  double* reward_f64; /* [n] may be NULL; written by earl_tabletop_step / earl_tabletop3_step only: the reward before it is rounded to
                         float32 (the reference's compute_reward returns a Python float under its pinned numpy 1.22, :176-191) */
} earl_tabletop_out;

/* Lifelong(PersistentStateWrapper(TabletopManipulation)).step(action) for every env of the shard.
 * Replaces: TabletopManipulation.step/move/_get_obs/compute_reward/is_successful
 *           (envs/tabletop_manipulation.py:128-204), PersistentStateWrapper.step
 *           (wrappers/persistent_state_wrapper.py:22-31), LifelongWrapper.step
 *           (wrappers/lifelong_wrapper.py:30-44).
 * act [n,3] fp32.  next_goal_idx: NULL, or [n] goal rows to use instead of the RNG whenever this call
 * resamples a goal (lifelong switch / auto-reset) -- the injection hook parity tests use, like
 * reset_goal(goal) in the reference. */
int earl_tabletop_step(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const float* act,
                       const int32_t* next_goal_idx, const earl_tabletop_out* out, earl_stream_t stream);

/* T consecutive steps in ONE launch: state stays in registers, act [T,n,3], outputs [T,n,..].
 * Equivalent to T calls of earl_tabletop_step with counter, counter+1, ... (bit-identical outputs). */
int earl_tabletop_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T,
                          const float* act, const earl_tabletop_out* out, earl_stream_t stream);

/* One evaluation episode per env in ONE launch: earl_tabletop_reset (all envs, Philox counter cfg->counter) followed by
 * earl_tabletop_rollout of T steps (counters cfg->counter + 1 ...).  Bit-identical to the two calls; the caller advances
 * its counter by T + 1.  (With lifelong switching / auto-reset enabled it is executed as the two launches.) */
int earl_tabletop_reset_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T,
                                const float* act, const earl_tabletop_out* out, earl_stream_t stream);

/* `episodes` evaluation episodes per env, back to back: episode e = earl_tabletop_reset_rollout with Philox counter
 * cfg->counter + e * (T + 1), its outputs at rows [e, T, n, ..] of `out` (obs [episodes, T, n, 12], ...), its actions at
 * act + e * act_episode_stride floats (act_episode_stride = T * n * 3: a contiguous [episodes, T, n, 3] array; 0: every episode replays
 * the same [T, n, 3] actions).  Bit-identical to that sequence of calls; the caller advances its counter by episodes * (T + 1).
 * This is the reference's evaluation loop (`for _ in range(num_eval_episodes): obs = env.reset(); while not done: env.step(...)`
 * over PersistentStateWrapper, persistent_state_wrapper.py:17-31) for the whole batch.  When the wave-specialised kernel applies
 * (no lifelong switching / auto-reset, all four outputs, T a multiple of 8) ALL episodes run in ONE launch: the launch's fixed cost
 * (prologue, pipeline fill and drain) is paid once instead of once per episode.  The episodes being independent of one another (each starts
 * with the reset), a batch that leaves CUs idle (up to 8192 envs) has several of them IN FLIGHT at a time, each group of episodes on its own
 * workgroups; outputs and the state left behind are those of the sequence, bit for bit. */
int earl_tabletop_eval_episodes(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T, const float* act,
                                int64_t act_episode_stride, const earl_tabletop_out* out, earl_stream_t stream);

/* ---- closed loop: an MLP policy evaluated INSIDE the rollout kernel ----
 * The reference's evaluation / training loop is closed (`obs = env.reset(); while not done: obs, ... = env.step(policy(obs))`); the entry points above
 * need every action up front.  This one takes the policy instead: a float32 MLP 12 -> hidden (-> hidden) -> 3, evaluated on gfx950 with
 * v_mfma_f32_16x16x4_f32 next to the fp64 recurrence, weights resident in registers for the whole launch.
 *
 * THE ARGUMENT CONTRACT of every closed-loop entry point -- the four of this header, and earl_physics.h's earl_sawyer_policy_rollout, earl_sawyer_population_rollout,
 * earl_sawyer_pair_rollout, earl_minitaur_policy_rollout, earl_minitaur_population_rollout, earl_kitchen_policy_rollout and earl_kitchen_population_rollout -- is one set of rules (csrc/policy_check.h states them once; tests/test_policy_contract.py holds every
 * entry point to them).  Each returns EARL_ERR_ARG before any HIP call for
 *   policy      NULL params; precision != 0 (the stepper envs of earl_physics.h: neither 0 nor EARL_PRECISION_BF16; with bf16: params not 16-byte aligned, a
 *               param_stride -- counted in elements of the stored type everywhere -- that is not a multiple of 8 or lies below the parameter count); n_layers not 2 or 3; dims[0] != the env's observation width; dims[n_layers] != the env's action width (head == NULL) or
 *               twice it (head given); a hidden width that is not a multiple of 16 in 16..256; dims[3] != 0 with two layers; hidden_act not EARL_ACT_RELU / _TANH;
 *               out_act not EARL_ACT_NONE / _TANH
 *   head        mode not EARL_HEAD_MEAN / _SAMPLE; log_std_map not EARL_LOGSTD_CLAMP / _TANH; bounds that are not finite, min <= max and inside [-20, 4]
 *   population  P < 1; G < 16 or G % 16 != 0; param_stride below the parameter count of one policy (the sum of dims[l+1] (dims[l] + 1)); cfg->env_offset < 0;
 *               (env_offset + n - 1) / G >= P
 *   pair        NULL pair / phase / steps_in_phase; switch_every[k] < 1; switch_on_success not 0 or 1; param_stride below the parameter count;
 *               cfg->goal_change_frequency > 0 (the pair IS the lifelong mechanism: the two clocks would fight over the same draw)
 * with the widths 12 / 3 here (20 / 3 for earl_tabletop3_policy_rollout), 14 / 4 for the Sawyer door and peg, 32 / 8 for the minitaur, 46 / 9 for the kitchen.  The differences are three, each listed with its entry point: the stepper
 * units read the weight rows in 16-byte pieces (params 16-byte aligned, param_stride % 4 == 0), the minitaur takes bounded policies only (out_act == EARL_ACT_TANH),
 * and this header's pair holds two weight sets in registers (EARL_PAIR_MAX_H2). */
enum { EARL_ACT_NONE = 0, EARL_ACT_RELU = 1, EARL_ACT_TANH = 2 };
/* earl_mlp_policy.precision: the STORED format of the parameters, named by its bits.  bf16 is a storage format only: a stored value u is the float32 whose bit
 * pattern is (uint32_t)u << 16 (subnormals, +-0 and +-inf as they are) and enters the same fmaf chain in the same order, so a launch is bit-identical to the fp32
 * launch fed with the widened values.  Taken by the closed-loop entry points of the door, the peg, the minitaur and the kitchen and by earl_mlp_policy_forward_cpu
 * (earl_physics.h); every entry point of this header refuses it (the tabletop's weights sit in registers for the whole launch). */
#define EARL_PRECISION_BF16 16
typedef struct earl_mlp_policy {
  int32_t n_layers;     /* linear layers: 2 (one hidden) or 3 (two hidden) */
  int32_t dims[4];      /* dims[0] = 12 (the 3-object variant: 20), dims[n_layers] = 3 (6 with a Gaussian head, below); hidden widths multiples of 16 in 16..256; unused = 0 */
  int32_t hidden_act;   /* EARL_ACT_RELU or EARL_ACT_TANH */
  int32_t out_act;      /* EARL_ACT_NONE (the env clips to [-1, 1] itself, tabletop_manipulation.py:130) or EARL_ACT_TANH */
  int32_t precision;    /* 0 = fp32; EARL_PRECISION_BF16 where an entry point says so (earl_physics.h); anything else is EARL_ERR_ARG */
  const float* params;  /* layer by layer: W_l [dims[l+1], dims[l]] row-major (= torch.nn.Linear.weight), then b_l [dims[l+1]].  precision ==
                           EARL_PRECISION_BF16: the same order in uint16_t bf16 values, biases too (the field keeps its type, the caller casts), 16-byte aligned */
} earl_mlp_policy;

/* reset (reset_first = 1) + T closed-loop steps, `episodes` times, in ONE launch.  Step t's action is pi(o), o the float32 observation the env last
 * produced: the reset's observation (reset_first = 1) or _get_obs() of the incoming state (reset_first = 0; episodes must be 1) for t = 0, otherwise row
 * t - 1 of out->obs (after a lifelong goal switch: the re-read row).  act_out (may be NULL) [episodes, T, n, 3] receives the actions as the policy
 * produced them, before the env's own clip / rescale.  out as for earl_tabletop_eval_episodes ([episodes, T, n, ..]); any of its pointers may be NULL.
 * Bit-identical to the open-loop entry point fed with act_out: reset_first = 1 == earl_tabletop_eval_episodes(cfg, st, episodes, T, act_out, T*n*3, out),
 * reset_first = 0 == earl_tabletop_rollout(cfg, st, T, act_out, out) -- outputs, state left behind, wrapper counters, Philox counter use
 * (episodes * (T + 1) resp. T).
 * Policy arithmetic (a contract: libearl_host.so states it as plain loops and the device agrees bit for bit): every pre-activation is
 * acc = b_j; for k ascending: acc = fmaf(x_k, W_jk, acc) in float32; ReLU is acc > 0 ? acc : +0 (= fmaxf(acc, 0) with -0 -> +0, NaN -> 0);
 * tanh is this build's own tanh_f32 (csrc/policy_math.h: fma, +, *, / and integer operations only, no libm). */
int earl_tabletop_policy_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, int32_t episodes, int32_t T,
                                 int32_t reset_first, const earl_tabletop_out* out, float* act_out, earl_stream_t stream);

/* ---- closed loop with exploration: a tanh-Gaussian head sampled INSIDE the rollout kernel ----
 * The reference's training loops collect every transition with a stochastic actor (`action = agent.act(obs, sample=True); obs, ... = env.step(action)` around
 * envs/tabletop_manipulation.py:128-138; the actor is the user's SAC-style network, not the reference's): mean and log_std from one Linear(H, 6), chunked,
 * action = tanh(mean + exp(log_std) eps).  Evaluation runs the same actor at its mean. */
enum { EARL_HEAD_MEAN = 0, EARL_HEAD_SAMPLE = 1 };
enum { EARL_LOGSTD_CLAMP = 0, EARL_LOGSTD_TANH = 1 };
typedef struct earl_gaussian_head {
  int32_t mode;          /* EARL_HEAD_MEAN: u = mean.  EARL_HEAD_SAMPLE: u = fmaf(sigma, eps, mean), sigma = exp_f32(ls) */
  int32_t log_std_map;   /* CLAMP: ls = min(max(raw, lo), hi).  TANH: ls = lo + 0.5 (hi - lo) (tanh_f32(raw) + 1)  (the pytorch_sac / DrQ actor) */
  float log_std_min;     /* lo and hi: finite, min <= max, inside [-20, 4] */
  float log_std_max;
  float* eps_out;        /* may be NULL: [episodes, T, n, 3] the standard-normal draws as used (written in both modes) */
} earl_gaussian_head;

/* earl_tabletop_policy_rollout with a Gaussian head: `policy` is the same struct with dims[n_layers] == 6 -- output rows 0..2 are the mean, rows 3..5 the raw
 * log_std, no activation on either; policy->out_act is applied to u (EARL_ACT_TANH: SAC's squashing; EARL_ACT_NONE leaves the clip to the env) and act_out
 * receives out_act(u).  This replaces the closed loop of the reference's training scripts (agent.act(obs, sample=True) between env.step calls,
 * envs/tabletop_manipulation.py:128-138) in SAMPLE mode and of its evaluation scripts (sample=False) in MEAN mode, for the whole batch in ONE launch.
 * eps: one Philox4x32-10 block per (env, step), key = cfg->seed, counter words {0x504F4C00, env_offset + env, counter lo, counter hi} with the counter of that env
 * step; words x, y, z -> dimensions 0, 1, 2; k = word >> 8, u = (k + 0.5) 2^-24, eps = Phi^-1(u) within 5 float32 ulp (csrc/policy_math.h states the
 * arithmetic).  The draws depend on (seed, global env id, counter) only: not on n, the shard split, episodes or mode, and they take no counter values of
 * their own -- everything earl_tabletop_policy_rollout promises carries over: reset_first / episodes rules, NULL-able outputs, argument errors before any HIP
 * call, Philox counter use (episodes * (T + 1) resp. T), and the launch is bit-identical to earl_tabletop_eval_episodes / earl_tabletop_rollout fed with
 * act_out.  EARL_HEAD_MEAN is bit-identical to earl_tabletop_policy_rollout on the 3-output policy made of rows 0..2 of the last layer. */
int earl_tabletop_policy_rollout_gaussian(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                          const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out,
                                          float* act_out, earl_stream_t stream);

/* ---- closed loop for a POPULATION of policies, with per-episode summaries ----
 * The EARL protocol evaluates many checkpoints and seeds of one agent, evolution strategies and population-based training evaluate hundreds of perturbed copies
 * of one network, and both mostly want one return and one success flag per episode (`for _ in range(num_eval_episodes): ...; returns.append(sum(rewards))`
 * around envs/tabletop_manipulation.py:128-138).  One launch serves all members: every workgroup of the kernel is 16 envs and loads its weights once, so it can
 * load its OWN member's.  All members share one earl_mlp_policy (dims, activations, precision = 0) and one earl_gaussian_head; only the parameters differ. */
typedef struct earl_policy_population {
  int32_t n_policies;        /* P >= 1 */
  int32_t envs_per_policy;   /* G: a multiple of 16, >= 16.  The env with GLOBAL id g = cfg->env_offset + i runs policy g / G */
  int64_t param_stride;      /* floats between consecutive policies in policy->params ([P, param_stride]); >= the parameter count of one policy */
} earl_policy_population;

typedef struct earl_episode_summary {   /* every pointer may be NULL; rows [episodes, n] */
  double*  ret;            /* sum over t ascending of (double)reward_t, reward_t the float32 value out->reward gets */
  uint8_t* success_last;   /* success of step T-1 */
  int32_t* first_success;  /* smallest t with success, -1 if none */
} earl_episode_summary;

/* earl_tabletop_policy_rollout (head == NULL: policy->dims[n_layers] == 3) or earl_tabletop_policy_rollout_gaussian (head != NULL: == 6) with
 *   pop      NULL = one policy, as those two; otherwise member g / G of policy->params for the env with global id g.  The member of an env depends on its
 *            global id only -- not on n or on how the batch is sharded; env_offset need not be a multiple of 16 or of G.  The launch is bit-identical to
 *            cutting the shard at the global ids that are multiples of G and calling the single-policy entry point on each piece (env_offset = its first
 *            global id, n = its length, the matching state rows) with that member's parameters: outputs, act_out, eps_out, state left behind, wrapper
 *            counters, Philox counter use.  With pop == NULL it is bit-identical to the single-policy entry point of the same head.
 *   summary  NULL, or per-episode reductions kept in registers over the T steps and stored once per episode: each array equals its definition applied to
 *            this launch's own out->reward / out->success, exactly, whether or not out's pointers / act_out are given (evaluation without any [T] array).
 * Everything else as the two single-policy entry points: reset_first / episodes rules, every `out` pointer / act_out / eps_out may be NULL (`out` itself
 * may not), Philox counter use episodes * (T + 1) resp. T, the Gaussian draw contract (seed, global env id, counter), lifelong switching and auto-reset,
 * argument errors before any HIP call: the contract's policy, head and (with pop) population rules.  Single-object env (the 3-object variant's is
 * earl_tabletop3_policy_rollout, below). */
int earl_tabletop_population_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                     const earl_policy_population* pop, const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                     const earl_tabletop_out* out, float* act_out, const earl_episode_summary* summary, earl_stream_t stream);

/* ---- closed loop for the AGENT PAIR of autonomous RL: a forward and a reset agent alternating inside one rollout ----
 * EARL's training stream is non-episodic: a forward agent works on the task goal, a reset (backward) agent brings the env back towards the initial state, and
 * they hand the env to each other after a fixed number of steps or as soon as the acting agent has succeeded.  Both agents share one earl_mlp_policy (dims,
 * activations) and one earl_gaussian_head; only the parameters differ: policy->params is [2, param_stride], row 0 the forward agent, row 1 the reset agent. */
typedef struct earl_agent_pair {
  int32_t switch_every[2];     /* steps after which agent 0 (forward) / agent 1 (reset) hands over; each >= 1 */
  int32_t switch_on_success;   /* 1 = also hand over after a step whose success flag is set; 0 = the clocks only */
  int32_t pad_;                /* unused (keeps param_stride 8-byte aligned in every compiler's layout) */
  int64_t param_stride;        /* floats between the two rows of policy->params; >= the parameter count of one policy */
  const double* backward_goal; /* NULL, or ONE goal row (6 doubles, goal-table format; the 3-object variant: 10) the reset agent is conditioned on */
  int8_t*  phase;              /* [n] caller-owned state: 0 forward, 1 reset */
  int32_t* steps_in_phase;     /* [n] caller-owned state: steps the env has spent in its phase */
  int8_t*  agent_out;          /* NULL or [episodes, T, n]: the agent that computed the action of step t */
  int32_t* forward_success;    /* NULL or [episodes, n]: forward phases of the episode that ended by success */
  int32_t* backward_success;   /* NULL or [episodes, n]: reset phases of the episode that ended by success */
} earl_agent_pair;

/* earl_tabletop_policy_rollout (head == NULL: policy->dims[n_layers] == 3) or earl_tabletop_policy_rollout_gaussian (head != NULL: == 6) with two agents.
 * Per env and step, in this order (the order is the contract; libearl_host.so states it as plain loops and the device agrees bit for bit under the sparse reward):
 *   1. the action is computed from the current observation by the network of the env's current `phase`: the same k-ascending fmaf chain, tanh_f32 and head
 *      as the single-policy entry points;
 *   2. with a head, the step's one Philox draw is the one earl_tabletop_policy_rollout_gaussian makes (seed, global env id, counter): it does not depend on
 *      the phase;
 *   3. agent_out and act_out are written;
 *   4. the wrapped env step runs; reward and success refer to the goal in force during the step;
 *   5. if the step auto-reset the env (cfg->auto_reset): phase = 0, steps_in_phase = 0, nothing else; the next action is computed from the observation the
 *      single-policy entry points hand on;
 *   6. otherwise steps_in_phase += 1, and the env hands over if (switch_on_success && success) || steps_in_phase >= switch_every[phase]:
 *      phase ^= 1, steps_in_phase = 0; forward_success / backward_success of the phase that ended is incremented if switch_on_success && success (a step
 *      where the clock ran out as well counts as ended by success).  Entering the reset phase with backward_goal != NULL, the goal in force becomes that
 *      row; state.goal_idx is NOT changed -- the env's stored goal stays a task goal, and every other entry point keeps working on the state a pair launch
 *      leaves behind.  Entering the forward phase, goal_idx = the draw the lifelong switch makes (Philox counter of this step, draw 0) and the goal in force
 *      becomes that table row.  The observation's goal slots are re-read with the goal in force, and the out->obs row carries them.
 * Launch entry: an env in the reset phase with backward_goal != NULL starts from that row, not from goal_table[goal_idx].  reset_first = 1 sets phase = 0,
 * steps_in_phase = 0 at each episode's reset.  Launch exit: phase, steps_in_phase and goal_idx are stored.
 * Never switching (switch_every > T, switch_on_success = 0, all envs in phase 0) the launch is bit-identical to the single-policy entry point of the same
 * head on row 0.  Everything else as those entry points: reset_first / episodes rules, NULL-able outputs / act_out / eps_out, Philox counter use
 * episodes * (T + 1) resp. T, argument errors before any HIP call: the contract's policy, head and pair rules, and this entry point's own: a second hidden layer
 * wider than EARL_PAIR_MAX_H2 (two weight sets share the registers of one wave per SIMD; one hidden layer may have every legal width).  This entry point is the single-object env's;
 * the 3-object variant's is earl_tabletop3_pair_rollout, below. */
#define EARL_PAIR_MAX_H2 128
int earl_tabletop_pair_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                               const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out,
                               earl_stream_t stream);

/* PersistentStateWrapper.reset() + TabletopManipulation.reset() for the envs with mask[i] != 0
 * (mask == NULL: all).  Replaces wrappers/persistent_state_wrapper.py:17-20 and
 * envs/tabletop_manipulation.py:105-126 (incl. is_valid_init :89-97, get_next_goal :62-76).
 * obs (may be NULL): [n,12] current observation of EVERY env after the reset. */
int earl_tabletop_reset(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const uint8_t* mask,
                        const int32_t* next_goal_idx, float* obs, earl_stream_t stream);

/* _get_obs() / is_successful() / compute_reward(_get_obs()) of the current state; any output may be NULL. */
int earl_tabletop_observe(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st,
                          const earl_tabletop_out* out, earl_stream_t stream);

/* compute_reward(obs) and is_successful(obs) on caller-supplied observations obs [n,12]
 * (envs/tabletop_manipulation.py:176-204).  reward / success may be NULL. */
int earl_tabletop_reward(int32_t n, const float* obs, int32_t reward_type, int32_t wide_init,
                         float* reward, uint8_t* success, earl_stream_t stream);

/* is_valid_init(state, goal_states) (:89-97) on candidates cand [n,4] -> valid [n] 0/1. */
int earl_tabletop_valid_init(int32_t n, const double* cand, uint8_t* valid, earl_stream_t stream);

/* ---- 3-object variant (envs/tabletop_manipulation_3obj.py; not wired into the reference's loader) ----
 * qpos [n,8], attached in {-1,0,1,2} (object index; the reference encodes it as (0,0)/(.5,.5)/(1,1)),
 * goal_table [n_goals,10], obs [n,20].  Same structs; reset_at_goal = goal + U(-0.3,0.3)^8 (:64-69); wide_init and
 * goal_change_frequency must be 0 (the reference class has neither). */
int earl_tabletop3_step(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const float* act,
                        const earl_tabletop_out* out, earl_stream_t stream);
int earl_tabletop3_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T,
                           const float* act, const earl_tabletop_out* out, earl_stream_t stream);
int earl_tabletop3_reset(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const uint8_t* mask,
                         float* obs, earl_stream_t stream);
int earl_tabletop3_reward(int32_t n, const float* obs, int32_t reward_type, float* reward, uint8_t* success,
                          earl_stream_t stream);

/* earl_tabletop_eval_episodes for the 3-object variant: `episodes` evaluation episodes per env, back to back.  Episode e is earl_tabletop3_reset (all envs,
 * Philox counter cfg->counter + e (T + 1)) followed by earl_tabletop3_rollout of T steps from the next counter, its outputs at rows [e, T, n, ..] of `out`
 * (obs [episodes, T, n, 20]), its actions at act + e * act_episode_stride floats (T * n * 3: a contiguous [episodes, T, n, 3] array; 0: every episode replays
 * the same [T, n, 3]).  Bit-identical to that sequence of calls: the four outputs (the dense reward included), the state left behind (qpos [n, 8], attached,
 * goal_idx, steps_since_reset, num_interventions) and the Philox counter use, episodes * (T + 1); nothing depends on n, on the shard split (draws are keyed by the
 * global env id) or on the launch form.  EARL_ERR_ARG before any HIP call for episodes < 0, T < 0, a negative stride, act / out NULL and the 3-object env's own
 * rules (wide_init, goal_change_frequency); episodes == 0 or n == 0 returns EARL_OK; T == 0 does the resets only.
 * ONE role-split launch walks all episodes (csrc/tabletop3_rollout_ws.h: a compute wave for the recurrence, loader and storer waves around it, several episodes
 * in flight while the batch fills at most half the CUs) when cfg->auto_reset == 0, all four `out` pointers are given, T is a multiple of
 * EARL_TABLETOP3_EVAL_CHUNK and at least twice it, episodes * T < 2^24, and out->obs is 16-byte aligned, out->reward / done / success 4-byte aligned (any
 * allocation is; a slice of a larger array need not be); any other legal call is executed as the sequence, with the same bits. */
#define EARL_TABLETOP3_EVAL_CHUNK 8
int earl_tabletop3_eval_episodes(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T,
                                 const float* act, int64_t act_episode_stride, const earl_tabletop_out* out, earl_stream_t stream);

/* The closed loop of the 3-object variant in ONE launch: earl_tabletop_population_rollout's general form on qpos [n,8] and the 20-wide observation -- the
 * deterministic policy (head == NULL: policy->dims[n_layers] == 3) or the Gaussian head (head != NULL: == 6), one policy (pop == NULL) or a population, [T] outputs
 * and / or per-episode summaries (summary == NULL: none).  policy->dims[0] == EARL_TABLETOP3_OBS_DIM; everything else is the argument contract above (float32
 * only: precision != 0 is EARL_ERR_ARG -- the weights live in registers; EARL_ERR_ARG before any HIP call; n == 0 returns EARL_OK).
 * out rows [episodes, T, n, ..] with obs 20 wide, act_out [episodes, T, n, 3], head->eps_out [episodes, T, n, 3], summary rows [episodes, n]; each may be NULL
 * (`out` itself may not).  Bit-identical to the open-loop entry points fed with act_out -- outputs, state left behind, wrapper counters, Philox counter use:
 *   reset_first = 1: for each episode e, earl_tabletop3_reset (all envs, counter cfg->counter + e (T + 1)) followed by earl_tabletop3_rollout of T steps from
 *                    the next counter (episodes * (T + 1) counter values in all);
 *   reset_first = 0: earl_tabletop3_rollout (episodes must be 1; T counter values), auto-reset included.
 * The policy arithmetic, the head, its draw (one Philox block per (env, step): seed, global env id, the step's counter; words x, y, z), EARL_HEAD_MEAN == the
 * deterministic launch on rows 0..2 of the last layer, the population's addressing (global id g runs member g / G) and the summaries are those of the single-object
 * entry points, word for word.  The agent pair's 3-object form is earl_tabletop3_pair_rollout. */
int earl_tabletop3_policy_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                  const earl_policy_population* pop, const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                  const earl_tabletop_out* out, float* act_out, const earl_episode_summary* summary, earl_stream_t stream);

/* The AGENT PAIR on the 3-object variant in ONE launch: earl_tabletop_pair_rollout on qpos [n,8] and the 20-wide observation.  policy->dims[0] ==
 * EARL_TABLETOP3_OBS_DIM; pair->backward_goal is NULL or ONE goal row of 10 doubles (goal-table format); out->obs rows are 20 wide.  The contract is items 1..6 of
 * earl_tabletop_pair_rollout, word for word: the network of the env's phase, the phase-independent Philox draw, agent_out / act_out, the wrapped env step (the
 * 3-object one), auto-reset -> phase 0, handover by clock or success.  Entering the forward phase, goal_idx = the draw of this step's counter (draw 0) and the
 * observation's goal slots 10..19 are re-read with the goal in force; entering the reset phase with a backward_goal leaves goal_idx alone.  Launch entry and exit,
 * reset_first / episodes, NULL-able outputs and Philox counter use as there.  Never switching, the launch is bit-identical to earl_tabletop3_policy_rollout with
 * one policy on row 0.  Argument errors before any HIP call: the 3-object env's (wide_init, goal_change_frequency), the contract's policy / head / pair rules, and a
 * second hidden layer wider than EARL_PAIR_MAX_H2.  n == 0 returns EARL_OK. */
int earl_tabletop3_pair_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out,
                                earl_stream_t stream);

/* ---- branches: K candidate action sequences per env scored FROM THE CURRENT STATE, the state left as it is ----
 * Every entry point above advances the envs or starts them from a reset.  A shooting planner (random shooting, CEM, MPPI -- the model-predictive control loops
 * around envs/tabletop_manipulation.py:128-138 that copy the env, step the copy and throw it away: `sim = copy.deepcopy(env); for a in plan: _, r, _, _ =
 * sim.step(a)`) asks what WOULD happen: K plans of H steps per env, one return and one success flag each, nothing kept.  One launch runs one lane per
 * (branch, env), reads 12 B of actions per env-step and stores nothing inside the loop.
 *   equivalence  branch k equals earl_tabletop_rollout(cfg, <a private copy of st>, H, act + k * act_branch_stride, out) with the same cfg->counter, bit for bit:
 *                step t of EVERY branch uses counter cfg->counter + t, so all branches see the same lifelong goal draws and the same auto-reset draws (common
 *                random numbers), and a branch predicts exactly what the next real rollout with those actions will produce.
 *   act          act_branch_stride = H * n * 3: a contiguous [K, H, n, 3] array; 0: every branch replays one [H, n, 3] block.
 *   summary      NULL, or rows [K, n] with earl_episode_summary's definitions: ret the float64 sum over t ascending of the float32 reward, success_last the
 *                success of step H - 1, first_success the first step with success or -1.
 *   last_obs     NULL, or [K, n, 12]: the row out->obs[H - 1] of that rollout, after a goal switch's re-read, exactly as the rollout emits it.
 *                Each of the four pointers may be NULL in any combination.
 *   state        `st` is read and never written -- qpos, attached, goal_idx, the four wrapper arrays -- and *counter_base is not read.  The caller does not
 *                advance its counter.
 * EARL_ERR_ARG before any HIP call for: everything the other entry points refuse in cfg / st; act NULL; K < 0; H < 0; a negative stride; a stride that is neither 0
 * nor >= H * n * 3; summary == NULL && last_obs == NULL; a grid that does not fit one launch -- the launch is 1-D, K * ceil(n / EARL_BRANCH_BLOCK) workgroups of
 * EARL_BRANCH_BLOCK lanes (the branch comes from the workgroup's index: K is a planner's large dimension), and that count may not exceed 2^31 - 1 nor the lanes
 * 2^32 - 1.  n == 0, K == 0 or H == 0 returns EARL_OK, launches nothing and writes nothing. */
#define EARL_BRANCH_BLOCK 64
int earl_tabletop_branch_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                 const earl_episode_summary* summary, float* last_obs, earl_stream_t stream);
/* the same on the 3-object variant: qpos [n,8], last_obs [K, n, 20], branch k equal to earl_tabletop3_rollout on a private copy of the state (auto-reset included) */
int earl_tabletop3_branch_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                  const earl_episode_summary* summary, float* last_obs, earl_stream_t stream);

/* ---- MPPI planning: I iterations of sample -> score -> reweight on the device, the candidates never in memory, the env left as it is ----
 * The planner the branch launch was made for (model-predictive path integral control around envs/tabletop_manipulation.py:128-138: K noisy copies of a mean plan
 * rolled out on copies of the env, the mean moved to their exponentially weighted average).  The noise is generated inside the scoring kernel and REGENERATED
 * inside the update kernel from the same Philox counters, so one iteration reads the [H, n, 3] mean and a [K, n] array of returns and nothing else.  Per
 * iteration two launches on the caller's stream (score, update); no host synchronisation, no allocation: the call can be captured into a HIP graph.
 * For iteration j = iteration0 + i (i = 0 .. iterations - 1), env `env` with global id g = cfg->env_offset + env, and the plan entering the iteration `mean`
 * (the argument for i = 0, the previous iteration's result afterwards):
 *   1 clipped mean  m[t][d] = clip(mean[t][d]) in float32, clip(x) = (y = x > -1 ? x : -1; y < 1 ? y : 1) = min(max(x, -1), 1).
 *   2 candidates    branch 0 is the plan itself, a_0 = m.  For k >= 1: a_k[t][d] = clip(fmaf(sigma[d], eps, m[t][d])), eps = normal_quantile_f32(word_d >> 8)
 *                   (csrc/policy_math.h; exported by the host library as earl_normal_quantile_f32), words x, y, z of ONE Philox4x32-10 block serving d = 0, 1, 2:
 *                   key = cfg->seed, counter words = {0x504C4E00 | j, g, (k << 16) | t, noise_counter}.  Word 0 collides with no other draw of this library
 *                   (the envs use 0 .. 2048, the Gaussian head 0x504F4C00).  The draws depend on (seed, g, j, k, t, noise_counter) only: not on n, not on
 *                   the shard split.
 *   3 scores        ret[k][env] = earl_episode_summary.ret of earl_tabletop[3]_branch_rollout fed with those candidates: the same wrapped step, step t of every
 *                   branch at counter cfg->counter + t (common random numbers, lifelong and auto-reset draws included), the float64 sum over t ascending of
 *                   the float32 reward.
 *   4 weights       beta = max_k ret[k];  x_k = (float)((ret[k] - beta) * inv_temperature) (two float64 roundings);  w_k = exp_f32(x_k) (csrc/policy_math.h;
 *                   earl_exp_f32);  W_k = (double)w_k * 2^24 rounded to nearest-even as int64 (0 .. 2^24);  S = sum_k W_k (>= 2^24: the best branch has W = 2^24).
 *   5 update        delta = a_k[t][d] - m[t][d] (one float32 subtraction);  D_k = (double)delta * 2^20 rounded to nearest-even as int64;  A = sum_k W_k * D_k in
 *                   int64 (|A| < 2^62 for K <= 2^16);  mean'[t][d] = clip(m[t][d] + (float)((double)A / ((double)S * 2^20))), (double)A rounded to nearest.
 *                   Integer sums are associative: the result does not depend on how the K branches are spread over lanes, waves and workgroups.
 *   6 outputs       plan [H, n, 3] float32: the mean after the last iteration; it may be the pointer `mean` itself (the in-place call), any other overlap of
 *                   the two arrays is refused.  ret [K, n] float64, REQUIRED: the workspace between the two launches; the last iteration's returns on exit.
 *                   ret0 NULL or [iterations, n] float64: the return of the plan entering each iteration (branch 0).  best_ret NULL or [n] float64: beta of
 *                   the last iteration.  best_k NULL or [n] int32: the smallest k attaining it (earl_tabletop_plan_candidates recovers that candidate).
 *   7 non-finite    clip() maps a NaN of `mean` to -1 and +-Inf to +-1, so every candidate is finite whatever `mean` holds.  A NaN return (a NaN in the
 *                   state under the dense reward) never wins: beta is the largest return that is not NaN, -Inf if there is none; x_k that is NaN (a NaN
 *                   return, or Inf - Inf) gives W_k = 0; if S == 0 (no branch has a weight) the update is skipped, mean' = m.  best_k is the smallest k
 *                   with ret[k] == beta when beta > -Inf, and 0 otherwise.  Nothing of this faults, and `st` is never written.
 *   chaining        `iterations` iterations in one call equal that many calls with iterations = 1 and iteration0 = j, each fed the previous plan, bit for bit.
 *   state           `st` is read and never written, *counter_base is not read, and the caller does not advance its counter: the env is as earl_tabletop_branch_rollout
 *                   leaves it.
 * EARL_ERR_ARG before any HIP call for: everything the other entry points refuse in cfg / st; params, mean, plan or ret NULL; K or H outside 1 .. 65536;
 * iterations < 1, iteration0 < 0, iteration0 + iterations > 256; a sigma that is negative or not finite; an inv_temperature that is not finite or <= 0; plan
 * overlapping mean without being equal to it; a grid that does not fit: the score launch is the branch launch's (K * ceil(n / 64) workgroups, earl_tabletop_branch_rollout's
 * limits), the update launch ceil(n / 64) * ceil(H / EARL_PLAN_UPDATE_STEPS) workgroups of 64 * EARL_PLAN_UPDATE_STEPS lanes under the same two limits.
 * n == 0 returns EARL_OK, launches nothing and writes nothing. */
typedef struct earl_plan_params {
  int32_t K;               /* candidates per env, branch 0 (the plan itself) included: 1 .. 65536 */
  int32_t H;               /* steps of a plan: 1 .. 65536 */
  int32_t iterations;      /* I >= 1 */
  int32_t iteration0;      /* index of the first iteration (a word of the noise counter): >= 0, iteration0 + iterations <= 256 */
  float sigma[3];          /* noise scale per action dimension, finite, >= 0 */
  uint32_t noise_counter;  /* a word of the noise counter: a fresh value per control step gives fresh noise */
  double inv_temperature;  /* 1 / lambda, finite, > 0 */
} earl_plan_params;
#define EARL_PLAN_UPDATE_STEPS 8
int earl_tabletop_plan_mppi(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan, double* ret,
                            double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream);
/* the same on the 3-object variant (qpos [n,8]; scores equal to earl_tabletop3_branch_rollout's) */
int earl_tabletop3_plan_mppi(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan, double* ret,
                             double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream);
/* Item 2 written out for ONE iteration j (0 .. 255): act_out [K, H, n, 3] float32, what earl_tabletop[3]_branch_rollout takes.  It reads cfg->n, env_offset and seed
 * and params->K, H, sigma and noise_counter only (no env state: one entry point serves both envs).  EARL_ERR_ARG for cfg, params, mean or act_out NULL, n < 0, K or
 * H outside 1 .. 65536, j outside 0 .. 255, a bad sigma and the branch launch's grid limits; n == 0 returns EARL_OK and writes nothing. */
int earl_tabletop_plan_candidates(const earl_tabletop_cfg* cfg, const earl_plan_params* params, int32_t j, const float* mean, float* act_out, earl_stream_t stream);

/* ---- receding-horizon MPPI control: T real steps of plan -> act -> shift in ONE launch ----
 * What a planner is called for (the model-predictive control loop around envs/tabletop_manipulation.py:128-138: plan from the current state, execute the first
 * action, shift the plan by one step, plan again).  The call is DEFINED by composition of the entry points above.  Let c0 = cfg->counter and P_0 = the `plan`
 * buffer on entry.  For real step s = 0 .. T - 1:
 *   1 plan    P'_s = the `plan` output of earl_tabletop[3]_plan_mppi on the state before step s, called with cfg->counter = c0 + s, mean = P_s and `params` with
 *             noise_counter replaced by (uint32)(params->noise_counter + s); iterations and iteration0 as given.  Row s of ret0 ([T, iterations, n]) is that
 *             call's ret0, row s of best_ret ([T, n]) its best_ret.
 *   2 act     a_s = P'_s[0] (already clipped).  Row s of `out` (rows [T, n], as earl_tabletop[3]_rollout) and the new state are what
 *             earl_tabletop[3]_rollout(T = 1, act = a_s) produces at cfg->counter = c0 + s;  act[s] = a_s.
 *   3 shift   P_{s+1}[t] = P'_s[t + 1] for t < H - 1, P_{s+1}[H - 1] = P'_s[H - 1].  Exception: an env whose step s came out `done` while cfg->auto_reset is set
 *             gets P_{s+1} = 0 in all H rows -- a new episode does not inherit the old plan.
 *   4 exit    `plan` holds P_T; the state, the wrapper arrays and num_interventions are as T one-step rollouts leave them; the caller advances its counter by T.
 *             Two calls of T1 and T2 steps (the second with counter c0 + T1 and noise_counter + T1) equal one call of T1 + T2, bit for bit.
 * As properties: look-ahead step t of real step s uses env counter c0 + s + t; the noise uses Philox word 0 0x504C4E00 | j, the global env id, (k << 16) | t and
 * noise_counter + s; nothing depends on n or on the shard split.  Items 4-5 of the planner's contract are integer sums, so the result does not depend on how the
 * launch spreads the K branches over lanes and waves: the fused launch equals the composed calls bit for bit under both rewards.
 *   launch    one workgroup per env for all T steps, its lanes the K branches (ceil(K / 64) waves); no cooperative launch, no flag between workgroups, no
 *             allocation, no host synchronisation, no [K, n] workspace: the only memory touched is what the caller passes.  *counter_base is not read.
 * EARL_ERR_ARG before any HIP call for: everything earl_tabletop[3]_plan_mppi refuses (its grid limits included); out NULL or every pointer of it NULL; mpc NULL or
 * mpc->plan NULL; T < 0; K > EARL_MPC_MAX_K (one branch per lane of one workgroup); H > EARL_MPC_MAX_H; n workgroups of 64 * ceil(K / 64) lanes beyond 2^32 - 1
 * lanes.  T == 0 or n == 0 returns EARL_OK, launches nothing and writes nothing. */
#define EARL_MPC_MAX_K 1024
#define EARL_MPC_MAX_H 256
typedef struct earl_mpc_out {
  float* act;       /* NULL or [T, n, 3]: the action executed at each real step */
  float* plan;      /* REQUIRED [H, n, 3], in/out: the warm start on entry, the shifted plan for the next call on exit */
  double* ret0;     /* NULL or [T, iterations, n]: the return of the plan entering each iteration of each real step */
  double* best_ret; /* NULL or [T, n]: beta of the last iteration of each real step */
} earl_mpc_out;
int earl_tabletop_mpc_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                              const earl_mpc_out* mpc, earl_stream_t stream);
/* the same on the 3-object variant (qpos [n,8], obs rows of 20) */
int earl_tabletop3_mpc_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                               const earl_mpc_out* mpc, earl_stream_t stream);

/* ---- discounted MPPI with a terminal value: the planner and the control loop above with ret = sum_t gamma^t r_t + gamma^H V(o_H), V evaluated inside the kernels ----
 * Under the sparse reward the undiscounted H-step sum is blind whenever the goal is more than H steps away: every branch returns the same value and the plan does
 * not move.  A short-horizon sampling planner handles that with a discount and a learned value function at the end of the look-ahead.  The four entry points below
 * are earl_tabletop[3]_plan_mppi and earl_tabletop[3]_mpc_rollout with ONE item of their contracts replaced: everything written above for those calls -- items 1, 2
 * and 4 - 7 of the planner, chaining, state, counters, the noise counter words, the MPC composition (with earl_tabletop[3]_plan_mppi_value as its planner) and every
 * refusal -- holds word for word.  Item 3 becomes, per (branch k, env):
 *   3 scores   d_0 = 1.0, ret = 0.0.  For t = 0 .. H - 1 ascending: ret = ret + d_t * (double)r_t -- the product rounded to float64, then the sum rounded, no fused
 *              multiply-add -- and d_{t+1} = d_t * gamma (one float64 rounding).  r_t is the float32 reward of the same wrapped step at the same counter as before
 *              (common random numbers unchanged).  d_t depends on t only: it keeps running across an auto-reset inside the look-ahead.
 *              value != NULL: v = the float32 output of the network on the branch's LAST observation row -- exactly what earl_tabletop[3]_branch_rollout writes to
 *              last_obs[k][env] (after a lifelong goal switch: the re-read row; after an auto-reset: the terminal row) -- and ret = ret + d_H * (double)v, rounded
 *              the same way.  The network is a float32 MLP obs -> hidden (-> hidden) -> 1 under the policy contract of this header: acc = b_j; k ascending:
 *              acc = fmaf(x_k, W_jk, acc); hidden_act on the hidden layers, out_act (EARL_ACT_NONE or EARL_ACT_TANH) on the output; relu / tanh_f32 of
 *              csrc/policy_math.h.  earl_mlp_policy_forward_cpu (earl_physics.h) with a 1-wide last layer and head = NULL states it on the host.
 *   non-finite values need no new rule: a NaN v gives a NaN return, which item 7 handles (W_k = 0, never beta); a +Inf return becomes beta, every x_k is then NaN
 *              (Inf - Inf) or -Inf, so S == 0 and the update is skipped.  Nothing faults.
 *   identity   discount == 1.0 and value == NULL: every output equals the value-free entry point's bit for bit (1.0 * r is exact).
 *   launch     the same launches as the value-free calls: each lane evaluates the network itself on the observation row it holds in registers, the weights read at
 *              wave-uniform addresses.  No [K, n, obs] tensor, no extra launch, no LDS beyond the value-free kernels'.
 * EARL_PLAN_VALUE_MAX_H1: a lane holds the FIRST hidden layer of a two-hidden-layer network in registers (the second is streamed into the output, as the only
 * hidden layer of a one-hidden-layer network is: those may be 256 wide).  16 is what every MPC kernel holds at 128 VGPRs under 1024-lane workgroups WITHOUT
 * scratch: the constants of the env step that the compiler keeps in registers across the whole control loop leave the network about 40 registers next to the
 * observation row, and 32, 48 and 64 spill (12 - 28, 20 - 76 and 96 - 148 bytes per lane).  It may be lowered, never raised.
 * EARL_ERR_ARG before any HIP call for: everything the value-free entry point refuses; pv NULL; a discount that is NaN, <= 0 or > 1; a value network the policy
 * contract refuses with the env's observation width (12 / 20), action width 1 and no head (NULL params, precision != 0, n_layers, a hidden width that is not a multiple of 16
 * in 16..256, dims[3] != 0 with two layers, the activation enums); n_layers == 3 with dims[1] > EARL_PLAN_VALUE_MAX_H1. */
#define EARL_PLAN_VALUE_MAX_H1 16
typedef struct earl_plan_value {
  double discount;               /* gamma: finite, 0 < gamma <= 1 */
  const earl_mlp_policy* value;  /* NULL: no terminal term.  Otherwise V: obs -> 1 (dims[0] = 12 / 20, dims[n_layers] = 1, precision 0) */
} earl_plan_value;
int earl_tabletop_plan_mppi_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                  const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream);
int earl_tabletop3_plan_mppi_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                   const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream);
int earl_tabletop_mpc_rollout_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                    const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream);
int earl_tabletop3_mpc_rollout_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                     const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream);

/* ---- MPPI with policy-prior branches: P of the K candidates rolled out closed loop under a policy, the policy evaluated inside the score kernel ----
 * A TD-MPC-style planner proposes a few of its candidates with a learned policy pi: they carry the search where Gaussian noise around a zero or stale mean never
 * gets (under the sparse reward with the goal further than H steps away, every noise branch scores the same).  The two entry points below are
 * earl_tabletop[3]_plan_mppi (pv == NULL) or earl_tabletop[3]_plan_mppi_value (pv != NULL: the `_value` block, item 3 included) with TWO items of the contract
 * amended; everything else written for those calls -- items 1, 3, 4, 6, 7, chaining, state, counters, the noise counter words and every refusal -- holds word for word.
 *   2 candidates, branches 1 <= k <= P (P = prior->branches).  x_t = the float32 observation row the branch's env last produced: at t = 0 _get_obs() of the incoming
 *              state; afterwards the row the wrapped step t - 1 emitted (after a lifelong goal switch: the re-read row; after an auto-reset inside the look-ahead:
 *              the terminal row) -- exactly what earl_tabletop[3]_policy_rollout(reset_first = 0) feeds its policy.  u = pi(x_t) under the policy contract of this
 *              header: acc = b_j; k ascending: acc = fmaf(x_k, W_jk, acc); relu / tanh_f32 of csrc/policy_math.h on the hidden layers, out_act on the output
 *              (earl_mlp_policy_forward_cpu with head = NULL states it on the host).  a_k[t][d] = clip(fmaf(prior->sigma[d], eps, u[d])), eps from the SAME Philox
 *              block item 2 assigns to (j, g, k, t, noise_counter): same word 0, no new draw id.  clip maps a NaN of u to -1, so every candidate stays finite whatever
 *              the weights hold.  a_k is stored to prior->act[k - 1][t][env][d].  Branch 0 and the branches k > P are as they were.  The prior branches are made
 *              again in every iteration j with that iteration's noise word, so `chaining` holds as it stands (prior->act then holds the last iteration's rows).
 *   5 update   for k <= P the update reads a_k back from prior->act instead of making it again; delta, D_k (|D_k| <= 2^21 still: both operands lie in [-1, 1]), the
 *              integer sums and mean' are unchanged.
 *   identity   branches == 0 (policy and act may then be NULL): every output equals earl_tabletop[3]_plan_mppi (pv == NULL) or earl_tabletop[3]_plan_mppi_value bit
 *              for bit.
 *   launch     per iteration three launches on the caller's stream: the score launch over the K - P branches that are not prior branches (plan_mppi's kernel body),
 *              a score launch of the same shape over the P prior branches (a wave is 64 envs of ONE branch, so the policy's weights are wave-uniform scalar loads:
 *              the noise branches pay nothing for the network, in registers or in time), and the update.  No allocation, no host synchronisation: the call can be
 *              captured.  `st` is never written and the caller does not advance its counter.
 * EARL_PLAN_PRIOR_MAX_H1: a lane holds the FIRST hidden layer of a two-hidden-layer policy in registers, the second is streamed into the three outputs (as the only
 * hidden layer of a one-hidden-layer policy is: those may be 256 wide).  The network runs inside the look-ahead loop, next to the env state; the score kernels are
 * 64-lane workgroups without a 128-VGPR cap and compile without scratch at 16 (DESIGN 8 has the table).
 * EARL_ERR_ARG before any HIP call for: everything the underlying call refuses (with pv: the `_value` block's refusals); prior NULL; branches < 0 or >= K; a prior
 * sigma that is negative or not finite; with branches > 0: policy or act NULL, a network the policy contract refuses with the env's observation width (12 / 20),
 * action width 3 and no head (csrc/policy_check.h), n_layers == 3 with dims[1] > EARL_PLAN_PRIOR_MAX_H1, act overlapping mean, plan or ret. */
#define EARL_PLAN_PRIOR_MAX_H1 16
typedef struct earl_plan_prior {
  const earl_mlp_policy* policy;  /* obs -> 3: dims[0] = 12 / 20, dims[n_layers] = 3, precision 0, no head */
  int32_t branches;               /* P: 0 .. K - 1 */
  float sigma[3];                 /* noise added to the policy's action, finite, >= 0 */
  float* act;                     /* [P, H, n, 3]: the workspace between the score and the update launch AND an output (the prior branches' actions of the last iteration) */
} earl_plan_prior;
int earl_tabletop_plan_mppi_prior(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                  const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                                  earl_stream_t stream);
int earl_tabletop3_plan_mppi_prior(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                   const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                                   earl_stream_t stream);

/* ---- CEM planning: the cross-entropy method on the same launches -- elites instead of weights, a refitted std per (step, env, dim) ----
 * The planner of PETS, PlaNet and TD-MPC around envs/tabletop_manipulation.py:128-138: K noisy copies of a mean plan, the E best of them refit mean AND standard
 * deviation.  The update regenerates only the E elites from their counters (MPPI's regenerates all K), and the refitted std widens or narrows the search inside the
 * launch.  Per iteration two launches on the caller's stream (score, update); no host synchronisation, no allocation: the calls can be captured into a HIP graph.
 * For iteration j = iteration0 + i, env with global id g = cfg->env_offset + env, the entering plan `mean` and the entering std (`std0` for i = 0, the previous
 * iteration's results afterwards):
 *   1 clipped mean and clamped std   m = clip(mean) as MPPI item 1.  s = sclamp(std), sclamp(x) = (y = x > std_min ? x : std_min; y < std_max ? y : std_max): a NaN
 *                   maps to std_min.  With std0 == NULL every row's std is sclamp(sigma[d]).
 *   2 candidates    branch 0 is m.  For k >= 1: a_k[t][d] = clip(fmaf(s[t][d], eps, m[t][d])), eps as MPPI item 2: the quantile of words x, y, z of one Philox block,
 *                   key and counter words MPPI's except word 0 = 0x43454D00 | j, which collides with nothing (the envs use 0 .. 2048, the Gaussian head 0x504F4C00,
 *                   MPPI 0x504C4E00).
 *   3 scores        pv == NULL: MPPI item 3, the plain float64 sum.  Otherwise item 3 of the `_value` block word for word: the discounted sum, V on the last row, its
 *                   rules (EARL_PLAN_VALUE_MAX_H1 included).  pv = {1.0, NULL} equals pv == NULL bit for bit.
 *   4 elites        a total order over the K branches: k stands before k' iff ret[k] is not NaN and ret[k'] is NaN; or neither is NaN and ret[k] > ret[k']; or
 *                   (ret[k] == ret[k'], or both are NaN) and k < k'.  rank_k = the number of branches before k.  k is an elite iff rank_k < E and ret[k] is not NaN;
 *                   Ne = the number of elites.  The elite set is defined by this order and by nothing in the implementation.  best_ret and best_k: MPPI items 4, 7.
 *   5 update        per (t, d), over the elites in any order, every sum integer: D_k = rint((double)(a_k - m) * 2^20) as int64 (the subtraction one float32
 *                   operation; |D_k| <= 2^21, branch 0 has D = 0).  A1 = sum D_k, A2 = sum D_k^2, V = Ne * A2 - A1^2: exact in int64 (A2 < 2^52, Ne * A2 and
 *                   A1^2 <= 2^62, V >= 0).  e_mean = m + (float)((double)A1 / ((double)Ne * 2^20)).  e_std = sqrtf((float)((double)V / ((double)Ne * (double)Ne *
 *                   2^40))), the float32 square root, correctly rounded.  mean' = clip(fmaf(alpha, m - e_mean, e_mean)); std' = sclamp(fmaf(alpha, s - e_std, e_std)).
 *                   Ne == 0 (every return NaN): mean' = m, std' = s.
 *   6 outputs       plan [H, n, 3]: may be `mean` itself.  std [H, n, 3], REQUIRED: the workspace between iterations and the result; may be `std0` itself.  Any
 *                   other overlap among the four arrays is refused.  ret [K, n], REQUIRED.  ret0, best_ret, best_k: as MPPI.
 *   7 chaining, state, non-finite   as MPPI: I iterations in one call equal I calls of one, each fed the previous plan and std; `st` is never written; nothing
 *                   faults on NaN or Inf in mean, std0 or the state.
 * EARL_ERR_ARG before any HIP call for: everything earl_tabletop[3]_plan_mppi refuses; K > EARL_CEM_MAX_K; elites outside 1 .. K; an alpha that is not finite or
 * outside [0, 1); std_min / std_max not finite or not 0 <= std_min <= std_max; std NULL; the overlaps of item 6; with pv, what the `_value` calls refuse.
 * n == 0 returns EARL_OK and writes nothing.
 * earl_tabletop_cem_candidates: item 2 written out for ONE iteration j (0 .. 255), act_out [K, H, n, 3], for both envs; std NULL: sigma.  It reads cfg->n, env_offset
 * and seed and params->K, H, sigma, noise_counter, std_min and std_max only, and refuses what earl_tabletop_plan_candidates refuses and those fields' ranges.
 * earl_tabletop[3]_mpc_rollout_cem: earl_tabletop[3]_mpc_rollout, DEFINED by the same composition with earl_tabletop[3]_plan_cem as its planner: real step s plans
 * with cfg->counter = c0 + s, noise_counter + s, mean = P_s and std0 = NULL -- the search starts from sigma at every control step, so there is no std to carry or
 * shift; act, shift, the zeroed plan after an auto-reset and exit are that block's items 2 - 4; two calls of T1 and T2 equal one of T1 + T2.  One workgroup per env,
 * one lane per branch, the elites ranked in LDS.  It refuses what earl_tabletop[3]_mpc_rollout and earl_tabletop[3]_plan_cem refuse, under EARL_MPC_MAX_H and
 * EARL_CEM_MAX_K; T == 0 or n == 0 returns EARL_OK and writes nothing.  pv != NULL is REFUSED (EARL_ERR_ARG), by the device call and by its twin: with the value
 * network inside, the three-object auto-reset kernel does not fit 128 VGPRs under 1024-lane workgroups without scratch (12 bytes per lane), and no spilling
 * kernel is shipped.  pv stays in the signature for the day it fits; the discounted loop is the composition of earl_tabletop[3]_plan_cem and the one-step rollout. */
#define EARL_CEM_MAX_K 1024
typedef struct earl_cem_params {
  int32_t K, H, iterations, iteration0;   /* as earl_plan_params; K in 1 .. EARL_CEM_MAX_K */
  int32_t elites;                          /* E: 1 .. K */
  float sigma[3];                          /* the std of every row when no std0 is given; finite, >= 0 */
  uint32_t noise_counter;
  float alpha;                             /* smoothing: finite, 0 <= alpha < 1 */
  float std_min, std_max;                  /* finite, 0 <= std_min <= std_max */
} earl_cem_params;
int earl_tabletop_plan_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                           const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream);
int earl_tabletop3_plan_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                            const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream);
int earl_tabletop_cem_candidates(const earl_tabletop_cfg* cfg, const earl_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out,
                                 earl_stream_t stream);
int earl_tabletop_mpc_rollout_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                  const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream);
int earl_tabletop3_mpc_rollout_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                   const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream);

/* ---- host build: the `_cpu` entry points (BASELINE.json configs[0] "1 env, CPU ... plumbing, no GPU") ----
 * csrc/libearl_host.so = the SAME per-env functions the gfx950 kernels run (csrc/tabletop_device.h, tabletop_step.h, philox.h), compiled for the host by
 * g++ with -ffp-contract=off; one OpenMP iteration per env where a kernel has one lane per env.  Same structs, same arguments minus the stream, HOST
 * pointers, synchronous.  Outputs are bit-identical to the device entry points for every discrete output, the fp64 state and the f32 observations; the
 * dense reward differs by the device's exp() (1e-6, like device vs oracle).  Replaces the same reference calls as the twin of each name, for ONE env or a
 * batch: envs/tabletop_manipulation.py:128-138 (step), :105-126 (reset), wrappers/persistent_state_wrapper.py:17-31, wrappers/lifelong_wrapper.py:30-44.
 * Nothing in the library falls back to these: a caller asks for them (Python: EARLEnvs(..., device='cpu')).
 * earl_host_last_error() holds the message of the last failure of THESE calls. */
int earl_tabletop_step_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const float* act, const int32_t* next_goal_idx,
                           const earl_tabletop_out* out);
int earl_tabletop_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T, const float* act, const earl_tabletop_out* out);
int earl_tabletop_reset_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T, const float* act, const earl_tabletop_out* out);
int earl_tabletop_eval_episodes_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T, const float* act,
                                    int64_t act_episode_stride, const earl_tabletop_out* out);
int earl_tabletop_policy_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, int32_t episodes, int32_t T,
                                     int32_t reset_first, const earl_tabletop_out* out, float* act_out);
/* host twin of earl_tabletop_policy_rollout_gaussian: the closed loop with the sampled actor (agent.act(obs, sample=...) around
 * envs/tabletop_manipulation.py:128-138), the contract's arithmetic as plain loops; eps_out is a HOST pointer */
int earl_tabletop_policy_rollout_gaussian_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                              const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                              const earl_tabletop_out* out, float* act_out);
/* host twin of earl_tabletop_population_rollout: per env, the member's parameters and the summary's plain loops; bit-identical under the sparse reward */
int earl_tabletop_population_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                         const earl_policy_population* pop, const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                         const earl_tabletop_out* out, float* act_out, const earl_episode_summary* summary);
/* host twin of earl_tabletop_pair_rollout: the plain loops of its contract, one env at a time; every pointer of `pair` is a HOST pointer; refuses the same shapes */
int earl_tabletop_pair_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                   const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out);
int earl_tabletop_reset_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const uint8_t* mask, const int32_t* next_goal_idx, float* obs);
int earl_tabletop_observe_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_tabletop_out* out);
int earl_tabletop_reward_cpu(int32_t n, const float* obs, int32_t reward_type, int32_t wide_init, float* reward, uint8_t* success);
int earl_tabletop_valid_init_cpu(int32_t n, const double* cand, uint8_t* valid);
int earl_tabletop3_step_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const float* act, const earl_tabletop_out* out);
int earl_tabletop3_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t T, const float* act, const earl_tabletop_out* out);
int earl_tabletop3_reset_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const uint8_t* mask, float* obs);
int earl_tabletop3_reward_cpu(int32_t n, const float* obs, int32_t reward_type, float* reward, uint8_t* success);
/* host twin of earl_tabletop3_eval_episodes: the plain loop, per episode earl_tabletop3_reset_cpu then earl_tabletop3_rollout_cpu */
int earl_tabletop3_eval_episodes_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T,
                                     const float* act, int64_t act_episode_stride, const earl_tabletop_out* out);
/* host twin of earl_tabletop3_policy_rollout: the same plain loops as the single-object twins, on the 20-wide observation; bit-identical under the sparse reward */
int earl_tabletop3_policy_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                      const earl_policy_population* pop, const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                      const earl_tabletop_out* out, float* act_out, const earl_episode_summary* summary);
/* host twin of earl_tabletop3_pair_rollout: earl_tabletop_pair_rollout_cpu's loops on the 3-object env; every pointer of `pair` is a HOST pointer; refuses the same shapes */
int earl_tabletop3_pair_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                    const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out);
/* host twins of earl_tabletop_branch_rollout / earl_tabletop3_branch_rollout: the kernel's per-(branch, env) function, one OpenMP iteration per (branch, 64 envs);
 * bit-identical to earl_tabletop[3]_rollout_cpu branch by branch under both rewards, and to the device under the sparse one (dense: success_last, first_success
 * and last_obs bit for bit, ret within 1e-6 relative of the sum of |reward|); they refuse what the device entry points refuse, the grid included */
int earl_tabletop_branch_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                     const earl_episode_summary* summary, float* last_obs);
int earl_tabletop3_branch_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                      const earl_episode_summary* summary, float* last_obs);
/* host twins of earl_tabletop[3]_plan_mppi and earl_tabletop_plan_candidates: the kernels' per-lane functions (csrc/tabletop_plan.h) in plain loops, the integer sums
 * in ascending k.  Bit-identical to the device in every output under the sparse reward; under the dense one ret / ret0 / best_ret within the branch launch's bound
 * (1e-6 relative of the sum of |reward|) and the plans not comparable.  They refuse what the device entry points refuse, the grids included. */
int earl_tabletop_plan_mppi_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan,
                                double* ret, double* ret0, double* best_ret, int32_t* best_k);
int earl_tabletop3_plan_mppi_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan,
                                 double* ret, double* ret0, double* best_ret, int32_t* best_k);
int earl_tabletop_plan_candidates_cpu(const earl_tabletop_cfg* cfg, const earl_plan_params* params, int32_t j, const float* mean, float* act_out);
/* host twins of earl_tabletop[3]_mpc_rollout: one OpenMP iteration per env, the kernel's per-lane functions (csrc/tabletop_mpc.h) with the branches in ascending k.
 * Bit-identical to the composition of the `_cpu` planner and rollout under both rewards, and to the device under the sparse one (dense: the device's exp moves
 * the plans apart after the first step; not comparable).  They refuse what the device entry points refuse. */
int earl_tabletop_mpc_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                                  const earl_mpc_out* mpc);
int earl_tabletop3_mpc_rollout_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                                   const earl_mpc_out* mpc);
/* host twins of earl_tabletop[3]_plan_mppi_value / earl_tabletop[3]_mpc_rollout_value: the twins above with the kernels' own per-lane functions of
 * csrc/tabletop_value.h; the value network's params is a HOST pointer.  Bit-identical to the device in every output under the sparse reward (the network's
 * arithmetic is the policy contract's); under the dense reward as the value-free twins.  They refuse what the device entry points refuse. */
int earl_tabletop_plan_mppi_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                      const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k);
int earl_tabletop3_plan_mppi_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                       const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k);
int earl_tabletop_mpc_rollout_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                        const earl_tabletop_out* out, const earl_mpc_out* mpc);
int earl_tabletop3_mpc_rollout_value_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                         const earl_tabletop_out* out, const earl_mpc_out* mpc);
/* host twins of earl_tabletop[3]_plan_mppi_prior: the planner's twin with the kernels' own per-lane functions of csrc/tabletop_prior.h; the policy's params and
 * prior->act are HOST pointers.  Bit-identical to the device in every output, prior->act included, under the sparse reward; under the dense one as the twins above.
 * They refuse what the device entry points refuse. */
int earl_tabletop_plan_mppi_prior_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                      const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k);
int earl_tabletop3_plan_mppi_prior_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                       const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k);
/* host twins of earl_tabletop[3]_plan_cem, earl_tabletop_cem_candidates and earl_tabletop[3]_mpc_rollout_cem: the kernels' per-lane functions (csrc/tabletop_cem.h) in
 * plain loops.  Items 4 - 5 are integer: bit-identical to the device in every output under the sparse reward; under the dense one ret, ret0 and best_ret within
 * 1e-6 relative of the sum of |reward| and the plans not comparable.  They refuse what the device entry points refuse. */
int earl_tabletop_plan_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                               const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k);
int earl_tabletop3_plan_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                                const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k);
int earl_tabletop_cem_candidates_cpu(const earl_tabletop_cfg* cfg, const earl_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out);
int earl_tabletop_mpc_rollout_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                      const earl_tabletop_out* out, const earl_mpc_out* mpc);
int earl_tabletop3_mpc_rollout_cem_cpu(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                       const earl_tabletop_out* out, const earl_mpc_out* mpc);
int earl_host_set_threads(int n);      /* OpenMP threads of the calls above (n <= 0: query); returns the count in force */
const char* earl_host_version(void);
const char* earl_host_last_error(void);

/* ---- library ---- */
/* Test/bench hook: which kernel earl_tabletop_rollout uses. 0 = automatic (the wave-specialised kernel whenever
 * lifelong switching and auto-reset are off and all four outputs are requested), 1 = always the plain
 * one-lane-per-env kernel.  Both produce bit-identical outputs.  Returns the previous setting. */
int earl_debug_set_rollout_impl(int impl);
/* Test/bench hook: the launch form of earl_tabletop3_eval_episodes.  0 = automatic, 1 = always the sequence of existing kernels, 2 = fused, but all episodes
 * on one group of workgroups (no episodes in flight).  All three produce bit-identical results.  Returns the previous setting. */
int earl_debug_set_rollout3_form(int form);
int earl_debug_set_rollout_wgs_per_cu(int k);
/* Diagnostic: per-workgroup cycle sums of the instrumented rollout variant (impl 9); blocks until the copy is done. */
int earl_debug_read_ws_profile(uint64_t* out, int32_t n_words);
const char* earl_version(void);
const char* earl_last_error(void);
int earl_device_count(void); /* number of HIP devices visible, <= 0 when there is none */

#ifdef __cplusplus
}
#endif
#endif /* EARL_TABLETOP_H */

"""Batched, GPU-resident counterpart of the reference's tabletop_manipulation env.

Mirrors `TabletopManipulation` (reference: earl_benchmark/envs/tabletop_manipulation.py) -- same
constructor arguments, same method names (`reset`, `step`, `reset_goal`, `get_next_goal`,
`compute_reward`, `is_successful`, `get_obs`/`_get_obs`, `set_state`), same observation layout -- but
every call acts on `num_envs` independent env instances whose state lives in HBM as torch tensors,
and all arithmetic runs in the hand-written HIP kernels behind include/earl_tabletop.h
(csrc/tabletop.hip).  There is no CPU FALLBACK: constructing an env on the default device without the HIP library
or without a GPU raises.  device='cpu', asked for by name, runs the same per-env functions compiled for the host
(csrc/libearl_host.so, the `_cpu` entry points of include/earl_tabletop.h; BASELINE configs[0]).

Batched conventions: observations `[N, 12] float32`, rewards `[N] float32`, done / success `[N] bool`
torch tensors on the env's device.  With `num_envs == 1` and `scalar_api=True` the env returns what
the reference returns (numpy obs `[12]`, python float reward, python bool done, `{}`), for code
written against the reference.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from .. import _abi
from ..policy import PairPopulation, PolicyPopulation, require_widths
from ..spaces import Box

INT32_MAX = 2**31 - 1

# reference: tabletop_manipulation.py:11-16
initial_states = np.array([[0.0, 0.0, 2.5, 0.0, -1., -1.]])
goal_states = np.array([[0.0, 0.0, -2.5, -1.0, -1., -1.],
                        [0.0, 0.0, -2.5, 1.0, -1., -1.],
                        [0.0, 0.0, 0.0, 2.0, -1., -1.],
                        [0.0, 0.0, 0.0, -2.0, -1., -1.]])
TARGET_COLORS = ['r', 'g', 'b', 'k']  # :35 -- task 'rc_<colour>' moves the mug to goal_states[index(colour)]


def task_goal_rows(task_list):
  """get_next_goal (:62-76): a task string 'rc_k' -> goal = initial_state with the mug slot set to the target of
  colour k.  Returns the goal-table rows [n_tasks, 6] in task order (uniformly sampled at reset)."""
  rows = []
  for task in task_list.split('-'):
    goal = initial_states[0].copy()
    for sub in task.split('__'):
      obj, colour = sub.split('_')
      if obj != 'rc':
        raise ValueError(f'unknown object {obj!r} in task {task!r} (the model has one mug: "rc")')
      goal[2:4] = goal_states[TARGET_COLORS.index(colour)][2:4]
    rows.append(goal)
  return np.stack(rows)


def _ptr(t):
  return None if t is None else t.data_ptr()


class TabletopManipulation:
  """N independent tabletop envs stepped by one HIP kernel launch (one lane per env)."""

  NOBJ = 1
  OBS_DIM = 12
  NQ = 4
  _FN = 'earl_tabletop_'

  def __init__(self, task_list='rc_r-rc_k-rc_g-rc_b', reward_type='dense', reset_at_goal=False, wide_init_distr=False,
               num_envs=1, device='cuda', seed=0, env_offset=0, scalar_api=None, auto_reset=False):
    dev = torch.device(device)
    if dev.type == 'cpu':
      # asked for by name, never a fallback: the `_cpu` entry points of include/earl_tabletop.h -- this file's kernels' own per-env functions
      # (csrc/tabletop_device.h, tabletop_step.h) compiled for the host (csrc/libearl_host.so), host tensors, no stream.  BASELINE configs[0].
      self._lib = _abi.load_host()
    elif dev.type != 'cuda':
      raise _abi.EarlHipError(f'device={device!r}: the tabletop hot path runs on MI355X (device="cuda"), or on the host when asked for device="cpu"')
    else:
      self._lib = _abi.load()
      if not torch.cuda.is_available():
        raise _abi.EarlHipError('no HIP device visible (torch.cuda.is_available() is False)')
      if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    if reward_type not in _abi.REWARD_TYPES:
      raise ValueError(f'reward_type must be sparse|dense, got {reward_type!r}')
    self.device = dev
    self.num_envs = int(num_envs)
    self.scalar_api = (self.num_envs == 1) if scalar_api is None else bool(scalar_api)
    if self.scalar_api and self.num_envs != 1:
      raise ValueError('scalar_api needs num_envs == 1')
    self._task_list = task_list
    self._reward_type = reward_type
    self._reset_at_goal = bool(reset_at_goal)
    self._wide_init_distr = bool(wide_init_distr)
    self.threshold = 0.4
    self.move_distance = 0.2
    self.initial_state = self._initial_states()[0].copy()
    self._goal_list = self._goal_states().copy()

    n = self.num_envs
    self._base_goals = self._task_rows(task_list)                    # rows the RNG samples from
    self._n_sample_goals = len(self._base_goals)
    self._goal_width = self._base_goals.shape[1]
    kw = dict(device=dev)
    self.qpos = torch.zeros(n, self.NQ, dtype=torch.float64, **kw)
    self.attached = torch.full((n,), -1, dtype=torch.int8, **kw)
    self.goal_idx = torch.zeros(n, dtype=torch.int32, **kw)
    self.goal_table = torch.tensor(self._base_goals, dtype=torch.float64, **kw)
    self.steps_since_reset = torch.zeros(n, dtype=torch.int32, **kw)
    self.interventions = torch.zeros(n, dtype=torch.int32, **kw)
    self.steps_since_goal_change = torch.zeros(n, dtype=torch.int32, **kw)
    self.lifelong_return_t = torch.zeros(n, dtype=torch.float64, **kw)
    self.total_step_count = 0
    self._last_success = None
    self.agent_phase = None                                          # [N] int8 / [N] int32, allocated by the first rollout_agents: an env that never saw an
    self.steps_in_phase = None                                       # agent pair behaves and serialises as it always did
    self._pair_counts = None

    self._cfg = _abi.TabletopCfg(n=n, env_offset=int(env_offset), reward_type=_abi.REWARD_TYPES[reward_type],
                                 wide_init=int(self._wide_init_distr), reset_at_goal=int(self._reset_at_goal),
                                 horizon=INT32_MAX, goal_change_frequency=0, auto_reset=int(bool(auto_reset)),
                                 n_goals=len(self._base_goals), n_sample_goals=self._n_sample_goals,
                                 seed=int(seed) & (2**64 - 1), counter=0)
    self._st = _abi.TabletopState()
    self._cfg_ref, self._st_ref = C.byref(self._cfg), C.byref(self._st)   # reused by the hot calls
    self._sync_state_ptrs()

    self.action_space = Box(-1.0, 1.0, (3,), np.float32)           # three ctrlrange=[-1,1] motors of the model
    self.observation_space = Box(-np.inf, np.inf, (self.OBS_DIM,), np.float32)
    # like gym's MujocoEnv constructor, leave the env in a reset state
    with self._ctx():
      self._reset_kernel(None, None, want_obs=False)
    self.interventions.zero_()

  # ------------------------------------------------------------------ tables (overridden by the 3obj variant)
  @staticmethod
  def _initial_states():
    return initial_states

  @staticmethod
  def _goal_states():
    return goal_states

  @staticmethod
  def _task_rows(task_list):
    return task_goal_rows(task_list)

  @property
  def unwrapped(self):
    return self

  # ------------------------------------------------------------------ plumbing
  def _sync_state_ptrs(self):
    s = self._st
    s.qpos, s.attached, s.goal_idx, s.goal_table = _ptr(self.qpos), _ptr(self.attached), _ptr(self.goal_idx), _ptr(self.goal_table)
    s.steps_since_reset, s.num_interventions = _ptr(self.steps_since_reset), _ptr(self.interventions)
    s.steps_since_goal_change, s.lifelong_return = _ptr(self.steps_since_goal_change), _ptr(self.lifelong_return_t)
    self._cfg.n_goals = self.goal_table.shape[0]

  def _stream(self):
    return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == 'cuda' else None

  def _ctx(self):
    """launches go to the current device's runtime context (nothing to select on the host)"""
    return torch.cuda.device(self.device) if self.device.type == 'cuda' else contextlib.nullcontext()

  def _check(self, rc, what):
    if rc:
      _abi.check(rc, what, self._lib)

  def _next_counter(self, k=1):
    c = self._cfg.counter
    self._cfg.counter = c + k
    return c

  def _as_i32(self, x):
    if x is None:
      return None
    return torch.as_tensor(x, device=self.device).to(torch.int32).contiguous()

  def _reset_kernel(self, mask, next_goal_idx, want_obs=True):
    obs = torch.empty(self.num_envs, self.OBS_DIM, dtype=torch.float32, device=self.device) if want_obs else None
    m = None if mask is None else torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
    g = self._as_i32(next_goal_idx)
    if self.NOBJ == 1:
      rc = self._lib.earl_tabletop_reset(C.byref(self._cfg), C.byref(self._st), _ptr(m), _ptr(g), _ptr(obs), self._stream())
    else:
      rc = self._lib.earl_tabletop3_reset(C.byref(self._cfg), C.byref(self._st), _ptr(m), _ptr(obs), self._stream())
    self._check(rc, 'reset')
    self._next_counter()
    return obs

  def _new_out(self, lead):
    kw = dict(device=self.device)
    obs = torch.empty(*lead, self.OBS_DIM, dtype=torch.float32, **kw)
    rew = torch.empty(*lead, dtype=torch.float32, **kw)
    done = torch.empty(*lead, dtype=torch.bool, **kw)
    succ = torch.empty(*lead, dtype=torch.bool, **kw)
    return (obs, rew, done, succ), _abi.TabletopOut(_ptr(obs), _ptr(rew), _ptr(done), _ptr(succ))

  def _actions(self, action, lead):
    a = torch.as_tensor(action, device=self.device)
    if a.dtype != torch.float32:
      a = a.to(torch.float32)
    a = a.reshape(*lead, 3)
    return a if a.is_contiguous() else a.contiguous()

  # ------------------------------------------------------------------ gym-style API
  def reset(self, mask=None, goal_idx=None):
    """reset() of the reference for every env (or the envs selected by the bool tensor `mask`).  `goal_idx`
    (optional, [N]) injects the goal-table rows instead of sampling, like `reset_goal(goal)` in the reference."""
    with self._ctx():
      obs = self._reset_kernel(mask, goal_idx)
      if self.agent_phase is not None:                               # a reset env is the forward agent's again
        if mask is None:
          self.agent_phase.zero_()
          self.steps_in_phase.zero_()
        else:
          m = torch.as_tensor(mask, device=self.device).bool()
          self.agent_phase[m] = 0
          self.steps_in_phase[m] = 0
    return obs[0].cpu().numpy() if self.scalar_api else obs

  def _out_struct(self, outs, lead):
    """validate caller-provided output tensors (obs, reward, done, success) and wrap their pointers"""
    want = [(lead + (self.OBS_DIM,), torch.float32), (lead, torch.float32), (lead, torch.bool), (lead, torch.bool)]
    if len(outs) != 4:
      raise ValueError('out must be (obs, reward, done, success)')
    for t, (shape, dt) in zip(outs, want):
      if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
        raise ValueError(f'out tensor must be contiguous {dt} {shape} on {self.device}')
    return _abi.TabletopOut(*(t.data_ptr() for t in outs))

  def step(self, action, next_goal_idx=None, out=None):
    """step(action) of the wrapped reference env for every env: action [N, 3] -> (obs [N, D], reward [N], done [N],
    {'success': [N]}).  Fresh output tensors per call like the reference (callers may keep them); pass
    `out=(obs, reward, done, success)` to write into preallocated tensors instead."""
    n = self.num_envs
    if (torch.is_tensor(action) and action.dtype == torch.float32 and action.device == self.device
        and action.shape == (n, 3) and action.is_contiguous()):
      act = action
    else:
      act = self._actions(action, (n,))
    if out is None:
      outs, ostruct = self._new_out((n,))
    else:
      outs, ostruct = tuple(out), self._out_struct(tuple(out), (n,))
    r64 = None
    if self.scalar_api:        # the reference returns the reward as a Python float (float64), not rounded to float32
      r64 = torch.empty(n, dtype=torch.float64, device=self.device)
      ostruct.reward_f64 = r64.data_ptr()
    ctx = None
    if self.device.type == 'cuda' and torch.cuda.current_device() != self.device.index:   # launches go to the current device's runtime context
      ctx = torch.cuda.device(self.device)
      ctx.__enter__()
    try:
      if self.NOBJ == 1:
        g = self._as_i32(next_goal_idx)
        rc = self._lib.earl_tabletop_step(self._cfg_ref, self._st_ref, act.data_ptr(), _ptr(g), C.byref(ostruct), self._stream())
      else:
        rc = self._lib.earl_tabletop3_step(self._cfg_ref, self._st_ref, act.data_ptr(), C.byref(ostruct), self._stream())
    finally:
      if ctx is not None:
        ctx.__exit__(None, None, None)
    if rc:
      self._check(rc, 'step')
    self._cfg.counter += 1          # every call uses the current Philox counter, then advances it
    self.total_step_count += 1
    obs, rew, done, succ = outs
    self._last_success = succ
    if self.scalar_api:
      return obs[0].cpu().numpy(), float(r64[0]), bool(done[0]), {}
    return obs, rew, done, {'success': succ}

  def rollout_episodes(self, actions, episodes=None, out=None):
    """`episodes` evaluation episodes of every env, back to back (each = reset() + T steps), in ONE kernel launch when the fused kernel
    applies (include/earl_tabletop.h: earl_tabletop_eval_episodes).  actions [T, N, 3] (replayed by every episode; give `episodes`) or
    [E, T, N, 3].  -> (obs [E,T,N,D], reward [E,T,N], done [E,T,N], success [E,T,N]); bit-identical to E calls of
    rollout(actions, reset_first=True).  The three-object env goes through earl_tabletop3_eval_episodes and returns obs [E,T,N,20]."""
    with self._ctx():
      a = torch.as_tensor(actions, device=self.device)
      if a.dim() == 4:
        E, T = int(a.shape[0]), int(a.shape[1])
        if episodes is not None and int(episodes) != E:
          raise ValueError(f'episodes = {episodes} but actions hold {E}')
        act, stride = self._actions(a, (E, T, self.num_envs)), T * self.num_envs * 3
      else:
        if episodes is None:
          raise ValueError('rollout_episodes: actions [T, N, 3] are replayed by every episode -- say how many (episodes=E), or pass [E, T, N, 3]')
        E, T = int(episodes), int(a.shape[0])
        act, stride = self._actions(a, (T, self.num_envs)), 0
      if out is None:
        outs, ostruct = self._new_out((E, T, self.num_envs))
      else:
        outs = tuple(out)
        ostruct = self._out_struct(outs, (E, T, self.num_envs))
      fn = self._lib.earl_tabletop_eval_episodes if self.NOBJ == 1 else self._lib.earl_tabletop3_eval_episodes
      rc = fn(self._cfg_ref, self._st_ref, E, T, act.data_ptr(), stride, C.byref(ostruct), self._stream())
    self._check(rc, 'eval_episodes')
    self._cfg.counter += E * (T + 1)
    self.total_step_count += E * T
    self._last_success = outs[3][-1, -1]
    return outs

  def rollout_policy(self, policy, T, episodes=None, reset_first=True, out=None, sample=True, return_noise=False):
    """Closed loop in ONE kernel launch (include/earl_tabletop.h: earl_tabletop_policy_rollout): `policy` (an `MLPPolicy`) is evaluated inside the
    kernel between the env steps, observation -> MLP -> action -> step.  reset_first=True: `episodes` (default 1) evaluation episodes, each reset() +
    T steps; reset_first=False: T steps continuing from the current state (lifelong switching and auto-reset included).
    -> (obs [E,T,N,D], reward [E,T,N], done, success, actions [E,T,N,3]) -- without the E axis when reset_first=False.  Bit-identical to
    rollout_episodes(actions) / rollout(actions) fed with the returned actions.
    A `GaussianMLPPolicy` goes to earl_tabletop_policy_rollout_gaussian: sample=True draws the actions inside the kernel (tanh(mean + exp(log_std) eps),
    eps from the env's Philox stream keyed by the global env id and the step's counter), sample=False evaluates the actor at its mean;
    return_noise=True appends eps [E,T,N,3], the standard-normal draws as used.  Both are for Gaussian policies only.
    A `PolicyPopulation` goes to earl_tabletop_population_rollout: the env with global id g runs member g // envs_per_policy, same returns.
    The three-object env takes the same three classes built with obs_dim=20, act_dim=3 and returns the same tuple with obs [.., 20], every form through
    earl_tabletop3_policy_rollout; bit-identical to reset() + rollout(actions) per episode / rollout(actions) fed with the returned actions."""
    gaussian = self._closed_loop_policy('rollout_policy', policy)
    if not gaussian and (return_noise or not sample):
      raise ValueError('rollout_policy: sample=False / return_noise=True need a GaussianMLPPolicy (an MLPPolicy is deterministic)')
    T = int(T)
    E, lead = self._closed_loop_shape('rollout_policy', T, episodes, reset_first)
    with self._ctx():
      outs, ostruct, actions, eps = self._closed_loop_out(lead, out, return_noise)
      if isinstance(policy, PolicyPopulation) or self.NOBJ != 1:
        rc = self._population_launch(policy, gaussian, E, T, reset_first, ostruct, actions, eps, sample, None)
      elif gaussian:
        head = policy.head(sample=bool(sample), eps_out=eps)
        rc = self._lib.earl_tabletop_policy_rollout_gaussian(self._cfg_ref, self._st_ref, C.byref(policy.struct), C.byref(head), E, T,
                                                             int(bool(reset_first)), C.byref(ostruct), actions.data_ptr(), self._stream())
      else:
        rc = self._lib.earl_tabletop_policy_rollout(self._cfg_ref, self._st_ref, C.byref(policy.struct), E, T, int(bool(reset_first)), C.byref(ostruct),
                                                    actions.data_ptr(), self._stream())
    self._closed_loop_done(rc, 'policy_rollout', E, T, reset_first, outs[3])
    if return_noise:
      return outs + (actions, eps)
    return outs + (actions,)

  # what rollout_policy, evaluate_policy and rollout_agents share: the refusals, the launch shape, the allocations and the bookkeeping after the launch
  def _closed_loop_policy(self, who, policy, pair=False):
    """the refusals every closed-loop launch begins with -> is the policy Gaussian"""
    if self.NOBJ == 3 and (getattr(policy, 'obs_dim', 12), getattr(policy, 'act_dim', 3)) == (20, 3):
      return require_widths(policy, who, 20, 3, env=self, pair=pair)    # the three-object env's own widths: earl_tabletop3_policy_rollout / earl_tabletop3_pair_rollout
    gaussian = require_widths(policy, who, 12, 3, env=self, pair=pair)
    if self.NOBJ != 1:
      raise NotImplementedError(f'{who}: single-object env only')
    return gaussian

  def _closed_loop_shape(self, who, T, episodes, reset_first):
    """-> (E, lead): `episodes` (default 1) episodes of reset() + T steps [E, T, N], or T continuing steps [T, N]"""
    if reset_first:
      E = 1 if episodes is None else int(episodes)
      return E, (E, T, self.num_envs)
    if episodes not in (None, 1):
      raise ValueError(f'{who}: a continuing rollout (reset_first=False) is one episode')
    return 1, (T, self.num_envs)

  def _closed_loop_out(self, lead, out, return_noise):
    """-> (outs, their struct, actions, eps or None): `out` as given by the caller, or fresh tensors"""
    if out is None:
      outs, ostruct = self._new_out(lead)
    else:
      outs = tuple(out)
      ostruct = self._out_struct(outs, lead)
    actions = torch.empty(*lead, 3, dtype=torch.float32, device=self.device)
    eps = torch.empty(*lead, 3, dtype=torch.float32, device=self.device) if return_noise else None
    return outs, ostruct, actions, eps

  def _closed_loop_done(self, rc, what, E, T, reset_first, success):
    """after the launch: its status, the Philox counter (every reset and every step took one), and the success flags of the last step"""
    self._check(rc, what)
    self._cfg.counter += E * (T + 1) if reset_first else T
    self.total_step_count += E * T
    self._last_success = success[(-1,) * (success.dim() - 1)]

  def _population_launch(self, policy, gaussian, E, T, reset_first, ostruct, actions, eps, sample, summary):
    """earl_tabletop_population_rollout (the three-object env: earl_tabletop3_policy_rollout, the same arguments) for a PolicyPopulation (pop) or one policy
    (pop = NULL); -> the return code"""
    head = policy.head(sample=bool(sample), eps_out=eps) if gaussian else None
    pop = getattr(policy, 'pop_struct', None)
    launch = self._lib.earl_tabletop_population_rollout if self.NOBJ == 1 else self._lib.earl_tabletop3_policy_rollout
    return launch(self._cfg_ref, self._st_ref, C.byref(policy.struct), None if pop is None else C.byref(pop),
                  None if head is None else C.byref(head), E, T, int(bool(reset_first)), C.byref(ostruct), _ptr(actions),
                  None if summary is None else C.byref(summary), self._stream())

  def evaluate_policy(self, policy, T, episodes=1, sample=False):
    """`episodes` evaluation episodes (each reset() + T closed-loop steps) of `policy` -- an MLPPolicy, a GaussianMLPPolicy (sample=False: at its mean) or a
    `PolicyPopulation` (the env with global id g runs member g // envs_per_policy) -- in ONE launch that writes only per-episode summaries
    (include/earl_tabletop.h: earl_tabletop_population_rollout with every `out` pointer NULL): nothing of size T is allocated.
    -> {'ret': [E, N] float64 undiscounted return (the float32 step rewards summed in float64, t ascending), 'success': [E, N] bool success at the last step,
        'first_success': [E, N] int32 first successful step, -1 if none}; each equals its definition applied to what rollout_policy would have returned.
    Philox counter and total_step_count advance as in rollout_policy."""
    gaussian = self._closed_loop_policy('evaluate_policy', policy)
    if sample and not gaussian:
      raise ValueError('evaluate_policy: sample=True needs a Gaussian policy (an MLPPolicy is deterministic)')
    E, T, n = int(episodes), int(T), self.num_envs
    with self._ctx():
      ret = torch.empty(E, n, dtype=torch.float64, device=self.device)
      succ = torch.empty(E, n, dtype=torch.bool, device=self.device)
      first = torch.empty(E, n, dtype=torch.int32, device=self.device)
      summary = _abi.EpisodeSummary(ret=ret.data_ptr(), success_last=succ.data_ptr(), first_success=first.data_ptr())
      rc = self._population_launch(policy, gaussian, E, T, True, _abi.TabletopOut(None, None, None, None), None, None, sample, summary)
    self._closed_loop_done(rc, 'population_rollout', E, T, True, succ)
    return {'ret': ret, 'success': succ, 'first_success': first}

  def rollout_agents(self, pair, T, episodes=None, reset_first=False, sample=True, return_noise=False, out=None):
    """The forward / reset agent pair of autonomous RL alternating inside ONE kernel launch (include/earl_tabletop.h: earl_tabletop_pair_rollout; the three-object env with a
    20-wide pair, `AgentPair(f, b, ..., obs_dim=20, act_dim=3)`: earl_tabletop3_pair_rollout, the goal row 10 wide): every env is
    driven by the agent of its phase (`env.agent_phase`: 0 forward, 1 reset) and handed over after pair.switch_every[phase] steps or, with
    pair.switch_on_success, after a step whose success flag is set.  The default is the continuing form -- T steps from the current state, the training
    stream; reset_first=True: `episodes` evaluation episodes, each reset() + T steps starting with the forward agent.
    -> (obs [T,N,D], reward [T,N], done, success, actions [T,N,3], agent [T,N] int8 = the agent that computed the action) -- with a leading E axis when
    reset_first=True; return_noise=True (Gaussian agents) appends eps.  `env.pair_counts` = (forward phases, reset phases) [E, N] that ended by success in
    this launch.  The reset agent sees pair.backward_goal in its observation's goal slots; `goal_idx` keeps the env's task goal throughout."""
    if not isinstance(pair, PairPopulation) and (getattr(pair, 'backward_goals', None) is not None or (isinstance(getattr(pair, 'backward_goal', None), str) and pair.backward_goal == 'initial_states')):
      raise ValueError('rollout_agents: a table of backward goals runs on the Sawyer door and peg only (earl_sawyer_agents_rollout); the tabletop pair takes ONE row')
    gaussian = self._closed_loop_policy('rollout_agents', pair, pair=True)
    if self._cfg.goal_change_frequency > 0:
      raise ValueError('rollout_agents: the agent pair IS the lifelong mechanism (the forward handover makes the lifelong switch\'s goal draw): '
                       'not under a LifelongWrapper, whose clock would fight the pair\'s over the same draw')
    if not gaussian and (return_noise or not sample):
      raise ValueError('rollout_agents: sample=False / return_noise=True need Gaussian agents (MLPPolicy agents are deterministic)')
    T = int(T)
    E, lead = self._closed_loop_shape('rollout_agents', T, episodes, reset_first)
    with self._ctx():
      if self.agent_phase is None:
        self.agent_phase = torch.zeros(self.num_envs, dtype=torch.int8, device=self.device)
        self.steps_in_phase = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
      outs, ostruct, actions, eps = self._closed_loop_out(lead, out, return_noise)
      agent = torch.empty(*lead, dtype=torch.int8, device=self.device)
      fwd = torch.empty(E, self.num_envs, dtype=torch.int32, device=self.device)
      bwd = torch.empty(E, self.num_envs, dtype=torch.int32, device=self.device)
      goal = pair.goal_row(self)
      ps = _abi.AgentPair(switch_every=(_abi.C.c_int32 * 2)(*pair.switch_every), switch_on_success=int(pair.switch_on_success), pad_=0, param_stride=pair.stride,
                          backward_goal=_ptr(goal), phase=self.agent_phase.data_ptr(), steps_in_phase=self.steps_in_phase.data_ptr(),
                          agent_out=agent.data_ptr(), forward_success=fwd.data_ptr(), backward_success=bwd.data_ptr())
      head = pair.head(sample=bool(sample), eps_out=eps) if gaussian else None
      launch = self._lib.earl_tabletop_pair_rollout if self.NOBJ == 1 else self._lib.earl_tabletop3_pair_rollout
      rc = launch(self._cfg_ref, self._st_ref, C.byref(pair.struct), C.byref(ps), None if head is None else C.byref(head), E, T, int(bool(reset_first)),
                  C.byref(ostruct), actions.data_ptr(), self._stream())
    self._closed_loop_done(rc, 'pair_rollout', E, T, reset_first, outs[3])
    self._pair_counts = (fwd, bwd)
    if return_noise:
      return outs + (actions, agent, eps)
    return outs + (actions, agent)

  @property
  def pair_counts(self):
    """(forward_success, backward_success) [E, N] int32 of the last rollout_agents launch: the phases that ended by success; None before the first"""
    return self._pair_counts

  def make_step_graph(self, T, policy=None):
    """Closed-loop stepping without the per-call host cost: a captured HIP graph of T step launches (see `StepGraph`)."""
    return StepGraph(self, T, policy)

  def rollout(self, actions, out=None, reset_first=False):
    """T steps in one kernel launch: actions [T, N, 3] -> (obs [T,N,D], reward [T,N], done [T,N], success [T,N]).
    Bit-identical to T calls of step().  `out`: optional tuple of preallocated output tensors to write into.
    `reset_first=True` folds a reset() of every env into the same launch (one evaluation episode per call)."""
    with self._ctx():
      a = torch.as_tensor(actions, device=self.device)
      T = a.shape[0]
      act = self._actions(a, (T, self.num_envs))
      if out is None:
        outs, out = self._new_out((T, self.num_envs))
      else:
        outs = tuple(out)
        out = self._out_struct(outs, (T, self.num_envs))
      if reset_first and self.NOBJ == 1:
        fn = self._lib.earl_tabletop_reset_rollout
      else:
        if reset_first:
          self._reset_kernel(None, None, want_obs=False)
        fn = self._lib.earl_tabletop_rollout if self.NOBJ == 1 else self._lib.earl_tabletop3_rollout
      rc = fn(C.byref(self._cfg), C.byref(self._st), T, act.data_ptr(), C.byref(out), self._stream())
    self._check(rc, 'rollout')
    self._cfg.counter += T + (1 if reset_first and self.NOBJ == 1 else 0)   # step t used counter (+1 after a fused reset) + t
    self.total_step_count += T
    self._last_success = outs[3][-1]
    return outs

  def rollout_branches(self, actions, last_obs=True, out=None):
    """K candidate action sequences of H steps scored per env FROM THE CURRENT STATE in one kernel launch (include/earl_tabletop.h:
    earl_tabletop_branch_rollout): actions [K, H, N, 3] -> {'ret' [K, N] float64, 'success' [K, N] bool (the success of step H - 1), 'first_success' [K, N]
    int32 (-1: none), 'last_obs' [K, N, D] float32}.  Row k is what rollout(actions[k]) would return next, reduced (ret = the float64 sum of its float32
    rewards), lifelong goal draws and auto-reset draws included; the env is left exactly as found -- state, counters, the Philox counter.  What a shooting
    planner (random shooting, CEM, MPPI) asks for.  `last_obs=False` leaves that array out.  `out`: an optional dict of preallocated tensors under the same
    keys; a key that is missing or None is not computed."""
    a = torch.as_tensor(actions, device=self.device)
    n = self.num_envs
    if a.dim() != 4 or a.shape[2] != n or a.shape[3] != 3:
      raise ValueError(f'rollout_branches: actions must be [K, H, N, 3] = [K, H, {n}, 3], got {list(a.shape)} (one plan for every env is [1, H, {n}, 3])')
    K, H = int(a.shape[0]), int(a.shape[1])
    kw = dict(device=self.device)
    want = {'ret': ((K, n), torch.float64), 'success': ((K, n), torch.bool), 'first_success': ((K, n), torch.int32),
            'last_obs': ((K, n, self.OBS_DIM), torch.float32)}
    if out is None:
      res = {k: torch.empty(*shape, dtype=dt, **kw) for k, (shape, dt) in want.items() if k != 'last_obs' or last_obs}
    else:
      if set(out) - set(want):
        raise ValueError(f'rollout_branches: out holds {sorted(set(out) - set(want))}; the keys are {list(want)}')
      res = {k: t for k, t in out.items() if t is not None}
      for k, t in res.items():
        shape, dt = want[k]
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
          raise ValueError(f'out[{k!r}] must be contiguous {dt} {shape} on {self.device}')
    if not res:
      raise ValueError('rollout_branches: nothing to compute (every key of out is missing or None)')
    if K == 0 or H == 0:                                             # (the entry point writes nothing then: no branch, or no step to reduce)
      raise ValueError(f'rollout_branches: K = {K}, H = {H}: at least one branch of at least one step')
    with self._ctx():
      act = self._actions(a, (K, H, n))
      summary = _abi.EpisodeSummary(ret=_ptr(res.get('ret')), success_last=_ptr(res.get('success')), first_success=_ptr(res.get('first_success')))
      fn = self._lib.earl_tabletop_branch_rollout if self.NOBJ == 1 else self._lib.earl_tabletop3_branch_rollout
      rc = fn(self._cfg_ref, self._st_ref, K, H, act.data_ptr(), H * n * 3, C.byref(summary), _ptr(res.get('last_obs')), self._stream())
    self._check(rc, 'branch_rollout')
    return res                                                       # (no counter advance, no step count: nothing happened to the env)

  def _plan_params(self, who, K, H, iterations, iteration0, sigma, temperature, noise_counter):
    s = torch.as_tensor(sigma, dtype=torch.float32).reshape(-1).tolist()
    if len(s) not in (1, 3):
      raise ValueError(f'{who}: sigma is a number or three, one per action dimension')
    if not temperature > 0:
      raise ValueError(f'{who}: temperature = {temperature} must be > 0')
    nc = self._cfg.counter if noise_counter is None else int(noise_counter)   # (None: the low word of the env's Philox counter -- fresh noise per control step)
    return _abi.PlanParams(K=int(K), H=int(H), iterations=int(iterations), iteration0=int(iteration0), sigma=(C.c_float * 3)(*(s * 3 if len(s) == 1 else s)),
                           noise_counter=nc & 0xFFFFFFFF, inv_temperature=1.0 / float(temperature))

  def _plan_mean(self, who, mean, horizon):
    n = self.num_envs
    if mean is None:
      if horizon is None:
        raise ValueError(f'{who}: give mean [H, N, 3] or horizon')
      return torch.zeros(int(horizon), n, 3, dtype=torch.float32, device=self.device)
    m = torch.as_tensor(mean, device=self.device)
    if m.dim() != 3 or m.shape[1] != n or m.shape[2] != 3 or (horizon is not None and m.shape[0] != horizon):
      raise ValueError(f'{who}: mean must be [H, N, 3] = [{"H" if horizon is None else horizon}, {n}, 3], got {list(m.shape)}')
    return self._actions(m, (int(m.shape[0]), n))

  def _plan_value(self, who, discount, value):
    """-> None (discount 1.0 and no value network: the value-free entry points, called exactly as before those keywords existed) or the struct earl_plan_value of
    the `_value` ones (with the network's struct kept alive beside it)"""
    if value is None and float(discount) == 1.0:
      return None
    if not (float(discount) > 0.0 and float(discount) <= 1.0):
      raise ValueError(f'{who}: discount = {discount}: 0 < discount <= 1')
    if value is None:
      return _abi.PlanValue(discount=float(discount), value=None)
    from ..policy import GaussianMLPPolicy, MLPPolicy
    if not isinstance(value, MLPPolicy) or isinstance(value, GaussianMLPPolicy):
      raise ValueError(f'{who}: value is an MLPPolicy(layers, hidden_act, out_act, obs_dim={self.OBS_DIM}, act_dim=1): a network from the observation to one number')
    require_widths(value, who, self.OBS_DIM, 1, env=self)
    if value.param_dtype != torch.float32:
      raise ValueError(f'{who}: the value network stores its parameters as {value.param_dtype}; float32 only (pass .widened())')
    if len(value.dims) == 4 and value.dims[1] > _abi.PLAN_VALUE_MAX_H1:
      raise ValueError(f'{who}: a value network of two hidden layers has a first one of at most {_abi.PLAN_VALUE_MAX_H1} (a lane holds it in registers), got '
                       f'{value.dims[1]}; one hidden layer may be 256 wide')
    pv = _abi.PlanValue(discount=float(discount), value=C.pointer(value.struct))
    pv._keep = value
    return pv

  def _plan_prior_check(self, who, prior, P, K):
    """what a policy prior must be before the call: an MLPPolicy from the observation to the three action dimensions, float32, on the env's device, no Gaussian head"""
    from ..policy import GaussianMLPPolicy, MLPPolicy
    if not isinstance(prior, MLPPolicy) or isinstance(prior, GaussianMLPPolicy):
      raise ValueError(f'{who}: prior is an MLPPolicy(layers, hidden_act, out_act, obs_dim={self.OBS_DIM}, act_dim=3) without a Gaussian head')
    require_widths(prior, who, self.OBS_DIM, 3, env=self)
    if prior.param_dtype != torch.float32:
      raise ValueError(f'{who}: the prior stores its parameters as {prior.param_dtype}; float32 only (pass .widened())')
    if len(prior.dims) == 4 and prior.dims[1] > _abi.PLAN_PRIOR_MAX_H1:
      raise ValueError(f'{who}: a prior of two hidden layers has a first one of at most {_abi.PLAN_PRIOR_MAX_H1} (a lane holds it in registers), got {prior.dims[1]}; '
                       'one hidden layer may be 256 wide')
    if P < 0 or P >= K:
      raise ValueError(f'{who}: prior_branches = {P}: 0 .. K - 1 = {K - 1} (branch 0 is the plan itself)')

  def plan_mppi(self, mean=None, horizon=None, K=64, iterations=1, sigma=0.3, temperature=1.0, iteration0=0, noise_counter=None, out=None, discount=1.0, value=None,
                prior=None, prior_branches=0, prior_sigma=0.0):
    """`iterations` MPPI iterations on the device from the CURRENT state (include/earl_tabletop.h: earl_tabletop_plan_mppi): K candidates per env -- the mean plan
    itself and K - 1 copies with clipped Gaussian noise of scale `sigma` (a number or three) -- scored as rollout_branches scores them, the mean moved to their
    average under the weights exp((ret - max ret) / temperature).  The candidates are never in memory: the noise is made inside the scoring kernel and made again
    inside the update.  mean [H, N, 3] (None: zeros of [horizon, N, 3]) -> {'plan' [H, N, 3] float32, 'ret' [K, N] float64 (the last iteration's returns),
    'ret0' [iterations, N] float64 (the return of the plan entering each iteration), 'best_ret' [N] float64, 'best_k' [N] int32 (plan_candidates(...)[best_k] is
    that candidate)}.  `noise_counter=None` takes the low 32 bits of the env's Philox counter, so successive control steps draw fresh noise; `iteration0` numbers
    the first iteration (iterations in one call == as many calls of one, numbered on).  `out`: an optional dict of preallocated tensors under the same keys; a
    key that is missing or None is not computed, except 'ret' (the workspace of the call), which is then allocated; out['plan'] may be the `mean` tensor.  The env
    is left exactly as found -- state, counters, the Philox counter.
    `discount` (0 < gamma <= 1) and `value` (an `MLPPolicy(layers, hidden_act, 'none' or 'tanh', obs_dim=D, act_dim=1)` on the env's device: V from the observation
    to one number) change the score of a candidate from the plain sum of its H rewards to  sum_t gamma^t r_t + gamma^H V(o_H)  (earl_tabletop_plan_mppi_value): the
    network is evaluated inside the scoring kernel on the last look-ahead observation of every branch, no [K, N, D] tensor and no extra launch in between.  Under
    the sparse reward that is what lets a short horizon see a goal further than H steps away.  One hidden layer may be 256 wide; of two, the first is at most
    16 (_abi.PLAN_VALUE_MAX_H1).  With both defaults the call is the value-free entry point, exactly as before.
    `prior` (an `MLPPolicy(layers, hidden_act, out_act, obs_dim=D, act_dim=3)` on the env's device, float32, no Gaussian head) makes the candidates 1 .. `prior_branches`
    closed-loop rollouts under that policy instead of noise around the mean (earl_tabletop_plan_mppi_prior): at every look-ahead step the lane that owns the branch
    evaluates the policy on the observation its own env copy just produced and adds `prior_sigma` (a number or three) times the branch's noise.  The result gains
    'prior_actions' [prior_branches, H, N, 3] float32, the actions those branches took in the last iteration (also the call's workspace: allocated when `out` leaves
    it out).  One hidden layer may be 256 wide; of two, the first is at most 16 (_abi.PLAN_PRIOR_MAX_H1).  `discount` / `value` combine with it as above.  With
    prior=None the call is the entry point it was before the keyword existed."""
    m = self._plan_mean('plan_mppi', mean, horizon)
    n, H, K, I = self.num_envs, int(m.shape[0]), int(K), int(iterations)
    pp = self._plan_params('plan_mppi', K, H, I, iteration0, sigma, temperature, noise_counter)
    kw = dict(device=self.device)
    want = {'plan': ((H, n, 3), torch.float32), 'ret': ((K, n), torch.float64), 'ret0': ((I, n), torch.float64), 'best_ret': ((n,), torch.float64),
            'best_k': ((n,), torch.int32)}
    if K < 1 or H < 1 or I < 1:
      raise ValueError(f'plan_mppi: K = {K}, H = {H}, iterations = {I}: at least one of each')
    P = int(prior_branches)
    if prior is None:
      if P != 0:
        raise ValueError(f'plan_mppi: prior_branches = {P} without a prior')
    else:
      self._plan_prior_check('plan_mppi', prior, P, K)
      want['prior_actions'] = ((P, H, n, 3), torch.float32)
    if out is None:
      res = {k: torch.empty(*shape, dtype=dt, **kw) for k, (shape, dt) in want.items()}
    else:
      if set(out) - set(want):
        raise ValueError(f'plan_mppi: out holds {sorted(set(out) - set(want))}; the keys are {list(want)}')
      res = {k: t for k, t in out.items() if t is not None}
      for k, t in res.items():
        shape, dt = want[k]
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
          raise ValueError(f'out[{k!r}] must be contiguous {dt} {shape} on {self.device}')
      if 'plan' not in res:
        raise ValueError("plan_mppi: out['plan'] is what the call computes")
      if 'ret' not in res:
        res['ret'] = torch.empty(K, n, dtype=torch.float64, **kw)
      if prior is not None and 'prior_actions' not in res:
        res['prior_actions'] = torch.empty(P, H, n, 3, dtype=torch.float32, **kw)
    pv = self._plan_value('plan_mppi', discount, value)
    with self._ctx():
      if prior is not None:
        ps = torch.as_tensor(prior_sigma, dtype=torch.float32).reshape(-1).tolist()
        if len(ps) not in (1, 3):
          raise ValueError('plan_mppi: prior_sigma is a number or three, one per action dimension')
        pr = _abi.PlanPrior(policy=C.pointer(prior.struct), branches=P, sigma=(C.c_float * 3)(*(ps * 3 if len(ps) == 1 else ps)),
                            act=res['prior_actions'].data_ptr() if P else None)
        fn = self._lib.earl_tabletop_plan_mppi_prior if self.NOBJ == 1 else self._lib.earl_tabletop3_plan_mppi_prior
        rc = fn(self._cfg_ref, self._st_ref, C.byref(pp), C.byref(pv) if pv is not None else None, C.byref(pr), m.data_ptr(), res['plan'].data_ptr(),
                res['ret'].data_ptr(), _ptr(res.get('ret0')), _ptr(res.get('best_ret')), _ptr(res.get('best_k')), self._stream())
      elif pv is None:
        fn = self._lib.earl_tabletop_plan_mppi if self.NOBJ == 1 else self._lib.earl_tabletop3_plan_mppi
        rc = fn(self._cfg_ref, self._st_ref, C.byref(pp), m.data_ptr(), res['plan'].data_ptr(), res['ret'].data_ptr(), _ptr(res.get('ret0')), _ptr(res.get('best_ret')),
                _ptr(res.get('best_k')), self._stream())
      else:
        fn = self._lib.earl_tabletop_plan_mppi_value if self.NOBJ == 1 else self._lib.earl_tabletop3_plan_mppi_value
        rc = fn(self._cfg_ref, self._st_ref, C.byref(pp), C.byref(pv), m.data_ptr(), res['plan'].data_ptr(), res['ret'].data_ptr(), _ptr(res.get('ret0')),
                _ptr(res.get('best_ret')), _ptr(res.get('best_k')), self._stream())
    self._check(rc, 'plan_mppi')
    return res                                                       # (no counter advance, no step count: nothing happened to the env)

  def plan_candidates(self, mean, K, sigma=0.3, iteration=0, noise_counter=None):
    """the K candidates of plan_mppi's iteration `iteration` around `mean` [H, N, 3], written out: [K, H, N, 3] float32, row 0 the clipped mean -- what
    rollout_branches takes (earl_tabletop_plan_candidates).  With plan_mppi's `noise_counter` (None: the env's counter, unchanged by plan_mppi) they are the
    candidates that call scored."""
    m = self._plan_mean('plan_candidates', mean, None)
    H = int(m.shape[0])
    pp = self._plan_params('plan_candidates', K, H, 1, 0, sigma, 1.0, noise_counter)
    if int(K) < 1 or H < 1:
      raise ValueError(f'plan_candidates: K = {K}, H = {H}: at least one of each')
    act = torch.empty(int(K), H, self.num_envs, 3, dtype=torch.float32, device=self.device)
    with self._ctx():
      rc = self._lib.earl_tabletop_plan_candidates(self._cfg_ref, C.byref(pp), int(iteration), m.data_ptr(), act.data_ptr(), self._stream())
    self._check(rc, 'plan_candidates')
    return act

  def _cem_params(self, who, K, H, iterations, iteration0, elites, sigma, noise_counter, alpha, std_min, std_max):
    s = torch.as_tensor(sigma, dtype=torch.float32).reshape(-1).tolist()
    if len(s) not in (1, 3):
      raise ValueError(f'{who}: sigma is a number or three, one per action dimension')
    K, E = int(K), int(elites)
    if K < 1 or K > _abi.CEM_MAX_K or E < 1 or E > K:
      raise ValueError(f'{who}: K = {K}, elites = {E}: 1 <= elites <= K <= {_abi.CEM_MAX_K}')
    if not (0.0 <= float(alpha) < 1.0) or not (0.0 <= float(std_min) <= float(std_max) < float('inf')):
      raise ValueError(f'{who}: alpha = {alpha}, std_min = {std_min}, std_max = {std_max}: 0 <= alpha < 1 and 0 <= std_min <= std_max, all finite')
    nc = self._cfg.counter if noise_counter is None else int(noise_counter)   # (None: the low word of the env's Philox counter, as plan_mppi)
    return _abi.CemParams(K=K, H=int(H), iterations=int(iterations), iteration0=int(iteration0), elites=E, sigma=(C.c_float * 3)(*(s * 3 if len(s) == 1 else s)),
                          noise_counter=nc & 0xFFFFFFFF, alpha=float(alpha), std_min=float(std_min), std_max=float(std_max))

  def plan_cem(self, mean=None, horizon=None, K=64, elites=8, iterations=1, sigma=0.3, std=None, alpha=0.0, std_min=0.0, std_max=2.0, iteration0=0, noise_counter=None,
               out=None, discount=1.0, value=None):
    """`iterations` iterations of the cross-entropy method on the device from the CURRENT state (include/earl_tabletop.h: earl_tabletop_plan_cem): K candidates per
    env -- the mean plan itself and K - 1 copies with clipped Gaussian noise of a scale per (step, env, dimension) -- scored as rollout_branches scores them; the
    `elites` best refit the mean AND the std (smoothed by `alpha`, the std kept inside [std_min, std_max]), so the search widens or narrows by itself inside the
    launch.  The candidates are never in memory; the update makes only the elites again.  mean [H, N, 3] (None: zeros of [horizon, N, 3]); std [H, N, 3] (None:
    every row `sigma`, a number or three) -> {'plan' [H, N, 3], 'std' [H, N, 3] float32, 'ret' [K, N] float64, 'ret0' [iterations, N] float64, 'best_ret' [N]
    float64, 'best_k' [N] int32 (cem_candidates(...)[best_k] is that candidate)}.  `noise_counter`, `iteration0`, `discount`, `value` and `out` are plan_mppi's;
    'plan', 'std' and 'ret' are allocated when `out` leaves them out, out['plan'] may be the `mean` tensor and out['std'] the `std` tensor.  The env is left
    exactly as found."""
    m = self._plan_mean('plan_cem', mean, horizon)
    n, H, K, I = self.num_envs, int(m.shape[0]), int(K), int(iterations)
    if H < 1 or I < 1:
      raise ValueError(f'plan_cem: H = {H}, iterations = {I}: at least one of each')
    cp = self._cem_params('plan_cem', K, H, I, iteration0, elites, sigma, noise_counter, alpha, std_min, std_max)
    s0 = None if std is None else self._plan_mean('plan_cem (std)', std, H)
    kw = dict(device=self.device)
    want = {'plan': ((H, n, 3), torch.float32), 'std': ((H, n, 3), torch.float32), 'ret': ((K, n), torch.float64), 'ret0': ((I, n), torch.float64),
            'best_ret': ((n,), torch.float64), 'best_k': ((n,), torch.int32)}
    if out is None:
      res = {k: torch.empty(*shape, dtype=dt, **kw) for k, (shape, dt) in want.items()}
    else:
      if set(out) - set(want):
        raise ValueError(f'plan_cem: out holds {sorted(set(out) - set(want))}; the keys are {list(want)}')
      res = {k: t for k, t in out.items() if t is not None}
      for k, t in res.items():
        shape, dt = want[k]
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
          raise ValueError(f'out[{k!r}] must be contiguous {dt} {shape} on {self.device}')
      if 'plan' not in res:
        raise ValueError("plan_cem: out['plan'] is what the call computes")
      for k in ('std', 'ret'):
        if k not in res:
          res[k] = torch.empty(*want[k][0], dtype=want[k][1], **kw)
    pv = self._plan_value('plan_cem', discount, value)
    with self._ctx():
      fn = self._lib.earl_tabletop_plan_cem if self.NOBJ == 1 else self._lib.earl_tabletop3_plan_cem
      rc = fn(self._cfg_ref, self._st_ref, C.byref(cp), None if pv is None else C.byref(pv), m.data_ptr(), _ptr(s0), res['plan'].data_ptr(), res['std'].data_ptr(),
              res['ret'].data_ptr(), _ptr(res.get('ret0')), _ptr(res.get('best_ret')), _ptr(res.get('best_k')), self._stream())
    self._check(rc, 'plan_cem')
    return res                                                       # (no counter advance, no step count: nothing happened to the env)

  def cem_candidates(self, mean, K, sigma=0.3, std=None, iteration=0, noise_counter=None):
    """the K candidates of plan_cem's iteration `iteration` around `mean` [H, N, 3] with the std `std` [H, N, 3] (None: `sigma`), written out: [K, H, N, 3]
    float32, row 0 the clipped mean -- what rollout_branches takes (earl_tabletop_cem_candidates).  The std is clamped into plan_cem's default [std_min, std_max] =
    [0, 2] first, so with plan_cem's `noise_counter` and those defaults they are the candidates that call scored."""
    m = self._plan_mean('cem_candidates', mean, None)
    H = int(m.shape[0])
    if H < 1:
      raise ValueError('cem_candidates: H = 0')
    cp = self._cem_params('cem_candidates', K, H, 1, 0, 1, sigma, noise_counter, 0.0, 0.0, 2.0)
    s0 = None if std is None else self._plan_mean('cem_candidates (std)', std, H)
    act = torch.empty(int(K), H, self.num_envs, 3, dtype=torch.float32, device=self.device)
    with self._ctx():
      rc = self._lib.earl_tabletop_cem_candidates(self._cfg_ref, C.byref(cp), int(iteration), m.data_ptr(), _ptr(s0), act.data_ptr(), self._stream())
    self._check(rc, 'cem_candidates')
    return act

  def rollout_mpc(self, T, plan=None, horizon=None, K=64, iterations=1, sigma=0.3, temperature=1.0, iteration0=0, noise_counter=None, out=None, discount=1.0,
                  value=None, method='mppi', elites=8, alpha=0.0, std_min=0.0, std_max=2.0):
    """T steps of receding-horizon MPPI control in ONE kernel launch (include/earl_tabletop.h: earl_tabletop_mpc_rollout): per step plan_mppi from the current
    state with the warm start, rollout of the plan's first action, the plan shifted by one step (zeroed for an env that auto-reset) -- bit for bit the loop
        for s in range(T): plan_mppi(plan, ..., out={'plan': plan}); rollout(plan[:1]); plan = cat(plan[1:], plan[-1:])
    with the env's state, the plan and the K returns on chip throughout.  plan [H, N, 3] (None: zeros of [horizon, N, 3]) -> {'obs' [T, N, D], 'reward' [T, N],
    'done' [T, N], 'success' [T, N], 'actions' [T, N, 3] (the executed ones), 'plan' [H, N, 3] (the warm start of the next call), 'ret0' [T, iterations, N]
    float64, 'best_ret' [T, N] float64}.  `noise_counter=None` takes the low 32 bits of the env's Philox counter (step s adds s), as plan_mppi does at each step
    of that loop.  `out`: an optional dict of preallocated tensors under the same keys; a key that is missing or None is not computed, except 'plan', which is
    then allocated; out['plan'] may be the `plan` tensor (the call is in place on it).  Advances the Philox counter and total_step_count by T, like rollout().
    `discount` and `value` are plan_mppi's: every planning step of the loop scores its candidates by  sum_t gamma^t r_t + gamma^H V(o_H)  with the value network
    evaluated inside the same launch (earl_tabletop_mpc_rollout_value); with both defaults the call is the value-free entry point, exactly as before.
    `method='cem'` plans every step with plan_cem instead (earl_tabletop_mpc_rollout_cem: `elites`, `alpha`, `std_min`, `std_max` are plan_cem's, the std starts
    from `sigma` at every step, `temperature` is ignored, and a `discount` / `value` other than the defaults is refused: that loop has no value build).  Under
    the default 'mppi' those four keywords must keep their defaults."""
    if method not in ('mppi', 'cem'):
      raise ValueError(f"rollout_mpc: method = {method!r}: 'mppi' or 'cem'")
    if method == 'mppi' and (elites, alpha, std_min, std_max) != (8, 0.0, 0.0, 2.0):
      raise ValueError("rollout_mpc: elites, alpha, std_min and std_max belong to method='cem'")
    n, T, K, I = self.num_envs, int(T), int(K), int(iterations)
    p0 = self._plan_mean('rollout_mpc', plan, horizon)
    H = int(p0.shape[0])
    if method == 'cem':
      if T < 1 or H < 1 or I < 1:
        raise ValueError(f'rollout_mpc: T = {T}, H = {H}, iterations = {I}: at least one of each')
      pp = self._cem_params('rollout_mpc', K, H, I, iteration0, elites, sigma, noise_counter, alpha, std_min, std_max)
      if self._plan_value('rollout_mpc', discount, value) is not None:
        raise ValueError("rollout_mpc: method='cem' takes no discount or value network (earl_tabletop_mpc_rollout_cem refuses them); compose plan_cem and rollout")
    else:
      pp = self._plan_params('rollout_mpc', K, H, I, iteration0, sigma, temperature, noise_counter)
    if T < 1 or K < 1 or H < 1 or I < 1:
      raise ValueError(f'rollout_mpc: T = {T}, K = {K}, H = {H}, iterations = {I}: at least one of each')
    if K > _abi.MPC_MAX_K or H > _abi.MPC_MAX_H:
      raise ValueError(f'rollout_mpc: K = {K}, H = {H}: at most {_abi.MPC_MAX_K} branches (one per lane of a workgroup) of {_abi.MPC_MAX_H} steps')
    pv = self._plan_value('rollout_mpc', discount, value)
    kw = dict(device=self.device)
    want = {'obs': ((T, n, self.OBS_DIM), torch.float32), 'reward': ((T, n), torch.float32), 'done': ((T, n), torch.bool), 'success': ((T, n), torch.bool),
            'actions': ((T, n, 3), torch.float32), 'plan': ((H, n, 3), torch.float32), 'ret0': ((T, I, n), torch.float64), 'best_ret': ((T, n), torch.float64)}
    if out is None:
      res = {k: torch.empty(*shape, dtype=dt, **kw) for k, (shape, dt) in want.items()}
    else:
      if set(out) - set(want):
        raise ValueError(f'rollout_mpc: out holds {sorted(set(out) - set(want))}; the keys are {list(want)}')
      res = {k: t for k, t in out.items() if t is not None}
      for k, t in res.items():
        shape, dt = want[k]
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
          raise ValueError(f'out[{k!r}] must be contiguous {dt} {shape} on {self.device}')
      if not any(k in res for k in ('obs', 'reward', 'done', 'success')):
        raise ValueError('rollout_mpc: out holds none of obs, reward, done, success')
      if 'plan' not in res:
        res['plan'] = torch.empty(H, n, 3, dtype=torch.float32, **kw)
    with self._ctx():
      if res['plan'].data_ptr() != p0.data_ptr():
        res['plan'].copy_(p0)                                          # (the entry point is in place on the plan)
      ostruct = _abi.TabletopOut(_ptr(res.get('obs')), _ptr(res.get('reward')), _ptr(res.get('done')), _ptr(res.get('success')))
      mpc = _abi.MpcOut(act=_ptr(res.get('actions')), plan=res['plan'].data_ptr(), ret0=_ptr(res.get('ret0')), best_ret=_ptr(res.get('best_ret')))
      if method == 'cem':
        fn = self._lib.earl_tabletop_mpc_rollout_cem if self.NOBJ == 1 else self._lib.earl_tabletop3_mpc_rollout_cem
        rc = fn(self._cfg_ref, self._st_ref, C.byref(pp), None, T, C.byref(ostruct), C.byref(mpc), self._stream())
      elif pv is None:
        fn = self._lib.earl_tabletop_mpc_rollout if self.NOBJ == 1 else self._lib.earl_tabletop3_mpc_rollout
        rc = fn(self._cfg_ref, self._st_ref, C.byref(pp), T, C.byref(ostruct), C.byref(mpc), self._stream())
      else:
        fn = self._lib.earl_tabletop_mpc_rollout_value if self.NOBJ == 1 else self._lib.earl_tabletop3_mpc_rollout_value
        rc = fn(self._cfg_ref, self._st_ref, C.byref(pp), C.byref(pv), T, C.byref(ostruct), C.byref(mpc), self._stream())
    self._check(rc, 'mpc_rollout')
    self._cfg.counter += T                                             # real step s used counter + s (its look-ahead step t: counter + s + t)
    self.total_step_count += T
    if 'success' in res:
      self._last_success = res['success'][-1]
    return res

  def _observe(self, want=('obs',)):
    kw = dict(device=self.device)
    n = self.num_envs
    obs = torch.empty(n, self.OBS_DIM, dtype=torch.float32, **kw) if 'obs' in want else None
    rew = torch.empty(n, dtype=torch.float32, **kw) if 'reward' in want else None
    succ = torch.empty(n, dtype=torch.bool, **kw) if 'success' in want else None
    if self.NOBJ == 1:
      out = _abi.TabletopOut(_ptr(obs), _ptr(rew), None, _ptr(succ))
      with self._ctx():
        self._check(self._lib.earl_tabletop_observe(C.byref(self._cfg), C.byref(self._st), C.byref(out), self._stream()), 'observe')
    else:
      # 3obj: obs through a no-op masked reset, reward/success through the pure reward kernel
      with self._ctx():
        o = torch.empty(n, self.OBS_DIM, dtype=torch.float32, **kw)
        zero = torch.zeros(n, dtype=torch.uint8, **kw)
        self._check(self._lib.earl_tabletop3_reset(C.byref(self._cfg), C.byref(self._st), zero.data_ptr(), o.data_ptr(), self._stream()), 'observe')
        if rew is not None or succ is not None:
          self._check(self._lib.earl_tabletop3_reward(n, o.data_ptr(), self._cfg.reward_type, _ptr(rew), _ptr(succ), self._stream()), 'reward')
        obs = o if obs is not None else None
    return obs, rew, succ

  def _get_obs(self):
    obs = self._observe(('obs',))[0]
    return obs[0].cpu().numpy() if self.scalar_api else obs

  def get_obs(self):
    return self._get_obs()

  def compute_reward(self, obs):
    """compute_reward(obs) of the reference on an observation batch [M, D] (any M)."""
    r, _ = self._reward(obs, want_reward=True, want_success=False)
    return float(r[0]) if self.scalar_api and r.numel() == 1 else r

  def is_successful(self, obs=None):
    if obs is None:
      s = self._observe(('success',))[2]
    else:
      _, s = self._reward(obs, want_reward=False, want_success=True)
    return bool(s[0]) if self.scalar_api and s.numel() == 1 else s

  def _reward(self, obs, want_reward, want_success):
    o = torch.as_tensor(obs, device=self.device).to(torch.float32).reshape(-1, self.OBS_DIM).contiguous()
    m = o.shape[0]
    r = torch.empty(m, dtype=torch.float32, device=self.device) if want_reward else None
    s = torch.empty(m, dtype=torch.bool, device=self.device) if want_success else None
    with self._ctx():
      if self.NOBJ == 1:
        rc = self._lib.earl_tabletop_reward(m, o.data_ptr(), self._cfg.reward_type, self._cfg.wide_init, _ptr(r), _ptr(s), self._stream())
      else:
        rc = self._lib.earl_tabletop3_reward(m, o.data_ptr(), self._cfg.reward_type, _ptr(r), _ptr(s), self._stream())
    self._check(rc, 'reward')
    return r, s

  # ------------------------------------------------------------------ goals / state injection
  def get_next_goal(self):
    """Sample a goal per env (uniform over the task list, Philox keyed by global env id) WITHOUT setting it."""
    idx = self._sample_goal_rows()
    g = self.goal_table[idx.long()]
    return g[0].cpu().numpy() if self.scalar_api else g

  def _sample_goal_rows(self):
    # same draw layout as the kernels: block(draw=0)[0] * n_sample >> 32; done through a masked-out reset on a scratch copy
    scratch = TabletopStateScratch(self)
    return scratch.sample()

  def reset_goal(self, goal=None, mask=None):
    """reset_goal(goal=None) (:78-81).  goal None -> resample; a [D]-vector -> every (masked) env; [N, D] -> per env."""
    sel = slice(None) if mask is None else torch.as_tensor(mask, device=self.device).bool()
    if goal is None:
      idx = self._sample_goal_rows()
      self.goal_idx[sel] = idx[sel]
      return
    g = torch.as_tensor(np.asarray(goal) if not torch.is_tensor(goal) else goal, device=self.device).to(torch.float64)
    if g.ndim == 1:
      g = g.expand(self.num_envs, -1)
    if g.shape != (self.num_envs, self._goal_width):
      raise ValueError(f'goal must have shape [{self._goal_width}] or [{self.num_envs}, {self._goal_width}]')
    # custom goals live in per-env rows appended after the sampled rows
    base = self._n_sample_goals
    if self.goal_table.shape[0] != base + self.num_envs:
      cur = self.goal_table[self.goal_idx.long()]
      self.goal_table = torch.cat([self.goal_table[:base], cur], 0).contiguous()
      self.goal_idx.copy_(torch.arange(base, base + self.num_envs, device=self.device, dtype=torch.int32))
      self._sync_state_ptrs()
    rows = torch.arange(base, base + self.num_envs, device=self.device)
    self.goal_table[rows[sel]] = g[sel]
    self.goal_idx[sel] = rows[sel].to(torch.int32)

  @property
  def goal(self):
    g = self.goal_table[self.goal_idx.long()]
    return g[0].cpu().numpy() if self.scalar_api else g

  @property
  def attached_object(self):
    """(-1,-1) free / (0,0) holding, like the reference (scalar API); the int8 tensor otherwise."""
    if self.scalar_api:
      k = int(self.attached[0])
      return (-1, -1) if k < 0 else (0.5 * k, 0.5 * k) if self.NOBJ > 1 else (0, 0)
    return self.attached

  def set_state(self, qpos, qvel=None):
    """set_state(qpos) (:83-87): overwrite the gripper/mug coordinates (only the first NQ entries are used)."""
    del qvel
    q = torch.as_tensor(np.asarray(qpos) if not torch.is_tensor(qpos) else qpos, device=self.device).to(torch.float64)
    q = q.reshape(-1, q.shape[-1])[:, :self.NQ]
    self.qpos.copy_(q.expand(self.num_envs, -1))

  # ------------------------------------------------------------------ checkpoint / counters
  def state_dict(self):
    sd = {'qpos': self.qpos.clone(), 'attached': self.attached.clone(), 'goal_idx': self.goal_idx.clone(),
          'goal_table': self.goal_table.clone(), 'steps_since_reset': self.steps_since_reset.clone(),
          'interventions': self.interventions.clone(), 'steps_since_goal_change': self.steps_since_goal_change.clone(),
          'lifelong_return': self.lifelong_return_t.clone(), 'total_step_count': self.total_step_count,
          'rng_counter': int(self._cfg.counter), 'seed': int(self._cfg.seed)}
    if self.agent_phase is not None:                                 # the agent pair's state, once a pair launch has created it -- and only then
      sd['agent_phase'], sd['steps_in_phase'] = self.agent_phase.clone(), self.steps_in_phase.clone()
    return sd

  def load_state_dict(self, sd):
    self.goal_table = sd['goal_table'].to(self.device).clone().contiguous()
    for name, key in (('qpos', 'qpos'), ('attached', 'attached'), ('goal_idx', 'goal_idx'),
                      ('steps_since_reset', 'steps_since_reset'), ('interventions', 'interventions'),
                      ('steps_since_goal_change', 'steps_since_goal_change'), ('lifelong_return_t', 'lifelong_return')):
      getattr(self, name).copy_(sd[key])
    self.total_step_count = int(sd['total_step_count'])
    self._cfg.counter = int(sd['rng_counter'])
    self._cfg.seed = int(sd['seed'])
    if 'agent_phase' in sd:
      self.agent_phase = sd['agent_phase'].to(self.device).clone().contiguous()
      self.steps_in_phase = sd['steps_in_phase'].to(self.device).clone().contiguous()
    elif self.agent_phase is not None:                               # a checkpoint from before any pair launch: every env is the forward agent's
      self.agent_phase.zero_()
      self.steps_in_phase.zero_()
    self._sync_state_ptrs()


class TabletopStateScratch:
  """Draws goal rows with the reset kernel on throw-away state (keeps get_next_goal() side-effect free)."""

  def __init__(self, env):
    self.env = env

  def sample(self):
    e = self.env
    n, dev = e.num_envs, e.device
    st = _abi.TabletopState()
    qpos = torch.empty(n, e.NQ, dtype=torch.float64, device=dev)
    att = torch.empty(n, dtype=torch.int8, device=dev)
    gi = torch.empty(n, dtype=torch.int32, device=dev)
    steps = torch.empty(n, dtype=torch.int32, device=dev)
    iv = torch.zeros(n, dtype=torch.int32, device=dev)
    sgc = torch.empty(n, dtype=torch.int32, device=dev)
    lr = torch.empty(n, dtype=torch.float64, device=dev)
    st.qpos, st.attached, st.goal_idx, st.goal_table = qpos.data_ptr(), att.data_ptr(), gi.data_ptr(), e.goal_table.data_ptr()
    st.steps_since_reset, st.num_interventions = steps.data_ptr(), iv.data_ptr()
    st.steps_since_goal_change, st.lifelong_return = sgc.data_ptr(), lr.data_ptr()
    cfg = _abi.TabletopCfg.from_buffer_copy(e._cfg)
    cfg.wide_init, cfg.reset_at_goal = 0, 0
    with e._ctx():
      if e.NOBJ == 1:
        rc = e._lib.earl_tabletop_reset(C.byref(cfg), C.byref(st), None, None, None, e._stream())
      else:
        rc = e._lib.earl_tabletop3_reset(C.byref(cfg), C.byref(st), None, None, e._stream())
    e._check(rc, 'sample_goal')
    e._next_counter()
    return gi


class StepGraph:
  """T gym-style `step()` launches of one env batch captured once into a HIP graph and replayed with a single host call: the closed-loop
  counterpart of `rollout()` (which needs all T actions up front).  One replay costs one graph launch instead of T x (ctypes call +
  argument marshalling + kernel launch): at N = 4096 the per-step wall time drops from ~14 us to about the kernel's own ~4 us.

    g = env.make_step_graph(T)                  # action ring: the caller (or its own captured kernels) fills g.actions[t] before replay
    g = env.make_step_graph(T, policy=pi)       # pi(obs [N, D]) -> actions [N, 3] is captured INTO the graph between the steps: step t
                                                #   consumes pi(observation of step t - 1); `g.obs_in` holds the observation the first
                                                #   step of a replay starts from and is refreshed by the graph's last node
    g.replay()                                  # obs / reward / done / success of the T steps are in g.obs[t], g.reward[t], ...

  Each captured step is exactly `step()` (same kernel, same state tensors), so a replay is bit-identical to T eager calls -- also with lifelong goal
  switching (the reference's train-env loop, wrappers/lifelong_wrapper.py:30-44) and auto-reset, whose draws use the launch's Philox counter: a kernel
  ARGUMENT would be frozen at capture time, so the captured launch of step t carries the OFFSET t and adds a base it reads from one device word
  (earl_tabletop_state.counter_base), which replay() refreshes from the env's counter before every replay."""

  def __init__(self, env, T, policy=None):
    u = env.unwrapped if hasattr(env, 'unwrapped') else env
    if u.scalar_api:
      raise ValueError('make_step_graph is for the batched API (scalar_api=False)')
    if u.device.type != 'cuda':
      raise ValueError('make_step_graph captures HIP launches: device="cuda" only')
    self.env, self.T, self.policy = u, int(T), policy
    n, dev = u.num_envs, u.device
    with torch.cuda.device(dev):
      self.actions = torch.zeros(self.T, n, 3, dtype=torch.float32, device=dev)
      (self.obs, self.reward, self.done, self.success), _ = u._new_out((self.T, n))
      self.obs_in = u._observe(('obs',))[0].clone()
      structs = [_abi.TabletopOut(self.obs[t].data_ptr(), self.reward[t].data_ptr(), self.done[t].data_ptr(), self.success[t].data_ptr())
                 for t in range(self.T)]
      step_fn = u._lib.earl_tabletop_step if u.NOBJ == 1 else u._lib.earl_tabletop3_step
      self.counter_dev = torch.zeros(1, dtype=torch.int64, device=dev)      # the Philox counter of the replay's first step (two's complement of the uint64)
      host_counter = int(u._cfg.counter)

      def launch(t):
        u._cfg.counter = t                                     # the captured launch draws with *counter_base + t
        if u.NOBJ == 1:
          rc = step_fn(u._cfg_ref, u._st_ref, self.actions[t].data_ptr(), None, C.byref(structs[t]), u._stream())
        else:
          rc = step_fn(u._cfg_ref, u._st_ref, self.actions[t].data_ptr(), C.byref(structs[t]), u._stream())
        if rc:
          _abi.check(rc, 'step (graph capture)')
      if policy is not None:                                   # warm the policy up outside the capture (lazy library initialisation)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
          policy(self.obs_in)
        torch.cuda.current_stream(dev).wait_stream(side)
      self.graph = torch.cuda.CUDAGraph()
      u._st.counter_base = self.counter_dev.data_ptr()
      try:
        with torch.cuda.graph(self.graph):
          prev = self.obs_in
          for t in range(self.T):
            if policy is not None:
              self.actions[t].copy_(policy(prev).to(torch.float32).reshape(n, 3))
            launch(t)
            prev = self.obs[t]
          if policy is not None:
            self.obs_in.copy_(self.obs[self.T - 1])
      finally:                                                 # eager calls keep the counter as their argument
        u._st.counter_base = None
        u._cfg.counter = host_counter

  def replay(self):
    """run the T captured steps (asynchronous, on torch's current stream); -> (obs, reward, done, {'success': success}), each [T, N, ...]"""
    u = self.env
    c = int(u._cfg.counter)
    self.counter_dev.fill_(c - (1 << 64) if c >= (1 << 63) else c)
    self.graph.replay()
    u._cfg.counter += self.T
    u.total_step_count += self.T
    u._last_success = self.success[-1]
    return self.obs, self.reward, self.done, {'success': self.success}

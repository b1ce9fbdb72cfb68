"""What the stepper envs (`SawyerDoor` and through it `SawyerPeg`, `Minitaur`, `Kitchen`) share on the host: the output dict and its ctypes struct, the hooks of
`PhysicsStepGraph` and of `physics_policy_rollout`, the closed-loop methods, goal / state access and checkpointing.  A subclass keeps what is its own -- `__init__`,
`reset`, `step`, `rollout`, `_graph_step`, `_launch_policy`, `_get_obs_t`, reward / success, goal sampling -- and states what differs as class data (below).  The
tabletop is not one of these: its API returns tuples, carries an episode axis and folds resets into launches (envs/tabletop.py)."""
import contextlib

import torch

from . import physics_policy_rollout as closed_loop
from .physics_step_graph import PhysicsStepGraph


class PhysicsEnv:
  # ------------------------------------------------------------------ the subclass's data
  ENV = None                          # the env as its messages name it: 'the minitaur', 'the kitchen'
  OBS_DIM = ACT_DIM = None            # the widths of an observation row and of an action row
  _OUT_STRUCT = None                  # _abi.SawyerOut / MinitaurOut / KitchenOut: obs, reward, done, success, status (the door's has 'info' on top, its override)
  _REWARD_DTYPE = torch.float64       # (the door's and the peg's reward rows are float32)
  _BOUNDED = None                     # require_widths(bounded=): the bound outside which the reference raises on an action (the minitaur), None where it clips
  _POLICY_TAKES_POPULATION = False    # rollout_policy takes a PolicyPopulation (the door and the peg, whose require_widths message also names their rollout_agents)
  # the lifelong goal switch against a closed-loop launch.  Where the kernel makes it (door, peg, minitaur) only a pair refuses it, after the width check: 'not under
  # {_PAIR_LIFELONG}'.  Where the host makes it (the kitchen: _HOST_LIFELONG) every closed-loop launch refuses it, and scalar_api, before the width check
  _PAIR_LIFELONG = 'a LifelongWrapper'
  _HOST_LIFELONG = False
  _GRAPH_COUNTER = 'step_counter'     # the cfg field a captured step overwrites with its offset t (the kitchen: 'counter'); _graph_capture restores it
  _graph_bounds = None                # (lo, hi) outside which PhysicsStepGraph flags an action (the minitaur), None where the reference clips silently
  _STATE = ()                         # the tensors of state_dict()
  _STALE_WITHOUT_ROW = False          # load_state_dict of a dict without 'last_obs_stale': stale if it has no 'last_obs' either (the door), else not stale

  # what a fresh env starts from (an instance attribute takes over at the first write)
  agent_phase = steps_in_phase = None # the agent pair's per-env state (a pair launch allocates it: 0 forward / 1 reset, steps spent in the phase)
  backward_row = None                 # [N] int32 once a pair launch has drawn from a table of backward goals: the row each env's reset goal came from, -1 = none yet
  _pair_counts = None
  _last_obs_stale = False             # last_obs no longer describes (state, goal): set by set_state() / reset_goal(), cleared by whatever rewrites every row
  total_step_count = 0

  # ------------------------------------------------------------------ the subclass's own
  def reset(self, mask=None):
    raise NotImplementedError

  def _get_obs_t(self):
    raise NotImplementedError

  def _graph_step(self, t, action, out, clock):
    raise NotImplementedError

  def _launch_policy(self, policy, head, obs0, T, out, summary=None, pair=None):
    raise NotImplementedError

  # ------------------------------------------------------------------ internals
  @property
  def unwrapped(self):
    return self

  def _stream(self):
    return torch.cuda.current_stream(self.device).cuda_stream

  def _new_out(self, lead):
    """the output dict of a launch: obs [*lead, N, OBS_DIM] float64, reward / done / success / status [*lead, N]"""
    n, kw = self.num_envs, dict(device=self.device)
    return dict(obs=torch.empty(*lead, n, self.OBS_DIM, dtype=torch.float64, **kw), reward=torch.empty(*lead, n, dtype=self._REWARD_DTYPE, **kw),
                done=torch.empty(*lead, n, dtype=torch.bool, **kw), success=torch.empty(*lead, n, dtype=torch.bool, **kw),
                status=torch.empty(*lead, n, dtype=torch.uint8, **kw))

  def _out_struct(self, out):
    """the ctypes out struct of `out`: a missing (or None) key is a NULL pointer, which the closed-loop entry points take for 'this row is not kept'"""
    g = out.get
    obs, reward, done, success, status = g('obs'), g('reward'), g('done'), g('success'), g('status')
    return self._OUT_STRUCT(obs=None if obs is None else obs.data_ptr(), reward=None if reward is None else reward.data_ptr(),
                            done=None if done is None else done.data_ptr(), success=None if success is None else success.data_ptr(),
                            status=None if status is None else status.data_ptr())

  # ------------------------------------------------------------------ hooks of PhysicsStepGraph (one captured step: the subclass's _graph_step)
  def make_step_graph(self, T, policy=None):
    """Closed-loop stepping without the per-call host cost: T step() launches captured into a HIP graph, replayed with one host call (see `PhysicsStepGraph`, which
    says what each env's graph holds and refuses)."""
    return PhysicsStepGraph(self, T, policy)

  def _graph_check(self):
    pass

  def _new_graph_out(self, T):
    return self._new_out((T,))

  @contextlib.contextmanager
  def _graph_capture(self):
    c = getattr(self._cfg, self._GRAPH_COUNTER)
    try:
      yield
    finally:
      setattr(self._cfg, self._GRAPH_COUNTER, c)

  def _graph_clock(self):
    return self._counter, self.total_step_count

  def _graph_advance(self, T, out):
    self.total_step_count += T
    self._last_obs_stale = False
    self._last_success = out['success'][-1]

  def _graph_info(self, out):
    raise NotImplementedError

  # ------------------------------------------------------------------ closed loop, the policy inside the rollout kernel (physics_policy_rollout)
  def _check_policy(self, policy, who, population=False):
    """-> is it Gaussian; `policy`: an MLPPolicy / GaussianMLPPolicy of OBS_DIM -> ACT_DIM on this env's device (bounded where _BOUNDED says so); population=True
    (rollout_population, evaluate_population; everywhere with _POLICY_TAKES_POPULATION): or a PolicyPopulation of them whose members cover this env's global ids"""
    from ..policy import AgentPair, PolicyPopulation, require_widths
    if not self._POLICY_TAKES_POPULATION:
      if isinstance(policy, PolicyPopulation) and not population:
        raise NotImplementedError(f'{who}: a PolicyPopulation on {self.ENV} goes to rollout_population / evaluate_population ({who} takes one MLPPolicy / '
                                  'GaussianMLPPolicy per launch)')
      if isinstance(policy, AgentPair):
        raise NotImplementedError(f'{who}: an AgentPair on {self.ENV} goes to rollout_pair / evaluate_pair ({who} takes one policy per env and launch)')
    if self._HOST_LIFELONG:
      self._refuse_host_side(who)
    return require_widths(policy, who, self.OBS_DIM, self.ACT_DIM, env=self, bounded=self._BOUNDED)

  def _check_pair(self, pair, who):
    """-> is it Gaussian; `pair`: an AgentPair or a PairPopulation of OBS_DIM -> ACT_DIM on this env's device (bounded where _BOUNDED says so), and no LifelongWrapper"""
    from ..policy import require_widths
    if self._HOST_LIFELONG:
      self._refuse_host_side(who)
    gaussian = require_widths(pair, who, self.OBS_DIM, self.ACT_DIM, env=self, pair=True, bounded=self._BOUNDED, pairs=True)
    if self._cfg.goal_change_frequency > 0:
      raise ValueError(f'{who}: the agent pair IS the lifelong mechanism (the forward handover makes the lifelong switch\'s goal draw): '
                       f'not under {self._PAIR_LIFELONG}, whose clock would fight the pair\'s over the same draw')
    return gaussian

  def _refuse_host_side(self, who):
    if self.scalar_api:
      raise ValueError(f'{who}: scalar_api returns one env\'s numpy rows; the closed-loop launch returns batched tensors ({type(self).__name__}(..., scalar_api=False))')
    if int(self._cfg.goal_change_frequency) > 0:
      raise ValueError(f'{who}: {self.ENV}\'s lifelong goal switch runs on the host (goal_change_frequency > 0) and cannot happen inside the launch, as make_step_graph says')

  def rollout_policy(self, policy, T, reset_first=False, sample=True, return_noise=False, out=None):
    """physics_policy_rollout's closed loop (its docstring is the contract) on the env's population entry point without a population: `policy` -- an `MLPPolicy` or a
    `GaussianMLPPolicy` built with obs_dim=OBS_DIM, act_dim=ACT_DIM (where _BOUNDED is set with a bounded output: out_act='tanh' / squash=True; elsewhere the env
    clips), evaluated by the lanes that own the env; with _POLICY_TAKES_POPULATION also a `PolicyPopulation` of them.  The policy sees the observation rows as
    emitted (the kitchen's with sensor noise: after set_state() / reset_goal() its first observation is a fresh reading, one noise draw more).
    -> rollout()'s dict plus 'actions' [T, N, ACT_DIM] and, with return_noise=True, 'eps' [T, N, ACT_DIM]"""
    return closed_loop.rollout_policy(self, policy, T, reset_first, sample, return_noise, out)

  def rollout_population(self, pop, T, reset_first=False, sample=True, return_noise=False, out=None):
    """rollout_policy for a `PolicyPopulation(..., obs_dim=OBS_DIM, act_dim=ACT_DIM)`: the env with global id g runs member g // envs_per_policy, every member in
    the ONE launch (physics_policy_rollout.rollout_population).  -> rollout_policy's dict"""
    return closed_loop.rollout_population(self, pop, T, reset_first, sample, return_noise, out)

  def evaluate_population(self, policy_or_pop, T, episodes=1, sample=False, reset_first=True):
    """physics_policy_rollout.evaluate (its docstring is the contract): per-env episode summaries of one policy or of a `PolicyPopulation`, no tensor with a T axis.
    -> {'ret', 'success', 'first_success', 'guard_steps'}, each [episodes, N]"""
    return closed_loop.evaluate(self, 'evaluate_population', policy_or_pop, T, episodes, sample, reset_first)

  def rollout_pair(self, pair, T, reset_first=False, sample=True, return_noise=False, out=None):
    """physics_policy_rollout.rollout_pair (its docstring is the contract) on the env's agents entry point: `pair` -- an `AgentPair(..., obs_dim=OBS_DIM,
    act_dim=ACT_DIM)` or a `PairPopulation` of them.  A goal row has the width of `goal_t`; backward_goal='initial' is the one row of `initial_states` where there is
    one, 'initial_states' the whole table; entering the forward phase the goal becomes a row of the env's forward goals.  Not under a LifelongWrapper.
    -> rollout_policy()'s dict plus 'agent' [T, N] int8 and, with a table of backward goals, 'backward_row' [T, N] int32"""
    return closed_loop.rollout_pair(self, pair, T, reset_first, sample, return_noise, out)

  def evaluate_pair(self, pair, T, sample=True):
    """physics_policy_rollout.evaluate_pair: T steps of `pair` from the current state with per-env summaries only.
    -> {'ret', 'success', 'first_success', 'guard_steps', 'forward_success', 'backward_success'}, each [N]"""
    return closed_loop.evaluate_pair(self, pair, T, sample)

  def rollout_agents(self, pair, T, **kw):
    raise NotImplementedError(f'rollout_agents: an AgentPair on {self.ENV} goes to rollout_pair / evaluate_pair (rollout_agents is the tabletop\'s, the Sawyer door\'s '
                              'and the Sawyer peg\'s name for it)')

  def evaluate_policy(self, policy, T, **kw):
    raise NotImplementedError(f'evaluate_policy: episode summaries on {self.ENV} are evaluate_population\'s (it takes one policy as well as a PolicyPopulation); '
                              'evaluate_policy runs on the tabletop, the Sawyer door and the Sawyer peg')

  def rollout_branches(self, actions, K=None, clock=None, **kwargs):      # (kwargs: discount=, value= and prior= / prior_branches= / prior_sigma= of the envs that have the launch are refused like the rest)
    raise NotImplementedError(f'rollout_branches: scoring K action plans from the current state is not built for {self.ENV or type(self).__name__} '
                              '(it runs on the tabletops, the Sawyer door and the Sawyer peg)')

  def _no_planner(self, who):
    return NotImplementedError(f'{who}: the MPPI planner is not built for {self.ENV or type(self).__name__} (it runs on the tabletops, the Sawyer door and the Sawyer peg)')

  def plan_mppi(self, *args, **kwargs):
    raise self._no_planner('plan_mppi')

  def plan_candidates(self, *args, **kwargs):
    raise self._no_planner('plan_candidates')

  def mpc_rollout(self, *args, **kwargs):
    raise self._no_planner('mpc_rollout')

  def _no_cem(self, who):
    return NotImplementedError(f'{who}: the CEM planner is not built for {self.ENV or type(self).__name__} (it runs on the tabletops, the Sawyer door and the Sawyer peg)')

  def plan_cem(self, *args, **kwargs):
    raise self._no_cem('plan_cem')

  def cem_candidates(self, *args, **kwargs):
    raise self._no_cem('cem_candidates')

  @property
  def pair_counts(self):
    """(forward_success, backward_success) [N] int32 of the last pair launch: the phases that ended by success; None before the first"""
    return self._pair_counts

  # ------------------------------------------------------------------ goals and state access
  def reset_goal(self, goal=None, mask=None):
    g = torch.as_tensor(self.get_next_goal() if goal is None else goal, dtype=torch.float64, device=self.device).expand_as(self.goal_t)
    if mask is None:
      self.goal_t.copy_(g)
    else:
      m = torch.as_tensor(mask, device=self.device).bool()
      self.goal_t[m] = g[m]
    self._last_obs_stale = True                            # (last_obs carries the old goal entries: a closed-loop launch computes its first observation anew)

  @property
  def goal(self):
    return self.goal_t[0].cpu().numpy() if self.scalar_api else self.goal_t

  def set_state(self, qpos, qvel):
    self._last_obs_stale = True                            # (last_obs no longer belongs to the state: a closed-loop launch computes its first observation anew)
    self.qpos.copy_(torch.as_tensor(qpos, dtype=torch.float64, device=self.device).reshape(self.qpos.shape))
    self.qvel.copy_(torch.as_tensor(qvel, dtype=torch.float64, device=self.device).reshape(self.qvel.shape))

  def state_dict(self):
    return {k: getattr(self, k).clone() for k in self._STATE} | {'counter': int(self._counter), 'total_step_count': self.total_step_count,
                                                                 'last_obs_stale': bool(self._last_obs_stale)} | closed_loop.pair_state_dict(self)

  def load_state_dict(self, sd):
    """the keys of `sd` that are this env's: a dict without a tensor leaves the env's own (so does one without the pair's, which are in it once a pair launch has
    allocated them); one written before 'last_obs_stale' existed: see _STALE_WITHOUT_ROW"""
    for k in self._STATE:
      if k in sd:
        getattr(self, k).copy_(sd[k])
    closed_loop.load_pair_state(self, sd)
    if 'counter' in sd:
      self._counter = int(sd['counter'])
    if 'total_step_count' in sd:
      self.total_step_count = int(sd['total_step_count'])
    self._last_obs_stale = bool(sd.get('last_obs_stale', self._STALE_WITHOUT_ROW and 'last_obs' not in sd))

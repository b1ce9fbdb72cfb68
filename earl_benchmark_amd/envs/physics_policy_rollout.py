"""The closed loop of the stepper envs (door, peg, minitaur, kitchen): what the envs share around the ONE launch of their rollout kernel with a policy inside it
(include/earl_physics.h: earl_{sawyer,minitaur,kitchen}_population_rollout and earl_{sawyer,minitaur,kitchen}_agents_rollout), next to `PhysicsStepGraph`.  Every
function below takes the env and serves all of them; the env's side is ONE set of hooks, held by `PhysicsEnv` (envs/physics_env.py) unless said otherwise:
  `_check_policy(policy, who, population=False)` -> is it Gaussian (policy.require_widths with the env's widths and rules, the subclass's class data; population=True:
      a PolicyPopulation is taken as well, its members checked against the env's global ids -- the Sawyer envs take one everywhere);
  `_check_pair(pair, who)` -> is it Gaussian, for an AgentPair or a PairPopulation;
  `_launch_policy(policy, head, obs0, T, out, summary=None, pair=None)`, the subclass's: the launch itself.  `out` may lack any key, 'obs' included (the env's row of
      last_obs then carries the observation); summary: None or an _abi.EpisodeSummary; pair: None, or what `pair_structs` returns;
  `_new_out((T,))`, and optionally `_new_pair_out((T,))` where a pair launch offers other keys (the door: no 'info'); the subclass's `reset()` and `_get_obs_t()`;
      `last_obs` / `_last_obs_stale`; the pair's state `agent_phase` / `steps_in_phase` / `backward_row` (None until `pair_structs` allocates it) and `_pair_counts`.
The public names differ by env for history's sake -- the Sawyer envs' rollout_agents / evaluate_agents / evaluate_policy are rollout_pair / evaluate_pair / evaluate
here -- so each takes `who`, the name its messages carry.

What rollout_policy promises, for every such env (A = the env's action width): closed loop in ONE launch of the rollout kernel, `policy` evaluated between the env
steps by the lanes that own the env: observation -> float32 MLP -> action -> env step.
-> rollout()'s dict plus 'actions' [T, N, A] float32 (as the policy produced them) and, with return_noise=True, 'eps' [T, N, A] (the standard-normal draws as used).
Bit-identical to rollout(out['actions']) from the same state.  The first action is computed from the observation the env last returned (`last_obs`: the row the
previous step / rollout / reset emitted, goal entries as patched, so T launches of one step equal one launch of T); after set_state() or reset_goal() that row no
longer describes the env, and the observation of the current state and goal (_get_obs()) is computed instead.  reset_first=True calls reset() before (a launch of
its own).  A Gaussian policy is sampled inside the kernel (sample=True: tanh(mean + exp(log_std) eps), eps from the env's Philox stream keyed by seed, global env
id and step counter) or evaluated at its mean (sample=False); both flags are for Gaussian policies only."""
import torch


def prepare(env, who, policy, gaussian, T, reset_first, sample, return_noise, out, what='a GaussianMLPPolicy (an MLPPolicy is deterministic)', new_out=None):
  """the rules of sample / return_noise / T, the reset, the outputs ('actions' and 'eps' added to `out`, or to a new dict: new_out((T,)), the env's _new_out unless
  given), the head and the first observation -> (T, out, head, obs0)"""
  if not gaussian and (return_noise or not sample):
    raise ValueError(f'{who}: sample=False / return_noise=True need {what}')
  T = int(T)
  if T < 1:
    raise ValueError(f'{who}: T = {T} < 1')
  if reset_first:
    env.reset()
  n, A = env.num_envs, env.action_space.shape[0]
  with torch.cuda.device(env.device):
    out = out if out is not None else (new_out or env._new_out)((T,))
    for k in ('actions',) + (('eps',) if return_noise else ()):
      if k not in out:
        out[k] = torch.empty(T, n, A, dtype=torch.float32, device=env.device)
    obs0 = (env._get_obs_t() if env._last_obs_stale else env.last_obs).contiguous()
  head = policy.head(sample=bool(sample), eps_out=out['eps'] if return_noise else None) if gaussian else None
  return T, out, head, obs0


def finish(env, T, rewards, success):
  """the bookkeeping after T env steps of every env; rewards: the steps' [T, N] (or their float64 sums [N]), success: the last step's [N]"""
  env.total_step_count += T
  if int(env._cfg.goal_change_frequency) > 0:
    env.lifelong_return_t += rewards.reshape(-1, env.num_envs).sum(0, dtype=torch.float64)
  env._last_success = success
  env._last_obs_stale = False                              # (every env's last_obs row was rewritten)


def rollout_policy(env, policy, T, reset_first=False, sample=True, return_noise=False, out=None):
  gaussian = env._check_policy(policy, 'rollout_policy')
  T, out, head, obs0 = prepare(env, 'rollout_policy', policy, gaussian, T, reset_first, sample, return_noise, out)
  env._launch_policy(policy, head, obs0, T, out)
  finish(env, T, out['reward'], out['success'][-1])
  return out


def rollout_population(env, pop, T, reset_first=False, sample=True, return_noise=False, out=None):
  """rollout_policy for a `PolicyPopulation` of the env's widths: the env with global id g runs member g // envs_per_policy, all members in the ONE launch
  (include/earl_physics.h: earl_minitaur_population_rollout / earl_kitchen_population_rollout).  Same dict, same bookkeeping; bit-identical to cutting the batch at
  the member boundaries and running rollout_policy on each piece with that member."""
  from ..policy import PolicyPopulation
  if not isinstance(pop, PolicyPopulation):
    raise ValueError('rollout_population: pop is a PolicyPopulation (one MLPPolicy / GaussianMLPPolicy goes to rollout_policy)')
  gaussian = env._check_policy(pop, 'rollout_population', population=True)
  T, out, head, obs0 = prepare(env, 'rollout_population', pop, gaussian, T, reset_first, sample, return_noise, out,
                               what='a population of GaussianMLPPolicy (MLPPolicy members are deterministic)')
  env._launch_policy(pop, head, obs0, T, out)
  finish(env, T, out['reward'], out['success'][-1])
  return out


def evaluate(env, who, policy, T, episodes=1, sample=False, reset_first=True):
  """`episodes` evaluation episodes of `policy` -- an MLPPolicy, a GaussianMLPPolicy (sample=False: at its mean) or a `PolicyPopulation` -- each a reset() launch plus
  ONE launch of the rollout kernel that writes only per-env summaries (`actions` and every `out` pointer NULL; the env's row of last_obs carries the observation from
  step to step): no tensor with a T axis is allocated.
  -> {'ret': [E, N] float64 undiscounted return (the step rewards summed t ascending), 'success': [E, N] bool success at the last step, 'first_success': [E, N] int32
      first successful step, -1 if none, 'guard_steps': [E, N] int32 env steps the failure guard rolled back (the growth of fail_count over the episode: such steps
      count with reward 0 and no success, and a summary must not hide them)}; the first three equal their definitions applied to what rollout_policy /
  rollout_population would have returned.  reset_first=False: one episode that continues from the current state.  State and bookkeeping end as after rollout_policy."""
  from .. import _abi
  gaussian = env._check_policy(policy, who, population=True)
  if sample and not gaussian:
    raise ValueError(f'{who}: sample=True needs a Gaussian policy (an MLPPolicy is deterministic)')
  E, T, n = int(episodes), int(T), env.num_envs
  if T < 1 or E < 1:
    raise ValueError(f'{who}: T = {T}, episodes = {E}: both >= 1')
  if not reset_first and E != 1:
    raise ValueError(f'{who}: a continuing evaluation (reset_first=False) is one episode')
  kw = dict(device=env.device)
  with torch.cuda.device(env.device):
    ret = torch.empty(E, n, dtype=torch.float64, **kw)
    succ = torch.empty(E, n, dtype=torch.bool, **kw)
    first = torch.empty(E, n, dtype=torch.int32, **kw)
    guard = torch.empty(E, n, dtype=torch.int32, **kw)
    for e in range(E):
      if reset_first:
        env.reset()
      before = env.fail_count.clone()
      obs0 = (env._get_obs_t() if env._last_obs_stale else env.last_obs).contiguous()
      head = policy.head(sample=bool(sample), eps_out=None) if gaussian else None
      summary = _abi.EpisodeSummary(ret=ret[e].data_ptr(), success_last=succ[e].data_ptr(), first_success=first[e].data_ptr())
      env._launch_policy(policy, head, obs0, T, {}, summary=summary)
      finish(env, T, ret[e], succ[e])
      guard[e] = env.fail_count - before
  return {'ret': ret, 'success': succ, 'first_success': first, 'guard_steps': guard}


# ---------------------------------------------------------------------------------------------------------------- the forward / reset agent pair
def backward_goal(env, pair):
  """-> (the ONE goal row of the reset phase or None, the table of rows or None): at most one is given ('initial' on an env with several initial states: a ValueError)"""
  table = pair.goal_table(env)
  return (None if table is not None else pair.goal_row(env)), table


def pair_structs(env, pair, out):
  """the pair's per-env state (`env.agent_phase`, `env.steps_in_phase`, with a table `env.backward_row`: allocated at their first use) and the structs of one launch
  -> (_abi.AgentPair, population struct or None, _abi.BackwardGoals or None), (forward_success, backward_success)"""
  import ctypes as C
  from .. import _abi
  ptr = lambda t: None if t is None else t.data_ptr()
  n, kw = env.num_envs, dict(device=env.device)
  goal, table = backward_goal(env, pair)
  with torch.cuda.device(env.device):
    if env.agent_phase is None:
      env.agent_phase = torch.zeros(n, dtype=torch.int8, **kw)
      env.steps_in_phase = torch.zeros(n, dtype=torch.int32, **kw)
    if table is not None and env.backward_row is None:
      env.backward_row = torch.full((n,), -1, dtype=torch.int32, **kw)
    fwd, bwd = torch.empty(n, dtype=torch.int32, **kw), torch.empty(n, dtype=torch.int32, **kw)
  ps = _abi.AgentPair(switch_every=(C.c_int32 * 2)(*pair.switch_every), switch_on_success=int(pair.switch_on_success), pad_=0, param_stride=pair.pair_stride,
                      backward_goal=ptr(goal), phase=env.agent_phase.data_ptr(), steps_in_phase=env.steps_in_phase.data_ptr(),
                      agent_out=ptr(out.get('agent')), forward_success=fwd.data_ptr(), backward_success=bwd.data_ptr())
  goals = None if table is None else _abi.BackwardGoals(table=table.data_ptr(), n_rows=int(table.shape[0]), pad_=0, row=env.backward_row.data_ptr(),
                                                        row_out=ptr(out.get('backward_row')))
  return (ps, getattr(pair, 'pop_struct', None), goals, (goal, table)), (fwd, bwd)      # (goal, table: kept alive until the launch is issued)


def reset_pair_state(env, mask=None):
  """reset() of the (masked) envs: a reset env starts with the forward agent, and its reset goal came from no row yet"""
  if env.agent_phase is not None:
    if mask is None:
      env.agent_phase.zero_()
      env.steps_in_phase.zero_()
    else:
      env.agent_phase.masked_fill_(mask.bool(), 0)
      env.steps_in_phase.masked_fill_(mask.bool(), 0)
  if env.backward_row is not None:
    if mask is None:
      env.backward_row.fill_(-1)
    else:
      env.backward_row.masked_fill_(mask.bool(), -1)


PAIR_STATE = ('agent_phase', 'steps_in_phase', 'backward_row')


def pair_state_dict(env):
  """the pair's part of state_dict(): in the dict once a pair launch has allocated it, and only then"""
  return {k: getattr(env, k).clone() for k in PAIR_STATE if getattr(env, k) is not None}


def load_pair_state(env, sd):
  """the pair's part of load_state_dict(): the keys of `sd` that are the pair's (a dict without them leaves the env's own)"""
  for k in PAIR_STATE:
    if k in sd:
      setattr(env, k, sd[k].to(env.device, torch.int8 if k == 'agent_phase' else torch.int32).clone())


def rollout_pair(env, pair, T, reset_first=False, sample=True, return_noise=False, out=None, who='rollout_pair'):
  """The forward / reset agent pair of autonomous RL alternating inside ONE launch of the env's rollout kernel (include/earl_physics.h: earl_sawyer_agents_rollout,
  earl_minitaur_agents_rollout, earl_kitchen_agents_rollout):
  `pair` -- an `AgentPair` of the env's widths or a `PairPopulation` of them (the env with global id g runs pair g // envs_per_policy) -- drives every env by the agent
  of its phase (`env.agent_phase`: 0 forward, 1 reset; `env.steps_in_phase`) and hands it over after pair.switch_every[phase] steps or, with pair.switch_on_success,
  after a step whose success flag is set.  Entering the reset phase the env's goal becomes pair.backward_goal ('initial': the one row of `env.initial_states`; None: the
  goal stays) or, with a table of backward goals (an array [R, goal_dim], or 'initial_states'), a row of it drawn from the env's counter-based RNG (seed, global id,
  step: draw index 0xFFFD); entering the forward phase it becomes a row of the env's forward goal table, drawn as the lifelong switch draws.  `goal_t` IS the goal in
  force and stays as the launch leaves it.
  -> rollout_policy()'s dict plus 'agent' [T, N] int8 (the agent that computed the action) and, with a table, 'backward_row' [T, N] int32 (the row drawn at that step,
  -1 elsewhere; `env.backward_row` [N]: the row each env's reset goal came from, -1 before its first entry and after its reset).
  Bookkeeping, the first observation, sample / return_noise and reset_first as rollout_policy.  `env.pair_counts`: the phases of this launch that ended by success."""
  gaussian = env._check_pair(pair, who)
  backward_goal(env, pair)                                 # (its ValueError comes before any reset)
  n, kw = env.num_envs, dict(device=env.device)
  T, out, head, obs0 = prepare(env, who, pair, gaussian, T, reset_first, sample, return_noise, out, what='Gaussian agents (MLPPolicy agents are deterministic)',
                               new_out=getattr(env, '_new_pair_out', None))
  with torch.cuda.device(env.device):
    if 'agent' not in out:
      out['agent'] = torch.empty(T, n, dtype=torch.int8, **kw)
    if pair.goal_table(env) is not None and 'backward_row' not in out:
      out['backward_row'] = torch.empty(T, n, dtype=torch.int32, **kw)
  structs, counts = pair_structs(env, pair, out)
  env._launch_policy(pair, head, obs0, T, out, pair=structs)
  finish(env, T, out['reward'], out['success'][-1])
  env._pair_counts = counts
  return out


def evaluate_pair(env, pair, T, sample=True, who='evaluate_pair'):
  """T steps of `pair` -- an `AgentPair` or a `PairPopulation` -- continuing from the current state, as rollout_pair runs them, in ONE launch that writes only per-env
  summaries (`actions` and every [T] pointer NULL; the env's row of last_obs carries the observation): no tensor with a T axis is allocated.
  -> {'ret': [N] float64 (the step rewards summed t ascending, each against the goal in force during its step), 'success': [N] bool success at the last step,
      'first_success': [N] int32 first successful step or -1, 'guard_steps': [N] int32 steps the failure guard rolled back, 'forward_success' / 'backward_success':
      [N] int32 phases that ended by success (`env.pair_counts`)}: each equals its definition applied to what rollout_pair would have returned.
  State and bookkeeping end as after rollout_pair.  sample=False: Gaussian agents at their mean."""
  from .. import _abi
  gaussian = env._check_pair(pair, who)
  if not gaussian and not sample:
    raise ValueError(f'{who}: sample=False needs Gaussian agents (MLPPolicy agents are deterministic)')
  T, n, kw = int(T), env.num_envs, dict(device=env.device)
  if T < 1:
    raise ValueError(f'{who}: T = {T} < 1')
  with torch.cuda.device(env.device):
    ret, succ = torch.empty(n, dtype=torch.float64, **kw), torch.empty(n, dtype=torch.bool, **kw)
    first = torch.empty(n, dtype=torch.int32, **kw)
    before = env.fail_count.clone()
    obs0 = (env._get_obs_t() if env._last_obs_stale else env.last_obs).contiguous()
  head = pair.head(sample=bool(sample), eps_out=None) if gaussian else None
  summary = _abi.EpisodeSummary(ret=ret.data_ptr(), success_last=succ.data_ptr(), first_success=first.data_ptr())
  structs, counts = pair_structs(env, pair, {})
  env._launch_policy(pair, head, obs0, T, {}, summary=summary, pair=structs)
  finish(env, T, ret, succ)
  env._pair_counts = counts
  return {'ret': ret, 'success': succ, 'first_success': first, 'guard_steps': env.fail_count - before, 'forward_success': counts[0], 'backward_success': counts[1]}

"""The closed loop of the stepper envs (door, peg, minitaur, kitchen) as their `rollout_policy` offers it: what the envs share around the ONE launch of their rollout kernel
with a policy inside it (include/earl_physics.h: earl_sawyer_population_rollout, earl_minitaur_policy_rollout, earl_kitchen_policy_rollout), next to `PhysicsStepGraph`.  The env's side is a few
hooks: `_check_policy(policy, who)` -> is it Gaussian (policy.require_widths with the env's widths and rules), `_new_out((T,))`, `reset()`, `last_obs` /
`_last_obs_stale` / `_get_obs_t()`, and `_launch_policy(policy, head, obs0, T, out)`: the launch itself.  The minitaur and the kitchen also share `rollout_population`
and `evaluate` below: their `_check_policy` takes `population=True` (a PolicyPopulation is then taken, require_widths checking its members against the env's global
ids) and their `_launch_policy` takes `summary=` (None or an _abi.EpisodeSummary) and an `out` that may lack any key.

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

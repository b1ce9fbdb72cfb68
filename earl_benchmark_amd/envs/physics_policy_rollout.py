"""The closed loop of the stepper envs (door, peg, minitaur, kitchen) as their `rollout_policy` offers it: what the envs share around the ONE launch of their rollout kernel
with a policy inside it (include/earl_physics.h: earl_sawyer_population_rollout, earl_minitaur_policy_rollout, earl_kitchen_policy_rollout), next to `PhysicsStepGraph`.  The env's side is a few
hooks: `_check_policy(policy, who)` -> is it Gaussian (policy.require_widths with the env's widths and rules), `_new_out((T,))`, `reset()`, `last_obs` /
`_last_obs_stale` / `_get_obs_t()`, and `_launch_policy(policy, head, obs0, T, out)`: the launch itself.

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

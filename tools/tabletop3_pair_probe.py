"""What the fused launch of the forward / reset agent pair on the THREE-object tabletop (earl_tabletop3_pair_rollout, env.rollout_agents) buys over what a user had
before it.  N = 4096, sparse reward, T = 200 continuing steps, handover every 25 steps, the pairs 20 -> 64 -> 3 and 20 -> 256 -> 128 -> 3 (the widest two-hidden-layer
shape a pair takes), deterministic agents, backward_goal = 'initial':
  (u) alternating       clock-only switching before the pair: T / 25 alternating 25-step launches of earl_tabletop3_policy_rollout (env.rollout_policy), the goal
                        installed by torch ops in between (the reset agent's row appended to the goal table)
  (k) pair_clock        the pair launch, switch_on_success = 0: every workgroup uniform                                -- env.rollout_agents(pair, T)
  (b) graph_both        switching on success before the pair: the captured per-step loop env.make_step_graph(T, policy=...) with both actors in torch, torch.where
                        on the phase, the handover rule and the goal install as torch ops
  (m) pair_mixed        the pair launch, switch_on_success = 1, on envs reset at their goals with random starting phases and clocks: mixed workgroups (the share
                        of mixed (workgroup, step) pairs is reported)
  (s) single_object_*   the single-object pair (earl_tabletop_pair_rollout) at the same N and the shapes 12 -> 64 -> 3 / 12 -> 256 -> 128 -> 3, clock-only and mixed
Device events around --inner back-to-back runs of a leg after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions, every timing from the same env
state; per leg the median, min and max of the per-run milliseconds, spread = max - min.
PASS CONDITION (per shape): (m) takes less time than (b) by more than the two spreads together.  For clock-only switching, (k) against (u) is reported as inside (u)'s
spread or as a gap; every other ratio is reported, not gated.  Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/tabletop3_pair_probe.py [--reps 5] [--inner 5] [--out profiles/tabletop3_pair_probe.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from tabletop3_policy_probe import interleaved, layers_of, summary      # noqa: E402 (the three-object probes share their method)

N, T, SE = 4096, 200, 25
DEV = 'cuda'
NETS = {'64': (64,), '256x128': (256, 128)}


def restorer(env):
  """-> restore(): the env's state, pair state and Philox counter as they are now, copied back IN PLACE (a captured graph holds the tensors' addresses)"""
  names = ('qpos', 'attached', 'goal_idx', 'steps_since_reset', 'interventions') + (('agent_phase', 'steps_in_phase') if env.agent_phase is not None else ())
  saved, counter = {k: getattr(env, k).clone() for k in names}, int(env._cfg.counter)

  def restore():
    for k, v in saved.items():
      getattr(env, k).copy_(v)
    env._cfg.counter = counter
  return restore


def both(*restores):
  def restore():
    for r in restores:
      r()
  return restore


def mixed_share(agent):
  a = agent.reshape(T, -1, 16)
  return float(((a == 1).any(-1) & (a == 0).any(-1)).float().mean())


def make_env(torch, nobj, at_goal):
  if nobj == 3:
    from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
    env = TabletopManipulation(reward_type='sparse', reset_at_goal=at_goal, num_envs=N, device=DEV, seed=1)
  else:
    from earl_benchmark_amd.envs.tabletop import TabletopManipulation
    env = TabletopManipulation(reward_type='sparse', reset_at_goal=at_goal, wide_init_distr=at_goal, num_envs=N, device=DEV, seed=1)
  env._cfg.horizon = 2**31 - 1
  env.reset()
  return env


def random_phases(torch, env, pair, gen):
  """a first launch creates the pair state; then random starting phases and clocks"""
  env.rollout_agents(pair, 1)
  env.agent_phase.copy_(torch.randint(0, 2, (N,), device=DEV, generator=gen).to(torch.int8))
  env.steps_in_phase.copy_(torch.randint(0, SE, (N,), device=DEV, generator=gen).to(torch.int32))


def probe(torch, net, reps, inner):
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  kw = dict(device=DEV, obs_dim=20, act_dim=3)
  agents = [MLPPolicy(layers_of(20, NETS[net], 3, seed=3 + k), 'relu', 'tanh', **kw) for k in range(2)]
  pair_k = AgentPair(agents[0], agents[1], switch_every=SE, switch_on_success=False, backward_goal='initial', **kw)
  pair_m = AgentPair(agents[0], agents[1], switch_every=SE, switch_on_success=True, backward_goal='initial', **kw)
  gen = torch.Generator(device=DEV).manual_seed(7)
  env_u, env_k, env_m, env_b = make_env(torch, 3, False), make_env(torch, 3, False), make_env(torch, 3, True), make_env(torch, 3, True)

  # (u): the reset agent's goal as one more row of the goal table, goal_idx pointed at it / back at the task row by torch ops between the launches
  env_u.goal_table = torch.cat([env_u.goal_table, torch.as_tensor(env_u.initial_state, dtype=torch.float64, device=DEV)[None]], 0).contiguous()
  env_u._sync_state_ptrs()
  row = env_u.goal_table.shape[0] - 1

  def alternating():
    for chunk in range(T // SE):
      k = chunk & 1
      env_u.rollout_policy(agents[k], SE, reset_first=False)
      if k == 0:
        env_u.goal_idx.fill_(row)
      else:
        env_u.goal_idx.copy_(torch.randint(0, row, (N,), device=DEV, generator=gen).to(torch.int32))

  env_k.rollout_agents(pair_k, 1)
  env_k.agent_phase.zero_()
  env_k.steps_in_phase.zero_()
  random_phases(torch, env_m, pair_m, gen)
  last = {}

  def mixed():
    last['agent'] = env_m.rollout_agents(pair_m, T)[5]

  # (b): the captured per-step loop; the phase state, the handover rule and the goal install are torch ops beside the two actors
  env_b.goal_table = torch.cat([env_b.goal_table, torch.as_tensor(env_b.initial_state, dtype=torch.float64, device=DEV)[None]], 0).contiguous()
  env_b._sync_state_ptrs()
  rows_b = env_b.goal_table.shape[0] - 1
  phase = torch.randint(0, 2, (N,), device=DEV, generator=gen).bool()
  sip = torch.randint(0, SE, (N,), device=DEV, generator=gen).to(torch.int32)
  task = env_b.goal_idx.clone()
  draws, at = torch.randint(0, rows_b, (T + 1, N), device=DEV, generator=gen).to(torch.int32), [0]
  state_b = (phase.clone(), sip.clone(), task.clone())

  def both_actors(obs):
    succ = (obs[:, 0:8] - obs[:, 10:18]).square().sum(1).sqrt() <= 0.4            # the success flag of the step that produced obs
    sip.add_(1)
    over = succ | (sip >= SE)
    to_forward = over & phase
    task.copy_(torch.where(to_forward, draws[at[0] % (T + 1)], task))
    at[0] += 1
    phase.logical_xor_(over)
    sip.mul_(~over)
    env_b.goal_idx.copy_(torch.where(phase, torch.full_like(task, rows_b), task))
    return torch.where(phase[:, None], agents[1](obs), agents[0](obs))
  graph = env_b.make_step_graph(T, policy=both_actors)
  restore_env_b = restorer(env_b)

  def restore_b():
    restore_env_b()
    for live, saved in zip((phase, sip, task), state_b):
      live.copy_(saved)
    graph.obs_in.copy_(env_b._observe(('obs',))[0])

  legs = {'u_alternating': alternating, 'k_pair_clock': lambda: env_k.rollout_agents(pair_k, T), 'b_graph_both': graph.replay, 'm_pair_mixed': mixed}
  ms = interleaved(torch, legs, reps, inner, both(restorer(env_u), restorer(env_k), restorer(env_m), restore_b))
  res = {k: summary(v) for k, v in ms.items()}
  u, k, b, m = (res[x] for x in ('u_alternating', 'k_pair_clock', 'b_graph_both', 'm_pair_mixed'))
  restorer_m = restorer(env_m)
  mixed()
  restorer_m()
  ak = env_k.rollout_agents(pair_k, T)[5]
  res.update(policy=f'20 -> {" -> ".join(map(str, NETS[net]))} -> 3', m_share_of_workgroup_steps_mixed=round(mixed_share(last['agent']), 4),
             k_share_of_workgroup_steps_mixed=round(mixed_share(ak), 4), b_over_m=round(b['ms_median'] / m['ms_median'], 2), k_over_u=round(k['ms_median'] / u['ms_median'], 3),
             m_over_k=round(m['ms_median'] / k['ms_median'], 3),
             k_vs_u={'difference_ms': round(k['ms_median'] - u['ms_median'], 4), 'spread_of_u_ms': u['spread_ms'],
                     'inside_the_spread_of_u': bool(abs(k['ms_median'] - u['ms_median']) <= u['spread_ms'])},
             pass_condition={'statement': 'm_pair_mixed median < b_graph_both median by more than the two spreads together',
                             'difference_ms': round(b['ms_median'] - m['ms_median'], 4), 'spreads_together_ms': round(b['spread_ms'] + m['spread_ms'], 4),
                             'met': bool(b['ms_median'] - m['ms_median'] > b['spread_ms'] + m['spread_ms'])})
  return res


def single_object(torch, net, reps, inner):
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  agents = [MLPPolicy(layers_of(12, NETS[net], 3, seed=3 + k), 'relu', 'tanh', device=DEV) for k in range(2)]
  pair_k = AgentPair(agents[0], agents[1], switch_every=SE, switch_on_success=False, device=DEV)
  pair_m = AgentPair(agents[0], agents[1], switch_every=SE, switch_on_success=True, device=DEV)
  gen = torch.Generator(device=DEV).manual_seed(7)
  env_k, env_m = make_env(torch, 1, False), make_env(torch, 1, True)
  env_k.rollout_agents(pair_k, 1)
  env_k.agent_phase.zero_()
  env_k.steps_in_phase.zero_()
  random_phases(torch, env_m, pair_m, gen)
  last = {}

  def mixed():
    last['agent'] = env_m.rollout_agents(pair_m, T)[5]
  legs = {'single_object_pair_clock': lambda: env_k.rollout_agents(pair_k, T), 'single_object_pair_mixed': mixed}
  ms = interleaved(torch, legs, reps, inner, both(restorer(env_k), restorer(env_m)))
  res = {k: summary(v) for k, v in ms.items()}
  res.update(policy=f'12 -> {" -> ".join(map(str, NETS[net]))} -> 3', mixed_share_of_workgroup_steps=round(mixed_share(last['agent']), 4))
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=5)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop3_pair_probe.py measures on the GPU: no HIP device visible')
  out = {'what': 'tools/tabletop3_pair_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'T': T, 'switch_every': [SE, SE], 'reward': 'sparse', 'form': 'continuing (reset_first = 0)', 'reps': args.reps, 'inner': args.inner, 'cases': {},
         'single_object': {}}
  for net in NETS:
    out['cases'][net] = probe(torch, net, args.reps, args.inner)
    out['single_object'][net] = single_object(torch, net, args.reps, args.inner)
    c, s = out['cases'][net], out['single_object'][net]
    c['three_over_single_object'] = {'clock_only': round(c['k_pair_clock']['ms_median'] / s['single_object_pair_clock']['ms_median'], 3),
                                     'mixed': round(c['m_pair_mixed']['ms_median'] / s['single_object_pair_mixed']['ms_median'], 3)}
  out['pass_condition_met'] = all(c['pass_condition']['met'] for c in out['cases'].values())
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0 if out['pass_condition_met'] else 1


if __name__ == '__main__':
  sys.exit(main())

"""The forward / reset agent pair on the minitaur (N = 4096, T = 250, 32 -> 64 -> 64 -> 8) and the kitchen (N = 2048, T = 400, 46 -> 64 -> 64 -> 9), handover every 25
steps, five ways over the same T env steps from the reset state:
  (a) single_policy   ONE rollout_policy launch of the forward agent: the floor (no pair)
  (b) alternating     the T / 25 single-policy launches, forward and reset agent in turn, with the goal writes in between, that clock-only switching replaces
  (c) pair_clock      rollout_pair(pair, T), switch_on_success = False: ONE launch, every wave uniform
  (d) pair_success    rollout_pair(pair, T), switch_on_success = True, from staggered phase state (phase = i % 2, steps_in_phase = i % 25): waves are mixed
  (e) graph_pair      the captured per-step loop make_step_graph(T, policy=actor) with both actors in torch: the actor works out the success flag of the observation it
                      is given, keeps phase / steps_in_phase on the device, writes the goal rows of the envs that hand over and answers with the network of the phase
                      -- what switching on success costs without the fused launch (the comparison for (d))
The backward goal is the env's reset state (minitaur: the reset pose's (x, y); kitchen: row 0 of get_init_states()), the forward goal the env's own table.
Device events after one warm-up; the legs are interleaved over --reps repetitions, every run from the same env state; per leg median / min / max ms and the ratios
(c)/(a), (c)/(b), (d)/(c), (d)/(e), the share of (wave, step) pairs of (d) that were mixed (a wave holds two envs), the handovers of (d) by success, and the share of
rows in the failure guard.
--parent-lib PATH: the single-policy launch (and the open-loop rollout) at this commit against another build of libearl_hip.so (the parent commit's), as
tools/physics_population_probe.py's gate: child processes taking turns, margin max(5 %, 3 x the other build's own spread); a miss ends with status 1.

  python tools/physics_pair_probe.py [--reps 5] [--envs minitaur,kitchen] [--parent-lib /path/to/libearl_hip.so] [--out-dir profiles]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from physics_population_probe import HIDDEN, SHAPE, gate_legs      # noqa: E402  (the shapes, the networks and the gate's legs of the population probe)

EVERY = 25
GOAL_AT = {'minitaur': 30, 'kitchen': 23}
NEW_ENTRY_POINTS = ('earl_minitaur_agents_rollout', 'earl_kitchen_agents_rollout')


def success_of(torch, kind, obs):
  """the env's success flag of an observation row (minitaur_gym_env.py:495-503; kitchen.py:180-183)"""
  if kind == 'minitaur':
    return (obs[:, 28:30] - obs[:, 30:32]).norm(dim=1) < 0.1
  return (obs[:, 9:23] - obs[:, 32:46]).norm(dim=1) <= 0.3


class TorchActors:
  """leg (e): both agents and the handover rule in torch, called between the captured steps with the observation the env last returned"""

  def __init__(self, torch, kind, env, pair, back, task, on_success):
    self.torch, self.kind, self.env, self.pair, self.back, self.task, self.on_success = torch, kind, env, pair, back, task, on_success
    self.phase = torch.zeros(env.num_envs, dtype=torch.int64, device='cuda')
    self.sip = torch.zeros(env.num_envs, dtype=torch.int64, device='cuda')

  def start(self, phase, sip):
    self.phase.copy_(phase)
    self.sip.copy_(sip)

  def __call__(self, obs):
    torch, u, at = self.torch, self.env, GOAL_AT[self.kind]
    if obs._base is not None:                                            # a row of the graph's [T, N, D] output: a step precedes it (its obs_in tensor: none does)
      ok = success_of(torch, self.kind, obs) & bool(self.on_success)
      self.sip += 1
      over = ok | (self.sip >= EVERY)
      self.phase.copy_(torch.where(over, self.phase ^ 1, self.phase))
      self.sip.copy_(torch.where(over, torch.zeros_like(self.sip), self.sip))
      new = torch.where((self.phase == 1)[:, None], self.back[None], self.task[None])
      u.goal_t.copy_(torch.where(over[:, None], new, u.goal_t))
      obs = torch.cat([obs[:, :at], u.goal_t], 1)
    return self.pair(obs, self.phase)


def probe(torch, kind, reps):
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  s = SHAPE[kind]
  n, T, W = s['n'], s['T'], s['obs'] - GOAL_AT[kind]
  env = s['mod'].make(n)
  mk = lambda seed: MLPPolicy(s['mod'].layers_of(HIDDEN, seed=seed), 'relu', 'tanh', device='cuda', obs_dim=s['obs'], act_dim=s['act'])
  fwd, bwd = mk(3), mk(4)
  back = torch.as_tensor(env.initial_states[0], dtype=torch.float64, device='cuda')
  task = env.goal_t[0].clone()
  clock = AgentPair(fwd, bwd, switch_every=EVERY, switch_on_success=False, backward_goal=back, obs_dim=s['obs'], act_dim=s['act'])
  onsuc = AgentPair(fwd, bwd, switch_every=EVERY, switch_on_success=True, backward_goal=back, obs_dim=s['obs'], act_dim=s['act'])
  i = torch.arange(n, device='cuda')
  ph0, sip0 = (i % 2).to(torch.int8), (i % EVERY).to(torch.int32)
  out = env.rollout_pair(clock, T)                                        # (allocates the phase state and the outputs every leg writes into)
  env.reset()
  snap = env.state_dict()
  out1 = {k: v[:EVERY] for k, v in out.items() if k != 'agent'}
  actors = TorchActors(torch, kind, env, clock, back, task, on_success=True)
  graph = None

  def restore():
    env.load_state_dict(snap)
    env.agent_phase.zero_()
    env.steps_in_phase.zero_()
    if graph is not None:
      graph.obs_in.copy_(snap['last_obs'])

  def alternating():
    for c in range((T + EVERY - 1) // EVERY):
      env.rollout_policy(bwd if c % 2 else fwd, min(EVERY, T - c * EVERY), out=out1 if T - c * EVERY >= EVERY else None)
      row = task if c % 2 else back                                      # the goal the NEXT chunk runs under, and the goal block its first action sees
      env.goal_t.copy_(row.expand(n, W))
      env.last_obs[:, GOAL_AT[kind]:] = row

  def staggered():
    env.agent_phase.copy_(ph0)
    env.steps_in_phase.copy_(sip0)
    return env.rollout_pair(onsuc, T, out=out)

  def graph_pair():
    actors.start(ph0.to(torch.int64), sip0.to(torch.int64))
    graph.replay()
  restore()
  graph = env.make_step_graph(T, policy=actors)
  restore()
  o = staggered()
  agent = o['agent'].reshape(T, n // 2, 2)
  mixed = float(((agent == 0).any(-1) & (agent == 1).any(-1)).float().mean())
  guard = float((o['status'] != 0).float().mean())
  by_success = int(env.pair_counts[0].sum() + env.pair_counts[1].sum())
  legs = {'single_policy': lambda: env.rollout_policy(fwd, T, out=out), 'alternating': alternating, 'pair_clock': lambda: env.rollout_pair(clock, T, out=out),
          'pair_success': staggered, 'graph_pair': graph_pair}
  ms = s['mod'].interleaved(torch, legs, reps, restore, warmup=1)
  res = {'n': n, 'T': T, 'net': [s['obs']] + list(HIDDEN) + [s['act']], 'switch_every': EVERY, 'guard_share_pair_success': guard,
         'mixed_wave_steps_share_pair_success': mixed, 'handovers_by_success_pair_success': by_success, 'device': torch.cuda.get_device_name(0)}
  for k in legs:
    res[k] = s['mod'].summary(ms[k], n, T)
  med = lambda k: res[k]['ms_median']
  for a, b in (('pair_clock', 'single_policy'), ('pair_clock', 'alternating'), ('pair_success', 'pair_clock'), ('pair_success', 'graph_pair')):
    res[f'{a}_over_{b}'] = round(med(a) / med(b), 4)
  return res


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='minitaur,kitchen')
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--gate-only', action='store_true', help='skip the five legs (with --parent-lib)')
  ap.add_argument('--out-dir', default=None, help='also write <env>_pair_probe.json per env into this directory (profiles)')
  ap.add_argument('--gate-child', default=None, help='(child process) load this libearl_hip.so (or "own") and time the gate\'s legs of --envs')
  ap.add_argument('--legs-child', default=None, help='(child process) the five legs of this env')
  a = ap.parse_args()
  kinds = a.envs.split(',')
  if a.gate_child:
    if a.gate_child != 'own':
      from earl_benchmark_amd import _abi
      _abi.LIB_PATH = a.gate_child
      for name in NEW_ENTRY_POINTS:                                       # (the older build does not export them; the gate's legs do not call them)
        _abi.SIGNATURES.pop(name, None)
    import torch
    print(json.dumps({kind: gate_legs(torch, kind, a.reps) for kind in kinds}))
    return
  if a.legs_child:
    import torch
    print(json.dumps(probe(torch, a.legs_child, a.reps)))
    return

  def child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), *args], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
      raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])
  res = {kind: {'tool': 'physics_pair_probe', 'env': kind,
                'timing': 'device events after 1 warm-up run, legs interleaved over the repetitions, every run from the same env state'} for kind in kinds}
  ok = True
  if a.parent_lib:                                                        # the builds take turns, two child processes each
    runs = {'parent': [], 'this': []}
    for _ in range(2):
      runs['parent'].append(child('--envs', a.envs, '--gate-child', a.parent_lib))
      runs['this'].append(child('--envs', a.envs, '--gate-child', 'own'))
    for kind in kinds:
      gate = {'margin': 'max(5 %, 3 x the parent legs\' own spread (max - min) / median)', 'n': SHAPE[kind]['n'], 'T': SHAPE[kind]['T']}
      passed_all = True
      for leg in ('rollout_policy', 'rollout'):
        ms = {b: [x for r in runs[b] for x in r[kind][leg]] for b in runs}
        pm, tm = statistics.median(ms['parent']), statistics.median(ms['this'])
        spread = (max(ms['parent']) - min(ms['parent'])) / pm
        margin = max(0.05, 3 * spread)
        passed = tm <= pm * (1 + margin)
        passed_all = passed_all and passed
        gate[leg] = {'parent_ms_median': round(pm, 3), 'this_ms_median': round(tm, 3), 'ratio': round(tm / pm, 4), 'parent_spread': round(spread, 4),
                     'margin': round(margin, 4), 'passed': passed, 'parent_ms_all': ms['parent'], 'this_ms_all': ms['this']}
      gate['passed'] = passed_all
      ok = ok and passed_all
      res[kind]['parent_gate'] = gate
    print(f'parent gate: {"passed" if ok else "MISSED"}', file=sys.stderr, flush=True)
  if not a.gate_only:
    for kind in kinds:
      res[kind].update(child('--legs-child', kind))
      print(f'{kind}: done', file=sys.stderr, flush=True)
  if a.out_dir:
    for kind in kinds:
      with open(os.path.join(a.out_dir, f'{kind}_pair_probe.json'), 'w') as f:
        json.dump(res[kind], f, indent=1)
        f.write('\n')
  print(json.dumps(res))
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  main()

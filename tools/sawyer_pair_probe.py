"""The forward / reset agent pair on the Sawyer door and peg, N = 8192 envs, 14 -> 64 -> 64 -> 4, the bench's T (door 300, peg 200), handover every 25 steps, five
ways over the same T env steps from the reset state:
  (a) single_policy   ONE rollout_policy launch of the forward agent: the floor (no pair)
  (b) alternating     the T / 25 single-policy launches, forward and reset agent in turn, with the goal writes in between, that clock-only switching replaces
  (c) pair_clock      rollout_agents(pair, T), switch_on_success = False: ONE launch, every wave uniform
  (d) pair_success    rollout_agents(pair, T), switch_on_success = True, from staggered phase state (phase = i % 2, steps_in_phase = i % 25): waves are mixed
  (e) graph_pair      the captured per-step loop make_step_graph(T, policy=actor) with both actors in torch: the actor works out the success flag of the observation it
                      is given, keeps phase / steps_in_phase on the device, writes the goal rows of the envs that hand over and answers with the network of the phase
                      -- what switching on success costs without the fused launch (the comparison for (d))
Device events after one warm-up; the legs are interleaved over --reps repetitions, every run from the same env state; per leg median / min / max ms and the ratios
(c)/(a), (c)/(b), (d)/(c), (d)/(e), the share of (wave, step) pairs of (d) that were mixed, the handovers of (d) by success, and the share of rows in the failure guard.
--parent-lib PATH: the gate on the shared kernel, as tools/sawyer_population_probe.py's: rollout_policy and rollout of door and peg at the bench's T, this build and
another build of libearl_hip.so (the parent commit's) in child processes taking turns, margin max(5 %, 3 x the other build's own spread); a miss ends with status 1.

  python tools/sawyer_pair_probe.py [--reps 5] [--envs door,peg] [--parent-lib /path/to/libearl_hip.so] [--out profiles/sawyer_pair_probe.json]
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

from sawyer_policy_probe import BENCH_T, NETS, interleaved, layers_of, make, summary      # noqa: E402
from sawyer_population_probe import gate_legs                                              # noqa: E402

N, EVERY, HIDDEN = 8192, 25, NETS['64x64']


class TorchActors:
  """leg (e): both agents and the handover rule in torch, called between the captured steps with the observation the env last returned"""

  def __init__(self, torch, env, pair, goal, on_success):
    self.torch, self.env, self.pair, self.goal, self.on_success = torch, env, pair, goal, on_success
    self.phase = torch.zeros(env.num_envs, dtype=torch.int64, device='cuda')
    self.sip = torch.zeros(env.num_envs, dtype=torch.int64, device='cuda')

  def start(self, phase, sip):
    self.phase.copy_(phase)
    self.sip.copy_(sip)

  def __call__(self, obs):
    torch, u = self.torch, self.env
    if obs._base is not None:                                            # a row of the graph's [T, N, 14] output: a step precedes it (its obs_in tensor: none does)
      ok = ((obs[:, 4:7] - obs[:, 11:14]).norm(dim=1) <= float(u._cfg.success_radius)) & bool(self.on_success)
      self.sip += 1
      over = ok | (self.sip >= EVERY)
      self.phase.copy_(torch.where(over, self.phase ^ 1, self.phase))
      self.sip.copy_(torch.where(over, torch.zeros_like(self.sip), self.sip))
      new = torch.where((self.phase == 1)[:, None], self.goal[None], u._goal_table[0][None])
      u.goal_t.copy_(torch.where(over[:, None], new, u.goal_t))
      obs = torch.cat([obs[:, :7], u.goal_t], 1)
    return self.pair(obs, self.phase)


def probe(torch, kind, reps):
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  T = BENCH_T[kind]
  env = make(kind, N)
  fwd = MLPPolicy(layers_of(HIDDEN, seed=3), 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4)
  bwd = MLPPolicy(layers_of(HIDDEN, seed=4), 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4)
  goal = torch.as_tensor(env.initial_states[0], dtype=torch.float64, device='cuda')
  task = env._goal_table[0].clone()
  clock = AgentPair(fwd, bwd, switch_every=EVERY, switch_on_success=False, backward_goal=goal, obs_dim=14, act_dim=4)
  onsuc = AgentPair(fwd, bwd, switch_every=EVERY, switch_on_success=True, backward_goal=goal, obs_dim=14, act_dim=4)
  i = torch.arange(N, device='cuda')
  ph0, sip0 = (i % 2).to(torch.int8), (i % EVERY).to(torch.int32)
  out = env.rollout_agents(clock, T)                                      # (allocates the phase state and the outputs every leg writes into)
  env.reset()
  snap = env.state_dict()
  out1 = {k: v[:EVERY] for k, v in out.items() if k != 'agent'}
  actors = TorchActors(torch, env, clock, goal, on_success=True)
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
      row = task if c % 2 else goal                                      # the goal the NEXT chunk runs under, and the goal block its first action sees
      env.goal_t.copy_(row.expand(N, 7))
      env.last_obs[:, 7:] = row

  def staggered():
    env.agent_phase.copy_(ph0)
    env.steps_in_phase.copy_(sip0)
    return env.rollout_agents(onsuc, T, out=out)

  def graph_pair():
    actors.start(ph0.to(torch.int64), sip0.to(torch.int64))
    graph.replay()
  restore()
  graph = env.make_step_graph(T, policy=actors)
  restore()
  o = staggered()
  agent = o['agent'].reshape(T, N // 4, 4)
  mixed = float(((agent == 0).any(-1) & (agent == 1).any(-1)).float().mean())
  guard = float((o['status'] != 0).float().mean())
  by_success = int(env.pair_counts[0].sum() + env.pair_counts[1].sum())
  legs = {'single_policy': lambda: env.rollout_policy(fwd, T, out=out), 'alternating': alternating, 'pair_clock': lambda: env.rollout_agents(clock, T, out=out),
          'pair_success': staggered, 'graph_pair': graph_pair}
  ms = interleaved(torch, legs, reps, restore, warmup=1)
  res = {'n': N, 'T': T, 'net': [14] + list(HIDDEN) + [4], 'switch_every': EVERY, 'guard_share_pair_success': guard, 'mixed_wave_steps_share_pair_success': mixed,
         'handovers_by_success_pair_success': by_success}
  for k in legs:
    res[k] = summary(ms[k], N, T)
  med = lambda k: res[k]['ms_median']
  for a, b in (('pair_clock', 'single_policy'), ('pair_clock', 'alternating'), ('pair_success', 'pair_clock'), ('pair_success', 'graph_pair')):
    res[f'{a}_over_{b}'] = round(med(a) / med(b), 4)
  return res


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--gate-only', action='store_true', help='skip the five legs (with --parent-lib)')
  ap.add_argument('--out', default=None, help='also write the JSON object to this file (profiles/sawyer_pair_probe.json)')
  ap.add_argument('--gate-child', default=None, help='(child process) load this libearl_hip.so (or "own") and time the gate\'s legs')
  a = ap.parse_args()
  kinds = a.envs.split(',')
  if a.gate_child:
    from earl_benchmark_amd import _abi
    if a.gate_child != 'own':
      _abi.LIB_PATH = a.gate_child
      _abi.SIGNATURES.pop('earl_sawyer_pair_rollout', None)               # (the older build does not export it; the gate's legs do not call it)
    import torch
    print(json.dumps({kind: gate_legs(torch, kind, a.reps) for kind in kinds}))
    return

  def child(lib):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--envs', a.envs, '--gate-child', lib], capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
      raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])
  res = {'tool': 'sawyer_pair_probe', 'timing': 'device events after 1 warm-up run, legs interleaved over the repetitions, every run from the same env state'}
  ok = True
  if a.parent_lib:                                                        # the builds take turns, two child processes each
    runs = {'parent': [], 'this': []}
    for _ in range(2):
      runs['parent'].append(child(a.parent_lib))
      runs['this'].append(child('own'))
    gate = {'margin': 'max(5 %, 3 x the parent legs\' own spread (max - min) / median)', 'n': N, 'net': [14, 64, 64, 4]}
    for kind in kinds:
      for leg in ('rollout_policy', 'rollout'):
        ms = {b: [x for r in runs[b] for x in r[kind][leg]] for b in runs}
        pm, tm = statistics.median(ms['parent']), statistics.median(ms['this'])
        spread = (max(ms['parent']) - min(ms['parent'])) / pm
        margin = max(0.05, 3 * spread)
        passed = tm <= pm * (1 + margin)
        ok = ok and passed
        gate[f'{kind}_{leg}_T{BENCH_T[kind]}'] = {'parent_ms_median': round(pm, 3), 'this_ms_median': round(tm, 3), 'ratio': round(tm / pm, 4),
                                                  'parent_spread': round(spread, 4), 'margin': round(margin, 4), 'passed': passed,
                                                  'parent_ms_all': ms['parent'], 'this_ms_all': ms['this']}
    gate['passed'] = ok
    print(f'parent gate: {"passed" if ok else "MISSED"}', file=sys.stderr, flush=True)
    res['parent_gate'] = gate
  if not a.gate_only:
    import torch
    res['device'] = torch.cuda.get_device_name(0)
    for kind in kinds:
      res[kind] = probe(torch, kind, a.reps)
      print(f'{kind}: done', file=sys.stderr, flush=True)
      torch.cuda.empty_cache()
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(res, f, indent=1)
      f.write('\n')
  print(json.dumps(res))
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  main()

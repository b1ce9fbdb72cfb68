#!/usr/bin/env python3
"""Is a build whose closed-loop kernel arguments, host fill and device pieces are shared (csrc/policy_closed_loop.h) as fast as the build before it?  Runs the project's own
gates against another build of libearl_hip.so -- tools/physics_pair_probe.py (minitaur, kitchen) and tools/sawyer_agents_probe.py (door, peg) with --parent-lib
--gate-only: the open-loop and single-policy launches, the Sawyer's one-row pair -- and then what those gates do not cover, by the same rule: each env's POPULATION leg
and PAIR leg (the probes' shapes and networks) timed with each build's library, loaded the way the gates' child processes load it.  Child processes take turns, two per
build; margin max(5 %, 3 x the parent legs' own spread (max - min) / median); a miss ends with status 1.
  python tools/closed_loop_args_gate.py --parent-lib /path/to/parent/libearl_hip.so [--reps 5] [--out profiles/closed_loop_args_gate.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
KINDS = ('minitaur', 'kitchen', 'door', 'peg')


def legs_of(torch, kind, reps):
  """(child process) {leg: [ms]} of one env: 'population', 'pair' (success handovers, phases staggered over the envs / a table of backward goals) and, on the Sawyer,
  'pair_population'"""
  import numpy as np
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy, PairPopulation
  if kind in ('minitaur', 'kitchen'):
    import physics_pair_probe as pp
    import physics_population_probe as pop_probe
    s = pop_probe.SHAPE[kind]
    n, T, mod = s['n'], s['T'], s['mod']
    env = mod.make(n)
    _, pop = pop_probe.population(torch, kind, n // pop_probe.G)
    mk = lambda seed: MLPPolicy(mod.layers_of(pop_probe.HIDDEN, seed=seed), 'relu', 'tanh', device='cuda', obs_dim=s['obs'], act_dim=s['act'])
    back = torch.as_tensor(env.initial_states[0], dtype=torch.float64, device='cuda')
    pair = AgentPair(mk(3), mk(4), switch_every=pp.EVERY, switch_on_success=True, backward_goal=back, obs_dim=s['obs'], act_dim=s['act'])
    i = torch.arange(n, device='cuda')
    ph0, sip0 = (i % 2).to(torch.int8), (i % pp.EVERY).to(torch.int32)
    out = env.rollout_pair(pair, T)
    out_pop = {k: v for k, v in out.items() if k != 'agent'}
    env.reset()
    snap = env.state_dict()

    def staggered():
      env.agent_phase.copy_(ph0)
      env.steps_in_phase.copy_(sip0)
      env.rollout_pair(pair, T, out=out)
    legs = {'population': lambda: env.rollout_population(pop, T, out=out_pop), 'pair': staggered}
    return mod.interleaved(torch, legs, reps, lambda: env.load_state_dict(snap), warmup=1)
  import sawyer_agents_probe as ap
  import sawyer_population_probe as sp
  T = ap.BENCH_T[kind]
  env = ap.make(kind, ap.N)
  row = np.asarray(env.initial_states[0], dtype=np.float64)
  if kind == 'peg':
    table = 'initial_states'
  else:
    table = np.repeat(row[None], 15, 0)
    table[:, 4:7] += 0.002 * np.arange(15)[:, None] * np.array([1.0, -0.5, 0.25])
  kw = dict(switch_every=ap.EVERY, switch_on_success=True, obs_dim=14, act_dim=4)
  tab = AgentPair(*ap.agents(3), backward_goal=table, **kw)
  pairs = PairPopulation([AgentPair(*ap.agents(3 + 2 * p), backward_goal=row, **kw) for p in range(ap.P)], envs_per_policy=ap.G, device='cuda')
  _, pop = sp.population(torch, ap.HIDDEN)
  out = env.rollout_agents(tab, T)
  out_pop = {k: v for k, v in out.items() if k not in ('agent', 'backward_row')}
  out_pairs = {k: v for k, v in out.items() if k != 'backward_row'}
  env.reset()
  snap = env.state_dict()
  legs = {'population': lambda: env.rollout_policy(pop, T, out=out_pop), 'pair': lambda: env.rollout_agents(tab, T, out=out),
          'pair_population': lambda: env.rollout_agents(pairs, T, out=out_pairs)}
  return ap.interleaved(torch, legs, reps, lambda: env.load_state_dict(snap), warmup=1)


def judged(ms):
  """the gate's rule on {'parent': [ms], 'this': [ms]}"""
  pm, tm = statistics.median(ms['parent']), statistics.median(ms['this'])
  spread = (max(ms['parent']) - min(ms['parent'])) / pm
  margin = max(0.05, 3 * spread)
  return {'parent_ms_median': round(pm, 3), 'this_ms_median': round(tm, 3), 'ratio': round(tm / pm, 4), 'parent_spread': round(spread, 4),
          'this_spread': round((max(ms['this']) - min(ms['this'])) / tm, 4), 'margin': round(margin, 4), 'passed': tm <= pm * (1 + margin),
          'parent_ms_all': ms['parent'], 'this_ms_all': ms['this']}


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default=','.join(KINDS))
  ap.add_argument('--out', default=None)
  ap.add_argument('--legs-child', default=None, help='(child process) load this libearl_hip.so (or "own") and time the extra legs of --envs')
  a = ap.parse_args()
  kinds = a.envs.split(',')
  if a.legs_child:
    if a.legs_child != 'own':
      from earl_benchmark_amd import _abi
      _abi.LIB_PATH = a.legs_child                                        # (both builds export every entry point: the ABI is what it was)
    import torch
    print(json.dumps({kind: {k: [round(x, 3) for x in v] for k, v in legs_of(torch, kind, a.reps).items()} for kind in kinds}))
    return
  if not a.parent_lib:
    ap.error('--parent-lib is required')

  def run(tool, *args, ok=(0,)):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool), '--reps', str(a.reps), *args], capture_output=True, text=True, timeout=1500)
    if r.returncode not in ok:
      raise RuntimeError(f'{tool} {args}: status {r.returncode}\n{r.stderr[-2000:]}')
    return json.loads(r.stdout.strip().splitlines()[-1])
  res = {'tool': 'closed_loop_args_gate', 'margin': 'max(5 %, 3 x the parent legs\' own spread (max - min) / median)',
         'timing': 'device events after 1 warm-up run, legs interleaved over the repetitions, every run from the same env state; the builds take turns, two child '
                   'processes each'}
  physics = [k for k in kinds if k in ('minitaur', 'kitchen')]
  sawyer = [k for k in kinds if k in ('door', 'peg')]
  if physics:
    got = run('physics_pair_probe.py', '--envs', ','.join(physics), '--parent-lib', a.parent_lib, '--gate-only', ok=(0, 1))
    res['physics_pair_probe'] = {k: got[k]['parent_gate'] for k in physics}
  if sawyer:
    res['sawyer_agents_probe'] = run('sawyer_agents_probe.py', '--envs', ','.join(sawyer), '--parent-lib', a.parent_lib, '--gate-only', ok=(0, 1))['parent_gate']
  runs = {'parent': [], 'this': []}
  for _ in range(2):
    runs['parent'].append(run('closed_loop_args_gate.py', '--envs', a.envs, '--legs-child', a.parent_lib))
    runs['this'].append(run('closed_loop_args_gate.py', '--envs', a.envs, '--legs-child', 'own'))
  res['population_and_pair_legs'] = {kind: {leg: judged({b: [x for r in runs[b] for x in r[kind][leg]] for b in runs}) for leg in runs['this'][0][kind]} for kind in kinds}
  import torch
  res['device'] = torch.cuda.get_device_name(0)
  ok = all(g['passed'] for g in res.get('physics_pair_probe', {}).values()) and res.get('sawyer_agents_probe', {'passed': True})['passed'] and \
      all(leg['passed'] for kind in res['population_and_pair_legs'].values() for leg in kind.values())
  res['passed'] = ok
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(res, f, indent=1)
      f.write('\n')
  print(json.dumps(res))
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  main()

"""A population of P = N / 16 policies on the minitaur (N = 4096, 32 -> 64 -> 64 -> 8, T = 250) and the kitchen (N = 2048, 46 -> 64 -> 64 -> 9, T = 400): the README's
shapes, G = 16 envs per member, four ways over the same T env steps from the reset state:
  (a) single_policy   ONE rollout_policy launch of one policy at N: the floor (every wave reads the same weights)
  (b) population      rollout_population(pop, T): ONE launch, every env through its member, every [T] array written
  (c) per_member      the P rollout_policy launches on a 16-env env, one per member, that the population launch replaces (--c-launches K < P: K of them are timed and
                      the time is scaled by P / K; the launches are sequential and alike)
  (d) evaluate        evaluate_population(pop, T, reset_first=False): the same launch writing summaries only, with its peak memory next to (b)'s
Device events after warm-up; the legs are interleaved over --reps repetitions, every run from the same env state; per leg median / min / max ms and the spread.
The members are perturbed copies of one network, so (a) and (b) walk through different trajectories (contacts, active-set passes): a difference between them below the
legs' spreads cannot be separated from that, and the tool says so per env (`a_b_separable`).
This process never opens the GPU: every env's legs run in a child process of their own, one at a time.
--parent-lib PATH: the gate on the shared kernels.  The single-policy rollout_policy and the open-loop rollout of both envs are timed in child processes that load this
build and another build of libearl_hip.so (the parent commit's), taking turns; each leg of this build must stay within max(5 %, 3 x the other build's own spread) of
the other build's median.  The result is part of the JSON; a miss ends the tool with exit status 1.

  python tools/physics_population_probe.py [--reps 5] [--envs minitaur,kitchen] [--parent-lib /path/to/libearl_hip.so] [--out-dir profiles]
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

import kitchen_policy_probe as kit      # noqa: E402  (the shapes, the networks and the timing of the single-policy probes)
import minitaur_policy_probe as mt      # noqa: E402

G = 16
SHAPE = {'minitaur': dict(mod=mt, n=4096, T=250, obs=32, act=8), 'kitchen': dict(mod=kit, n=2048, T=400, obs=46, act=9)}
HIDDEN = (64, 64)


def population(torch, kind, P, sigma=0.01):
  """P perturbed copies of one small-gain network (an evolution strategy's population)"""
  from earl_benchmark_amd.policy import MLPPolicy, PolicyPopulation
  s = SHAPE[kind]
  pi = MLPPolicy(s['mod'].layers_of(HIDDEN), 'relu', 'tanh', device='cuda', obs_dim=s['obs'], act_dim=s['act'])
  gen = torch.Generator(device='cuda').manual_seed(5)
  theta = pi.params[None, :] + sigma * torch.randn(P, pi.params.numel(), generator=gen, device='cuda')
  return pi, PolicyPopulation(pi, params=theta, envs_per_policy=G, device='cuda', obs_dim=s['obs'], act_dim=s['act'])


def probe(torch, kind, reps, c_launches):
  from earl_benchmark_amd.policy import MLPPolicy
  s = SHAPE[kind]
  n, T, P = s['n'], s['T'], s['n'] // G
  env, small = s['mod'].make(n), s['mod'].make(G)
  pi, pop = population(torch, kind, P)
  snap, snap_small = env.state_dict(), small.state_dict()
  out = env.rollout_population(pop, T)
  guard = float((out['status'] != 0).float().mean())
  out_small = small.rollout_policy(pi, T)
  member = MLPPolicy(s['mod'].layers_of(HIDDEN), 'relu', 'tanh', device='cuda', obs_dim=s['obs'], act_dim=s['act'])      # its struct is pointed at one row of pop.params per launch
  K = min(c_launches, P)

  def per_member():
    for p in range(K):
      member.struct.params = pop.params[p].data_ptr()
      small.rollout_policy(member, T, out=out_small)

  def restore():
    env.load_state_dict(snap)
    small.load_state_dict(snap_small)
  legs = {'single_policy': lambda: env.rollout_policy(pi, T, out=out), 'population': lambda: env.rollout_population(pop, T, out=out), 'per_member': per_member,
          'evaluate': lambda: env.evaluate_population(pop, T, reset_first=False)}
  ms = s['mod'].interleaved(torch, legs, reps, restore, warmup=1)
  ms['per_member'] = [x * P / K for x in ms['per_member']]
  res = {'n': n, 'T': T, 'P': P, 'G': G, 'net': [s['obs']] + list(HIDDEN) + [s['act']], 'population_bytes': int(pop.params.numel() * 4), 'guard_share': guard,
         'per_member_launches_timed': K, 'device': torch.cuda.get_device_name(0)}
  for k in legs:
    res[k] = s['mod'].summary(ms[k], n, T)
  med = lambda k: res[k]['ms_median']
  res['population_over_single_policy'] = med('population') / med('single_policy')
  res['population_over_per_member'] = med('population') / med('per_member')
  res['evaluate_over_population'] = med('evaluate') / med('population')
  # (a) and (b) run different trajectories: their difference counts only beyond the two legs' own spreads
  res['a_b_separable'] = abs(med('population') - med('single_policy')) > max(res['population']['ms_max'] - res['population']['ms_min'],
                                                                              res['single_policy']['ms_max'] - res['single_policy']['ms_min'])
  # peak memory of one (b) and one (d) above what is resident before it (env state, weights): (b) allocates its [T] outputs, (d) none
  del out
  for name, fn in (('population', lambda: env.rollout_population(pop, T)), ('evaluate', lambda: env.evaluate_population(pop, T, reset_first=False))):
    restore()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    res[name]['max_memory_allocated_above_resident_bytes'] = int(torch.cuda.max_memory_allocated() - base)
    del r
  return res


def gate_legs(torch, kind, reps):
  """(child process) the two legs of the gate at the README's shape: what both builds can run"""
  from earl_benchmark_amd.policy import MLPPolicy
  s = SHAPE[kind]
  env = s['mod'].make(s['n'])
  pi = MLPPolicy(s['mod'].layers_of(HIDDEN), 'relu', 'tanh', device='cuda', obs_dim=s['obs'], act_dim=s['act'])
  snap = env.state_dict()
  out = env.rollout_policy(pi, s['T'])
  acts = out['actions'].clone()
  ms = s['mod'].interleaved(torch, {'rollout_policy': lambda: env.rollout_policy(pi, s['T'], out=out), 'rollout': lambda: env.rollout(acts, out=out)}, reps,
                            lambda: env.load_state_dict(snap), warmup=1)
  return {k: [round(x, 3) for x in v] for k, v in ms.items()}


def older_build(path):
  """load another build of libearl_hip.so: it does not export the population entry points, its single-policy ones take the call"""
  from earl_benchmark_amd import _abi
  _abi.LIB_PATH = path
  for name in ('earl_minitaur_population_rollout', 'earl_kitchen_population_rollout'):
    _abi.SIGNATURES.pop(name, None)
  lib = _abi.load()
  lib.earl_minitaur_population_rollout = lambda model, col, cfg, st, pol, pop, head, obs0, T, clock, actions, out, summ, stream: \
      lib.earl_minitaur_policy_rollout(model, col, cfg, st, pol, head, obs0, T, clock, actions, out, stream)
  lib.earl_kitchen_population_rollout = lambda model, col, params, cfg, st, pol, pop, head, obs0, T, clock, actions, out, summ, stream: \
      lib.earl_kitchen_policy_rollout(model, col, params, cfg, st, pol, head, obs0, T, clock, actions, out, stream)


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='minitaur,kitchen')
  ap.add_argument('--c-launches', type=int, default=8, help='per-member launches timed in leg (c), scaled to P')
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--gate-only', action='store_true', help='skip the four legs (with --parent-lib)')
  ap.add_argument('--out-dir', default=None, help='also write <env>_population_probe.json per env into this directory (profiles)')
  ap.add_argument('--gate-child', default=None, help='(child process) load this libearl_hip.so (or "own") and time the gate\'s legs of --envs')
  ap.add_argument('--legs-child', default=None, help='(child process) the four legs of this env')
  a = ap.parse_args()
  kinds = a.envs.split(',')
  if a.gate_child:
    if a.gate_child != 'own':
      older_build(a.gate_child)
    import torch
    print(json.dumps({kind: gate_legs(torch, kind, a.reps) for kind in kinds}))
    return
  if a.legs_child:
    import torch
    print(json.dumps(probe(torch, a.legs_child, a.reps, a.c_launches)))
    return

  def child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--c-launches', str(a.c_launches), *args], capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
      raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])
  res = {kind: {'tool': 'physics_population_probe', 'env': kind,
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
      with open(os.path.join(a.out_dir, f'{kind}_population_probe.json'), 'w') as f:
        json.dump(res[kind], f, indent=1)
        f.write('\n')
  print(json.dumps(res))
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  main()

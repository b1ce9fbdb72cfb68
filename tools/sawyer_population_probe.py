"""A population of P = 512 policies on the Sawyer door and peg, N = 8192 envs, G = 16 envs per member, four ways over the same T env steps from the reset state:
  (a) per_member      the P rollout_policy launches on a 16-env env, one per member, that the population launch replaces (--a-launches K < P: K of them are timed
                      and the time is scaled by P / K; the launches are sequential and alike)
  (b) single_policy   ONE rollout_policy launch of one policy at N: the floor (every wavefront reads the same weights)
  (c) population      rollout_policy(pop, T): ONE launch, every env through its member, every [T] array written
  (d) evaluate        evaluate_policy(pop, T, reset_first=False): the same launch writing summaries only
for two networks (14 -> 64 -> 64 -> 4 and 14 -> 256 -> 256 -> 4; 512 copies of the wide one are 145 MB: they sit in Infinity Cache, not in the 4 MiB L2s) and two
lengths (T = 20 and the bench's: door 300, peg 200).  Device events after warm-up; the legs are interleaved over --reps repetitions, every run from the same env
state; per leg median / min / max ms, the ratios (c)/(a), (c)/(b), (d)/(c), and torch.cuda.max_memory_allocated over (c) and over (d).
--parent-lib PATH: the gate on the shared kernel.  The single-policy rollout_policy and the open-loop rollout of door and peg are timed in child processes that
load this build and another build of libearl_hip.so (the parent commit's), taking turns; each leg of this build must stay within max(5 %, 3 x the other build's own
spread) of the other build's median.  The result is part of the JSON; a miss ends the tool with exit status 1.

  python tools/sawyer_population_probe.py [--reps 5] [--envs door,peg] [--parent-lib /path/to/libearl_hip.so] [--out profiles/sawyer_population_probe.json]
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

from sawyer_policy_probe import BENCH_T, NETS, interleaved, layers_of, make, summary      # noqa: E402  (the shapes, the networks and the timing of the single-policy probe)

N, G, P = 8192, 16, 512


def population(torch, hidden, sigma=0.01):
  """P perturbed copies of one small-gain network (an evolution strategy's population)"""
  from earl_benchmark_amd.policy import MLPPolicy, PolicyPopulation
  pi = MLPPolicy(layers_of(hidden), 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4)
  gen = torch.Generator(device='cuda').manual_seed(5)
  theta = pi.params[None, :] + sigma * torch.randn(P, pi.params.numel(), generator=gen, device='cuda')
  return pi, PolicyPopulation(pi, params=theta, envs_per_policy=G, device='cuda', obs_dim=14, act_dim=4)


def probe(torch, kind, T, hidden, reps, a_launches):
  from earl_benchmark_amd.policy import MLPPolicy
  env, small = make(kind, N), make(kind, G)
  pi, pop = population(torch, hidden)
  snap, snap_small = env.state_dict(), small.state_dict()
  out = env.rollout_policy(pop, T)
  guard = float((out['status'] != 0).float().mean())
  out_small = small.rollout_policy(pi, T)
  member = MLPPolicy(layers_of(hidden), 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4)      # its struct is pointed at one row of pop.params per launch
  K = min(a_launches, P)

  def per_member():
    for p in range(K):
      member.struct.params = pop.params[p].data_ptr()
      small.rollout_policy(member, T, out=out_small)

  def restore():
    env.load_state_dict(snap)
    small.load_state_dict(snap_small)
  legs = {'per_member': per_member, 'single_policy': lambda: env.rollout_policy(pi, T, out=out), 'population': lambda: env.rollout_policy(pop, T, out=out),
          'evaluate': lambda: env.evaluate_policy(pop, T, reset_first=False)}
  ms = interleaved(torch, legs, reps, restore, warmup=1)
  ms['per_member'] = [x * P / K for x in ms['per_member']]
  res = {'n': N, 'T': T, 'P': P, 'G': G, 'net': [14] + list(hidden) + [4], 'population_bytes': int(pop.params.numel() * 4), 'guard_share': guard,
         'per_member_launches_timed': K}
  for k in legs:
    res[k] = summary(ms[k], N, T)
  med = lambda k: res[k]['ms_median']
  res['population_over_per_member'] = med('population') / med('per_member')
  res['population_over_single_policy'] = med('population') / med('single_policy')
  res['evaluate_over_population'] = med('evaluate') / med('population')
  # peak memory of one (c) and one (d) above what is resident before it (env state, weights): (c) allocates its [T] outputs, (d) none
  del out
  for name, fn in (('population', lambda: env.rollout_policy(pop, T)), ('evaluate', lambda: env.evaluate_policy(pop, T, reset_first=False))):
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
  """(child process) the two legs of the gate at N, the bench's T, the 64 x 64 network: what both builds can run"""
  from earl_benchmark_amd.policy import MLPPolicy
  T = BENCH_T[kind]
  env = make(kind, N)
  pi = MLPPolicy(layers_of(NETS['64x64']), 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4)
  snap = env.state_dict()
  out = env.rollout_policy(pi, T)
  acts = out['actions'].clone()
  ms = interleaved(torch, {'rollout_policy': lambda: env.rollout_policy(pi, T, out=out), 'rollout': lambda: env.rollout(acts, out=out)}, reps,
                   lambda: env.load_state_dict(snap), warmup=1)
  return {k: [round(x, 3) for x in v] for k, v in ms.items()}


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--a-launches', type=int, default=P, help='per-member launches timed in leg (a) at T = 20')
  ap.add_argument('--a-launches-long', type=int, default=P, help='... at the bench\'s T')
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--gate-only', action='store_true', help='skip the four legs (with --parent-lib)')
  ap.add_argument('--out', default=None, help='also write the JSON object to this file (profiles/sawyer_population_probe.json)')
  ap.add_argument('--gate-child', default=None, help='(child process) load this libearl_hip.so (or "own") and time the gate\'s legs')
  a = ap.parse_args()
  kinds = a.envs.split(',')
  if a.gate_child:
    from earl_benchmark_amd import _abi
    if a.gate_child != 'own':
      _abi.LIB_PATH = a.gate_child
      _abi.SIGNATURES.pop('earl_sawyer_population_rollout', None)        # (the older build does not export it: its single-policy entry point takes the call)
      lib = _abi.load()
      lib.earl_sawyer_population_rollout = lambda model, col, nv, cfg, st, pol, pop, head, obs0, T, clock, actions, out, summ, stream: \
          lib.earl_sawyer_policy_rollout(model, col, nv, cfg, st, pol, head, obs0, T, clock, actions, out, stream)
    import torch
    print(json.dumps({kind: gate_legs(torch, kind, a.reps) for kind in kinds}))
    return

  def child(lib):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--envs', a.envs, '--gate-child', lib], capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
      raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])
  res = {'tool': 'sawyer_population_probe', 'timing': 'device events after 1 warm-up run, legs interleaved over the repetitions, every run from the same env state'}
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
      res[kind] = {}
      for T in (20, BENCH_T[kind]):
        for name, hidden in NETS.items():
          res[kind][f'T{T}_{name}'] = probe(torch, kind, T, hidden, a.reps, a.a_launches if T == 20 else a.a_launches_long)
          print(f'{kind} T{T} {name}: done', file=sys.stderr, flush=True)
          torch.cuda.empty_cache()
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(res, f, indent=1)
      f.write('\n')
  print(json.dumps(res))
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  main()

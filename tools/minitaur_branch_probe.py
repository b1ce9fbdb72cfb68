"""Times the minitaur's branch launch and planner on one MI355X -> profiles/minitaur_branch_probe.json.

Protocol: H = 20; per shape the outputs of all routes are compared for equality first; then medians of five interleaved repetitions with max - min, each repetition
timed by device events around one call after a warm-up call.  Shapes (N, K) = (16, 256), (64, 64), (1024, 4): 4096 virtual envs each.
  branch      env.branch_rollout(actions [K, H, N, 8])
  loop (a)    the route it replaces: K x (load_state_dict, rollout(actions[k]), three torch reductions)
  batch (b)   ONE plain rollout of K N envs at the same H through the same library (another env of K N envs: the cost of the physics alone)
  plan        env.mppi_plan(I = 1) against torch.randn -> clamp -> branch_rollout -> softmax -> weighted sum in torch
A cell is FAVOURABLE when branch is within the two spreads together of (b), UNFAVOURABLE otherwise (the replicate kernel and the lost [T] stores are all that differ).
--parent-lib PATH: the parent commit's libearl_hip.so; in this process `rollout` and `rollout_policy` (the population entry point without a population: the same
kernels) at N = 4096 are timed through both libraries and their outputs compared bit for bit (the kernels are byte-identical: the difference must stay inside the two spreads together)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from earl_benchmark_amd import _abi                                       # noqa: E402
from earl_benchmark_amd.envs.minitaur import Minitaur                     # noqa: E402

H, REPS = 20, 5


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  a.record()
  fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b)


def interleaved(routes):
  """{name: fn} -> {name: {median_ms, spread_ms, ms}}: one warm-up each, then REPS rounds, every route once per round"""
  for fn in routes.values():
    fn()
  ms = {k: [] for k in routes}
  for _ in range(REPS):
    for k, fn in routes.items():
      ms[k].append(timed(fn))
  return {k: dict(median_ms=statistics.median(v), spread_ms=max(v) - min(v), ms=v) for k, v in ms.items()}


def reduce3(out):
  s = out['success']
  first = torch.where(s.any(0), s.to(torch.int8).argmax(0), torch.full_like(s[0], -1, dtype=torch.int64))
  return out['reward'].sum(0), s[-1], first


def shape_cell(n, K, seed=3):
  env = Minitaur(num_envs=n, seed=seed, scalar_api=False)
  big = Minitaur(num_envs=n * K, seed=seed, scalar_api=False)
  g = torch.Generator(device='cuda').manual_seed(1)
  acts = (torch.rand(K, H, n, 8, generator=g, device='cuda') * 2 - 1).float()
  flat = acts.permute(1, 0, 2, 3).reshape(H, K * n, 8).contiguous()
  sd, bsd = env.state_dict(), big.state_dict()

  def loop():
    rows = []
    for k in range(K):
      env.load_state_dict(sd)
      rows.append(reduce3(env.rollout(acts[k])))
    env.load_state_dict(sd)
    return rows

  def batch():
    big.load_state_dict(bsd)
    return big.rollout(flat)

  got = env.branch_rollout(acts)
  rows = loop()
  equal = all(torch.equal(got['success'][k], rows[k][1]) and torch.equal(got['first_success'][k].long(), rows[k][2].long()) for k in range(K))
  # (ret: torch's sum is a tree, the launch's is t ascending: compared to rounding here, bit for bit in tests/test_minitaur_branches_gpu.py)
  close = all(torch.allclose(got['ret'][k], rows[k][0], rtol=1e-12, atol=1e-12) for k in range(K))
  res = interleaved({'branch': lambda: env.branch_rollout(acts), 'loop_a': loop, 'batch_b': batch})
  within = abs(res['branch']['median_ms'] - res['batch_b']['median_ms']) <= res['branch']['spread_ms'] + res['batch_b']['spread_ms']
  faster = res['branch']['median_ms'] <= res['batch_b']['median_ms']
  return dict(N=n, K=K, H=H, outputs_equal=bool(equal and close), **res, speedup_over_loop=res['loop_a']['median_ms'] / res['branch']['median_ms'],
              verdict='FAVOURABLE' if within or faster else 'UNFAVOURABLE')


def plan_cell(n, K, seed=3):
  env = Minitaur(num_envs=n, seed=seed, scalar_api=False)
  mean = torch.zeros(H, n, 8, device='cuda')

  def in_torch():
    a = (mean[None] + 0.3 * torch.randn(K, H, n, 8, device='cuda')).clamp(-1, 1)
    a[0] = mean
    r = env.branch_rollout(a)['ret']
    w = torch.softmax(r.float(), 0)
    return (w[:, None, :, None] * a).sum(0)

  res = interleaved({'mppi_plan': lambda: env.mppi_plan(mean, K=K, sigma=0.3), 'torch_composition': in_torch, 'branch_alone': lambda: env.branch_rollout(mean, K=K)})
  own = res['mppi_plan']['median_ms'] - res['branch_alone']['median_ms']
  return dict(N=n, K=K, H=H, **res, planner_kernels_ms=own, planner_kernels_share=own / res['mppi_plan']['median_ms'])


def parent_cell(path, n=4096, T=H, seed=3):
  from earl_benchmark_amd.policy import MLPPolicy
  parent = C.CDLL(path)
  for name, argtypes in _abi.SIGNATURES.items():
    if hasattr(parent, name):
      fn = getattr(parent, name)
      fn.argtypes, fn.restype = argtypes, _abi._RESTYPES.get(name, C.c_int)
  here, there = Minitaur(num_envs=n, seed=seed, scalar_api=False), Minitaur(num_envs=n, seed=seed, scalar_api=False)
  there._lib = parent
  g = torch.Generator(device='cuda').manual_seed(2)
  acts = (torch.rand(T, n, 8, generator=g, device='cuda') * 2 - 1).float()
  rng = np.random.default_rng(0)
  layers = [((rng.standard_normal((16, 32)) / np.sqrt(32)).astype(np.float32), np.zeros(16, np.float32)),
            ((rng.standard_normal((8, 16)) / 4).astype(np.float32), np.zeros(8, np.float32))]
  pi = MLPPolicy(layers, 'relu', 'tanh', device='cuda', obs_dim=32, act_dim=8)
  sds = {id(e): e.state_dict() for e in (here, there)}

  def roll(e):
    e.load_state_dict(sds[id(e)])
    return e.rollout(acts)

  def pop(e):
    e.load_state_dict(sds[id(e)])
    return e.rollout_policy(pi, T)

  a, b = roll(here), roll(there)
  identical = {'rollout': all(torch.equal(a[k], b[k]) for k in a)}
  routes = {'rollout_this': lambda: roll(here), 'rollout_parent': lambda: roll(there), 'population_this': lambda: pop(here), 'population_parent': lambda: pop(there)}
  a, b = pop(here), pop(there)
  identical['rollout_population'] = all(torch.equal(a[k], b[k]) for k in a)
  res = interleaved(routes)
  ok = lambda x, y: abs(res[x]['median_ms'] - res[y]['median_ms']) <= res[x]['spread_ms'] + res[y]['spread_ms']
  inside = {'rollout': ok('rollout_this', 'rollout_parent'), 'rollout_population': ok('population_this', 'population_parent')}
  return dict(N=n, T=T, bit_identical=identical, inside_two_spreads=inside, **res)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'minitaur_branch_probe.json'))
  args = ap.parse_args()
  doc = dict(device=torch.cuda.get_device_name(0), protocol=f'H = {H}; medians of {REPS} interleaved repetitions, spread = max - min; outputs compared first',
             shapes=[shape_cell(n, K) for n, K in ((16, 256), (64, 64), (1024, 4))], planner=[plan_cell(16, 256), plan_cell(64, 64)])
  if args.parent_lib:
    doc['parent_build'] = parent_cell(args.parent_lib)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(doc, f, indent=1)
  print(json.dumps({k: v for k, v in doc.items() if k != 'protocol'}, indent=1)[:6000])


if __name__ == '__main__':
  main()

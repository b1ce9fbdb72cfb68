"""What the Sawyer CEM planning step (earl_sawyer_plan_cem, env.plan_cem) costs next to the route it replaces, next to MPPI and next to the branch launch inside it,
and what its O(K) elite selection costs next to MPPI's update.  Door and peg, sparse reward, H = 20, one iteration, E = K / 8, the branch probe's three shapes
(N envs, K candidates): (16, 256), (64, 64), (1024, 8).  Four legs:
  (a) plan_cem       env.plan_cem(mean, K=, elites=K/8, iterations=1, out=): the candidates kernel, the branch launch, the update kernel
  (b) torch_route    the route on public methods: env.cem_candidates -> env.rollout_branches -> torch.topk -> mean / std of the elites in torch
  (c) plan_mppi      env.plan_mppi(mean, K=, iterations=1, out=)
  (d) branches       env.rollout_branches(actions [K, H, N, 4]) alone: what all of them contain
Device events around each run after one warm-up round, the legs taking turns inside each of --reps repetitions; no leg moves the env, so every run starts from the
same state; per leg the median, min, max, spread = max - min.  UNFAVOURABLE where (a) is not below (b) by more than the two spreads together.
The update alone: earl_sawyer_cem_update on random returns at n = 16, H = 20, K = 256, 1024, 8192 (E = K / 8), device events around --inner back-to-back launches,
medians of --reps.  MPPI's update kernel has no entry point of its own: its time inside plan_mppi at the same shapes (and the CEM update's, inside plan_cem) come
from a kernel trace taken in a run of its own (`--trace-only` under `rocprofv3 --kernel-trace`, door, 1 warm-up + 5 calls per K of each planner), handed to the timed
run with --kernel-trace FILE.  The multiple is recorded, not asserted.

  python tools/sawyer_cem_probe.py [--reps 5] [--inner 20] [--envs door,peg] [--kernel-trace FILE] [--out profiles/sawyer_cem_probe.json]
"""
import argparse
import csv
import ctypes as C
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sawyer_branch_probe import H, SHAPES, summary      # noqa: E402  (the branch probe's shapes and figures)
from sawyer_policy_probe import interleaved, make      # noqa: E402  (the Sawyer probes share their method)

SIGMA, TEMPERATURE = 0.3, 1.0
UPDATE_N, UPDATE_KS, TRACE_CALLS = 16, (256, 1024, 8192), 5


def probe(torch, kind, n, K, reps):
  E = max(K // 8, 1)
  env = make(kind, n)
  gen = torch.Generator(device='cuda').manual_seed(7)
  env.rollout((torch.rand(5, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous())        # off the reset state
  mean = ((torch.rand(H, n, 4, device='cuda', generator=gen) * 2 - 1) * 0.5).contiguous()
  acts = (torch.rand(K, H, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous()
  f64 = dict(dtype=torch.float64, device='cuda')
  out = {'plan': torch.empty(H, n, 4, device='cuda'), 'std': torch.empty(H, n, 4, device='cuda'), 'ret': torch.empty(K, n, **f64), 'ret0': torch.empty(1, n, **f64),
         'best_ret': torch.empty(n, **f64), 'best_k': torch.empty(n, dtype=torch.int32, device='cuda'), 'elite': torch.empty(K, n, dtype=torch.uint8, device='cuda'),
         'fail': torch.empty(K, n, dtype=torch.int32, device='cuda')}
  mout = {k: (torch.empty_like(v) if k != 'plan' else torch.empty(H, n, 4, device='cuda')) for k, v in out.items() if k not in ('std', 'elite')}
  got = {}

  def plan_cem():
    env.plan_cem(mean, K=K, elites=E, iterations=1, sigma=SIGMA, noise_counter=3, out=out)

  def torch_route():
    act = env.cem_candidates(mean, K, sigma=SIGMA, noise_counter=3)
    br = env.rollout_branches(act)
    idx = torch.topk(br['ret'], E, dim=0).indices                                          # [E, n]
    el = torch.gather(act, 0, idx[:, None, :, None].expand(E, H, n, 4))
    got['plan'], got['std'] = el.mean(0).clamp_(-1, 1), el.std(0, unbiased=False).clamp_(0.0, 2.0)

  def plan_mppi():
    env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=mout)

  def branches():
    got.update(env.rollout_branches(acts))

  legs = {'a_plan_cem': plan_cem, 'b_torch_route': torch_route, 'c_plan_mppi': plan_mppi, 'd_branches': branches}
  ms = interleaved(torch, legs, reps, lambda: None, warmup=1)
  res = {k: summary(v, n * K * H) for k, v in ms.items()}
  a, b, c, d = (res[k] for k in legs)
  faster_than_b = b['ms_median'] - a['ms_median'] > a['spread_ms'] + b['spread_ms']
  return {'n': n, 'K': K, 'E': E, 'H': H, 'iterations': 1, 'virtual_envs': n * K, 'candidate_bytes': K * H * n * 16,
          'share_of_branches_with_a_rolled_back_step': round(float((out['fail'] != 0).float().mean()), 5),
          'plan_max_abs_difference_a_b': float((out['plan'] - got['plan']).abs().max()),   # (the same candidates; torch.topk breaks ties its own way)
          'legs': res,
          'b_over_a': round(b['ms_median'] / a['ms_median'], 3), 'a_over_c': round(a['ms_median'] / c['ms_median'], 3), 'a_minus_d_ms': round(a['ms_median'] - d['ms_median'], 3),
          'a_minus_d_within_spreads': bool(abs(a['ms_median'] - d['ms_median']) <= a['spread_ms'] + d['spread_ms']),
          'a_faster_than_b_beyond_spreads': bool(faster_than_b), 'verdict': ['favourable'] if faster_than_b else ['UNFAVOURABLE: (a) is not faster than (b) beyond the spreads']}


def update_alone(torch, K, reps, inner):
  """earl_sawyer_cem_update alone on random returns and candidates: n = 16, H = 20, E = K / 8 -> microseconds per launch"""
  from earl_benchmark_amd import _abi
  lib = _abi.load()
  n, E = UPDATE_N, K // 8
  gen = torch.Generator(device='cuda').manual_seed(K)
  mean = ((torch.rand(H, n, 4, device='cuda', generator=gen) * 2 - 1) * 0.5).contiguous()
  act = (torch.rand(K, H, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous()
  act[0] = mean
  ret = torch.randn(K, n, dtype=torch.float64, device='cuda', generator=gen)
  plan, std = torch.empty_like(mean), torch.empty_like(mean)
  elite = torch.empty(K, n, dtype=torch.uint8, device='cuda')
  cfg = _abi.SawyerCfg(n=n, env_offset=0, seed=1)
  pp = _abi.SawyerCemParams(K=K, H=H, iterations=1, iteration0=0, elites=E, sigma=(C.c_float * 4)(*[SIGMA] * 4), noise_counter=3, alpha=0.0, std_min=0.0, std_max=2.0)
  stream = torch.cuda.current_stream().cuda_stream

  def launch():
    _abi.check(lib.earl_sawyer_cem_update(C.byref(cfg), C.byref(pp), 0, mean.data_ptr(), None, act.data_ptr(), ret.data_ptr(), plan.data_ptr(), std.data_ptr(), None, None,
                                          None, elite.data_ptr(), stream), 'earl_sawyer_cem_update')

  us = {}
  for name, r in (('random_returns', ret), ('equal_returns', torch.zeros_like(ret))):       # equal returns: the sparse reward's case, every key in one bin
    ret.copy_(r)
    launch()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(inner):
        launch()
      e1.record()
      torch.cuda.synchronize()
      t.append(e0.elapsed_time(e1) * 1e3 / inner)
    us[name] = {'us_median': round(statistics.median(t), 3), 'us_min': round(min(t), 3), 'us_max': round(max(t), 3), 'spread_us': round(max(t) - min(t), 3)}
  return {'n': n, 'K': K, 'E': E, 'H': H, 'inner': inner, 'elites_found': int(elite.sum()), 'timing': 'device events around `inner` back-to-back launches: launch gaps included', **us}


def trace_only(torch):
  """the calls a kernel trace is taken over: per K, 1 + TRACE_CALLS calls of plan_mppi, then as many of plan_cem (door, n = 16, H = 20, sparse)"""
  env = make('door', UPDATE_N)
  mean = torch.zeros(H, UPDATE_N, 4, device='cuda')
  for K in UPDATE_KS:
    for _ in range(1 + TRACE_CALLS):
      env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3)
    for _ in range(1 + TRACE_CALLS):
      env.plan_cem(mean, K=K, elites=K // 8, iterations=1, sigma=SIGMA, noise_counter=3)
    torch.cuda.synchronize()
  return 0


def kernel_times(path):
  """{kernel: {K: dict(us_median, us_min, us_max)}} of the two update kernels from a rocprofv3 kernel_trace.csv taken over trace_only(): the dispatches of a kernel in
  the order of their start, 1 + TRACE_CALLS per K, the first of each group dropped"""
  rows = {}
  for row in csv.DictReader(open(path)):
    for name in ('sawyer_plan_update_kernel', 'sawyer_cem_update_kernel'):
      if name in row['Kernel_Name']:
        rows.setdefault(name, []).append((int(row['Start_Timestamp']), int(row['End_Timestamp'])))
  out = {}
  for name, r in rows.items():
    r.sort()
    if len(r) != len(UPDATE_KS) * (1 + TRACE_CALLS):
      raise SystemExit(f'{path}: {len(r)} dispatches of {name}, expected {len(UPDATE_KS) * (1 + TRACE_CALLS)}')
    for g, K in enumerate(UPDATE_KS):
      us = [(e - s) / 1e3 for s, e in r[g * (1 + TRACE_CALLS) + 1:(g + 1) * (1 + TRACE_CALLS)]]
      out.setdefault(name, {})[f'K{K}'] = {'us_median': round(statistics.median(us), 3), 'us_min': round(min(us), 3), 'us_max': round(max(us), 3), 'calls': len(us)}
  return out


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=20)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--trace-only', action='store_true')
  ap.add_argument('--kernel-trace')
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/sawyer_cem_probe.py measures on the GPU: no HIP device visible')
  if args.trace_only:
    return trace_only(torch)
  res = {'what': 'tools/sawyer_cem_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'boxes': 1, 'build': eb.__version__,
         'reward': 'sparse', 'H': H, 'iterations': 1, 'elites': 'K / 8', 'sigma': SIGMA, 'temperature': TEMPERATURE, 'reps': args.reps, 'warmup': 1,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count),
         'timing': 'device events around one run, legs interleaved over the repetitions, every run from the same env state (no leg moves the env); spread = max - min'}
  for kind in args.envs.split(','):
    res[kind] = {}
    for n, K in SHAPES:
      res[kind][f'N{n}_K{K}'] = probe(torch, kind, n, K, args.reps)
      print(f'{kind} N={n} K={K}: done', file=sys.stderr, flush=True)
      torch.cuda.empty_cache()
  res['update_alone'] = {f'K{K}': update_alone(torch, K, args.reps, args.inner) for K in UPDATE_KS}
  if args.kernel_trace:
    kt = kernel_times(args.kernel_trace)
    res['kernel_trace'] = {'source': 'rocprofv3 --kernel-trace over --trace-only, a run of its own: door, n = 16, H = 20, sparse, 5 calls per K after one warm-up', 'kernels': kt}
    if len(kt) == 2:
      res['kernel_trace']['cem_update_over_mppi_update'] = {k: round(kt['sawyer_cem_update_kernel'][k]['us_median'] / kt['sawyer_plan_update_kernel'][k]['us_median'], 3)
                                                            for k in kt['sawyer_cem_update_kernel']}
  else:
    res['kernel_trace'] = 'not measured'
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

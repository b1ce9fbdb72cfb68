"""What the discount and the terminal value net cost in the Sawyer MPPI planning step (earl_sawyer_plan_mppi_value, env.plan_mppi(discount=, value=)) next to the route
they replace and next to the value-free call.  Door and peg, sparse reward, H = 20, one iteration, the plan probe's three shapes (N envs, K candidates): (16, 256),
(64, 64), (1024, 8); value networks 14 -> 64 -> 64 -> 1 and 14 -> 256 -> 256 -> 1.  Four legs:
  (a) plan_mppi_value   env.plan_mppi(mean, K=, iterations=1, discount=0.99, value=V, out=): candidates, the discounted branch launch, the value kernel, the update
  (b) torch_route       what it replaces, on public methods: env.plan_candidates -> env.rollout_branches -> a torch MLP on last_obs (float32) -> softmax of the returns
                        and the weighted mean in torch.  discount = 1: that route cannot discount, a branch keeps no per-step reward
  (c) plan_mppi         env.plan_mppi(mean, K=, iterations=1, out=) without either keyword, on this build
  (d) plan_mppi_parent  the same call through the PARENT commit's libearl_hip.so (--parent: a path to that library), loaded beside this build's in the same process,
                        so that the four legs take turns inside each repetition (left out without --parent)
Device events around each run after one warm-up round, the legs taking turns inside each of --reps repetitions; no leg moves the env; per leg the median, min, max,
spread = max - min.  Reported per shape and network: (a) / (b) and (a) - (c) (recorded, not asserted: nobody has measured them before); UNFAVOURABLE where (a) is not
below (b) by more than the two spreads together.  THE ONE CONDITION: (c) against (d) within the two spreads together at every shape -- the value-free calls run the old
kernels, so a difference means something existing changed.
The value kernel's time alone comes from a kernel trace in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/sawyer_value_probe.py --trace-legs
  python tools/sawyer_value_probe.py --merge-trace DIR/.../*_kernel_trace.csv --out profiles/sawyer_value_probe.json      (adds 'value_kernel_us' to the JSON at --out)

  python tools/sawyer_value_probe.py [--reps 5] [--envs door,peg] [--parent PATH/libearl_hip.so] [--out profiles/sawyer_value_probe.json]
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
from sawyer_plan_probe import SIGMA, TEMPERATURE        # noqa: E402
from sawyer_policy_probe import interleaved, make       # noqa: E402  (the Sawyer probes share their method)

DISCOUNT = 0.99
NETS = {'64x64': (64, 64), '256x256': (256, 256)}
TRACE_RUNS = 6                                          # runs of leg (a) per (env, shape, network) under the kernel trace: the first is the warm-up


def value_net(hidden, seed=5):
  import numpy as np
  from earl_benchmark_amd.policy import MLPPolicy
  rng = np.random.default_rng(seed)
  dims = [14] + list(hidden) + [1]
  layers = [((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32)) for k, n in zip(dims[:-1], dims[1:])]
  return MLPPolicy(layers, 'relu', 'none', device='cuda', obs_dim=14, act_dim=1)


def parent_library(path):
  """the parent commit's library beside this build's: the same prototypes, for the entry points it has"""
  from earl_benchmark_amd import _abi
  lib = C.CDLL(path)
  for name, argtypes in _abi.SIGNATURES.items():
    if hasattr(lib, name):
      fn = getattr(lib, name)
      fn.argtypes, fn.restype = argtypes, _abi._RESTYPES.get(name, C.c_int)
  return lib


def outs(torch, n, K):
  return {'plan': torch.empty(H, n, 4, device='cuda'), 'ret': torch.empty(K, n, dtype=torch.float64, device='cuda'), 'ret0': torch.empty(1, n, dtype=torch.float64, device='cuda'),
          'best_ret': torch.empty(n, dtype=torch.float64, device='cuda'), 'best_k': torch.empty(n, dtype=torch.int32, device='cuda'),
          'fail': torch.empty(K, n, dtype=torch.int32, device='cuda')}


def setup(torch, kind, n):
  env = make(kind, n)
  gen = torch.Generator(device='cuda').manual_seed(7)
  env.rollout((torch.rand(5, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous())        # off the reset state
  mean = ((torch.rand(H, n, 4, device='cuda', generator=gen) * 2 - 1) * 0.5).contiguous()
  return env, mean


def probe(torch, kind, n, K, hidden, reps, parent):
  env, mean = setup(torch, kind, n)
  V = value_net(hidden)
  out = outs(torch, n, K)
  got = {}

  def plan_mppi_value():
    env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=out, discount=DISCOUNT, value=V)

  def torch_route():
    act = env.plan_candidates(mean, K, sigma=SIGMA, noise_counter=3)
    br = env.rollout_branches(act)
    ret = br['ret'] + V(br['last_obs'].to(torch.float32)).to(torch.float64)[..., 0]
    w = torch.softmax(ret / TEMPERATURE, 0)
    m = act[0]
    got['plan'] = (m + (w[:, None, :, None] * (act - m[None])).sum(0).to(torch.float32)).clamp_(-1, 1)

  def plan_mppi():
    env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=out)

  legs = {'a_plan_mppi_value': plan_mppi_value, 'b_torch_route': torch_route, 'c_plan_mppi': plan_mppi}
  if parent is not None:
    old, _ = setup(torch, kind, n)
    old._lib = parent                                    # (the structs and the device tables are the same on both sides of this commit)
    old_out = outs(torch, n, K)
    legs['d_plan_mppi_parent'] = lambda: old.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=old_out)
  ms = interleaved(torch, legs, reps, lambda: None, warmup=1)
  res = {k: summary(v, n * K * H) for k, v in ms.items()}
  a, b, c = (res[k] for k in ('a_plan_mppi_value', 'b_torch_route', 'c_plan_mppi'))
  faster_than_b = b['ms_median'] - a['ms_median'] > a['spread_ms'] + b['spread_ms']
  rec = {'n': n, 'K': K, 'H': H, 'iterations': 1, 'virtual_envs': n * K, 'value_net': [14] + list(hidden) + [1], 'discount': DISCOUNT, 'legs': res,
         'a_over_b': round(a['ms_median'] / b['ms_median'], 3), 'a_minus_c_ms': round(a['ms_median'] - c['ms_median'], 3),
         'a_minus_c_within_spreads': bool(abs(a['ms_median'] - c['ms_median']) <= a['spread_ms'] + c['spread_ms']),
         'a_faster_than_b_beyond_spreads': bool(faster_than_b), 'verdict': ['favourable'] if faster_than_b else ['UNFAVOURABLE: (a) is not faster than (b) beyond the spreads']}
  if parent is not None:
    d = res['d_plan_mppi_parent']
    same_bits = bool(torch.equal(out['plan'], old_out['plan'])) and bool(torch.equal(out['ret'], old_out['ret']))      # (leg (c) ran last on `out` among this build's legs)
    rec.update(c_minus_d_ms=round(c['ms_median'] - d['ms_median'], 3), c_and_d_spreads_ms=round(c['spread_ms'] + d['spread_ms'], 3),
               c_equals_d_within_spreads=bool(abs(c['ms_median'] - d['ms_median']) <= c['spread_ms'] + d['spread_ms']), c_and_d_same_bits=same_bits)
  return rec


def trace_legs(torch, kinds):
  """leg (a) alone, TRACE_RUNS runs per (env, shape, network) in a fixed order, for a kernel trace around this process"""
  for kind in kinds:
    for n, K in SHAPES:
      env, mean = setup(torch, kind, n)
      out = outs(torch, n, K)
      for hidden in NETS.values():
        V = value_net(hidden)
        for _ in range(TRACE_RUNS):
          env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=out, discount=DISCOUNT, value=V)
        torch.cuda.synchronize()


def merge_trace(path, kinds, out_path):
  """the value kernel's and the rollout kernel's dispatches of a kernel trace of --trace-legs, in order -> 'value_kernel_us' in the JSON at out_path"""
  rows = list(csv.DictReader(open(path)))
  dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
  value = [dur(r) for r in rows if 'sawyer_value_kernel' in r['Kernel_Name']]
  branch = [dur(r) for r in rows if 'sawyer_branch_rollout_kernel' in r['Kernel_Name']]
  cells = [(kind, f'N{n}_K{K}', net) for kind in kinds for n, K in SHAPES for net in NETS]
  assert len(value) == len(branch) == len(cells) * TRACE_RUNS, (len(value), len(branch), len(cells))
  res = json.load(open(out_path))
  rec = {}
  for i, (kind, shape, net) in enumerate(cells):
    v, b = value[i * TRACE_RUNS + 1:(i + 1) * TRACE_RUNS], branch[i * TRACE_RUNS + 1:(i + 1) * TRACE_RUNS]
    rec.setdefault(kind, {}).setdefault(shape, {})[net] = {'value_kernel_us_median': round(statistics.median(v), 2), 'value_kernel_us_min': round(min(v), 2),
                                                           'value_kernel_us_max': round(max(v), 2), 'discounted_rollout_kernel_us_median': round(statistics.median(b), 2),
                                                           'value_over_rollout': round(statistics.median(v) / statistics.median(b), 4)}
  res['value_kernel_us'] = {'how': f'rocprofv3 --kernel-trace around --trace-legs: {TRACE_RUNS} runs of leg (a) per cell, the first left out', **rec}
  with open(out_path, 'w') as fh:
    fh.write(json.dumps(res, indent=1) + '\n')
  print(json.dumps(res['value_kernel_us'], indent=1))


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--parent', help="the parent commit's libearl_hip.so: leg (d)")
  ap.add_argument('--trace-legs', action='store_true', help='run leg (a) alone for a kernel trace')
  ap.add_argument('--merge-trace', help='a kernel trace CSV of --trace-legs to merge into --out')
  ap.add_argument('--out')
  args = ap.parse_args()
  kinds = args.envs.split(',')
  if args.merge_trace:
    merge_trace(args.merge_trace, kinds, args.out)
    return 0
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/sawyer_value_probe.py measures on the GPU: no HIP device visible')
  if args.trace_legs:
    trace_legs(torch, kinds)
    return 0
  parent = parent_library(args.parent) if args.parent else None
  res = {'what': 'tools/sawyer_value_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'boxes': 1, 'build': eb.__version__,
         'reward': 'sparse', 'H': H, 'iterations': 1, 'sigma': SIGMA, 'temperature': TEMPERATURE, 'discount': DISCOUNT, 'reps': args.reps, 'warmup': 1,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count), 'parent_leg': parent is not None,
         'timing': 'device events around one run, legs interleaved over the repetitions in one process, every run from the same env state (no leg moves the env); '
                   'spread = max - min'}
  for kind in kinds:
    res[kind] = {}
    for n, K in SHAPES:
      for net, hidden in NETS.items():
        res[kind][f'N{n}_K{K}_V{net}'] = probe(torch, kind, n, K, hidden, args.reps, parent)
        print(f'{kind} N={n} K={K} V={net}: done', file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
  if parent is not None:
    cells = [res[k][c] for k in kinds for c in res[k]]
    res['the_one_condition'] = {'what': '(c) plan_mppi on this build against (d) the same call on the parent build: |median difference| <= the two spreads together',
                                'holds_everywhere': all(c['c_equals_d_within_spreads'] for c in cells), 'same_bits_everywhere': all(c['c_and_d_same_bits'] for c in cells)}
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

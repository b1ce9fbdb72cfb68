"""What the MPPI planning call (earl_tabletop_plan_mppi / earl_tabletop3_plan_mppi, env.plan_mppi) buys over the route it replaces.
N = 4096 envs, K = 64 candidates of H = 32 steps, I = 4 iterations, sparse reward, both tabletop envs, everything into preallocated tensors:
  (p) plan_mppi      env.plan_mppi(mean, iterations=4, out=...): per iteration a score and an update launch, the candidates never in memory
  (u) torch_route    per iteration: torch.randn([K, H, N, 3]) -> scale / add the mean / clamp -> env.rollout_branches -> softmax over K -> weighted sum: the route a
                     user of rollout_branches writes today (its own noise, so its plan is not comparable)
  (c) candidates     route (u) with earl_tabletop_plan_candidates in place of the torch sampling: the SAME candidates as (p), float32 softmax weights; its plan must
                     equal (p)'s to within float32 rounding -- the largest difference is reported, not asserted
  (b) branches       env.rollout_branches alone on one iteration's candidates (the 32 us launch of profiles/tabletop_branch_probe.json)
Device events around `--inner` back-to-back runs after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions; per leg the median, min and max of
the milliseconds per run, spread = max - min.
  (s) the score kernel alone has no entry point of its own: its time, the update kernel's and the branch kernel's come from a kernel trace taken in a run of its own
      (`--trace-only` under `rocprofv3 --kernel-trace --stats`: 20 calls of (p) and 80 of (b)), handed to the timed run with --kernel-stats FILE.  s / b is a
      finding, whichever way it falls.
BAR: (p) takes less time than (u) by more than the two spreads together.  Also recorded: the peak memory route (u) allocates beyond its inputs against (p)'s
[K, N] float64 workspace.  Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/tabletop_plan_probe.py [--reps 5] [--inner 5] [--kernel-stats FILE] [--out profiles/tabletop_plan_probe.json]
"""
import argparse
import csv
import ctypes as C
import datetime
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from tabletop3_policy_probe import interleaved      # noqa: E402 (the tabletop probes share their method)

N, K, H, I = 4096, 64, 32, 4
DEV = 'cuda'
SIGMA, TEMPERATURE, NOISE_COUNTER = 0.3, 1.0, 12345


def summary(ms):
  med = statistics.median(ms)
  return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'spread_ms': round(max(ms) - min(ms), 4),
          'ms_all': [round(x, 4) for x in ms]}


def setup(torch, nobj):
  if nobj == 1:
    from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  else:
    from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device=DEV, seed=1, reset_at_goal=True)    # (near the goal: both values of success occur)
  env._cfg.horizon = 10 * H
  gen = torch.Generator(device=DEV).manual_seed(7)
  env.rollout((torch.rand(5, N, 3, device=DEV, generator=gen) * 2 - 1).contiguous())        # off the reset state
  kw = dict(device=DEV)
  mean0 = ((torch.rand(H, N, 3, generator=gen, **kw) * 2 - 1) * 0.5).contiguous()
  bufs = {'mean': mean0.clone(), 'act': torch.empty(K, H, N, 3, **kw), 'eps': torch.empty(K, H, N, 3, **kw), 'ret': torch.empty(K, N, dtype=torch.float64, **kw),
          'm': torch.empty(H, N, 3, **kw)}
  out_p = {'plan': torch.empty(H, N, 3, **kw), 'ret': torch.empty(K, N, dtype=torch.float64, **kw), 'ret0': torch.empty(I, N, dtype=torch.float64, **kw),
           'best_ret': torch.empty(N, dtype=torch.float64, **kw), 'best_k': torch.empty(N, dtype=torch.int32, **kw)}
  lib = env._lib

  def plan_mppi(iterations=I):
    out = out_p if iterations == I else {'plan': out_p['plan'], 'ret': out_p['ret']}
    env.plan_mppi(mean0, K=K, iterations=iterations, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=NOISE_COUNTER, out=out)

  def reweight(mean):
    """softmax over K and the weighted sum, on the candidates in bufs['act'] around the clipped mean bufs['m'] -> the new mean, in place"""
    env.rollout_branches(bufs['act'], out={'ret': bufs['ret']})
    w = torch.softmax(bufs['ret'] * (1.0 / TEMPERATURE), 0).to(torch.float32)
    torch.sub(bufs['act'], bufs['m'][None], out=bufs['eps'])
    mean.copy_(torch.einsum('kn,khnd->hnd', w, bufs['eps'])).add_(bufs['m']).clamp_(-1, 1)

  def torch_route():
    mean = bufs['mean'].copy_(mean0)
    for _ in range(I):
      torch.clamp(mean, -1, 1, out=bufs['m'])
      torch.randn(bufs['eps'].shape, generator=gen, out=bufs['eps'], **kw)
      torch.add(bufs['m'][None], bufs['eps'], alpha=SIGMA, out=bufs['act']).clamp_(-1, 1)
      bufs['act'][0].copy_(bufs['m'])
      reweight(mean)

  def candidates(mean, j):
    pp = env._plan_params('probe', K, H, 1, 0, SIGMA, 1.0, NOISE_COUNTER)
    rc = lib.earl_tabletop_plan_candidates(C.byref(env._cfg), C.byref(pp), j, mean.data_ptr(), bufs['act'].data_ptr(), env._stream())
    assert rc == 0, rc

  def candidates_route(iterations=I):
    mean = bufs['mean'].copy_(mean0)
    for j in range(iterations):
      torch.clamp(mean, -1, 1, out=bufs['m'])
      candidates(mean, j)
      reweight(mean)

  def branches():
    env.rollout_branches(bufs['act'], out={'ret': bufs['ret']})

  return env, bufs, out_p, mean0, {'p_plan_mppi': plan_mppi, 'u_torch_route': torch_route, 'c_candidates_route': candidates_route, 'b_branches': branches}, candidates


def probe(torch, nobj, reps, inner):
  env, bufs, out_p, mean0, legs, candidates = setup(torch, nobj)
  plan_mppi, torch_route, candidates_route = legs['p_plan_mppi'], legs['u_torch_route'], legs['c_candidates_route']
  before = {k: getattr(env, k).clone() for k in ('qpos', 'attached', 'goal_idx', 'steps_since_reset')}
  plan_mppi(1)
  candidates_route(1)
  diff1 = float((bufs['mean'] - out_p['plan']).abs().max())
  plan_mppi()
  candidates_route()
  torch.cuda.synchronize()
  assert all(torch.equal(getattr(env, k), v) for k, v in before.items()), 'the env moved'
  per_env = (bufs['mean'] - out_p['plan']).abs().amax((0, 2))
  diff, apart = float(per_env.max()), int((per_env > 1e-5).sum())
  moved = float((out_p['plan'] - mean0.clamp(-1, 1)).abs().max())
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  torch_route()
  torch.cuda.synchronize()
  peak_u = torch.cuda.max_memory_allocated() - base + sum(bufs[k].numel() * bufs[k].element_size() for k in ('act', 'eps', 'ret', 'm'))
  torch.cuda.reset_peak_memory_stats()
  plan_mppi()
  torch.cuda.synchronize()
  peak_p = torch.cuda.max_memory_allocated() - base + out_p['ret'].numel() * 8
  candidates(mean0, 0)                                    # (b) scores iteration 0's candidates
  ms = interleaved(torch, legs, reps, inner, lambda: None)
  res = {k: summary(v) for k, v in ms.items()}
  p, u = res['p_plan_mppi'], res['u_torch_route']
  return {'obs_dim': env.OBS_DIM, 'legs': res, 'u_over_p': round(u['ms_median'] / p['ms_median'], 2),
          'c_over_p': round(res['c_candidates_route']['ms_median'] / p['ms_median'], 2),
          'p_per_iteration_ms': round(p['ms_median'] / I, 4), 'p_over_I_branch_launches': round(p['ms_median'] / (I * res['b_branches']['ms_median']), 2),
          'plan_c_vs_plan_p_max_abs_difference': {'after_one_iteration': diff1, 'after_all_iterations': diff, 'envs_beyond_1e-5_after_all_iterations': apart,
                                                  'note': 'one iteration differs by the rounding of the float32 softmax and sum; over further iterations an env whose '
                                                          'candidate sits at a success threshold scores the two slightly different plans differently (sparse reward)'},
          'plan_p_vs_clipped_mean_max_abs_difference': moved,
          'memory_bytes': {'u_peak_beyond_its_inputs': int(peak_u), 'p_peak_beyond_its_inputs': int(peak_p), 'p_workspace_ret_K_N_float64': K * N * 8,
                           'candidates_K_H_N_3_float32': K * H * N * 12},
          'bar': {'statement': 'p_plan_mppi median < u_torch_route median by more than the two spreads together',
                  'difference_ms': round(u['ms_median'] - p['ms_median'], 4), 'spreads_together_ms': round(u['spread_ms'] + p['spread_ms'], 4),
                  'met': bool(u['ms_median'] - p['ms_median'] > u['spread_ms'] + p['spread_ms'])}}


def trace_only(torch):
  """the launches a kernel trace should see, and nothing around them worth timing"""
  for nobj in (1, 3):
    _, _, _, mean0, legs, candidates = setup(torch, nobj)
    candidates(mean0, 0)
    for _ in range(20):
      legs['p_plan_mppi']()
    for _ in range(80):
      legs['b_branches']()
    torch.cuda.synchronize()


def kernel_times(path):
  """{short kernel name: dict(calls, average_us, min_us, max_us)} of the planner's and the branch launch's kernels from a rocprofv3 kernel_stats.csv"""
  out = {}
  for row in csv.DictReader(open(path)):
    m = re.search(r'\b((?:plan_score|plan_update|plan_candidates|branch)_kernel(?:<[^>]*>)?)', row['Name'])
    if m:
      out[m.group(1)] = {'calls': int(row['Calls']), 'average_us': round(float(row['AverageNs']) / 1e3, 3), 'min_us': round(float(row['MinNs']) / 1e3, 3),
                         'max_us': round(float(row['MaxNs']) / 1e3, 3)}
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=5)
  ap.add_argument('--trace-only', action='store_true')
  ap.add_argument('--kernel-stats')
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop_plan_probe.py measures on the GPU: no HIP device visible')
  if args.trace_only:
    trace_only(torch)
    return 0
  out = {'what': 'tools/tabletop_plan_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'K': K, 'H': H, 'iterations': I, 'sigma': SIGMA, 'temperature': TEMPERATURE, 'reward': 'sparse', 'reps': args.reps, 'inner': args.inner, 'warmup': 2,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count),
         'one_object': probe(torch, 1, args.reps, args.inner), 'three_objects': probe(torch, 3, args.reps, args.inner)}
  if args.kernel_stats:
    kt = kernel_times(args.kernel_stats)
    out['kernel_trace'] = {'source': 'rocprofv3 --kernel-trace --stats over --trace-only, a run of its own', 'kernels': kt}
    for tag, nobj in (('one_object', 1), ('three_objects', 3)):
      s, b, upd = (kt.get(f'{k}<{nobj}, false>' if k != 'plan_update_kernel' else k) for k in ('plan_score_kernel', 'branch_kernel', 'plan_update_kernel'))
      if s and b:
        out[tag]['s_score_kernel_us'], out[tag]['b_branch_kernel_us'] = s['average_us'], b['average_us']
        out[tag]['s_over_b'] = round(s['average_us'] / b['average_us'], 3)
    out['kernel_trace']['note'] = 'plan_update_kernel serves both envs: its figure is the average over the two'
  else:
    out['kernel_trace'] = 'not measured in this run'
  out['bar_met'] = bool(out['one_object']['bar']['met'] and out['three_objects']['bar']['met'])
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

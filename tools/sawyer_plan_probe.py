"""What the Sawyer MPPI planning step (earl_sawyer_plan_mppi, env.plan_mppi) costs next to the route it replaces and next to the branch launch inside it.  Door and peg,
sparse reward, H = 20, one iteration, the branch probe's three shapes (N envs, K candidates): (16, 256), (64, 64), (1024, 8).  Three legs:
  (a) plan_mppi      env.plan_mppi(mean, K=, iterations=1, out=): the candidates kernel, the branch launch, the update kernel
  (b) torch_route    the route on public methods: torch.randn noise + clamp -> env.rollout_branches -> softmax of the returns and the weighted mean in torch
  (c) branches       env.rollout_branches(actions [K, H, N, 4]) alone: what (a) and (b) both contain
Device events around each run after one warm-up round, the legs taking turns inside each of --reps repetitions; no leg moves the env, so every run starts from the
same state; per leg the median, min, max, spread = max - min.  Reported per shape: (b) / (a), and (a) - (c), the planner's own cost (recorded, not asserted: nobody
has measured it before).  UNFAVOURABLE where (a) is not below (b) by more than the two spreads together.  (a) and (b) draw different noise (Philox against torch's
generator), so they are not compared; tests/test_sawyer_plan_gpu.py holds (a) to its oracle bit for bit.
A steering record on top: the door under the DENSE reward, (N, K) = (16, 256), four iterations in one call, ret0 (the return of the plan entering each iteration)
averaged over the envs.  Recorded, not asserted: contact dynamics promise no monotone improvement.

  python tools/sawyer_plan_probe.py [--reps 5] [--envs door,peg] [--out profiles/sawyer_plan_probe.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sawyer_branch_probe import H, SHAPES, summary      # noqa: E402  (the branch probe's shapes and figures)
from sawyer_policy_probe import interleaved, make      # noqa: E402  (the Sawyer probes share their method)

SIGMA, TEMPERATURE = 0.3, 1.0


def probe(torch, kind, n, K, reps):
  env = make(kind, n)
  gen = torch.Generator(device='cuda').manual_seed(7)
  env.rollout((torch.rand(5, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous())        # off the reset state
  mean = ((torch.rand(H, n, 4, device='cuda', generator=gen) * 2 - 1) * 0.5).contiguous()
  acts = (torch.rand(K, H, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous()
  out = {'plan': torch.empty(H, n, 4, device='cuda'), 'ret': torch.empty(K, n, dtype=torch.float64, device='cuda'), 'ret0': torch.empty(1, n, dtype=torch.float64, device='cuda'),
         'best_ret': torch.empty(n, dtype=torch.float64, device='cuda'), 'best_k': torch.empty(n, dtype=torch.int32, device='cuda'),
         'fail': torch.empty(K, n, dtype=torch.int32, device='cuda')}
  got = {}

  def plan_mppi():
    env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=out)

  def torch_route():
    m = mean.clamp(-1, 1)
    act = (m[None] + SIGMA * torch.randn(K, H, n, 4, device='cuda', generator=gen)).clamp_(-1, 1)
    act[0] = m
    br = env.rollout_branches(act)
    w = torch.softmax(br['ret'] / TEMPERATURE, 0)
    got['plan'] = (m + (w[:, None, :, None] * (act - m[None])).sum(0).to(torch.float32)).clamp_(-1, 1)

  def branches():
    got.update(env.rollout_branches(acts))

  legs = {'a_plan_mppi': plan_mppi, 'b_torch_route': torch_route, 'c_branches': branches}
  ms = interleaved(torch, legs, reps, lambda: None, warmup=1)
  res = {k: summary(v, n * K * H) for k, v in ms.items()}
  a, b, c = (res[k] for k in legs)
  faster_than_b = b['ms_median'] - a['ms_median'] > a['spread_ms'] + b['spread_ms']
  return {'n': n, 'K': K, 'H': H, 'iterations': 1, 'virtual_envs': n * K, 'candidate_bytes': K * H * n * 16,
          'share_of_branches_with_a_rolled_back_step': round(float((out['fail'] != 0).float().mean()), 5), 'legs': res,
          'b_over_a': round(b['ms_median'] / a['ms_median'], 3), 'a_minus_c_ms': round(a['ms_median'] - c['ms_median'], 3),
          'a_minus_c_within_spreads': bool(abs(a['ms_median'] - c['ms_median']) <= a['spread_ms'] + c['spread_ms']),
          'a_faster_than_b_beyond_spreads': bool(faster_than_b), 'verdict': ['favourable'] if faster_than_b else ['UNFAVOURABLE: (a) is not faster than (b) beyond the spreads']}


def steering(torch, n=16, K=256, iterations=4):
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  env = SawyerDoor(num_envs=n, scalar_api=False, info='minimal', reward_type='dense')
  res = env.plan_mppi(horizon=H, K=K, iterations=iterations, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3)
  torch.cuda.synchronize()
  return {'env': 'door', 'reward': 'dense', 'n': n, 'K': K, 'H': H, 'iterations': iterations, 'sigma': SIGMA, 'temperature': TEMPERATURE, 'mean': 'zeros, from the reset state',
          'ret0_mean_over_envs': [round(float(v), 6) for v in res['ret0'].mean(1)], 'best_ret_mean_over_envs': round(float(res['best_ret'].mean()), 6),
          'rolled_back_steps': int(res['fail'].sum()), 'asserted': False}


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/sawyer_plan_probe.py measures on the GPU: no HIP device visible')
  res = {'what': 'tools/sawyer_plan_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'boxes': 1, 'build': eb.__version__,
         'reward': 'sparse', 'H': H, 'iterations': 1, 'sigma': SIGMA, 'temperature': TEMPERATURE, 'reps': args.reps, 'warmup': 1,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count),
         'timing': 'device events around one run, legs interleaved over the repetitions, every run from the same env state (no leg moves the env); spread = max - min'}
  for kind in args.envs.split(','):
    res[kind] = {}
    for n, K in SHAPES:
      res[kind][f'N{n}_K{K}'] = probe(torch, kind, n, K, args.reps)
      print(f'{kind} N={n} K={K}: done', file=sys.stderr, flush=True)
      torch.cuda.empty_cache()
  res['steering_record'] = steering(torch)
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

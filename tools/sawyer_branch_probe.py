"""What the Sawyer branch launch (earl_sawyer_branch_rollout, env.rollout_branches) costs next to the route it replaces and next to its floor.  Door and peg, sparse
reward, H = 20, three shapes (N envs, K plans): (16, 256), (64, 64), (1024, 8).  Three legs over the same stepper work:
  (a) branches      env.rollout_branches(actions [K, H, N, 4]): one launch over K N virtual envs (plus the replicate kernel in front), five [K, N] results
  (b) round_trips   the route on public methods: K x (load_state_dict, rollout(actions[k], out=), the three reductions in torch)
  (c) floor         ONE plain rollout of K N independent envs for H steps (an env of K N instances holding K copies of the N states): the same stepper work
                    with every [H] output written
Before any timing (a) is compared with (b) bit for bit (ret, success, first_success; sparse rewards are 0 / 1, so torch's sum has one value in any order).
Device events around each run after one warm-up round, the legs taking turns inside each of --reps repetitions, every run from the same env state; per leg the
median, min, max, spread = max - min.  Per shape the JSON says UNFAVOURABLE where (a) is not faster than (b) by more than the two spreads together, or slower than
(c) by more than the two spreads together.  Nothing is promised: the numbers are what they are.

  python tools/sawyer_branch_probe.py [--reps 5] [--envs door,peg] [--out profiles/sawyer_branch_probe.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sawyer_policy_probe import interleaved, make      # noqa: E402  (the Sawyer probes share their method)

H = 20
SHAPES = ((16, 256), (64, 64), (1024, 8))


def summary(ms, env_steps):
  med = statistics.median(ms)
  return {'ms_median': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'spread_ms': round(max(ms) - min(ms), 3),
          'env_steps_per_s': round(env_steps / (med * 1e-3)), 'ms_all': [round(x, 3) for x in ms]}


def probe(torch, kind, n, K, reps):
  env, big = make(kind, n), make(kind, K * n)
  gen = torch.Generator(device='cuda').manual_seed(7)
  acts = (torch.rand(K, H, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous()
  env.rollout((torch.rand(5, n, 4, device='cuda', generator=gen) * 2 - 1).contiguous())        # off the reset state
  snap = env.state_dict()
  # the floor's env: virtual env k n + i is env i, its actions the branch's
  big.load_state_dict({k: (v.repeat(K, *([1] * (v.dim() - 1))) if torch.is_tensor(v) else v) for k, v in snap.items()})
  big_snap = big.state_dict()
  big_acts = acts.permute(1, 0, 2, 3).reshape(H, K * n, 4).contiguous()
  out, big_out = env._new_out((H,)), big._new_out((H,))
  u = {'ret': torch.empty(K, n, dtype=torch.float64, device='cuda'), 'success': torch.empty(K, n, dtype=torch.bool, device='cuda'),
       'first_success': torch.empty(K, n, dtype=torch.int32, device='cuda')}
  steps_t = torch.arange(H, device='cuda', dtype=torch.int32)[:, None]
  got = {}

  def branches():
    got.update(env.rollout_branches(acts))

  def round_trips():
    for k in range(K):
      env.load_state_dict(snap)
      o = env.rollout(acts[k], out=out)
      torch.sum(o['reward'], 0, dtype=torch.float64, out=u['ret'][k])
      u['success'][k].copy_(o['success'][-1])
      u['first_success'][k].copy_(torch.where(o['success'], steps_t, H).amin(0))

  def floor():
    big.rollout(big_acts, out=big_out)

  def restore():
    env.load_state_dict(snap)
    big.load_state_dict(big_snap)

  restore()
  branches()
  round_trips()
  torch.cuda.synchronize()
  u['first_success'][u['first_success'] == H] = -1
  for k in u:
    assert torch.equal(got[k].view(torch.uint8), u[k].view(torch.uint8)), f'{kind} N={n} K={K}: {k} of the branch launch differs from the round trips'
  guard = float((got['fail'] != 0).float().mean())
  legs = {'a_branches': branches, 'b_round_trips': round_trips, 'c_floor': floor}
  ms = interleaved(torch, legs, reps, restore, warmup=1)
  res = {k: summary(v, n * K * H) for k, v in ms.items()}
  a, b, c = (res[k] for k in legs)
  faster_than_b = b['ms_median'] - a['ms_median'] > a['spread_ms'] + b['spread_ms']
  slower_than_c = a['ms_median'] - c['ms_median'] > a['spread_ms'] + c['spread_ms']
  verdict = []
  if not faster_than_b:
    verdict.append('UNFAVOURABLE: (a) is not faster than (b) beyond the spreads')
  if slower_than_c:
    verdict.append('UNFAVOURABLE: (a) is slower than (c) beyond the spreads')
  return {'n': n, 'K': K, 'H': H, 'virtual_envs': n * K, 'outputs_bit_identical_to_round_trips': True, 'share_of_branches_with_a_rolled_back_step': round(guard, 5),
          'share_of_successful_branches': round(float(got['success'].float().mean()), 5), 'legs': res,
          'b_over_a': round(b['ms_median'] / a['ms_median'], 2), 'a_over_c': round(a['ms_median'] / c['ms_median'], 3),
          'a_faster_than_b_beyond_spreads': bool(faster_than_b), 'a_slower_than_c_beyond_spreads': bool(slower_than_c), 'verdict': verdict or ['favourable']}


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/sawyer_branch_probe.py measures on the GPU: no HIP device visible')
  res = {'what': 'tools/sawyer_branch_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'boxes': 1, 'build': eb.__version__,
         'reward': 'sparse', 'H': H, 'reps': args.reps, 'warmup': 1, 'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count),
         'timing': 'device events around one run, legs interleaved over the repetitions, every run from the same env state; spread = max - min'}
  for kind in args.envs.split(','):
    res[kind] = {}
    for n, K in SHAPES:
      res[kind][f'N{n}_K{K}'] = probe(torch, kind, n, K, args.reps)
      print(f'{kind} N={n} K={K}: done', file=sys.stderr, flush=True)
      torch.cuda.empty_cache()
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

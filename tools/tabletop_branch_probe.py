"""What the branch launch (earl_tabletop_branch_rollout / earl_tabletop3_branch_rollout, env.rollout_branches) buys a shooting planner over the route it had before.
N = 4096 envs, K = 64 candidate plans of H = 32 steps, sparse reward, both tabletop envs, everything into preallocated tensors:
  (b) branches      env.rollout_branches(a, out=...): one launch, one lane per (branch, env), nothing stored inside the loop, the state untouched
  (u) round_trips   K x (the state tensors copied back from a snapshot, env.rollout(a[k], out=...), the three reductions in torch): the API before this launch
  (z) stride_zero   the launch of (b) with act_branch_stride = 0 (every branch reads ONE [H, N, 3] block, 1.6 MB: cache-resident) -- what the action traffic costs
and, at K = 1:
  (b1) the branch launch with one branch   (r1) the open-loop env.rollout(a[0], out=...) of the same H
Device events around `--inner` back-to-back runs after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions; per leg the median, min and max of
the milliseconds per run, spread = max - min.  Before any timing (b) is compared with (u) bit for bit.
PASS CONDITION: (b) takes less time than (u) by more than the two spreads together.  Also recorded: TB/s on the algorithmic 12 bytes per env-step (the actions; the
state is read once and the four result words are stored once per branch) against 8 TB/s, and b1 / r1.  The [K, H, N, 3] actions are 101 MB, less than the 256 MiB
Infinity Cache: a launch repeated back to back may find part of them on the die, which the JSON says next to the figure.
Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/tabletop_branch_probe.py [--reps 5] [--inner 10] [--out profiles/tabletop_branch_probe.json]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from tabletop3_policy_probe import interleaved      # noqa: E402 (the tabletop probes share their method)

N, K, H = 4096, 64, 32
BYTES_PER_ENV_STEP = 12                              # the three float32 of the action; nothing is stored inside the loop
HBM_PEAK = 8e12
STATE = ('qpos', 'attached', 'goal_idx', 'steps_since_reset', 'interventions', 'steps_since_goal_change', 'lifelong_return_t')


def summary(ms, env_steps):
  med = statistics.median(ms)
  rate = env_steps / (med * 1e-3)
  return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'spread_ms': round(max(ms) - min(ms), 4),
          'env_steps_per_s': round(rate), 'algorithmic_TB_per_s': round(rate * BYTES_PER_ENV_STEP / 1e12, 4),
          'share_of_8_TB_per_s': round(rate * BYTES_PER_ENV_STEP / HBM_PEAK, 4), 'ms_all': [round(x, 4) for x in ms]}


def probe(torch, nobj, reps, inner):
  from earl_benchmark_amd import _abi
  if nobj == 1:
    from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  else:
    from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device='cuda', seed=1, reset_at_goal=True)    # (near the goal: both values of success occur)
  env._cfg.horizon = 10 * H
  gen = torch.Generator(device='cuda').manual_seed(7)
  a = (torch.rand(K, H, N, 3, device='cuda', generator=gen) * 2 - 1).contiguous()
  env.rollout((torch.rand(5, N, 3, device='cuda', generator=gen) * 2 - 1).contiguous())        # off the reset state
  snap, counter, steps = {k: getattr(env, k).clone() for k in STATE}, int(env._cfg.counter), env.total_step_count

  def restore():
    for k, v in snap.items():
      getattr(env, k).copy_(v)
    env._cfg.counter, env.total_step_count = counter, steps

  def blank():
    return {'ret': torch.empty(K, N, dtype=torch.float64, device='cuda'), 'success': torch.empty(K, N, dtype=torch.bool, device='cuda'),
            'first_success': torch.empty(K, N, dtype=torch.int32, device='cuda'), 'last_obs': torch.empty(K, N, env.OBS_DIM, device='cuda')}

  got = {k: blank() for k in 'buz'}
  one = {k: v[:1].clone() for k, v in blank().items()}
  outs = env._new_out((H, N))[0]
  steps_t = torch.arange(H, device='cuda', dtype=torch.int32)[:, None]

  def branches():
    env.rollout_branches(a, out=got['b'])

  def round_trips():
    for k in range(K):
      restore()
      obs, rew, done, succ = env.rollout(a[k], out=outs)
      g = got['u']
      torch.sum(rew, 0, dtype=torch.float64, out=g['ret'][k])
      g['success'][k].copy_(succ[-1])
      g['first_success'][k].copy_(torch.where(succ, steps_t, H).amin(0))
      g['last_obs'][k].copy_(obs[-1])

  lib, fn = _abi.load(), 'earl_tabletop_branch_rollout' if nobj == 1 else 'earl_tabletop3_branch_rollout'

  def stride_zero():
    g = got['z']
    sm = _abi.EpisodeSummary(ret=g['ret'].data_ptr(), success_last=g['success'].data_ptr(), first_success=g['first_success'].data_ptr())
    rc = getattr(lib, fn)(C.byref(env._cfg), C.byref(env._st), K, H, a.data_ptr(), 0, C.byref(sm), g['last_obs'].data_ptr(), env._stream())
    assert rc == 0, rc

  def branches_k1():
    env.rollout_branches(a[:1], out=one)

  def rollout_k1():
    env.rollout(a[0], out=outs)

  restore()
  branches()
  round_trips()
  restore()
  torch.cuda.synchronize()
  u = got['u']
  u['first_success'][u['first_success'] == H] = -1
  for k in got['b']:
    assert torch.equal(got['b'][k].view(torch.uint8), u[k].view(torch.uint8)), f'{k}: the branch launch differs from the round trips'
  spread_of_success = float(got['b']['success'].float().mean())

  legs = {'b_branches': branches, 'u_round_trips': round_trips, 'z_stride_zero': stride_zero, 'b1_branches_k1': branches_k1, 'r1_rollout': rollout_k1}
  ms = interleaved(torch, legs, reps, inner, restore)
  work = {'b_branches': N * K * H, 'u_round_trips': N * K * H, 'z_stride_zero': N * K * H, 'b1_branches_k1': N * H, 'r1_rollout': N * H}
  res = {k: summary(v, work[k]) for k, v in ms.items()}
  b, uu, z, b1, r1 = (res[k] for k in legs)
  return {'obs_dim': env.OBS_DIM, 'outputs_bit_identical': True, 'share_of_successful_branches': round(spread_of_success, 4), 'legs': res,
          'b_over_u': round(b['ms_median'] / uu['ms_median'], 4), 'u_over_b': round(uu['ms_median'] / b['ms_median'], 2),
          'z_over_b': round(z['ms_median'] / b['ms_median'], 4), 'b1_over_r1': round(b1['ms_median'] / r1['ms_median'], 4),
          'pass_condition': {'statement': 'b_branches median < u_round_trips median by more than the two spreads together',
                             'difference_ms': round(uu['ms_median'] - b['ms_median'], 4), 'spreads_together_ms': round(uu['spread_ms'] + b['spread_ms'], 4),
                             'met': bool(uu['ms_median'] - b['ms_median'] > uu['spread_ms'] + b['spread_ms'])}}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=10)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop_branch_probe.py measures on the GPU: no HIP device visible')
  out = {'what': 'tools/tabletop_branch_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'K': K, 'H': H, 'reward': 'sparse', 'reps': args.reps, 'inner': args.inner, 'warmup': 2,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count),
         'action_bytes': N * K * H * BYTES_PER_ENV_STEP,
         'note': 'the actions (101 MB) fit the 256 MiB Infinity Cache: repeated launches may read part of them on the die, so algorithmic_TB_per_s is a rate of '
                 'the launch, not of HBM; z_stride_zero reads one 1.6 MB block for all branches',
         'one_object': probe(torch, 1, args.reps, args.inner), 'three_objects': probe(torch, 3, args.reps, args.inner)}
  out['pass_condition_met'] = bool(out['one_object']['pass_condition']['met'] and out['three_objects']['pass_condition']['met'])
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0 if out['pass_condition_met'] else 1


if __name__ == '__main__':
  sys.exit(main())

"""What the one-launch evaluation of the THREE-object tabletop (earl_tabletop3_eval_episodes, env.rollout_episodes) buys over what a user had before it.
N = 4096, T = 200, E = 28 episodes, every episode its own actions, sparse reward, outputs into preallocated tensors:
  (u) per_episode   28 x env.rollout(a[e], reset_first=True, out=...): a reset launch and a plain one-lane-per-env rollout launch per episode
  (f) fused         env.rollout_episodes(a, out=...): the role-split launch, groups of episodes in flight
  (s) fused_serial  the same launch in form 2 (earl_debug_set_rollout3_form): all episodes on one group of workgroups
Device events around each run after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions; per leg the median, min and max of the
milliseconds, spread = max - min.  Before any timing the three legs' outputs are compared bit for bit.
PASS CONDITION: (f) takes less time than (u) by more than the two spreads together.  Also recorded: f / u, f / s, env-steps/s, and GB/s on the algorithmic
98 bytes per env-step (12 read, 86 written) against 8 TB/s.  Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/tabletop3_eval_probe.py [--reps 5] [--out profiles/tabletop3_eval_probe.json]
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

from tabletop3_policy_probe import interleaved      # noqa: E402 (the three-object probes share their method)

N, T, E = 4096, 200, 28
BYTES_PER_ENV_STEP = 98                              # 12 of actions read; 80 of observation, 4 of reward, 2 flag bytes written
HBM_PEAK = 8e12


def summary(ms):
  med = statistics.median(ms)
  rate = N * T * E / (med * 1e-3)
  return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'spread_ms': round(max(ms) - min(ms), 4),
          'env_steps_per_s': round(rate), 'algorithmic_GB_per_s': round(rate * BYTES_PER_ENV_STEP / 1e9, 1),
          'share_of_8_TB_per_s': round(rate * BYTES_PER_ENV_STEP / HBM_PEAK, 3), 'ms_all': [round(x, 4) for x in ms]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  from earl_benchmark_amd import _abi
  from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop3_eval_probe.py measures on the GPU: no HIP device visible')
  lib = _abi.load()
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device='cuda', seed=1)
  env._cfg.horizon = T
  a = (torch.rand(E, T, N, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(7)) * 2 - 1).contiguous()
  counter = int(env._cfg.counter)
  outs = {k: tuple(torch.empty_like(t) for t in env._new_out((E, T, N))[0]) for k in 'ufs'}

  def restore():
    env._cfg.counter = counter                       # (every leg starts with a reset: the state needs no restoring)

  def per_episode():
    for e in range(E):
      env.rollout(a[e], reset_first=True, out=tuple(t[e] for t in outs['u']))

  def fused():
    env.rollout_episodes(a, out=outs['f'])

  def fused_serial():
    prev = lib.earl_debug_set_rollout3_form(2)
    try:
      env.rollout_episodes(a, out=outs['s'])
    finally:
      lib.earl_debug_set_rollout3_form(prev)

  legs = {'u_per_episode': per_episode, 'f_fused': fused, 's_fused_serial': fused_serial}
  state = {}
  for name, fn in legs.items():                      # the legs compute the same thing, bit for bit
    restore()
    fn()
    torch.cuda.synchronize()
    state[name] = [getattr(env, k).clone() for k in ('qpos', 'attached', 'goal_idx', 'steps_since_reset')]
  for k in 'fs':
    for x, y in zip(outs['u'], outs[k]):
      assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f'leg {k} differs from the per-episode launches'
  for name in ('f_fused', 's_fused_serial'):
    assert all(torch.equal(x, y) for x, y in zip(state['u_per_episode'], state[name])), f'{name}: the state left behind differs'

  ms = interleaved(torch, legs, args.reps, 1, restore)
  res = {k: summary(v) for k, v in ms.items()}
  u, f, s = res['u_per_episode'], res['f_fused'], res['s_fused_serial']
  out = {'what': 'tools/tabletop3_eval_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'T': T, 'episodes': E, 'reward': 'sparse', 'actions': 'own per episode', 'reps': args.reps, 'warmup': 2,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count), 'outputs_bit_identical': True, 'legs': res,
         'f_over_u': round(f['ms_median'] / u['ms_median'], 4), 'u_over_f': round(u['ms_median'] / f['ms_median'], 2),
         'f_over_s': round(f['ms_median'] / s['ms_median'], 4), 's_over_f': round(s['ms_median'] / f['ms_median'], 2),
         'pass_condition': {'statement': 'f_fused median < u_per_episode median by more than the two spreads together',
                            'difference_ms': round(u['ms_median'] - f['ms_median'], 4), 'spreads_together_ms': round(u['spread_ms'] + f['spread_ms'], 4),
                            'met': bool(u['ms_median'] - f['ms_median'] > u['spread_ms'] + f['spread_ms'])}}
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0 if out['pass_condition']['met'] else 1


if __name__ == '__main__':
  sys.exit(main())

"""What the terminal value inside the planner's kernels (earl_tabletop[3]_plan_mppi_value / _mpc_rollout_value; env.plan_mppi(discount=, value=),
env.rollout_mpc(discount=, value=)) costs, and what it buys over the route it replaces.  N = 4096 envs, K = 64 candidates, H = 8 and 32, one iteration, sparse
reward, both tabletop envs, everything into preallocated tensors.  Value networks: D -> 256 -> 1, D -> 64 -> 1, D -> 16 -> 64 -> 1 and
D -> EARL_PLAN_VALUE_MAX_H1 -> 256 -> 1 (D -> 64 -> 64 -> 1 is refused: a first hidden layer of two is at most EARL_PLAN_VALUE_MAX_H1 = 16 wide).
  (v) value    env.plan_mppi(mean, discount=0.99, value=V, out=...): two launches, V evaluated by every lane of the score kernel on its own last observation
  (p) plain    env.plan_mppi(mean, out=...) as it stands, the existing entry point: v - p is what the discount and the terminal term cost
  (u) unfused  the route (v) replaces, at discount 1 where it can be expressed: env.plan_candidates -> env.rollout_branches(last_obs=True) -> V(last_obs) in torch
               on [K N, D] -> ret + V -> softmax over K -> the weighted sum of the candidates, clipped.  Float32 / float64 torch arithmetic: close to (v) at
               discount 1, not bit-equal (the maximum difference of the plans is recorded)
  (f) loop     env.rollout_mpc(T = 50) with (fv) and without (fp) the value network
Device events around `--inner` back-to-back runs after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions, the env restored before each
timing; per leg the median, min and max of the milliseconds per run, spread = max - min.  No speed bar is fixed in advance: every ratio is a finding.  One run on
one box.  Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/tabletop_value_probe.py [--reps 5] [--inner 2] [--out profiles/tabletop_value_probe.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from tabletop3_policy_probe import interleaved, restorer      # noqa: E402 (the tabletop probes share their method)
from tabletop_mpc_probe import summary                        # noqa: E402

N, K, T = 4096, 64, 50
HORIZONS = (8, 32)
DEV = 'cuda'
SIGMA, TEMPERATURE, GAMMA = 0.3, 1.0, 0.99


def nets(D, max_h1):
  return {f'{D}-256-1': (256,), f'{D}-64-1': (64,), f'{D}-16-64-1': (16, 64), f'{D}-{max_h1}-256-1': (max_h1, 256)}


def value_net(torch, D, hidden, seed):
  from earl_benchmark_amd.policy import MLPPolicy
  gen = torch.Generator().manual_seed(seed)
  dims = [D, *hidden, 1]
  layers = [((torch.rand(n, k, generator=gen) * 2 - 1) / k ** 0.5, (torch.rand(n, generator=gen) * 2 - 1) * 0.1) for k, n in zip(dims[:-1], dims[1:])]
  return MLPPolicy(layers, 'tanh', 'none', device=DEV, obs_dim=D, act_dim=1)


def probe(torch, nobj, H, reps, inner, max_h1):
  if nobj == 1:
    from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  else:
    from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device=DEV, seed=1, reset_at_goal=True)
  env._cfg.horizon = 10 * (H + T)
  gen = torch.Generator(device=DEV).manual_seed(7)
  env.rollout((torch.rand(5, N, 3, device=DEV, generator=gen) * 2 - 1).contiguous())        # off the reset state
  kw = dict(device=DEV)
  mean = ((torch.rand(H, N, 3, generator=gen, **kw) * 2 - 1) * 0.5).contiguous()
  D = env.OBS_DIM
  args = dict(K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=11)
  plan_out = lambda: {'plan': torch.zeros(H, N, 3, **kw), 'ret': torch.zeros(K, N, dtype=torch.float64, **kw)}
  restore_env = restorer(env)
  out_p = plan_out()
  branch_out = {'ret': torch.zeros(K, N, dtype=torch.float64, **kw), 'last_obs': torch.zeros(K, N, D, **kw)}

  def loop_out():
    return {'obs': torch.zeros(T, N, D, **kw), 'reward': torch.zeros(T, N, **kw), 'done': torch.zeros(T, N, dtype=torch.bool, **kw),
            'success': torch.zeros(T, N, dtype=torch.bool, **kw), 'actions': torch.zeros(T, N, 3, **kw), 'plan': mean.clone()}

  legs = {'p_plain': lambda: env.plan_mppi(mean, out=out_p, **args)}
  loops = {'fp_loop_plain': loop_out()}
  legs['fp_loop_plain'] = lambda: env.rollout_mpc(T, loops['fp_loop_plain']['plan'], out=loops['fp_loop_plain'], **args)
  checks = {}
  for name, hidden in nets(D, max_h1).items():
    V = value_net(torch, D, hidden, seed=len(name))
    out_v, out_u = plan_out(), torch.zeros(H, N, 3, **kw)

    def fused(V=V, out_v=out_v):
      env.plan_mppi(mean, discount=GAMMA, value=V, out=out_v, **args)

    def unfused(V=V, out_u=out_u):
      cand = env.plan_candidates(mean, K, sigma=SIGMA, iteration=0, noise_counter=11)           # [K, H, N, 3]
      env.rollout_branches(cand, out=branch_out)
      ret = branch_out['ret'] + V(branch_out['last_obs'].reshape(K * N, D)).reshape(K, N).double()
      w = torch.softmax((ret - ret.max(0).values) / TEMPERATURE, 0).float()
      out_u.copy_((w[:, None, :, None] * cand).sum(0).clamp_(-1, 1))

    legs['v_value ' + name], legs['u_unfused ' + name] = fused, unfused
    if hidden in ((256,), (max_h1, 256)):
      loops[name] = loop_out()
      legs['fv_loop_value ' + name] = lambda V=V, o=loops[name]: env.rollout_mpc(T, o['plan'], discount=GAMMA, value=V, out=o, **args)
    one = env.plan_mppi(mean, discount=1.0, value=V, **args)                                     # (u) states discount 1: how close is it?
    unfused()
    checks[name] = {'max_abs_plan_difference_u_vs_value_at_discount_1': float((out_u - one['plan']).abs().max())}

  def restore():
    restore_env()
    for o in loops.values():
      o['plan'].copy_(mean)

  ms = interleaved(torch, legs, reps, inner, restore)
  res = {k: summary(v) for k, v in ms.items()}
  p = res['p_plain']
  for name in nets(D, max_h1):
    v, u = res['v_value ' + name], res['u_unfused ' + name]
    checks[name].update(v_minus_p_ms=round(v['ms_median'] - p['ms_median'], 4), v_over_p=round(v['ms_median'] / p['ms_median'], 3),
                        u_over_v=round(u['ms_median'] / v['ms_median'], 3),
                        v_minus_u_beyond_the_spreads=bool(abs(v['ms_median'] - u['ms_median']) > v['spread_ms'] + u['spread_ms']))
    if 'fv_loop_value ' + name in res:
      checks[name]['fv_over_fp'] = round(res['fv_loop_value ' + name]['ms_median'] / res['fp_loop_plain']['ms_median'], 3)
  return {'obs_dim': D, 'H': H, 'legs': res, 'per_network': checks}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=2)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  from earl_benchmark_amd import _abi
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop_value_probe.py measures on the GPU: no HIP device visible')
  out = {'what': 'tools/tabletop_value_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'K': K, 'T_of_the_loop': T, 'iterations': 1, 'sigma': SIGMA, 'temperature': TEMPERATURE, 'discount': GAMMA, 'reward': 'sparse', 'reps': args.reps,
         'inner': args.inner, 'warmup': 2, 'plan_value_max_h1': _abi.PLAN_VALUE_MAX_H1, 'one_run_on_one_box': True,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count)}
  for tag, nobj in (('one_object', 1), ('three_objects', 3)):
    out[tag] = {f'H_{H}': probe(torch, nobj, H, args.reps, args.inner, _abi.PLAN_VALUE_MAX_H1) for H in HORIZONS}
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

"""What the fused closed-loop launch of the THREE-object tabletop (earl_tabletop3_policy_rollout, env.rollout_policy) buys over the closed loop the env had before it.
N = 4096, sparse reward, T = 200, the policies 20 -> 64 -> 3 and 20 -> 256 -> 256 -> 3, deterministic and sampled (a Gaussian head), over the same T env steps from the
same state:
  (a) graph_policy   env.make_step_graph(T, policy=pi): the captured per-step loop, the network as torch kernels between the steps (a Gaussian policy: at its mean).
                     If the capture fails for NOBJ = 3 the leg is T eager step() calls with pi(obs) instead, and the JSON says so ('graph_policy_form')
  (b) open_loop      env.rollout(actions) with the actions (c) produced: the env steps alone
  (c) fused          env.rollout_policy(pi, T, reset_first=False): ONE launch
and for context (d) single_object_fused: the single-object env's fused launch with a 12 -> 64 -> 3 policy at the same N.
Device events around --inner back-to-back runs of a leg after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions, every timing from the same env
state; per leg the median, min and max of the per-run milliseconds, spread = max - min.
PASS CONDITION: the deterministic 20 -> 64 -> 3 fused launch takes less time than the captured per-step loop it replaces by more than the two spreads together.
Every other ratio is reported, not gated.  Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/tabletop3_policy_probe.py [--reps 5] [--inner 10] [--out profiles/tabletop3_policy_probe.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T = 4096, 200
NETS = {'64': (64,), '256x256': (256, 256)}


def layers_of(obs_dim, hidden, out_dim, seed=3):
  """a small-gain random network: the envs move gently, grip and release"""
  import numpy as np
  rng = np.random.default_rng(seed)
  dims = [obs_dim] + list(hidden) + [out_dim]
  return [((rng.standard_normal((n, k)) * (0.5 if l == len(dims) - 2 else 1.0) / np.sqrt(k)).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32))
          for l, (k, n) in enumerate(zip(dims[:-1], dims[1:]))]


def interleaved(torch, legs, reps, inner, restore, warmup=2):
  """per-run device-event milliseconds of every leg (`inner` runs back to back per timing), the legs taking turns inside each repetition"""
  ms = {k: [] for k in legs}
  for i in range(warmup + reps):
    for name, fn in legs.items():
      restore()
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(inner):
        fn()
      e1.record()
      torch.cuda.synchronize()
      if i >= warmup:
        ms[name].append(e0.elapsed_time(e1) / inner)
  return ms


def restorer(env):
  """-> restore(): the env's state and Philox counter as they are now, copied back IN PLACE (a captured graph holds the tensors' addresses)"""
  names = ('qpos', 'attached', 'goal_idx', 'steps_since_reset', 'interventions')
  saved, counter = {k: getattr(env, k).clone() for k in names}, int(env._cfg.counter)

  def restore():
    for k, v in saved.items():
      getattr(env, k).copy_(v)
    env._cfg.counter = counter
  return restore


def summary(ms):
  med = statistics.median(ms)
  return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'spread_ms': round(max(ms) - min(ms), 4),
          'env_steps_per_s': round(N * T / (med * 1e-3)), 'ms_all': [round(x, 4) for x in ms]}


def probe(torch, net, sampled, reps, inner):
  from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device='cuda', seed=1)
  kw = dict(device='cuda', obs_dim=20, act_dim=3)
  pi = GaussianMLPPolicy(layers_of(20, NETS[net], 6), 'relu', **kw) if sampled else MLPPolicy(layers_of(20, NETS[net], 3), 'relu', 'tanh', **kw)
  env.reset()
  restore = restorer(env)
  actions = env.rollout_policy(pi, T, reset_first=False)[4].clone()
  restore()
  form = 'captured graph'
  try:
    graph = env.make_step_graph(T, policy=pi)
    graph_leg = graph.replay
  except Exception as e:                                                 # the capture is the measured baseline: say what stands in for it, never skip the leg silently
    form = f'T eager step() calls with pi(obs) (the capture failed: {type(e).__name__}: {str(e)[:120]})'

    def graph_leg():
      obs = env._get_obs()
      for _ in range(T):
        obs = env.step(pi(obs))[0]
  legs = {'graph_policy': graph_leg, 'open_loop': lambda: env.rollout(actions), 'fused': lambda: env.rollout_policy(pi, T, reset_first=False)}
  ms = interleaved(torch, legs, reps, inner, restore)
  res = {k: summary(v) for k, v in ms.items()}
  g, f, o = res['graph_policy'], res['fused'], res['open_loop']
  res.update(policy=f'20 -> {" -> ".join(map(str, NETS[net]))} -> {6 if sampled else 3}', head='sampled' if sampled else 'deterministic', graph_policy_form=form,
             graph_over_fused=round(g['ms_median'] / f['ms_median'], 2), fused_over_open_loop=round(f['ms_median'] / o['ms_median'], 2),
             policy_phase_us_per_step=round((f['ms_median'] - o['ms_median']) * 1e3 / T, 3))
  return res


def single_object(torch, reps, inner):
  from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  from earl_benchmark_amd.policy import MLPPolicy
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device='cuda', seed=1)
  pi = MLPPolicy(layers_of(12, (64,), 3), 'relu', 'tanh', device='cuda')
  env.reset()
  ms = interleaved(torch, {'single_object_fused': lambda: env.rollout_policy(pi, T, reset_first=False)}, reps, inner, restorer(env))
  return dict(summary(ms['single_object_fused']), policy='12 -> 64 -> 3', head='deterministic')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=10)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop3_policy_probe.py measures on the GPU: no HIP device visible')
  out = {'what': 'tools/tabletop3_policy_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'T': T, 'reward': 'sparse', 'reps': args.reps, 'inner': args.inner, 'cases': {}}
  for net in NETS:
    for sampled in (False, True):
      out['cases'][f'{net}-{"sampled" if sampled else "deterministic"}'] = probe(torch, net, sampled, args.reps, args.inner)
  out['single_object_fused'] = single_object(torch, args.reps, args.inner)
  gate = out['cases']['64-deterministic']
  g, f = gate['graph_policy'], gate['fused']
  out['three_over_single_object_fused'] = round(f['ms_median'] / out['single_object_fused']['ms_median'], 2)
  out['pass_condition'] = {'statement': 'fused 20 -> 64 -> 3 median < graph_policy median by more than the two spreads together',
                           'difference_ms': round(g['ms_median'] - f['ms_median'], 4), 'spreads_together_ms': round(g['spread_ms'] + f['spread_ms'], 4),
                           'met': bool(g['ms_median'] - f['ms_median'] > g['spread_ms'] + f['spread_ms'])}
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0 if out['pass_condition']['met'] else 1


if __name__ == '__main__':
  sys.exit(main())

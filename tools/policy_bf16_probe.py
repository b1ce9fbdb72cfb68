"""What bf16 STORAGE of the policy parameters (earl_mlp_policy.precision = EARL_PRECISION_BF16, MLPPolicy(param_dtype=torch.bfloat16)) buys inside the closed-loop
rollouts of the four stepper envs.  Per env at its bench batch (door and peg N = 8192, minitaur N = 4096, kitchen N = 2048), at T = 20 and at its bench length
(door 300, peg 200, minitaur 250, kitchen 400), for 64 x 64 and 256 x 256, over the same T env steps from the same state:
  (a) graph_policy    make_step_graph(T, policy=pi): the captured per-step loop, the policy as torch kernels between the steps
  (b) open_loop       rollout(actions) with the actions (c) produced -- timed BEFORE and AFTER the other legs of every repetition: the plain kernels are byte-identical
                      to the build before, so the two must agree within that leg's own repeat spread
  (c) fused_fp32      rollout_policy(pi.widened(), T): ONE launch, float32 parameters
  (d) fused_bf16      rollout_policy(pi, T): ONE launch, the same values stored as bf16 (the same actions, bit for bit: checked here before anything is timed)
Device events after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions, every run from the same env state; per leg median (min - max) ms.
From those the POLICY PHASE per env step, ((c) - (b)) / T and ((d) - (b)) / T in microseconds, and whether the difference (c) - (d) exceeds the legs' spread.
Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/policy_bf16_probe.py [--reps 5] [--envs door,peg,minitaur,kitchen] [--out profiles/policy_bf16_probe.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {'door': (8192, 300), 'peg': (8192, 200), 'minitaur': (4096, 250), 'kitchen': (2048, 400)}      # (N, bench T)
WIDTHS = {'door': (14, 4), 'peg': (14, 4), 'minitaur': (32, 8), 'kitchen': (46, 9)}
NETS = {'64x64': (64, 64), '256x256': (256, 256)}
SHORT_T = 20


def make(kind, n):
  if kind == 'door':
    from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
    return SawyerDoor(num_envs=n, scalar_api=False, info='minimal')
  if kind == 'peg':
    from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
    return SawyerPeg(num_envs=n, scalar_api=False, info='minimal')
  if kind == 'minitaur':
    from earl_benchmark_amd.envs.minitaur import Minitaur
    return Minitaur(num_envs=n, scalar_api=False)
  from earl_benchmark_amd.envs.kitchen import Kitchen
  return Kitchen(num_envs=n, scalar_api=False)


def layers_of(kind, hidden, seed=3):
  """a small-gain random network with a tanh output: most envs move gently (few rows end in the failure guard)"""
  import numpy as np
  rng = np.random.default_rng(seed)
  O, A = WIDTHS[kind]
  dims = [O] + list(hidden) + [A]
  return [((rng.standard_normal((n, k)) * (0.5 if l == len(dims) - 2 else 1.0) / np.sqrt(k)).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32))
          for l, (k, n) in enumerate(zip(dims[:-1], dims[1:]))]


def interleaved(torch, legs, reps, restore, warmup=2):
  """device-event times of every leg, the legs taking turns inside each repetition; every run starts from the same env state"""
  ms = {k: [] for k in legs}
  for i in range(warmup + reps):
    for name, fn in legs.items():
      restore()
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      torch.cuda.synchronize()
      if i >= warmup:
        ms[name].append(e0.elapsed_time(e1))
  return ms


def summary(ms):
  med = statistics.median(ms)
  return {'ms_median': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'spread': round((max(ms) - min(ms)) / med, 4),
          'ms_all': [round(x, 3) for x in ms]}


def probe(torch, kind, n, T, hidden, reps):
  from earl_benchmark_amd.policy import MLPPolicy
  O, A = WIDTHS[kind]
  env = make(kind, n)
  pi16 = MLPPolicy(layers_of(kind, hidden), 'relu', 'tanh', device='cuda', obs_dim=O, act_dim=A, param_dtype=torch.bfloat16)
  pi32 = pi16.widened()
  snap = env.state_dict()
  g = None

  def restore():
    env.load_state_dict(snap)
    if g is not None:
      g.obs_in.copy_(snap['last_obs'])                                    # the captured loop's first action belongs to the restored state too
  out = env.rollout_policy(pi32, T)
  acts, obs32, guard = out['actions'].clone(), out['obs'].clone(), float((out['status'] != 0).float().mean())
  restore()
  out16 = env.rollout_policy(pi16, T)
  identical = bool(torch.equal(out16['actions'].view(torch.int32), acts.view(torch.int32)) and torch.equal(out16['obs'].view(torch.int64), obs32.view(torch.int64)))
  if not identical:
    raise RuntimeError(f'{kind} T={T} {hidden}: the bf16 launch does not return the bits of the float32 launch of the widened policy')
  del out16, obs32
  restore()
  g = env.make_step_graph(T, policy=pi32)
  open_loop = lambda: env.rollout(acts, out=out)
  legs = {'open_loop_before': open_loop, 'graph_policy': g.replay, 'fused_fp32': lambda: env.rollout_policy(pi32, T, out=out),
          'fused_bf16': lambda: env.rollout_policy(pi16, T, out=out), 'open_loop_after': open_loop}
  ms = interleaved(torch, legs, reps, restore)
  res = {'n': n, 'T': T, 'net': [O] + list(hidden) + [A], 'guard_share': guard, 'bf16_bit_identical_to_fp32_of_widened': identical}
  for k in legs:
    res[k] = summary(ms[k])
  both = ms['open_loop_before'] + ms['open_loop_after']
  b = statistics.median(both)
  res['open_loop'] = summary(both)
  res['open_loop_moved'] = {'after_minus_before_ms': round(res['open_loop_after']['ms_median'] - res['open_loop_before']['ms_median'], 3),
                            'leg_spread_ms': round(max(max(ms[k]) - min(ms[k]) for k in ('open_loop_before', 'open_loop_after')), 3)}
  res['open_loop_moved']['within_spread'] = abs(res['open_loop_moved']['after_minus_before_ms']) <= res['open_loop_moved']['leg_spread_ms']
  c, d, a = res['fused_fp32']['ms_median'], res['fused_bf16']['ms_median'], res['graph_policy']['ms_median']
  res['policy_phase_us_per_env_step'] = {'fp32': round((c - b) / T * 1e3, 3), 'bf16': round((d - b) / T * 1e3, 3)}
  noise = max(max(ms[k]) - min(ms[k]) for k in ('fused_fp32', 'fused_bf16'))
  res['bf16_vs_fp32'] = {'fp32_minus_bf16_ms': round(c - d, 3), 'legs_spread_ms': round(noise, 3), 'beyond_spread': abs(c - d) > noise, 'bf16_over_fp32': round(d / c, 4)}
  res['fused_over_graph'] = {'fp32': round(c / a, 4), 'bf16': round(d / a, 4)}
  return res


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg,minitaur,kitchen')
  ap.add_argument('--nets', default=','.join(NETS))
  ap.add_argument('--scale', type=int, default=1, help='divide every N and the bench T by this (a rehearsal; 1 for a measurement)')
  ap.add_argument('--out', default=None, help='also write the JSON object to this file (profiles/policy_bf16_probe.json)')
  a = ap.parse_args()
  import torch
  from earl_benchmark_amd import _abi
  if not torch.cuda.is_available():
    raise SystemExit('policy_bf16_probe: needs a GPU (a timing taken elsewhere says nothing)')
  out = {'tool': 'policy_bf16_probe', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0),
         'build': {'library': _abi.load().earl_version().decode(), 'hip': torch.version.hip, 'torch': torch.__version__},
         'timing': 'device events after 2 warm-up rounds, legs interleaved over the repetitions (open loop first and last), every run from the same env state',
         'reps': a.reps, 'scale': a.scale}
  for kind in a.envs.split(','):
    n, bench_T = SIZES[kind]
    out[kind] = {}
    for T in (SHORT_T, max(SHORT_T + 1, bench_T // a.scale)):
      for name in a.nets.split(','):
        out[kind][f'T{T}_{name}'] = probe(torch, kind, max(16, n // a.scale), T, NETS[name], a.reps)
        torch.cuda.empty_cache()
        if a.out:                                                         # (kept up to date as the run goes: a run cut short leaves what it measured)
          with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
  print(json.dumps(out))


if __name__ == '__main__':
  main()

"""Closed-loop tabletop stepping, three ways, at N = 4096, T = 200 (device events, one process, interleaved rounds):
  (a) the captured per-step loop without a policy   -- env.make_step_graph(T)
  (b) the captured loop with MLPPolicy.__call__     -- env.make_step_graph(T, policy=pi): torch kernels between the captured steps
  (c) the fused launch                              -- env.rollout_policy(pi, T, episodes=E): the MLP inside the rollout kernel (csrc/tabletop_policy.h)
for the policy shapes 12 -> 64 -> 3 (ReLU, tanh out) and 12 -> 256 -> 256 -> 3 (ReLU, tanh out).  Writes env-steps/s of each, the fp32 ceiling
157.3e12 / (2 MACs per env step) and the fused figure as a fraction of it to profiles/policy_rollout_probe.json (quoted in DESIGN.md 4.1).

  python tools/policy_rollout_probe.py [--out profiles/policy_rollout_probe.json] [--n 4096] [--steps 200] [--episodes 4] [--rounds 9]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import earl_benchmark_amd as eb  # noqa: E402
from earl_benchmark_amd.policy import MLPPolicy  # noqa: E402

FP32_PEAK = 157.3e12      # MI355X dense fp32 FLOP/s (vector = f32-input MFMA rate)


def random_policy(hidden, seed, device):
  rng = np.random.default_rng(seed)
  dims = [12] + list(hidden) + [3]
  layers = [((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)) for k, n in zip(dims[:-1], dims[1:])]
  return MLPPolicy(layers, 'relu', 'tanh', device=device)


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e-3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'policy_rollout_probe.json'))
  ap.add_argument('--n', type=int, default=4096)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--episodes', type=int, default=4)
  ap.add_argument('--rounds', type=int, default=9)
  args = ap.parse_args()
  n, T, E, dev = args.n, args.steps, args.episodes, 'cuda:0'
  result = {'n': n, 'T': T, 'episodes': E, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'fp32_peak_flops': FP32_PEAK, 'shapes': {}}
  for name, hidden in (('12-64-3', (64,)), ('12-256-256-3', (256, 256))):
    pi = random_policy(hidden, 1, dev)

    def make_env():
      _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=dev, seed=5, eval_horizon=T).get_envs()
      return env
    env_a, env_b, env_c = make_env(), make_env(), make_env()
    g_a, g_b = env_a.make_step_graph(T), env_b.make_step_graph(T, policy=pi)
    legs = {'a_captured_loop_no_policy': (g_a.replay, n * T), 'b_captured_loop_torch_policy': (g_b.replay, n * T),
            'c_fused_launch': (lambda: env_c.rollout_policy(pi, T, episodes=E), n * T * E)}
    for fn, _ in legs.values():          # warm-up
      fn()
      fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):         # interleaved rounds in one process
      for k, (fn, _) in legs.items():
        times[k].append(timed(fn))
    ceiling = FP32_PEAK / (2 * pi.macs)
    shape = {'macs_per_env_step': pi.macs, 'fp32_ceiling_env_steps_per_s': ceiling}
    for k, (_, steps) in legs.items():
      med, best = statistics.median(times[k]), min(times[k])
      shape[k] = {'env_steps_per_s_median': steps / med, 'env_steps_per_s_best': steps / best, 'seconds_median': med, 'us_per_step_median': med / (steps / n) * 1e6}
    shape['fused_fraction_of_fp32_ceiling'] = shape['c_fused_launch']['env_steps_per_s_median'] / ceiling
    shape['fused_over_a'] = shape['c_fused_launch']['env_steps_per_s_median'] / shape['a_captured_loop_no_policy']['env_steps_per_s_median']
    shape['fused_over_b'] = shape['c_fused_launch']['env_steps_per_s_median'] / shape['b_captured_loop_torch_policy']['env_steps_per_s_median']
    result['shapes'][name] = shape
    print(name, json.dumps(shape))
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1)
    f.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()

"""Closed-loop tabletop stepping, three ways, at N = 4096, T = 200 (device events, one process, interleaved rounds):
  (a) the captured per-step loop without a policy   -- env.make_step_graph(T)
  (b) the captured loop with MLPPolicy.__call__     -- env.make_step_graph(T, policy=pi): torch kernels between the captured steps
  (c) the fused launch                              -- env.rollout_policy(pi, T, episodes=E): the MLP inside the rollout kernel (csrc/tabletop_policy.h)
for the policy shapes 12 -> 64 -> 3 (ReLU, tanh out) and 12 -> 256 -> 256 -> 3 (ReLU, tanh out).  Writes env-steps/s of each, the fp32 ceiling
157.3e12 / (2 MACs per env step) and the fused figure as a fraction of it to profiles/policy_rollout_probe.json (quoted in DESIGN.md 4.1).

  python tools/policy_rollout_probe.py [--out profiles/policy_rollout_probe.json] [--n 4096] [--steps 200] [--episodes 4] [--rounds 9]

--gaussian: the stochastic legs, same method, for 12 -> 64 -> 6 and 12 -> 256 -> 256 -> 6 (GaussianMLPPolicy, tanh-squashed, tanh log_std map):
  (b') the captured per-step loop with the same actor sampled in torch -- make_step_graph(T, policy=lambda obs: pi.sample(obs, torch.randn(...))), the
       randn INSIDE the capture (if the capture cannot hold it: noise pre-drawn outside the timed region, and the result says so)
  (c)  today's deterministic fused launch of the 3-output twin (rows 0..2 of the last layer)
  (c') the fused launch in SAMPLE mode                           -- env.rollout_policy(pi, T, episodes=E): the draws on wave 1 beside the output layer, the head on
       lanes 0..47 of wave 0
and writes profiles/policy_gaussian_probe.json: (c') over (b') is the bar (>= 1), (c') over (c) the price of sampling.

--population: one launch for a population of policies (earl_tabletop_population_rollout), same method, for 12 -> 64 -> 3 and 12 -> 256 -> 256 -> 3:
  (c) today's single-policy fused launch, through the unchanged entry point  -- env.rollout_policy(pi, T, episodes=E)
  (p) the population launch, P = N / 16 members of 16 envs, full outputs     -- env.rollout_policy(PolicyPopulation, T, episodes=E)
  (s) the same launch with summaries only                                    -- env.evaluate_policy(PolicyPopulation, T, episodes=E)
  (u) what a user could do before: P launches of the single-policy entry point on 16-env shards, one stream
and writes profiles/policy_population_probe.json.  The bar: (p) no slower than (c) beyond max(5 %, 3 x the round-to-round spread of (c) in this run), the
spread being (max - min) / median of (c)'s rounds; (s) is reported against (p) and (u) as the baseline, neither with a bar."""
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
from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation  # noqa: E402

FP32_PEAK = 157.3e12      # MI355X dense fp32 FLOP/s (vector = f32-input MFMA rate)


def random_policy(hidden, seed, device):
  rng = np.random.default_rng(seed)
  dims = [12] + list(hidden) + [3]
  layers = [((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)) for k, n in zip(dims[:-1], dims[1:])]
  return MLPPolicy(layers, 'relu', 'tanh', device=device)


def random_gaussian_policy(hidden, seed, device):
  """-> (the Gaussian actor, its deterministic 3-output twin)"""
  rng = np.random.default_rng(seed)
  dims = [12] + list(hidden) + [6]
  layers = [((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)) for k, n in zip(dims[:-1], dims[1:])]
  twin = layers[:-1] + [(np.ascontiguousarray(layers[-1][0][:3]), np.ascontiguousarray(layers[-1][1][:3]))]
  return GaussianMLPPolicy(layers, 'relu', squash=True, log_std_bounds=(-5.0, 2.0), log_std_map='tanh', device=device), MLPPolicy(twin, 'relu', 'tanh', device=device)


def gaussian_main(args):
  n, T, E, dev = args.n, args.steps, args.episodes, 'cuda:0'
  result = {'n': n, 'T': T, 'episodes': E, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'shapes': {}}
  for name, hidden in (('12-64-6', (64,)), ('12-256-256-6', (256, 256))):
    pi, twin = random_gaussian_policy(hidden, 1, dev)

    def make_env():
      _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=dev, seed=5, eval_horizon=T).get_envs()
      return env
    env_b, env_c, env_g = make_env(), make_env(), make_env()
    try:
      g_b = env_b.make_step_graph(T, policy=lambda obs: pi.sample(obs, torch.randn(n, 3, device=dev)))
      noise = 'torch.randn inside the capture'
    except RuntimeError as e:           # the capture could not hold the generator: noise drawn once, outside the timed region
      torch.cuda.synchronize()
      if torch.cuda.is_current_stream_capturing():      # torch.cuda.graph ends its capture when it unwinds; if one is still open nothing can be measured
        raise
      env_b = make_env()
      pre, at = torch.randn(T + 1, n, 3, device=dev), [0]

      def sampled(obs):
        at[0] += 1
        return pi.sample(obs, pre[(at[0] - 1) % (T + 1)])
      g_b = env_b.make_step_graph(T, policy=sampled)
      noise = f'pre-drawn outside the timed region ({type(e).__name__} when torch.randn was captured)'
    legs = {'b_captured_loop_torch_sampled_actor': (g_b.replay, n * T), 'c_fused_launch_deterministic_twin': (lambda: env_c.rollout_policy(twin, T, episodes=E), n * T * E),
            'c_fused_launch_sample_mode': (lambda: env_g.rollout_policy(pi, T, episodes=E), n * T * E)}
    for fn, _ in legs.values():
      fn()
      fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
      for k, (fn, _) in legs.items():
        times[k].append(timed(fn))
    shape = {'macs_per_env_step': pi.macs, 'noise_of_b': noise}
    for k, (_, steps) in legs.items():
      med, best = statistics.median(times[k]), min(times[k])
      shape[k] = {'env_steps_per_s_median': steps / med, 'env_steps_per_s_best': steps / best, 'seconds_median': med, 'us_per_step_median': med / (steps / n) * 1e6}
    rate = lambda k: shape[k]['env_steps_per_s_median']
    shape['sample_over_b'] = rate('c_fused_launch_sample_mode') / rate('b_captured_loop_torch_sampled_actor')
    shape['sample_over_deterministic'] = rate('c_fused_launch_sample_mode') / rate('c_fused_launch_deterministic_twin')
    result['shapes'][name] = shape
    print(name, json.dumps(shape))
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1)
    f.write('\n')
  print('wrote', args.out)


def population_main(args):
  n, T, E, G, dev = args.n, args.steps, args.episodes, 16, 'cuda:0'
  P = n // G
  assert n % G == 0, 'the population legs give every member 16 envs: --n a multiple of 16'
  result = {'n': n, 'T': T, 'episodes': E, 'rounds': args.rounds, 'n_policies': P, 'envs_per_policy': G, 'device': torch.cuda.get_device_name(0), 'shapes': {}}
  for name, hidden in (('12-64-3', (64,)), ('12-256-256-3', (256, 256))):
    members = [random_policy(hidden, 1 + p, dev) for p in range(P)]
    pop = PolicyPopulation(members, envs_per_policy=G, device=dev)

    def make_env(num=n, offset=0):
      _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=num, env_offset=offset, device=dev, seed=5, eval_horizon=T).get_envs()
      return env
    env_c, env_p, env_s = make_env(), make_env(), make_env()
    shards = [make_env(G, G * p) for p in range(P)]

    def per_policy_launches():
      for env, pi in zip(shards, members):
        env.rollout_policy(pi, T, episodes=E)
    legs = {'c_single_policy_fused_launch': lambda: env_c.rollout_policy(members[0], T, episodes=E), 'p_population_launch_full_outputs': lambda: env_p.rollout_policy(pop, T, episodes=E),
            's_population_launch_summary_only': lambda: env_s.evaluate_policy(pop, T, episodes=E), 'u_one_launch_per_policy_on_16_env_shards': per_policy_launches}
    for fn in legs.values():             # warm-up
      fn()
      fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):         # interleaved rounds in one process
      for k, fn in legs.items():
        times[k].append(timed(fn))
    steps = n * T * E
    shape = {'macs_per_env_step': members[0].macs, 'population_parameter_bytes': pop.params.numel() * 4}
    for k in legs:
      med, best = statistics.median(times[k]), min(times[k])
      shape[k] = {'env_steps_per_s_median': steps / med, 'env_steps_per_s_best': steps / best, 'seconds_median': med, 'seconds_rounds': times[k], 'us_per_step_median': med / (T * E) * 1e6}
    sec = lambda k: shape[k]['seconds_median']
    tc = times['c_single_policy_fused_launch']
    spread = (max(tc) - min(tc)) / statistics.median(tc)
    shape['spread_of_c'] = spread
    shape['margin'] = max(0.05, 3 * spread)
    shape['p_over_c_seconds'] = sec('p_population_launch_full_outputs') / sec('c_single_policy_fused_launch')
    shape['p_within_margin_of_c'] = shape['p_over_c_seconds'] <= 1 + shape['margin']
    shape['s_over_p_seconds'] = sec('s_population_launch_summary_only') / sec('p_population_launch_full_outputs')
    shape['u_over_p_seconds'] = sec('u_one_launch_per_policy_on_16_env_shards') / sec('p_population_launch_full_outputs')
    result['shapes'][name] = shape
    print(name, json.dumps(shape))
    del shards
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1)
    f.write('\n')
  print('wrote', args.out)


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e-3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--gaussian', action='store_true', help="the stochastic legs (b'), (c), (c') -> profiles/policy_gaussian_probe.json")
  ap.add_argument('--population', action='store_true', help='the population legs (c), (p), (s), (u) -> profiles/policy_population_probe.json')
  ap.add_argument('--n', type=int, default=4096)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--episodes', type=int, default=4)
  ap.add_argument('--rounds', type=int, default=9)
  args = ap.parse_args()
  args.out = args.out or os.path.join(REPO, 'profiles', 'policy_gaussian_probe.json' if args.gaussian else
                                      'policy_population_probe.json' if args.population else 'policy_rollout_probe.json')
  if args.gaussian:
    return gaussian_main(args)
  if args.population:
    return population_main(args)
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

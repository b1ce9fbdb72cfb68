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
spread being (max - min) / median of (c)'s rounds; (s) is reported against (p) and (u) as the baseline, neither with a bar.

--pair: the forward / reset agent pair alternating inside one launch (earl_tabletop_pair_rollout), same method, continuing form, switch_every = (25, 25), for
12 -> 64 -> 3 and 12 -> 256 -> 128 -> 3 (the widest two-hidden-layer shape a pair takes):
  (c) the unchanged single-policy entry point, T steps                        -- env.rollout_policy(forward, T, reset_first=False)
  (u) today's way for clock-only switching: T / 25 alternating 25-step single-policy launches, the goal installed by torch ops in between
  (k) the pair launch, switch_on_success = 0 (every workgroup uniform)        -- env.rollout_agents(pair, T)
  (m) the pair launch, switch_on_success = 1, on an input with mixed workgroups (envs reset at their goals, random starting phases); reports the mixed share
  (b) today's only way to switch on success: the captured per-step loop with both actors in torch and torch.where on the phase
and writes profiles/policy_pair_probe.json.  The bars, each against code that existed before the pair: (k) no slower than (u), (m) no slower than (b), beyond
max(5 %, 3 x the spread of (u) resp. (b)); (k) / (c) (the price of the ballot and the second weight set) and (m) / (k) (the price of evaluating both networks)
are reported without a bar."""
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
from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy, PolicyPopulation  # noqa: E402

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


def pair_main(args):
  n, T, dev, se = args.n, args.steps, 'cuda:0', 25
  assert T % (2 * se) == 0, '--steps a multiple of 50: whole forward + reset periods'
  result = {'n': n, 'T': T, 'switch_every': [se, se], 'rounds': args.rounds, 'form': 'continuing (reset_first = 0)', 'device': torch.cuda.get_device_name(0), 'shapes': {}}
  for name, hidden in (('12-64-3', (64,)), ('12-256-128-3', (256, 128))):
    agents = [random_policy(hidden, 1 + k, dev) for k in range(2)]
    pair_k = AgentPair(agents[0], agents[1], switch_every=se, switch_on_success=False, backward_goal='initial', device=dev)
    pair_m = AgentPair(agents[0], agents[1], switch_every=se, switch_on_success=True, backward_goal='initial', device=dev)

    def make_env(at_goal=False):
      env, _ = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', reset_train_env_at_goal=at_goal, wide_init_distr=at_goal, num_envs=n, device=dev, seed=5,
                           train_horizon=2**31 - 1).get_envs()
      return env
    env_c, env_u, env_k, env_m, env_b = make_env(), make_env(), make_env(), make_env(True), make_env(True)
    gen = torch.Generator(device=dev).manual_seed(7)

    # (u): the reset agent's goal as one more row of the goal table, goal_idx pointed at it / at a fresh task row by torch ops between the launches
    uu = env_u.unwrapped
    uu.goal_table = torch.cat([uu.goal_table, torch.as_tensor(uu.initial_state, dtype=torch.float64, device=dev)[None]], 0).contiguous()
    uu._sync_state_ptrs()
    row = uu.goal_table.shape[0] - 1

    def alternating_launches():
      for chunk in range(T // se):
        k = chunk & 1
        env_u.rollout_policy(agents[k], se, reset_first=False)
        if k == 0:
          uu.goal_idx.fill_(row)
        else:
          uu.goal_idx.copy_(torch.randint(0, 4, (n,), device=dev, generator=gen).to(torch.int32))

    # (m): random starting phases and clocks on envs that sit at their goals -> success and clock handovers at different steps inside one workgroup
    um = env_m.unwrapped
    env_m.rollout_agents(pair_m, 1)
    um.agent_phase.copy_(torch.randint(0, 2, (n,), device=dev, generator=gen).to(torch.int8))
    um.steps_in_phase.copy_(torch.randint(0, se, (n,), device=dev, generator=gen).to(torch.int32))
    last = {}

    def mixed_launch():
      last['agent'] = env_m.rollout_agents(pair_m, T)[5]

    # (b): the captured per-step loop; the phase state, the handover rule and the goal install are torch ops beside the two actors
    ub = env_b.unwrapped
    ub.goal_table = torch.cat([ub.goal_table, torch.as_tensor(ub.initial_state, dtype=torch.float64, device=dev)[None]], 0).contiguous()
    ub._sync_state_ptrs()
    phase = torch.randint(0, 2, (n,), device=dev, generator=gen).bool()
    sip = torch.randint(0, se, (n,), device=dev, generator=gen).to(torch.int32)
    task = ub.goal_idx.clone()
    draws, at = torch.randint(0, 4, (T + 1, n), device=dev, generator=gen).to(torch.int32), [0]

    def both_actors(obs):
      succ = (obs[:, 2:4] - obs[:, 8:10]).square().sum(1).sqrt() <= 0.2            # the success flag of the step that produced obs (wide_init: the mug only)
      sip.add_(1)
      over = succ | (sip >= se)
      to_forward = over & phase
      task.copy_(torch.where(to_forward, draws[at[0] % (T + 1)], task))
      at[0] += 1
      phase.logical_xor_(over)
      sip.mul_(~over)
      ub.goal_idx.copy_(torch.where(phase, torch.full_like(task, ub.goal_table.shape[0] - 1), task))
      return torch.where(phase[:, None], agents[1](obs), agents[0](obs))
    g_b = env_b.make_step_graph(T, policy=both_actors)

    legs = {'c_single_policy_fused_launch': lambda: env_c.rollout_policy(agents[0], T, reset_first=False), 'u_alternating_25_step_launches': alternating_launches,
            'k_pair_launch_clock_only': lambda: env_k.rollout_agents(pair_k, T), 'm_pair_launch_switch_on_success_mixed': mixed_launch,
            'b_captured_loop_both_actors_torch_where': g_b.replay}
    for fn in legs.values():             # warm-up
      fn()
      fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):         # interleaved rounds in one process
      for k, fn in legs.items():
        times[k].append(timed(fn))
    steps = n * T
    shape = {'macs_per_env_step': agents[0].macs}
    for k in legs:
      med, best = statistics.median(times[k]), min(times[k])
      shape[k] = {'env_steps_per_s_median': steps / med, 'env_steps_per_s_best': steps / best, 'seconds_median': med, 'seconds_rounds': times[k], 'us_per_step_median': med / T * 1e6,
                  'spread': (max(times[k]) - min(times[k])) / med}
    sec = lambda k: shape[k]['seconds_median']
    a = last['agent'].reshape(T, n // 16, 16) if n % 16 == 0 else last['agent'][:, :n // 16 * 16].reshape(T, n // 16, 16)
    any1, any0 = (a == 1).any(-1), (a == 0).any(-1)
    shape['m_share_of_workgroup_steps'] = {'mixed': float((any1 & any0).float().mean()), 'uniform_forward': float((any0 & ~any1).float().mean()),
                                           'uniform_reset': float((any1 & ~any0).float().mean())}
    ak = env_k.rollout_agents(pair_k, T)[5].reshape(T, -1)
    shape['k_share_of_workgroup_steps_mixed'] = float(((ak == 1).any(-1) & (ak == 0).any(-1)).float().mean())      # (over the whole batch: 0 = every workgroup uniform)
    for leg, base in (('k_pair_launch_clock_only', 'u_alternating_25_step_launches'), ('m_pair_launch_switch_on_success_mixed', 'b_captured_loop_both_actors_torch_where')):
      tag = leg[0] + '_over_' + base[0]
      shape[f'margin_of_{base[0]}'] = max(0.05, 3 * shape[base]['spread'])
      shape[tag + '_seconds'] = sec(leg) / sec(base)
      shape[tag + '_within_margin'] = shape[tag + '_seconds'] <= 1 + shape[f'margin_of_{base[0]}']
    shape['k_over_c_seconds'] = sec('k_pair_launch_clock_only') / sec('c_single_policy_fused_launch')
    shape['k_within_margin_of_c'] = shape['k_over_c_seconds'] <= 1 + max(0.05, 3 * shape['c_single_policy_fused_launch']['spread'])
    shape['m_over_k_seconds'] = sec('m_pair_launch_switch_on_success_mixed') / sec('k_pair_launch_clock_only')
    result['shapes'][name] = shape
    print(name, json.dumps(shape))
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
  ap.add_argument('--pair', action='store_true', help='the agent-pair legs (c), (u), (k), (m), (b) -> profiles/policy_pair_probe.json')
  ap.add_argument('--n', type=int, default=4096)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--episodes', type=int, default=4)
  ap.add_argument('--rounds', type=int, default=9)
  args = ap.parse_args()
  args.out = args.out or os.path.join(REPO, 'profiles', 'policy_gaussian_probe.json' if args.gaussian else
                                      'policy_population_probe.json' if args.population else 'policy_pair_probe.json' if args.pair else 'policy_rollout_probe.json')
  if args.gaussian:
    return gaussian_main(args)
  if args.population:
    return population_main(args)
  if args.pair:
    return pair_main(args)
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

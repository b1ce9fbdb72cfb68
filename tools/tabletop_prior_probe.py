"""What the policy-prior branches inside the MPPI planner (earl_tabletop[3]_plan_mppi_prior, env.plan_mppi(prior=...)) cost next to the planner without them and next to
the route they replace.  N = 4096 envs, K = 64 candidates of H = 32 steps, P = 8 of them prior branches, sparse reward, both tabletop envs, policies obs -> 64 -> 3 and
obs -> 256 -> 3 (tanh / tanh), I = 1 and 4 iterations, everything into preallocated tensors:
  a_plan_mppi_prior  env.plan_mppi(..., prior=pi, prior_branches=P, out=...): 3 I launches, no candidate but the P prior branches' actions in memory
  b_plan_mppi        env.plan_mppi at the same K without a prior: a - b is what the prior costs
  c_torch_route      the route it replaces on the public methods, per iteration: P times (restore the state, then H x (get_obs -> the policy in torch -> add the branch's
                     noise -> step)), restore, env.plan_candidates with rows 1 .. P overwritten by the recorded actions, env.rollout_branches, softmax weights and the
                     weighted sum in torch
Before anything is timed (a) and (c) run once from the same state (I = 1) and their [K, N] returns are compared bit for bit: the torch policy rounds differently from
the kernel's fused multiply-add chains, so under the sparse reward the returns agree unless an action's last bits move an env across a success threshold; the count
of returns that differ is recorded and the probe stops if more than 1 in 1000 do.  Device events around `--inner` back-to-back runs after 2 warm-up rounds, the legs
taking turns inside each of --reps repetitions; per leg the median, min and max of the milliseconds per run, spread = max - min.  No ratio is fixed in advance.
Prints one JSON object (--out FILE: written there too).

  python tools/tabletop_prior_probe.py [--reps 5] [--inner 2] [--out profiles/tabletop_prior_probe.json]
"""
import argparse
import datetime
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from tabletop3_policy_probe import interleaved, restorer      # noqa: E402 (the tabletop probes share their method)
from tabletop_mpc_probe import summary                         # noqa: E402

N, K, P, H = 4096, 64, 8, 32
ITERATIONS = (1, 4)
WIDTHS = (64, 256)
SIGMA, PRIOR_SIGMA, TEMPERATURE = 0.3, 0.1, 1.0


def make_env(torch, nobj, dev, n):
  if nobj == 1:
    from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  else:
    from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  env = TabletopManipulation(reward_type='sparse', num_envs=n, device=dev, seed=1, reset_at_goal=True)    # (near the goal: both values of success occur)
  env._cfg.horizon = 10 * H
  gen = torch.Generator(device=dev).manual_seed(7)
  env.rollout((torch.rand(5, n, 3, device=dev, generator=gen) * 2 - 1).contiguous())        # off the reset state
  plan0 = ((torch.rand(H, n, 3, generator=gen, device=dev) * 2 - 1) * 0.5).contiguous()
  return env, plan0


def make_policy(torch, D, width, dev):
  from earl_benchmark_amd.policy import MLPPolicy
  gen = torch.Generator().manual_seed(width)
  layers = [((torch.rand(o, i, generator=gen) * 2 - 1) * (1.5 / math.sqrt(i)), (torch.rand(o, generator=gen) * 2 - 1) * 0.3) for i, o in ((D, width), (width, 3))]
  return MLPPolicy(layers, 'tanh', 'tanh', device=dev, obs_dim=D, act_dim=3), [(w.to(dev), b.to(dev)) for w, b in layers]


def legs_of(torch, nobj, width, I, dev='cuda', n=N, k=K, p=P):
  env, plan0 = make_env(torch, nobj, dev, n)
  pi, layers = make_policy(torch, env.OBS_DIM, width, dev)
  kw = dict(device=dev)
  out_a = {'plan': torch.empty(H, n, 3, **kw), 'ret': torch.empty(k, n, dtype=torch.float64, **kw), 'prior_actions': torch.empty(p, H, n, 3, **kw)}
  out_b = {'plan': torch.empty(H, n, 3, **kw), 'ret': torch.empty(k, n, dtype=torch.float64, **kw)}
  out_c = {'ret': torch.empty(k, n, dtype=torch.float64, **kw)}
  c_plan, zeros = torch.empty(H, n, 3, **kw), torch.zeros(H, n, 3, **kw)
  step_out = (torch.empty(n, env.OBS_DIM, **kw), torch.empty(n, **kw), torch.empty(n, dtype=torch.bool, **kw), torch.empty(n, dtype=torch.bool, **kw))
  common = dict(K=k, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=5)
  restore = restorer(env)
  steps0 = env.total_step_count

  def a_plan_mppi_prior():
    env.plan_mppi(plan0, iterations=I, prior=pi, prior_branches=p, prior_sigma=PRIOR_SIGMA, out=out_a, **common)

  def b_plan_mppi():
    env.plan_mppi(plan0, iterations=I, out=out_b, **common)

  def c_torch_route():
    mean = plan0
    for j in range(I):
      cand = env.plan_candidates(mean, k, sigma=SIGMA, iteration=j, noise_counter=5)
      eps = env.plan_candidates(zeros, k, sigma=PRIOR_SIGMA, iteration=j, noise_counter=5)       # rows 1 .. P: prior_sigma * the branches' own noise
      for kk in range(1, p + 1):
        restore()
        obs = env.get_obs()
        for t in range(H):
          x = obs
          for li, (w, b) in enumerate(layers):
            x = torch.tanh(torch.addmm(b, x, w.t()))
          a = (x + eps[kk, t]).clamp(-1, 1)
          cand[kk, t].copy_(a)
          obs = env.step(a, out=step_out)[0]
      restore()
      env.total_step_count = steps0
      ret = env.rollout_branches(cand, last_obs=False, out=out_c)['ret']
      w = torch.softmax((ret - ret.max(0).values) / TEMPERATURE, 0).to(torch.float32)
      m = mean.clamp(-1, 1)
      mean = (m + (w[:, None, :, None] * (cand - m[None])).sum(0)).clamp(-1, 1)
    c_plan.copy_(mean)

  return env, {'a_plan_mppi_prior': a_plan_mppi_prior, 'b_plan_mppi': b_plan_mppi, 'c_torch_route': c_torch_route}, (out_a, out_b, out_c, c_plan), restore


def probe(torch, nobj, width, I, reps, inner):
  env, legs, (out_a, out_b, out_c, c_plan), restore = legs_of(torch, nobj, width, I)
  checks = {}
  if I == 1:
    legs['a_plan_mppi_prior']()
    legs['c_torch_route']()
    torch.cuda.synchronize()
    differ = int((out_a['ret'] != out_c['ret']).sum())
    checks = {'returns_a_vs_c_bit_equal': differ == 0, 'returns_that_differ': differ, 'of': int(out_a['ret'].numel()),
              'plan_max_abs_difference_a_vs_c': float((out_a['plan'] - c_plan).abs().max())}
    if differ > out_a['ret'].numel() // 1000:
      raise SystemExit(f'tools/tabletop_prior_probe.py: plan_mppi(prior) and the torch route disagree on {differ} returns: nothing worth timing')
  ms = interleaved(torch, legs, reps, inner, restore)
  res = {name: summary(v) for name, v in ms.items()}
  a, b, c = (res[key]['ms_median'] for key in ('a_plan_mppi_prior', 'b_plan_mppi', 'c_torch_route'))
  beyond = lambda x, y: bool(abs(res[x]['ms_median'] - res[y]['ms_median']) > res[x]['spread_ms'] + res[y]['spread_ms'])
  return {'obs_dim': env.OBS_DIM, 'width': width, 'iterations': I, 'legs': res, 'checks': checks, 'prior_cost_ms_a_minus_b': round(a - b, 4), 'a_over_b': round(a / b, 3),
          'c_over_a': round(c / a, 2), 'a_minus_b_beyond_the_spreads': beyond('a_plan_mppi_prior', 'b_plan_mppi'), 'c_minus_a_beyond_the_spreads': beyond('c_torch_route', 'a_plan_mppi_prior'),
          'policy_evaluations_per_call': P * H * N * I, 'ns_per_policy_evaluation_from_a_minus_b': round((a - b) * 1e6 / (P * H * N * I), 4)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=2)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop_prior_probe.py measures on the GPU: no HIP device visible')
  out = {'what': 'tools/tabletop_prior_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'K': K, 'P': P, 'H': H, 'sigma': SIGMA, 'prior_sigma': PRIOR_SIGMA, 'temperature': TEMPERATURE, 'reward': 'sparse', 'reps': args.reps, 'inner': args.inner,
         'warmup': 2, 'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count)}
  for tag, nobj in (('one_object', 1), ('three_objects', 3)):
    out[tag] = {f'width_{w}': {f'iterations_{I}': probe(torch, nobj, w, I, args.reps, args.inner) for I in ITERATIONS} for w in WIDTHS}
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

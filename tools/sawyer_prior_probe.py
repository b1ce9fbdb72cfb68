"""What policy-prior branches cost in the Sawyer MPPI planning step (earl_sawyer_plan_mppi_prior, env.plan_mppi(prior=, prior_branches=, prior_sigma=)).  Door and peg,
sparse reward, H = 20, one iteration, P = K / 8 prior branches, the plan probe's shapes with K in {64, 256}: (N envs, K candidates) = (64, 64) and (16, 256); priors
14 -> 64 -> 64 -> 4 and 14 -> 256 -> 256 -> 4.  Three legs:
  (a) plan_mppi_prior    env.plan_mppi(mean, K=, iterations=1, prior=pi, prior_branches=K / 8, prior_sigma=0.1, out=) in the shipped launch shape: candidates, ONE launch
                         of the prior kernel over all K N virtual envs (the first K - P branches load their action inside it), the update
  (b) ..._two_launches   the same call in the other shape (earl_debug_set_sawyer_prior_launches(2)): the untouched branch kernels over the first (K - P) N virtual envs,
                         then the prior kernel over the last P N, each behind its replicate launch
  (c) plan_mppi          env.plan_mppi(mean, K=, iterations=1, out=) without the keywords, on this build
  (d) plan_mppi_parent   the same call through the PARENT commit's libearl_hip.so (--parent: a path to that library), loaded beside this build's in the same process,
                         so that the legs take turns inside each repetition (left out without --parent)
Device events around each run after one warm-up round, the legs taking turns inside each of --reps repetitions; no leg moves the env; per leg the median, min, max,
spread = max - min.  Reported per cell: (a) - (d) and (a) / (d), THE COST OF THE PRIOR at the same K (against (c) without --parent); (c) - (d) with the two spreads and
whether the outputs are the same bits.  The verdict per cell, stated before anything was measured: the prior branches are an eighth of the candidates, so a prior that
cost its share of the work would leave (a) within (d) / 8 of (d); FAVOURABLE where (a) - (d) <= (d) / 8 + the two spreads together, UNFAVOURABLE otherwise.  When K N
fits one round of waves (both shapes here: 4096 virtual envs on 1024 SIMDs) the second launch cannot overlap the first and about doubles the latency, so UNFAVOURABLE
is the expected outcome of the two-launch shape (b); the one-launch shape (a) is what ships where it measures faster.
THE ONE CONDITION: (c) against (d) within the two spreads together in every cell, with the same bits -- prior=None runs the old kernels.

  python tools/sawyer_prior_probe.py [--reps 5] [--envs door,peg] [--parent PATH/libearl_hip.so] [--out profiles/sawyer_prior_probe.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sawyer_branch_probe import H, summary                      # noqa: E402  (the branch probe's horizon and figures)
from sawyer_plan_probe import SIGMA, TEMPERATURE                # noqa: E402
from sawyer_policy_probe import NETS, interleaved, layers_of    # noqa: E402  (the Sawyer probes share their method and their networks)
from sawyer_value_probe import outs, parent_library, setup      # noqa: E402

SHAPES = ((64, 64), (16, 256))                                  # the earlier probes' N at K = 64 and K = 256
PRIOR_SIGMA = 0.1


def probe(torch, kind, n, K, hidden, reps, parent):
  from earl_benchmark_amd.policy import MLPPolicy
  env, mean = setup(torch, kind, n)
  pi = MLPPolicy(layers_of(hidden), 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4)
  P = K // 8
  out = outs(torch, n, K)
  pout = dict(outs(torch, n, K), prior_actions=torch.empty(P, H, n, 4, device='cuda'))

  def plan_mppi_prior():
    env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=pout, prior=pi, prior_branches=P, prior_sigma=PRIOR_SIGMA)

  def plan_mppi():
    env.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=out)

  def plan_mppi_prior_two_launches():
    assert env._lib.earl_debug_set_sawyer_prior_launches(2) == 0
    try:
      plan_mppi_prior()
    finally:
      assert env._lib.earl_debug_set_sawyer_prior_launches(1) == 0

  legs = {'a_plan_mppi_prior': plan_mppi_prior, 'b_plan_mppi_prior_two_launches': plan_mppi_prior_two_launches, 'c_plan_mppi': plan_mppi}
  if parent is not None:
    old, _ = setup(torch, kind, n)
    old._lib = parent                                    # (the structs and the device tables are the same on both sides of this commit)
    old_out = outs(torch, n, K)
    legs['d_plan_mppi_parent'] = lambda: old.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=3, out=old_out)
  ms = interleaved(torch, legs, reps, lambda: None, warmup=1)
  res = {k: summary(v, n * K * H) for k, v in ms.items()}
  a, b, c = res['a_plan_mppi_prior'], res['b_plan_mppi_prior_two_launches'], res['c_plan_mppi']
  base = res.get('d_plan_mppi_parent', c)
  cost = a['ms_median'] - base['ms_median']
  favourable = cost <= base['ms_median'] / 8 + a['spread_ms'] + base['spread_ms']
  replay = env.rollout_branches(torch.cat([env.plan_candidates(mean, K, sigma=SIGMA, noise_counter=3)[:K - P], pout['prior_actions']]))
  rec = {'n': n, 'K': K, 'P': P, 'H': H, 'iterations': 1, 'virtual_envs': n * K, 'prior_net': [14] + list(hidden) + [4], 'prior_sigma': PRIOR_SIGMA, 'legs': res,
         'baseline': 'd_plan_mppi_parent' if parent is not None else 'c_plan_mppi', 'a_minus_baseline_ms': round(cost, 3),
         'a_over_baseline': round(a['ms_median'] / base['ms_median'], 3), 'b_minus_baseline_ms': round(b['ms_median'] - base['ms_median'], 3),
         'b_over_baseline': round(b['ms_median'] / base['ms_median'], 3), 'a_faster_than_b_beyond_spreads': bool(b['ms_median'] - a['ms_median'] > a['spread_ms'] + b['spread_ms']),
         'an_eighth_of_baseline_ms': round(base['ms_median'] / 8, 3),
         'spreads_ms': round(a['spread_ms'] + base['spread_ms'], 3), 'replay_identity_same_bits': bool(torch.equal(replay['ret'], pout['ret'])),
         'prior_branch_is_best_in_envs': int((pout['best_k'] >= K - P).sum()),
         'verdict': ['FAVOURABLE'] if favourable else ['UNFAVOURABLE: the prior costs more than its share of the candidates beyond the spreads']}
  if parent is not None:
    d = res['d_plan_mppi_parent']
    same_bits = bool(torch.equal(out['plan'], old_out['plan'])) and bool(torch.equal(out['ret'], old_out['ret']))
    rec.update(c_minus_d_ms=round(c['ms_median'] - d['ms_median'], 3), c_and_d_spreads_ms=round(c['spread_ms'] + d['spread_ms'], 3),
               c_equals_d_within_spreads=bool(abs(c['ms_median'] - d['ms_median']) <= c['spread_ms'] + d['spread_ms']), c_and_d_same_bits=same_bits)
  return rec


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--parent', help="the parent commit's libearl_hip.so: leg (d)")
  ap.add_argument('--out')
  args = ap.parse_args()
  kinds = args.envs.split(',')
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/sawyer_prior_probe.py measures on the GPU: no HIP device visible')
  parent = parent_library(args.parent) if args.parent else None
  res = {'what': 'tools/sawyer_prior_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'boxes': 1, 'build': eb.__version__,
         'reward': 'sparse', 'H': H, 'iterations': 1, 'sigma': SIGMA, 'temperature': TEMPERATURE, 'prior_branches': 'K / 8', 'prior_sigma': PRIOR_SIGMA, 'reps': args.reps,
         'warmup': 1, 'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count), 'parent_leg': parent is not None,
         'launch_shape': '(a), the default: one launch of the prior kernel over all K N virtual envs; (b): the plain branch kernels over the first (K - P) N, then the prior '
                         'kernel over the last P N',
         'rule': 'FAVOURABLE where (a) - baseline <= baseline / 8 + the two spreads together (the prior branches are an eighth of the candidates)',
         'timing': 'device events around one run, legs interleaved over the repetitions in one process, every run from the same env state (no leg moves the env); '
                   'spread = max - min'}
  for kind in kinds:
    res[kind] = {}
    for n, K in SHAPES:
      for net, hidden in NETS.items():
        res[kind][f'N{n}_K{K}_P{net}'] = probe(torch, kind, n, K, hidden, args.reps, parent)
        print(f'{kind} N={n} K={K} prior={net}: done', file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
  if parent is not None:
    cells = [res[k][c] for k in kinds for c in res[k]]
    res['the_one_condition'] = {'what': '(c) plan_mppi on this build against (d) the same call on the parent build: |median difference| <= the two spreads together',
                                'holds_everywhere': all(c['c_equals_d_within_spreads'] for c in cells), 'same_bits_everywhere': all(c['c_and_d_same_bits'] for c in cells)}
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

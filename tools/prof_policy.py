"""Where a step of the closed-loop policy kernel spends its cycles: runs the stamped build (tools/build_policy_stamped.sh) at N = 4096, T = 200 for the
probe's two policy shapes and prints / writes the per-phase s_memtime sums of wave 0 of workgroup 0 per step (ticks of the constant-rate counter) and each
phase's share of the step.  The stamps cost
time of their own; the shipped kernel's timings are those of tools/policy_rollout_probe.py.

  bash tools/build_policy_stamped.sh && python tools/prof_policy.py [--out profiles/policy_rollout_phases.json]
  python tools/prof_policy.py --gaussian [--out profiles/policy_gaussian_phases.json]     # the Gaussian-head kernels in SAMPLE mode: a sixth phase, the head on
                                                                                          # wave 0 (the draws run on wave 1 under the output layer's phase)
  python tools/prof_policy.py --pair [--out profiles/policy_pair_phases.json]             # the agent-pair kernel with clock-only switching (every workgroup uniform)
                                                                                          # beside the single-policy kernel on the same env form: the probe's
                                                                                          # legs (k) and (c), continuing form, switch_every = (25, 25).  The stamps
                                                                                          # are in csrc/tabletop_pair_kernel.h's pair_kernel; the stamped build
                                                                                          # recompiles the one-object unit only, so they read pair_kernel<1, ..>"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from earl_benchmark_amd import _abi  # noqa: E402

_abi.LIB_PATH = os.path.join(REPO, 'tools', 'ubench', 'libearl_policy_stamped.so')
import torch  # noqa: E402
import earl_benchmark_amd as eb  # noqa: E402
from earl_benchmark_amd.policy import AgentPair  # noqa: E402
from policy_rollout_probe import random_gaussian_policy, random_policy  # noqa: E402

PHASES = ('obs_to_lds+barrier', 'layer0+barrier', 'hidden_layer+barrier', 'output_layer+barrier', 'env_step')
GAUSSIAN_PHASES = PHASES + ('gaussian_head',)


def read(name, count):
  buf = (C.c_uint64 * count)()
  assert getattr(C.CDLL(_abi.LIB_PATH), name)(buf) == 0
  return list(buf)


def pair_main(out):
  n, T, dev, se = 4096, 200, 'cuda:0', 25
  res = {'n': n, 'T': T, 'switch_every': [se, se], 'form': 'continuing (reset_first = 0)',
         'unit': 's_memtime ticks per step and share of the step, wave 0 of workgroup 0, stamped build', 'shapes': {}}
  for name, hidden in (('12-64-3', (64,)), ('12-256-128-3', (256, 128))):
    agents = [random_policy(hidden, 1 + k, dev) for k in range(2)]
    pair = AgentPair(agents[0], agents[1], switch_every=se, switch_on_success=False, backward_goal='initial', device=dev)
    envs = [eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=dev, seed=5, train_horizon=2**31 - 1).get_envs()[0] for _ in range(2)]
    shape = {}
    for leg, launch, reader in (('c_single_policy_kernel', lambda: envs[0].rollout_policy(agents[0], T, reset_first=False), 'earl_debug_read_policy_profile'),
                                ('k_pair_kernel_clock_only', lambda: envs[1].rollout_agents(pair, T), 'earl_debug_read_policy_pair_profile')):
      for _ in range(3):
        launch()
      torch.cuda.synchronize()
      ticks = [v / T for v in read(reader, len(PHASES))]
      shape[leg] = {'ticks_per_step': dict(zip(PHASES, ticks), total=sum(ticks)), 'share': {k: v / sum(ticks) for k, v in zip(PHASES, ticks)}}
    shape['k_over_c_ticks'] = dict({k: (shape['k_pair_kernel_clock_only']['ticks_per_step'][k] / shape['c_single_policy_kernel']['ticks_per_step'][k]
                                        if shape['c_single_policy_kernel']['ticks_per_step'][k] else None) for k in PHASES + ('total',)})
    res['shapes'][name] = shape
    print(name, json.dumps(shape))
  with open(out, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--pair', action='store_true', help='the agent-pair kernel beside the single-policy kernel -> profiles/policy_pair_phases.json')
  ap.add_argument('--gaussian', action='store_true', help='the Gaussian-head kernels (SAMPLE mode) -> profiles/policy_gaussian_phases.json')
  args = ap.parse_args()
  if args.pair:
    assert _abi.load()._handle
    return pair_main(args.out or os.path.join(REPO, 'profiles', 'policy_pair_phases.json'))
  args.out = args.out or os.path.join(REPO, 'profiles', 'policy_gaussian_phases.json' if args.gaussian else 'policy_rollout_phases.json')
  phases = GAUSSIAN_PHASES if args.gaussian else PHASES
  shapes = (('12-64-6', (64,)), ('12-256-256-6', (256, 256))) if args.gaussian else (('12-64-3', (64,)), ('12-256-256-3', (256, 256)))
  n, T, dev = 4096, 200, 'cuda:0'
  lib = _abi.load()
  res = {'n': n, 'T': T, 'unit': 's_memtime ticks per step and share of the step, wave 0 of workgroup 0, stamped build', 'shapes': {}}
  for name, hidden in shapes:
    pi = random_gaussian_policy(hidden, 1, dev)[0] if args.gaussian else random_policy(hidden, 1, dev)
    _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=dev, seed=5, eval_horizon=T).get_envs()
    for _ in range(3):
      env.rollout_policy(pi, T, episodes=1)
    torch.cuda.synchronize()
    buf = (C.c_uint64 * len(phases))()
    reader = 'earl_debug_read_policy_gaussian_profile' if args.gaussian else 'earl_debug_read_policy_profile'     # (each unit reads its own sums)
    assert lib._handle and getattr(C.CDLL(_abi.LIB_PATH), reader)(buf) == 0
    ticks = [v / T for v in buf]
    res['shapes'][name] = {'ticks_per_step': dict(zip(phases, ticks), total=sum(ticks)), 'share': {k: v / sum(ticks) for k, v in zip(phases, ticks)}}
    print(name, res['shapes'][name])
  with open(args.out, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()

"""The closed loop of the kitchen, three ways over the same T env steps at N = 2048 (the bench's batch), from the reset state:
  (a) graph_policy   make_step_graph(T, policy=pi): T captured T = 1 launches with the policy as torch kernels in between -- the closed loop there was before
  (b) open_loop      rollout(actions) with the actions (c) produced: the floor, all actions known up front
  (c) rollout_policy rollout_policy(pi, T): ONE launch, the policy evaluated inside the rollout kernel
for two networks (46 -> 64 -> 64 -> 9 and 46 -> 256 -> 256 -> 9) and two lengths (T = 20 and T = 400, the bench's horizon).  Device events after warm-up;
the legs are interleaved over --reps repetitions, every run from the same env state (the noise counter included); per leg median / min / max ms and env-steps/s, the
ratios (c)/(a), (c)/(b) and the share of rows in the failure guard.  What (c)/(a) shows: a captured loop of T one-step launches lasts T times the slowest wave of a
step, one launch of T steps the slowest wave's sum.
--parent-lib PATH: leg (b) with scripted actions is also timed in child processes that load another build of libearl_hip.so (the parent commit's) and this build's,
taking turns before and after the three legs' runs: the open-loop path must not have slowed.  The gate per T: this build's median within
max(5 %, 3 x the spread of the other build's runs) of the other build's median.  Prints one JSON object (--out FILE: written there too).

  python tools/kitchen_policy_probe.py [--reps 5] [--parent-lib /path/to/libearl_hip.so] [--out profiles/kitchen_policy_probe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 2048
LENGTHS = (20, 400)
NETS = {'64x64': (64, 64), '256x256': (256, 256)}


def make(n):
  from earl_benchmark_amd.envs.kitchen import Kitchen
  return Kitchen(num_envs=n, scalar_api=False)


def layers_of(hidden, seed=3):
  """a small-gain random network with a tanh output: actions in [-1, 1], where the kitchen does not diverge"""
  import numpy as np
  rng = np.random.default_rng(seed)
  dims = [46] + list(hidden) + [9]
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


def summary(ms, n, T):
  med = statistics.median(ms)
  return {'ms_median': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'env_steps_per_s': n * T / (med * 1e-3),
          'spread': round((max(ms) - min(ms)) / med, 4), 'ms_all': [round(x, 3) for x in ms]}


def probe(torch, T, hidden, reps, n=N):
  from earl_benchmark_amd.policy import MLPPolicy
  env = make(n)
  pi = MLPPolicy(layers_of(hidden), 'relu', 'tanh', device='cuda', obs_dim=46, act_dim=9)
  snap = env.state_dict()
  g = None

  def restore():
    env.load_state_dict(snap)
    if g is not None:
      g.obs_in.copy_(snap['last_obs'])                                    # the captured loop's first action belongs to the restored state too
  out = env.rollout_policy(pi, T)
  acts, guard = out['actions'].clone(), float((out['status'] != 0).float().mean())
  restore()
  g = env.make_step_graph(T, policy=pi)
  legs = {'graph_policy': g.replay, 'open_loop': lambda: env.rollout(acts, out=out), 'rollout_policy': lambda: env.rollout_policy(pi, T, out=out)}
  ms = interleaved(torch, legs, reps, restore)
  res = {'n': n, 'T': T, 'net': [46] + list(hidden) + [9], 'guard_share': guard}
  for k in legs:
    res[k] = summary(ms[k], n, T)
  res['policy_over_graph'] = res['rollout_policy']['ms_median'] / res['graph_policy']['ms_median']
  res['policy_over_open'] = res['rollout_policy']['ms_median'] / res['open_loop']['ms_median']
  return res


def open_loop_only(torch, T, reps, n=N):
  """leg (b) alone with scripted uniform actions: what a build without the policy entry point can run too"""
  env = make(n)
  gen = torch.Generator(device='cuda').manual_seed(3)
  acts = (torch.rand(T, n, 9, generator=gen, device='cuda') * 2 - 1).to(torch.float32)
  snap = env.state_dict()
  out = env.rollout(acts)
  ms = interleaved(torch, {'open_loop': lambda: env.rollout(acts, out=out)}, reps, lambda: env.load_state_dict(snap))
  return summary(ms['open_loop'], n, T)


def gate(other, own):
  """per T: this build's open-loop median against the other build's, margin max(5 %, 3 x the other build's spread over all its runs)"""
  res = {}
  for T in other[0]:
    o = [x for run in other for x in run[T]['ms_all']]
    m = [x for run in own for x in run[T]['ms_all']]
    om, mm = statistics.median(o), statistics.median(m)
    margin = max(0.05, 3 * (max(o) - min(o)) / om)
    res[T] = {'other_ms_median': round(om, 3), 'this_ms_median': round(mm, 3), 'ratio': round(mm / om, 4), 'margin': round(margin, 4), 'passed': mm <= om * (1 + margin)}
  return res


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--out', default=None, help='also write the JSON object to this file (profiles/kitchen_policy_probe.json)')
  ap.add_argument('--open-loop-only', default=None, help='(child process) load this libearl_hip.so and time leg (b) alone')
  ap.add_argument('--legs-only', action='store_true', help='(child process) the three legs of this build')
  a = ap.parse_args()
  if a.open_loop_only:
    from earl_benchmark_amd import _abi
    if a.open_loop_only != 'own':
      _abi.LIB_PATH = a.open_loop_only
      _abi.SIGNATURES.pop('earl_kitchen_policy_rollout', None)           # (an older build does not export it)
    import torch
    print(json.dumps({str(T): open_loop_only(torch, T, a.reps) for T in LENGTHS}))
    return
  if a.legs_only:
    import torch
    res = {'device': torch.cuda.get_device_name(0)}
    for T in LENGTHS:
      for name, hidden in NETS.items():
        res[f'T{T}_{name}'] = probe(torch, T, hidden, a.reps)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    return

  # this process never opens the GPU: every measurement runs in a child of its own, one at a time
  def child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), *args], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
      raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])
  out = {'tool': 'kitchen_policy_probe', 'timing': 'device events after 2 warm-up runs, legs interleaved over the repetitions, every run from the same env state'}
  if a.parent_lib:                                                        # children before and after the legs, the two builds taking turns
    out['open_loop_other_build'] = [child('--open-loop-only', a.parent_lib)]
    out['open_loop_this_build'] = [child('--open-loop-only', 'own')]
  out.update(child('--legs-only'))
  if a.parent_lib:
    out['open_loop_other_build'].append(child('--open-loop-only', a.parent_lib))
    out['open_loop_this_build'].append(child('--open-loop-only', 'own'))
    out['open_loop_gate'] = gate(out['open_loop_other_build'], out['open_loop_this_build'])
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(out, f, indent=1)
      f.write('\n')
  print(json.dumps(out))


if __name__ == '__main__':
  main()

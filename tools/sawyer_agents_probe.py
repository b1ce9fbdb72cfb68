"""The Sawyer agent pair in its general form (earl_sawyer_agents_rollout) on the door and the peg, N = 8192 envs, 14 -> 64 -> 64 -> 4, the bench's T (door 300, peg 200),
handover every 25 steps or on success, every run from the reset state:
  (a) pair_one_row      rollout_agents(pair, T), backward_goal ONE row: what the pair did before
  (b) pair_table        rollout_agents(pair, T), a table of 15 backward goals (the peg: 'initial_states'; the door: 15 rows around its initial state).  The trajectories
                        differ from (a)'s, so (b) / (a) bounds the cost of the draw; it does not isolate it
  (c) pair_population   rollout_agents(PairPopulation of 512 pairs, 16 envs each, T), ONE row: against (a), one pair at N
  (d) per_member        door only: 128 launches of rollout_agents(one member's pair, T) on a 16-env env (put back to the reset state before each: a dozen small
                        copies, included), scaled to the 512 members: what (c) replaces
  (e) evaluate_agents   evaluate_agents(pair, T) with the table, against (b); and the peak of device memory above the resident state of (b) when it allocates its outputs, and of (e)
Device events after one warm-up; the legs are interleaved over --reps repetitions; ONE measurement (one env kind, or one build's gate legs) per child process; per leg
median / min / max ms and the share of rows in the failure guard.
--parent-lib PATH: the gate on the shared kernel.  rollout, rollout_policy and the ONE-row pair launch (earl_sawyer_pair_rollout, which both builds export) of door and
peg at the bench's T, this build and another build of libearl_hip.so (the parent commit's) in child processes taking turns, two each; margin max(5 %, 3 x the parent
legs' own spread); a miss ends with status 1.

  python tools/sawyer_agents_probe.py [--reps 5] [--envs door,peg] [--parent-lib /path/to/libearl_hip.so] [--out profiles/sawyer_agents_probe.json]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sawyer_policy_probe import BENCH_T, NETS, interleaved, layers_of, make, summary      # noqa: E402

N, EVERY, HIDDEN, P, G, MEMBER_LAUNCHES = 8192, 25, NETS['64x64'], 512, 16, 128


def agents(seed):
  from earl_benchmark_amd.policy import MLPPolicy
  return [MLPPolicy(layers_of(HIDDEN, seed=seed + k), 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4) for k in range(2)]


def guard_of(out):
  return float((out['status'] != 0).float().mean())


def probe(torch, kind, reps):
  import numpy as np
  from earl_benchmark_amd.policy import AgentPair, PairPopulation
  T = BENCH_T[kind]
  env = make(kind, N)
  row = np.asarray(env.initial_states[0], dtype=np.float64)
  if kind == 'peg':
    table = 'initial_states'
  else:
    table = np.repeat(row[None], 15, 0)
    table[:, 4:7] += 0.002 * np.arange(15)[:, None] * np.array([1.0, -0.5, 0.25])
  kw = dict(switch_every=EVERY, switch_on_success=True, obs_dim=14, act_dim=4)
  one = AgentPair(*agents(3), backward_goal=row, **kw)
  tab = AgentPair(*agents(3), backward_goal=table, **kw)
  pop = PairPopulation([AgentPair(*agents(3 + 2 * p), backward_goal=row, **kw) for p in range(P)], envs_per_policy=G, device='cuda')
  out = env.rollout_agents(one, T)                                        # (allocates the phase state and the outputs every leg writes into)
  out_t = dict(out, backward_row=torch.empty(T, N, dtype=torch.int32, device='cuda'))
  env.evaluate_agents(tab, 1)                                             # (... and the table's row state)
  env.reset()
  snap = env.state_dict()

  def restore():
    env.load_state_dict(snap)

  legs = {'pair_one_row': lambda: env.rollout_agents(one, T, out=out), 'pair_table': lambda: env.rollout_agents(tab, T, out=out_t),
          'pair_population': lambda: env.rollout_agents(pop, T, out=out), 'evaluate_agents': lambda: env.evaluate_agents(tab, T)}
  guards = {}
  for k in ('pair_one_row', 'pair_table', 'pair_population'):
    restore()
    guards[k] = guard_of(legs[k]())
  restore()
  guards['evaluate_agents'] = float(env.evaluate_agents(tab, T)['guard_steps'].sum()) / (N * T)
  small = None
  if kind == 'door':
    small = make(kind, G)
    members = [pop.pair(p) for p in range(MEMBER_LAUNCHES)]
    out_s = small.rollout_agents(members[0], T)
    small.reset()
    snap_s = small.state_dict()

    def per_member():
      for m in members:
        small.load_state_dict(snap_s)
        small.rollout_agents(m, T, out=out_s)
    legs['per_member'] = per_member
    small.load_state_dict(snap_s)
    guards['per_member'] = guard_of(small.rollout_agents(members[0], T, out=out_s))
  ms = interleaved(torch, legs, reps, restore, warmup=1)
  # peak device memory above the resident state: rollout_agents allocating its own outputs, and evaluate_agents
  peaks = {}
  del out, out_t
  torch.cuda.empty_cache()
  for k, fn in (('rollout_agents', lambda: env.rollout_agents(tab, T)), ('evaluate_agents', lambda: env.evaluate_agents(tab, T))):
    restore()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peaks[k] = int(torch.cuda.max_memory_allocated() - base)
    torch.cuda.empty_cache()
  res = {'n': N, 'T': T, 'net': [14] + list(HIDDEN) + [4], 'switch_every': EVERY, 'switch_on_success': True, 'table_rows': 15, 'pairs': P, 'envs_per_pair': G,
         'guard_share': guards, 'peak_bytes_above_resident_state': peaks}
  for k in legs:
    res[k] = summary(ms[k], N if k != 'per_member' else G * MEMBER_LAUNCHES, T)
  med = lambda k: res[k]['ms_median']
  res['pair_table_over_pair_one_row'] = round(med('pair_table') / med('pair_one_row'), 4)
  res['pair_population_over_pair_one_row'] = round(med('pair_population') / med('pair_one_row'), 4)
  res['evaluate_agents_over_pair_table'] = round(med('evaluate_agents') / med('pair_table'), 4)
  if kind == 'door':
    res['per_member_launches_timed'] = MEMBER_LAUNCHES
    res['per_member_scaled_to_all_pairs_ms'] = round(med('per_member') * P / MEMBER_LAUNCHES, 3)
    res['per_member_scaled_over_pair_population'] = round(med('per_member') * P / MEMBER_LAUNCHES / med('pair_population'), 2)
  return res


def gate_legs(torch, kind, reps):
  """(child process) the gate's legs at N, the bench's T, the 64 x 64 network, through entry points both builds export"""
  from earl_benchmark_amd import _abi
  from earl_benchmark_amd.policy import AgentPair
  T = BENCH_T[kind]
  env = make(kind, N)
  fwd, bwd = agents(3)
  row = torch.as_tensor(env.initial_states[0], dtype=torch.float64, device='cuda')
  pair = AgentPair(fwd, bwd, switch_every=EVERY, switch_on_success=True, backward_goal=row, obs_dim=14, act_dim=4)
  snap = env.state_dict()
  out = env.rollout_policy(fwd, T)
  acts = out['actions'].clone()
  out['agent'] = torch.empty(T, N, dtype=torch.int8, device='cuda')
  phase, sip = torch.zeros(N, dtype=torch.int8, device='cuda'), torch.zeros(N, dtype=torch.int32, device='cuda')
  fs, bs = torch.empty(N, dtype=torch.int32, device='cuda'), torch.empty(N, dtype=torch.int32, device='cuda')
  o = _abi.SawyerOut(obs=out['obs'].data_ptr(), reward=out['reward'].data_ptr(), done=out['done'].data_ptr(), success=out['success'].data_ptr(),
                     status=out['status'].data_ptr(), info=None)
  ps = _abi.AgentPair(switch_every=(C.c_int32 * 2)(EVERY, EVERY), switch_on_success=1, pad_=0, param_stride=pair.stride, backward_goal=row.data_ptr(),
                      phase=phase.data_ptr(), steps_in_phase=sip.data_ptr(), agent_out=out['agent'].data_ptr(), forward_success=fs.data_ptr(), backward_success=bs.data_ptr())

  def pair_one_row():
    phase.zero_()
    sip.zero_()
    env._cfg.step_counter = env.total_step_count
    if env._uses_queue(T):
      env.sched.zero_()
    _abi.check(env._lib.earl_sawyer_pair_rollout(env.model.buf.data_ptr(), env.model.col_ptr, env.nv, env._cfg_ref, env._st_ref, C.byref(pair.struct), C.byref(ps), None,
                                                 env.last_obs.data_ptr(), T, None, out['actions'].data_ptr(), C.byref(o), env._stream()), 'earl_sawyer_pair_rollout')
  legs = {'rollout_policy': lambda: env.rollout_policy(fwd, T, out=out), 'rollout': lambda: env.rollout(acts, out=out), 'pair_one_row': pair_one_row}
  ms = interleaved(torch, legs, reps, lambda: env.load_state_dict(snap), warmup=1)
  env.load_state_dict(snap)
  pair_one_row()
  return {'ms': {k: [round(x, 3) for x in v] for k, v in ms.items()}, 'guard_share_pair_one_row': guard_of(out)}


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--envs', default='door,peg')
  ap.add_argument('--parent-lib', default=None)
  ap.add_argument('--gate-only', action='store_true', help='skip the probe\'s legs (with --parent-lib)')
  ap.add_argument('--out', default=None, help='also write the JSON object to this file (profiles/sawyer_agents_probe.json)')
  ap.add_argument('--gate-child', default=None, help='(child process) load this libearl_hip.so (or "own") and time the gate\'s legs')
  ap.add_argument('--probe-child', default=None, help='(child process) the probe\'s legs of this env kind')
  a = ap.parse_args()
  kinds = a.envs.split(',')
  if a.gate_child:
    from earl_benchmark_amd import _abi
    if a.gate_child != 'own':
      _abi.LIB_PATH = a.gate_child
      _abi.SIGNATURES.pop('earl_sawyer_agents_rollout', None)             # (the older build does not export it; the gate's legs do not call it)
    import torch
    print(json.dumps({kind: gate_legs(torch, kind, a.reps) for kind in kinds}))
    return
  if a.probe_child:
    import torch
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'result': probe(torch, a.probe_child, a.reps)}))
    return

  def child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--reps', str(a.reps), '--envs', a.envs, *args], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
      raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])
  res = {'tool': 'sawyer_agents_probe', 'date': datetime.date.today().isoformat(),
         'timing': 'device events after 1 warm-up run, legs interleaved over the repetitions, every run from the same env state, one measurement per child process'}
  ok = True
  if a.parent_lib:                                                        # the builds take turns, two child processes each
    runs = {'parent': [], 'this': []}
    for _ in range(2):
      runs['parent'].append(child('--gate-child', a.parent_lib))
      runs['this'].append(child('--gate-child', 'own'))
    gate = {'margin': 'max(5 %, 3 x the parent legs\' own spread (max - min) / median)', 'n': N, 'net': [14, 64, 64, 4]}
    for kind in kinds:
      for leg in ('rollout', 'rollout_policy', 'pair_one_row'):
        ms = {b: [x for r in runs[b] for x in r[kind]['ms'][leg]] for b in runs}
        pm, tm = statistics.median(ms['parent']), statistics.median(ms['this'])
        spread = (max(ms['parent']) - min(ms['parent'])) / pm
        margin = max(0.05, 3 * spread)
        passed = tm <= pm * (1 + margin)
        ok = ok and passed
        gate[f'{kind}_{leg}_T{BENCH_T[kind]}'] = {'parent_ms_median': round(pm, 3), 'this_ms_median': round(tm, 3), 'ratio': round(tm / pm, 4),
                                                  'parent_spread': round(spread, 4), 'margin': round(margin, 4), 'passed': passed,
                                                  'parent_ms_all': ms['parent'], 'this_ms_all': ms['this']}
      gate[f'{kind}_guard_share_pair_one_row'] = {b: [r[kind]['guard_share_pair_one_row'] for r in runs[b]] for b in runs}
    gate['passed'] = ok
    print(f'parent gate: {"passed" if ok else "MISSED"}', file=sys.stderr, flush=True)
    res['parent_gate'] = gate
  if not a.gate_only:
    for kind in kinds:
      got = child('--probe-child', kind)
      res['device'], res[kind] = got['device'], got['result']
      print(f'{kind}: done', file=sys.stderr, flush=True)
  if a.out:
    with open(a.out, 'w') as f:
      json.dump(res, f, indent=1)
      f.write('\n')
  print(json.dumps(res))
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  main()

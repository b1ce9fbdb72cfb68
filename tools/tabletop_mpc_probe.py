"""What the fused receding-horizon launch (earl_tabletop_mpc_rollout / earl_tabletop3_mpc_rollout, env.rollout_mpc) buys over the route it replaces.
N = 4096 envs, K = 64 candidates of H = 32 steps, sparse reward, T = 50 controlled steps, I = 1 and I = 4 iterations per step, both tabletop envs, everything into
preallocated tensors:
  (f) fused    env.rollout_mpc(T, plan, out=...): one launch, the env, the plan and the K returns on chip throughout
  (e) eager    the loop the call replaces, on the public methods: per step env.plan_mppi(plan, out={'plan': plan, 'ret': workspace}) -> env.rollout(plan[:1]) ->
               the shift as two torch copies; 2 I + 1 kernel launches and two copies per step, a [K, N] float64 workspace between each pair
  (g) graph    the same loop captured once into a HIP graph and replayed (the noise counters frozen at capture: the same bits as (e) from the same state), if the
               capture works; otherwise the reason is recorded
Before anything is timed the three routes run once from the same state and their outputs are compared bit for bit (recorded, and the probe stops if they differ).
Device events around `--inner` back-to-back runs after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions, the env and the plan restored
before each timing; per leg the median, min and max of the milliseconds per run, spread = max - min.  No ratio is fixed in advance: e / f and g / f are findings.
Prints one JSON object (--out FILE: written there too, with date, device and build).

  python tools/tabletop_mpc_probe.py [--reps 5] [--inner 2] [--out profiles/tabletop_mpc_probe.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from tabletop3_policy_probe import interleaved, restorer      # noqa: E402 (the tabletop probes share their method)

N, K, H, T = 4096, 64, 32, 50
ITERATIONS = (1, 4)
DEV = 'cuda'
SIGMA, TEMPERATURE = 0.3, 1.0
KEYS = ('obs', 'reward', 'done', 'success', 'actions', 'plan')


def summary(ms):
  med = statistics.median(ms)
  return {'ms_median': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'spread_ms': round(max(ms) - min(ms), 4),
          'ms_all': [round(x, 4) for x in ms]}


def probe(torch, nobj, I, reps, inner):
  if nobj == 1:
    from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  else:
    from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device=DEV, seed=1, reset_at_goal=True)    # (near the goal: both values of success occur)
  env._cfg.horizon = 10 * (H + T)
  gen = torch.Generator(device=DEV).manual_seed(7)
  env.rollout((torch.rand(5, N, 3, device=DEV, generator=gen) * 2 - 1).contiguous())        # off the reset state
  kw = dict(device=DEV)
  plan0 = ((torch.rand(H, N, 3, generator=gen, **kw) * 2 - 1) * 0.5).contiguous()
  D = env.OBS_DIM

  def outputs():
    return {'obs': torch.zeros(T, N, D, **kw), 'reward': torch.zeros(T, N, **kw), 'done': torch.zeros(T, N, dtype=torch.bool, **kw),
            'success': torch.zeros(T, N, dtype=torch.bool, **kw), 'actions': torch.zeros(T, N, 3, **kw), 'plan': plan0.clone()}

  out_f, out_e, out_g = outputs(), outputs(), outputs()
  ws, tmp = torch.empty(K, N, dtype=torch.float64, **kw), torch.empty(H, N, 3, **kw)
  args = dict(K=K, iterations=I, sigma=SIGMA, temperature=TEMPERATURE)
  restore_env = restorer(env)

  def restore():
    restore_env()
    for o in (out_f, out_e, out_g):
      o['plan'].copy_(plan0)

  def fused():
    env.rollout_mpc(T, out_f['plan'], out=out_f, **args)

  def loop(o):
    plan = o['plan']
    for s in range(T):
      env.plan_mppi(plan, out={'plan': plan, 'ret': ws}, **args)
      env.rollout(plan[:1], out=(o['obs'][s:s + 1], o['reward'][s:s + 1], o['done'][s:s + 1], o['success'][s:s + 1]))
      o['actions'][s].copy_(plan[0])
      tmp.copy_(plan)
      plan[:-1].copy_(tmp[1:])

  def eager():
    loop(out_e)

  legs = {'f_fused': fused, 'e_eager_loop': eager}
  snap = lambda o: {k: o[k].clone() for k in KEYS}                    # (restore() puts the start plan back into every route's buffer)
  restore()
  fused()
  got_f = snap(out_f)
  restore()
  eager()
  got_e = snap(out_e)
  torch.cuda.synchronize()
  counter_after = int(env._cfg.counter)
  graph_note = 'captured'
  try:
    restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      loop(out_g)
    torch.cuda.synchronize()
    restore()
    graph.replay()
    got_g = snap(out_g)
    torch.cuda.synchronize()

    def replay():
      graph.replay()
      env._cfg.counter = counter_after                                # (the captured launches carry the counters of the capture)
    legs['g_graph_of_the_loop'] = replay
  except Exception as exc:                                            # noqa: BLE001 (whatever the capture says is the finding)
    graph_note = f'capture failed: {type(exc).__name__}: {exc}'[:300]
    torch.cuda.synchronize()
  equal = {'fused_vs_eager': all(torch.equal(got_f[k], got_e[k]) for k in KEYS)}
  if 'g_graph_of_the_loop' in legs:
    equal['graph_vs_eager'] = all(torch.equal(got_g[k], got_e[k]) for k in KEYS)
  if not all(equal.values()):
    raise SystemExit(f'tools/tabletop_mpc_probe.py: the routes disagree ({equal}): nothing worth timing')
  moved = float((got_f['actions'][0] - plan0[0].clamp(-1, 1)).abs().max())
  ms = interleaved(torch, legs, reps, inner, restore)
  res = {k: summary(v) for k, v in ms.items()}
  f, e = res['f_fused'], res['e_eager_loop']
  out = {'obs_dim': D, 'iterations': I, 'legs': res, 'outputs_bit_equal': equal, 'graph': graph_note, 'first_action_vs_clipped_plan_max_abs_difference': moved,
         'launches_per_step_of_the_loop': 2 * I + 1, 'f_ms_per_step': round(f['ms_median'] / T, 5), 'e_ms_per_step': round(e['ms_median'] / T, 5),
         'e_over_f': round(e['ms_median'] / f['ms_median'], 3),
         'e_minus_f_beyond_the_spreads': bool(abs(e['ms_median'] - f['ms_median']) > e['spread_ms'] + f['spread_ms'])}
  if 'g_graph_of_the_loop' in res:
    g = res['g_graph_of_the_loop']
    out.update(g_ms_per_step=round(g['ms_median'] / T, 5), g_over_f=round(g['ms_median'] / f['ms_median'], 3),
               g_minus_f_beyond_the_spreads=bool(abs(g['ms_median'] - f['ms_median']) > g['spread_ms'] + f['spread_ms']))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=2)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop_mpc_probe.py measures on the GPU: no HIP device visible')
  out = {'what': 'tools/tabletop_mpc_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'K': K, 'H': H, 'T': T, 'sigma': SIGMA, 'temperature': TEMPERATURE, 'reward': 'sparse', 'reps': args.reps, 'inner': args.inner, 'warmup': 2,
         'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count)}
  for tag, nobj in (('one_object', 1), ('three_objects', 3)):
    out[tag] = {f'iterations_{I}': probe(torch, nobj, I, args.reps, args.inner) for I in ITERATIONS}
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

"""What the in-kernel cross-entropy planner (earl_tabletop[3]_plan_cem, env.plan_cem) and its fused control loop (earl_tabletop[3]_mpc_rollout_cem,
env.rollout_mpc(method='cem')) cost next to the routes they replace and next to MPPI.  N = 4096 envs, K = 64 candidates of H = 32 steps, E = 8 elites, sparse reward,
both tabletop envs, everything into preallocated tensors:
  (a) planner, I = 1 and I = 4 iterations
      c_plan_cem      env.plan_cem(..., out=...): 2 I launches, the candidates never in memory
      t_torch_route   the route it replaces: env.cem_candidates -> env.rollout_branches -> a stable sort of the returns -> mean / std of the E best in torch
      m_plan_mppi     env.plan_mppi at the same K, H, I (another algorithm: timed, not compared)
      k_plan_cem_all  env.plan_cem with E = K: its update makes ALL K candidates again, as MPPI's does; k - c is what making E instead of K is worth, and from it
                      the split of c into score and update is DERIVED (update_regen ~ (k - c) * K / (K - E) * E / K; labelled as an estimate in the output)
  (b) control loop, T = 50 real steps, I = 1
      f_fused_cem     env.rollout_mpc(T, plan, method='cem', out=...): one launch
      e_eager_loop    the loop it replaces on the public methods: plan_cem -> rollout(plan[:1]) -> the shift as torch copies
      g_graph_of_the_loop  the same loop captured once into a HIP graph and replayed, if the capture works; otherwise the reason is recorded
      p_fused_mppi    env.rollout_mpc(T, plan) (method='mppi')
  (c) the rank pass at its widest: plan_cem at K = 1024, E = 64, I = 1 (and plan_mppi at K = 1024 beside it)
Before anything is timed the compared routes run once from the same state: the planner's `ret` against the torch route's bit for bit (I = 1; its plan and std, made in
float arithmetic there and in integers here, by their largest difference), the fused loop against the eager and the replayed one bit for bit; the probe stops if they
differ.  Device events around `--inner` back-to-back runs after 2 warm-up rounds, the legs taking turns inside each of --reps repetitions; per leg the median, min
and max of the milliseconds per run, spread = max - min.  No ratio is fixed in advance.  Prints one JSON object (--out FILE: written there too).

  python tools/tabletop_cem_probe.py [--reps 5] [--inner 2] [--out profiles/tabletop_cem_probe.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from tabletop3_policy_probe import interleaved, restorer      # noqa: E402 (the tabletop probes share their method)
from tabletop_mpc_probe import summary                         # noqa: E402

N, K, E, H, T = 4096, 64, 8, 32, 50
WIDE_K, WIDE_E = 1024, 64
ITERATIONS = (1, 4)
DEV = 'cuda'
SIGMA, TEMPERATURE = 0.3, 1.0
KEYS = ('obs', 'reward', 'done', 'success', 'actions', 'plan')


def make_env(torch, nobj):
  if nobj == 1:
    from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  else:
    from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  env = TabletopManipulation(reward_type='sparse', num_envs=N, device=DEV, seed=1, reset_at_goal=True)    # (near the goal: both values of success occur)
  env._cfg.horizon = 10 * (H + T)
  gen = torch.Generator(device=DEV).manual_seed(7)
  env.rollout((torch.rand(5, N, 3, device=DEV, generator=gen) * 2 - 1).contiguous())        # off the reset state
  plan0 = ((torch.rand(H, N, 3, generator=gen, device=DEV) * 2 - 1) * 0.5).contiguous()
  return env, plan0


def ratios(res, base, others):
  b = res[base]
  return {f'{o}_over_{base}': round(res[o]['ms_median'] / b['ms_median'], 3) for o in others if o in res} | {
      f'{o}_minus_{base}_beyond_the_spreads': bool(abs(res[o]['ms_median'] - b['ms_median']) > res[o]['spread_ms'] + b['spread_ms']) for o in others if o in res}


def planner(torch, nobj, I, reps, inner, k=K, e=E, torch_route=True):
  env, plan0 = make_env(torch, nobj)
  kw = dict(device=DEV)
  ar = torch.arange(N, device=DEV)

  def bufs(kk):
    return {'plan': torch.empty(H, N, 3, **kw), 'std': torch.empty(H, N, 3, **kw), 'ret': torch.empty(kk, N, dtype=torch.float64, **kw)}

  out_c, out_k, out_m = bufs(k), bufs(k), {'plan': torch.empty(H, N, 3, **kw), 'ret': torch.empty(k, N, dtype=torch.float64, **kw)}
  out_b = {'ret': torch.empty(k, N, dtype=torch.float64, **kw)}
  t_plan, t_std = torch.empty(H, N, 3, **kw), torch.empty(H, N, 3, **kw)
  cem = dict(K=k, elites=e, iterations=I, sigma=SIGMA, noise_counter=5)

  def c_plan_cem():
    env.plan_cem(plan0, out=out_c, **cem)

  def k_plan_cem_all():
    env.plan_cem(plan0, out=out_k, **{**cem, 'elites': k})

  def m_plan_mppi():
    env.plan_mppi(plan0, K=k, iterations=I, sigma=SIGMA, temperature=TEMPERATURE, noise_counter=5, out=out_m)

  def t_torch_route():
    mean, std = plan0, None
    for j in range(I):
      cand = env.cem_candidates(mean, k, sigma=SIGMA, std=std, iteration=j, noise_counter=5)
      ret = env.rollout_branches(cand, last_obs=False, out=out_b)['ret']
      top = torch.sort(ret, dim=0, descending=True, stable=True).indices[:e]              # (ties go to the smaller k, as item 4)
      el = cand[top, :, ar.expand(e, N)].permute(0, 2, 1, 3)                               # [e, H, N, 3]
      mean = el.mean(0).clamp(-1, 1)
      std = el.std(0, unbiased=False).clamp(0.0, 2.0)
    t_plan.copy_(mean)
    t_std.copy_(std)

  legs = {'c_plan_cem': c_plan_cem, 'm_plan_mppi': m_plan_mppi, 'k_plan_cem_all': k_plan_cem_all}
  c_plan_cem()
  equal = {}
  if torch_route:
    legs['t_torch_route'] = t_torch_route
    t_torch_route()
    torch.cuda.synchronize()
    if I == 1:
      equal['ret_cem_vs_torch_route_bit_equal'] = bool(torch.equal(out_c['ret'], out_b['ret']))
      if not equal['ret_cem_vs_torch_route_bit_equal']:
        raise SystemExit('tools/tabletop_cem_probe.py: plan_cem and the torch route disagree on the returns: nothing worth timing')
    equal['plan_max_abs_difference_to_torch_route'] = float((out_c['plan'] - t_plan).abs().max())
    equal['std_max_abs_difference_to_torch_route'] = float((out_c['std'] - t_std).abs().max())
  ms = interleaved(torch, legs, reps, inner, lambda: None)
  res = {name: summary(v) for name, v in ms.items()}
  c, ka = res['c_plan_cem']['ms_median'], res['k_plan_cem_all']['ms_median']
  out = {'obs_dim': env.OBS_DIM, 'K': k, 'elites': e, 'iterations': I, 'legs': res, 'checks': equal, **ratios(res, 'c_plan_cem', ('t_torch_route', 'm_plan_mppi', 'k_plan_cem_all'))}
  if k > e:
    per_candidate = (ka - c) / (k - e) / I                                                  # ms per regenerated candidate per iteration (ESTIMATE: a difference of two medians)
    out['estimate_update_regeneration_ms_per_iteration'] = round(per_candidate * e, 4)
    out['estimate_rest_ms_per_iteration_score_rank_launches'] = round(c / I - per_candidate * e, 4)
    out['estimate_regenerating_all_K_ms_per_iteration'] = round(per_candidate * k, 4)
  return out


def loop_probe(torch, nobj, reps, inner, I=1):
  env, plan0 = make_env(torch, nobj)
  kw = dict(device=DEV)
  D = env.OBS_DIM

  def outputs():
    return {'obs': torch.zeros(T, N, D, **kw), 'reward': torch.zeros(T, N, **kw), 'done': torch.zeros(T, N, dtype=torch.bool, **kw),
            'success': torch.zeros(T, N, dtype=torch.bool, **kw), 'actions': torch.zeros(T, N, 3, **kw), 'plan': plan0.clone()}

  out_f, out_e, out_g, out_p = outputs(), outputs(), outputs(), outputs()
  ws, sd, tmp = torch.empty(K, N, dtype=torch.float64, **kw), torch.empty(H, N, 3, **kw), torch.empty(H, N, 3, **kw)
  cem = dict(K=K, elites=E, iterations=I, sigma=SIGMA)
  restore_env = restorer(env)

  def restore():
    restore_env()
    for o in (out_f, out_e, out_g, out_p):
      o['plan'].copy_(plan0)

  def fused():
    env.rollout_mpc(T, out_f['plan'], out=out_f, method='cem', **cem)

  def mppi():
    env.rollout_mpc(T, out_p['plan'], out=out_p, K=K, iterations=I, sigma=SIGMA, temperature=TEMPERATURE)

  def loop(o):
    plan = o['plan']
    for s in range(T):
      env.plan_cem(plan, out={'plan': plan, 'std': sd, 'ret': ws}, **cem)
      env.rollout(plan[:1], out=(o['obs'][s:s + 1], o['reward'][s:s + 1], o['done'][s:s + 1], o['success'][s:s + 1]))
      o['actions'][s].copy_(plan[0])
      tmp.copy_(plan)
      plan[:-1].copy_(tmp[1:])

  legs = {'f_fused_cem': fused, 'e_eager_loop': lambda: loop(out_e), 'p_fused_mppi': mppi}
  snap = lambda o: {k: o[k].clone() for k in KEYS}
  restore()
  fused()
  got_f = snap(out_f)
  restore()
  loop(out_e)
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
    raise SystemExit(f'tools/tabletop_cem_probe.py: the routes disagree ({equal}): nothing worth timing')
  ms = interleaved(torch, legs, reps, inner, restore)
  res = {k: summary(v) for k, v in ms.items()}
  return {'obs_dim': D, 'iterations': I, 'legs': res, 'outputs_bit_equal': equal, 'graph': graph_note, 'launches_per_step_of_the_loop': 2 * I + 1,
          'f_ms_per_step': round(res['f_fused_cem']['ms_median'] / T, 5), **ratios(res, 'f_fused_cem', ('e_eager_loop', 'g_graph_of_the_loop', 'p_fused_mppi'))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--inner', type=int, default=2)
  ap.add_argument('--out')
  args = ap.parse_args()
  import torch
  import earl_benchmark_amd as eb
  if not torch.cuda.is_available():
    raise SystemExit('tools/tabletop_cem_probe.py measures on the GPU: no HIP device visible')
  out = {'what': 'tools/tabletop_cem_probe.py', 'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0), 'build': eb.__version__,
         'n': N, 'K': K, 'elites': E, 'H': H, 'T': T, 'sigma': SIGMA, 'temperature_of_the_mppi_legs': TEMPERATURE, 'reward': 'sparse', 'reps': args.reps,
         'inner': args.inner, 'warmup': 2, 'compute_units': int(torch.cuda.get_device_properties(0).multi_processor_count)}
  for tag, nobj in (('one_object', 1), ('three_objects', 3)):
    out[tag] = {'a_planner': {f'iterations_{I}': planner(torch, nobj, I, args.reps, args.inner) for I in ITERATIONS},
                'b_control_loop': loop_probe(torch, nobj, args.reps, args.inner),
                'c_rank_pass_K_1024': planner(torch, nobj, 1, args.reps, 1, k=WIDE_K, e=WIDE_E, torch_route=False)}
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(text + '\n')
  return 0


if __name__ == '__main__':
  sys.exit(main())

"""The Sawyer door / peg CEM planner on the device (include/earl_physics.h, "CEM planning on the door and the peg": earl_sawyer_plan_cem, earl_sawyer_cem_candidates,
earl_sawyer_cem_update; env.plan_cem, env.cem_candidates, env.mpc_rollout(method='cem')).  Every comparison is bit for bit against a reference that uses none of the new
kernels (tests/sawyer_cem_helpers.py): Python candidates on a numpy Philox with CEM's own counter word, the EXISTING rollout_branches for the returns and the
rolled-back step counts, a Python sort for the elites and Python integers for the two moments.
  1. the selection alone, through earl_sawyer_cem_update on crafted returns without stepping physics: n = 3, H = 2 (H = 9 once: more steps than waves),
     K in {1, 2, 65, 513, 8192}, E in {1, a middle value, min(K, 1024)}, the nine patterns of sawyer_cem_helpers.pattern -- each pattern's own condition asserted on
     the oracle's data first -- and the host twin at K = 8192;
  2. the whole planner: door and peg, dense and sparse, n = 5, env_offset = 3, K = 6, E = 2, H = 6, two iterations after 4 random steps: all eight outputs, the env
     byte-equal before and after; std0 given, the in-place pairs, three iterations == three calls, cem_candidates == the twin == the oracle,
     rollout_branches(cem_candidates) == ret; goal switches inside the look-ahead; a poisoned env; the eight-wave door build and the time-sliced peg schedule; shards;
     capture into a graph; the 64-lane switch; mpc_rollout(method='cem') against the loop over public methods it is defined as, and method='mppi' against its own."""
import numpy as np
import pytest

import sawyer_cem_helpers as sc
from test_physics_step_graph_gpu import make, same
from test_sawyer_branches_gpu import lifelong, snapshot, unchanged
from test_sawyer_cem import HI, LO, check_crafted, middle
from test_sawyer_plan_gpu import mean_plan, off_the_reset_pose
from test_sawyer_population_gpu import rows_of

pytestmark = pytest.mark.gpu

OUTS = ('plan', 'std', 'ret', 'ret0', 'best_ret', 'best_k', 'elite', 'fail')
SIGMA = (0.5, 0.4, 0.6, 0.8)
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- 1. the selection on crafted returns
@pytest.mark.parametrize('K', [1, 2, 65, 513, 8192])
def test_the_selection_on_crafted_returns(K):
  from earl_benchmark_amd import _abi
  lib, host = _abi.load(), _abi.load_host()
  dev = lambda *a, **kw: sc.device_update(lib, *a, **kw)
  for E in sorted({1, middle(K), min(K, sc.MAX_E)}):
    for group in range(3):
      seed = 100 * K + 10 * E + group
      check_crafted(dev, K, E, 2, group, seed, 'earl_sawyer_cem_update', std_given=group != 1)
      if K == 8192:                                                          # the host twin against the same oracle on the same inputs: device == twin
        check_crafted(lambda *a, **kw: sc.host_update(host, *a, **kw), K, E, 2, group, seed, 'the host twin', std_given=group != 1)


def test_more_plan_steps_than_waves_and_the_in_place_update():
  from earl_benchmark_amd import _abi
  lib = _abi.load()
  dev = lambda *a, **kw: sc.device_update(lib, *a, **kw)
  for group in range(3):
    check_crafted(dev, 65, 8, 9, group, 40 + group, 'H = 9')
    check_crafted(dev, 513, 64, 9, group, 50 + group, 'H = 9, plan is mean and std is std_in', in_place=True)
  check_crafted(dev, 65, 8, 9, 0, 44, 'H = 9, plan is mean, no std_in', std_given=False, in_place=True)


# ---------------------------------------------------------------------------------------------------------------- 2. the whole planner
def std_plan(H, n, seed):
  """a std with entries below std_min and above std_max"""
  import torch
  return torch.from_numpy(np.random.default_rng(seed).uniform(-0.1, 0.9, (H, n, 4)).astype(F32)).cuda()


def oracle(u, mean, std0, K, I, E, sigma, alpha, lo, hi, nc, iteration0=0):
  """-> (the eight outputs as host tensors, per iteration dict(act, m, s, ret, el, std)): Python candidates -> the existing rollout_branches -> sort -> Python integers"""
  import torch
  plan, n, H = mean.cpu().numpy(), u.num_envs, int(mean.shape[0])
  std = sc.std_rows(None if std0 is None else std0.cpu().numpy(), sigma, H, n)
  ret0, iters = np.empty((I, n), np.float64), []
  for i in range(I):
    s = sc.sclamp(std, lo, hi)
    act, m = sc.candidates(int(u._cfg.seed), int(u._cfg.env_offset), n, K, H, iteration0 + i, nc, plan, s)
    br = u.rollout_branches(torch.from_numpy(act).cuda())
    ret = br['ret'].cpu().numpy()
    o = sc.oracle_update(act, m, s, ret, E, alpha, lo, hi)
    plan, std = o['plan'], o['std']
    ret0[i] = ret[0]
    iters.append(dict(act=act, m=m, s=s, ret=ret, el=o['el'], std=std))
  out = dict(plan=plan, std=std, ret=ret, ret0=ret0, best_ret=o['best_ret'], best_k=o['best_k'], elite=o['elite'], fail=br['fail'].cpu().numpy())
  return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}, iters


def check(got, want, what='', keys=OUTS):
  for k in keys:
    same(got[k].cpu(), want[k].cpu(), f'{k} {what}')


@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('reward_type', ['dense', 'sparse'])
def test_plan_cem_equals_the_oracle_and_leaves_the_env_alone(kind, reward_type):
  import torch
  K, E, H, n, I = 6, 2, 6, 5, 2
  u = off_the_reset_pose(kind, n, seed=5, env_offset=3, reward_type=reward_type)
  mean = mean_plan(H, n, 2)
  before = snapshot(u, kind)
  got = u.plan_cem(mean, K=K, elites=E, iterations=I, sigma=SIGMA, alpha=0.25, std_min=LO, std_max=HI)
  unchanged(u, kind, before)
  assert {k: (tuple(v.shape), v.dtype) for k, v in got.items()} == {
      'plan': ((H, n, 4), torch.float32), 'std': ((H, n, 4), torch.float32), 'ret': ((K, n), torch.float64), 'ret0': ((I, n), torch.float64),
      'best_ret': ((n,), torch.float64), 'best_k': ((n,), torch.int32), 'elite': ((K, n), torch.uint8), 'fail': ((K, n), torch.int32)}
  want, iters = oracle(u, mean, None, K, I, E, SIGMA, 0.25, LO, HI, u.total_step_count)      # (noise_counter=None: the env's step count, 4 here)
  unchanged(u, kind, before)
  assert u.total_step_count == 4
  if reward_type == 'dense':                                              # on the oracle: the returns decide the elites, and the refit moves the std
    assert any(sorted(el) != [0, 1] for it in iters for el in it['el']), 'the elites are branches 0 and 1 everywhere: the returns never differed'
    assert bool((iters[0]['std'] != iters[0]['s']).any()) and not np.array_equal(iters[0]['std'], iters[1]['std'])
  else:
    assert all(sorted(el) == [0, 1] for el in iters[0]['el']) or bool((iters[0]['ret'] != iters[0]['ret'][:1]).any())      # equal returns: the tie goes to k = 0, 1
  check(got, want, f'{kind} {reward_type}')
  assert bool((got['plan'].abs() <= 1).all()) and bool((got['std'] >= LO).all()) and bool((got['std'] <= HI).all())
  assert bool((got['elite'].sum(0) == E).all())
  assert not np.array_equal(iters[0]['act'][1:], iters[1]['act'][1:])


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_std0_in_place_chaining_and_candidates(kind):
  import torch
  from earl_benchmark_amd import _abi
  K, E, H, n, nc = 6, 2, 6, 5, 0x9E3779B9
  u = off_the_reset_pose(kind, n, seed=7, env_offset=3, reward_type='dense')
  mean, std0 = mean_plan(H, n, 3), std_plan(H, n, 4)
  kw = dict(K=K, elites=E, sigma=SIGMA, alpha=0.1, std_min=LO, std_max=HI, noise_counter=nc)
  whole = u.plan_cem(mean, iterations=3, std=std0, **kw)
  check(whole, oracle(u, mean, std0, K, 3, E, SIGMA, 0.1, LO, HI, nc)[0], 'with std0 given')
  assert not torch.equal(whole['std'], u.plan_cem(mean, iterations=3, **kw)['std'])
  # in place: plan is mean, std is std0
  buf, sbuf = mean.clone(), std0.clone()
  res = u.plan_cem(buf, iterations=3, std=sbuf, out={'plan': buf, 'std': sbuf, 'best_k': None}, **kw)
  assert res['plan'] is buf and res['std'] is sbuf and set(res) == {'plan', 'std', 'ret'}
  same(buf, whole['plan'], 'plan of the in-place call')
  same(sbuf, whole['std'], 'std of the in-place call')
  same(res['ret'], whole['ret'], 'ret of the in-place call')
  # three iterations == three calls of one, numbered on, each fed the previous plan and std
  plan, std, ret0 = mean, std0, []
  for j in range(3):
    one = u.plan_cem(plan, iterations=1, iteration0=j, std=std, **kw)
    plan, std = one['plan'], one['std']
    ret0.append(one['ret0'])
  check(one, whole, 'of the third single call', ('plan', 'std', 'ret', 'best_ret', 'best_k', 'elite', 'fail'))
  same(torch.cat(ret0), whole['ret0'], 'ret0 of three single calls')
  # the candidates: Python == the host twin == the oracle, and what plan_cem scored
  s_np = sc.sclamp(std0.cpu().numpy(), LO, HI)
  for j in (0, 255):
    cand = u.cem_candidates(mean, K, sigma=SIGMA, std=std0, iteration=j, noise_counter=nc, std_min=LO, std_max=HI)
    want = sc.candidates(int(u._cfg.seed), 3, n, K, H, j, nc, mean.cpu().numpy(), s_np)[0]
    same(cand.cpu(), torch.from_numpy(want), f'cem_candidates of iteration {j} against the oracle')
    twin = sc.host_candidates(_abi.load_host(), sc.cfg_of(n, 3, int(u._cfg.seed)), sc.params(K, H, sigma=SIGMA, lo=LO, hi=HI, nc=nc), j, mean.cpu().numpy(), std0.cpu().numpy())
    same(cand.cpu(), torch.from_numpy(twin), f'cem_candidates of iteration {j} against the host twin')
  first = u.plan_cem(mean, iterations=1, **kw)
  cand = u.cem_candidates(mean, K, sigma=SIGMA, noise_counter=nc, std_min=LO, std_max=HI)
  same(cand.cpu(), torch.from_numpy(sc.candidates(int(u._cfg.seed), 3, n, K, H, 0, nc, mean.cpu().numpy(), sc.sclamp(sc.std_rows(None, SIGMA, H, n), LO, HI))[0]),
       'cem_candidates without a std')
  br = u.rollout_branches(cand)
  same(br['ret'], first['ret'], 'rollout_branches(cem_candidates) against ret')
  same(br['fail'], first['fail'], 'rollout_branches(cem_candidates) against fail')
  same(first['ret0'][0], first['ret'][0], 'ret0 is branch 0')


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_goal_switches_inside_the_look_ahead(kind):
  K, E, H, n, I = 5, 2, 7, 6, 2
  u = lifelong(kind, n, env_offset=3, reward_type='dense').unwrapped      # goal_change_frequency 5 < H, the clocks staggered per env
  assert 0 < int(u._cfg.goal_change_frequency) < H
  mean = mean_plan(H, n, 4)
  before = snapshot(u, kind)
  kw = dict(K=K, elites=E, iterations=I, sigma=SIGMA, noise_counter=11)
  got, again = u.plan_cem(mean, **kw), u.plan_cem(mean, **kw)
  unchanged(u, kind, before)                                              # goal_t and steps_since_goal_change among them
  check(again, got, 'of the second call (the workspace carries nothing over)')
  check(got, oracle(u, mean, None, K, I, E, SIGMA, 0.0, 0.0, 2.0, 11)[0], f'{kind} with goal switches')


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_a_poisoned_env_next_to_healthy_ones(kind):
  import torch
  K, E, H, n, bad = 5, 2, 6, 7, 5
  clean, env = make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped, make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped
  env.qvel[bad, 1] = float('nan')
  mean = mean_plan(H, n, 5)
  kw = dict(K=K, elites=E, iterations=2, sigma=SIGMA, noise_counter=3)
  want, got = clean.plan_cem(mean, **kw), env.plan_cem(mean, **kw)
  ok = [i for i in range(n) if i != bad]
  for k in ('ret', 'fail', 'plan', 'std', 'elite', 'ret0'):
    same(got[k][:, ok], want[k][:, ok], k + ' of the healthy envs')
  for k in ('best_ret', 'best_k'):
    same(got[k][ok], want[k][ok], k + ' of the healthy envs')
  assert bool((got['fail'][:, bad] == H).all()) and int(got['best_k'][bad]) == 0      # every step rolled back
  assert not bool((torch.isnan(got['ret']) & (got['elite'] != 0)).any()), 'a NaN return is never an elite'
  assert bool(torch.isfinite(got['plan']).all()) and bool((got['plan'].abs() <= 1).all()) and bool(torch.isfinite(got['std']).all())
  assert bool(torch.isnan(env.qvel[bad, 1])) and int(env.fail_count[bad]) == 0
  check(got, oracle(env, mean, None, K, 2, E, SIGMA, 0.0, 0.0, 2.0, 3)[0], 'of the poisoned batch')


def against_branches_and_the_update_twin(u, mean, K, E, nc):
  """one iteration: ret and fail == rollout_branches(cem_candidates); plan, std, ret0, best_ret, best_k and elite == the host twin of the update kernel on those returns"""
  import torch
  from earl_benchmark_amd import _abi
  H, n = int(mean.shape[0]), u.num_envs
  got = u.plan_cem(mean, K=K, elites=E, iterations=1, sigma=SIGMA, alpha=0.1, std_min=LO, std_max=HI, noise_counter=nc)
  cand = u.cem_candidates(mean, K, sigma=SIGMA, noise_counter=nc, std_min=LO, std_max=HI)
  br = u.rollout_branches(cand)
  same(got['ret'], br['ret'], 'ret')
  same(got['fail'], br['fail'], 'fail')
  twin = sc.host_update(_abi.load_host(), sc.cfg_of(n, int(u._cfg.env_offset), int(u._cfg.seed)), sc.params(K, H, E=E, sigma=SIGMA, alpha=0.1, lo=LO, hi=HI, nc=nc), 0,
                        mean.cpu().numpy(), None, cand.cpu().numpy(), br['ret'].cpu().numpy())
  for k in ('plan', 'std', 'ret0', 'best_ret', 'best_k', 'elite'):
    same((got[k][0] if k == 'ret0' else got[k]).cpu(), torch.from_numpy(twin[k]), k)
  return got


def test_the_eight_wave_door_build_above_4096_virtual_envs():
  K, H, n = 65, 6, 64
  u = make('door', n, seed=10, reward_type='dense', info='minimal').unwrapped
  before = snapshot(u, 'door')
  got = against_branches_and_the_update_twin(u, mean_plan(H, n, 6), K, 8, 21)
  unchanged(u, 'door', before)
  assert int(got['best_k'].max()) > 0


def test_the_time_sliced_peg_schedule_when_the_grid_exceeds_the_cu_count():
  import torch
  K, H, n = 65, 12, 64
  assert (K * n + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count
  u = lifelong('peg', n, seed=11, reward_type='dense').unwrapped
  before = snapshot(u, 'peg')
  against_branches_and_the_update_twin(u, mean_plan(H, n, 7), K, 8, 22)
  unchanged(u, 'peg', before)


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_two_shards_equal_the_batch(kind):
  K, E, H, n = 6, 2, 6, 5
  u = lifelong(kind, n, seed=12, reward_type='dense').unwrapped
  mean = mean_plan(H, n, 9)
  kw = dict(K=K, elites=E, iterations=2, sigma=SIGMA, alpha=0.1, noise_counter=5)
  full = u.plan_cem(mean, **kw)
  for a, b in ((0, 3), (3, 5)):
    piece = lifelong(kind, b - a, seed=12, env_offset=a, reward_type='dense').unwrapped
    piece.load_state_dict(rows_of(u.state_dict(), a, b))
    got = piece.plan_cem(mean[:, a:b].contiguous(), **kw)
    for k in OUTS:
      rows = full[k][a:b] if full[k].dim() == 1 else full[k][:, a:b]
      same(got[k], rows.contiguous(), f'{k} of envs {a}..{b}')


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_the_call_is_captured_into_a_graph_after_one_eager_call(kind):
  import torch
  K, E, H, n = 5, 2, 5, 5
  u = lifelong(kind, n, reward_type='dense').unwrapped
  mean = mean_plan(H, n, 10)
  kw = dict(K=K, elites=E, iterations=2, sigma=SIGMA, alpha=0.1, noise_counter=9)
  eager = u.plan_cem(mean, **kw)
  before = snapshot(u, kind)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    res = u.plan_cem(mean, **kw)
  for rep in range(2):
    for v in res.values():
      v.zero_()
    g.replay()
    torch.cuda.synchronize()
    check(res, eager, f'of replay {rep}')                                 # (the same noise: noise_counter is a host word of the captured call)
  unchanged(u, kind, before)


def test_the_64_lane_switch_refuses_the_call():
  from earl_benchmark_amd import _abi
  u = make('door', 4, seed=3, info='minimal').unwrapped
  lib = _abi.load()
  assert lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
  try:
    with pytest.raises(_abi.EarlHipError, match='earl_sawyer_plan_cem'):
      u.plan_cem(horizon=3, K=2, elites=1)
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK
  u.plan_cem(horizon=3, K=2, elites=1)


@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('method', ['cem', 'mppi'])
def test_mpc_rollout_is_the_loop_over_public_methods(kind, method):
  import torch
  T, K, E, H, n, I = 3, 6, 2, 5, 5, 2
  ua, ub = (off_the_reset_pose(kind, n, seed=13, env_offset=1, reward_type='dense') for _ in range(2))
  plan0 = mean_plan(H, n, 11)
  if method == 'cem':
    got = ua.mpc_rollout(T, plan=plan0, K=K, iterations=I, sigma=SIGMA, method='cem', elites=E, alpha=0.1, std_min=LO, std_max=HI)
    planner = lambda P, nc: ub.plan_cem(P, K=K, elites=E, iterations=I, sigma=SIGMA, std=None, alpha=0.1, std_min=LO, std_max=HI, noise_counter=nc)
  else:                                                                   # the default path, named: the loop of tests/test_sawyer_plan_gpu.py
    got = ua.mpc_rollout(T, plan=plan0, K=K, iterations=I, sigma=SIGMA, temperature=0.5, method='mppi')
    planner = lambda P, nc: ub.plan_mppi(P, K=K, iterations=I, sigma=SIGMA, temperature=0.5, noise_counter=nc)
  assert ua.total_step_count == 4 + T
  # the definition, written out on the second env
  P, nc0, rows = plan0.clone(), ub.total_step_count, []
  for s in range(T):
    res = planner(P, (nc0 + s) & 0xFFFFFFFF)
    P = res['plan']
    rows.append(dict(ub.rollout(P[:1]), act=P[0].clone(), ret0=res['ret0'], best_ret=res['best_ret']))
    P = torch.cat([P[1:], P[-1:]])
  assert ub.total_step_count == 4 + T
  for k in ('obs', 'reward', 'done', 'success', 'status'):
    same(got[k], torch.cat([r[k] for r in rows]), k + ' of the control loop')
  for k in ('act', 'ret0', 'best_ret'):
    same(got[k], torch.stack([r[k] for r in rows]), k + ' of the control loop')
  same(got['plan'], P, 'the plan the loop leaves')
  assert tuple(got['ret0'].shape) == (T, I, n) and bool((got['act'].abs() <= 1).all())
  assert not torch.equal(got['act'][0], got['act'][1])
  for k in ('qpos', 'qvel', 'mocap_pos', 'last_obs', 'steps_since_reset'):
    same(getattr(ua, k), getattr(ub, k), k + ' after the loop')

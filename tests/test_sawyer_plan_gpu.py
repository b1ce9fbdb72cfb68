"""The Sawyer door / peg MPPI planner on the device (include/earl_physics.h: earl_sawyer_plan_mppi, earl_sawyer_plan_candidates; env.plan_mppi, env.plan_candidates,
env.mpc_rollout).  Every case is bit for bit against a reference that uses none of the new kernels: the Python candidates of tests/sawyer_plan_helpers.py (a numpy
Philox, host-built quantile, exact fmaf), the EXISTING rollout_branches for the returns and the rolled-back step counts, and items 4 - 5 in Python integers
(tests/tabletop_plan_helpers.py: weights / update) or, where K is large, the host twin of the update kernel (held to those integers by tests/test_sawyer_plan.py).
  1. door and peg, dense and sparse, n = 5, env_offset = 3, K = 4, H = 6, two iterations, after 4 random steps: all six outputs, the env byte-equal before and after;
  2. the in-place call, three iterations == three calls of one, plan_candidates == the host twin == the oracle, rollout_branches(plan_candidates) == ret;
  3. lifelong goal switches inside the look-ahead, staggered per env;
  4. a poisoned env next to healthy ones;
  5. the eight-wave door build and the time-sliced peg schedule at the branch tests' smallest shapes, and a K wide enough for every strided loop of the update kernel;
  6. shards, capture into a graph, the 64-lane switch, mpc_rollout against the loop over public methods it is defined as."""
import numpy as np
import pytest

import sawyer_plan_helpers as sp
from tabletop_plan_helpers import update, weights
from test_physics_step_graph_gpu import make, rand_actions, same
from test_sawyer_branches_gpu import lifelong, snapshot, unchanged
from test_sawyer_population_gpu import rows_of

pytestmark = pytest.mark.gpu

OUTS = ('plan', 'ret', 'ret0', 'best_ret', 'best_k', 'fail')
SIGMA = (0.5, 0.4, 0.6, 0.8)
F32 = np.float32


def mean_plan(H, n, seed):
  """entries beyond the action box (item 1 clips them) and close to its faces (item 2 clips candidates), the gripper word included"""
  import torch
  return torch.from_numpy(np.random.default_rng(seed).uniform(-1.15, 1.15, (H, n, 4)).astype(F32)).cuda()


def oracle(u, mean, K, I, sigma, inv_t, nc, iteration0=0):
  """-> (the six outputs as host tensors, per iteration dict(act, m, ret, W)): Python candidates -> the existing rollout_branches -> weights / update in Python integers"""
  import torch
  plan, n, H = mean.cpu().numpy(), u.num_envs, int(mean.shape[0])
  ret0, iters = np.empty((I, n), np.float64), []
  for i in range(I):
    act, m, _ = sp.candidates(int(u._cfg.seed), int(u._cfg.env_offset), n, K, H, iteration0 + i, sigma, nc, plan)
    br = u.rollout_branches(torch.from_numpy(act).cuda())
    ret = br['ret'].cpu().numpy()
    W, beta, bk = weights(ret, inv_t)
    plan = update(act, m, W)
    ret0[i] = ret[0]
    iters.append(dict(act=act, m=m, ret=ret, W=W))
  out = dict(plan=plan, ret=ret, ret0=ret0, best_ret=beta, best_k=bk, fail=br['fail'].cpu().numpy())
  return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}, iters


def check(got, want, what='', keys=OUTS):
  for k in keys:
    same(got[k].cpu(), want[k].cpu(), f'{k} {what}')


def off_the_reset_pose(kind, n, **kw):
  u = make(kind, n, info='minimal', **kw).unwrapped
  u.rollout(rand_actions(4, n, 4, 1))                                     # (steps_since_reset, last_obs and total_step_count are not their initial values)
  return u


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('reward_type', ['dense', 'sparse'])
def test_plan_mppi_equals_the_oracle_and_leaves_the_env_alone(kind, reward_type):
  import torch
  K, H, n, I, temperature = 4, 6, 5, 2, 0.5
  u = off_the_reset_pose(kind, n, seed=5, env_offset=3, reward_type=reward_type)
  mean = mean_plan(H, n, 2)
  before = snapshot(u, kind)
  got = u.plan_mppi(mean, K=K, iterations=I, sigma=SIGMA, temperature=temperature)
  unchanged(u, kind, before)
  assert {k: (tuple(v.shape), v.dtype) for k, v in got.items()} == {'plan': ((H, n, 4), torch.float32), 'ret': ((K, n), torch.float64), 'ret0': ((I, n), torch.float64),
                                                                    'best_ret': ((n,), torch.float64), 'best_k': ((n,), torch.int32), 'fail': ((K, n), torch.int32)}
  want, iters = oracle(u, mean, K, I, SIGMA, 1.0 / temperature, u.total_step_count)      # (noise_counter=None: the env's step count, 4 here)
  unchanged(u, kind, before)
  assert u.total_step_count == 4
  check(got, want, f'{kind} {reward_type}')
  assert bool((got['plan'].abs() <= 1).all()) and not torch.equal(got['plan'], mean.clamp(-1, 1))
  if reward_type == 'dense':
    assert any(len(np.unique(it['W'][:, i])) > 1 for it in iters for i in range(n)), 'one weight per env everywhere: the returns never differed'
  assert not np.array_equal(iters[0]['act'][1:], iters[1]['act'][1:])


# ---------------------------------------------------------------------------------------------------------------- 2. in place, chaining, candidates
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_in_place_chaining_and_candidates(kind):
  import torch
  from earl_benchmark_amd import _abi
  K, H, n, nc = 4, 6, 5, 0x9E3779B9
  u = off_the_reset_pose(kind, n, seed=7, env_offset=3, reward_type='dense')
  mean = mean_plan(H, n, 3)
  kw = dict(K=K, sigma=SIGMA, temperature=0.5, noise_counter=nc)
  whole = u.plan_mppi(mean, iterations=3, **kw)
  # in place
  buf = mean.clone()
  res = u.plan_mppi(buf, iterations=3, out={'plan': buf, 'best_k': None}, **kw)
  assert res['plan'] is buf and set(res) == {'plan', 'ret'}
  same(buf, whole['plan'], 'the in-place call')
  same(res['ret'], whole['ret'], 'ret of the in-place call')
  # three iterations == three calls of one, numbered on
  plan, ret0 = mean, []
  for j in range(3):
    one = u.plan_mppi(plan, iterations=1, iteration0=j, **kw)
    plan = one['plan']
    ret0.append(one['ret0'])
  check(one, whole, 'of the third single call', ('plan', 'ret', 'best_ret', 'best_k', 'fail'))
  same(torch.cat(ret0), whole['ret0'], 'ret0 of three single calls')
  # the candidates: Python == the host twin == the oracle, and what plan_mppi scored
  for j in (0, 255):
    cand = u.plan_candidates(mean, K, sigma=SIGMA, iteration=j, noise_counter=nc)
    want = sp.candidates(int(u._cfg.seed), 3, n, K, H, j, SIGMA, nc, mean.cpu().numpy())[0]
    same(cand.cpu(), torch.from_numpy(want), f'plan_candidates of iteration {j} against the oracle')
    twin = sp.host_candidates(_abi.load_host(), sp.cfg_of(n, 3, int(u._cfg.seed)), sp.params(K, H, sigma=SIGMA, nc=nc), j, mean.cpu().numpy())
    same(cand.cpu(), torch.from_numpy(twin), f'plan_candidates of iteration {j} against the host twin')
  first = u.plan_mppi(mean, iterations=1, **kw)
  br = u.rollout_branches(u.plan_candidates(mean, K, sigma=SIGMA, iteration=0, noise_counter=nc))
  same(br['ret'], first['ret'], 'rollout_branches(plan_candidates) against ret')
  same(br['fail'], first['fail'], 'rollout_branches(plan_candidates) against fail')
  same(first['ret0'][0], first['ret'][0], 'ret0 is branch 0')
  pick = u.plan_candidates(mean, K, sigma=SIGMA, noise_counter=nc)[first['best_k'].long(), :, torch.arange(n, device='cuda')].permute(1, 0, 2).contiguous()
  same(u.rollout_branches(pick[None])['ret'][0], first['best_ret'], 'candidate best_k scores best_ret')


# ---------------------------------------------------------------------------------------------------------------- 3. goal switches inside the look-ahead
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_goal_switches_inside_the_look_ahead(kind):
  K, H, n, I = 3, 7, 6, 2
  u = lifelong(kind, n, env_offset=3, reward_type='dense').unwrapped      # goal_change_frequency 5 < H, the clocks staggered per env
  assert 0 < int(u._cfg.goal_change_frequency) < H
  mean = mean_plan(H, n, 4)
  before = snapshot(u, kind)
  got = u.plan_mppi(mean, K=K, iterations=I, sigma=SIGMA, temperature=0.5, noise_counter=11)
  again = u.plan_mppi(mean, K=K, iterations=I, sigma=SIGMA, temperature=0.5, noise_counter=11)
  unchanged(u, kind, before)                                              # goal_t and steps_since_goal_change among them
  check(again, got, 'of the second call (the workspace carries nothing over)')
  want, _ = oracle(u, mean, K, I, SIGMA, 2.0, 11)
  check(got, want, f'{kind} with goal switches')


# ---------------------------------------------------------------------------------------------------------------- 4. the failure guard
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_a_poisoned_env_next_to_healthy_ones(kind):
  import torch
  K, H, n, bad = 3, 6, 7, 5
  clean, env = make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped, make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped
  env.qvel[bad, 1] = float('nan')
  mean = mean_plan(H, n, 5)
  kw = dict(K=K, iterations=2, sigma=SIGMA, temperature=0.5, noise_counter=3)
  want, got = clean.plan_mppi(mean, **kw), env.plan_mppi(mean, **kw)
  ok = [i for i in range(n) if i != bad]
  for k in ('ret', 'fail', 'plan'):
    same(got[k][:, ok], want[k][:, ok], k + ' of the healthy envs')
  for k in ('best_ret', 'best_k'):
    same(got[k][ok], want[k][ok], k + ' of the healthy envs')
  same(got['ret0'][:, ok], want['ret0'][:, ok], 'ret0 of the healthy envs')
  assert bool((got['fail'][:, bad] == H).all()) and bool((got['ret'][:, bad] == 0).all()) and int(got['best_k'][bad]) == 0      # every step rolled back: reward 0, equal weights
  assert bool(torch.isfinite(got['plan']).all()) and bool((got['plan'].abs() <= 1).all())
  assert bool(torch.isnan(env.qvel[bad, 1])) and int(env.fail_count[bad]) == 0
  check(got, oracle(env, mean, K, 2, SIGMA, 2.0, 3)[0], 'of the poisoned batch')


# ---------------------------------------------------------------------------------------------------------------- 5. launch forms, wide K
def against_branches_and_the_update_twin(u, mean, K, nc, temperature=0.5):
  """one iteration: ret and fail == rollout_branches(plan_candidates); plan, ret0, best_ret and best_k == the host twin of the update kernel on those returns"""
  import torch
  from earl_benchmark_amd import _abi
  H, n = int(mean.shape[0]), u.num_envs
  got = u.plan_mppi(mean, K=K, iterations=1, sigma=SIGMA, temperature=temperature, noise_counter=nc)
  cand = u.plan_candidates(mean, K, sigma=SIGMA, noise_counter=nc)
  br = u.rollout_branches(cand)
  same(got['ret'], br['ret'], 'ret')
  same(got['fail'], br['fail'], 'fail')
  twin = sp.host_update(_abi.load_host(), sp.cfg_of(n, int(u._cfg.env_offset), int(u._cfg.seed)), sp.params(K, H, sigma=SIGMA, inv_t=1.0 / temperature, nc=nc), 0,
                        mean.cpu().numpy(), cand.cpu().numpy(), br['ret'].cpu().numpy())
  for k, name in (('plan', 'plan'), ('ret0', 'ret0'), ('best_ret', 'best_ret'), ('best_k', 'best_k')):
    same((got[k][0] if k == 'ret0' else got[k]).cpu(), torch.from_numpy(twin[name]), k)
  return got


def test_the_eight_wave_door_build_above_4096_virtual_envs():
  K, H, n = 65, 6, 64
  u = make('door', n, seed=10, reward_type='dense', info='minimal').unwrapped
  before = snapshot(u, 'door')
  against_branches_and_the_update_twin(u, mean_plan(H, n, 6), K, 21)
  unchanged(u, 'door', before)


def test_the_time_sliced_peg_schedule_when_the_grid_exceeds_the_cu_count():
  import torch
  K, H, n = 65, 12, 64
  assert (K * n + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count
  u = lifelong('peg', n, seed=11, reward_type='dense').unwrapped
  before = snapshot(u, 'peg')
  against_branches_and_the_update_twin(u, mean_plan(H, n, 7), K, 22)
  unchanged(u, 'peg', before)


def test_a_wide_K_walks_every_strided_loop_of_the_update_kernel():
  """K = 1100: three passes of the workgroup's 512 lanes over the returns and the weights and eighteen of a wave's 64 lanes over the candidates, the last pass of each
  partial; H = 11: more plan steps than the workgroup has waves"""
  K, H, n = 1100, 11, 2
  u = make('door', n, seed=12, reward_type='dense', info='minimal').unwrapped
  got = against_branches_and_the_update_twin(u, mean_plan(H, n, 8), K, 23, temperature=0.05)
  assert int(got['best_k'].max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 6. shards, capture, switches, the control loop
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_two_shards_equal_the_batch(kind):
  K, H, n = 4, 6, 5
  u = lifelong(kind, n, seed=12, reward_type='dense').unwrapped
  mean = mean_plan(H, n, 9)
  kw = dict(K=K, iterations=2, sigma=SIGMA, temperature=0.5, noise_counter=5)
  full = u.plan_mppi(mean, **kw)
  for a, b in ((0, 3), (3, 5)):
    piece = lifelong(kind, b - a, seed=12, env_offset=a, reward_type='dense').unwrapped
    piece.load_state_dict(rows_of(u.state_dict(), a, b))
    got = piece.plan_mppi(mean[:, a:b].contiguous(), **kw)
    for k in OUTS:
      rows = full[k][a:b] if full[k].dim() == 1 else full[k][:, a:b]
      same(got[k], rows.contiguous(), f'{k} of envs {a}..{b}')


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_the_call_is_captured_into_a_graph_after_one_eager_call(kind):
  import torch
  K, H, n = 3, 5, 5
  u = lifelong(kind, n, reward_type='dense').unwrapped
  mean = mean_plan(H, n, 10)
  kw = dict(K=K, iterations=2, sigma=SIGMA, temperature=0.5, noise_counter=9)
  eager = u.plan_mppi(mean, **kw)
  before = snapshot(u, kind)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    res = u.plan_mppi(mean, **kw)
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
    with pytest.raises(_abi.EarlHipError, match='earl_sawyer_plan_mppi'):
      u.plan_mppi(horizon=3, K=2)
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK
  u.plan_mppi(horizon=3, K=2)


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_mpc_rollout_is_the_loop_over_public_methods(kind):
  import torch
  T, K, H, n, I = 3, 4, 5, 5, 2
  ua, ub = (off_the_reset_pose(kind, n, seed=13, env_offset=1, reward_type='dense') for _ in range(2))
  plan0 = mean_plan(H, n, 11)
  got = ua.mpc_rollout(T, plan=plan0, K=K, iterations=I, sigma=SIGMA, temperature=0.5)
  assert ua.total_step_count == 4 + T
  # the definition, written out on the second env
  P, nc0, rows = plan0.clone(), ub.total_step_count, []
  for s in range(T):
    res = ub.plan_mppi(P, K=K, iterations=I, sigma=SIGMA, temperature=0.5, noise_counter=(nc0 + s) & 0xFFFFFFFF)
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

"""Discount and a terminal value net in the Sawyer door / peg planners on the device (include/earl_physics.h, "discount and a terminal value on the door and the peg";
env.rollout_branches / plan_mppi / plan_cem / mpc_rollout with discount= and value=).  Every case is bit for bit against a reference that uses none of the new code:
per-step rewards and the last observation come from K load_state_dict + rollout(actions[k]) calls, the discounted sum is numpy float64 in the stated order (term =
d * r; ret = ret + term; d = d * gamma), and V is earl_mlp_policy_forward_cpu on the float32 row.  gamma = 0.9: inexact in binary, so the order of operations shows.
  1. rollout_branches against the oracle: door and peg, dense and sparse, n = 5, env_offset = 3, K = 4, H = 6, after 4 random steps -- discount only, value only, both --
     every output, the env byte-equal before and after;
  2. the defaults and discount = 1.0: the value-free call bit for bit; with a network ret == plain ret + (double)V exactly;
  3. lifelong goal switches inside the look-ahead (K n = 18: the value kernel's last wave is partial); a poisoned env next to healthy ones (K n = 21): every step of it
     rolls back, contributes 0 and the terminal term is d_H V(the env's row of last_obs); without that row the return is NaN and nothing faults;
  4. the eight-wave door build and the time-sliced peg schedule at their smallest shapes, the oracle on branches 0, 31 and 64, and two shards (which run the OTHER form);
  5. plan_mppi / plan_cem: ret and fail == rollout_branches(candidates, discount=, value=), the rest == the Python-integer update (K = 4) or the update's host twin
     (K = 65); in place; I iterations == I calls; shards; capture into a graph; the 64-lane switch; mpc_rollout == its loop over public methods, both methods;
  6. the purpose: sparse door, the goal farther than H away -- without V every branch scores alike, with a hand-built distance network they differ and the plan moves.
The resource bar of the new kernels needs no GPU: tests/test_sawyer_value.py."""
import numpy as np
import pytest

import sawyer_cem_helpers as sc
import sawyer_plan_helpers as sp
from tabletop_plan_helpers import update, weights
from test_physics_step_graph_gpu import make, rand_actions, same
from test_sawyer_branches_gpu import KEYS, busy_actions, lifelong, snapshot, unchanged
from test_sawyer_plan_gpu import SIGMA, mean_plan, off_the_reset_pose
from test_sawyer_policy_rollout import forward_cpu, random_layers
from test_sawyer_population_gpu import by_definition, rows_of

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GAMMA = 0.9


class Net:
  """a value network 14 -> .. -> 1: numpy layers for the host oracle, the MLPPolicy the env takes"""

  def __init__(self, dims=(14, 64, 64, 1), hidden_act='tanh', out_act='none', seed=3, layers=None):
    import torch
    from earl_benchmark_amd.policy import MLPPolicy
    self.layers, self.hidden_act, self.out_act = layers if layers is not None else random_layers(dims, seed, gain=1.5), hidden_act, out_act
    self.policy = MLPPolicy([(torch.from_numpy(w), torch.from_numpy(b)) for w, b in self.layers], hidden_act, out_act, device='cuda', obs_dim=14, act_dim=1)

  def __call__(self, obs):
    """V [rows] float32 of float64 rows [rows, 14]: the policy contract's host statement on the float32 rounding"""
    obs = np.ascontiguousarray(obs, F64).reshape(-1, 14)
    return forward_cpu(self.layers, self.hidden_act, self.out_act, np.nan_to_num(obs.astype(F32)))[:, 0]


def reference(u, acts, gamma=1.0, net=None):
  """acts [K, H, n, 4] -> the five outputs as host tensors, each branch a restored state + rollout() + the definitions; the env ends as it started"""
  import torch
  sd = u.state_dict()
  rows = {k: [] for k in KEYS}
  for k in range(acts.shape[0]):
    u.load_state_dict(sd)
    out = u.rollout(acts[k])
    r = out['reward'].cpu().numpy()
    _, last, first = by_definition(out['reward'], out['success'])
    ret, d = np.zeros(r.shape[1], F64), F64(1.0)
    for t in range(r.shape[0]):
      term = d * r[t].astype(F64)
      ret = ret + term
      d = d * F64(gamma)
    o_H = out['obs'][-1].cpu().numpy()
    if net is not None:
      term = d * net(o_H).astype(F64)
      ret = ret + term
      ret[np.isnan(o_H).any(1)] = np.nan
    rows['ret'].append(torch.from_numpy(ret))
    rows['success'].append(torch.from_numpy(last))
    rows['first_success'].append(torch.from_numpy(first))
    rows['last_obs'].append(torch.from_numpy(o_H))
    rows['fail'].append((out['status'] != 0).sum(0).to(torch.int32).cpu())
  u.load_state_dict(sd)
  return {k: torch.stack(v) for k, v in rows.items()}


def same_ret(got, want, what):
  """float64 returns, bit for bit where they are numbers and NaN where NaN is wanted"""
  import torch
  got, want = got.cpu(), want.cpu()
  nan = torch.isnan(want)
  assert torch.equal(torch.isnan(got), nan), what + ': the NaN returns'
  same(got[~nan], want[~nan], what)


def check(got, want, what='', rows=None):
  assert set(got) == set(KEYS)
  for k in KEYS:
    g, w = got[k].cpu(), want[k].cpu()
    if rows is not None:
      g = g[rows]
    (same_ret if k == 'ret' else same)(g, w, f'{k} {what}')


VARIANTS = (('discount only', GAMMA, False), ('value only', 1.0, True), ('both', GAMMA, True))


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('reward_type', ['dense', 'sparse'])
def test_rollout_branches_equals_the_oracle_and_leaves_the_env_alone(kind, reward_type):
  K, H, n = 4, 6, 5
  u = off_the_reset_pose(kind, n, seed=5, env_offset=3, reward_type=reward_type)
  acts = busy_actions(K, H, n, 2)
  net = Net((14, 64, 64, 1), 'tanh', 'none', seed=4)
  before = snapshot(u, kind)
  got = {name: u.rollout_branches(acts, discount=g, value=net.policy if v else None) for name, g, v in VARIANTS}
  plain = u.rollout_branches(acts)
  unchanged(u, kind, before)
  for name, g, v in VARIANTS:
    want = reference(u, acts, g, net if v else None)
    check(got[name], want, f'{kind} {reward_type} {name}')
    print(name, want['ret'][:, 0].tolist())
    if reward_type == 'dense' or v:
      assert not bool((got[name]['ret'] == plain['ret']).all()), name + ': the score is the plain sum'
  unchanged(u, kind, before)


# ---------------------------------------------------------------------------------------------------------------- 2. the defaults and discount = 1
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('dims,hidden_act,out_act', [((14, 16, 1), 'relu', 'tanh'), ((14, 256, 256, 1), 'relu', 'none')], ids=['16', '256-256'])
def test_the_defaults_and_discount_one(kind, dims, hidden_act, out_act):
  import torch
  K, H, n = 3, 5, 5                                                        # K n = 15: no multiple of a wave's four virtual envs
  u = off_the_reset_pose(kind, n, seed=6, reward_type='dense')
  acts = busy_actions(K, H, n, 3)
  net = Net(dims, hidden_act, out_act, seed=5)
  plain = u.rollout_branches(acts)
  again = u.rollout_branches(acts, discount=1.0, value=None)
  for k in KEYS:
    same(again[k], plain[k], k + ' of the defaults')
  got = u.rollout_branches(acts, discount=1.0, value=net.policy)
  V = torch.from_numpy(net(plain['last_obs'].cpu().numpy()).astype(F64).reshape(K, n))
  same(got['ret'].cpu(), plain['ret'].cpu() + V, 'ret == plain ret + (double)V')
  assert len(np.unique(V.numpy())) > K                                     # (the branches and the envs differ in V)
  for k in KEYS[1:]:
    same(got[k], plain[k], k + ' with a network')


# ---------------------------------------------------------------------------------------------------------------- 3. goal switches, the failure guard
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_goal_switches_inside_the_look_ahead(kind):
  K, H, n = 3, 7, 6                                                        # K n = 18: the value kernel's second workgroup holds two virtual envs
  u = lifelong(kind, n, env_offset=3, reward_type='dense').unwrapped
  assert 0 < int(u._cfg.goal_change_frequency) < H
  acts = busy_actions(K, H, n, 4)
  net = Net((14, 32, 1), 'tanh', 'tanh', seed=6)
  before = snapshot(u, kind)
  got = u.rollout_branches(acts, discount=GAMMA, value=net.policy)
  again = u.rollout_branches(acts, discount=GAMMA, value=net.policy)
  unchanged(u, kind, before)
  for k in KEYS:
    same(got[k], again[k], k + ' of the second call (the workspace carries nothing over)')
  want = reference(u, acts, GAMMA, net)
  check(got, want, f'{kind} with goal switches')
  changed = (want['last_obs'][:, :, 7:] != before['goal_t'].cpu()[None]).any(-1)
  assert bool(changed.any()), 'no goal switch changed the goal block V reads'


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_a_poisoned_env_next_to_healthy_ones(kind):
  import torch
  K, H, n, bad = 3, 6, 7, 5                                                # K n = 21
  clean, env = make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped, make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped
  env.qvel[bad, 1] = float('nan')
  stable = env.last_obs[bad].clone()
  acts = busy_actions(K, H, n, 5)
  net = Net((14, 64, 64, 1), 'relu', 'none', seed=7)
  want, got = clean.rollout_branches(acts, discount=GAMMA, value=net.policy), env.rollout_branches(acts, discount=GAMMA, value=net.policy)
  ok = [i for i in range(n) if i != bad]
  for k in KEYS:
    same(got[k][:, ok], want[k][:, ok], k + ' of the healthy envs')
  # every step of the poisoned env is rolled back: each contributes 0, and step 0 diverging leaves the env's own row of last_obs for V
  assert bool((got['fail'][:, bad] == H).all())
  same(got['last_obs'][:, bad], stable.expand(K, 14).contiguous(), 'the carried row of the poisoned env is its row of last_obs')
  d = F64(1.0)
  for _ in range(H):
    d = d * F64(GAMMA)
  term = d * F64(net(stable.cpu().numpy())[0])
  same(got['ret'][:, bad].cpu(), torch.full((K,), float(F64(0.0) + term), dtype=torch.float64), 'ret of the poisoned env == d_H V(last_obs row)')
  check(got, reference(env, acts, GAMMA, net), 'of the poisoned batch against the oracle')
  # without the env's row of last_obs the carried row is NaN: a NaN return (with a relu network too), the neighbours as before, nothing faults
  keep = env._st.last_obs
  env._st.last_obs = None
  try:
    blind = env.rollout_branches(acts, discount=GAMMA, value=net.policy)
  finally:
    env._st.last_obs = keep
  torch.cuda.synchronize()
  assert bool(torch.isnan(blind['ret'][:, bad]).all()) and bool(torch.isnan(blind['last_obs'][:, bad]).all())
  for k in KEYS:
    same(blind[k][:, ok], want[k][:, ok], k + ' of the healthy envs next to a NaN row')
  assert bool(torch.isnan(env.qvel[bad, 1])) and int(env.fail_count[bad]) == 0


# ---------------------------------------------------------------------------------------------------------------- 4. the other two launch forms
def forms_case(u, kind, K, H, n, seed, make_piece):
  """the oracle on branches 0, 31 and 64, and two shards of 32 envs (few enough virtual envs for the OTHER launch form) against the batch"""
  acts = busy_actions(K, H, n, seed)
  net = Net((14, 64, 64, 1), 'tanh', 'none', seed=8)
  before = snapshot(u, kind)
  got = u.rollout_branches(acts, discount=GAMMA, value=net.policy)
  unchanged(u, kind, before)
  pick = [0, 31, 64]
  check(got, reference(u, acts[pick].contiguous(), GAMMA, net), f'of branches {pick}', rows=pick)
  sd = u.state_dict()
  for a, b in ((0, 32), (32, 64)):
    piece = make_piece(b - a, a)
    piece.load_state_dict(rows_of(sd, a, b))
    part = piece.rollout_branches(acts[:, :, a:b].contiguous(), discount=GAMMA, value=net.policy)
    for k in KEYS:
      same(part[k], got[k][:, a:b].contiguous(), f'{k} of envs {a}..{b}')


def test_the_eight_wave_door_build_above_4096_virtual_envs():
  K, H, n = 65, 6, 64
  u = make('door', n, seed=10, reward_type='dense', info='minimal').unwrapped
  forms_case(u, 'door', K, H, n, 6, lambda m, off: make('door', m, seed=10, env_offset=off, reward_type='dense', info='minimal').unwrapped)


def test_the_time_sliced_peg_schedule_when_the_grid_exceeds_the_cu_count():
  import torch
  K, H, n = 65, 12, 64
  assert (K * n + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count
  u = lifelong('peg', n, seed=11, reward_type='dense').unwrapped
  forms_case(u, 'peg', K, H, n, 7, lambda m, off: lifelong('peg', m, seed=11, env_offset=off, reward_type='dense').unwrapped)


# ---------------------------------------------------------------------------------------------------------------- 5. the planners
MPPI_OUTS = ('plan', 'ret', 'ret0', 'best_ret', 'best_k', 'fail')
CEM_OUTS = ('plan', 'std', 'ret', 'ret0', 'best_ret', 'best_k', 'elite', 'fail')
E, ALPHA, LO, HI = 2, 0.1, 0.05, 0.7


def plan(u, method, mean, K, **kw):
  if method == 'cem':
    return u.plan_cem(mean, K=K, elites=E, sigma=SIGMA, alpha=ALPHA, std_min=LO, std_max=HI, **kw)
  return u.plan_mppi(mean, K=K, sigma=SIGMA, temperature=0.5, **kw)


def candidates_of(u, method, mean, K, nc, j=0, std=None):
  if method == 'cem':
    return u.cem_candidates(mean, K, sigma=SIGMA, std=std, iteration=j, noise_counter=nc, std_min=LO, std_max=HI)
  return u.plan_candidates(mean, K, sigma=SIGMA, iteration=j, noise_counter=nc)


def outs_of(method):
  return CEM_OUTS if method == 'cem' else MPPI_OUTS


def check_plan(got, want, method, what, keys=None):
  for k in keys or outs_of(method):
    (same_ret if k in ('ret', 'ret0', 'best_ret') else same)(got[k].cpu(), want[k].cpu(), f'{k} {what}')


def planner_oracle(u, method, mean, K, I, nc, value_kw):
  """Python candidates -> rollout_branches(discount=, value=) (held to the old code by the cases above) -> the update in Python integers"""
  import torch
  plan_, n, H = mean.cpu().numpy(), u.num_envs, int(mean.shape[0])
  std = sc.std_rows(None, SIGMA, H, n)
  ret0 = np.empty((I, n), F64)
  for i in range(I):
    if method == 'cem':
      s = sc.sclamp(std, LO, HI)
      act, m = sc.candidates(int(u._cfg.seed), int(u._cfg.env_offset), n, K, H, i, nc, plan_, s)
    else:
      act, m, _ = sp.candidates(int(u._cfg.seed), int(u._cfg.env_offset), n, K, H, i, SIGMA, nc, plan_)
    br = u.rollout_branches(torch.from_numpy(act).cuda(), **value_kw)
    ret = br['ret'].cpu().numpy()
    ret0[i] = ret[0]
    if method == 'cem':
      o = sc.oracle_update(act, m, s, ret, E, ALPHA, LO, HI)
      plan_, std = o['plan'], o['std']
      out = dict(plan=plan_, std=std, ret=ret, ret0=ret0, best_ret=o['best_ret'], best_k=o['best_k'], elite=o['elite'], fail=br['fail'].cpu().numpy())
    else:
      W, beta, bk = weights(ret, 2.0)
      plan_ = update(act, m, W)
      out = dict(plan=plan_, ret=ret, ret0=ret0, best_ret=beta, best_k=bk, fail=br['fail'].cpu().numpy())
  return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('method', ['mppi', 'cem'])
def test_planners_equal_the_python_integer_update_in_place_and_chained(kind, method):
  import torch
  K, H, n, I, nc = 4, 6, 5, 3, 0x9E3779B9
  u = off_the_reset_pose(kind, n, seed=7, env_offset=3, reward_type='dense')
  mean = mean_plan(H, n, 3)
  net = Net((14, 64, 64, 1), 'tanh', 'none', seed=9)
  vk = dict(discount=GAMMA, value=net.policy)
  before = snapshot(u, kind)
  whole = plan(u, method, mean, K, iterations=I, noise_counter=nc, **vk)
  unchanged(u, kind, before)
  check_plan(whole, planner_oracle(u, method, mean, K, I, nc, vk), method, f'{kind} against the oracle')
  free = plan(u, method, mean, K, iterations=I, noise_counter=nc)
  assert not torch.equal(free['ret'], whole['ret']) and not torch.equal(free['plan'], whole['plan'])      # (the keywords change the scores, and with them the plan)
  # ret and fail are rollout_branches' on the candidates of the first iteration
  first = plan(u, method, mean, K, iterations=1, noise_counter=nc, **vk)
  br = u.rollout_branches(candidates_of(u, method, mean, K, nc), **vk)
  same(br['ret'], first['ret'], 'rollout_branches(candidates, discount=, value=) against ret')
  same(br['fail'], first['fail'], 'rollout_branches(candidates) against fail')
  # in place
  buf = mean.clone()
  res = plan(u, method, buf, K, iterations=I, noise_counter=nc, out={'plan': buf, 'best_k': None}, **vk)
  assert res['plan'] is buf
  same(buf, whole['plan'], 'the in-place call')
  same(res['ret'], whole['ret'], 'ret of the in-place call')
  # I iterations == I calls of one, numbered on
  p, s, ret0 = mean, None, []
  for j in range(I):
    one = plan(u, method, p, K, iterations=1, iteration0=j, noise_counter=nc, **(dict(std=s) if method == 'cem' else {}), **vk)
    p, s = one['plan'], one.get('std')
    ret0.append(one['ret0'])
  check_plan(one, whole, method, 'of the last single call', [k for k in outs_of(method) if k != 'ret0'])
  same(torch.cat(ret0), whole['ret0'], 'ret0 of the single calls')


@pytest.mark.parametrize('method', ['mppi', 'cem'])
def test_planners_at_K_65_against_the_update_twins(method):
  import torch
  from earl_benchmark_amd import _abi
  K, H, n, nc = 65, 4, 5, 21
  u = off_the_reset_pose('door', n, seed=8, env_offset=1, reward_type='dense')
  mean = mean_plan(H, n, 6)
  vk = dict(discount=GAMMA, value=Net((14, 16, 1), 'relu', 'none', seed=10).policy)
  got = plan(u, method, mean, K, iterations=1, noise_counter=nc, **vk)
  cand = candidates_of(u, method, mean, K, nc)
  br = u.rollout_branches(cand, **vk)
  same(got['ret'], br['ret'], 'ret')
  same(got['fail'], br['fail'], 'fail')
  cfg = sp.cfg_of(n, int(u._cfg.env_offset), int(u._cfg.seed))
  if method == 'cem':
    twin = sc.host_update(_abi.load_host(), cfg, sc.params(K, H, E=E, sigma=SIGMA, alpha=ALPHA, lo=LO, hi=HI, nc=nc), 0, mean.cpu().numpy(), None, cand.cpu().numpy(),
                          br['ret'].cpu().numpy())
    keys = ('plan', 'std', 'ret0', 'best_ret', 'best_k', 'elite')
  else:
    twin = sp.host_update(_abi.load_host(), cfg, sp.params(K, H, sigma=SIGMA, inv_t=2.0, nc=nc), 0, mean.cpu().numpy(), cand.cpu().numpy(), br['ret'].cpu().numpy())
    keys = ('plan', 'ret0', 'best_ret', 'best_k')
  for k in keys:
    same((got[k][0] if k == 'ret0' else got[k]).cpu(), torch.from_numpy(twin[k]), k)


@pytest.mark.parametrize('kind,method', [('door', 'mppi'), ('peg', 'cem')])
def test_two_shards_equal_the_batch_and_the_call_is_captured_into_a_graph(kind, method):
  import torch
  K, H, n = 4, 6, 5
  u = lifelong(kind, n, seed=12, reward_type='dense').unwrapped
  mean = mean_plan(H, n, 9)
  net = Net((14, 64, 64, 1), 'tanh', 'none', seed=11)
  kw = dict(iterations=2, noise_counter=5, discount=GAMMA, value=net.policy)
  full = plan(u, method, mean, K, **kw)
  for a, b in ((0, 3), (3, 5)):
    piece = lifelong(kind, b - a, seed=12, env_offset=a, reward_type='dense').unwrapped
    piece.load_state_dict(rows_of(u.state_dict(), a, b))
    got = plan(piece, method, mean[:, a:b].contiguous(), K, **kw)
    for k in outs_of(method):
      rows = full[k][a:b] if full[k].dim() == 1 else full[k][:, a:b]
      same(got[k], rows.contiguous(), f'{k} of envs {a}..{b}')
  before = snapshot(u, kind)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    res = plan(u, method, mean, K, **kw)
  for rep in range(2):
    for v in res.values():
      v.zero_()
    g.replay()
    torch.cuda.synchronize()
    check_plan(res, full, method, f'of replay {rep}')
  unchanged(u, kind, before)


def test_the_64_lane_switch_refuses_the_calls():
  from earl_benchmark_amd import _abi
  u = make('door', 4, seed=3, info='minimal').unwrapped
  net = Net((14, 16, 1), 'relu', 'none')
  lib = _abi.load()
  calls = (('earl_sawyer_branch_rollout_value', lambda: u.rollout_branches(busy_actions(2, 3, 4, 1), discount=GAMMA, value=net.policy)),
           ('earl_sawyer_plan_mppi_value', lambda: u.plan_mppi(horizon=3, K=2, discount=GAMMA, value=net.policy)),
           ('earl_sawyer_plan_cem_value', lambda: u.plan_cem(horizon=3, K=2, elites=1, discount=GAMMA, value=net.policy)))
  assert lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
  try:
    for name, fn in calls:
      with pytest.raises(_abi.EarlHipError, match=name):
        fn()
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK
  for _, fn in calls:
    fn()


@pytest.mark.parametrize('method', ['mppi', 'cem'])
def test_mpc_rollout_is_the_loop_over_public_methods(method):
  import torch
  T, K, H, n, I = 3, 4, 5, 5, 2
  ua, ub = (off_the_reset_pose('door', n, seed=13, env_offset=1, reward_type='dense') for _ in range(2))
  plan0 = mean_plan(H, n, 11)
  net = Net((14, 64, 64, 1), 'tanh', 'none', seed=12)
  vk = dict(discount=GAMMA, value=net.policy)
  mk = dict(method='cem', elites=E, alpha=ALPHA, std_min=LO, std_max=HI) if method == 'cem' else dict(temperature=0.5)
  got = ua.mpc_rollout(T, plan=plan0, K=K, iterations=I, sigma=SIGMA, **mk, **vk)
  free = off_the_reset_pose('door', n, seed=13, env_offset=1, reward_type='dense').mpc_rollout(T, plan=plan0, K=K, iterations=I, sigma=SIGMA, **mk)
  assert not torch.equal(free['ret0'], got['ret0'])                        # (the keywords reach the planner)
  P, nc0, rows = plan0.clone(), ub.total_step_count, []
  for s in range(T):
    res = plan(ub, method, P, K, iterations=I, noise_counter=(nc0 + s) & 0xFFFFFFFF, **vk)
    P = res['plan']
    rows.append(dict(ub.rollout(P[:1]), act=P[0].clone(), ret0=res['ret0'], best_ret=res['best_ret']))
    P = torch.cat([P[1:], P[-1:]])
  for k in ('obs', 'reward', 'done', 'success', 'status'):
    same(got[k], torch.cat([r[k] for r in rows]), k + ' of the control loop')
  for k in ('act', 'ret0', 'best_ret'):
    same(got[k], torch.stack([r[k] for r in rows]), k + ' of the control loop')
  same(got['plan'], P, 'the plan the loop leaves')
  for k in ('qpos', 'qvel', 'mocap_pos', 'last_obs', 'steps_since_reset'):
    same(getattr(ua, k), getattr(ub, k), k + ' after the loop')


# ---------------------------------------------------------------------------------------------------------------- 6. the purpose
def distance_net():
  """V(o) = -sum_i |o[i] - o[7 + i]|, i = 0, 1, 2: the hand against the goal's hand block.  ReLU pairs make the absolute values, the output weights are -1"""
  W0, W1 = np.zeros((16, 14), F32), np.zeros((1, 16), F32)
  for i in range(3):
    W0[2 * i, i], W0[2 * i, 7 + i] = 1.0, -1.0
    W0[2 * i + 1, i], W0[2 * i + 1, 7 + i] = -1.0, 1.0
    W1[0, 2 * i] = W1[0, 2 * i + 1] = -1.0
  return Net(layers=[(W0, np.zeros(16, F32)), (W1, np.zeros(1, F32))], hidden_act='relu', out_act='none')


def test_the_purpose_a_distance_value_net_unblinds_the_sparse_planner():
  import torch
  K, H, n, nc = 16, 5, 4, 17
  u = make('door', n, seed=14, reward_type='sparse', info='minimal').unwrapped
  mean = torch.zeros(H, n, 4, device='cuda')
  net = distance_net()
  # on the oracle first: the goal is farther than H steps away -- every candidate's rollout earns the same rewards --, while the network tells the candidates apart
  cand = u.plan_candidates(mean, K, sigma=0.5, noise_counter=nc)
  blind_want, seeing_want = reference(u, cand), reference(u, cand, 0.95, net)
  assert bool((blind_want['ret'] == blind_want['ret'][:1]).all()) and not bool(blind_want['success'].any())
  assert bool((seeing_want['ret'].max(0).values > seeing_want['ret'].min(0).values).all())
  assert bool((seeing_want['ret'].argmax(0) > 0).any())
  blind = u.plan_mppi(mean, K=K, sigma=0.5, temperature=0.01, noise_counter=nc)
  seeing = u.plan_mppi(mean, K=K, sigma=0.5, temperature=0.01, noise_counter=nc, discount=0.95, value=net.policy)
  same(blind['ret'].cpu(), blind_want['ret'], 'ret without V')
  same(seeing['ret'].cpu(), seeing_want['ret'], 'ret with V')
  assert bool((blind['ret'] == blind['ret'][:1]).all()) and bool((blind['best_k'] == 0).all())
  assert not bool((seeing['ret'] == seeing['ret'][:1]).all()) and bool((seeing['best_k'] > 0).any())
  four = u.plan_mppi(mean, K=K, iterations=4, sigma=0.5, temperature=0.01, noise_counter=nc, discount=0.95, value=net.policy)
  print('ret0 over four iterations (recorded, not asserted):', four['ret0'].cpu().numpy().tolist())

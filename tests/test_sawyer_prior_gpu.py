"""Policy-prior branches inside the Sawyer door / peg shooting planners on the device (include/earl_physics.h, "policy-prior branches on the door and the peg";
env.rollout_branches / plan_mppi / plan_cem / mpc_rollout with prior=, prior_branches=, prior_sigma=).  Every equality is bit for bit against an oracle that runs none
of the new code: a prior branch is restored state + H single-step rollout() calls whose actions are a_t = clip(fmaf(sigma, eps, forward_cpu(f32(obs_t)))) with numpy
Philox (tests/sawyer_prior_helpers.py), reduced by the definitions; the discounted sum and V as tests/test_sawyer_value_gpu.py states them.
  1. the oracle: door and peg, dense and sparse, n = 5, env_offset = 3, K = 4, P = 2, H = 6 after 4 random steps ((K - P) n = P n = 10: both launches end in a partial
     wave), sigma 0 and 0.2, with and without discount = 0.9 / value=; the env byte-equal before and after;
  2. the replay identity: the existing rollout_branches(res['actions'], ...) equals every output of all K branches;
  3. the closed-loop identity: with sigma = 0 a prior branch equals rollout_policy(policy, H) from the same state, reduced by the definitions;
  4. the defaults: prior=None / prior_branches=0 equal today's calls; gamma = 1 through the prior kernels equals the plain sum;
  5. hard rows: lifelong goal switches inside the look-ahead (the policy sees the patched goal block), a poisoned env next to healthy ones, a stale last_obs;
  6. the forms: the prior launch alone crosses into the eight-wave door build and into the time-sliced peg schedule, in both launch shapes (the prior branches inside
     ONE launch over all K n virtual envs, the default, or in a launch of their own behind the plain one: earl_debug_set_sawyer_prior_launches); two shards equal the
     batch; the two shapes give the same bits;
  7. the planners: ret / fail == rollout_branches on the reconstructed candidates, the plan (std, elite) == the Python-integer update (K = 4) or the update twins
     (K = 65), in place, I iterations == I calls, capture into a graph, mpc_rollout == its loop over public methods;
  8. the purpose: a hand-built network that moves the hand toward the handle wins the dense door's look-ahead against noise around a zero plan."""
import numpy as np
import pytest

import sawyer_cem_helpers as sc
import sawyer_plan_helpers as sp
import sawyer_prior_helpers as spr
from tabletop_plan_helpers import update, weights
from test_physics_step_graph_gpu import make, rand_actions, same
from test_sawyer_branches_gpu import KEYS, busy_actions, lifelong, snapshot, unchanged
from test_sawyer_plan_gpu import SIGMA, mean_plan, off_the_reset_pose
from test_sawyer_policy_rollout import random_layers
from test_sawyer_population_gpu import by_definition, rows_of
from test_sawyer_value_gpu import ALPHA, E, GAMMA, HI, LO, Net, candidates_of, check, check_plan, outs_of, plan, reference

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PSIGMA = (0.2, 0.1, 0.3, 0.25)


class Pol:
  """a policy 14 -> .. -> 4: numpy layers for the host oracle, the MLPPolicy the env takes.  tanh output: the rollout kernels clip x, y, z and not the gripper word,
  so only a bounded policy makes clip(u) == u, which the closed-loop identity needs"""

  def __init__(self, dims=(14, 64, 64, 4), hidden_act='tanh', out_act='tanh', seed=3, layers=None, gain=2.0):
    import torch
    from earl_benchmark_amd.policy import MLPPolicy
    self.layers, self.hidden_act, self.out_act = layers if layers is not None else random_layers(dims, seed, gain=gain), hidden_act, out_act
    self.policy = MLPPolicy([(torch.from_numpy(w), torch.from_numpy(b)) for w, b in self.layers], hidden_act, out_act, device='cuda', obs_dim=14, act_dim=4)


def prior_branch(u, pol, k, H, j, nc, sigma, obs0=None, cem=False):
  """prior branch k from the env's current state, by OLD code only: H single-step rollouts whose action is the oracle's function of the row the previous one emitted
  -> dict(act [H, n, 4], reward [H, n], success [H, n], obs [H, n, 14], status [H, n]) as host arrays; the env ends as it started"""
  import torch
  sd = u.state_dict()
  seen = (u.last_obs if obs0 is None else obs0).cpu().numpy()
  rows = dict(act=[], reward=[], success=[], obs=[], status=[])
  for t in range(H):
    a = spr.step_actions(pol.layers, pol.hidden_act, pol.out_act, seen, int(u._cfg.seed), int(u._cfg.env_offset), k, t, j, nc, sigma, cem=cem)
    out = u.rollout(torch.from_numpy(a[None]).cuda())
    seen = out['obs'][0].cpu().numpy()
    rows['act'].append(a)
    for key in ('reward', 'success', 'obs', 'status'):
      rows[key].append(out[key][0].cpu().numpy())
  u.load_state_dict(sd)
  return {k_: np.stack(v) for k_, v in rows.items()}


def reduce_branch(b, gamma=1.0, net=None):
  """the five outputs of one branch from its per-step rows: the definitions, the discounted sum in the stated order, V on the last row"""
  import torch
  r = b['reward']
  ret, d = np.zeros(r.shape[1], F64), F64(1.0)
  first = np.full(r.shape[1], -1, np.int32)
  for t in range(r.shape[0]):
    term = d * r[t].astype(F64)
    ret = ret + term
    d = d * F64(gamma)
    first = np.where((first < 0) & b['success'][t].astype(bool), t, first).astype(np.int32)
  o_H = b['obs'][-1]
  if net is not None:
    term = d * net(o_H).astype(F64)
    ret = ret + term
    ret[np.isnan(o_H).any(1)] = np.nan
  return dict(ret=torch.from_numpy(ret), success=torch.from_numpy(b['success'][-1].astype(bool)), first_success=torch.from_numpy(first), last_obs=torch.from_numpy(o_H),
              fail=torch.from_numpy((b['status'] != 0).sum(0).astype(np.int32)))


def check_prior(u, pol, got, K, P, H, j, nc, sigma, variants, pick=None, obs0=None, what=''):
  """the prior branches `pick` (default: all P) of results got[name] against the oracle; variants: {name: (gamma, net)}"""
  import torch
  for k in (range(K - P, K) if pick is None else pick):
    b = prior_branch(u, pol, k, H, j, nc, sigma, obs0=obs0)
    for name, (gamma, net) in variants.items():
      want = reduce_branch(b, gamma, net)
      same(got[name]['prior_actions'][k - (K - P)].cpu(), torch.from_numpy(b['act']), f'prior_actions of branch {k} {name} {what}')
      same(got[name]['actions'][k].cpu(), torch.from_numpy(b['act']), f'actions of branch {k} {name} {what}')
      check({key: got[name][key][k:k + 1] for key in KEYS}, {key: v[None] for key, v in want.items()}, f'of prior branch {k} {name} {what}')


# ---------------------------------------------------------------------------------------------------------------- 1. - 2. the oracle, the replay identity
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('reward_type', ['dense', 'sparse'])
def test_prior_branches_equal_the_oracle_replay_and_leave_the_env_alone(kind, reward_type):
  K, P, H, n, j, nc = 4, 2, 6, 5, 2, 0x9E3779B9
  u = off_the_reset_pose(kind, n, seed=5, env_offset=3, reward_type=reward_type)
  acts = busy_actions(K - P, H, n, 2)
  pol = Pol((14, 64, 64, 4), 'tanh', 'tanh', seed=4)
  net = Net((14, 64, 64, 1), 'tanh', 'none', seed=4)
  variants = {'plain': (1.0, None), 'both': (GAMMA, net)}
  before = snapshot(u, kind)
  for sigma in (0.0, PSIGMA):
    got = {name: u.rollout_branches(acts, prior=pol.policy, prior_branches=P, prior_sigma=sigma, noise_counter=nc, iteration=j, discount=g,
                                    value=v.policy if v else None) for name, (g, v) in variants.items()}
    unchanged(u, kind, before)
    for name, (g, v) in variants.items():
      res = got[name]
      assert set(res) == set(KEYS) | {'prior_actions', 'actions'} and tuple(res['prior_actions'].shape) == (P, H, n, 4) and tuple(res['actions'].shape) == (K, H, n, 4)
      same(res['actions'][:K - P], acts, 'the given blocks are left as they were')
      same(res['actions'][K - P:], res['prior_actions'], 'the last P blocks are the prior actions')
      # the given branches: today's call on the given blocks
      head = u.rollout_branches(acts, discount=g, value=v.policy if v else None)
      check({key: res[key][:K - P] for key in KEYS}, head, f'of the given branches {name}')
      # 2. the replay identity, through the EXISTING call
      check({key: res[key] for key in KEYS}, u.rollout_branches(res['actions'], discount=g, value=v.policy if v else None), f'of the replay {name} sigma {sigma}')
    check_prior(u, pol, got, K, P, H, j, nc, sigma, variants, what=f'{kind} {reward_type} sigma {sigma}')
    if sigma == 0.0:
      quiet = got['plain']['prior_actions'].clone()
    else:
      import torch
      assert not torch.equal(got['plain']['prior_actions'], quiet)           # (the noise reaches the actions)
      assert not torch.equal(got['plain']['prior_actions'][0], got['plain']['prior_actions'][1])      # (and is keyed by the branch)
  unchanged(u, kind, before)


# ---------------------------------------------------------------------------------------------------------------- 3. the closed-loop identity
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('dims', [(14, 16, 4), (14, 256, 256, 4)], ids=['16', '256-256'])
def test_a_quiet_prior_branch_is_rollout_policy_from_the_same_state(kind, dims):
  import torch
  K, P, H, n = 3, 2, 7, 5
  u = off_the_reset_pose(kind, n, seed=6, env_offset=1, reward_type='dense')
  pol = Pol(dims, 'relu', 'tanh', seed=5)
  got = u.rollout_branches(busy_actions(K - P, H, n, 3), prior=pol.policy, prior_branches=P, prior_sigma=0.0)
  sd = u.state_dict()
  out = u.rollout_policy(pol.policy, H)
  u.load_state_dict(sd)
  ret, last, first = by_definition(out['reward'], out['success'])
  for k in range(K - P, K):
    same(got['actions'][k], out['actions'], f'the actions of prior branch {k}')
    same(got['ret'][k].cpu(), torch.from_numpy(ret), 'ret')
    same(got['success'][k].cpu(), torch.from_numpy(last), 'success')
    same(got['first_success'][k].cpu(), torch.from_numpy(first), 'first_success')
    same(got['last_obs'][k], out['obs'][-1], 'last_obs')
    same(got['fail'][k].cpu(), (out['status'] != 0).sum(0).to(torch.int32).cpu(), 'fail')
  assert len(torch.unique(out['actions'])) > H * n                          # (the policy's actions differ over steps and envs)


# ---------------------------------------------------------------------------------------------------------------- 4. the defaults
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_no_prior_and_no_prior_branch_are_todays_calls_and_gamma_one_is_the_plain_sum(kind):
  import torch
  K, H, n, nc = 4, 5, 5, 11
  u = off_the_reset_pose(kind, n, seed=7, env_offset=2, reward_type='dense')
  pol = Pol((14, 32, 4), 'tanh', 'tanh', seed=6)
  net = Net((14, 16, 1), 'relu', 'none', seed=6)
  acts, mean = busy_actions(K, H, n, 4), mean_plan(H, n, 4)
  for vk in ({}, dict(discount=GAMMA, value=net.policy)):
    plain = u.rollout_branches(acts, **vk)
    none = u.rollout_branches(acts, prior=None, prior_branches=0, prior_sigma=0.3, **vk)
    zero = u.rollout_branches(acts, prior=pol.policy, prior_branches=0, prior_sigma=0.3, **vk)
    assert set(none) == set(KEYS) and tuple(zero['prior_actions'].shape) == (0, H, n, 4)
    same(zero['actions'], acts, 'the scored array')
    for k in KEYS:
      same(none[k], plain[k], k + ' with prior=None')
      same(zero[k], plain[k], k + ' with prior_branches=0')
    for method in ('mppi', 'cem'):
      want = plan(u, method, mean, K, iterations=2, noise_counter=nc, **vk)
      for kw in (dict(prior=None, prior_branches=0), dict(prior=pol.policy, prior_branches=0, prior_sigma=0.3)):
        got = plan(u, method, mean, K, iterations=2, noise_counter=nc, **kw, **vk)
        check_plan(got, want, method, f'{method} {sorted(kw)}')
        assert ('prior_actions' in got) == (kw['prior'] is not None)
  # gamma = 1 through the prior kernels (built with the discounted sum only) is the plain sum: the replay runs the plain kernels
  res = u.rollout_branches(acts[:2], prior=pol.policy, prior_branches=2, prior_sigma=PSIGMA, noise_counter=nc, discount=1.0)
  replay = u.rollout_branches(res['actions'])
  for k in KEYS:
    same(res[k], replay[k], k + ' at gamma = 1 against the plain kernels')
  assert bool((res['ret'][2:] != 0).any())


# ---------------------------------------------------------------------------------------------------------------- 5. hard rows
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_goal_switches_inside_the_look_ahead_reach_the_policy(kind):
  import torch
  K, P, H, n, nc = 3, 2, 7, 6, 13
  u = lifelong(kind, n, env_offset=3, reward_type='dense').unwrapped
  assert 0 < int(u._cfg.goal_change_frequency) < H
  layers = random_layers((14, 32, 4), 7, gain=2.0)
  layers[0][0][:, 7:] *= 4.0                                                # (a policy that listens to the goal block)
  pol = Pol(layers=layers, hidden_act='tanh', out_act='tanh')
  net = Net((14, 32, 1), 'tanh', 'tanh', seed=6)
  acts = busy_actions(K - P, H, n, 4)
  before = snapshot(u, kind)
  kw = dict(prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA, noise_counter=nc, discount=GAMMA, value=net.policy)
  got = u.rollout_branches(acts, **kw)
  again = u.rollout_branches(acts, **kw)
  unchanged(u, kind, before)
  for k in KEYS + ('prior_actions',):
    same(got[k], again[k], k + ' of the second call (the workspace carries nothing over)')
  check_prior(u, pol, {'both': got}, K, P, H, 0, nc, PSIGMA, {'both': (GAMMA, net)}, what=f'{kind} with goal switches')
  check({k: got[k] for k in KEYS}, u.rollout_branches(got['actions'], discount=GAMMA, value=net.policy), 'of the replay')
  # the policy saw the patched goal block: the oracle's rows change their goal inside the look-ahead, and a policy fed the OLD goal would have acted otherwise
  b = prior_branch(u, pol, K - 1, H, 0, nc, PSIGMA)
  switched = (b['obs'][:-1, :, 7:] != before['goal_t'].cpu().numpy()[None]).any(-1)      # rows that steps 1 .. H - 1 read
  assert switched.any(), 'no goal switch before the last step'
  t, i = (int(x[0]) for x in np.nonzero(switched))
  stale_row = b['obs'][t, i].copy()
  stale_row[7:] = before['goal_t'][i].cpu().numpy()
  a_stale = spr.step_actions(pol.layers, pol.hidden_act, pol.out_act, stale_row[None], int(u._cfg.seed), int(u._cfg.env_offset) + i, K - 1, t + 1, 0, nc, PSIGMA)
  assert not np.array_equal(a_stale[0], got['prior_actions'][P - 1, t + 1, i].cpu().numpy())


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_a_poisoned_env_next_to_healthy_ones(kind):
  import torch
  K, P, H, n, bad, nc = 3, 2, 6, 7, 5, 17
  clean, env = make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped, make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped
  env.qvel[bad, 1] = float('nan')
  stable = env.last_obs[bad].clone()
  pol = Pol((14, 64, 64, 4), 'relu', 'tanh', seed=8)
  acts = busy_actions(K - P, H, n, 5)
  kw = dict(prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA, noise_counter=nc)
  want, got = clean.rollout_branches(acts, **kw), env.rollout_branches(acts, **kw)
  torch.cuda.synchronize()
  ok = [i for i in range(n) if i != bad]
  for k in KEYS:
    same(got[k][:, ok], want[k][:, ok], k + ' of the healthy envs')
  same(got['prior_actions'][:, :, ok], want['prior_actions'][:, :, ok], 'prior_actions of the healthy envs')
  # every step of the poisoned env rolls back: the carried row stays the env's row of last_obs, and that is what the policy sees at every step
  assert bool((got['fail'][:, bad] == H).all()) and bool((got['ret'][:, bad] == 0).all())
  same(got['last_obs'][:, bad], stable.expand(K, 14).contiguous(), 'the carried row of the poisoned env is its row of last_obs')
  for k in range(K - P, K):
    for t in range(H):
      a = spr.step_actions(pol.layers, pol.hidden_act, pol.out_act, stable.cpu().numpy()[None], int(env._cfg.seed), int(env._cfg.env_offset) + bad, k, t, 0, nc, PSIGMA)
      same(got['prior_actions'][k - (K - P), t, bad].cpu(), torch.from_numpy(a[0]), f'the action of the poisoned env, branch {k} step {t}')
  check_prior(env, pol, {'plain': got}, K, P, H, 0, nc, PSIGMA, {'plain': (1.0, None)}, what='of the poisoned batch')
  assert bool(torch.isnan(env.qvel[bad, 1])) and int(env.fail_count[bad]) == 0


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_a_stale_last_obs_gives_the_fresh_observation_to_step_zero(kind):
  import torch
  K, P, H, n, nc = 3, 1, 3, 5, 19
  u = off_the_reset_pose(kind, n, seed=10, env_offset=1, reward_type='dense')
  pol = Pol((14, 32, 4), 'tanh', 'tanh', seed=9)
  acts = busy_actions(K - P, H, n, 6)
  fresh = u._get_obs_t().clone()
  want = u.rollout_branches(acts, prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA, noise_counter=nc)
  goal = u.goal_t.clone()
  goal[:, 4:] += 0.01
  u.reset_goal(goal)                                                       # (last_obs carries the old goal entries: stale)
  assert u._last_obs_stale
  fresh = u._get_obs_t().clone()
  assert not torch.equal(fresh, u.last_obs)
  got = u.rollout_branches(acts, prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA, noise_counter=nc)
  assert u._last_obs_stale
  a0 = spr.step_actions(pol.layers, pol.hidden_act, pol.out_act, fresh.cpu().numpy(), int(u._cfg.seed), int(u._cfg.env_offset), K - 1, 0, 0, nc, PSIGMA)
  same(got['prior_actions'][0, 0].cpu(), torch.from_numpy(a0), 'step 0 acts on the fresh observation')
  a_old = spr.step_actions(pol.layers, pol.hidden_act, pol.out_act, u.last_obs.cpu().numpy(), int(u._cfg.seed), int(u._cfg.env_offset), K - 1, 0, 0, nc, PSIGMA)
  assert not np.array_equal(a_old, a0) and not torch.equal(got['prior_actions'], want['prior_actions'])
  check_prior(u, pol, {'plain': got}, K, P, H, 0, nc, PSIGMA, {'plain': (1.0, None)}, obs0=fresh, what='with a stale last_obs')


# ---------------------------------------------------------------------------------------------------------------- 6. the other two launch forms
def forms_case(u, kind, K, P, H, n, seed, make_piece):
  """the oracle on the first, a middle and the last prior branch, the replay identity over all K, and two shards of 32 envs (few enough virtual envs for the OTHER
  launch form) against the batch"""
  acts = busy_actions(K - P, H, n, seed)
  pol = Pol((14, 64, 64, 4), 'tanh', 'tanh', seed=8)
  nc = 23
  kw = dict(prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA, noise_counter=nc, discount=GAMMA)
  before = snapshot(u, kind)
  got = u.rollout_branches(acts, **kw)
  unchanged(u, kind, before)
  check_prior(u, pol, {'disc': got}, K, P, H, 0, nc, PSIGMA, {'disc': (GAMMA, None)}, pick=[K - P, K - P + P // 2, K - 1])
  check({k: got[k] for k in KEYS}, u.rollout_branches(got['actions'], discount=GAMMA), 'of the replay')
  sd = u.state_dict()
  for a, b in ((0, 32), (32, 64)):
    piece = make_piece(b - a, a)
    piece.load_state_dict(rows_of(sd, a, b))
    part = piece.rollout_branches(acts[:, :, a:b].contiguous(), **kw)
    for k in KEYS:
      same(part[k], got[k][:, a:b].contiguous(), f'{k} of envs {a}..{b}')
    same(part['prior_actions'], got['prior_actions'][:, :, a:b].contiguous(), f'prior_actions of envs {a}..{b}')


class launches:
  """the launch shape of the prior branches for the block: 1 = inside ONE launch over all K n virtual envs (the default), 2 = a launch of their own over the last P n"""

  def __init__(self, count):
    from earl_benchmark_amd import _abi
    self.lib, self.count = _abi.load(), count

  def __enter__(self):
    assert self.lib.earl_debug_set_sawyer_prior_launches(self.count) == 0

  def __exit__(self, *exc):
    assert self.lib.earl_debug_set_sawyer_prior_launches(1) == 0


@pytest.mark.parametrize('shape', [1, 2], ids=['one-launch', 'two-launches'])
def test_the_prior_launch_alone_crosses_into_the_eight_wave_door_build(shape):
  K, P, H, n = 67, 65, 2, 64                                               # P n = 4160 > 4096 virtual envs; the given branches' launch has 128
  u = make('door', n, seed=10, reward_type='dense', info='minimal').unwrapped
  with launches(shape):
    forms_case(u, 'door', K, P, H, n, 6, lambda m, off: make('door', m, seed=10, env_offset=off, reward_type='dense', info='minimal').unwrapped)


@pytest.mark.parametrize('shape', [1, 2], ids=['one-launch', 'two-launches'])
def test_the_prior_launch_alone_crosses_into_the_time_sliced_peg_schedule(shape):
  import torch
  K, P, H, n = 67, 65, 12, 64                                              # 260 workgroups of 16 virtual envs, twelve steps > the ten-step slice
  assert (P * n + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count >= ((K - P) * n + 15) // 16
  u = lifelong('peg', n, seed=11, reward_type='dense').unwrapped           # (the goal row, its counter, the carried row and the summary words travel across the slices)
  with launches(shape):
    forms_case(u, 'peg', K, P, H, n, 7, lambda m, off: lifelong('peg', m, seed=11, env_offset=off, reward_type='dense').unwrapped)


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_the_two_launch_shapes_give_the_same_bits(kind):
  """small (both of the second shape's launches end in a partial wave) and with goal switches; discounted with a network, and the planner on top"""
  K, P, H, n, nc = 5, 2, 7, 5, 29
  u = lifelong(kind, n, seed=12, env_offset=2, reward_type='dense').unwrapped
  pol = Pol((14, 64, 64, 4), 'tanh', 'tanh', seed=13)
  net = Net((14, 32, 1), 'tanh', 'none', seed=13)
  acts, mean = busy_actions(K - P, H, n, 8), mean_plan(H, n, 8)
  kw = dict(prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA, noise_counter=nc)
  got = {}
  for shape in (1, 2):
    with launches(shape):
      got[shape] = (u.rollout_branches(acts, **kw), u.rollout_branches(acts, discount=GAMMA, value=net.policy, **kw),
                    plan(u, 'mppi', mean, K, iterations=2, **kw), plan(u, 'cem', mean, K, iterations=2, discount=GAMMA, **kw))
  for one, two in zip(got[1], got[2]):
    assert set(one) == set(two)
    for k in one:
      same(one[k], two[k], f'{k} of the two launch shapes')
  from earl_benchmark_amd import _abi
  assert _abi.load().earl_debug_set_sawyer_prior_launches(0) != 0 and _abi.load().earl_debug_set_sawyer_prior_launches(3) != 0


# ---------------------------------------------------------------------------------------------------------------- 7. the planners
def with_tail(cand, prior_actions):
  import torch
  P = int(prior_actions.shape[0])
  return torch.cat([cand[:cand.shape[0] - P], prior_actions]).contiguous()


def planner_step(u, method, mean, std, K, j, nc, res, vk):
  """one iteration by old code on the reconstructed candidates: numpy candidates with the tail replaced by res['prior_actions'] -> the existing rollout_branches -> the
  update in Python integers -> dict of host arrays"""
  import torch
  n, H = u.num_envs, int(mean.shape[0])
  if method == 'cem':
    s = sc.sclamp(std, LO, HI)
    act, m = sc.candidates(int(u._cfg.seed), int(u._cfg.env_offset), n, K, H, j, nc, mean, s)
  else:
    act, m, _ = sp.candidates(int(u._cfg.seed), int(u._cfg.env_offset), n, K, H, j, SIGMA, nc, mean)
  pa = res['prior_actions'].cpu().numpy()
  act[K - pa.shape[0]:] = pa
  br = u.rollout_branches(torch.from_numpy(act).cuda(), **vk)
  ret = br['ret'].cpu().numpy()
  if method == 'cem':
    o = sc.oracle_update(act, m, s, ret, E, ALPHA, LO, HI)
    return dict(plan=o['plan'], std=o['std'], ret=ret, ret0=ret[0], best_ret=o['best_ret'], best_k=o['best_k'], elite=o['elite'], fail=br['fail'].cpu().numpy())
  W, beta, bk = weights(ret, 2.0)
  return dict(plan=update(act, m, W), ret=ret, ret0=ret[0], best_ret=beta, best_k=bk, fail=br['fail'].cpu().numpy())


@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('method', ['mppi', 'cem'])
def test_planners_with_a_prior_equal_the_python_integer_update_in_place_and_chained(kind, method):
  import torch
  K, P, H, n, I, nc = 4, 2, 6, 5, 3, 0x9E3779B9
  u = off_the_reset_pose(kind, n, seed=7, env_offset=3, reward_type='dense')
  mean = mean_plan(H, n, 3)
  pol = Pol((14, 64, 64, 4), 'tanh', 'tanh', seed=9)
  net = Net((14, 64, 64, 1), 'tanh', 'none', seed=9)
  vk = dict(discount=GAMMA, value=net.policy)
  pk = dict(prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA)
  before = snapshot(u, kind)
  whole = plan(u, method, mean, K, iterations=I, noise_counter=nc, **pk, **vk)
  unchanged(u, kind, before)
  free = plan(u, method, mean, K, iterations=I, noise_counter=nc, **vk)
  assert not torch.equal(free['ret'], whole['ret']) and not torch.equal(free['plan'], whole['plan'])      # (the prior changes the scores, and with them the plan)
  # I iterations == I calls of one, numbered on; each single call against old code on its reconstructed candidates
  p, s, ret0 = mean, None, []
  for j in range(I):
    one = plan(u, method, p, K, iterations=1, iteration0=j, noise_counter=nc, **(dict(std=s) if method == 'cem' else {}), **pk, **vk)
    # the prior branches of this iteration against the oracle (MPPI's or CEM's draw word, this iteration's j)
    b = prior_branch(u, pol, K - 1, H, j, nc, PSIGMA, cem=method == 'cem')
    same(one['prior_actions'][P - 1].cpu(), torch.from_numpy(b['act']), f'prior_actions of iteration {j} against the oracle')
    want = planner_step(u, method, p.cpu().numpy(), sc.std_rows(None if s is None else s.cpu().numpy(), SIGMA, H, n), K, j, nc, one, vk)
    for k in outs_of(method):
      g = one[k][0] if k == 'ret0' else one[k]
      same(g.cpu(), torch.from_numpy(np.ascontiguousarray(want[k])), f'{k} of iteration {j} against old code on the reconstructed candidates')
    cand = with_tail(candidates_of(u, method, p, K, nc, j, std=s), one['prior_actions'])
    br = u.rollout_branches(cand, **vk)
    same(br['ret'], one['ret'], 'rollout_branches(reconstructed candidates) against ret')
    same(br['fail'], one['fail'], 'rollout_branches(reconstructed candidates) against fail')
    p, s = one['plan'], one.get('std')
    ret0.append(one['ret0'])
  check_plan(one, whole, method, 'of the last single call', [k for k in outs_of(method) if k != 'ret0'])
  same(one['prior_actions'], whole['prior_actions'], 'prior_actions are the last iteration\'s')
  same(torch.cat(ret0), whole['ret0'], 'ret0 of the single calls')
  # in place
  buf = mean.clone()
  res = plan(u, method, buf, K, iterations=I, noise_counter=nc, out={'plan': buf, 'best_k': None}, **pk, **vk)
  assert res['plan'] is buf
  same(buf, whole['plan'], 'the in-place call')
  same(res['ret'], whole['ret'], 'ret of the in-place call')
  same(res['prior_actions'], whole['prior_actions'], 'prior_actions of the in-place call')
  unchanged(u, kind, before)


@pytest.mark.parametrize('method', ['mppi', 'cem'])
def test_planners_with_a_prior_at_K_65_against_the_update_twins(method):
  import torch
  from earl_benchmark_amd import _abi
  K, P, H, n, nc = 65, 8, 4, 5, 21
  u = off_the_reset_pose('door', n, seed=8, env_offset=1, reward_type='dense')
  mean = mean_plan(H, n, 6)
  pol = Pol((14, 16, 4), 'relu', 'tanh', seed=10)
  pk = dict(prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA)
  got = plan(u, method, mean, K, iterations=1, noise_counter=nc, **pk)
  cand = with_tail(candidates_of(u, method, mean, K, nc), got['prior_actions'])
  br = u.rollout_branches(cand)
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
  for k in (K - P, K - 1):
    b = prior_branch(u, pol, k, H, 0, nc, PSIGMA, cem=method == 'cem')
    same(got['prior_actions'][k - (K - P)].cpu(), torch.from_numpy(b['act']), f'prior_actions of branch {k}')


@pytest.mark.parametrize('kind,method', [('door', 'mppi'), ('peg', 'cem')])
def test_two_shards_equal_the_batch_and_the_call_is_captured_into_a_graph(kind, method):
  import torch
  K, P, H, n = 4, 2, 6, 5
  u = lifelong(kind, n, seed=12, reward_type='dense').unwrapped
  mean = mean_plan(H, n, 9)
  pol = Pol((14, 64, 64, 4), 'tanh', 'tanh', seed=11)
  kw = dict(iterations=2, noise_counter=5, discount=GAMMA, prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA)
  full = plan(u, method, mean, K, **kw)
  keys = outs_of(method) + ('prior_actions',)
  for a, b in ((0, 3), (3, 5)):
    piece = lifelong(kind, b - a, seed=12, env_offset=a, reward_type='dense').unwrapped
    piece.load_state_dict(rows_of(u.state_dict(), a, b))
    got = plan(piece, method, mean[:, a:b].contiguous(), K, **kw)
    for k in keys:
      rows = full[k][a:b] if full[k].dim() == 1 else (full[k][:, :, a:b] if k == 'prior_actions' else full[k][:, a:b])
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
    same(res['prior_actions'], full['prior_actions'], f'prior_actions of replay {rep}')
  unchanged(u, kind, before)


def test_the_64_lane_switch_refuses_the_calls():
  from earl_benchmark_amd import _abi
  u = make('door', 4, seed=3, info='minimal').unwrapped
  pol = Pol((14, 16, 4), 'relu', 'tanh')
  pk = dict(prior=pol.policy, prior_branches=1)
  lib = _abi.load()
  calls = (('earl_sawyer_branch_rollout_prior', lambda: u.rollout_branches(busy_actions(2, 3, 4, 1), **pk)),
           ('earl_sawyer_plan_mppi_prior', lambda: u.plan_mppi(horizon=3, K=3, **pk)),
           ('earl_sawyer_plan_cem_prior', lambda: u.plan_cem(horizon=3, K=3, elites=1, **pk)))
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
def test_mpc_rollout_with_a_prior_is_the_loop_over_public_methods(method):
  import torch
  T, K, P, H, n, I = 3, 4, 2, 5, 5, 2
  ua, ub = (off_the_reset_pose('door', n, seed=13, env_offset=1, reward_type='dense') for _ in range(2))
  plan0 = mean_plan(H, n, 11)
  pol = Pol((14, 64, 64, 4), 'tanh', 'tanh', seed=12)
  pk = dict(prior=pol.policy, prior_branches=P, prior_sigma=PSIGMA)
  mk = dict(method='cem', elites=E, alpha=ALPHA, std_min=LO, std_max=HI) if method == 'cem' else dict(temperature=0.5)
  got = ua.mpc_rollout(T, plan=plan0, K=K, iterations=I, sigma=SIGMA, **mk, **pk)
  free = off_the_reset_pose('door', n, seed=13, env_offset=1, reward_type='dense').mpc_rollout(T, plan=plan0, K=K, iterations=I, sigma=SIGMA, **mk)
  assert not torch.equal(free['best_ret'], got['best_ret'])                # (the keywords reach the planner)
  Pl, nc0, rows = plan0.clone(), ub.total_step_count, []
  for s in range(T):
    res = plan(ub, method, Pl, K, iterations=I, noise_counter=(nc0 + s) & 0xFFFFFFFF, **pk)
    Pl = res['plan']
    rows.append(dict(ub.rollout(Pl[:1]), act=Pl[0].clone(), ret0=res['ret0'], best_ret=res['best_ret']))
    Pl = torch.cat([Pl[1:], Pl[-1:]])
  for k in ('obs', 'reward', 'done', 'success', 'status'):
    same(got[k], torch.cat([r[k] for r in rows]), k + ' of the control loop')
  for k in ('act', 'ret0', 'best_ret'):
    same(got[k], torch.stack([r[k] for r in rows]), k + ' of the control loop')
  same(got['plan'], Pl, 'the plan the loop leaves')
  for k in ('qpos', 'qvel', 'mocap_pos', 'last_obs', 'steps_since_reset'):
    same(getattr(ua, k), getattr(ub, k), k + ' after the loop')


# ---------------------------------------------------------------------------------------------------------------- 8. the purpose
def reach_net(gain=20.0):
  """u_i = tanh(gain * (o[4 + i] - o[i])), i = 0, 1, 2: the hand toward the handle; the gripper word 0.  ReLU pairs make the signed difference"""
  W0, W1 = np.zeros((16, 14), F32), np.zeros((4, 16), F32)
  for i in range(3):
    W0[2 * i, 4 + i], W0[2 * i, i] = 1.0, -1.0
    W0[2 * i + 1, 4 + i], W0[2 * i + 1, i] = -1.0, 1.0
    W1[i, 2 * i], W1[i, 2 * i + 1] = gain, -gain
  return Pol(layers=[(W0, np.zeros(16, F32)), (W1, np.zeros(4, F32))], hidden_act='relu', out_act='tanh')


def test_the_purpose_a_reaching_prior_wins_the_dense_door_look_ahead():
  import torch
  K, P, H, n, nc = 8, 2, 6, 4, 17
  u = make('door', n, seed=14, reward_type='dense', info='minimal').unwrapped
  pol = reach_net()
  mean = torch.zeros(H, n, 4, device='cuda')
  # with OLD code only: from this state the policy's H-step return strictly exceeds the zero plan's in every env
  sd = u.state_dict()
  ret_policy = by_definition(*(lambda o: (o['reward'], o['success']))(u.rollout_policy(pol.policy, H)))[0]
  u.load_state_dict(sd)
  ret_zero = by_definition(*(lambda o: (o['reward'], o['success']))(u.rollout(mean)))[0]
  u.load_state_dict(sd)
  print('H-step returns, policy against zeros:', ret_policy.tolist(), ret_zero.tolist())
  assert (ret_policy > ret_zero).all()
  res = u.plan_mppi(mean, K=K, sigma=0.02, temperature=0.01, noise_counter=nc, prior=pol.policy, prior_branches=P, prior_sigma=0.0)
  print('ret', res['ret'].cpu().numpy().tolist(), 'best_k', res['best_k'].tolist())
  assert bool((res['best_k'] >= K - P).all())
  assert bool((res['best_ret'] > res['ret0'][0]).all())
  a0 = res['prior_actions'][res['best_k'].long() - (K - P), 0, torch.arange(n, device='cuda')]      # [n, 4]: the winning prior branch's first action
  d_plan, d_zero = (res['plan'][0] - a0).norm(dim=-1), (mean[0] - a0).norm(dim=-1)
  print('distance of the first plan row to the prior\'s first action, after and before:', d_plan.tolist(), d_zero.tolist())
  assert bool((d_plan < d_zero).all())

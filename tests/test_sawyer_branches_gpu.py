"""The Sawyer door / peg branch launch on the device (include/earl_physics.h: earl_sawyer_branch_rollout; env.rollout_branches).  Every case is bit for bit against a
reference that uses none of the new code: for each branch k the state is restored, the public env runs rollout(actions[k]) (earl_sawyer_rollout), and the summary is
worked out by definition on the host (by_definition of tests/test_sawyer_population_gpu.py); the guard count is the sum of the status rows.
  1. door and peg, dense and sparse, n = 5 (no multiple of a wave's four envs: waves straddle branches and hold dead groups), K = 3, H = 7, env_offset = 3: all five
     outputs, and the env byte-equal before and after;
  2. K = 1 == rollout on a copy; stride 0 == K copies of one block;
  3. lifelong goal switches inside the look-ahead, staggered per env; st->goal untouched; a second call returns the same bits;
  4. the failure guard next to a poisoned env;
  5. the eight-wave door build and the time-sliced peg schedule, at the smallest shapes that reach them;
  6. the clock words; shards; capture into a graph; the 64-lane switch; the envs without a branch launch."""
import numpy as np
import pytest

from test_physics_step_graph_gpu import STATE, make, rand_actions, same
from test_sawyer_population_gpu import by_definition, rows_of, same_np

pytestmark = pytest.mark.gpu

KEYS = ('ret', 'success', 'first_success', 'last_obs', 'fail')
RAW = {'door': STATE['door'] + ('interventions', 'obj_init'), 'peg': STATE['peg'] + ('interventions',)}


def snapshot(u, kind):
  return {k: getattr(u, k).clone() for k in RAW[kind]} | {'counter': int(u._cfg.counter), 'step_counter': int(u._cfg.step_counter), 'total': u.total_step_count,
                                                           'stale': u._last_obs_stale}


def unchanged(u, kind, before):
  for k in RAW[kind]:
    same(getattr(u, k), before[k], k + ' of the env after the branch launch')
  assert (int(u._cfg.counter), u.total_step_count, u._last_obs_stale) == (before['counter'], before['total'], before['stale'])


def reference(u, acts):
  """acts [K, H, n, 4] -> the five outputs, each branch a restored state + rollout() + the definitions; the env ends as it started"""
  import torch
  sd = u.state_dict()
  rows = {k: [] for k in KEYS}
  for k in range(acts.shape[0]):
    u.load_state_dict(sd)
    out = u.rollout(acts[k])
    ret, last, first = by_definition(out['reward'], out['success'])
    rows['ret'].append(torch.from_numpy(ret))
    rows['success'].append(torch.from_numpy(last))
    rows['first_success'].append(torch.from_numpy(first))
    rows['last_obs'].append(out['obs'][-1].clone().cpu())
    rows['fail'].append((out['status'] != 0).sum(0).to(torch.int32).cpu())
  u.load_state_dict(sd)
  return {k: torch.stack(v) for k, v in rows.items()}


def check(got, want, cols=None, what=''):
  assert set(got) == set(KEYS)
  for k in KEYS:
    g, w = got[k].cpu(), want[k]
    if cols is not None:
      g, w = g[:, cols], w[:, cols]
    same(g, w, f'{k} {what}')


def busy_actions(K, H, n, seed):
  """uniform in [-1, 1]^4, the gripper closing in some branches and opening in others"""
  a = rand_actions(K * H, n, 4, seed).reshape(K, H, n, 4).contiguous()
  a[::2, :, :, 3] = a[::2, :, :, 3].abs()
  return a


# ---------------------------------------------------------------------------------------------------------------- 1. branches == restored rollouts
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('reward_type', ['dense', 'sparse'])
def test_branches_equal_restored_rollouts_and_leave_the_env_alone(kind, reward_type):
  K, H, n = 3, 7, 5
  env = make(kind, n, seed=5, env_offset=3, reward_type=reward_type, info='minimal')
  u = env.unwrapped
  u.rollout(rand_actions(4, n, 4, 1))                                     # (off the reset pose: steps_since_reset, last_obs and total_step_count are not their initial values)
  acts = busy_actions(K, H, n, 2)
  before = snapshot(u, kind)
  sd = u.state_dict()
  got = u.rollout_branches(acts)
  assert [tuple(got[k].shape) for k in KEYS] == [(K, n), (K, n), (K, n), (K, n, 14), (K, n)]
  unchanged(u, kind, before)
  after = u.state_dict()
  assert set(after) == set(sd)
  for k, v in sd.items():
    if hasattr(v, 'shape'):
      same(after[k], v, 'state_dict ' + k)
    else:
      assert after[k] == v, k
  want = reference(u, acts)
  check(got, want)
  if reward_type == 'dense':
    assert len(np.unique(want['ret'].numpy())) > n                         # (the branches differ: K n different returns would be 15)
  assert int(want['fail'].sum()) == 0 or int(want['fail'].max()) < H       # (a healthy env: the guard case is below)


# ---------------------------------------------------------------------------------------------------------------- 2. K = 1, stride 0
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_one_branch_is_a_rollout_on_a_copy_and_stride_zero_replays_one_block(kind):
  import torch
  H, n = 6, 5
  ea, eb = make(kind, n, seed=8, reward_type='dense', info='minimal'), make(kind, n, seed=8, reward_type='dense', info='minimal')
  ua, ub = ea.unwrapped, eb.unwrapped
  acts = busy_actions(1, H, n, 3)
  got = ua.rollout_branches(acts)
  out = ub.rollout(acts[0])                                               # the copy moves, the env does not
  ret, last, first = by_definition(out['reward'], out['success'])
  same_np(got['ret'][0], ret, 'ret')
  same_np(got['success'][0], last, 'success')
  same_np(got['first_success'][0], first, 'first_success')
  same(got['last_obs'][0], out['obs'][-1], 'last_obs')
  same(got['fail'][0], (out['status'] != 0).sum(0).to(torch.int32), 'fail')
  # one [H, n, 4] block replayed by K = 4 branches == the block given four times == four equal rows
  rep = ua.rollout_branches(acts[0], K=4)
  full = ua.rollout_branches(acts.expand(4, H, n, 4).contiguous())
  for k in KEYS:
    same(rep[k], full[k], k + ' of the stride-0 call')
    same(rep[k], got[k].expand_as(rep[k]).contiguous(), k + ' of each replayed branch')


# ---------------------------------------------------------------------------------------------------------------- 3. goal switches inside the look-ahead
def lifelong(kind, n, seed=6, **kw):
  """an env under LifelongWrapper(5) whose switches show in the goal block: the peg draws from its fifteen goal rows, the door's one-row table replaces a custom goal;
  the per-env clocks are staggered"""
  import torch
  env = make(kind, n, seed=seed, gcf=5, info='minimal', **({'reset_at_goal': True} if kind == 'peg' else {}), **kw)
  u = env.unwrapped
  u.rollout(torch.zeros(2, n, 4, device='cuda'))
  if kind == 'door':
    custom = u.goal_t[0].clone()
    custom[:3] += 0.05
    custom[4:] -= 0.03
    u.reset_goal(custom)
    u.last_obs.copy_(u._get_obs_t())
    u._last_obs_stale = False
  u.steps_since_goal_change.copy_((torch.arange(n, device='cuda') % 5).to(torch.int32))
  return env


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_goal_switches_inside_the_look_ahead(kind):
  K, H, n = 3, 7, 6
  u = lifelong(kind, n, env_offset=3).unwrapped
  acts = busy_actions(K, H, n, 4)
  before = snapshot(u, kind)
  got = u.rollout_branches(acts)
  again = u.rollout_branches(acts)
  unchanged(u, kind, before)                                              # goal_t and steps_since_goal_change among them
  for k in KEYS:
    same(got[k], again[k], k + ' of the second call (the workspace carries nothing over)')
  want = reference(u, acts)
  check(got, want)
  goal0 = before['goal_t'].cpu()
  changed = (want['last_obs'][:, :, 7:] != goal0[None]).any(-1)
  assert bool(changed.any()), 'no goal switch changed the goal block inside the look-ahead'
  if kind == 'door':
    assert bool(changed.all())                                            # (H = 7 > 5: every env's clock runs out once, and the table's row is not the custom goal)
  same(got['last_obs'][0, :, 7:], got['last_obs'][1, :, 7:], 'every branch of an env sees the env\'s own goal draws')


# ---------------------------------------------------------------------------------------------------------------- 4. the failure guard
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_branches_next_to_a_poisoned_env(kind):
  import torch
  K, H, n, bad = 3, 6, 7, 5
  clean, env = make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped, make(kind, n, seed=9, env_offset=2, info='minimal').unwrapped
  env.qvel[bad, 1] = float('nan')
  stable = env.last_obs[bad].clone()
  acts = busy_actions(K, H, n, 5)
  want = clean.rollout_branches(acts)
  got = env.rollout_branches(acts)
  ok = [i for i in range(n) if i != bad]
  for k in KEYS:
    same(got[k][:, ok], want[k][:, ok], k + ' of the healthy envs')
  assert bool((got['fail'][:, bad] == H).all()) and bool((got['ret'][:, bad] == 0).all()) and bool((got['first_success'][:, bad] == -1).all())
  assert not bool(got['success'][:, bad].any())
  same(got['last_obs'][:, bad], stable.expand(K, 14).contiguous(), 'the carried row of the poisoned env is its row of last_obs')
  assert bool(torch.isnan(env.qvel[bad, 1])) and int(env.fail_count[bad]) == 0
  check(want, reference(clean, acts), what='of the unpoisoned run')


# ---------------------------------------------------------------------------------------------------------------- 5. the other two launch forms
def test_the_eight_wave_door_build_above_4096_virtual_envs():
  K, H, n = 65, 6, 64                                                     # 4160 virtual envs; every reference launch has 64
  u = make('door', n, seed=10, reward_type='dense', info='minimal').unwrapped
  acts = busy_actions(K, H, n, 6)
  before = snapshot(u, 'door')
  got = u.rollout_branches(acts)
  unchanged(u, 'door', before)
  check(got, reference(u, acts))


def test_the_time_sliced_peg_schedule_when_the_grid_exceeds_the_cu_count():
  import torch
  K, H, n = 65, 12, 64                                                    # 260 workgroups of 16 virtual envs, twelve steps > the ten-step slice
  assert (K * n + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count
  u = lifelong('peg', n, seed=11, reward_type='dense').unwrapped           # (the goal row, its counter and the summary words travel across the slices)
  acts = busy_actions(K, H, n, 7)
  before = snapshot(u, 'peg')
  got = u.rollout_branches(acts)
  unchanged(u, 'peg', before)
  check(got, reference(u, acts))


# ---------------------------------------------------------------------------------------------------------------- 6. clock, shards, capture, switches
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_clock_words_add_to_the_step_counter(kind):
  import torch
  K, H, n, s, c = 2, 7, 5, 11, 1000
  u = lifelong(kind, n, env_offset=1).unwrapped
  acts = busy_actions(K, H, n, 8)
  u.total_step_count = s + c
  want = u.rollout_branches(acts)
  u.total_step_count = s
  clock = torch.tensor([0, c], dtype=torch.int64, device='cuda')
  got = u.rollout_branches(acts, clock=clock.data_ptr())
  for k in KEYS:
    same(got[k], want[k], k)
  if kind == 'peg':
    other = u.rollout_branches(acts)                                      # (step counter s without the clock: other draws, so the clock was read)
    assert not torch.equal(other['last_obs'][:, :, 7:], want['last_obs'][:, :, 7:])


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_a_shard_equals_its_rows_of_the_full_launch(kind):
  K, H, n, a, b = 3, 7, 11, 3, 9
  u = lifelong(kind, n, seed=12).unwrapped
  acts = busy_actions(K, H, n, 9)
  full = u.rollout_branches(acts)
  piece = lifelong(kind, b - a, seed=12, env_offset=a).unwrapped
  piece.load_state_dict(rows_of(u.state_dict(), a, b))
  got = piece.rollout_branches(acts[:, :, a:b].contiguous())
  for k in KEYS:
    same(got[k], full[k][:, a:b].contiguous(), f'{k} of rows {a}..{b}')


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_the_launch_is_captured_into_a_graph_after_one_eager_call(kind):
  import torch
  K, H, n = 3, 5, 5
  u = lifelong(kind, n).unwrapped
  acts = busy_actions(K, H, n, 10)
  eager = u.rollout_branches(acts)
  before = snapshot(u, kind)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    res = u.rollout_branches(acts)
  for rep in range(2):
    for v in res.values():
      v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
      same(res[k], eager[k], f'{k} of replay {rep}')
  unchanged(u, kind, before)


def test_the_64_lane_switch_refuses_the_call():
  from earl_benchmark_amd import _abi
  u = make('door', 4, seed=3, info='minimal').unwrapped
  lib = _abi.load()
  assert lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
  try:
    with pytest.raises(_abi.EarlHipError, match='earl_sawyer_branch_rollout'):
      u.rollout_branches(busy_actions(2, 3, 4, 1))
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK
  u.rollout_branches(busy_actions(2, 3, 4, 1))


@pytest.mark.parametrize('kind', ['minitaur', 'kitchen'])
def test_envs_without_a_branch_launch_raise(kind):
  import torch
  env = make(kind, 2, seed=3)
  with pytest.raises(NotImplementedError, match='rollout_branches'):
    env.unwrapped.rollout_branches(torch.zeros(1, 1, 2, 4))

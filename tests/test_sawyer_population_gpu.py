"""Policy populations and episode summaries on the Sawyer door and peg (include/earl_physics.h: earl_sawyer_population_rollout; env.rollout_policy(pop) /
env.evaluate_policy):
  1. population == pieces: the launch equals cutting the batch at the global ids that are multiples of G and running each piece as a single policy on a fresh env;
  2. summary == definition, applied to the same launch's reward / success rows;
  3. a summary-only launch (no [T] array at all) == the full launch: summaries, state, last_obs, fail_count, counters -- also across a goal switch and next to a
     poisoned env;
  4. evaluate_policy(pop, T, episodes=3) == three reset() + rollout_policy(pop) rounds reduced on the host; population_fitness is additive over two shards;
  5. one launch of T == T launches of one.
The networks are the small-gain ones of tests/test_sawyer_policy_rollout_gpu.py; its MAX_GUARD_SHARE is the condition on every un-poisoned case."""

import numpy as np
import pytest

from test_physics_step_graph_gpu import STATE, make, same
from test_sawyer_policy_rollout_gpu import MAX_GUARD_SHARE, OUT_KEYS, guard_share, policy

pytestmark = pytest.mark.gpu

T = 23


def population(P, G, hidden=(64, 64), head=None, seed=0):
  """P small-gain members of one architecture with different weights -> PolicyPopulation on the GPU"""
  from earl_benchmark_amd.policy import PolicyPopulation
  members = [policy(hidden, 'relu', 'tanh', head=head, seed=seed + 17 * p)[0] for p in range(P)]
  return PolicyPopulation(members, envs_per_policy=G, device='cuda', obs_dim=14, act_dim=4)


def rows_of(sd, a, b):
  import torch
  return {k: (v[a:b].clone() if torch.is_tensor(v) else v) for k, v in sd.items()}


def by_definition(reward, success):
  """the summary's definitions as plain loops on the host: ret = sum over t ascending of (double)reward_t, success at step T - 1, the smallest t with success or -1"""
  r, s = reward.cpu().numpy(), success.cpu().numpy().astype(bool)
  ret = np.zeros(r.shape[1], np.float64)
  first = np.full(r.shape[1], -1, np.int32)
  for t in range(r.shape[0]):
    ret = ret + r[t].astype(np.float64)
    first = np.where((first < 0) & s[t], t, first).astype(np.int32)
  return ret, s[-1], first


def same_np(got, want, what):
  got = got.cpu().numpy()
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype)
  if got.dtype == np.float64:
    got, want = got.view(np.int64), want.view(np.int64)
  np.testing.assert_array_equal(got, want, err_msg=what)


def raw_launch(env, pol, full, summary, sample=False):
  """earl_sawyer_population_rollout called directly, with the env's bookkeeping done by hand: full = every `out` array and the actions, or none of them (every
  pointer NULL); summary = three arrays pre-filled with rubbish (step 0 must initialise them), or NULL.  -> (out dict or {}, (ret, success, first) or None)"""
  import torch
  from earl_benchmark_amd import _abi
  u = env.unwrapped
  n = u.num_envs
  out = {}
  if full:
    out = u._new_out((T,))
    out['actions'] = torch.empty(T, n, 4, dtype=torch.float32, device='cuda')
  bufs, sm = None, None
  if summary:
    bufs = (torch.full((n,), 1e300, dtype=torch.float64, device='cuda'), torch.ones(n, dtype=torch.bool, device='cuda'),
            torch.full((n,), 12345, dtype=torch.int32, device='cuda'))
    sm = _abi.EpisodeSummary(ret=bufs[0].data_ptr(), success_last=bufs[1].data_ptr(), first_success=bufs[2].data_ptr())
  assert not u._last_obs_stale
  head = pol.head(sample=sample) if pol.gaussian else None
  u._cfg.step_counter = u.total_step_count
  u._issue_rollout(None, T, out, policy=(pol, head, u.last_obs), summary=sm)
  u.total_step_count += T
  return out, bufs


def state_rows(env, kind, a=None, b=None, skip=()):
  u = env.unwrapped
  return {k: getattr(u, k)[a:b].clone() for k in STATE[kind] if k not in skip}


# ---------------------------------------------------------------------------------------------------------------- 1. population == pieces
SETTINGS = [('door', 64, 16, 8, 5), ('door', 64, 16, 10, 5), ('door', 4160, 1040, 0, 4), ('peg', 64, 16, 8, 5), ('peg', 4160, 1040, 0, 4)]


@pytest.mark.parametrize('kind,n,G,off,P', SETTINGS, ids=[f'{s[0]}-{s[1]}-G{s[2]}-off{s[3]}' for s in SETTINGS])
@pytest.mark.parametrize('head', [None, 'sample'])
def test_population_launch_equals_its_single_policy_pieces_bit_for_bit(kind, n, G, off, P, head):
  """door 64 at env_offset 8: the first and the last member are partial; at 10 a wavefront's four envs belong to two members; door 4160: the eight-wave build
  against single-wave pieces; peg 4160: the time-sliced schedule against unsliced pieces"""
  import torch
  big = make(kind, n, seed=5, env_offset=off)
  u = big.unwrapped
  if kind == 'peg' and n > 64:
    assert u._uses_queue(T) and (n + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count
  pop = population(P, G, head=head, seed=n + off)
  assert (off + n - 1) // G == P - 1
  sd = u.state_dict()
  obs0 = u.last_obs.clone()
  kw = {'return_noise': True} if head else {}
  got = {k: v.clone() for k, v in big.rollout_policy(pop, T, **kw).items()}
  assert tuple(got['actions'].shape) == (T, n, 4) and not bool(got['actions'].isnan().any())
  print(f'{kind} n={n} G={G} off={off} head={head}: guard share {guard_share(got):.5f}')
  assert guard_share(got) <= MAX_GUARD_SHARE
  cuts = [off] + [g for g in range((off // G + 1) * G, off + n, G)] + [off + n]
  assert len(cuts) - 1 == P
  for a, b in zip(cuts[:-1], cuts[1:]):
    p = a // G
    piece = make(kind, b - a, seed=5, env_offset=a)
    piece.unwrapped.load_state_dict(rows_of(sd, a - off, b - off))
    want = piece.rollout_policy(pop.member(p), T, **kw)
    for k in OUT_KEYS + ('actions',) + (('eps',) if head else ()):
      assert (k in got) == (k in want), k
      if k in got:
        same(got[k][:, a - off:b - off], want[k], f'{k} of member {p}')
    end = state_rows(piece, kind)
    for k, v in state_rows(big, kind, a - off, b - off).items():
      same(v, end[k], f'{k} of member {p}')
    pu = piece.unwrapped
    assert pu.total_step_count == u.total_step_count == T and int(pu._cfg.counter) == int(u._cfg.counter)
    same(u._last_success[a - off:b - off], pu._last_success, '_last_success')
  if head is None:
    # members with different weights must not pass by all reading member 0: step 0 of every env of another member differs from member 0's action on its observation
    a0 = pop.member(0)(obs0)
    other = (torch.arange(n, device='cuda') + off) // G > 0
    assert bool(((got['actions'][0] - a0).abs() > 1e-3).any(-1)[other].all())
    assert bool(((got['actions'][0] - a0).abs() < 1e-4).all(-1)[~other].all())


# ---------------------------------------------------------------------------------------------------------------- 2. summary == definition
@pytest.mark.parametrize('kind,reward_type,gcf', [('door', 'dense', 0), ('peg', 'sparse', 0), ('peg', 'dense', 0), ('door', 'dense', 5), ('peg', 'dense', 5)])
def test_summary_is_its_definition_applied_to_the_launch_own_rows(kind, reward_type, gcf):
  n, G, off, P = 64, 16, 8, 5
  env = make(kind, n, seed=7, gcf=gcf, env_offset=off, reward_type=reward_type)
  pop = population(P, G, head='sample', seed=3)
  out, (ret, succ, first) = raw_launch(env, pop, full=True, summary=True, sample=True)
  want = by_definition(out['reward'], out['success'])
  same_np(ret, want[0], 'ret')
  same_np(succ, want[1], 'success_last')
  same_np(first, want[2], 'first_success')
  if reward_type == 'dense':
    r = out['reward'].cpu().numpy()
    assert len(np.unique(r)) > n and float(np.abs(r).max()) > 0            # (many different float32 terms: the order of the fp64 sum is visible)
  print(f'{kind} {reward_type} gcf={gcf}: guard share {guard_share(out):.5f}')
  assert guard_share(out) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 3. summary only == full launch
def summary_only_equals_full(kind, n, G, off, P, gcf=0, prepare=None, **kw):
  """three twins: the full launch through rollout_policy, evaluate_policy(reset_first=False), and the raw entry point with every `out` pointer and `actions` NULL"""
  pop = population(P, G, head=None, seed=11)
  envs = [make(kind, n, seed=9, gcf=gcf, env_offset=off, **kw) for _ in range(3)]
  for e in envs:
    if prepare:
      prepare(e)
  ea, eb, ec = envs
  before = ea.unwrapped.fail_count.clone()
  out = ea.rollout_policy(pop, T)
  want = by_definition(out['reward'], out['success'])
  s = eb.evaluate_policy(pop, T, reset_first=False)
  assert set(s) == {'ret', 'success', 'first_success', 'guard_steps'} and all(tuple(v.shape) == (1, n) for v in s.values())
  _, (ret, succ, first) = raw_launch(ec, pop, full=False, summary=True)
  for got in ((s['ret'][0], s['success'][0], s['first_success'][0]), (ret, succ, first)):
    same_np(got[0], want[0], 'ret')
    same_np(got[1], want[1], 'success_last')
    same_np(got[2], want[2], 'first_success')
  same(s['guard_steps'][0], (ea.unwrapped.fail_count - before), 'guard_steps')
  same(s['guard_steps'][0], out['status'].to(s['guard_steps'].dtype).sum(0).to(s['guard_steps'].dtype), 'guard_steps against the status rows')
  ua = ea.unwrapped
  for e in (eb, ec):
    u = e.unwrapped
    for k in STATE[kind]:
      if k != 'lifelong_return_t':                                        # (Python bookkeeping: evaluate_policy adds `ret`, rollout_policy torch's sum of the rows)
        same(getattr(ua, k), getattr(u, k), k)
    same(u.last_obs, out['obs'][-1], 'last_obs is the full launch\'s last row')
    assert u.total_step_count == ua.total_step_count and int(u._cfg.counter) == int(ua._cfg.counter)
  same(ua._last_success, eb.unwrapped._last_success, '_last_success')
  assert not eb.unwrapped._last_obs_stale
  np.testing.assert_allclose(eb.unwrapped.lifelong_return_t.cpu().numpy(), ua.lifelong_return_t.cpu().numpy(), rtol=1e-12, atol=0)
  return out, s, envs


@pytest.mark.parametrize('kind,n,G,off,P', [('door', 64, 16, 8, 5), ('door', 4160, 1040, 0, 4), ('peg', 64, 16, 8, 5), ('peg', 4160, 1040, 0, 4)])
def test_summary_only_launch_equals_the_full_launch(kind, n, G, off, P):
  out, _, _ = summary_only_equals_full(kind, n, G, off, P)
  print(f'{kind} n={n}: guard share {guard_share(out):.5f}')
  assert guard_share(out) <= MAX_GUARD_SHARE


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_summary_only_launch_carries_the_patched_goal_block_to_the_next_action(kind):
  """a goal switch inside the launch: the patched goal block lives in the carried row of last_obs and the policy of the next step reads it -- the state the launch
  leaves equals the full launch's, whose actions follow the patched rows (tests/test_sawyer_policy_rollout_gpu.py).  The door's one-row goal table makes the switch
  visible because a custom goal is replaced by the table's row; the peg runs with reset_at_goal (15 goal rows)"""
  import torch

  def prepare(env):
    u = env.unwrapped
    env.rollout(torch.zeros(3, u.num_envs, 4, device='cuda'))            # the switch does not fall on a launch boundary
    if kind == 'door':
      custom = u.goal_t[0].clone()
      custom[:3] += 0.05
      custom[4:] -= 0.03
      u.reset_goal(custom)
      u.last_obs.copy_(u._get_obs_t())                                    # (the row the env would have returned under the custom goal)
      u._last_obs_stale = False

  out, _, envs = summary_only_equals_full(kind, 64, 16, 8, 5, gcf=5, prepare=prepare, **({'reset_at_goal': True} if kind == 'peg' else {}))
  goal = out['obs'][:, :, 7:]
  switched = (goal[1:] != goal[:-1]).any(-1).any(-1)
  assert bool(switched.any()) and int(switched.nonzero()[0]) + 1 < T - 1, 'no goal switch changed the goal block inside the launch'
  assert int(envs[1].unwrapped.steps_since_goal_change[0]) == (3 + T) % 5
  assert guard_share(out) <= MAX_GUARD_SHARE


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_summary_only_launch_next_to_a_poisoned_env(kind):
  """NaN in one env's qvel row (as tests/test_sawyer_full_gpu.py does): the failure guard rolls it back at every step -- guard_steps = T, ret = 0, no success, its
  carried row stays the last stable observation -- and its neighbours, those of its own wavefront included, are bit-identical to the unpoisoned run"""
  import torch
  n, G, off, P, bad = 64, 16, 8, 5, 5
  pop = population(P, G, head=None, seed=11)
  clean, env = make(kind, n, seed=9, env_offset=off), make(kind, n, seed=9, env_offset=off)
  u = env.unwrapped
  u.qvel[bad, 1] = float('nan')
  stable = u.last_obs[bad].clone()
  want = clean.evaluate_policy(pop, T, reset_first=False)
  got = env.evaluate_policy(pop, T, reset_first=False)
  ok = [i for i in range(n) if i != bad]
  for k in want:
    same(got[k][:, ok], want[k][:, ok], k)
  for k in STATE[kind]:
    same(getattr(u, k)[ok], getattr(clean.unwrapped, k)[ok], k)
  assert int(got['guard_steps'][0, bad]) == T and float(got['ret'][0, bad]) == 0.0 and not bool(got['success'][0, bad]) and int(got['first_success'][0, bad]) == -1
  same(u.last_obs[bad], stable, 'the carried row of the poisoned env')
  assert int(u.fail_count[bad]) == T and bool(torch.isnan(u.qvel[bad, 1]))
  share = float(want['guard_steps'].sum()) / (T * n)
  print(f'{kind}: guard share of the unpoisoned run {share:.5f}')
  assert share <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 4. episodes and shards
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_evaluate_policy_episodes_equal_reset_and_rollout_rounds_and_fitness_adds_over_shards(kind):
  import torch
  from earl_benchmark_amd import sharding
  n, G, P, E = 64, 16, 4, 3
  pop = population(P, G, head='sample', seed=21)
  ea, eb = make(kind, n, seed=13, reward_type='dense'), make(kind, n, seed=13, reward_type='dense')
  s = ea.evaluate_policy(pop, T, episodes=E, sample=True)
  assert all(tuple(v.shape) == (E, n) for v in s.values())
  assert (s['ret'].dtype, s['success'].dtype, s['first_success'].dtype, s['guard_steps'].dtype) == (torch.float64, torch.bool, torch.int32, torch.int32)
  guard = 0
  for e in range(E):
    eb.reset()
    out = eb.rollout_policy(pop, T, sample=True)
    want = by_definition(out['reward'], out['success'])
    same_np(s['ret'][e], want[0], f'ret of episode {e}')
    same_np(s['success'][e], want[1], f'success of episode {e}')
    same_np(s['first_success'][e], want[2], f'first_success of episode {e}')
    same(s['guard_steps'][e], out['status'].to(torch.int32).sum(0).to(torch.int32), f'guard_steps of episode {e}')
    guard += int((out['status'] != 0).sum())
  assert guard <= MAX_GUARD_SHARE * E * T * n
  for k in STATE[kind]:
    same(getattr(ea.unwrapped, k), getattr(eb.unwrapped, k), k)
  assert ea.unwrapped.total_step_count == eb.unwrapped.total_step_count == E * T and int(ea.unwrapped._cfg.counter) == int(eb.unwrapped._cfg.counter)
  assert bool((s['ret'][0] != s['ret'][1]).any())                          # (the episodes differ: each starts from a reset of its own)
  # two shards of the same global ids: the same rows, and the fitness table adds up
  whole = sharding.population_fitness(s, 0, G, P)
  parts = []
  for a, b in ((0, 24), (24, n)):                                        # (the cut is no multiple of G)
    sh = make(kind, b - a, seed=13, env_offset=a, reward_type='dense')
    ps = sh.evaluate_policy(pop, T, episodes=E, sample=True)
    for k in s:
      same(ps[k], s[k][:, a:b], f'{k} of shard {a}..{b}')
    parts.append(sharding.population_fitness(ps, a, G, P))
  total = parts[0] + parts[1]
  assert torch.equal(total[:, 1:], whole[:, 1:]) and float(whole[:, 2].sum()) == E * n
  np.testing.assert_allclose(total[:, 0].cpu().numpy(), whole[:, 0].cpu().numpy(), rtol=1e-12, atol=0)
  with pytest.raises(ValueError, match='one episode'):
    ea.evaluate_policy(pop, T, episodes=2, reset_first=False)
  with pytest.raises(ValueError, match='need members'):
    make(kind, 8, seed=13, env_offset=P * G - 4).evaluate_policy(pop, T)


# ---------------------------------------------------------------------------------------------------------------- 5. one launch == T launches
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('head', [None, 'sample'])
def test_one_population_launch_of_T_equals_T_launches_of_one(kind, head):
  import torch
  n, G, off, P = 40, 16, 8, 3
  ea, eb = make(kind, n, seed=9, gcf=7, env_offset=off), make(kind, n, seed=9, gcf=7, env_offset=off)
  pop = population(P, G, head=head, seed=2)
  kw = {'return_noise': True} if head else {}
  one = ea.rollout_policy(pop, T, **kw)
  rows = [{k: v.clone() for k, v in eb.rollout_policy(pop, 1, **kw).items()} for _ in range(T)]
  for k in one:
    same(one[k], torch.cat([r[k] for r in rows]), k)
  for k in STATE[kind]:
    same(getattr(ea.unwrapped, k), getattr(eb.unwrapped, k), k)
  assert ea.unwrapped.total_step_count == eb.unwrapped.total_step_count == T
  assert guard_share(one) <= MAX_GUARD_SHARE

"""env.rollout_policy on the Sawyer door and peg (include/earl_physics.h: earl_sawyer_policy_rollout): T closed-loop env steps in ONE launch of the rollout
kernel, the policy evaluated by the lanes that own the env.
  5. closed loop == open loop: rollout(out['actions']) from the same state returns the same bits and leaves the same state -- at 64 envs, above 4096 door envs
     (the eight-wave build), at a peg batch the time-sliced schedule takes, and under a LifelongWrapper whose goal switch fires inside the launch;
  6. the actions are the contract: every (t, env) action equals earl_mlp_policy_forward_cpu (libearl_host.so) on float32(obs[t - 1]) (obs0 for t = 0), bit for
     bit; a sampled head with the returned eps, and the eps equal to normal_quantile_f32 of the Philox words recomputed on the host;
  7. one launch of T == T launches of one, and the draws depend on (seed, global env id, step counter) only.

The width matrix (every hidden width, partial groups of 64 output rows, the eight-wave build) lives in tests/test_sawyer_policy_widths_gpu.py."""

import numpy as np
import pytest

from test_sawyer_policy_rollout import forward_cpu, random_layers
from test_physics_step_graph_gpu import STATE, make, same

pytestmark = pytest.mark.gpu

GAUSS_DRAW = 0x504F4C00
HEADS = {None: None, 'mean': 0, 'sample': 1}
# Small-gain networks (hidden layers at unit gain, the last layer at LAST_GAIN / sqrt(K), biases 0.3 LAST_GAIN), so that most envs move gently: the bound of 1 % of
# rows with status != 0 below is a condition on the test, not a measurement of the code
GAIN, LAST_GAIN = 1.0, 0.5
MAX_GUARD_SHARE = 0.01


def policy(hidden, hidden_act='relu', out_act='tanh', head=None, log_std_map='clamp', seed=0):
  """-> (the policy on the GPU, its host layers)"""
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  layers = random_layers([14] + list(hidden) + [8 if head else 4], seed=seed, gain=GAIN, last_gain=LAST_GAIN)
  if head:
    w, b = layers[-1]
    b[4:] = np.array([-3.0, -2.0, -1.5, -2.5], np.float32)               # sigma around 0.05 .. 0.2: the noise moves the actions without saturating them
    pi = GaussianMLPPolicy(layers, hidden_act, squash=(out_act == 'tanh'), log_std_bounds=(-5.0, 2.0), log_std_map=log_std_map, device='cuda', obs_dim=14, act_dim=4)
  else:
    pi = MLPPolicy(layers, hidden_act, out_act, device='cuda', obs_dim=14, act_dim=4)
  return pi, layers


def snapshot(env):
  u = env.unwrapped
  return u.state_dict()


def restore(env, sd):
  env.unwrapped.load_state_dict(sd)


def state_of(env):
  u = env.unwrapped
  return {k: getattr(u, k).clone() for k in STATE['peg' if u.nv >= 15 else 'door']}, u.total_step_count, int(u._cfg.counter), u._last_success.clone()


def same_state(a, b):
  for k in a[0]:
    same(a[0][k], b[0][k], k)
  assert a[1] == b[1] and a[2] == b[2]
  same(a[3], b[3], '_last_success')


OUT_KEYS = ('obs', 'reward', 'done', 'success', 'status', 'info')


def closed_equals_open(env, pi, T, **kw):
  sd = snapshot(env)
  got = env.rollout_policy(pi, T, **kw)
  got = {k: v.clone() for k, v in got.items()}
  end = state_of(env)
  assert not bool(got['actions'].isnan().any())
  restore(env, sd)
  want = env.rollout(got['actions'])
  for k in OUT_KEYS:
    assert (k in got) == (k in want), k
    if k in got:
      same(got[k], want[k], k)
  same_state(end, state_of(env))
  return got, sd


def guard_share(out):
  return float((out['status'] != 0).float().mean())


# ---------------------------------------------------------------------------------------------------------------- 5. closed loop == open loop
def cu_count():
  import torch
  return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize('kind,n', [('door', 64), ('door', 4160), ('peg', 64), ('peg', 4160)])
@pytest.mark.parametrize('head', [None, 'sample'])
def test_closed_loop_equals_open_loop_bit_for_bit(kind, n, head):
  """observed share of rows with status != 0 (first run, one MI355X): 0 in every case"""
  T = 23
  env = make(kind, n, seed=5)
  u = env.unwrapped
  if kind == 'door' and n > 64:
    assert n > 4096                                                     # the launcher's condition for the eight-wave build (csrc/physics.hip)
  if kind == 'peg' and n > 64:
    assert u._uses_queue(T) and (n + 15) // 16 > cu_count() and T >= 21     # more 16-env workgroups than CUs and T > 1: the time-sliced schedule, slices of 10 env steps
  pi, _ = policy((64, 64), 'relu', 'tanh', head=head, seed=n)
  got, _ = closed_equals_open(env, pi, T, **({'return_noise': True} if head else {}))
  assert tuple(got['actions'].shape) == (T, n, 4) and u.total_step_count == T
  print(f'{kind} n={n} head={head}: guard share {guard_share(got):.5f}')
  assert guard_share(got) <= MAX_GUARD_SHARE
  # a second launch continues from the first (obs0 = the state's observation, counters advanced)
  got2, _ = closed_equals_open(env, pi, 5)
  assert u.total_step_count == T + 5 and not bool((got2['obs'][0] == got['obs'][-1]).all())


@pytest.mark.parametrize('kind,n', [('door', 64), ('door', 4160), ('peg', 64), ('peg', 4160)])
def test_closed_loop_equals_open_loop_under_the_lifelong_wrapper(kind, n):
  """a goal switch inside the launch: the policy of the step after it sees the patched goal block, and the open-loop rollout fed with the actions walks through the
  same switches (the draws are keyed by the step counter, not by the entry point)"""
  import torch
  T, gcf = 23, 5
  env = make(kind, n, seed=6, gcf=gcf)
  u = env.unwrapped
  pi, _ = policy((64,), 'tanh', 'tanh', head='sample', seed=3)
  env.rollout(torch.zeros(3, n, 4, device='cuda'))                      # the switch does not fall on a launch boundary
  got, _ = closed_equals_open(env, pi, T)
  assert int(u.steps_since_goal_change[0]) == (3 + T) % gcf
  switched = (got['obs'][1:, :, 7:] != got['obs'][:-1, :, 7:]).any(-1).any(-1)
  if u._cfg.n_goal_rows > 1:
    assert bool(switched.any()), 'no goal switch changed the goal block inside the launch'
  assert guard_share(got) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 6. the actions are the contract
def expected_eps(seed, env_offset, n, step0, T):
  """[T, n, 4] float32: normal_quantile_f32(word >> 8) of the Philox block {GAUSS_DRAW, global env id, ev lo, ev hi}, ev = step0 + t, key = seed -- the block
  function is tests/gaussian_policy_helpers.py's numpy statement, the quantile libearl_host.so's"""
  from earl_benchmark_amd import _abi
  from gaussian_policy_helpers import philox4x32_10
  host = _abi.load_host()
  ev = (np.uint64(step0) + np.arange(T, dtype=np.uint64))[:, None] + np.zeros((1, n), np.uint64)
  env = (np.uint64(env_offset) + np.arange(n, dtype=np.uint64))[None, :] + np.zeros_like(ev)
  words = philox4x32_10(np.full_like(ev, GAUSS_DRAW), env, ev & np.uint64(0xFFFFFFFF), ev >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
  k = np.stack(words, axis=-1) >> np.uint64(8)
  return np.array([host.earl_normal_quantile_f32(int(v)) for v in k.reshape(-1)], np.float32).reshape(T, n, 4)


CASES = [((16,), 'relu', 'none', None, 'clamp'), ((64, 64), 'tanh', 'tanh', None, 'clamp'), ((256, 256), 'relu', 'tanh', None, 'clamp'),
         ((256,), 'tanh', 'tanh', None, 'clamp'), ((16, 64), 'relu', 'tanh', 'mean', 'clamp'), ((64, 16), 'tanh', 'tanh', 'sample', 'tanh'),
         ((256, 64), 'relu', 'none', 'sample', 'clamp')]


@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('hidden,hact,oact,head,lmap', CASES, ids=[f'{"x".join(map(str, c[0]))}-{c[1]}-{c[2]}-{c[3]}-{c[4]}' for c in CASES])
def test_actions_are_the_contract_bit_for_bit(kind, hidden, hact, oact, head, lmap):
  """every action of the launch == earl_mlp_policy_forward_cpu on the float32 observation the step consumed; rolled-back rows included.
  observed share of rows with status != 0 (first run, one MI355X): 0 in every case"""
  from earl_benchmark_amd import _abi
  n, T, seed, off = 64, 23, 11, 3
  env = make(kind, n, seed=seed, env_offset=off)
  u = env.unwrapped
  pi, layers = policy(hidden, hact, oact, head=head, log_std_map=lmap, seed=len(hidden) * 7 + hidden[0])
  env.rollout_policy(pi, 2)                                             # (the launch under test starts at a step counter that is not 0)
  step0 = u.total_step_count
  obs0 = u.last_obs.clone()                                             # what the env last returned: the launch's obs0
  kw = {} if head is None else {'sample': head == 'sample', 'return_noise': True}
  out = env.rollout_policy(pi, T, **kw)
  x = np.concatenate([obs0.cpu().numpy()[None], out['obs'].cpu().numpy()[:-1]]).astype(np.float32).reshape(T * n, 14)
  hd, eps = None, None
  if head is not None:
    hd = (HEADS[head], _abi.LOGSTD_MAPS[lmap], -5.0, 2.0)
    eps = out['eps'].cpu().numpy()
    np.testing.assert_array_equal(eps.view(np.uint32), expected_eps(seed, off, n, step0, T).view(np.uint32))       # written in both modes
  want = forward_cpu(layers, hact, oact, x, head=hd, eps=None if eps is None else eps.reshape(T * n, 4)).reshape(T, n, 4)
  got = out['actions'].cpu().numpy()
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  if head == 'sample':
    mean = forward_cpu(layers, hact, oact, x, head=(0,) + hd[1:]).reshape(T, n, 4)
    assert (got != mean).mean() > 0.9                                   # ... and the noise is in the actions
  assert np.abs(got).max() > 1e-3 and len(np.unique(got[:, :, 0])) > T * n // 2
  print(f'{kind} {hidden} {hact} {oact} {head}: guard share {guard_share(out):.5f}')
  assert guard_share(out) <= MAX_GUARD_SHARE


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_actions_follow_the_goal_block_across_reset_goal_and_a_goal_switch(kind):
  """the goal block the policy sees is the one in force: after reset_goal(custom) the first action is the oracle's on the observation of the NEW goal (last_obs still
  carries the old one and is marked stale, through state_dict too), and after a lifelong goal switch inside the launch the next action is the oracle's on the patched
  row.  The door's one-row goal table makes the switch visible because the custom goal is replaced by the table's row; the peg runs with reset_at_goal (15 goal rows)"""
  import torch
  n, T, gcf = 64, 23, 5
  env = make(kind, n, seed=12, gcf=gcf, **({'reset_at_goal': True} if kind == 'peg' else {}))
  u = env.unwrapped
  pi, layers = policy((64,), 'tanh', 'tanh', seed=5)
  env.rollout_policy(pi, 2)
  assert not u._last_obs_stale
  custom = u.goal_t[0].clone()
  custom[:3] += 0.05
  custom[4:] -= 0.03
  u.reset_goal(custom)
  assert u._last_obs_stale and not bool((u.last_obs[:, 7:] == custom).all())
  obs0 = u._get_obs_t().clone()
  same(obs0[:, 7:].contiguous(), custom.expand(n, 7).contiguous(), 'the recomputed observation carries the new goal')
  sd = u.state_dict()
  assert sd['last_obs_stale'] is True
  out = env.rollout_policy(pi, T)
  assert not u._last_obs_stale
  x = np.concatenate([obs0.cpu().numpy()[None], out['obs'].cpu().numpy()[:-1]]).astype(np.float32).reshape(T * n, 14)
  want = forward_cpu(layers, 'tanh', 'tanh', x).reshape(T, n, 4)
  got = out['actions'].cpu().numpy()
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  goal = out['obs'][:, :, 7:]
  same(goal[0].contiguous(), custom.expand(n, 7).contiguous(), 'row 0 is emitted under the custom goal')
  switched = (goal[1:] != goal[:-1]).any(-1).any(-1)
  assert bool(switched.any()) and int(switched.nonzero()[0]) + 1 < T - 1, 'no goal switch changed the goal block inside the launch'
  ts = int(switched.nonzero()[0]) + 1                                  # the first row emitted with a switched goal block; step ts + 1 consumes it
  obs = out['obs'].cpu().numpy()
  pre = np.concatenate([obs[ts, :, :7], obs[ts - 1, :, 7:]], -1).astype(np.float32)     # that row as it stood before the patch
  assert (got[ts + 1] != forward_cpu(layers, 'tanh', 'tanh', pre)).any()                # ... a policy fed the pre-patch row would have acted differently
  assert guard_share(out) <= MAX_GUARD_SHARE
  # the flag travels with the dict: loaded, the env recomputes its first observation again and repeats the launch's first action
  u.load_state_dict(sd)
  assert u._last_obs_stale
  again = env.rollout_policy(pi, 1)
  same(again['actions'][0], out['actions'][0], 'first action after load_state_dict')
  # a dict saved in the ordinary state clears the flag of a stale env
  sd2 = u.state_dict()
  u.reset_goal(custom)
  u.load_state_dict(sd2)
  assert not u._last_obs_stale


# ---------------------------------------------------------------------------------------------------------------- 7. one launch == T launches
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('head', [None, 'sample'])
def test_one_launch_of_T_equals_T_launches_of_one(kind, head):
  import torch
  n, T = 40, 23
  ea, eb = make(kind, n, seed=9, gcf=7), make(kind, n, seed=9, gcf=7)
  pi, _ = policy((64, 64), 'relu', 'tanh', head=head, seed=2)
  kw = {'return_noise': True} if head else {}
  one = ea.rollout_policy(pi, T, **kw)
  rows = [{k: v.clone() for k, v in eb.rollout_policy(pi, 1, **kw).items()} for _ in range(T)]
  for k in one:
    same(one[k], torch.cat([r[k] for r in rows]), k)
  same_state(state_of(ea), state_of(eb))


def test_draws_depend_on_the_global_env_id_not_on_the_shard():
  """two envs with different env_offset that share global ids draw the same noise at the same step counter"""
  import torch
  pi, _ = policy((16,), 'relu', 'tanh', head='sample', seed=1)
  ea, eb = make('door', 8, seed=4, env_offset=0), make('door', 8, seed=4, env_offset=4)
  a = ea.rollout_policy(pi, 6, return_noise=True)['eps']
  b = eb.rollout_policy(pi, 6, return_noise=True)['eps']
  same(a[:, 4:], b[:, :4], 'eps of global ids 4..7')
  assert not torch.equal(a[:, :4], b[:, :4])
  c = eb.rollout_policy(pi, 6, return_noise=True)['eps']                # the next launch: the step counter has advanced
  assert not torch.equal(b, c)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_rollout_policy_refuses_what_it_cannot_run():
  from earl_benchmark_amd.policy import MLPPolicy
  env = make('door', 8)
  pi, layers = policy((16,), seed=0)
  with pytest.raises(ValueError, match='need a GaussianMLPPolicy'):
    env.rollout_policy(pi, 3, sample=False)
  with pytest.raises(ValueError, match='need a GaussianMLPPolicy'):
    env.rollout_policy(pi, 3, return_noise=True)
  with pytest.raises(ValueError, match='the policy is on cpu'):
    env.rollout_policy(MLPPolicy(layers, obs_dim=14, act_dim=4), 3)
  with pytest.raises(ValueError, match='observation width 12 and action width 3'):
    env.rollout_policy(MLPPolicy(random_layers([12, 16, 3], seed=0), device='cuda'), 3)
  with pytest.raises(ValueError, match='T = 0'):
    env.rollout_policy(pi, 0)
  n0 = int(env.interventions.sum())
  out = env.rollout_policy(pi, 3, reset_first=True)
  assert int(env.interventions.sum()) == n0 + 8 and tuple(out['obs'].shape) == (3, 8, 14) and int(env.steps_since_reset[0]) == 3
  # the 64-lanes-per-env measurement builds have no policy form: an argument error, not a silent other kernel
  from earl_benchmark_amd import _abi
  lib = _abi.load()
  assert lib.earl_debug_set_physics_lanes(64) == 0
  try:
    with pytest.raises(_abi.EarlHipError):
      env.rollout_policy(pi, 3)
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == 0

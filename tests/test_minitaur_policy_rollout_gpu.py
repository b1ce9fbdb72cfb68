"""env.rollout_policy on the minitaur (include/earl_physics.h: earl_minitaur_policy_rollout): T closed-loop env steps in ONE launch of either rollout kernel, the
policy evaluated by the 32 lanes that own the env.
  1. closed loop == open loop: rollout(out['actions']) from the same state returns the same bits and leaves the same state, in all three one-wave launch shapes
     and in the two-wave form;
  2. the two forms return the same bits;
  3. the actions are the contract: every (t, env) action equals earl_mlp_policy_forward_cpu (libearl_host.so) on float32(obs[t - 1]) (last_obs for t = 0), bit
     for bit; a sampled head with the returned eps, and the eps equal to normal_quantile_f32 of the two Philox blocks recomputed on the host;
  4. a goal switch inside the launch; 5. the failure guard; 6. one launch of T == T launches of one; 7. shards; 8. the stale first observation; 9. the Python surface.

Every test asserts that at most 1 % of its rows sit in the failure guard: a condition on the inputs (small-gain networks, a standing robot), not a measurement of the
code.  (5) poisons one env on purpose: there the condition is held by the other envs' rows and by the unpoisoned run."""
import contextlib

import numpy as np
import pytest

from test_sawyer_policy_rollout import forward_cpu, random_layers
from test_physics_step_graph_gpu import STATE, make, same

pytestmark = pytest.mark.gpu

GAUSS_DRAW = 0x504F4C00
HEADS = {None: None, 'mean': 0, 'sample': 1}
GAIN, LAST_GAIN = 1.0, 0.5
MAX_GUARD_SHARE = 0.01
T12 = 12
OUT_KEYS = ('obs', 'reward', 'done', 'success', 'status')
STATE_KEYS = STATE['minitaur'] + ('motor_param', 'interventions')


def policy(hidden, hidden_act='relu', head=None, log_std_map='clamp', seed=0):
  """-> (the policy on the GPU, its host layers): tanh output, with a head the raw log-std biases at -2"""
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  layers = random_layers([32] + list(hidden) + [16 if head else 8], seed=seed, gain=GAIN, last_gain=LAST_GAIN)
  if head:
    layers[-1][1][8:] = np.float32(-2.0)
    pi = GaussianMLPPolicy(layers, hidden_act, squash=True, log_std_bounds=(-5.0, 2.0), log_std_map=log_std_map, device='cuda', obs_dim=32, act_dim=8)
  else:
    pi = MLPPolicy(layers, hidden_act, 'tanh', device='cuda', obs_dim=32, act_dim=8)
  return pi, layers


@contextlib.contextmanager
def launch_form(solo=-1, duo=-1):
  """the minitaur launch switches for the block, restored afterwards: solo -1 (by batch size) / 0 (packed) / 1 (env per wave) / 2 (env per workgroup); duo 0 / 1 / -1"""
  from earl_benchmark_amd import _abi
  lib = _abi.load()
  prev_solo, prev_duo = lib.earl_debug_set_solo_mt(solo), lib.earl_debug_set_minitaur_duo(duo)
  try:
    yield
  finally:
    lib.earl_debug_set_solo_mt(prev_solo)
    lib.earl_debug_set_minitaur_duo(prev_duo)


FORMS = {'one_wave_packed': dict(solo=0, duo=0), 'one_wave_env_per_wave': dict(solo=1, duo=0), 'one_wave_env_per_workgroup': dict(solo=2, duo=0),
         'two_wave': dict(solo=0, duo=1)}


def state_of(env):
  u = env.unwrapped
  return {k: getattr(u, k).clone() for k in STATE_KEYS}, u.total_step_count, u._counter, u._last_success.clone()


def same_state(a, b, skip=()):
  for k in a[0]:
    if k not in skip:
      same(a[0][k], b[0][k], k)
  assert a[1] == b[1] and a[2] == b[2]
  same(a[3], b[3], '_last_success')


def guard_share(out, what=''):
  share = float((out['status'] != 0).float().mean())
  print(f'{what}: share of rows in the failure guard {share:.5f}')
  return share


def closed_equals_open(env, pi, T, **kw):
  u = env.unwrapped
  sd = u.state_dict()
  got = {k: v.clone() for k, v in env.rollout_policy(pi, T, **kw).items()}
  end = state_of(env)
  assert not bool(got['actions'].isnan().any()) and float(got['actions'].abs().max()) <= 1.0
  u.load_state_dict(sd)
  want = env.rollout(got['actions'])
  for k in OUT_KEYS:
    same(got[k], want[k], k)
  same_state(end, state_of(env))
  return got


def expected_eps(seed, env_offset, n, step0, T):
  """[T, n, 8] float32: normal_quantile_f32(word >> 8) of the two Philox blocks {GAUSS_DRAW + b, global env id, ev lo, ev hi}, ev = step0 + t, key = seed; words
  x, y, z, w of block b -> dimensions 4 b .. 4 b + 3.  The block function is tests/gaussian_policy_helpers.py's numpy statement, the quantile libearl_host.so's"""
  from earl_benchmark_amd import _abi
  from gaussian_policy_helpers import philox4x32_10
  host = _abi.load_host()
  ev = (np.uint64(step0) + np.arange(T, dtype=np.uint64))[:, None] + np.zeros((1, n), np.uint64)
  env = (np.uint64(env_offset) + np.arange(n, dtype=np.uint64))[None, :] + np.zeros_like(ev)
  blocks = [np.stack(philox4x32_10(np.full_like(ev, GAUSS_DRAW + b), env, ev & np.uint64(0xFFFFFFFF), ev >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32), axis=-1)
            for b in (0, 1)]
  k = np.concatenate(blocks, axis=-1) >> np.uint64(8)
  return np.array([host.earl_normal_quantile_f32(int(v)) for v in k.reshape(-1)], np.float32).reshape(T, n, 8)


def oracle_actions(layers, hact, obs0, out, head=None, lmap='clamp', eps=None):
  """earl_mlp_policy_forward_cpu on float32 of the rows the steps consumed: obs0, then out['obs'][:-1] as emitted -> [T, n, 8]"""
  from earl_benchmark_amd import _abi
  T, n = out['obs'].shape[:2]
  x = np.concatenate([obs0.cpu().numpy()[None], out['obs'].cpu().numpy()[:-1]]).astype(np.float32).reshape(T * n, 32)
  hd = None if head is None else (HEADS[head], _abi.LOGSTD_MAPS[lmap], -5.0, 2.0)
  return forward_cpu(layers, hact, 'tanh', x, head=hd, eps=None if eps is None else eps.reshape(T * n, 8)).reshape(T, n, 8)


# ---------------------------------------------------------------------------------------------------------------- 1. closed loop == open loop
@pytest.mark.parametrize('form,n', [('one_wave_packed', 45), ('one_wave_env_per_wave', 45), ('one_wave_env_per_workgroup', 45), ('two_wave', 91)])
@pytest.mark.parametrize('head', [None, 'sample'])
def test_closed_loop_equals_open_loop_bit_for_bit(form, n, head):
  """n = 45: an odd batch, the last wave of the packed shape has an idle group; n = 91 in the two-wave form: a ragged last workgroup (5 x 16 + 11) and a wave with
  one live group"""
  with launch_form(**FORMS[form]):
    env = make('minitaur', n, seed=5)
    u = env.unwrapped
    pi, _ = policy((64, 64), 'relu', head=head, seed=n)
    got = closed_equals_open(env, pi, T12, **({'return_noise': True} if head else {}))
    assert tuple(got['actions'].shape) == (T12, n, 8) and u.total_step_count == T12
    assert guard_share(got, f'{form} n={n} head={head}') <= MAX_GUARD_SHARE
    # a second launch continues from the first
    got2 = closed_equals_open(env, pi, 5)
    assert u.total_step_count == T12 + 5 and not bool((got2['obs'][0] == got['obs'][-1]).all())
    assert guard_share(got2, 'second launch') <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 2. the two forms
def test_the_two_forms_return_the_same_bits():
  n, res = 91, {}
  pi, _ = policy((64, 64), 'tanh', head='sample', seed=8)
  for form in ('one_wave_packed', 'two_wave'):
    with launch_form(**FORMS[form]):
      env = make('minitaur', n, seed=6)
      out = env.rollout_policy(pi, T12, return_noise=True)
      res[form] = ({k: v.clone() for k, v in out.items()}, state_of(env))
      assert guard_share(out, form) <= MAX_GUARD_SHARE
  a, b = res['one_wave_packed'], res['two_wave']
  assert set(a[0]) == set(b[0]) == set(OUT_KEYS) | {'actions', 'eps'}
  for k in a[0]:
    same(a[0][k], b[0][k], k)
  same_state(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- 3. the actions are the contract
# every branch of the lane-group layer: widths below the group width (16), half-full k-tiles (48, 144), partial groups of 128 output rows (144), full width (256), one
# and two hidden layers; relu / tanh; no head / mean / sample; both log-std maps
CASES = [((16,), 'relu', None, 'clamp', 'one'), ((16,), 'tanh', 'sample', 'tanh', 'one'), ((48, 16), 'tanh', 'mean', 'clamp', 'one'),
         ((48, 16), 'relu', 'sample', 'clamp', 'one'), ((64, 64), 'relu', None, 'clamp', 'one'), ((64, 64), 'tanh', 'sample', 'tanh', 'one'),
         ((256,), 'tanh', None, 'clamp', 'one'), ((256,), 'relu', 'sample', 'clamp', 'one'), ((144, 256), 'relu', 'mean', 'tanh', 'one'),
         ((144, 256), 'tanh', 'sample', 'clamp', 'one'), ((256, 256), 'relu', None, 'clamp', 'one'), ((256, 256), 'tanh', 'sample', 'tanh', 'one'),
         ((256, 256), 'relu', 'sample', 'clamp', 'two')]


@pytest.mark.parametrize('hidden,hact,head,lmap,form', CASES, ids=[f'{"x".join(map(str, c[0]))}-{c[1]}-{c[2]}-{c[3]}-{c[4]}' for c in CASES])
def test_actions_are_the_contract_bit_for_bit(hidden, hact, head, lmap, form):
  """every action of the launch == earl_mlp_policy_forward_cpu on the float32 observation the step consumed"""
  seed, off = 11, 3
  n = 45 if form == 'one' else 32
  with launch_form(**(dict(solo=-1, duo=0) if form == 'one' else FORMS['two_wave'])):
    env = make('minitaur', n, seed=seed, env_offset=off)
    u = env.unwrapped
    pi, layers = policy(hidden, hact, head=head, log_std_map=lmap, seed=len(hidden) * 7 + hidden[0])
    env.rollout_policy(pi, 2)                                           # (the launch under test starts at a step counter that is not 0)
    step0 = u.total_step_count
    obs0 = u.last_obs.clone()
    kw = {} if head is None else {'sample': head == 'sample', 'return_noise': True}
    out = env.rollout_policy(pi, T12, **kw)
  eps = None
  if head is not None:
    eps = out['eps'].cpu().numpy()
    np.testing.assert_array_equal(eps.view(np.uint32), expected_eps(seed, off, n, step0, T12).view(np.uint32))       # written in both modes
  want = oracle_actions(layers, hact, obs0, out, head=head, lmap=lmap, eps=eps)
  got = out['actions'].cpu().numpy()
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  if head == 'sample':
    mean = oracle_actions(layers, hact, obs0, out, head='mean', lmap=lmap)
    assert (got != mean).mean() > 0.9                                   # ... and the noise is in the actions
  assert np.abs(got).max() > 1e-3 and len(np.unique(got[:, :, 0])) > T12 * n // 2
  assert guard_share(out, f'{hidden} {hact} {head} {form}') <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 4. a goal switch inside the launch
@pytest.mark.parametrize('form,n', [('one_wave_packed', 45), ('two_wave', 91)])
def test_goal_switch_inside_the_launch(form, n):
  import torch
  gcf = 5
  with launch_form(**FORMS[form]):
    env = make('minitaur', n, seed=12, gcf=gcf)
    u = env.unwrapped
    pi, layers = policy((64,), 'tanh', seed=5)
    env.rollout(torch.zeros(3, n, 8, device='cuda'))                    # the switch does not fall on a launch boundary
    obs0 = u.last_obs.clone()
    got = closed_equals_open(env, pi, T12)
  assert int(u.steps_since_goal_change[0]) == (3 + T12) % gcf
  goal = got['obs'][:, :, 30:]
  switched = (goal[1:] != goal[:-1]).any(-1).any(-1)
  assert bool(switched.any()), 'no goal switch changed entries 30 / 31 inside the launch'
  ts = int(switched.nonzero()[0]) + 1                                   # the first row emitted with switched goal entries; step ts + 1 consumes it
  assert ts + 1 < T12
  acts = got['actions'].cpu().numpy()
  np.testing.assert_array_equal(acts.view(np.uint32), oracle_actions(layers, 'tanh', obs0, got).view(np.uint32))      # ... the patched rows included
  obs = got['obs'].cpu().numpy()
  pre = np.concatenate([obs[ts, :, :30], obs[ts - 1, :, 30:]], -1).astype(np.float32)      # that row as it stood before the patch
  assert (acts[ts + 1] != forward_cpu(layers, 'tanh', 'tanh', pre)).any()                  # a policy fed the pre-patch row would have acted differently
  assert guard_share(got, form) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 5. the failure guard
def test_failure_guard_repeats_the_row_and_the_action():
  """the input of tests/test_minitaur_gpu.py::test_failure_guard_rolls_back_one_env (a NaN velocity in one env's state rows: the env sits in its guard, no GPU fault)"""
  n, T, bad = 8, 2, 3
  env, ref = make('minitaur', n, seed=4), make('minitaur', n, seed=4)
  pi, layers = policy((64, 64), 'relu', seed=2)
  env.qvel[bad, 7] = float('nan')
  last = env.last_obs.clone()
  ra, rb = env.rollout_policy(pi, T), ref.rollout_policy(pi, T)
  assert ra['status'][:, bad].tolist() == [1, 1] and int(ra['status'].sum()) == 2 and int(env.fail_count[bad]) == 2
  for t in range(T):
    same(ra['obs'][t, bad], last[bad], 'the rolled-back env repeats last_obs')
  want = forward_cpu(layers, 'relu', 'tanh', last.cpu().numpy().astype(np.float32))
  for t in range(T):
    np.testing.assert_array_equal(ra['actions'][t, bad].cpu().numpy().view(np.uint32), want[bad].view(np.uint32))
  keep = [i for i in range(n) if i != bad]
  for k in OUT_KEYS + ('actions',):
    same(ra[k][:, keep], rb[k][:, keep], k + ' of the neighbours')
  assert guard_share(rb, 'unpoisoned run') <= MAX_GUARD_SHARE and int(ra['status'][:, keep].sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 6. one launch == T launches
@pytest.mark.parametrize('head', [None, 'sample'])
def test_one_launch_of_T_equals_T_launches_of_one(head):
  import torch
  n = 45
  ea, eb = make('minitaur', n, seed=9, gcf=7), make('minitaur', n, seed=9, gcf=7)
  pi, _ = policy((64, 64), 'relu', head=head, seed=2)
  kw = {'return_noise': True} if head else {}
  one = ea.rollout_policy(pi, T12, **kw)
  rows = [{k: v.clone() for k, v in eb.rollout_policy(pi, 1, **kw).items()} for _ in range(T12)]
  for k in one:
    same(one[k], torch.cat([r[k] for r in rows]), k)
  # lifelong_return_t is the front end's float64 sum of the reward rows, the expression rollout() uses: one launch adds reward.sum(0) (torch's reduction order), T
  # launches add row by row.  Same rows (checked above), two summation orders: equal to the rounding of T additions, every other state tensor bit for bit
  sa, sb = state_of(ea), state_of(eb)
  same_state(sa, sb, skip=('lifelong_return_t',))
  bound = T12 * 2.0 ** -52 * one['reward'].abs().sum(0)
  assert bool(((sa[0]['lifelong_return_t'] - sb[0]['lifelong_return_t']).abs() <= bound).all())
  assert guard_share(one, f'head={head}') <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 7. shards
def test_two_shards_equal_the_batch():
  """eps, and with it everything else, depends on (seed, global env id, step counter) only"""
  import torch
  pi, _ = policy((64,), 'relu', head='sample', seed=1)
  full = make('minitaur', 48, seed=4).rollout_policy(pi, T12, return_noise=True)
  parts = [make('minitaur', 24, seed=4, env_offset=off).rollout_policy(pi, T12, return_noise=True) for off in (0, 24)]
  for k in full:
    same(full[k], torch.cat([p[k] for p in parts], dim=1), k)
  assert not torch.equal(parts[0]['eps'], parts[1]['eps'])
  assert guard_share(full, 'shards') <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 8. the stale first observation
def test_reset_goal_and_set_state_mark_last_obs_stale():
  import torch
  n = 16
  env = make('minitaur', n, seed=12)
  u = env.unwrapped
  pi, layers = policy((64,), 'tanh', seed=5)
  first = lambda obs: forward_cpu(layers, 'tanh', 'tanh', obs.cpu().numpy().astype(np.float32))
  out = env.rollout(torch.zeros(2, n, 8, device='cuda'))
  assert not u._last_obs_stale
  same(u._get_obs_t().contiguous(), u.last_obs, 'after a plain launch _get_obs() is last_obs')
  custom = torch.tensor([0.3, -0.1], dtype=torch.float64, device='cuda')
  u.reset_goal(custom.cpu().numpy())
  assert u._last_obs_stale and not bool((u.last_obs[:, 30:] == custom).all())
  obs0 = u._get_obs_t().clone()
  same(obs0[:, 30:].contiguous(), custom.expand(n, 2).contiguous(), 'the recomputed observation carries the new goal')
  sd = u.state_dict()
  assert sd['last_obs_stale'] is True
  out = env.rollout_policy(pi, 3)
  assert not u._last_obs_stale
  np.testing.assert_array_equal(out['actions'][0].cpu().numpy().view(np.uint32), first(obs0).view(np.uint32))
  same(out['obs'][0, :, 30:].contiguous(), custom.expand(n, 2).contiguous(), 'row 0 is emitted under the custom goal')
  # the flag travels with the dict: loaded, the env recomputes its first observation again and repeats the launch's first action
  u.load_state_dict(sd)
  assert u._last_obs_stale
  same(env.rollout_policy(pi, 1)['actions'][0], out['actions'][0], 'first action after load_state_dict')
  # a dict saved in the ordinary state clears the flag of a stale env; a dict written before the flag existed loads as not stale
  sd2 = u.state_dict()
  u.reset_goal(custom.cpu().numpy())
  u.load_state_dict(sd2)
  assert not u._last_obs_stale
  u.reset_goal(custom.cpu().numpy())
  u.load_state_dict({k: v for k, v in sd2.items() if k != 'last_obs_stale'})
  assert not u._last_obs_stale
  # set_state: the first action is the oracle's on the observation of the state that was set
  qpos, qvel = u.qpos.clone(), u.qvel.clone()
  qpos[:, 0] += 0.05
  u.set_state(qpos, qvel)
  assert u._last_obs_stale
  obs1 = u._get_obs_t().clone()
  assert not torch.equal(obs1, u.last_obs)
  out = env.rollout_policy(pi, 2)
  np.testing.assert_array_equal(out['actions'][0].cpu().numpy().view(np.uint32), first(obs1).view(np.uint32))
  u.reset_goal(custom.cpu().numpy())
  env.reset()
  assert not u._last_obs_stale                                          # a full reset rewrites every row
  assert guard_share(out, 'after set_state') <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 9. the Python surface
def test_rollout_policy_refuses_what_it_cannot_run():
  from earl_benchmark_amd import _abi
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  from earl_benchmark_amd.wrappers import LifelongWrapper
  n = 8
  env = make('minitaur', n)
  pi, layers = policy((16,), seed=0)
  with pytest.raises(ValueError, match='need a GaussianMLPPolicy'):
    env.rollout_policy(pi, 3, sample=False)
  with pytest.raises(ValueError, match='need a GaussianMLPPolicy'):
    env.rollout_policy(pi, 3, return_noise=True)
  with pytest.raises(ValueError, match='the policy is on cpu'):
    env.rollout_policy(MLPPolicy(layers, 'relu', 'tanh', obs_dim=32, act_dim=8), 3)
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    env.rollout_policy(MLPPolicy(random_layers([14, 16, 4], seed=0), device='cuda', obs_dim=14, act_dim=4), 3)
  with pytest.raises(ValueError, match="out_act='none'.*unbounded"):
    env.rollout_policy(MLPPolicy(layers, 'relu', 'none', device='cuda', obs_dim=32, act_dim=8), 3)
  glayers = random_layers([32, 16, 16], seed=0, last_gain=LAST_GAIN)
  with pytest.raises(ValueError, match='squash=False.*unbounded'):
    env.rollout_policy(GaussianMLPPolicy(glayers, squash=False, device='cuda', obs_dim=32, act_dim=8), 3)
  with pytest.raises(ValueError, match='T = 0'):
    env.rollout_policy(pi, 0)
  with pytest.raises((NotImplementedError, ValueError), match='PolicyPopulation on the minitaur'):
    env.rollout_policy(PolicyPopulation([pi, pi], envs_per_policy=16, device='cuda', obs_dim=32, act_dim=8), 3)
  pair = AgentPair(pi, pi, backward_goal=None, device='cuda', obs_dim=32, act_dim=8)
  with pytest.raises((NotImplementedError, ValueError), match='AgentPair on the minitaur'):
    env.rollout_policy(pair, 3)
  with pytest.raises((NotImplementedError, ValueError), match='AgentPair on the minitaur'):
    env.rollout_agents(pair, 3)
  with pytest.raises((NotImplementedError, ValueError), match='on the minitaur'):
    env.evaluate_policy(pi, 3)
  n0 = int(env.interventions.sum())
  out = env.rollout_policy(pi, 3, reset_first=True)
  assert int(env.interventions.sum()) == n0 + n and tuple(out['obs'].shape) == (3, n, 32) and int(env.steps_since_reset[0]) == 3
  assert guard_share(out, 'reset_first') <= MAX_GUARD_SHARE
  # the generic-stepper comparison build has no policy form: an argument error, not a silent other kernel
  lib = _abi.load()
  assert lib.earl_debug_set_minitaur_stepper(0) == 0
  try:
    with pytest.raises(_abi.EarlHipError):
      env.rollout_policy(pi, 3)
  finally:
    assert lib.earl_debug_set_minitaur_stepper(1) == 0
  # the wrappers forward the call, and the lifelong one switches goals inside it
  lenv = LifelongWrapper(make('minitaur', n, seed=2), 3)
  out = lenv.rollout_policy(pi, 7)
  goal = out['obs'][:, :, 30:]
  assert bool((goal[1:] != goal[:-1]).any()) and int(lenv.unwrapped.steps_since_goal_change[0]) == 7 % 3 and float(lenv.lifelong_return.abs().sum()) > 0
  assert guard_share(out, 'lifelong') <= MAX_GUARD_SHARE

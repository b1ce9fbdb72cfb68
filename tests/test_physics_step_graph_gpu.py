"""make_step_graph on the physics envs (envs/physics_step_graph.py) and the clocked rollout entry points behind it (include/earl_physics.h
earl_*_rollout_clocked): a replay of T captured T = 1 launches returns what T eager step() calls return, bit for bit, and leaves the same state --
across replays (the counters the draws use are read from a device clock the host refreshes before every replay), with lifelong goal switches
inside and across replays, with a policy captured between the steps, and interleaved with eager steps."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

A_DIM = {'door': 4, 'peg': 4, 'kitchen': 9, 'minitaur': 8}
STATE = {'door': ('qpos', 'qvel', 'mocap_pos', 'goal_t', 'steps_since_reset', 'steps_since_goal_change', 'last_obs', 'fail_count', 'lifelong_return_t'),
         'kitchen': ('qpos', 'qvel', 'mocap_pos', 'last_qp_robot', 'att', 'steps_since_reset', 'last_obs', 'fail_count'),
         'minitaur': ('qpos', 'qvel', 'goal_t', 'observed_torque', 'overheat', 'motor_enabled', 'steps_since_reset', 'steps_since_goal_change', 'last_obs',
                      'fail_count', 'lifelong_return_t')}
STATE['peg'] = STATE['door'] + ('obj_init',)


def make(kind, n, seed=3, gcf=0, **kw):
  if kind == 'door':
    from earl_benchmark_amd.envs.sawyer_door import SawyerDoor as cls
  elif kind == 'peg':
    from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg as cls
  elif kind == 'kitchen':
    from earl_benchmark_amd.envs.kitchen import Kitchen as cls
  else:
    from earl_benchmark_amd.envs.minitaur import Minitaur as cls
  env = cls(num_envs=n, seed=seed, scalar_api=False, **kw)
  if gcf:
    from earl_benchmark_amd.wrappers import LifelongWrapper
    env = LifelongWrapper(env, gcf)
  return env


def bits(x):
  import torch
  if x.dtype == torch.float64:
    return x.view(torch.int64)
  if x.dtype == torch.float32:
    return x.view(torch.int32)
  return x


def same(x, y, what):
  import torch
  assert x.shape == y.shape and x.dtype == y.dtype, what
  assert torch.equal(bits(x.contiguous()), bits(y.contiguous())), what


def rand_actions(T, n, a, seed):
  import torch
  g = torch.Generator(device='cuda').manual_seed(seed)
  return (torch.rand(T, n, a, generator=g, device='cuda') * 2 - 1).to(torch.float32)


def eager(env, acts):
  """T eager step() calls -> dict of stacked [T, N, ...] outputs and a dict of stacked info entries"""
  import torch
  rows = [env.step(acts[t]) for t in range(acts.shape[0])]
  res = {'obs': torch.stack([r[0] for r in rows]), 'reward': torch.stack([r[1] for r in rows]), 'done': torch.stack([r[2] for r in rows])}
  info = {k: torch.stack([r[3][k] for r in rows]) for k in rows[0][3] if torch.is_tensor(rows[0][3][k])}
  return res, info


def compare(kind, ea, eb, res, info, g_out, g_info):
  for k in ('obs', 'reward', 'done'):
    same(res[k], g_out[k], k)
  for k in g_info:
    same(info[k], g_info[k], 'info ' + k)
  compare_state(kind, ea, eb)


def compare_state(kind, ea, eb):
  ua, ub = ea.unwrapped, eb.unwrapped
  for k in STATE[kind]:
    same(getattr(ua, k), getattr(ub, k), k)
  assert ua.total_step_count == ub.total_step_count
  if kind in ('door', 'peg'):
    assert int(ua._cfg.counter) == int(ub._cfg.counter)
  else:
    assert ua._counter == ub._counter
  same(ua._last_success, ub._last_success, '_last_success')


@pytest.mark.parametrize('kind', ['door', 'peg', 'kitchen', 'minitaur'])
def test_ring_replay_equals_eager_stepping_bit_for_bit(kind):
  n, T = 13, 4
  kw = {'sensor_noise': True} if kind == 'kitchen' else {}
  ea, eb = make(kind, n, seed=7, **kw), make(kind, n, seed=7, **kw)
  g = eb.make_step_graph(T)
  assert eb.unwrapped.total_step_count == 0                      # building the graph steps nothing
  for rep in range(2):                                           # the second replay uses the clock refreshed from the advanced counters
    acts = rand_actions(T, n, A_DIM[kind], 11 + rep)
    res, info = eager(ea, acts)
    g.actions.copy_(acts)
    obs, rew, done, g_info = g.replay()
    assert set(g_info) == set(info) or kind == 'kitchen'
    assert {'success', 'status'} <= set(g_info) or {'is_successful', 'status'} <= set(g_info)
    compare(kind, ea, eb, res, info, {'obs': obs, 'reward': rew, 'done': done}, {k: v for k, v in g_info.items() if k in info})
    assert eb.unwrapped.total_step_count == (rep + 1) * T


def test_kitchen_second_replay_draws_fresh_sensor_noise():
  """the kitchen's noise counter advances across replays: two replays of the SAME actions from the same state differ in their noise"""
  import torch
  n, T = 5, 2
  env = make('kitchen', n, seed=4, sensor_noise=True)
  g = env.make_step_graph(T)
  snap = env.state_dict()
  o1 = g.replay()[0].clone()
  env.load_state_dict(snap)                                       # the same state, counter included ...
  assert torch.equal(g.replay()[0], o1)                           # ... the same draws
  env.load_state_dict(snap)
  env._counter = snap['counter'] + T                              # the same state on the counter the replay after it would see
  o2 = g.replay()[0]
  assert not torch.equal(o1, o2)                                  # a frozen counter would repeat the first replay's draws
  assert torch.equal(o1[:, :, 23:], o2[:, :, 23:])                # (the goal block carries no noise)


@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur'])
def test_lifelong_goal_switches_inside_and_across_replays(kind):
  n, T, gcf = 11, 8, 3
  kw = {'reset_at_goal': True} if kind == 'peg' else {}         # (the peg's reset-at-goal table has 15 goal rows: the switch draw shows)
  ea, eb = make(kind, n, seed=9, gcf=gcf, **kw), make(kind, n, seed=9, gcf=gcf, **kw)
  g = eb.make_step_graph(T)
  for rep in range(2):
    acts = rand_actions(T, n, A_DIM[kind], 21 + rep)
    res, info = eager(ea, acts)
    g.actions.copy_(acts)
    obs, rew, done, g_info = g.replay()
    assert set(g_info) == set(info)                               # (door: the seven evaluate_state slots, incl. the pre-switch target on switch rows)
    compare(kind, ea, eb, res, info, {'obs': obs, 'reward': rew, 'done': done}, g_info)
  same(ea.unwrapped.lifelong_return_t, eb.unwrapped.lifelong_return_t, 'lifelong_return_t')
  if kind == 'minitaur':                                          # (dense reward: the sum shows; the Sawyer envs' sparse reward is 0 on random actions)
    assert bool((ea.unwrapped.lifelong_return_t != 0).any())
  if kind != 'door':                                              # (the door's one-row goal table switches to the same goal)
    import torch
    assert bool((torch.diff(res['obs'][:, :, -2:], dim=0) != 0).any())


def mlp(d_in, d_out, seed):
  import torch
  gen = torch.Generator(device='cuda').manual_seed(seed)
  w1 = torch.randn(d_in, 32, generator=gen, device='cuda') * 0.3
  w2 = torch.randn(32, d_out, generator=gen, device='cuda') * 0.3

  def pi(ob):
    return torch.tanh(torch.tanh(ob.to(torch.float32) @ w1) @ w2)
  return pi


@pytest.mark.parametrize('kind', ['door', 'minitaur'])
def test_policy_in_the_loop_equals_eager_bit_for_bit(kind):
  import torch
  n, T = 9, 5
  ea, eb = make(kind, n, seed=5), make(kind, n, seed=5)
  d = ea.unwrapped.OBS_DIM
  pi = mlp(d, A_DIM[kind], 17)
  obs = ea.unwrapped.last_obs.clone()
  g = eb.make_step_graph(T, policy=pi)
  for rep in range(2):
    rows = []
    for t in range(T):
      obs, rew, done, info = ea.step(pi(obs))
      rows.append((obs.clone(), rew.clone(), done.clone()))
    g_obs, g_rew, g_done, _ = g.replay()
    torch.cuda.synchronize()
    same(torch.stack([r[0] for r in rows]), g_obs, 'obs')
    same(torch.stack([r[1] for r in rows]), g_rew, 'reward')
    same(torch.stack([r[2] for r in rows]), g_done, 'done')
    same(g.obs_in, obs, 'obs_in')
  compare_state(kind, ea, eb)


@pytest.mark.parametrize('kind', ['peg', 'minitaur'])
def test_eager_steps_and_replays_interleave(kind):
  n, T = 7, 3
  kw = {'reset_at_goal': True} if kind == 'peg' else {}
  ea, eb = make(kind, n, seed=12, gcf=2, **kw), make(kind, n, seed=12, gcf=2, **kw)
  g = eb.make_step_graph(T)
  acts = rand_actions(2 * T + 2, n, A_DIM[kind], 31)
  res, _ = eager(ea, acts)
  o0 = eb.step(acts[0])[0].clone()
  g.actions.copy_(acts[1:1 + T])
  o1 = g.replay()[0].clone()
  o2 = eb.step(acts[1 + T])[0].clone()
  g.actions.copy_(acts[2 + T:])
  o3 = g.replay()[0].clone()
  same(res['obs'][0], o0, 'eager 0')
  same(res['obs'][1:1 + T], o1, 'replay 1')
  same(res['obs'][1 + T], o2, 'eager 1')
  same(res['obs'][2 + T:], o3, 'replay 2')
  assert eb.unwrapped.total_step_count == 2 * T + 2
  compare_state(kind, ea, eb)


# ---------------------------------------------------------------------------------------------------- the C entry points
def goal_rows(k, seed):
  import torch
  gen = torch.Generator(device='cuda').manual_seed(seed)
  return (torch.rand(k, 7, generator=gen, device='cuda', dtype=torch.float64) * 0.1 + 0.3).contiguous()


def sawyer_call(env, acts, out, clock, clocked):
  from earl_benchmark_amd import _abi
  u = env
  o = _abi.SawyerOut(obs=out['obs'].data_ptr(), reward=out['reward'].data_ptr(), done=out['done'].data_ptr(), success=out['success'].data_ptr(),
                     status=out['status'].data_ptr(), info=out['info'].data_ptr())
  args = (u.model.buf.data_ptr(), u.model.col_ptr, u.nv, u._cfg_ref, u._st_ref, acts.data_ptr(), acts.shape[0])
  if clocked:
    rc = u._lib.earl_sawyer_rollout_clocked(*args, clock, C.byref(o), u._stream())
  else:
    rc = u._lib.earl_sawyer_rollout(*args, C.byref(o), u._stream())
  _abi.check(rc, 'sawyer')


def kitchen_call(env, acts, out, clock, clocked):
  from earl_benchmark_amd import _abi
  u = env
  o = _abi.KitchenOut(obs=out['obs'].data_ptr(), reward=out['reward'].data_ptr(), done=out['done'].data_ptr(), success=out['success'].data_ptr(),
                      status=out['status'].data_ptr())
  args = (u.model.buf.data_ptr(), u.model.col_ptr, C.byref(u._params), C.byref(u._cfg), C.byref(u._st), acts.data_ptr(), acts.shape[0])
  if clocked:
    rc = u._lib.earl_kitchen_rollout_clocked(*args, clock, C.byref(o), u._stream())
  else:
    rc = u._lib.earl_kitchen_rollout(*args, C.byref(o), u._stream())
  _abi.check(rc, 'kitchen')


def minitaur_call(env, acts, out, clock, clocked):
  from earl_benchmark_amd import _abi
  u = env
  o = _abi.MinitaurOut(obs=out['obs'].data_ptr(), reward=out['reward'].data_ptr(), done=out['done'].data_ptr(), success=out['success'].data_ptr(),
                       status=out['status'].data_ptr())
  args = (u.model.buf.data_ptr(), u.model.col_ptr, C.byref(u._cfg), C.byref(u._st), acts.data_ptr(), acts.shape[0])
  if clocked:
    rc = u._lib.earl_minitaur_rollout_clocked(*args, clock, C.byref(o), u._stream())
  else:
    rc = u._lib.earl_minitaur_rollout(*args, C.byref(o), u._stream())
  _abi.check(rc, 'minitaur')


def set_counters(kind, env, c0, c1):
  env._cfg.counter = c0
  if kind != 'kitchen':
    env._cfg.step_counter = c1


def abi_case(kind, n, T, switch=None):
  """three identical envs: old entry point with counters (B0, B1); clocked with NULL and the same counters; clocked with clock {B0, B1} and counters 0"""
  import torch
  from earl_benchmark_amd import _abi
  lib = _abi.load()
  call = {'door': sawyer_call, 'kitchen': kitchen_call, 'minitaur': minitaur_call}[kind]
  B0, B1 = 1000003, (1 << 40) + 77
  envs, outs = [], []
  for _ in range(4):
    e = make(kind, n, seed=2, **({'sensor_noise': True} if kind == 'kitchen' else {}))
    if kind == 'door':                                      # a goal table of several rows: the goal-switch draw shows in the observation
      e._rows = goal_rows(6, 1)
      e._cfg.n_goal_rows, e._cfg.goal_table = 6, e._rows.data_ptr()
    if kind != 'kitchen':
      e._cfg.goal_change_frequency = 2
    envs.append(e)
    outs.append((e._new_out((T,)) if kind != 'kitchen' else e._new_graph_out(T)))
    if kind == 'door':
      outs[-1]['info'].zero_()
  acts = rand_actions(T, n, A_DIM[kind], 41)
  clock = torch.tensor([B0, B1], dtype=torch.int64, device='cuda')
  if switch:
    switch(lib, True)
  try:
    set_counters(kind, envs[0], B0, B1)
    call(envs[0], acts, outs[0], None, False)
    set_counters(kind, envs[1], B0, B1)
    call(envs[1], acts, outs[1], None, True)
    set_counters(kind, envs[2], 0, 0)
    call(envs[2], acts, outs[2], clock.data_ptr(), True)
    set_counters(kind, envs[3], 0, 0)                       # (the same without the clock: must differ, or the case shows nothing)
    call(envs[3], acts, outs[3], None, True)
    torch.cuda.synchronize()
  finally:
    if switch:
      switch(lib, False)
  for k in outs[0]:
    same(outs[0][k], outs[1][k], f'{kind} NULL clock: {k}')
    same(outs[0][k], outs[2][k], f'{kind} clock words: {k}')
  assert not torch.equal(outs[0]['obs'], outs[3]['obs']), f'{kind}: the counters do not show at this size'
  for k in STATE[kind]:
    if k != 'lifelong_return_t':
      same(getattr(envs[0], k), getattr(envs[2], k), f'{kind} state {k}')


def test_clocked_sawyer_entry_point_default_and_eight_wave_door():
  abi_case('door', 37, 6)                                   # four single-wave workgroups per CU
  abi_case('door', 4100, 4)                                 # > 4096 envs: the eight-wave build (csrc/physics_w8.hip)


def test_clocked_sawyer_entry_point_64_lanes_per_env():
  def lanes(lib, on):
    assert lib.earl_debug_set_physics_lanes(64 if on else 16) == 0
  abi_case('door', 21, 4, lanes)


@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_clocked_kitchen_entry_point_in_every_launch_mode(mode):
  def solo(lib, on):
    lib.earl_debug_set_solo(mode if on else -1)
  abi_case('kitchen', 5, 3, solo)


@pytest.mark.parametrize('form', ['duo', 'one_wave', 'generic'])
def test_clocked_minitaur_entry_point_in_every_kernel(form):
  def pick(lib, on):
    if form == 'duo':
      lib.earl_debug_set_minitaur_duo(1 if on else -1)
    elif form == 'one_wave':
      lib.earl_debug_set_minitaur_duo(0 if on else -1)
    else:
      assert lib.earl_debug_set_minitaur_stepper(0 if on else 1) == 0
  abi_case('minitaur', 1100 if form != 'generic' else 19, 4, pick)     # (1100 > 4 x CUs: packed launches, where the duo switch applies)


# ---------------------------------------------------------------------------------------------------- refusals
def test_kitchen_graph_refuses_lifelong_goal_switching():
  env = make('kitchen', 3, gcf=5)
  with pytest.raises(ValueError, match='goal'):
    env.make_step_graph(2)


def test_minitaur_out_of_bounds_policy_is_flagged_and_check_actions_raises():
  import torch
  n, T = 4, 3
  env = make('minitaur', n)

  def pi(ob):
    a = torch.zeros(ob.shape[0], 8, device=ob.device)
    a[:, 5] = 2.0
    return a
  g = env.make_step_graph(T, policy=pi)
  g.replay()
  assert bool(g.action_out_of_bounds.all())
  with pytest.raises(ValueError, match=r'^5th action out of bounds\.$'):
    g.check_actions()
  ok = make('minitaur', n).make_step_graph(T)                # a ring of in-range actions: nothing to report
  ok.replay()
  assert not bool(ok.action_out_of_bounds.any())
  ok.check_actions()


def test_scalar_api_is_refused():
  from earl_benchmark_amd.envs.minitaur import Minitaur
  env = Minitaur(num_envs=1, scalar_api=True)
  with pytest.raises(ValueError, match='batched'):
    env.make_step_graph(2)

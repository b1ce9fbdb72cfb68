"""env.rollout_agents on the Sawyer door and peg (include/earl_physics.h: earl_sawyer_pair_rollout): the forward and the reset agent alternating inside ONE launch of
the rollout kernel.  The oracles use only entry points that existed before the pair (rollout, rollout_policy, earl_mlp_policy_forward_cpu) and numpy:
  4. the handover rule (tests/pair_helpers.handover_rule on the launch's own success), from staggered phase state, all four handover causes and mixed waves;
  5. the actions are the contract: row agent[t]'s network on float32(obs[t - 1]), bit for bit, eps independent of the phase;
  6. one pair launch == the step-by-step procedure of rollout(actions[t:t+1]) launches with the goal rows written by the test;
  7. never switching == rollout_policy of the phase's agent;  8. one launch of T == T launches of one;  9. two shards == the batch;
 10. every output pointer NULL leaves the same state;  11. the Python surface.
Shapes: T = 23, door 64 (one-wave build) and 4160 (eight-wave build), peg 64 and 4160 (time-sliced schedule, slices of 10 steps), switch_every = (5, 3): handovers fall
inside and across slices."""
import ctypes as C

import numpy as np
import pytest

from pair_helpers import assert_bits, handover_rule
from test_physics_step_graph_gpu import STATE, make, same
from test_sawyer_policy_rollout import forward_cpu
from test_sawyer_policy_rollout_gpu import MAX_GUARD_SHARE, expected_eps, guard_share, policy

pytestmark = pytest.mark.gpu

T = 23
SE = (5, 3)
SHAPES = [('door', 64), ('door', 4160), ('peg', 64), ('peg', 4160)]
GOAL_DRAW = 0xFFFE
OUT_KEYS = ('obs', 'reward', 'done', 'success', 'status', 'info')


def make_env(kind, n, seed=5, **kw):
  """the peg with reset_at_goal: its goal table has 15 rows, so a forward entry's draw is visible"""
  env = make(kind, n, seed=seed, **(dict(reset_at_goal=True) if kind == 'peg' else {}), **kw)
  u = env.unwrapped
  if kind == 'door' and n > 64:
    assert n > 4096                                                       # the launcher's condition for the eight-wave build (csrc/physics.hip)
  if kind == 'peg' and n > 64:
    import torch
    assert u._uses_queue(T) and (n + 15) // 16 > torch.cuda.get_device_properties(0).multi_processor_count and T >= 21      # the time-sliced schedule, slices of 10
  return env


def make_pair(hidden=(64, 64), head=None, seed=0, switch_every=SE, sos=False, goal=None):
  from earl_benchmark_amd.policy import AgentPair
  (pf, lf), (pb, lb) = policy(hidden, 'relu', 'tanh', head=head, seed=seed), policy(hidden, 'relu', 'tanh', head=head, seed=seed + 1)
  return AgentPair(pf, pb, switch_every=switch_every, switch_on_success=sos, backward_goal=goal, obs_dim=14, act_dim=4), (lf, lb)


def stagger(u, offset=0):
  """hand-set phase state: phase = i % 2, steps_in_phase = i % 3 by GLOBAL index -- every 4-env wave is mixed"""
  import torch
  i = torch.arange(u.num_envs, device='cuda') + offset
  u.agent_phase, u.steps_in_phase = (i % 2).to(torch.int8), (i % 3).to(torch.int32)
  return u.agent_phase.cpu().numpy().copy(), u.steps_in_phase.cpu().numpy().copy()


def reset_row(u):
  """a backward goal built from env 0's reset observation: hand, gripper and object where the reset left them"""
  return u.last_obs[0, :7].clone()


def host(out):
  return {k: v.cpu().numpy() for k, v in out.items()}


def guard_share_host(out):
  """guard_share of a dict of numpy arrays"""
  return float((out['status'] != 0).mean())


def state_of(u):
  return {k: getattr(u, k).clone() for k in STATE['peg' if u.nv >= 15 else 'door']}


def same_state(a, b):
  for k in a:
    same(a[k], b[k], k)


def goal_draw(u, step):
  """the lifelong switch's draw of env step `step` (the env's total step count before the step) for every env -> table rows [n, 7]: Philox block {0xFFFE, global id, ev},
  u01 = (y:x >> 11) 2^-53, index = min(int(u01 rows), rows - 1)"""
  from gaussian_policy_helpers import philox4x32_10
  n, seed, rows = u.num_envs, int(u._cfg.seed), int(u._cfg.n_goal_rows)
  gid = np.uint64(int(u._cfg.env_offset)) + np.arange(n, dtype=np.uint64)
  ev = np.full(n, step, np.uint64)
  x, y, _, _ = philox4x32_10(np.full(n, GOAL_DRAW, np.uint64), gid, ev & np.uint64(0xFFFFFFFF), ev >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
  u01 = (((y << np.uint64(32)) | x) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
  idx = np.minimum((u01 * float(rows)).astype(np.int64), rows - 1)
  return u._goal_table.cpu().numpy()[idx], idx


def mixed_waves(agent):
  a = agent[:, :agent.shape[1] // 4 * 4].reshape(agent.shape[0], -1, 4)
  return int(((a == 0).any(-1) & (a == 1).any(-1)).sum())


# ---------------------------------------------------------------------------------------------------------------- 4. the handover rule
@pytest.mark.parametrize('kind,n', SHAPES)
@pytest.mark.parametrize('head', [None, 'sample'])
def test_handover_rule_from_staggered_phase_state(kind, n, head):
  """agent, final phase / steps_in_phase and both counters == the contract's item 5 applied to the launch's own success, for: the clocks only (switch_on_success = 0),
  every stable step a success (radius 1e3), no success (radius 0), and the env's own radius with the backward goal where the reset left the env"""
  env = make_env(kind, n)
  u = env.unwrapped
  own = float(u._cfg.success_radius)
  row = reset_row(u)
  sd = u.state_dict()
  total = np.zeros(4, np.int64)
  mixed = 0
  for sos, radius, goal in ((False, own, None), (True, 1e3, None), (True, 0.0, None), (True, own, row)):
    u.load_state_dict(sd)
    ph0, sip0 = stagger(u)
    u._cfg.success_radius = radius
    pair, _ = make_pair(head=head, seed=n, sos=sos, goal=goal)
    out = host(env.rollout_agents(pair, T))
    u._cfg.success_radius = own
    agent, ph, sip, fs, bs, causes = handover_rule(out['success'][None], np.zeros((1, T, n), bool), ph0, sip0, SE, sos, False, False)
    got = dict(agent=out['agent'], phase=u.agent_phase.cpu().numpy(), sip=u.steps_in_phase.cpu().numpy(), fs=u.pair_counts[0].cpu().numpy(), bs=u.pair_counts[1].cpu().numpy())
    assert_bits(got, dict(agent=agent[0], phase=ph, sip=sip, fs=fs[0], bs=bs[0]), ('agent', 'phase', 'sip', 'fs', 'bs'))
    if radius == 1e3:
      assert out['success'][out['status'] == 0].all()
    if radius == 0.0:
      assert not out['success'].any()
    total += causes
    mixed += mixed_waves(out['agent'])
    print(f'{kind} n={n} head={head} sos={sos} radius={radius}: causes {causes.tolist()} guard share {guard_share_host(out):.5f}')
    assert guard_share_host(out) <= MAX_GUARD_SHARE
  assert (total > 0).all(), total                                         # forward by success, forward by clock, reset by success, reset by clock
  assert mixed > 0


# ---------------------------------------------------------------------------------------------------------------- 5. the actions are the contract
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('hidden,head', [((64, 64), None), ((64, 64), 'sample'), ((16,), None)], ids=['64x64', '64x64-sample', '16'])
def test_actions_are_the_contract_per_phase(kind, hidden, head):
  from earl_benchmark_amd import _abi
  n, seed, off = 64, 11, 3
  env = make_env(kind, n, seed=seed, env_offset=off)
  u = env.unwrapped
  pair, layers = make_pair(hidden, head, seed=7, sos=True, goal=reset_row(u))
  env.rollout_agents(pair, 2)                                             # (the launch under test starts at a step counter that is not 0)
  stagger(u)
  step0, obs0 = u.total_step_count, u.last_obs.clone()
  out = host(env.rollout_agents(pair, T, **({'return_noise': True} if head else {})))
  x = np.concatenate([obs0.cpu().numpy()[None], out['obs'][:-1]]).astype(np.float32).reshape(T * n, 14)
  hd = eps = None
  if head:
    hd = (1, _abi.LOGSTD_MAPS['clamp'], -5.0, 2.0)
    eps = out['eps'].reshape(T * n, 4)
    np.testing.assert_array_equal(out['eps'].view(np.uint32), expected_eps(seed, off, n, step0, T).view(np.uint32))      # (independent of the phase)
  want = np.stack([forward_cpu(layers[k], 'relu', 'tanh', x, head=hd, eps=eps).reshape(T, n, 4) for k in range(2)])
  agent = out['agent'].astype(np.int64)
  assert set(np.unique(agent)) == {0, 1} and mixed_waves(out['agent']) > 0
  sel = np.where(agent[..., None] == 1, want[1], want[0])
  np.testing.assert_array_equal(out['actions'].view(np.uint32), sel.view(np.uint32))
  assert (want[0] != want[1]).mean() > 0.9                                # (the agents differ: the wrong row would show)
  assert (out['obs'][1:, :, 7:] != out['obs'][:-1, :, 7:]).any(), 'no handover changed the goal block the next action saw'
  assert guard_share_host(out) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 6. pair launch == step-by-step procedure
@pytest.mark.parametrize('kind,n', SHAPES)
@pytest.mark.parametrize('head', [None, 'sample'])
def test_pair_launch_equals_the_step_by_step_procedure(kind, n, head):
  """T launches of rollout(actions[t:t+1]); after step t the test hands over by the rule and writes goal_t and last_obs[:, 7:] of the envs that changed goal (the
  backward row, or the table row of the 0xFFFE draw recomputed on the host), clearing the stale flag by hand (reset_goal() would have the observation recomputed)."""
  import torch
  env = make_env(kind, n, seed=8)
  u = env.unwrapped
  row = reset_row(u)
  pair, _ = make_pair(head=head, seed=3, sos=True, goal=row)
  env.rollout(torch.zeros(2, n, 4, device='cuda'))                       # (step counter not 0)
  sd = u.state_dict()
  ph, sip = stagger(u)
  step0 = u.total_step_count
  got = host(env.rollout_agents(pair, T))
  end, end_phase, end_sip = state_of(u), u.agent_phase.cpu().numpy(), u.steps_in_phase.cpu().numpy()
  fs_got, bs_got = (c.cpu().numpy() for c in u.pair_counts)
  assert (kind == 'peg') == ('info' in got)
  u.load_state_dict(sd)
  actions = torch.as_tensor(got['actions'], device='cuda')
  row_h = row.cpu().numpy()
  ph, sip = ph.astype(np.int64), sip.astype(np.int64)
  fs, bs = np.zeros(n, np.int32), np.zeros(n, np.int32)
  forward_changed = 0
  for t in range(T):
    np.testing.assert_array_equal(got['agent'][t], ph)
    r = host(env.rollout(actions[t:t + 1]))
    s = r['success'][0].astype(bool)
    sip += 1
    over = s | (sip >= np.array(SE)[ph])
    fs += over & s & (ph == 0)
    bs += over & s & (ph == 1)
    ph = np.where(over, ph ^ 1, ph)
    sip = np.where(over, 0, sip)
    table, _ = goal_draw(u, step0 + t)
    new = np.where((ph == 1)[:, None], row_h[None], table)
    before = u.goal_t.cpu().numpy()
    forward_changed += int((over & (ph == 0) & (new != before).any(-1)).sum())
    m = torch.as_tensor(over, device='cuda')
    rows = torch.as_tensor(new, device='cuda')
    u.goal_t[m] = rows[m]
    u.last_obs[m, 7:] = rows[m]
    u._last_obs_stale = False
    r['obs'][0][over, 7:] = new[over]
    for k in OUT_KEYS:
      if k in got:
        assert_bits({k: got[k][t]}, {k: r[k][0]}, (k,))
  same_state(end, state_of(u))
  np.testing.assert_array_equal(end_phase, ph)
  np.testing.assert_array_equal(end_sip, sip)
  np.testing.assert_array_equal(fs_got, fs)
  np.testing.assert_array_equal(bs_got, bs)
  if kind == 'peg':
    assert u._cfg.n_goal_rows > 1 and forward_changed > 0, 'no forward entry changed the goal block'
  assert guard_share_host(got) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 7. never switching
@pytest.mark.parametrize('kind,n', [('door', 4160), ('peg', 4160)])
@pytest.mark.parametrize('phase,head', [(0, None), (1, 'sample')])
def test_never_switching_equals_the_single_policy_launch(kind, n, phase, head):
  import torch
  env = make_env(kind, n, seed=9)
  u = env.unwrapped
  pair, _ = make_pair(head=head, seed=4, switch_every=T + 1, sos=False, goal=None)
  sd = u.state_dict()
  kw = {'return_noise': True} if head else {}
  want = {k: v.clone() for k, v in env.rollout_policy(pair.agent(phase), T, **kw).items()}
  want_state, want_last = state_of(u), u._last_success.clone()
  u.load_state_dict(sd)
  u.agent_phase = torch.full((n,), phase, dtype=torch.int8, device='cuda')
  u.steps_in_phase = torch.zeros(n, dtype=torch.int32, device='cuda')
  got = env.rollout_agents(pair, T, **kw)
  for k in OUT_KEYS + ('actions', 'eps'):
    if k == 'info' and kind == 'door':
      assert 'info' not in got
    elif k in want:
      same(got[k], want[k], k)
  same_state(state_of(u), want_state)
  same(u._last_success, want_last, '_last_success')
  assert bool((got['agent'] == phase).all()) and bool((u.agent_phase == phase).all()) and bool((u.steps_in_phase == T).all())
  assert int(u.pair_counts[0].sum()) == 0 and int(u.pair_counts[1].sum()) == 0
  assert guard_share(got) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 8. one launch == T launches
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('head', [None, 'sample'])
def test_one_launch_of_T_equals_T_launches_of_one(kind, head):
  import torch
  n = 40
  ea, eb = make_env(kind, n, seed=9), make_env(kind, n, seed=9)
  pair, _ = make_pair(head=head, seed=2, sos=True, goal=reset_row(ea.unwrapped))
  kw = {'return_noise': True} if head else {}
  stagger(ea.unwrapped)
  stagger(eb.unwrapped)
  one = ea.rollout_agents(pair, T, **kw)
  rows, fs, bs = [], 0, 0
  for _ in range(T):
    rows.append({k: v.clone() for k, v in eb.rollout_agents(pair, 1, **kw).items()})
    fs, bs = fs + eb.unwrapped.pair_counts[0], bs + eb.unwrapped.pair_counts[1]
  for k in one:
    same(one[k], torch.cat([r[k] for r in rows]), k)
  ua, ub = ea.unwrapped, eb.unwrapped
  same_state(state_of(ua), state_of(ub))
  same(ua.agent_phase, ub.agent_phase, 'phase')
  same(ua.steps_in_phase, ub.steps_in_phase, 'steps_in_phase')
  same(ua.pair_counts[0], fs, 'forward_success')
  same(ua.pair_counts[1], bs, 'backward_success')
  assert int(ua.pair_counts[0].sum() + ua.pair_counts[1].sum()) > 0 and guard_share(one) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 9. shards
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_two_shards_equal_the_batch(kind):
  import torch
  n, cut = 64, 26                                                         # (a cut inside a wave)
  whole, parts = make_env(kind, n, seed=4), [make_env(kind, cut, seed=4), make_env(kind, n - cut, seed=4, env_offset=cut)]
  sd = whole.unwrapped.state_dict()
  for p, (a, b) in zip(parts, ((0, cut), (cut, n))):                     # the shards start from the batch's rows
    p.unwrapped.load_state_dict({k: (v[a:b].clone() if torch.is_tensor(v) else v) for k, v in sd.items()})
  pair, _ = make_pair(head='sample', seed=6, sos=True, goal=reset_row(whole.unwrapped))
  stagger(whole.unwrapped)
  out = whole.rollout_agents(pair, T, return_noise=True)
  outs = []
  for p, off in zip(parts, (0, cut)):
    stagger(p.unwrapped, off)
    outs.append(p.rollout_agents(pair, T, return_noise=True))
  for k in out:
    same(out[k], torch.cat([o[k] for o in outs], 1), k)
  for k in STATE[kind] + ('agent_phase', 'steps_in_phase'):
    same(getattr(whole.unwrapped, k), torch.cat([getattr(p.unwrapped, k) for p in parts]), k)
  for c in range(2):
    same(whole.unwrapped.pair_counts[c], torch.cat([p.unwrapped.pair_counts[c] for p in parts]), 'counts')
  assert guard_share(out) <= MAX_GUARD_SHARE


# ---------------------------------------------------------------------------------------------------------------- 10. every output pointer NULL
def abi_launch(u, pair, goal, full, rubbish):
  """earl_sawyer_pair_rollout on the env's own structs, with every output given (`full`) or every optional pointer but the two counters NULL; the counters start as
  `rubbish`"""
  import torch
  from earl_benchmark_amd import _abi
  n, kw = u.num_envs, dict(device='cuda')
  fs, bs = torch.full((n,), rubbish, dtype=torch.int32, **kw), torch.full((n,), -rubbish, dtype=torch.int32, **kw)
  keep = u._new_out((T,), info=u.nv >= 15) if full else {}
  keep['actions'], keep['agent'] = torch.empty(T, n, 4, dtype=torch.float32, **kw), torch.empty(T, n, dtype=torch.int8, **kw)
  ptr = lambda k: keep[k].data_ptr() if full and k in keep else None
  o = _abi.SawyerOut(obs=ptr('obs'), reward=ptr('reward'), done=ptr('done'), success=ptr('success'), status=ptr('status'), info=ptr('info'))
  ps = _abi.AgentPair(switch_every=(C.c_int32 * 2)(*pair.switch_every), switch_on_success=int(pair.switch_on_success), pad_=0, param_stride=pair.stride,
                      backward_goal=goal.data_ptr(), phase=u.agent_phase.data_ptr(), steps_in_phase=u.steps_in_phase.data_ptr(), agent_out=ptr('agent'),
                      forward_success=fs.data_ptr(), backward_success=bs.data_ptr())
  u._cfg.step_counter = u.total_step_count
  if u._uses_queue(T):
    u.sched.zero_()
  _abi.check(u._lib.earl_sawyer_pair_rollout(u.model.buf.data_ptr(), u.model.col_ptr, u.nv, u._cfg_ref, u._st_ref, C.byref(pair.struct), C.byref(ps), None,
                                             u.last_obs.data_ptr(), T, None, ptr('actions'), C.byref(o), u._stream()), 'earl_sawyer_pair_rollout')
  torch.cuda.synchronize()
  return keep, fs, bs


@pytest.mark.parametrize('kind,n', [('door', 64), ('peg', 4160)])
def test_a_launch_without_any_output_leaves_the_same_state(kind, n):
  env = make_env(kind, n, seed=10)
  u = env.unwrapped
  goal = reset_row(u)
  pair, _ = make_pair(seed=5, sos=True)
  sd = u.state_dict()
  ends = []
  for full, rubbish in ((True, 12345), (False, -7)):
    u.load_state_dict(sd)
    stagger(u)
    keep, fs, bs = abi_launch(u, pair, goal, full, rubbish)
    ends.append((state_of(u), u.agent_phase.clone(), u.steps_in_phase.clone(), fs, bs))
    if full:
      assert float((keep['status'] != 0).float().mean()) <= MAX_GUARD_SHARE
      assert int(fs.min()) >= 0 and int(bs.min()) >= 0 and int(fs.max()) <= T and int(bs.max()) <= T and int((fs + bs).sum()) > 0      # (the rubbish is gone)
  same_state(ends[0][0], ends[1][0])
  for a, b, what in zip(ends[0][1:], ends[1][1:], ('phase', 'steps_in_phase', 'forward_success', 'backward_success')):
    same(a, b, what)


# ---------------------------------------------------------------------------------------------------------------- 11. the Python surface
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_python_surface(kind):
  import torch
  from earl_benchmark_amd.policy import AgentPair
  from earl_benchmark_amd.wrappers import LifelongWrapper, PersistentStateWrapper
  n = 64
  env = make_env(kind, n, seed=2)
  u = env.unwrapped
  pair, _ = make_pair(seed=1, sos=True, goal=reset_row(u))
  sd0 = u.state_dict()
  assert u.agent_phase is None and u.pair_counts is None and 'agent_phase' not in sd0 and 'steps_in_phase' not in sd0
  out = PersistentStateWrapper(env, episode_horizon=10**6).rollout_agents(pair, T) if kind == 'door' else env.rollout_agents(pair, T)
  assert tuple(out['agent'].shape) == (T, n) and out['agent'].dtype == torch.int8 and tuple(out['actions'].shape) == (T, n, 4)
  assert ('info' in out) == (kind == 'peg') and u.total_step_count == T and not u._last_obs_stale
  same(u._last_success, out['success'][-1], '_last_success')
  fs, bs = u.pair_counts
  assert tuple(fs.shape) == (n,) and fs.dtype == torch.int32 and int(fs.sum() + bs.sum()) > 0
  assert u.agent_phase.dtype == torch.int8 and u.steps_in_phase.dtype == torch.int32 and bool((u.agent_phase != 0).any())
  # state_dict carries the pair's state once it exists; a dict without the keys leaves the env's own
  sd = u.state_dict()
  same(sd['agent_phase'], u.agent_phase, 'agent_phase')
  ph, sip = u.agent_phase.clone(), u.steps_in_phase.clone()
  nxt = {k: v.clone() for k, v in env.rollout_agents(pair, 4).items()}
  u.load_state_dict(sd)
  same(u.agent_phase, ph, 'phase restored')
  same(u.steps_in_phase, sip, 'steps_in_phase restored')
  again = env.rollout_agents(pair, 4)
  for k in nxt:
    same(again[k], nxt[k], k)
  ph, sip = u.agent_phase.clone(), u.steps_in_phase.clone()
  u.load_state_dict(sd0)
  same(u.agent_phase, ph, 'a dict without the pair keys')
  # reset(mask) zeroes the masked envs' phase state only
  u.agent_phase.fill_(1)
  u.steps_in_phase.fill_(2)
  mask = (torch.arange(n, device='cuda') % 3 == 0)
  env.reset(mask)
  assert bool((u.agent_phase[mask] == 0).all()) and bool((u.steps_in_phase[mask] == 0).all())
  assert bool((u.agent_phase[~mask] == 1).all()) and bool((u.steps_in_phase[~mask] == 2).all())
  env.reset()
  assert not bool(u.agent_phase.any()) and not bool(u.steps_in_phase.any())
  # 'initial': the door's one row; the peg has fifteen and wants the row itself
  pf, pb = pair.agent(0), pair.agent(1)
  init = AgentPair(pf, pb, switch_every=SE, obs_dim=14, act_dim=4)
  if kind == 'door':
    got = env.rollout_agents(init, T)
    entered = (got['agent'][1:] == 1) & (got['agent'][:-1] == 0)
    assert bool(entered.any())
    t, i = (int(v) for v in entered.nonzero()[0])
    same(got['obs'][t, i, 7:].contiguous(), torch.as_tensor(u.initial_states[0], device='cuda'), "the reset agent sees env.initial_states[0]")
  else:
    with pytest.raises(ValueError, match=r'env\.initial_states'):
      env.rollout_agents(init, T)
    env.rollout_agents(AgentPair(pf, pb, switch_every=SE, backward_goal=u.initial_states[3], obs_dim=14, act_dim=4), 2)
  # refusals
  with pytest.raises(ValueError, match='agent pair IS the lifelong mechanism'):
    LifelongWrapper(make_env(kind, 4), 5).rollout_agents(pair, 2)
  with pytest.raises(ValueError, match='AgentPair goes to rollout_agents'):
    env.rollout_policy(pair, 2)
  with pytest.raises(ValueError, match='need Gaussian agents'):
    env.rollout_agents(pair, 2, return_noise=True)

"""earl_tabletop_pair_rollout (include/earl_tabletop.h): the forward / reset agent pair of autonomous RL alternating inside one closed-loop rollout.
Without a GPU, through csrc/libearl_host.so (the host twin) -- and csrc/libearl_hip.so for the argument errors, which come before any HIP call:
  1. never switching is the existing single-policy entry point on the forward row, bit for bit: outputs, actions, eps, final state;
  2. clock-only switching equals alternating launches of the existing entry point in chunks of switch_every[k] with the goal installed in between;
  3. success switching equals a per-step composition of T = 1 single-policy launches, step and the handover rule in numpy;
  4. agent_out, phase, steps_in_phase and both counters equal the handover rule applied to the launch's own success / done;
  5. two launches of T1 and T2 equal one of T1 + T2;   6. two ragged shards equal the batch;
  7. in the configurations of 3 and 4 together, each of the four handover causes makes up at least 1 % of all handovers;
  8. every argument error from both libraries, the struct layout against gcc;
  9. AgentPair, env.rollout_agents on device='cpu' through the loader and the wrappers, the refusals, reset(mask), the state dict;
 10. the pair kernels have no scratch and the figures on record (cross-compiled).
tests/test_policy_pair_gpu.py holds the device to the host twin bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import hip_harness as hx
import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import GaussPolicy, head_struct
from pair_helpers import (INITIAL, OUT, Pair, PairState, assert_bits, goal_draw, handover_rule, pair_rollout, pair_struct, single_rollout, still_pair, with_goal_row)
from test_policy_rollout import Policy, final_state, restore, snapshot

CPU = 'cpu'
OFFSET = 3
HEADS = {'deterministic': None, 'sample_tanh': dict(mode='sample', log_std_map='tanh'), 'sample_clamp': dict(mode='sample', log_std_map='clamp'),
         'mean': dict(mode='mean', log_std_map='tanh')}
FORMS = {'evaluation': (2, True, dict(horizon=60)), 'continuing': (1, False, dict(horizon=10**6)), 'auto_reset': (1, False, dict(auto_reset=True, horizon=13))}


def prepared(n, reset_first, device=CPU, **kw):
  """a harness in the state a launch starts from: a continuing rollout starts somewhere (a reset and a few scripted steps)"""
  h = hx.HipTabletop(n, device=device, **kw)
  h.reset()
  if not reset_first:
    h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, n, 3)).astype(np.float32))
  return h


def keys_of(head):
  return OUT + ('act',) + (('eps',) if head is not None else ())


def assert_state(end, want_state, what=''):
  for k, v in want_state.items():
    np.testing.assert_array_equal(end[k].view(np.uint8), np.ascontiguousarray(v).view(np.uint8), err_msg=f'{what} state {k}')


# ---------------------------------------------------------------------------------------------------------------- 1. never switching
@pytest.mark.parametrize('head', list(HEADS))
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('hidden', [(16,), (256,), (48, 32), (64, 128)], ids=str)
def test_never_switching_is_the_existing_entry_point_on_the_forward_row(hidden, form, head):
  E, reset_first, cfg_kw = FORMS[form]
  T = 60
  for n in (1, 100):
    kw = dict(reward_type='sparse', wide_init=n == 100, seed=11, env_offset=OFFSET, **cfg_kw)
    pr = Pair(hidden, gaussian=HEADS[head] is not None, hidden_act='tanh' if len(hidden) == 2 else 'relu', seed0=len(hidden) * 10)
    h = prepared(n, reset_first, **kw)
    snap = snapshot(h)
    ps = PairState(n)
    got = pair_rollout(h, pr, ps, E, T, reset_first, T + 1, 0, head=HEADS[head])
    end = final_state(h)
    assert not any(np.isnan(got[k]).any() for k in keys_of(HEADS[head]) if got[k].dtype == np.float32), 'an output was not written, or a read left the agent\'s parameters'
    restore(h, snap)
    want = single_rollout(h, pr.members[0], E, T, reset_first, head=HEADS[head])
    assert_bits(got, want, keys_of(HEADS[head]))
    again = final_state(h)
    assert_state(end[0], again[0], f'n={n}')
    assert end[1] == again[1] == snap[1] + (E * (T + 1) if reset_first else T)
    assert (got['agent'] == 0).all() and (got['fs'] == 0).all() and (got['bs'] == 0).all() and (ps.host()[0] == 0).all()
    if form == 'auto_reset':
      assert got['done'].any() and (ps.host()[1] == (9 + T) % 13).all()
    elif form == 'continuing':
      assert (ps.host()[1] == T).all()


# ---------------------------------------------------------------------------------------------------------------- 2. clock-only switching
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('goal', [None, 'initial'])
@pytest.mark.parametrize('switch_every', [(25, 25), (7, 5), (1, 3)], ids=str)
def test_clock_only_switching_equals_alternating_launches_of_the_existing_entry_point(switch_every, goal, head):
  """what a user does today: chunks of switch_every[k] steps of the single-policy entry point (reset_first = 0) with agent k's parameters; between chunks the goal is
  installed the way reset_goal does it -- the reset agent's row appended to the goal table and goal_idx pointed at it, resp. goal_idx set to the sampled index (the
  draw of the chunk's last step).  The chunk's last observation row is re-read with the installed goal, which is what the next chunk's first action sees."""
  n, T = 100, 83
  kw = dict(reward_type='sparse', wide_init=True, seed=5, env_offset=OFFSET, horizon=10**6)
  pr = Pair((64,), gaussian=HEADS[head] is not None, seed0=2)
  h = prepared(n, False, **kw)
  row = with_goal_row(h, INITIAL)
  snap = snapshot(h)
  ps = PairState(n)
  got = pair_rollout(h, pr, ps, 1, T, False, switch_every, 0, backward_goal=None if goal is None else INITIAL, head=HEADS[head])
  end = final_state(h)
  restore(h, snap)
  task = h.host('goal_idx').copy()
  table = h.goal_table.cpu().numpy()
  parts, agents, phase, t, sip = [], [], 0, 0, 0
  while t < T:
    m = min(switch_every[phase], T - t)
    part = single_rollout(h, pr.members[phase], 1, m, False, head=HEADS[head])
    agents.append(np.full((m, n), phase, np.int8))
    t += m
    sip = m
    if m == switch_every[phase]:                              # the handover after the chunk's last step, whose Philox counter is the launch's last
      phase, sip = phase ^ 1, 0
      if phase == 0:
        task = goal_draw(h, int(h.cfg.counter) - 1)
        h.goal_idx.copy_(torch.from_numpy(task))
      elif goal is not None:
        h.goal_idx.fill_(row)
      part['obs'][-1, :, 6:] = table[h.host('goal_idx')].astype(np.float32)
    parts.append(part)
  want = {k: np.concatenate([p[k] for p in parts], axis=0) for k in keys_of(HEADS[head])}
  assert_bits(got, want, keys_of(HEADS[head]))
  np.testing.assert_array_equal(got['agent'], np.concatenate(agents, axis=0))
  want_state = final_state(h)[0]
  want_state['goal_idx'] = task                               # the pair leaves the env's TASK goal in goal_idx, also while the reset agent's row is in force
  assert_state(end[0], want_state)
  assert end[1] == snap[1] + T
  assert (ps.host()[0] == phase).all() and (ps.host()[1] == sip).all() and (got['fs'] == 0).all() and (got['bs'] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. success switching = per-step composition
COMPOSE = {  # name: (pair factory, cfg, backward goal, switch_every)
    'random_nets_at_goal': (lambda g: Pair((64,), gaussian=g, seed0=4), dict(reset_at_goal=True, wide_init=True), None, (7, 5)),
    'random_nets_at_goal_initial': (lambda g: Pair((48, 32), gaussian=g, hidden_act='tanh', seed0=4), dict(reset_at_goal=True, wide_init=True), 'initial', (7, 5)),
    'still_at_goal': (lambda g: still_pair(gaussian=g), dict(reset_at_goal=True), None, (7, 5)),
    'still_default_initial': (lambda g: still_pair(gaussian=g), dict(), 'initial', (6, 4)),
}


def composition(name, head_name, n=80, T=40):
  """-> the four handover-cause counts.  Per step, from entry points that existed before the pair: a T = 1 single-policy launch per agent on a restored copy of the
  state (goal_idx pointing at the goal in force) for that agent's action, select by phase, step(), then the handover rule restated in numpy.  (Without auto-reset:
  after one, the closed-loop kernels compute the next action from the terminal observation, which a fresh T = 1 launch does not see.)"""
  make, cfg_kw, goal, se = COMPOSE[name]
  head = HEADS[head_name]
  kw = dict(dict(reward_type='sparse', seed=9, env_offset=OFFSET, horizon=10**6), **cfg_kw)
  pr = make(head is not None)
  h = prepared(n, False, **kw)
  row = with_goal_row(h, INITIAL)
  rng = np.random.default_rng(0)
  phase, sip = rng.integers(0, 2, n).astype(np.int8), rng.integers(0, 3, n).astype(np.int32)
  snap = snapshot(h)
  ps = PairState(n, phase=phase, sip=sip)
  got = pair_rollout(h, pr, ps, 1, T, False, se, 1, backward_goal=None if goal is None else INITIAL, head=head)
  end = final_state(h)
  restore(h, snap)
  table = h.goal_table.cpu().numpy()
  task = h.host('goal_idx').copy()
  want = {k: [] for k in keys_of(head) + ('agent',)}
  fs, bs, causes = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(4, np.int64)

  def in_force():
    return np.where((phase == 1) & (goal is not None), row, task).astype(np.int32)

  for t in range(T):
    h.goal_idx.copy_(torch.from_numpy(in_force()))
    s = snapshot(h)
    acts = []
    for k in (0, 1):
      restore(h, s)
      acts.append(single_rollout(h, pr.members[k], 1, 1, False, head=head))
    restore(h, s)
    act = np.where((phase == 1)[:, None], acts[1]['act'][0], acts[0]['act'][0])
    counter = int(h.cfg.counter)
    obs, rew, done, succ = h.step(act)
    want['agent'].append(phase.copy())
    want['act'].append(act)
    if head is not None:
      np.testing.assert_array_equal(acts[0]['eps'], acts[1]['eps'])        # the draw does not depend on the agent
      want['eps'].append(acts[0]['eps'][0])
    sip = (sip + 1).astype(np.int32)
    s_ = succ.astype(bool)
    over = s_ | (sip >= np.asarray(se)[phase])
    fs += over & s_ & (phase == 0)
    bs += over & s_ & (phase == 1)
    for k, m in enumerate((over & s_ & (phase == 0), over & ~s_ & (phase == 0), over & s_ & (phase == 1), over & ~s_ & (phase == 1))):
      causes[k] += int(m.sum())
    to_forward = over & (phase == 1)
    phase = np.where(over, phase ^ 1, phase).astype(np.int8)
    sip = np.where(over, 0, sip).astype(np.int32)
    if to_forward.any():
      task = np.where(to_forward, goal_draw(h, counter), task).astype(np.int32)
    obs[over, 6:] = table[in_force()[over]].astype(np.float32)
    for k, v in zip(OUT, (obs, rew, done, succ)):
      want[k].append(v)
  want = {k: np.stack(v) for k, v in want.items()}
  assert_bits(got, want, keys_of(head) + ('agent',))
  want_state = final_state(h)[0]
  want_state['goal_idx'] = task
  assert_state(end[0], want_state, name)
  assert end[1] == snap[1] + T
  np.testing.assert_array_equal(ps.host()[0], phase)
  np.testing.assert_array_equal(ps.host()[1], sip)
  np.testing.assert_array_equal(got['fs'][0], fs)
  np.testing.assert_array_equal(got['bs'][0], bs)
  return causes


@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('name', list(COMPOSE))
def test_success_switching_equals_a_per_step_composition_of_existing_entry_points(name, head):
  causes = composition(name, head)
  print(name, head, 'handovers (forward by success, forward by clock, reset by success, reset by clock):', causes)
  assert causes.sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 4. the rule recomputed
RULE = {  # name: (pair factory, cfg, backward goal, switch_every, form)
    'still_at_goal': (lambda g: still_pair(gaussian=g), dict(reset_at_goal=True), None, (7, 5), 'continuing'),
    'still_at_goal_initial': (lambda g: still_pair(gaussian=g), dict(reset_at_goal=True), 'initial', (7, 5), 'continuing'),
    'still_default_initial': (lambda g: still_pair(gaussian=g), dict(), 'initial', (6, 4), 'evaluation'),
    'random_nets_evaluation': (lambda g: Pair((64,), gaussian=g, seed0=4), dict(reset_at_goal=True, wide_init=True), 'initial', (7, 5), 'evaluation'),
    'random_nets_auto_reset': (lambda g: Pair((64,), gaussian=g, seed0=4), dict(reset_at_goal=True, wide_init=True), None, (7, 5), 'auto_reset'),
}


def rule_recomputed(name, head_name, n=333, T=60):
  make, cfg_kw, goal, se, form = RULE[name]
  E, reset_first, form_kw = FORMS[form]
  kw = dict(dict(reward_type='sparse', seed=9, env_offset=OFFSET), **form_kw, **cfg_kw)
  h = prepared(n, reset_first, **kw)
  rng = np.random.default_rng(0)
  phase, sip = rng.integers(0, 2, n).astype(np.int8), rng.integers(0, 3, n).astype(np.int32)
  ps = PairState(n, phase=phase, sip=sip)
  got = pair_rollout(h, make(HEADS[head_name] is not None), ps, E, T, reset_first, se, 1, backward_goal=None if goal is None else INITIAL, head=HEADS[head_name])
  lead = (E, T, n)
  agent, ph, sp, fs, bs, causes = handover_rule(got['success'].reshape(lead), got['done'].reshape(lead), phase, sip, se, 1, bool(kw.get('auto_reset')), reset_first)
  np.testing.assert_array_equal(got['agent'].reshape(lead), agent)
  np.testing.assert_array_equal(ps.host()[0], ph)
  np.testing.assert_array_equal(ps.host()[1], sp)
  np.testing.assert_array_equal(got['fs'], fs)
  np.testing.assert_array_equal(got['bs'], bs)
  return causes


@pytest.mark.parametrize('head', ['deterministic', 'sample_clamp'])
@pytest.mark.parametrize('name', list(RULE))
def test_agent_phase_clock_and_counters_equal_the_rule_on_the_launch_s_own_flags(name, head):
  causes = rule_recomputed(name, head)
  print(name, head, 'handovers (forward by success, forward by clock, reset by success, reset by clock):', causes)
  assert causes.sum() > 0


@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_an_auto_reset_in_the_reset_phase_puts_the_task_goal_back_in_force(head):
  """contract item 5 with a goal overlay: an env that the auto-reset hits while the reset agent's row is in force is the forward agent's again, and the goal it sees
  from the next step on is its stored task goal, goal_table[goal_idx], not the overlay.  Checked on the returned observations' goal slots and the final goal_idx,
  without the host twin's own step: clock-only switching with switch_every = (7, 8) under horizon 13 -- after the first auto-reset every env spends steps 8..13 of
  each episode in the reset phase, so every later auto-reset hits the overlay."""
  n, T, se = 100, 60, (7, 8)
  kw = dict(reward_type='sparse', wide_init=True, seed=9, env_offset=OFFSET, auto_reset=True, horizon=13)
  h = prepared(n, False, **kw)
  table = h.goal_table.cpu().numpy()
  assert not (table == INITIAL).all(axis=1).any()              # the overlay is told apart from every task row
  rng = np.random.default_rng(0)
  ps = PairState(n, phase=rng.integers(0, 2, n).astype(np.int8), sip=rng.integers(0, 3, n).astype(np.int32))
  got = pair_rollout(h, Pair((64,), gaussian=HEADS[head] is not None, seed0=4), ps, 1, T, False, se, 0, backward_goal=INITIAL, head=HEADS[head])
  done, agent, goal_seen = got['done'].astype(bool), got['agent'], got['obs'][:, :, 6:]
  hit = done[:-1] & (agent[:-1] == 1)                          # [T - 1, n]: auto-reset at step t while the overlay was in force
  print(head, 'auto-resets that hit an env in the reset phase:', int(hit.sum()), 'of', int(done.sum()), 'auto-resets')
  assert hit.sum() >= 2 * n
  assert (agent[1:][hit] == 0).all()
  task32 = table.astype(np.float32)
  seen = goal_seen[1:][hit]                                    # the step after: se[0] > 1, so no handover has replaced the goal yet
  assert not (seen == INITIAL.astype(np.float32)).all(axis=1).any(), 'the overlay outlived the auto-reset'
  assert (seen[:, None, :] == task32[None]).all(axis=2).any(axis=1).all(), 'not a task goal'
  assert (ps.host()[0] == 0).all() and (ps.host()[1] < se[0]).all() and done[-se[0]:].any(axis=0).all()      # the launch ends in the forward phase that followed a reset
  np.testing.assert_array_equal(goal_seen[-1], task32[h.host('goal_idx')])


# ---------------------------------------------------------------------------------------------------------------- 7. coverage of 3 and 4
def test_each_of_the_four_handover_causes_is_at_least_one_percent_of_the_handovers_of_3_and_4():
  total = np.zeros(4, np.int64)
  for name in COMPOSE:
    total += composition(name, 'deterministic')
  for name in RULE:
    total += rule_recomputed(name, 'deterministic')
  share = total / total.sum()
  print('handovers of the configurations of 3 and 4: forward by success %d (%.3f), forward by clock %d (%.3f), reset by success %d (%.3f), reset by clock %d (%.3f)'
        % tuple(v for pair in zip(total, share) for v in pair))
  assert (share >= 0.01).all(), share


# ---------------------------------------------------------------------------------------------------------------- 5. split launches, 6. shards
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_two_launches_equal_one_and_two_ragged_shards_equal_the_batch(head):
  n, T1, T2 = 100, 23, 31
  kw = dict(reward_type='sparse', reset_at_goal=True, wide_init=True, seed=21, horizon=10**6)
  pr = Pair((64,), gaussian=HEADS[head] is not None, seed0=5)
  args = dict(switch_every=(7, 5), switch_on_success=1, backward_goal=INITIAL, head=HEADS[head])
  whole = prepared(n, False, env_offset=OFFSET, **kw)
  snap = snapshot(whole)
  ps = PairState(n)
  got = pair_rollout(whole, pr, ps, 1, T1 + T2, False, **args)
  end = final_state(whole)
  assert 0 < got['agent'].mean() < 1
  # two launches: the state carries everything
  restore(whole, snap)
  ps2 = PairState(n)
  a = pair_rollout(whole, pr, ps2, 1, T1, False, **args)
  b = pair_rollout(whole, pr, ps2, 1, T2, False, **args)
  keys = keys_of(HEADS[head]) + ('agent',)
  assert_bits({k: np.concatenate([a[k], b[k]], axis=0) for k in keys}, got, keys)
  np.testing.assert_array_equal(a['fs'] + b['fs'], got['fs'])
  np.testing.assert_array_equal(a['bs'] + b['bs'], got['bs'])
  assert_state(final_state(whole)[0], end[0])
  assert final_state(whole)[1] == end[1]
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])
  np.testing.assert_array_equal(ps2.host()[1], ps.host()[1])
  # two ragged shards
  parts, states, pss = [], [], []
  for i0, m in ((0, 60), (60, 40)):
    hs = hx.HipTabletop(m, device=CPU, env_offset=OFFSET + i0, **kw)
    for k, v in snap[0].items():
      getattr(hs, k).copy_(v[i0:i0 + m])
    hs.cfg.counter = snap[1]
    p = PairState(m)
    parts.append(pair_rollout(hs, pr, p, 1, T1 + T2, False, **args))
    states.append(final_state(hs))
    pss.append(p.host())
  assert_bits({k: np.concatenate([p[k] for p in parts], axis=1) for k in keys + ('fs', 'bs')}, got, keys + ('fs', 'bs'))
  assert_state({k: np.concatenate([s[0][k] for s in states], axis=0) for k in end[0]}, end[0])
  assert states[0][1] == states[1][1] == end[1]
  np.testing.assert_array_equal(np.concatenate([p[0] for p in pss]), ps.host()[0])
  np.testing.assert_array_equal(np.concatenate([p[1] for p in pss]), ps.host()[1])


def test_null_outputs_leave_the_rest_what_it_was():
  n, T = 50, 30
  kw = dict(reward_type='dense', reset_at_goal=True, wide_init=True, seed=2, env_offset=OFFSET, horizon=10**6)
  pr = Pair((32,), gaussian=True, seed0=1)
  args = dict(switch_every=(7, 5), switch_on_success=1, backward_goal=INITIAL, head=HEADS['sample_clamp'])
  h = prepared(n, False, **kw)
  snap = snapshot(h)
  ps = PairState(n)
  got = pair_rollout(h, pr, ps, 1, T, False, **args)
  end = final_state(h)
  restore(h, snap)
  ps2 = PairState(n)
  bare = pair_rollout(h, pr, ps2, 1, T, False, null=OUT + ('act', 'eps', 'agent', 'fs', 'bs'), **args)
  for k in OUT + ('act', 'eps'):
    assert np.isnan(bare[k]).all() if bare[k].dtype == np.float32 else (bare[k] == 7).all()
  assert (bare['agent'] == 7).all() and (bare['fs'] == -7).all() and (bare['bs'] == -7).all()
  assert_state(final_state(h)[0], end[0])
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])
  np.testing.assert_array_equal(ps2.host()[1], ps.host()[1])


# ---------------------------------------------------------------------------------------------------------------- 8. argument errors
def _edge_calls(lib, host):
  n = 40
  h = hx.HipTabletop(n, device=CPU, env_offset=OFFSET)
  st = h._state()
  arrs, out = h._outs((1, 4, n))
  det, gau, wide = Pair((16,)), Pair((16,), gaussian=True), Pair((16, 144))
  ps = PairState(n)
  good_head = head_struct()

  def pairv(p=det, **kw):
    s = pair_struct(p, ps, (5, 5), 1)
    for k, v in kw.items():
      setattr(s, k, v)
    return s

  def call(cfg=h.cfg, state=st, p=det.struct, pair=pairv(), hd=None, E=1, T=4, rf=1, o=out):
    ref = lambda x: C.byref(x) if x is not None else None
    args = [ref(cfg), ref(state), ref(p), ref(pair), ref(hd), E, T, rf, ref(o), None]
    return lib.earl_tabletop_pair_rollout_cpu(*args) if host else lib.earl_tabletop_pair_rollout(*args, None)

  def cfgv(**kw):
    c = _abi.TabletopCfg.from_buffer_copy(h.cfg)
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def variant(base, **kw):
    d = dict(n_layers=base.n_layers, dims=tuple(base.dims), hidden_act=base.hidden_act, out_act=base.out_act, precision=0, params=base.params)
    d.update(kw)
    d['dims'] = (C.c_int32 * 4)(*d['dims'])
    return _abi.MlpPolicy(**d)

  bad = [dict(pair=None), dict(pair=pairv(phase=None)), dict(pair=pairv(steps_in_phase=None)),                                                  # NULL pair / phase / steps_in_phase
         dict(pair=pairv(switch_every=(C.c_int32 * 2)(0, 5))), dict(pair=pairv(switch_every=(C.c_int32 * 2)(5, 0))), dict(pair=pairv(switch_every=(C.c_int32 * 2)(5, -3))),
         dict(pair=pairv(switch_on_success=2)), dict(pair=pairv(switch_on_success=-1)),
         dict(pair=pairv(param_stride=det.n_params - 1)), dict(pair=pairv(param_stride=0)), dict(pair=pairv(param_stride=-1)),
         dict(cfg=cfgv(goal_change_frequency=10)),                                                                                              # the pair is the lifelong mechanism
         dict(p=wide.struct, pair=pairv(wide)),                                                                                                 # H2 = 144 > EARL_PAIR_MAX_H2
         dict(hd=good_head), dict(p=gau.struct, pair=pairv(gau)),                                                                               # head and dims[n_layers] disagree
         dict(p=gau.struct, pair=pairv(gau), hd=head_struct(mode=2)), dict(p=gau.struct, pair=pairv(gau), hd=head_struct(bounds=(1.0, -1.0))),
         # what the single-policy entry points refuse
         dict(cfg=None), dict(state=None), dict(p=None), dict(o=None), dict(p=variant(det.struct, params=None)), dict(p=variant(det.struct, precision=1)),
         dict(p=variant(det.struct, dims=(12, 24, 3, 0))), dict(p=variant(det.struct, hidden_act=0)), dict(T=0), dict(E=0), dict(E=2, rf=0), dict(rf=2)]
  for kw in bad:
    assert call(**kw) == -1, kw
    assert (lib.earl_host_last_error if host else lib.earl_last_error)(), kw
  assert call(p=wide.struct, pair=pairv(wide)) == -1
  assert b'EARL_PAIR_MAX_H2 = 128' in (lib.earl_host_last_error if host else lib.earl_last_error)()
  call.keep = (h, arrs, det, gau, wide, ps)
  return call, gau, good_head, pairv


def test_argument_errors_from_the_host_library():
  lib = _abi.load_host()
  call, gau, good_head, pairv = _edge_calls(lib._cdll, True)
  assert call() == 0                                                       # the good call runs (host pointers)
  assert call(p=gau.struct, pair=pairv(gau), hd=good_head) == 0
  assert call(pair=pairv(backward_goal=None)) == 0 and call(rf=0) == 0
  w128 = Pair((16, 128))
  assert call(p=w128.struct, pair=pairv(w128)) == 0                      # the widest second hidden layer that ships


def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  _edge_calls(lib, False)
  assert lib.earl_tabletop_pair_rollout(None, None, None, None, None, 1, 1, 1, None, None, None) == -1
  assert b'NULL' in lib.earl_last_error()


def test_struct_layout_matches_what_gcc_sees(tmp_path):
  src = '#include <stdio.h>\n#include <stddef.h>\n#include "earl_tabletop.h"\nint main(void) {\n'
  cname, cls = 'earl_agent_pair', _abi.AgentPair
  src += f'printf("%zu ", sizeof({cname}));\n' + ''.join(f'printf("%zu ", offsetof({cname}, {f[0]}));\n' for f in cls._fields_)
  src += 'printf("%d ", EARL_PAIR_MAX_H2);\n'
  want = [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_] + [_abi.PAIR_MAX_H2]
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src + 'return 0; }\n')
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  assert [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == want
  assert C.sizeof(_abi.AgentPair) == 72


# ---------------------------------------------------------------------------------------------------------------- 9. the Python surface on the host
def test_agent_pair_packs_indexes_and_rejects():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy
  refs = [Policy((64,), seed=s) for s in range(2)]
  pis = [MLPPolicy(r.layers, 'relu', 'tanh') for r in refs]
  pair = AgentPair(pis[0], pis[1], switch_every=(30, 20))
  assert eb.AgentPair is AgentPair and pair.stride == pair.n_params == refs[0].params.numel() and not pair.gaussian
  assert pair.switch_every == (30, 20) and pair.switch_on_success is True and pair.backward_goal == 'initial'
  assert AgentPair(pis[0], pis[1]).switch_every == (200, 200) and AgentPair(pis[0], pis[1], switch_every=7).switch_every == (7, 7)
  np.testing.assert_array_equal(pair.params.numpy(), np.stack([r.params.numpy() for r in refs]))
  assert pair.params.dtype == torch.float32 and pair.params.is_contiguous() and pair.struct.params == pair.params.data_ptr()
  for k in (0, 1):
    np.testing.assert_array_equal(pair.agent(k).params.numpy(), refs[k].params.numpy())
    assert isinstance(pair.agent(k), MLPPolicy) and pair.agent(k).dims == [12, 64, 3]
  ptr = pair.params.data_ptr()
  pair.params.mul_(2.0)                                                     # in-place writes reach the kernel's view
  assert pair.params.data_ptr() == ptr == pair.struct.params
  np.testing.assert_array_equal(pair.agent(1).params.numpy(), 2.0 * refs[1].params.numpy())
  pair.params.mul_(0.5)
  assert pair.to('cpu') is pair
  # the torch statement: each env through the agent of its phase
  x, ph = torch.randn(3, 10, 12), torch.tensor([0, 1] * 5)
  y = pair(x, ph)
  for k in (0, 1):
    torch.testing.assert_close(y[:, k::2], pis[k](x[:, k::2].reshape(-1, 12)).reshape(3, 5, 3))
  torch.testing.assert_close(pair(x, ph.expand(3, 10)), y)
  # rejections name the member, as PolicyPopulation's
  with pytest.raises(ValueError, match='member 1'):
    AgentPair(pis[0], MLPPolicy(Policy((32,), seed=0).layers))
  with pytest.raises(ValueError, match='member 1'):
    AgentPair(pis[0], MLPPolicy(refs[1].layers, 'tanh', 'tanh'))
  with pytest.raises(ValueError, match='member 1'):
    AgentPair(pis[0], MLPPolicy(refs[1].layers, 'relu', 'none'))
  g = [GaussPolicy((64,), seed=s) for s in range(2)]
  gp = [GaussianMLPPolicy(r.layers, 'relu') for r in g]
  assert AgentPair(gp[0], gp[1]).gaussian and AgentPair(gp[0], gp[1]).dims == [12, 64, 6]
  assert isinstance(AgentPair(gp[0], gp[1]).agent(1), GaussianMLPPolicy)
  with pytest.raises(ValueError, match='member 1'):
    AgentPair(pis[0], gp[1])
  for kw in (dict(squash=False), dict(log_std_bounds=(-4.0, 2.0)), dict(log_std_map='clamp')):
    with pytest.raises(ValueError, match='member 1'):
      AgentPair(gp[0], GaussianMLPPolicy(g[1].layers, 'relu', **kw))
  for se in (0, (5, 0), (1, 2, 3), -4):
    with pytest.raises(ValueError):
      AgentPair(pis[0], pis[1], switch_every=se)
  with pytest.raises(ValueError):
    AgentPair(pis[0], pis[1], backward_goal=[0.0] * 5)
  with pytest.raises(ValueError):
    AgentPair(pis[0], object())
  wide = [MLPPolicy(Policy((16, 144), seed=s).layers) for s in range(2)]
  with pytest.raises(ValueError, match='128'):
    AgentPair(wide[0], wide[1])
  assert AgentPair(*[MLPPolicy(Policy((16, 128), seed=s).layers) for s in range(2)]).dims == [12, 16, 128, 3]


@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian'])
def test_rollout_agents_on_the_host_through_the_loader_and_the_wrappers(gaussian):
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy
  if gaussian:
    refs = [GaussPolicy((64,), seed=s, log_std_gain=1.0) for s in range(2)]
    agents = [GaussianMLPPolicy(r.layers, 'relu') for r in refs]
  else:
    refs = [Policy((64,), seed=s) for s in range(2)]
    agents = [MLPPolicy(r.layers, 'relu', 'tanh') for r in refs]
  n, T = 100, 40
  kw = dict(reward_type='sparse', reset_train_env_at_goal=True, wide_init_distr=True, num_envs=n, device='cpu', seed=3, env_offset=OFFSET)
  env, _ = eb.EARLEnvs('tabletop_manipulation', **kw).get_envs()
  u = env.unwrapped
  # before any pair launch: no pair state, the state dict as it always was
  assert u.agent_phase is None and u.steps_in_phase is None and u.pair_counts is None
  sd = u.state_dict()
  assert 'agent_phase' not in sd and 'steps_in_phase' not in sd
  pair = AgentPair(agents[0], agents[1], switch_every=(7, 5))
  outs = env.rollout_agents(pair, T, **(dict(return_noise=True) if gaussian else {}))
  obs, rew, done, succ, act, agent = outs[:6]
  assert len(outs) == (7 if gaussian else 6)
  assert tuple(obs.shape) == (T, n, 12) and tuple(act.shape) == (T, n, 3) and tuple(agent.shape) == (T, n) and agent.dtype == torch.int8
  assert rew.dtype == torch.float32 and done.dtype == torch.bool and succ.dtype == torch.bool
  assert env.total_steps == T and u.state_dict()['rng_counter'] == sd['rng_counter'] + T
  assert u.agent_phase.dtype == torch.int8 and u.steps_in_phase.dtype == torch.int32 and 0 < float(agent.float().mean()) < 1
  fwd, bwd = u.pair_counts
  assert tuple(fwd.shape) == (1, n) and fwd.dtype == torch.int32 and int(fwd.sum()) > 0
  # the same launch through the C ABI of the host twin
  h = hx.HipTabletop(n, device=CPU, reward_type='sparse', reset_at_goal=True, wide_init=True, seed=3, env_offset=OFFSET, horizon=int(u._cfg.horizon),
                     goal_table=u.goal_table.numpy())
  for k, key in (('qpos', 'qpos'), ('attached', 'attached'), ('goal_idx', 'goal_idx'), ('steps_since_reset', 'steps_since_reset'), ('num_interventions', 'interventions')):
    getattr(h, k).copy_(sd[key])
  h.cfg.counter = sd['rng_counter']
  ps = PairState(n)
  got = pair_rollout(h, Pair(members=refs, gaussian=gaussian), ps, 1, T, False, (7, 5), 1, backward_goal=INITIAL, head=HEADS['sample_tanh'] if gaussian else None)
  for k, v in zip(OUT + ('act', 'agent'), (obs, rew, done.to(torch.uint8), succ.to(torch.uint8), act, agent)):
    np.testing.assert_array_equal(v.numpy().view(np.uint8), got[k].view(np.uint8), err_msg=k)
  if gaussian:
    np.testing.assert_array_equal(outs[6].numpy(), got['eps'])
  np.testing.assert_array_equal(u.agent_phase.numpy(), ps.host()[0])
  np.testing.assert_array_equal(u.steps_in_phase.numpy(), ps.host()[1])
  np.testing.assert_array_equal(fwd.numpy(), got['fs'])
  np.testing.assert_array_equal(bwd.numpy(), got['bs'])
  # the torch statement is close to the kernel's actions (deterministic agents; the first step's observation is not returned)
  if not gaussian:
    torch.testing.assert_close(pair(obs[:-1], agent[1:]), act[1:], rtol=1e-4, atol=1e-4)
  # the state dict carries the pair state now; a round trip continues the stream exactly
  sd1 = u.state_dict()
  assert torch.equal(sd1['agent_phase'], u.agent_phase) and torch.equal(sd1['steps_in_phase'], u.steps_in_phase)
  a = env.rollout_agents(pair, 20)
  env2, _ = eb.EARLEnvs('tabletop_manipulation', **kw).get_envs()
  env2.unwrapped.load_state_dict(sd1)
  b = env2.rollout_agents(pair, 20)
  assert all(torch.equal(x, y) for x, y in zip(a, b))
  # reset(mask) zeroes the pair state of the masked envs only
  u.agent_phase.fill_(1)
  u.steps_in_phase.fill_(3)
  mask = torch.zeros(n, dtype=torch.bool)
  mask[::3] = True
  env.reset(mask=mask)
  assert (u.agent_phase[mask] == 0).all() and (u.steps_in_phase[mask] == 0).all() and (u.agent_phase[~mask] == 1).all() and (u.steps_in_phase[~mask] == 3).all()
  env.reset()
  assert (u.agent_phase == 0).all() and (u.steps_in_phase == 0).all()
  # the evaluation form, and the argument checks of the method
  o2 = env.rollout_agents(pair, 10, episodes=2, reset_first=True, sample=True)
  assert tuple(o2[0].shape) == (2, 10, n, 12) and tuple(o2[5].shape) == (2, 10, n) and tuple(u.pair_counts[0].shape) == (2, n) and (o2[5][:, 0] == 0).all()
  with pytest.raises(ValueError):
    env.rollout_agents(pair, 10, episodes=2)
  with pytest.raises(ValueError):
    env.rollout_agents(agents[0], 10)
  if not gaussian:
    with pytest.raises(ValueError):
      env.rollout_agents(pair, 10, sample=False)
    with pytest.raises(ValueError):
      env.rollout_agents(pair, 10, return_noise=True)
  # the other entry points keep working on the state a pair launch leaves behind: goal_idx is a task goal
  assert int(u.goal_idx.max()) < 4 and int(u.goal_idx.min()) >= 0
  env.rollout_policy(agents[0], 5, reset_first=False)


def test_lifelong_wrapper_refuses_and_the_three_object_env_has_no_pair_entry():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation as TabletopManipulation3Obj
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  from earl_benchmark_amd.wrappers import LifelongWrapper
  pis = [MLPPolicy(Policy((16,), seed=s).layers) for s in range(2)]
  pair = AgentPair(pis[0], pis[1], switch_every=5)
  train = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', setup_as_lifelong_learning=True, num_envs=8, device='cpu').get_envs()
  assert isinstance(train, LifelongWrapper)
  with pytest.raises(ValueError, match='lifelong'):
    train.rollout_agents(pair, 5)
  with pytest.raises(ValueError, match='lifelong'):
    train.unwrapped.rollout_agents(pair, 5)                                 # (the env itself, with the wrapper's clock configured)
  env = TabletopManipulation3Obj(num_envs=4, device='cpu')
  with pytest.raises(NotImplementedError):
    env.rollout_agents(pair, 5)


# ---------------------------------------------------------------------------------------------------------------- 10. kernel resources
def test_the_pair_kernels_have_no_scratch_and_the_recorded_figures():
  now = kernel_build.unit('tabletop_policy_pair.hip').figures
  assert len(now) == 6 and all('4earl11pair_kernelILi1E' in k for k in now), sorted(now)      # pair_kernel<NOBJ = 1, NT2, GAUSS>: NT2 in {0, 1, 2} x {deterministic, Gaussian head}
  recorded = kernel_build.recorded_figures()
  for name, fig in now.items():
    print(name, fig)
    assert fig[3] == 0, (name, 'scratch', fig[3])
    assert fig[1] + fig[2] <= 512, (name, 'registers', fig[1] + fig[2])
    assert recorded.get(name) == [fig], (name, fig, recorded.get(name))
  assert [k for k in recorded if ('4earl11pair_kernelILi1E' in k or 'policy_pair_kernel' in k) and k not in now] == []      # (nor a line under the kernel's earlier name)

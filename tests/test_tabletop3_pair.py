"""earl_tabletop3_pair_rollout (include/earl_tabletop.h): the forward / reset agent pair alternating inside one closed-loop rollout of the THREE-object tabletop.
Without a GPU, through csrc/libearl_host.so (the host twin) -- and csrc/libearl_hip.so for the argument errors, which come before any HIP call:
  1. never switching is earl_tabletop3_policy_rollout_cpu on the forward row, bit for bit: both heads, evaluation / continuing / auto-reset forms, sparse and dense;
  2. clock-only switching equals the alternating single-policy launches it replaces, the goal installed on the host in between;
  3. without a backward goal the state trajectory equals earl_tabletop3_rollout_cpu fed with act_out;
  4. agent_out, phase, steps_in_phase, goal_idx, both counters and the goal slots of every out->obs row equal the handover rule in numpy applied to the launch's own success / done, in a run that is asserted to hold a
     forward phase ended by success, a reset phase ended by success, a phase ended by the clock, an auto-reset and a held object;
  5. the observation's goal slots 10..19 carry the goal in force after every handover, and goal_idx stays an index the open-loop entry points take;
  6. shards equal the batch, two launches equal one, reset_first puts every env into phase 0 at each reset;
  7. every argument error from both libraries; n = 0;
  8. AgentPair(obs_dim=20, act_dim=3) and TabletopManipulation3Obj.rollout_agents on device='cpu'; the pinned refusals (the one test here that also passes without
     the entry point: it pins what must not change);
  9. the six kernels of csrc/tabletop3_pair.hip: no scratch, within 512 registers, the figures on record; the twelve kernels of csrc/tabletop_pair_kernel.h (this unit's
     and csrc/tabletop_policy_pair.hip's) are instruction for instruction the kernels of the build before they became one text (cross-compiled).
tests/test_tabletop3_pair_gpu.py holds the device to the host twin bit for bit."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import kernel_build
import tabletop3_pair_helpers as p3
import tabletop3_policy_helpers as t3
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import head_struct
from tabletop3_pair_helpers import INITIAL3, OUT, Pair3, PairState, assert_bits, handover_rule, keys_of, pair_rollout3, pair_struct, single_rollout3, with_goal_row
from test_policy_rollout import final_state, restore, snapshot

CPU = 'cpu'
N, OFFSET = t3.N, t3.OFFSET                                  # 40 envs at env_offset 3: three workgroups of the kernel, the last one ragged
HEADS = {'deterministic': None, 'sample_tanh': dict(mode='sample', log_std_map='tanh'), 'sample_clamp': dict(mode='sample', log_std_map='clamp')}
FORMS = {'evaluation': (2, True, dict(horizon=60)), 'continuing': (1, False, dict(horizon=10**6)), 'auto_reset': (1, False, dict(auto_reset=True, horizon=7))}


def assert_state(end, want_state, what=''):
  for k, v in want_state.items():
    np.testing.assert_array_equal(end[k].view(np.uint8), np.ascontiguousarray(v).view(np.uint8), err_msg=f'{what} state {k}')


# ---------------------------------------------------------------------------------------------------------------- 1. never switching
@pytest.mark.parametrize('reward', ['sparse', 'dense'])
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('hidden', [(16,), (48, 32), (64, 128)], ids=str)
def test_never_switching_is_the_single_policy_entry_point_on_the_forward_row(hidden, form, head, reward):
  E, reset_first, cfg_kw = FORMS[form]
  T = 18
  pr = Pair3(hidden, gaussian=HEADS[head] is not None, hidden_act='tanh' if len(hidden) == 2 else 'relu', seed0=len(hidden) * 10)
  h = p3.prepared(CPU, reset_first, reward_type=reward, reset_at_goal=True, seed=11, **cfg_kw)
  snap = snapshot(h)
  ps = PairState(N)
  got = pair_rollout3(h, pr, ps, E, T, reset_first, T + 1, 0, head=HEADS[head])
  end = final_state(h)
  assert not any(np.isnan(got[k]).any() for k in keys_of(HEADS[head]) if got[k].dtype == np.float32), 'an output was not written, or a read left the agent\'s parameters'
  restore(h, snap)
  want = single_rollout3(h, pr.members[0], E, T, reset_first, head=HEADS[head])
  assert_bits(got, want, keys_of(HEADS[head]))
  again = final_state(h)
  assert_state(end[0], again[0])
  assert end[1] == again[1] == snap[1] + (E * (T + 1) if reset_first else T)
  assert (got['agent'] == 0).all() and (got['fs'] == 0).all() and (got['bs'] == 0).all() and (ps.host()[0] == 0).all()
  if form == 'auto_reset':
    assert got['done'].any() and (ps.host()[1] == (9 + T) % 7).all()
  elif form == 'continuing':
    assert (ps.host()[1] == T).all()


# ---------------------------------------------------------------------------------------------------------------- 2. clock-only switching
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('goal', [None, 'initial'])
@pytest.mark.parametrize('switch_every', [(7, 5), (1, 3)], ids=str)
def test_clock_only_switching_equals_the_alternating_single_policy_launches(switch_every, goal, head):
  """what a user did before: chunks of switch_every[k] steps of earl_tabletop3_policy_rollout (reset_first = 0) with agent k's parameters; between chunks the goal is
  installed on the host -- the reset agent's row appended to the goal table and goal_idx pointed at it, resp. goal_idx set to the index drawn at the handover step's
  counter.  The chunk's last observation row is re-read with the installed goal, which is what the next chunk's first action sees."""
  T = 23
  pr = Pair3((64,), gaussian=HEADS[head] is not None, seed0=2)
  h = p3.prepared(CPU, False, reward_type='sparse', reset_at_goal=True, seed=5, horizon=10**6)
  row = with_goal_row(h, INITIAL3)
  snap = snapshot(h)
  ps = PairState(N)
  got = pair_rollout3(h, pr, ps, 1, T, False, switch_every, 0, backward_goal=None if goal is None else INITIAL3, head=HEADS[head])
  end = final_state(h)
  restore(h, snap)
  task = h.host('goal_idx').copy()
  table = h.goal_table.cpu().numpy()
  parts, agents, phase, t, sip, draws = [], [], 0, 0, 0, 0
  while t < T:
    m = min(switch_every[phase], T - t)
    part = single_rollout3(h, pr.members[phase], 1, m, False, head=HEADS[head])
    agents.append(np.full((m, N), phase, np.int8))
    t += m
    sip = m
    if m == switch_every[phase]:                              # the handover after the chunk's last step, whose Philox counter is the launch's last
      phase, sip = phase ^ 1, 0
      if phase == 0:
        task = p3.goal_draw3(h, int(h.cfg.counter) - 1)
        draws += 1
        h.goal_idx.copy_(torch.from_numpy(task))
      elif goal is not None:
        h.goal_idx.fill_(row)
      part['obs'][-1, :, 10:] = table[h.host('goal_idx')].astype(np.float32)
    parts.append(part)
  assert draws >= 1 and len(np.unique(task)) > 1             # the forward goal was drawn, and not every env drew the same row
  want = {k: np.concatenate([p[k] for p in parts], axis=0) for k in keys_of(HEADS[head])}
  assert_bits(got, want, keys_of(HEADS[head]))
  np.testing.assert_array_equal(got['agent'], np.concatenate(agents, axis=0))
  want_state = final_state(h)[0]
  want_state['goal_idx'] = task                               # the pair leaves the env's TASK goal in goal_idx, also while the reset agent's row is in force
  assert_state(end[0], want_state)
  assert end[1] == snap[1] + T
  assert (ps.host()[0] == phase).all() and (ps.host()[1] == sip).all() and (got['fs'] == 0).all() and (got['bs'] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. the state trajectory
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_the_state_trajectory_equals_the_open_loop_rollout_fed_with_act_out(head):
  """without a backward goal the pair changes which goal an env sees, never how the env moves: qpos and the held flags of every step, and the state left behind but
  for goal_idx, are those of earl_tabletop3_rollout_cpu on the launch's own actions (auto-reset included: its draws are keyed by the same counters)"""
  T = 24
  pr = Pair3((48, 32), gaussian=HEADS[head] is not None, hidden_act='tanh', seed0=7)
  h = p3.prepared(CPU, False, reward_type='sparse', seed=3, auto_reset=True, horizon=7)
  snap = snapshot(h)
  rng = np.random.default_rng(0)
  ps = PairState(N, phase=rng.integers(0, 2, N), sip=rng.integers(0, 3, N))
  got = pair_rollout3(h, pr, ps, 1, T, False, (5, 3), 1, head=HEADS[head])
  end = final_state(h)
  assert got['done'].any() and 0 < got['agent'].mean() < 1
  restore(h, snap)
  want = dict(zip(OUT, h.rollout(np.ascontiguousarray(got['act']))))
  np.testing.assert_array_equal(got['obs'][..., :10].view(np.uint32), want['obs'][..., :10].view(np.uint32))
  np.testing.assert_array_equal(got['done'], want['done'])
  again = final_state(h)
  for k in ('qpos', 'attached', 'steps_since_reset', 'num_interventions'):
    np.testing.assert_array_equal(end[0][k].view(np.uint8), again[0][k].view(np.uint8), err_msg=k)
  assert end[1] == again[1]


# ---------------------------------------------------------------------------------------------------------------- 4. the handover rule, with the coverage condition
def coverage_run(device, head_name, switch_every=(3, 2), T=24):
  """envs at the initial state (no reset_at_goal) with `still_pair`: the arm stays put, so a forward phase whose drawn goal is the table's INITIAL3 row and every reset
  phase (backward_goal = 'initial') succeed at once, a forward phase with another goal ends by the clock, horizon 7 < T auto-resets every env, and the envs whose
  gripper was put 0.1 beside object 0 latch it as soon as the forward agent closes the gripper.  -> (results, PairState, (start phase, clock, goal_idx, Philox counter), harness)"""
  h = p3.harness(device, reward_type='sparse', seed=9, auto_reset=True, horizon=7)
  h.reset()
  q = h.host('qpos').copy()
  near = np.arange(N) % 4 == 0
  q[near, 0:2] = q[near, 2:4] + np.array([0.1, 0.0])
  h.qpos.copy_(torch.from_numpy(q))
  rng = np.random.default_rng(0)
  phase, sip = rng.integers(0, 2, N).astype(np.int8), rng.integers(0, 2, N).astype(np.int32)
  ps = PairState(N, device=device, phase=phase, sip=sip)
  pr = p3.still_pair(gaussian=HEADS[head_name] is not None, device=device)
  start = (phase, sip, h.host('goal_idx').copy(), int(h.cfg.counter))
  got = pair_rollout3(h, pr, ps, 1, T, False, switch_every, 1, backward_goal=INITIAL3, head=HEADS[head_name])
  return got, ps, start, h


@pytest.mark.parametrize('switch_every', [(3, 2), (1, 1)], ids=str)
@pytest.mark.parametrize('head', ['deterministic', 'sample_clamp'])
def test_agent_phase_clock_and_counters_equal_the_rule_on_the_launch_s_own_flags(head, switch_every):
  T = 24
  got, ps, (phase, sip, goal0, counter0), h = coverage_run(CPU, head, switch_every, T)
  lead = (1, T, N)
  agent, ph, sp, fs, bs, causes = handover_rule(got['success'].reshape(lead), got['done'].reshape(lead), phase, sip, switch_every, 1, True, False)
  np.testing.assert_array_equal(got['agent'].reshape(lead), agent)
  np.testing.assert_array_equal(ps.host()[0], ph)
  np.testing.assert_array_equal(ps.host()[1], sp)
  np.testing.assert_array_equal(got['fs'], fs)
  np.testing.assert_array_equal(got['bs'], bs)
  held = got['obs'][..., 8] >= 0
  print(head, switch_every, 'handovers (forward by success, forward by clock, reset by success, reset by clock):', causes, 'auto-resets:', int(got['done'].sum()),
        '(env, step) pairs with a held object:', int(held.sum()))
  # the coverage condition
  assert causes[0] > 0, 'no forward phase ended by success'
  assert causes[2] > 0, 'no reset phase ended by success'
  assert causes[1] + causes[3] > 0, 'no phase ended by the clock'
  assert got['done'].any(), 'no auto-reset'
  assert held.any(), 'no held object'
  if switch_every == (1, 1):                                  # a handover at every step that is not an auto-reset
    a, d = got['agent'], got['done'].astype(bool)
    assert ((a[1:] != a[:-1]) | d[:-1]).all()
  # goal_idx left behind and the goal slots of every out->obs row equal the rule: the draw of the last step that entered the forward phase by handover or by
  # auto-reset (the start's where there is none); the backward goal's row after a handover into the reset phase
  gi = h.host('goal_idx')
  want_gi, want_rows = p3.goal_rule(h, got['success'], got['done'], phase, sip, goal0, counter0, switch_every, 1, True, INITIAL3)
  np.testing.assert_array_equal(gi, want_gi)
  np.testing.assert_array_equal(got['obs'][:, :, 10:].view(np.uint32), want_rows.view(np.uint32))
  assert (gi != goal0).any() and len(np.unique(gi)) > 1
  # ... and is a table index the open-loop entry points accept
  assert gi.min() >= 0 and gi.max() < len(p3.TABLE3)
  h.rollout(np.zeros((2, N, 3), np.float32))


def test_the_goal_slots_carry_the_goal_in_force_after_every_handover():
  """the out->obs row of a handover step is the row the next action is computed from: slots 10..19 hold the reset agent's row after a handover to the reset agent, a
  task row after one to the forward agent; between handovers they do not change.  Clock-only, no auto-reset, so the agent of step t + 1 tells what step t did"""
  T, se = 20, (3, 2)
  h = p3.prepared(CPU, False, reward_type='sparse', seed=4, horizon=10**6)
  ps = PairState(N)
  got = pair_rollout3(h, Pair3((32,), seed0=1), ps, 1, T, False, se, 0, backward_goal=INITIAL3)
  goal_seen, agent = got['obs'][:, :, 10:], got['agent']
  table32 = p3.TABLE3.astype(np.float32)
  assert not (table32 == INITIAL3.astype(np.float32)).all(axis=1)[[0, 2]].any()
  for t in range(T - 1):
    nxt = agent[t + 1]
    is_init = (goal_seen[t] == INITIAL3.astype(np.float32)).all(axis=1)
    is_task = (goal_seen[t][:, None, :] == table32[None]).all(axis=2).any(axis=1)
    assert is_init[nxt == 1].all(), t
    assert is_task[nxt == 0].all(), t
  assert (ps.host()[0] == 0).all() and T % sum(se) < se[0]      # the launch ends in a forward phase: the last row's goal is the task goal left in goal_idx
  np.testing.assert_array_equal(goal_seen[-1], table32[h.host('goal_idx')])
  assert len(np.unique(h.host('goal_idx'))) > 1                # the forward handover drew, per env


# ---------------------------------------------------------------------------------------------------------------- 6. split launches, shards, reset_first
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_two_launches_equal_one_and_two_ragged_shards_equal_the_batch(head):
  T1, T2 = 11, 13
  kw = dict(reward_type='sparse', reset_at_goal=True, seed=21, auto_reset=True, horizon=7)
  pr = Pair3((64,), gaussian=HEADS[head] is not None, seed0=5)
  args = dict(switch_every=(4, 3), switch_on_success=1, backward_goal=INITIAL3, head=HEADS[head])
  whole = p3.prepared(CPU, False, **kw)
  snap = snapshot(whole)
  ps = PairState(N)
  got = pair_rollout3(whole, pr, ps, 1, T1 + T2, False, **args)
  end = final_state(whole)
  assert 0 < got['agent'].mean() < 1
  restore(whole, snap)
  ps2 = PairState(N)
  a = pair_rollout3(whole, pr, ps2, 1, T1, False, **args)
  b = pair_rollout3(whole, pr, ps2, 1, T2, False, **args)
  keys = keys_of(HEADS[head]) + ('agent',)
  assert_bits({k: np.concatenate([a[k], b[k]], axis=0) for k in keys}, got, keys)
  np.testing.assert_array_equal(a['fs'] + b['fs'], got['fs'])
  np.testing.assert_array_equal(a['bs'] + b['bs'], got['bs'])
  assert_state(final_state(whole)[0], end[0])
  assert final_state(whole)[1] == end[1]
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])
  np.testing.assert_array_equal(ps2.host()[1], ps.host()[1])
  parts, states, pss = [], [], []
  for i0, m in ((0, 25), (25, 15)):                           # the cut is inside a workgroup of the batch
    hs = p3.harness(CPU, n=m, env_offset=OFFSET + i0, **kw)
    for k, v in snap[0].items():
      getattr(hs, k).copy_(v[i0:i0 + m])
    hs.cfg.counter = snap[1]
    p = PairState(m)
    parts.append(pair_rollout3(hs, pr, p, 1, T1 + T2, False, **args))
    states.append(final_state(hs))
    pss.append(p.host())
  assert_bits({k: np.concatenate([p[k] for p in parts], axis=1) for k in keys + ('fs', 'bs')}, got, keys + ('fs', 'bs'))
  assert_state({k: np.concatenate([s[0][k] for s in states], axis=0) for k in end[0]}, end[0])
  assert states[0][1] == states[1][1] == end[1]
  np.testing.assert_array_equal(np.concatenate([p[0] for p in pss]), ps.host()[0])
  np.testing.assert_array_equal(np.concatenate([p[1] for p in pss]), ps.host()[1])


def test_reset_first_puts_every_env_into_the_forward_phase_at_each_reset():
  T = 12
  h = p3.prepared(CPU, True, reward_type='sparse', seed=2, horizon=60)
  ps = PairState(N, phase=np.ones(N), sip=np.full(N, 2))
  got = pair_rollout3(h, Pair3((32,), seed0=3), ps, 2, T, True, (5, 4), 0, backward_goal=INITIAL3)
  assert got['agent'].shape == (2, T, N) and (got['agent'][:, :5] == 0).all() and (got['agent'][:, 5:9] == 1).all() and (got['agent'][:, 9:] == 0).all()
  assert (ps.host()[0] == 0).all() and (ps.host()[1] == 3).all()


def test_null_outputs_leave_the_state_what_it_was():
  T = 16
  kw = dict(reward_type='dense', reset_at_goal=True, seed=2, horizon=10**6)
  pr = Pair3((32,), gaussian=True, seed0=1)
  args = dict(switch_every=(4, 3), switch_on_success=1, backward_goal=INITIAL3, head=HEADS['sample_clamp'])
  h = p3.prepared(CPU, False, **kw)
  snap = snapshot(h)
  ps = PairState(N)
  pair_rollout3(h, pr, ps, 1, T, False, **args)
  end = final_state(h)
  restore(h, snap)
  ps2 = PairState(N)
  bare = pair_rollout3(h, pr, ps2, 1, T, False, null=OUT + ('act', 'eps', 'agent', 'fs', 'bs'), **args)
  for k in OUT + ('act', 'eps'):
    assert np.isnan(bare[k]).all() if bare[k].dtype == np.float32 else (bare[k] == 7).all()
  assert (bare['agent'] == 7).all() and (bare['fs'] == -7).all() and (bare['bs'] == -7).all()
  assert_state(final_state(h)[0], end[0])
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])
  np.testing.assert_array_equal(ps2.host()[1], ps.host()[1])


# ---------------------------------------------------------------------------------------------------------------- 7. argument errors
def _edge_calls(lib, host):
  h = p3.harness(CPU)
  st = h._state()
  arrs, out = h._outs((1, 4, N))
  det, gau, wide = Pair3((16,)), Pair3((16,), gaussian=True), Pair3((16, 144))
  ps = PairState(N)
  good_head = head_struct()
  from test_policy_rollout import Policy
  twelve = Policy((16,), seed=0)

  def pairv(p=det, **kw):
    s = pair_struct(p, ps, (5, 5), 1)
    for k, v in kw.items():
      setattr(s, k, v)
    return s

  def call(cfg=h.cfg, state=st, p=det.struct, pair=pairv(), hd=None, E=1, T=4, rf=1, o=out):
    ref = lambda x: C.byref(x) if x is not None else None
    args = [ref(cfg), ref(state), ref(p), ref(pair), ref(hd), E, T, rf, ref(o), None]
    return lib.earl_tabletop3_pair_rollout_cpu(*args) if host else lib.earl_tabletop3_pair_rollout(*args, None)

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
         dict(cfg=cfgv(goal_change_frequency=10)), dict(cfg=cfgv(wide_init=1)),                                                                 # the three-object env has neither
         dict(p=wide.struct, pair=pairv(wide)),                                                                                                 # H2 = 144 > EARL_PAIR_MAX_H2
         dict(p=twelve.struct, pair=pairv(param_stride=twelve.params.numel())), dict(p=variant(det.struct, dims=(12, 16, 3, 0))),               # the single-object env's 12-wide input
         dict(hd=good_head), dict(p=gau.struct, pair=pairv(gau)),                                                                               # head and dims[n_layers] disagree
         dict(p=gau.struct, pair=pairv(gau), hd=head_struct(mode=2)), dict(p=gau.struct, pair=pairv(gau), hd=head_struct(bounds=(1.0, -1.0))),
         # what the single-policy entry point refuses
         dict(cfg=None), dict(state=None), dict(p=None), dict(o=None), dict(p=variant(det.struct, params=None)), dict(p=variant(det.struct, precision=1)),
         dict(p=variant(det.struct, dims=(20, 24, 3, 0))), dict(p=variant(det.struct, hidden_act=0)), dict(T=0), dict(E=0), dict(E=2, rf=0), dict(rf=2)]
  err = lib.earl_host_last_error if host else lib.earl_last_error
  for kw in bad:
    assert call(**kw) == -1, kw
    assert err(), kw
  assert call(p=wide.struct, pair=pairv(wide)) == -1
  assert b'EARL_PAIR_MAX_H2 = 128' in err()
  assert call(cfg=cfgv(n=0)) == 0                                           # the empty batch is not an error
  call.keep = (h, arrs, det, gau, wide, ps, twelve)
  return call, gau, good_head, pairv


def test_argument_errors_from_the_host_library():
  lib = _abi.load_host()
  call, gau, good_head, pairv = _edge_calls(lib._cdll, True)
  assert call() == 0                                                       # the good call runs (host pointers)
  assert call(p=gau.struct, pair=pairv(gau), hd=good_head) == 0
  assert call(pair=pairv(backward_goal=None)) == 0 and call(rf=0) == 0
  w128 = Pair3((16, 128))
  assert call(p=w128.struct, pair=pairv(w128)) == 0                      # the widest second hidden layer that ships


def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  _edge_calls(lib, False)
  assert lib.earl_tabletop3_pair_rollout(None, None, None, None, None, 1, 1, 1, None, None, None) == -1
  assert b'NULL' in lib.earl_last_error()


# ---------------------------------------------------------------------------------------------------------------- 8. the Python surface on the host
def layers_of(pol):
  return [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in pol.layers]


def agents_of(gaussian, hidden=(48, 32), **kw):
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  refs = [t3.net3(hidden, gaussian=gaussian, seed=s, log_std_gain=1.0) for s in range(2)]
  if gaussian:
    return refs, [GaussianMLPPolicy(layers_of(r), 'relu', obs_dim=20, act_dim=3, **kw) for r in refs]
  return refs, [MLPPolicy(layers_of(r), 'relu', 'tanh', obs_dim=20, act_dim=3, **kw) for r in refs]


def env3(device=CPU, n=N, **kw):
  from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  return TabletopManipulation(reward_type='sparse', num_envs=n, device=device, seed=5, env_offset=OFFSET, **kw)


def test_agent_pair_at_the_three_object_widths():
  from earl_benchmark_amd.policy import GOAL_DIMS, AgentPair, MLPPolicy, PairPopulation
  refs, pis = agents_of(False, (64,))
  pair = AgentPair(pis[0], pis[1], switch_every=(30, 20), obs_dim=20, act_dim=3)
  assert GOAL_DIMS[(20, 3)] == 10 and pair.goal_dim == 10 and pair.dims == [20, 64, 3] and pair.backward_goal == 'initial'
  assert pair.stride == pair.n_params == refs[0].params.numel()            # the tabletop's rows are taken as they are
  np.testing.assert_array_equal(pair.params.numpy(), np.stack([r.params.numpy() for r in refs]))
  env = env3()
  np.testing.assert_array_equal(pair.goal_row(env).numpy(), INITIAL3)
  assert AgentPair(pis[0], pis[1], backward_goal=None, obs_dim=20, act_dim=3).goal_row(env) is None
  np.testing.assert_array_equal(AgentPair(pis[0], pis[1], backward_goal=p3.TASK3, obs_dim=20, act_dim=3).goal_row(env).numpy(), p3.TASK3)
  for bad in ([0.0] * 6, np.zeros((3, 10)), 'initial_states'):            # a row of the single-object width; a table of goals
    with pytest.raises(ValueError):
      env.rollout_agents(AgentPair(pis[0], pis[1], backward_goal=bad, obs_dim=20, act_dim=3), 4)
  wide = [MLPPolicy(layers_of(t3.net3((16, 144), seed=s)), obs_dim=20, act_dim=3) for s in range(2)]
  with pytest.raises(ValueError, match='128'):
    AgentPair(wide[0], wide[1], obs_dim=20, act_dim=3)
  with pytest.raises(ValueError, match='a PairPopulation runs on the Sawyer door and peg only'):
    saw = [MLPPolicy([(torch.zeros(16, 14), torch.zeros(16)), (torch.zeros(4, 16), torch.zeros(4))], obs_dim=14, act_dim=4) for _ in range(2)]
    env.rollout_agents(PairPopulation([AgentPair(saw[0], saw[1], obs_dim=14, act_dim=4, backward_goal=None)] * 2, 32), 4)
  _, bf = agents_of(False, (16,), param_dtype=torch.bfloat16)
  with pytest.raises(ValueError, match=re.escape('.widened()')):
    env.rollout_agents(AgentPair(bf[0], bf[1], obs_dim=20, act_dim=3), 4)


def test_the_pinned_refusals_stay():
  """a pin of behaviour this entry point must NOT change: unlike the other tests of this file it passes without earl_tabletop3_pair_rollout too"""
  from earl_benchmark_amd.envs.tabletop import TabletopManipulation as OneObject
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  from test_policy_rollout import Policy
  narrow = [MLPPolicy(Policy((16,), seed=s).layers) for s in range(2)]
  with pytest.raises(NotImplementedError, match=re.escape('rollout_agents: single-object env only')):
    env3().rollout_agents(AgentPair(narrow[0], narrow[1]), 4)
  _, pis = agents_of(False, (16,))
  one = OneObject(reward_type='sparse', num_envs=4, device=CPU)
  with pytest.raises(ValueError, match='observation width 20 and action width 3; the tabletop takes 12 and 3'):
    one.rollout_agents(AgentPair(pis[0], pis[1], obs_dim=20, act_dim=3), 4)
  saw = [MLPPolicy([(torch.zeros(16, 14), torch.zeros(16)), (torch.zeros(4, 16), torch.zeros(4))], obs_dim=14, act_dim=4) for _ in range(2)]
  for env in (one, env3()):
    with pytest.raises(ValueError, match='observation width 14 and action width 4'):
      env.rollout_agents(AgentPair(saw[0], saw[1], obs_dim=14, act_dim=4), 4)


@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian'])
def test_rollout_agents_on_the_host(gaussian):
  from earl_benchmark_amd.policy import AgentPair
  refs, agents = agents_of(gaussian)
  T = 20
  env = env3()
  assert env.agent_phase is None and env.steps_in_phase is None and env.pair_counts is None
  env.reset()
  sd = env.state_dict()
  assert 'agent_phase' not in sd
  pair = AgentPair(agents[0], agents[1], switch_every=(4, 3), obs_dim=20, act_dim=3)
  outs = env.rollout_agents(pair, T, **(dict(return_noise=True) if gaussian else {}))
  obs, rew, done, succ, act, agent = outs[:6]
  assert len(outs) == (7 if gaussian else 6)
  assert tuple(obs.shape) == (T, N, 20) and tuple(act.shape) == (T, N, 3) and tuple(agent.shape) == (T, N) and agent.dtype == torch.int8
  assert obs.dtype == torch.float32 and rew.dtype == torch.float32 and done.dtype == torch.bool and succ.dtype == torch.bool
  assert env.total_step_count == T and env.state_dict()['rng_counter'] == sd['rng_counter'] + T
  assert env.agent_phase.dtype == torch.int8 and env.steps_in_phase.dtype == torch.int32 and 0 < float(agent.float().mean()) < 1
  fwd, bwd = env.pair_counts
  assert tuple(fwd.shape) == (1, N) and fwd.dtype == torch.int32 and tuple(bwd.shape) == (1, N)
  # the same launch through the C ABI of the host twin
  h = t3.harness(CPU, reward_type='sparse', seed=5, horizon=int(env._cfg.horizon), goal_table=env.goal_table.numpy(), n_sample_goals=int(env._cfg.n_sample_goals))
  for k, key in (('qpos', 'qpos'), ('attached', 'attached'), ('goal_idx', 'goal_idx'), ('steps_since_reset', 'steps_since_reset'), ('num_interventions', 'interventions')):
    getattr(h, k).copy_(sd[key])
  h.cfg.counter = sd['rng_counter']
  ps = PairState(N)
  got = pair_rollout3(h, Pair3(members=refs, gaussian=gaussian), ps, 1, T, False, (4, 3), 1, backward_goal=INITIAL3, head=HEADS['sample_tanh'] if gaussian else None)
  for k, v in zip(OUT + ('act', 'agent'), (obs, rew, done.to(torch.uint8), succ.to(torch.uint8), act, agent)):
    np.testing.assert_array_equal(v.numpy().view(np.uint8), got[k].view(np.uint8), err_msg=k)
  if gaussian:
    np.testing.assert_array_equal(outs[6].numpy(), got['eps'])
  np.testing.assert_array_equal(env.agent_phase.numpy(), ps.host()[0])
  np.testing.assert_array_equal(env.steps_in_phase.numpy(), ps.host()[1])
  np.testing.assert_array_equal(fwd.numpy(), got['fs'])
  np.testing.assert_array_equal(bwd.numpy(), got['bs'])
  # the state dict carries the pair state now; a round trip continues the stream exactly
  sd1 = env.state_dict()
  assert torch.equal(sd1['agent_phase'], env.agent_phase) and torch.equal(sd1['steps_in_phase'], env.steps_in_phase)
  a = env.rollout_agents(pair, 8)
  env2 = env3()
  env2.load_state_dict(sd1)
  b = env2.rollout_agents(pair, 8)
  assert all(torch.equal(x, y) for x, y in zip(a, b))
  # reset(mask) zeroes the pair state of the masked envs only
  env.agent_phase.fill_(1)
  env.steps_in_phase.fill_(3)
  mask = torch.zeros(N, dtype=torch.bool)
  mask[::3] = True
  env.reset(mask=mask)
  assert (env.agent_phase[mask] == 0).all() and (env.steps_in_phase[mask] == 0).all() and (env.agent_phase[~mask] == 1).all() and (env.steps_in_phase[~mask] == 3).all()
  # the evaluation form, and the argument checks of the method
  o2 = env.rollout_agents(pair, 6, episodes=2, reset_first=True)
  assert tuple(o2[0].shape) == (2, 6, N, 20) and tuple(o2[5].shape) == (2, 6, N) and tuple(env.pair_counts[0].shape) == (2, N) and (o2[5][:, 0] == 0).all()
  with pytest.raises(ValueError):
    env.rollout_agents(pair, 6, episodes=2)
  with pytest.raises(ValueError):
    env.rollout_agents(agents[0], 6)
  if not gaussian:
    with pytest.raises(ValueError):
      env.rollout_agents(pair, 6, sample=False)
  # the other entry points keep working on the state a pair launch leaves behind
  assert int(env.goal_idx.max()) < env.goal_table.shape[0] and int(env.goal_idx.min()) >= 0
  env.rollout_policy(agents[0], 3, reset_first=False)


def test_wrappers_forward_and_the_lifelong_wrapper_refuses():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import AgentPair
  from earl_benchmark_amd.wrappers import LifelongWrapper, PersistentStateWrapper
  _, agents = agents_of(False, (16,))
  pair = AgentPair(agents[0], agents[1], switch_every=3, obs_dim=20, act_dim=3)
  env = PersistentStateWrapper(env3(n=8), episode_horizon=50)
  outs = env.rollout_agents(pair, 5)
  assert tuple(outs[0].shape) == (5, 8, 20) and env.unwrapped.agent_phase is not None
  with pytest.raises(ValueError, match='lifelong'):
    LifelongWrapper(env3(n=8), 10).rollout_agents(pair, 5)
  assert eb.AgentPair is AgentPair


# ---------------------------------------------------------------------------------------------------------------- 9. kernel resources
def test_the_six_kernels_have_no_scratch_and_the_recorded_figures():
  built = kernel_build.units(('tabletop3_pair.hip', 'tabletop_policy_pair.hip'))
  now = built['tabletop3_pair.hip'].figures
  assert len(now) == 6 and all('4earl11pair_kernelILi3E' in k for k in now), sorted(now)      # pair_kernel<NOBJ = 3, NT2, GAUSS>: NT2 in {0, 1, 2} x {deterministic, Gaussian head}
  recorded = kernel_build.recorded_figures()
  for name, fig in now.items():
    print(name, fig)
    assert fig[3] == 0, (name, 'scratch', fig[3])
    assert fig[1] + fig[2] <= 512, (name, 'registers', fig[1] + fig[2])
    assert recorded.get(name) == [fig], (name, fig, recorded.get(name))
  assert [k for k in recorded if ('4earl11pair_kernelILi3E' in k or 'tabletop3_pair_kernel' in k) and k not in now] == []      # (nor a line under the kernel's earlier name)
  single = built['tabletop_policy_pair.hip'].figures                         # the single-object pair keeps its six recorded lines
  assert len(single) == 6
  for name, fig in single.items():
    assert recorded.get(name) == [fig], (name, fig, recorded.get(name))


# unit -> (its kernels' names now, their names in the build on record: one __global__ template <NT2, GAUSS> per unit then)
RENAMED = {'tabletop_policy_pair.hip': ('_ZN4earl11pair_kernelILi1E', '_ZN4earl18policy_pair_kernelI'), 'tabletop3_pair.hip': ('_ZN4earl11pair_kernelILi3E', '_ZN4earl21tabletop3_pair_kernelI')}


def test_the_twelve_kernels_are_instruction_for_instruction_the_build_before_they_became_one_text():
  want = kernel_build.recorded('tabletop_pair_parent_build.json')['kernels']
  built = kernel_build.units(RENAMED)
  now = {}
  for unit, (new, old) in RENAMED.items():
    for name, dig in built[unit].nameless_digests.items():
      assert name.startswith(new), (unit, name)                             # (the units hold no other function)
      now[old + name[len(new):]] = dig
  assert len(want) == 12 and sorted(now) == sorted(want), (sorted(now), sorted(want))
  for name in want:
    print(name, now[name], want[name])
  assert now == want, sorted(k for k in want if now[k] != want[k])

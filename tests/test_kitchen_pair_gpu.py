"""earl_kitchen_agents_rollout (include/earl_physics.h) and Kitchen.rollout_pair / evaluate_pair on the device: the forward / reset agent pair inside ONE launch of the
kitchen rollout kernel in each of its five forms.  Everything is compared bit for bit, through the C ABI with banded buffers (tests/physics_pair_abi.py):
  1. the handover rule: agent, phase, steps_in_phase, counters, st->goal and the patched goal block (out->obs AND last_obs) == items 5 and 6 applied to the launch's
     own success;  2. actions per phase == earl_mlp_policy_forward_cpu with the parameters of agent[t]'s row;
  3. the pair launch == T launches of the plain earl_kitchen_rollout_clocked with the handover applied by the test between them;
  4. never switching == earl_kitchen_population_rollout with row 0 / row 1;  5. the five launch forms and the launcher's choice return the same bits;
  6. one launch of T == T launches of one; two shards == the batch;  7. a population of pairs == its pieces; a table of one row == the fixed row; a table of five rows:
  the recomputed 0xFFFD draw;  8. every optional pointer NULL, the summary == its definitions, also with an env in the failure guard;  9. the Python surface.
Shapes: n = 37 and one case n = 1, T = 6, G = 16, env_offset = 3, switch_every = (3, 2), phase state staggered by global id (phase = g % 2, steps_in_phase = g % 3).
Networks and seeds are tests/test_kitchen_policy_rollout_gpu.py's (small gains, sensor noise on): at most 1 % of the rows outside a poisoned env sit in the failure guard,
a condition on the inputs.  Success is made, not hoped for: the env is built for ONE task, so every env resets to the same settled qpos; a goal row equal to it succeeds at
once (success compares the fourteen fixture entries within 0.3), the task goal is 0.8 or more away and never does within six steps of an arm that barely moves."""
import numpy as np
import pytest

import physics_pair_abi as pp
import population_abi as pa
from physics_abi import Snapshot, form, same
from test_kitchen_policy_rollout_gpu import policy
from test_physics_step_graph_gpu import make

pytestmark = pytest.mark.gpu

N, T6, OFF = 37, 6, 3
SOLOS = (0, 1, 2, 3, 4)
NEVER = (1000, 1000)
_SNAPS = {}


def snapshot(n=N, seed=6):
  """a freshly reset single-task env of n envs at env_offset = 3, made once per shape and left unchanged; .here: the settled reset qpos, .there: the task goal,
  .fwd: the forward table of the two, .table5: five backward goals, rows 0 and 3 the reset qpos"""
  if (n, seed) not in _SNAPS:
    env = make('kitchen', n, seed=seed, env_offset=OFF, task='microwave')
    assert env.sensor_noise
    snap = Snapshot('kitchen', env)
    q = snap.state['qpos'].cpu().numpy()
    assert np.array_equal(q, np.repeat(q[:1], n, 0))                      # one task: one reset row
    snap.here, snap.there = q[0].copy(), snap.state['goal'][0].cpu().numpy().copy()
    assert np.linalg.norm(snap.here[9:] - snap.there[9:]) > 0.6
    snap.fwd = np.stack([snap.here, snap.there])
    far = [snap.there + 0.01 * k for k in (1, 2)]
    snap.table5 = np.stack([snap.here, snap.there, far[0], snap.here, far[1]])
    _SNAPS[n, seed] = snap
  return _SNAPS[n, seed]


def pairs_of(n, hidden, head, hidden_act='relu'):
  return pp.make_pairs('kitchen', policy, max(n, 17), OFF, hidden, head, hidden_act)


def member_of(n):
  return (OFF + np.arange(n)) // pp.G


# ---------------------------------------------------------------------------------------------------------------- 1. + 2. the handover rule, the actions per phase
@pytest.mark.parametrize('solo,sos,head', [(0, 0, None), (0, 1, 'sample'), (1, 1, None), (2, 1, 'sample'), (3, 1, None), (4, 1, 'sample'), (3, 0, 'sample')])
def test_handover_rule_and_actions_per_phase(solo, sos, head):
  snap, pairs = snapshot(), pairs_of(N, (16,), head)
  ph, sp = pp.stagger(snap)
  what = f'solo={solo}'
  with form(solo=solo):
    res, _ = pp.launch(snap, T6, 0x00, pairs, head=head, phase=ph, sip=sp, sos=sos, goal=snap.here, fwd=snap.fwd)
  causes = pp.check_handover(snap, res, what, ph, sp, sos=sos, goal=snap.here, fwd=snap.fwd)
  if sos:
    pp.all_four_events(causes, what)
  else:
    assert causes[0] == causes[2] == 0 and causes[1] > 0 and causes[3] > 0
  pp.check_actions(snap, res, pairs, head, what, member_of=member_of(N))
  pp.check_summary(res, what)
  pa.guard_ok(res, what)


@pytest.mark.parametrize('hidden,solo', [((48, 80), 0), ((256, 256), 4)])
def test_actions_per_phase_in_wider_networks(hidden, solo):
  snap, pairs = snapshot(), pairs_of(N, hidden, 'sample', 'tanh')
  ph, sp = pp.stagger(snap)
  with form(solo=solo):
    res, _ = pp.launch(snap, T6, 0xFF, pairs, head='sample', phase=ph, sip=sp, goal=snap.here, fwd=snap.fwd)
  pp.check_actions(snap, res, pairs, 'sample', f'solo={solo}', member_of=member_of(N))
  pa.guard_ok(res, f'solo={solo}')


# ---------------------------------------------------------------------------------------------------------------- 3. the step-by-step procedure
@pytest.mark.parametrize('solo,tabled', [(0, True), (3, False)])
def test_pair_launch_equals_the_step_by_step_procedure(solo, tabled):
  snap, pairs = snapshot(), pairs_of(N, (16,), 'sample')
  ph, sp = pp.stagger(snap)
  kw = dict(table=snap.table5, fwd=snap.fwd) if tabled else dict(goal=snap.here, fwd=snap.fwd)
  with form(solo=solo):
    res, _ = pp.launch(snap, T6, 0x00, pairs, head='sample', phase=ph, sip=sp, **kw)
  with form():
    want = pp.stepwise(snap, res['actions'], ph, sp, **kw)
  pp.same_results(res, want, f'solo={solo} vs the step-by-step procedure', keys=sorted(want))
  assert int(res['pair.bs'].sum()) > 0 and int(res['pair.fs'].sum()) > 0
  pa.guard_ok(res, f'solo={solo}')


# ---------------------------------------------------------------------------------------------------------------- 4. never switching
@pytest.mark.parametrize('solo,k', [(0, 0), (4, 1), (1, 1)])
def test_never_switching_equals_the_population_entry_point(solo, k):
  snap, pairs = snapshot(), pairs_of(N, (16,), 'sample')
  with form(solo=solo):
    res, _ = pp.launch(snap, T6, 0x00, pairs, head='sample', phase=np.full(N, k, np.int8), se=NEVER, sos=0, goal=snap.here if k == 0 else None,
                       fwd=snap.fwd if k == 0 else None)
    want, _ = pa.launch(snap, T6, 0xFF, pairs.row(k), head='sample')
  pp.same_results(res, want, f'solo={solo} never switching, row {k}', keys=sorted(want))
  assert bool((res['pair.agent'] == k).all()) and int(res['pair.fs'].sum()) == int(res['pair.bs'].sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- 5. launch forms
@pytest.mark.parametrize('head', [None, 'sample'])
def test_all_launch_forms_return_the_same_bits(head):
  res = {}
  snap, pairs = snapshot(), pairs_of(N, (16,), head, 'tanh')
  ph, sp = pp.stagger(snap)
  for solo in SOLOS + (-1,):
    with form(solo=solo):
      res[solo], _ = pp.launch(snap, T6, 0x00 if solo & 1 else 0xFF, pairs, head=head, phase=ph, sip=sp, table=snap.table5, fwd=snap.fwd)
  for solo in res:
    assert set(res[solo]) == set(res[0])
    pp.same_results(res[0], res[solo], f'solo={solo}')
  pp.all_four_events(pp.check_handover(snap, res[3], 'solo=3', ph, sp, table=snap.table5, fwd=snap.fwd), 'forms')
  pa.guard_ok(res[0], 'forms')


@pytest.mark.parametrize('solo', SOLOS + (-1,))
def test_one_env(solo):
  """n = 1 at global id 3 (it starts in the reset phase): in every form, against the host's rule and the pair-only call"""
  snap, pairs = snapshot(1), pairs_of(1, (16,), 'sample')
  ph, sp = pp.stagger(snap)
  kw = dict(head='sample', phase=ph, sip=sp, goal=snap.here, fwd=snap.fwd)
  with form(solo=solo):
    full, _ = pp.launch(snap, T6, 0x00, pairs, **kw)
    alone, _ = pp.launch(snap, T6, 0xFF, pairs, pop=False, member=0, **kw)
  pp.same_results(full, alone, f'n = 1 solo={solo}')
  pp.check_handover(snap, full, f'n = 1 solo={solo}', ph, sp, goal=snap.here, fwd=snap.fwd)
  pp.check_actions(snap, full, pairs, 'sample', f'n = 1 solo={solo}')
  pp.check_summary(full, f'n = 1 solo={solo}')


# ---------------------------------------------------------------------------------------------------------------- 6. cutting in time and in space
@pytest.mark.parametrize('solo', (0, 4))
def test_one_launch_of_T_equals_T_launches_of_one_and_two_shards_equal_the_batch(solo):
  import torch
  snap, pairs = snapshot(), pairs_of(N, (16,), 'sample')
  ph, sp = pp.stagger(snap)
  kw = dict(head='sample', table=snap.table5, fwd=snap.fwd)
  with form(solo=solo):
    full, _ = pp.launch(snap, T6, 0x00, pairs, phase=ph, sip=sp, **kw)
    parts = [pp.launch(snap, T6, 0xFF, pairs, phase=ph, sip=sp, rows=r, **kw)[0] for r in ((0, 19), (19, N))]      # cut inside a wave and inside a member
    state, p, s, row, steps = snap.state, ph, sp, None, []
    for t in range(T6):
      one, _ = pp.launch(snap, 1, 0x00, pairs, phase=p, sip=s, state=state, dt=t, row0=row, **kw)
      steps.append(one)
      state = {f: one['st.' + f] for f in snap.state}
      p, s, row = one['pair.phase'].cpu().numpy(), one['pair.sip'].cpu().numpy(), one['goals.row'].cpu().numpy()
  pp.same_results(full, pp.concat(parts), f'solo={solo} shards')
  for k in [k for k in full if k.startswith('out.') or k in ('actions', 'eps') + pp.PAIR_T_KEYS]:
    same(full[k], torch.cat([o[k] for o in steps]), f'solo={solo} T launches of one: {k}')
  for k in [k for k in full if k.startswith('st.')] + ['pair.phase', 'pair.sip', 'goals.row']:
    same(full[k], steps[-1][k], f'solo={solo} T launches of one: {k}')
  for k in ('pair.fs', 'pair.bs'):
    same(full[k], sum(o[k] for o in steps), f'solo={solo} T launches of one: {k}')
  pa.guard_ok(full, f'solo={solo}')


# ---------------------------------------------------------------------------------------------------------------- 7. population and table
@pytest.mark.parametrize('solo', (0, 3))
def test_population_of_pairs_equals_its_pieces_and_a_table_of_one_row_equals_the_fixed_row(solo):
  snap, pairs = snapshot(), pairs_of(N, (16,), 'sample')
  ph, sp = pp.stagger(snap)
  kw = dict(head='sample', phase=ph, sip=sp, fwd=snap.fwd)
  with form(solo=solo):
    full, _ = pp.launch(snap, T6, 0x00, pairs, table=snap.table5, **kw)
    pieces = pa.member_pieces(OFF, N)
    assert len(pieces) >= 3 and any(hi - lo < pp.G for lo, hi, _ in pieces)
    parts = [pp.launch(snap, T6, 0xFF, pairs, table=snap.table5, pop=False, member=p, rows=(lo, hi), **kw)[0] for lo, hi, p in pieces]
    fixed, _ = pp.launch(snap, T6, 0x00, pairs, goal=snap.there, **kw)
    one_row, _ = pp.launch(snap, T6, 0xFF, pairs, table=snap.there[None], **kw)
    one_fwd, _ = pp.launch(snap, T6, 0xFF, pairs, goal=snap.there, head='sample', phase=ph, sip=sp, fwd=snap.here[None])
  pp.same_results(full, pp.concat(parts), f'solo={solo} population of pairs vs pieces')
  pp.same_results(fixed, one_row, f'solo={solo} a table of one row vs the fixed row', keys=sorted(fixed))
  assert bool(((one_row['goals.row_out'] == 0) | (one_row['goals.row_out'] == -1)).all()) and bool((one_row['goals.row_out'] == 0).any())
  pp.check_handover(snap, full, f'solo={solo}', ph, sp, table=snap.table5, fwd=snap.fwd)
  pp.check_handover(snap, one_fwd, f'solo={solo} a forward table of one row', ph, sp, goal=snap.there, fwd=snap.here[None])
  assert len(set(full['goals.row_out'][full['goals.row_out'] >= 0].tolist())) == 5      # every row of the table was drawn
  pa.guard_ok(full, f'solo={solo}')


# ---------------------------------------------------------------------------------------------------------------- 8. outputs and summary
@pytest.mark.parametrize('solo', SOLOS)
def test_null_pointers_and_summary_with_an_env_in_the_failure_guard(solo):
  """the poisoning of tests/test_kitchen_population_gpu.py: an obs0 whose row 7 is NaN (last_obs finite), tanh hidden units: NaN actions at step 0, the step diverges, is
  rolled back -- it counts with success 0 and advances steps_in_phase -- and step 1 acts on the last stable row"""
  bad = 7
  snap = snapshot()
  obs0 = snap.state['last_obs'].clone()
  obs0[bad] = float('nan')
  head = 'sample' if solo in (1, 3) else None
  pairs = pairs_of(N, (16,), head, 'tanh')
  ph, sp = pp.stagger(snap)
  kw = dict(head=head, phase=ph, sip=sp, table=snap.table5, fwd=snap.fwd, obs0=obs0)
  every = {'actions', 'pair.agent', 'pair.fs', 'pair.bs', 'goals.row', 'goals.row_out'} | ({'eps'} if head else set()) | {'out.' + k for k in pa.T_OUT}
  with form(solo=solo):
    full, _ = pp.launch(snap, T6, 0x00, pairs, **kw)
    bare = [pp.launch(snap, T6, fill, pairs, null=every, **kw)[0] for fill in (0x00, 0xFF)]
    each = {k: pp.launch(snap, T6, (0x00, 0xFF)[i & 1], pairs, null={k}, **kw)[0] for i, k in enumerate(sorted(every))}
  what = f'solo={solo}'
  pp.check_summary(full, what)
  pa.guard_ok(full, what, bad)
  assert full['out.status'][:, bad].tolist() == [1] + [0] * (T6 - 1) and int(full['st.fail_count'][bad]) == 1
  assert float(full['out.reward'][0, bad]) == 0.0 and int(full['out.success'][0, bad]) == 0
  pp.check_handover(snap, full, what, ph, sp, table=snap.table5, fwd=snap.fwd)      # (the rolled-back step included: success 0, steps_in_phase advanced)
  keep = [k for k in full if k.startswith(('st.', 'sum.')) or k in ('pair.phase', 'pair.sip')]
  for got in bare:
    assert not (set(got) & every)
    pp.same_results(got, full, what + ' every optional pointer NULL', keys=keep)
  for k, got in each.items():
    assert k not in got
    pp.same_results(got, full, f'{what} {k} NULL', keys=[x for x in full if x != k])


# ---------------------------------------------------------------------------------------------------------------- 9. the Python surface
def test_rollout_pair_and_evaluate_pair():
  import torch
  from earl_benchmark_amd.policy import AgentPair, PairPopulation
  n, T = N, T6
  mk = lambda seed: policy((16,), 'relu', head='sample', seed=seed)[0]
  members = [AgentPair(mk(10 + 2 * p), mk(11 + 2 * p), switch_every=(3, 2), backward_goal='initial_states', obs_dim=46, act_dim=9) for p in range(3)]
  pop = PairPopulation(members)
  assert members[0].goal_dim == 23 and pop.pair(1).obs_dim == 46 and pop.pair(1).act_dim == 9
  ea, eb = make('kitchen', n, seed=6, env_offset=OFF), make('kitchen', n, seed=6, env_offset=OFF)
  with pytest.raises(NotImplementedError, match='AgentPair on the kitchen'):
    ea.rollout_agents(members[0], 3)
  with pytest.raises(ValueError, match='initial_states'):                 # six initial states: 'initial' cannot pick one
    ea.rollout_pair(AgentPair(mk(10), mk(11), backward_goal='initial', obs_dim=46, act_dim=9), 3)
  assert ea.agent_phase is None and 'agent_phase' not in ea.state_dict()
  c0 = ea._counter
  out = ea.rollout_pair(pop, T, return_noise=True)
  assert tuple(out['backward_row'].shape) == (T, n) and out['backward_row'].dtype == torch.int32 and tuple(out['agent'].shape) == (T, n) and out['agent'].dtype == torch.int8
  assert tuple(out['actions'].shape) == (T, n, 9) and ea.total_step_count == T and ea._counter == c0 + T
  same(ea.goal_t, out['obs'][-1][:, 23:].contiguous(), 'goal_t is the goal in force')
  same(ea.last_obs, out['obs'][-1], 'last_obs is the last emitted row')
  init = torch.as_tensor(np.asarray(ea.get_init_states(), np.float64), device='cuda')
  drew = out['backward_row'] >= 0
  assert bool(drew.any()) and bool((out['obs'][drew][:, 23:] == init[out['backward_row'][drew].long()]).all())      # 'initial_states' resolved to get_init_states()
  same(ea.backward_row >= 0, drew.any(0), 'env.backward_row is set where a row was drawn')
  ev = eb.evaluate_pair(pop, T)
  assert set(ev) == {'ret', 'success', 'first_success', 'guard_steps', 'forward_success', 'backward_success'} and all(tuple(v.shape) == (n,) for v in ev.values())
  ret, last, first = pa.summary_by_definition(out['reward'], out['success'])
  same(ev['ret'], ret, 'ret')
  same(ev['success'].to(torch.uint8), last, 'success')
  same(ev['first_success'], first, 'first_success')
  same(ev['guard_steps'], (out['status'] != 0).sum(0).to(torch.int32), 'guard_steps')
  same(ev['forward_success'], ea.pair_counts[0], 'forward_success')
  same(ev['backward_success'], ea.pair_counts[1], 'backward_success')
  for k in ('qpos', 'qvel', 'mocap_pos', 'goal_t', 'last_qp_robot', 'last_obs', 'att', 'fail_count', 'agent_phase', 'steps_in_phase', 'backward_row'):
    same(getattr(ea, k), getattr(eb, k), k)
  assert ea._counter == eb._counter and float((out['status'] != 0).float().mean()) <= pa.MAX_GUARD_SHARE
  # the state dict round trip; reset() zeroes the phase of the reset envs; reset_goal() marks last_obs stale
  sd = ea.state_dict()
  assert {'agent_phase', 'steps_in_phase', 'backward_row'} <= set(sd)
  ec = make('kitchen', n, seed=6, env_offset=OFF)
  ec.load_state_dict(sd)
  a, c = ea.rollout_pair(pop, 4), ec.rollout_pair(pop, 4)
  for k in a:
    same(a[k], c[k], 'after load_state_dict: ' + k)
  mask = torch.arange(n, device='cuda') % 2 == 0
  ea.agent_phase.fill_(1)
  ea.reset(mask)
  assert bool((ea.agent_phase[mask] == 0).all()) and bool((ea.agent_phase[~mask] == 1).all()) and bool((ea.steps_in_phase[mask] == 0).all())
  assert bool((ea.backward_row[mask] == -1).all())
  ea.reset()
  assert int(ea.agent_phase.abs().sum()) == 0 and bool((ea.backward_row == -1).all())
  ea.reset_goal()
  assert ea._last_obs_stale
  # nothing that grows with T: the smallest tensor with a T axis a launch could allocate is [T, N] int8, which adds 3 T N bytes between T and 4 T (the caching
  # allocator hands out whole 512-byte blocks, and the first call after other work may find another block free: one call to settle that)
  eb.evaluate_pair(pop, T)
  peaks = []
  for t in (T, 2 * T, 4 * T):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    eb.evaluate_pair(pop, t)
    torch.cuda.synchronize()
    peaks.append(torch.cuda.max_memory_allocated() - base)
  print('evaluate_pair peak bytes above the resident state at T, 2 T, 4 T:', peaks)
  assert max(peaks) - min(peaks) < 3 * T * n, peaks

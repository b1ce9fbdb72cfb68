"""earl_minitaur_population_rollout (include/earl_physics.h) on the device: a population of policies in ONE launch of either minitaur rollout kernel, per-env episode
summaries, every [T] pointer optional.  Everything is compared bit for bit, through the C ABI with banded buffers (tests/population_abi.py):
  1. the population launch equals its pieces through earl_minitaur_policy_rollout;  2. pop = summary = NULL equals earl_minitaur_policy_rollout;
  3. the four launch forms return the same bits;  4. the summary equals its definitions, also for an env in the failure guard;
  5. every [T] pointer NULL, and each in turn;  6. two shards equal the batch;  7. a goal switch inside the launch with the carried row;
  8. evaluate_population equals the definitions applied to rollout_population's arrays, and allocates nothing that grows with T.
Shapes: n = 45 in the three one-wave shapes (an idle group in the last wave), n = 91 in the two-wave form (a ragged last workgroup), T = 12, G = 16, env_offset = 3:
member boundaries fall inside waves, the first member is partial and, at n = 91, the last one too.  Networks, seeds and start states are tests/test_minitaur_policy_rollout_gpu.py's (small gains, a
standing robot): at most 1 % of the rows outside a poisoned env sit in the failure guard, a condition on the inputs."""
import pytest

import population_abi as pa
from physics_abi import Snapshot, form
from test_minitaur_policy_rollout_gpu import policy
from test_physics_step_graph_gpu import make, same

pytestmark = pytest.mark.gpu

T12, OFF = 12, 3
FORMS = {'one_wave_packed': dict(solo_mt=0, minitaur_duo=0), 'one_wave_env_per_wave': dict(solo_mt=1, minitaur_duo=0),
         'one_wave_env_per_workgroup': dict(solo_mt=2, minitaur_duo=0), 'two_wave': dict(solo_mt=0, minitaur_duo=1)}
N_OF = {'one_wave_packed': 45, 'one_wave_env_per_wave': 45, 'one_wave_env_per_workgroup': 45, 'two_wave': 91}
_SNAPS = {}


def snapshot(n, gcf=0, seed=5):
  """the state of a freshly reset env of n envs at env_offset = 3, made once per shape and left unchanged"""
  key = (n, gcf, seed)
  if key not in _SNAPS:
    _SNAPS[key] = Snapshot('minitaur', make('minitaur', n, seed=seed, env_offset=OFF), gcf=gcf)
  return _SNAPS[key]


def pop_of(n, hidden, head, hidden_act='relu'):
  members = [policy(hidden, hidden_act, head=head, seed=100 + p)[0] for p in range((OFF + n - 1) // pa.G + 1)]
  return pa.population('minitaur', members)


CASES = [('one_wave_packed', (16,), None), ('one_wave_env_per_wave', (16,), 'sample'), ('one_wave_env_per_workgroup', (16,), None), ('two_wave', (16,), 'sample'),
         ('one_wave_packed', (48, 80), 'sample'), ('two_wave', (256, 256), None)]


@pytest.mark.parametrize('name,hidden,head', CASES, ids=[f'{c[0]}-{"x".join(map(str, c[1]))}-{c[2]}' for c in CASES])
def test_population_launch_equals_its_pieces_and_null_equals_the_policy_entry_point(name, hidden, head):
  n = N_OF[name]
  with form(**FORMS[name]):
    pa.population_equals_pieces(snapshot(n), T12, pop_of(n, hidden, head), head, name)


@pytest.mark.parametrize('head', [None, 'sample'])
def test_all_launch_forms_return_the_same_bits(head):
  n, res = 45, {}
  pop = pop_of(n, (16,), head, 'tanh')
  for name, sw in FORMS.items():
    with form(**sw):
      res[name], _ = pa.launch(snapshot(n), T12, 0x00, pop, head=head)
  with form():
    res['auto'], _ = pa.launch(snapshot(n), T12, 0xFF, pop, head=head)
  for name in res:
    pa.same_results(res['one_wave_packed'], res[name], name)
    assert set(res[name]) == set(res['one_wave_packed'])
  pa.check_summary(res['two_wave'], 'two_wave')
  pa.guard_ok(res['one_wave_packed'], 'forms')


@pytest.mark.parametrize('name', ['one_wave_packed', 'two_wave'])
def test_null_pointers_and_summary_with_an_env_in_the_failure_guard(name):
  """the poisoning of tests/test_minitaur_policy_rollout_gpu.py::test_failure_guard_repeats_the_row_and_the_action: a NaN velocity in one env's state rows"""
  n, bad = N_OF[name], 14
  base = snapshot(n)
  snap = Snapshot('minitaur', base.env, gcf=0)
  snap.state = {k: v.clone() for k, v in base.state.items()}
  snap.state['qvel'][bad, 7] = float('nan')
  with form(**FORMS[name]):
    full = pa.null_pointers(snap, T12, pop_of(n, (16,), 'sample'), 'sample', name, poisoned=bad)
  assert int(full['out.status'][:, bad].sum()) == T12 and float(full['sum.ret'][bad]) == 0.0 and int(full['sum.first'][bad]) == -1
  same(full['st.last_obs'][bad], snap.state['last_obs'][bad], 'the rolled-back env keeps its last stable observation')


def test_null_pointers_without_a_head_in_the_small_batch_forms():
  n = 45
  for name in ('one_wave_env_per_wave', 'one_wave_env_per_workgroup'):
    with form(**FORMS[name]):
      pa.null_pointers(snapshot(n), T12, pop_of(n, (16,), None), None, name)


@pytest.mark.parametrize('name', ['one_wave_packed', 'two_wave'])
def test_two_shards_equal_the_batch(name):
  n = N_OF[name]
  with form(**FORMS[name]):
    pa.shards_equal_batch(snapshot(n), T12, pop_of(n, (16,), 'sample'), 'sample', 19, name)


@pytest.mark.parametrize('name', ['one_wave_packed', 'two_wave'])
def test_goal_switch_inside_the_launch_with_the_carried_row(name):
  """goal_change_frequency = 5, the envs at different distances from their switch: with out->obs == NULL entries 30 / 31 of the env's row of last_obs are patched and
  the policy of the next step sees them -- the actions, the state and the summary are the full launch's, whose rows show the switches"""
  n, gcf = N_OF[name], 5
  snap = snapshot(n, gcf=gcf)
  pop = pop_of(n, (16,), None, 'tanh')
  with form(**FORMS[name]):
    full, _ = pa.launch(snap, T12, 0x00, pop)
    carried, _ = pa.launch(snap, T12, 0xFF, pop, null={'out.obs'})
    pieces = pa.concat([pa.launch(snap, T12, 0x00, pop.member(p), entry='policy', rows=(lo, hi))[0] for lo, hi, p in pa.member_pieces(OFF, n)])
  goal = full['out.obs'][:, :, 30:]
  switched = (goal[1:] != goal[:-1]).any(-1)
  assert int(switched.any(0).sum()) > n // 2, 'too few envs changed entries 30 / 31 inside the launch'
  assert 'out.obs' not in carried
  pa.same_results(carried, full, name + ' carried row', keys=[k for k in full if k != 'out.obs'])
  same(carried['st.last_obs'], full['out.obs'][-1], 'the carried row ends as the last emitted row')
  same(carried['st.last_obs'][:, 30:].contiguous(), full['st.goal'], 'entries 30 / 31 are the goal in force')
  pa.same_results(full, pieces, name + ' pieces under goal switching', keys=sorted(pieces))
  pa.guard_ok(full, name)


def test_evaluate_population_equals_the_definitions_and_allocates_nothing_that_grows_with_T():
  import torch
  n, T = 45, T12
  pop = pop_of(n, (16,), 'sample')
  ea, eb = make('minitaur', n, seed=5, env_offset=OFF), make('minitaur', n, seed=5, env_offset=OFF)
  out = ea.rollout_population(pop, T, return_noise=True)
  ev = eb.evaluate_population(pop, T, sample=True, reset_first=False)
  assert set(ev) == {'ret', 'success', 'first_success', 'guard_steps'} and all(tuple(v.shape) == (1, n) for v in ev.values())
  ret, last, first = pa.summary_by_definition(out['reward'], out['success'])
  same(ev['ret'][0], ret, 'ret')
  same(ev['success'][0].to(torch.uint8), last, 'success')
  same(ev['first_success'][0], first, 'first_success')
  same(ev['guard_steps'][0], (out['status'] != 0).sum(0).to(torch.int32), 'guard_steps')
  for k in ('qpos', 'qvel', 'goal_t', 'last_obs', 'fail_count', 'steps_since_reset', 'observed_torque', 'overheat', 'motor_enabled'):
    same(getattr(ea, k), getattr(eb, k), k)
  assert ea.total_step_count == eb.total_step_count == T
  assert float((out['status'] != 0).float().mean()) <= pa.MAX_GUARD_SHARE
  # a single policy (pop = NULL) and several episodes, each a reset plus one launch
  one = pop.member(0)
  ev2 = eb.evaluate_population(one, 5, episodes=2, sample=False)
  assert tuple(ev2['ret'].shape) == (2, n) and eb.total_step_count == T + 10
  # peak memory above the resident state: T and 2 T
  peaks = []
  for t in (T, 2 * T):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    eb.evaluate_population(pop, t, sample=True)
    torch.cuda.synchronize()
    peaks.append(torch.cuda.max_memory_allocated() - base)
  print('evaluate_population peak bytes above the resident state at T, 2 T:', peaks)
  assert peaks[0] == peaks[1], peaks

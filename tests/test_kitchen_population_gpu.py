"""earl_kitchen_population_rollout (include/earl_physics.h) on the device: a population of policies in ONE launch of the kitchen rollout kernel in each of its five
forms, per-env episode summaries, every [T] pointer optional.  Everything is compared bit for bit, through the C ABI with banded buffers (tests/population_abi.py):
  1. the population launch equals its pieces through earl_kitchen_policy_rollout;  2. pop = summary = NULL equals earl_kitchen_policy_rollout;
  3. the five launch forms return the same bits;  4. the summary equals its definitions, also for an env in the failure guard;
  5. every [T] pointer NULL, and each in turn;  6. two shards equal the batch;
  8. evaluate_population equals the definitions applied to rollout_population's arrays, and allocates nothing that grows with T.
Shapes: n = 37, T = 6, G = 16, env_offset = 3 (member boundaries inside waves, the last member partial), and one case with n = 1.  Networks, seeds and start states
are tests/test_kitchen_policy_rollout_gpu.py's (small gains, sensor noise on): at most 1 % of the rows outside a poisoned env sit in the failure guard, a condition
on the inputs."""
import pytest

import population_abi as pa
from physics_abi import Snapshot, form
from test_kitchen_policy_rollout_gpu import policy
from test_physics_step_graph_gpu import make, same

pytestmark = pytest.mark.gpu

N, T6, OFF = 37, 6, 3
SOLOS = (0, 1, 2, 3, 4)
_SNAPS = {}


def snapshot(n, seed=6):
  """the state of a freshly reset env of n envs at env_offset = 3, made once per shape and left unchanged"""
  if (n, seed) not in _SNAPS:
    env = make('kitchen', n, seed=seed, env_offset=OFF)
    assert env.sensor_noise
    _SNAPS[n, seed] = Snapshot('kitchen', env)
  return _SNAPS[n, seed]


def pop_of(n, hidden, head, hidden_act='relu'):
  members = [policy(hidden, hidden_act, head=head, seed=100 + p)[0] for p in range(max((OFF + n - 1) // pa.G + 1, 2))]
  return pa.population('kitchen', members)


CASES = [(0, (16,), None), (1, (16,), 'sample'), (2, (16,), None), (3, (16,), 'sample'), (4, (16,), None), (0, (48, 80), 'sample'), (4, (256, 256), None)]


@pytest.mark.parametrize('solo,hidden,head', CASES, ids=[f'solo{c[0]}-{"x".join(map(str, c[1]))}-{c[2]}' for c in CASES])
def test_population_launch_equals_its_pieces_and_null_equals_the_policy_entry_point(solo, hidden, head):
  with form(solo=solo):
    pa.population_equals_pieces(snapshot(N), T6, pop_of(N, hidden, head), head, f'solo={solo}')


@pytest.mark.parametrize('head', [None, 'sample'])
def test_all_launch_forms_return_the_same_bits(head):
  res = {}
  pop = pop_of(N, (16,), head, 'tanh')
  for solo in SOLOS + (-1,):
    with form(solo=solo):
      res[solo], _ = pa.launch(snapshot(N), T6, 0x00 if solo & 1 else 0xFF, pop, head=head)
  for solo in res:
    assert set(res[solo]) == set(res[0])
    pa.same_results(res[0], res[solo], f'solo={solo}')
  pa.check_summary(res[3], 'solo=3')
  pa.guard_ok(res[0], 'forms')
  assert float(res[0]['out.obs'][:, :, :9].std(0).mean()) > 0             # the arm moved


@pytest.mark.parametrize('solo', SOLOS)
def test_null_pointers_and_summary_with_an_env_in_the_failure_guard(solo):
  """the poisoning of tests/test_kitchen_policy_rollout_gpu.py::test_failure_guard_repeats_the_last_stable_row: an obs0 whose row 7 is NaN (last_obs finite), tanh
  hidden units: NaN actions at step 0, the step diverges, is rolled back, and step 1 acts on the last stable row"""
  bad = 7
  snap = snapshot(N)
  obs0 = snap.state['last_obs'].clone()
  obs0[bad] = float('nan')
  head = 'sample' if solo in (1, 3) else None
  with form(solo=solo):
    full = pa.null_pointers(snap, T6, pop_of(N, (16,), head, 'tanh'), head, f'solo={solo}', poisoned=bad, obs0=obs0)
  assert full['out.status'][:, bad].tolist() == [1] + [0] * (T6 - 1) and int(full['st.fail_count'][bad]) == 1
  same(full['out.obs'][0, bad], snap.state['last_obs'][bad], 'the rolled-back step repeats last_obs')


@pytest.mark.parametrize('solo', (0, 4))
def test_two_shards_equal_the_batch(solo):
  with form(solo=solo):
    pa.shards_equal_batch(snapshot(N), T6, pop_of(N, (16,), 'sample'), 'sample', 19, f'solo={solo}')


@pytest.mark.parametrize('solo', SOLOS + (-1,))
def test_one_env(solo):
  """n = 1 at global id 3: member 0, in every form (a wave with one live group, a workgroup of two envs with one)"""
  snap, pop = snapshot(1), pop_of(1, (16,), 'sample')
  with form(solo=solo):
    full, _ = pa.launch(snap, T6, 0x00, pop, head='sample')
    want, _ = pa.launch(snap, T6, 0xFF, pop.member(0), head='sample', entry='policy')
    bare, _ = pa.launch(snap, T6, 0xFF, pop, head='sample', null={'actions', 'eps'} | {'out.' + k for k in pa.T_OUT})
  pa.same_results(full, want, f'n = 1 solo={solo}', keys=sorted(want))
  pa.check_summary(full, f'n = 1 solo={solo}')
  pa.same_results(bare, full, f'n = 1 solo={solo} every [T] pointer NULL', keys=sorted(bare))
  pa.guard_ok(full, 'n = 1')


def test_evaluate_population_equals_the_definitions_and_allocates_nothing_that_grows_with_T():
  import torch
  n, T = N, T6
  pop = pop_of(n, (16,), 'sample')
  ea, eb = make('kitchen', n, seed=6, env_offset=OFF), make('kitchen', n, seed=6, env_offset=OFF)
  out = ea.rollout_population(pop, T, return_noise=True)
  ev = eb.evaluate_population(pop, T, sample=True, reset_first=False)
  assert set(ev) == {'ret', 'success', 'first_success', 'guard_steps'} and all(tuple(v.shape) == (1, n) for v in ev.values())
  ret, last, first = pa.summary_by_definition(out['reward'], out['success'])
  same(ev['ret'][0], ret, 'ret')
  same(ev['success'][0].to(torch.uint8), last, 'success')
  same(ev['first_success'][0], first, 'first_success')
  same(ev['guard_steps'][0], (out['status'] != 0).sum(0).to(torch.int32), 'guard_steps')
  for k in ('qpos', 'qvel', 'mocap_pos', 'last_qp_robot', 'last_obs', 'att', 'steps_since_reset', 'fail_count'):
    same(getattr(ea, k), getattr(eb, k), k)
  assert ea.total_step_count == eb.total_step_count == T and ea._counter == eb._counter      # the noise counter advanced by T in both
  assert float((out['status'] != 0).float().mean()) <= pa.MAX_GUARD_SHARE
  # a stale last_obs: one fresh reading, then T
  c0 = eb._counter
  eb.set_state(eb.qpos.clone(), eb.qvel.clone())
  eb.evaluate_population(pop.member(0), 3, sample=False, reset_first=False)
  assert eb._counter == c0 + 1 + 3
  ev2 = eb.evaluate_population(pop.member(0), 3, episodes=2, sample=False)
  assert tuple(ev2['ret'].shape) == (2, n)
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

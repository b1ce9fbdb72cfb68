"""The tabletop C ABI at its edges without a GPU: tests/tabletop_abi.py's driver against csrc/libearl_host.so (the `_cpu` twins of include/earl_tabletop.h), every
buffer inside guard bands in host memory, every case with bands of 0x00 and of 0xFF.  This proves the harness of tests/test_tabletop_abi_gpu.py where it can be
run by anyone, and gives the host twin -- the oracle of the closed-loop entry points there -- the same extent check: a reduced list, n in {1, 17, 65}.

  entry point (`_cpu`)                     extents          optional pointers      empty work
  step, tabletop3_step                     oracle           reward_f64, lifelong   n = 0
  rollout, tabletop3_rollout               oracle, T 1/9    obs reward done succ   n = 0, T = 0
  reset_rollout                            oracle, T 1/9    the same               n = 0, T = 0 (= the reset)
  eval_episodes (both stride forms)        oracle, (16, 2)  the same               n = 0, T = 0, episodes = 0
  reset, tabletop3_reset                   oracle           obs                    n = 0
  observe                                  oracle           obs reward done succ   n = 0
  reward, tabletop3_reward                 oracle           reward, success        n = 0
  valid_init                               oracle                                  n = 0
  policy_rollout, _gaussian                bands, fills     out, act_out, eps_out  n = 0
  population_rollout                       bands, fills     ... + summary rows     n = 0
  pair_rollout                             bands, fills     ... + agent, counters  n = 0
"""
import pytest

import tabletop_abi as ta
from test_tabletop_gpu import DENSE_ATOL, DENSE_RTOL

NS = (1, 17, 65)
DENSE = (DENSE_RTOL, DENSE_ATOL)


@pytest.fixture(scope='module')
def side():
  return ta.Side('cpu')


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('entry', ta.OPEN_ENTRIES)
def test_open_loop_extents_on_the_host(side, entry, rt):
  for n in NS:
    if 'rollout' in entry:
      for T in (1, 9):
        ta.check_open(side, ta.OpenCase(entry, n, rt, T=T), DENSE)
    elif entry == 'eval_episodes':
      for shared in (False, True):
        ta.check_open(side, ta.OpenCase(entry, n, rt, T=16, E=2, shared=shared), DENSE)
    else:
      ta.check_open(side, ta.OpenCase(entry, n, rt), DENSE)


@pytest.mark.parametrize('general', ['lifelong', 'auto_reset'])
@pytest.mark.parametrize('entry', ['step', 'rollout', 'reset_rollout', 'eval_episodes'])
def test_open_loop_extents_of_the_general_form_on_the_host(side, entry, general):
  for n in NS:
    ta.check_open(side, ta.OpenCase(entry, n, T=9, E=2, general=general), DENSE)


@pytest.mark.parametrize('E', [1, 2, 0], ids=['one_episode', 'two_episodes', 'continuing'])
@pytest.mark.parametrize('kind', ta.CLOSED_KINDS)
def test_closed_loop_extents_on_the_host(side, kind, E):
  for n in NS:
    for T, hidden, gaussian in ((1, (16,), False), (9, (32, 16), kind != 'policy')):
      for off in ((0, 5) if kind == 'population' else (2,)):
        ta.check_closed(side, ta.ClosedCase(kind, n, T, E, hidden=hidden, gaussian=gaussian, env_offset=off, seed=n))


@pytest.mark.parametrize('entry', [e for e in ta.OPEN_ENTRIES if e != 'valid_init'])
def test_open_loop_optional_pointers_on_the_host(side, entry):
  for n in NS:
    ta.check_optional_open(side, ta.OpenCase(entry, n, T=9, E=2), DENSE)


@pytest.mark.parametrize('kind', ta.CLOSED_KINDS)
def test_closed_loop_optional_pointers_on_the_host(side, kind):
  for n in NS:
    ta.check_optional_closed(side, ta.ClosedCase(kind, n, 9, 2, hidden=(16,), gaussian=kind != 'policy', env_offset=5, seed=n))


@pytest.mark.parametrize('entry', ta.OPEN_ENTRIES)
def test_open_loop_empty_work_on_the_host(side, entry):
  ta.check_empty_open(side, entry)


@pytest.mark.parametrize('kind', ta.CLOSED_KINDS)
def test_closed_loop_empty_work_on_the_host(side, kind):
  ta.check_empty_closed(side, kind)


def test_a_scene_copied_from_a_harness_state(side):
  """Scene.of: the state an env object holds after some use (tests/hip_harness.py), copied into bands; the rollout from it equals the oracle's"""
  import hip_harness as hx
  kw = dict(reward_type='sparse', horizon=12, seed=3, env_offset=4)
  h = hx.HipTabletop(17, device='cpu', **kw)
  h.reset()
  h.rollout(ta.actions(1, 5, 17, poison=False))
  case = ta.OpenCase('rollout', 17, T=9)
  case.sc = ta.Scene.of(h, **kw)
  assert case.sc.counter == 6 and int(case.sc.state['steps_since_reset'][0]) == 5
  ta.check_open(side, case, DENSE)

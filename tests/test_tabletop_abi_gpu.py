"""The tabletop C ABI at its edges on the device (include/earl_tabletop.h), driven directly through tests/tabletop_abi.py: every buffer inside guard bands that
must stay untouched, every case with bands of 0x00 and of 0xFF bytes that must not change a bit of the results, every output's interior pre-filled with a
pattern that must be gone afterwards, and the result equal to the reference.  References: the open-loop entry points against the oracle bit for bit (the dense
reward within DENSE_RTOL / DENSE_ATOL of tests/test_tabletop_gpu.py), the closed-loop ones against their `_cpu` twin bit for bit (the stated contract; sparse
reward), the 3-object ones against the oracle at nobj = 3.  C = the device's CU count (256 on an MI355X); every threshold shape is derived from it.

Entry points, each with at least one banded run (test, shapes):
  earl_tabletop_step / earl_tabletop3_step                 extents n 1..257; general form; reward_f64 / counter_base / lifelong arrays NULL; n = 0
  earl_tabletop_rollout                                    extents n x T {1, 7, 8, 9, 17}; general form; large grids T = 9; each output NULL; n = 0, T = 0
  earl_tabletop_reset_rollout                              the same; large grids T = 17
  earl_tabletop_eval_episodes                              extents (16, 2) (24, 3) (40, 3) (17, 2), both stride forms; large grids (24, 3) (40, 2); launch forms
                                                           0 / 1 / 36 / 38 x wgs_per_cu 1 / 2 at (40, 3); each output NULL; n = 0, T = 0, episodes = 0
  earl_tabletop_reset / earl_tabletop3_reset               extents with mask and next_goal_idx; obs NULL; n = 0
  earl_tabletop_observe                                    extents; each output NULL; n = 0
  earl_tabletop_reward / earl_tabletop3_reward             extents; each output NULL; n = 0
  earl_tabletop_valid_init                                 extents; n = 0
  earl_tabletop3_rollout                                   extents n x T
  earl_tabletop_policy_rollout, _policy_rollout_gaussian   extents n {1, 15, 16, 17, 33} x T {1, 9} x (E 1, E 2, continuing) x hidden (16) (32, 16); general form;
  earl_tabletop_population_rollout (env_offset 0 and 5)    every optional pointer NULL singly and together; n = 0
  earl_tabletop_pair_rollout

Branches of do_rollout's launch switch (csrc/tabletop.hip) that libearl_hip.so ships, each with at least one run against the oracle, sparse and dense:
  rollout_ws_kernel<RT, 3, 2, 8, 8, 3>           one episode, grid.x <= C            extents (n <= 257); large grids n = 64 C
  rollout_ws_kernel<RT, 3, 2, 8, 8, 2>           one episode, grid.x > C             large grids n = 64 C + 64, 64 C + 65 (rollout, reset_rollout)
  rollout_ws_kernel<.., 8, 16, 2, MULTI>         episodes, T >= 32, one group        launch forms n = 32 C + 64 and 64 C (forms 0, 38), 32 C (form 38); large grids
                                                                                     n = 64 C at (40, 2)
  rollout_ws_kernel<.., 8, 8, 3, MULTI>          episodes, grid.x <= C otherwise     extents (16, 2) (24, 3) (40, 3) (episode groups); launch forms: form 36, and
                                                                                     n = 32 C in two groups; large grids n = 64 C at (24, 3)
  rollout_ws_kernel<.., 8, 8, 2, MULTI>          episodes, grid.x > C                large grids n = 64 C + 64, 64 C + 65; launch forms at wgs_per_cu = 2: n = 32 C
                                                                                     (three groups) and 64 C (two groups)
  rollout_kernel<1, false> / <1, true>           form 1, a NULL output / general     extents, optional pointers, large grids (form 1)
  rollout_kernel<3, false>                       the 3-object env                    extents
  launch per episode                             T % 8 != 0 or T < 16, form 1        extents (17, 2); launch forms
  cases 11, 13, 20, 22 (other lane layouts)      tests/test_tabletop_gpu.py::test_rollout_kernels_agree (not banded)
"""
import pytest

import tabletop_abi as ta
from test_tabletop_gpu import DENSE_ATOL, DENSE_RTOL

pytestmark = pytest.mark.gpu

DENSE = (DENSE_RTOL, DENSE_ATOL)
NS = (1, 63, 64, 65, 66, 68, 255, 256, 257)      # 64: the wave-specialised workgroup; 256: the plain kernels' block; 65, 66: byte-wise flags; 68: n % 4 == 0 with a
                                                 # ragged last workgroup -- dword and byte flag stores in one launch
TS = (1, 7, 8, 9, 17)
EVAL = ((16, 2), (24, 3), (40, 3), (17, 2))      # (T, E); the last takes the launch-per-episode fallback
CLOSED_NS = (1, 15, 16, 17, 33)                  # a workgroup of the policy kernels is 16 envs


@pytest.fixture(scope='module')
def side():
  return ta.Side('cuda')


# ---------------------------------------------------------------------------------------------------- 1. extents, open loop
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('entry', ['step', 'reset', 'observe', 'reward', 'valid_init', 'step3', 'reset3', 'reward3'])
def test_open_loop_extents_of_the_one_row_entry_points(side, entry, rt):
  for n in NS:
    ta.check_open(side, ta.OpenCase(entry, n, rt), DENSE)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('entry', ['rollout', 'reset_rollout', 'rollout3'])
def test_open_loop_extents_of_the_rollouts(side, entry, rt):
  for n in NS:
    for T in TS:
      ta.check_open(side, ta.OpenCase(entry, n, rt, T=T), DENSE)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('shared', [False, True], ids=['own_actions', 'replayed_actions'])
def test_open_loop_extents_of_eval_episodes(side, shared, rt):
  for n in NS:
    for T, E in EVAL:
      ta.check_open(side, ta.OpenCase('eval_episodes', n, rt, T=T, E=E, shared=shared), DENSE)


@pytest.mark.parametrize('general', ['lifelong', 'auto_reset'])
@pytest.mark.parametrize('entry', ['step', 'rollout', 'reset_rollout', 'eval_episodes'])
def test_open_loop_extents_of_the_general_kernel(side, entry, general):
  for n in NS:
    for T in (1, 9):
      ta.check_open(side, ta.OpenCase(entry, n, T=T, E=2, general=general), DENSE)


# ---------------------------------------------------------------------------------------------------- 2. extents, closed loop
@pytest.mark.parametrize('hidden', [(16,), (32, 16)], ids=['h16', 'h32x16'])
@pytest.mark.parametrize('E', [1, 2, 0], ids=['one_episode', 'two_episodes', 'continuing'])
@pytest.mark.parametrize('kind', ta.CLOSED_KINDS)
def test_closed_loop_extents(side, kind, E, hidden):
  gaussian = kind != 'policy' and len(hidden) == 2         # (population and pair: the deterministic form with one hidden layer, the sampled one with two)
  for n in CLOSED_NS:
    for T in (1, 9):
      for off in ((0, 5) if kind == 'population' else (2,)):   # 5: the first workgroup has lanes below local index 0, and a piece boundary falls inside the shard
        ta.check_closed(side, ta.ClosedCase(kind, n, T, E, hidden=hidden, gaussian=gaussian, env_offset=off, seed=n + T))


@pytest.mark.parametrize('general', ['lifelong', 'auto_reset'])
@pytest.mark.parametrize('kind', ta.CLOSED_KINDS)
def test_closed_loop_extents_of_the_general_form(side, kind, general):
  if kind == 'pair' and general == 'lifelong':
    general = 'auto_reset'                                 # (a pair refuses goal_change_frequency > 0: it is the lifelong mechanism; this id repeats auto_reset)
  for n in CLOSED_NS:
    ta.check_closed(side, ta.ClosedCase(kind, n, 9, 0, hidden=(16,), gaussian=kind != 'policy', env_offset=5, general=general, seed=n))


# ---------------------------------------------------------------------------------------------------- 3. large grids
def large_case(entry, which, rt):
  n = ta.large_grid_sizes(ta.cus())[which]
  if entry == 'rollout':
    return ta.OpenCase('rollout', n, rt, T=9)
  if entry == 'reset_rollout':
    return ta.OpenCase('reset_rollout', n, rt, T=17)
  if entry == 'eval_24x3':
    return ta.OpenCase('eval_episodes', n, rt, T=24, E=3)
  return ta.OpenCase('eval_episodes', n, rt, T=40, E=2, shared=True)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('which', [0, 1, 2], ids=['64C', '64C+64', '64C+65'])
@pytest.mark.parametrize('entry', ['rollout', 'reset_rollout', 'eval_24x3', 'eval_40x2'])
def test_large_grids_against_the_oracle_and_the_plain_kernel(side, entry, which, rt):
  """n = 64 C is the last batch of the `grid.x <= cus` branch, 64 C + 64 and 64 C + 65 the first of the large-grid form (LEAD 2), whole and ragged"""
  case = large_case(entry, which, rt)
  assert case.n == (64 * ta.cus(), 64 * ta.cus() + 64, 64 * ta.cus() + 65)[which]
  got = ta.check_open(side, case, DENSE)
  with ta.form(impl=1):
    plain = ta.both_fills(case.run, side, what=case.what + ' form 1')
  ta.agree(got, plain, case.what + ': shipped form vs form 1')


# ---------------------------------------------------------------------------------------------------- 4. launch forms of eval_episodes
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('which', [0, 1, 2], ids=['32C', '32C+64', '64C'])
def test_launch_forms_of_eval_episodes_agree(side, which, rt):
  """forms 0 (shipped), 1 (plain kernel, a launch per episode), 36 (8-step chunks) and 38 (one episode group) at one and two workgroups per CU: 32 C is the last
  batch that splits into episode groups at one per CU, 32 C + 64 the first that does not, 64 C splits again at two per CU"""
  case = ta.OpenCase('eval_episodes', ta.episode_group_sizes(ta.cus())[which], rt, T=40, E=3)
  first = None
  for wgs in (1, 2):
    for impl in (0, 1, 36, 38):
      with ta.form(impl=impl, wgs_per_cu=wgs):
        res = ta.check_open(side, case, DENSE)
      if first is None:
        first = res
      else:
        ta.agree(res, first, f'{case.what}: form {impl} wgs_per_cu {wgs} vs form 0 wgs_per_cu 1')
  lib = ta._abi.load()
  assert lib.earl_debug_set_rollout_impl(0) == 0 and lib.earl_debug_set_rollout_wgs_per_cu(1) == 1      # the switches are back at their defaults


# ---------------------------------------------------------------------------------------------------- 5. optional pointers
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('entry', [e for e in ta.OPEN_ENTRIES if e != 'valid_init'])
def test_open_loop_optional_pointers(side, entry, rt):
  for n in (1, 65, 68, 257):
    for T, E in ((9, 2), (16, 2)):
      if (T, E) == (9, 2) or entry == 'eval_episodes':     # (eval_episodes: the fallback and the fused form, which a NULL output turns into the fallback)
        ta.check_optional_open(side, ta.OpenCase(entry, n, rt, T=T, E=E), DENSE)


@pytest.mark.parametrize('E', [2, 0], ids=['two_episodes', 'continuing'])
@pytest.mark.parametrize('kind', ta.CLOSED_KINDS)
def test_closed_loop_optional_pointers(side, kind, E):
  for n in (1, 17, 33):
    ta.check_optional_closed(side, ta.ClosedCase(kind, n, 9, E, hidden=(16,), gaussian=kind != 'policy', env_offset=5, seed=n))


# ---------------------------------------------------------------------------------------------------- 6. empty work
@pytest.mark.parametrize('entry', ta.OPEN_ENTRIES)
def test_open_loop_empty_work(side, entry):
  ta.check_empty_open(side, entry)


@pytest.mark.parametrize('kind', ta.CLOSED_KINDS)
def test_closed_loop_empty_work(side, kind):
  ta.check_empty_closed(side, kind)

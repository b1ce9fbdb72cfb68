"""The two MPPI update kernels (csrc/sawyer_plan.hip: sawyer_plan_update_kernel, csrc/minitaur_plan.hip: minitaur_plan_update_kernel) on the device, on returns that no
rollout produces.  The product reaches them only behind real rollouts, whose returns are finite, distinct and close together; here the probe of
tests/plan_update_probe.hip (the product units' own text, one launcher added) launches them on GIVEN arrays.

Every output is compared BIT FOR BIT (NaN payloads in ret0 aside) with items 4 - 7 in Python integers (tests/tabletop_plan_helpers.py: weights / update, update_fast
where K > 512) and with the host twin on the same arrays -- nothing the device returned is an expectation.  Every return column is checked ON THE ORACLE to be the case
its name says (tests/plan_update_cases.py: COLUMNS).  Outputs are sentinel-filled, a guard row stands after the plan; the guard row, the candidates, the returns and the
mean are unchanged afterwards.

What a shape (K, H) reaches in the kernel -- passes of `k += kUpdateThreads` (512 lanes: beta / best_k and the weights), passes of `k += 64` (a wave's lanes over the
candidates of a plan step), plan steps of wave 0 / of wave 7 under `t += kUpdateWaves`:
     K     H   lane passes   wave passes   steps of wave 0 / wave 7
     1     9        1             1              2 / 1          one lane holds a return; 511 lanes merge (-Inf, 0)
     2    19        1             1              3 / 2
    63     9        1             1 partial      2 / 1          one wave, its last lane idle
    64     9        1             1 full         2 / 1
    65     9        1             2              2 / 1          the second wave holds one return: the tie 63 / 64 crosses waves
   511     9        1 partial     8              2 / 1
   512     9        1 full        8              2 / 1
   513    19        2             9              3 / 2          the tie 511 / 512 crosses passes of one lane (lane 0 holds k = 0 and k = 512)
   513     1        2             9              1 / 0          waves 1 .. 7 take no step
  1100     8        3            18              1 / 1          every wave one step
  1100     9        3            18              2 / 1
  8192     9       16           128              2 / 1          EARL_*_PLAN_MAX_K: the weights fill the 32 KB of LDS
(tests/plan_update_cases.py: trip_counts restates the three loop headers; the table is asserted against it below.)"""
import numpy as np
import pytest

import plan_update_cases as pc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9), (2, 19), (63, 9), (64, 9), (65, 9), (511, 9), (512, 9), (513, 19), (513, 1), (1100, 8), (1100, 9), (8192, 9)]
TABLE = {(1, 9): (1, 1, 2, 1), (2, 19): (1, 1, 3, 2), (63, 9): (1, 1, 2, 1), (64, 9): (1, 1, 2, 1), (65, 9): (1, 2, 2, 1), (511, 9): (1, 8, 2, 1), (512, 9): (1, 8, 2, 1),
         (513, 19): (2, 9, 3, 2), (513, 1): (2, 9, 1, 0), (1100, 8): (3, 18, 1, 1), (1100, 9): (3, 18, 2, 1), (8192, 9): (16, 128, 2, 1)}
UNITS = ['sawyer', 'minitaur']


def run_groups(name, K, H, inv_t, in_place=False, null=(), names=None, sizes=(3,)):
  """every column K allows, `size` envs per launch: the oracle's checks, then device == oracle == twin"""
  unit = pc.UNITS[name]
  cols = pc.columns(K, inv_t, names)
  seen = []
  for size in sizes:
    for group, ret in pc.groups(cols, size):
      n = len(group)
      mean, act, m = pc.drawn(name, K, H, n)
      want, twin = pc.expected(unit, mean, act, m, ret, inv_t)
      pc.check_columns(group, ret, want, inv_t)
      what = f'({name}, K = {K}, H = {H}, n = {n}, 1/T = {inv_t}, {group})'
      pc.compare(twin, want, 'of the host twin against Python integers ' + what)
      got = pc.device_update(unit, mean, act, ret, inv_t, in_place=in_place, null=null)
      assert set(got) == {'plan', 'ret0', 'best_ret', 'best_k'} - set(null)
      pc.compare(got, want, 'against Python integers ' + what, keys=[k for k in ('plan', 'best_k', 'best_ret', 'ret0') if k not in null])
      assert bool((np.abs(got['plan']) <= 1).all())
      seen += group
      if K > 1 and 'distinct' in group:
        assert bool((want['plan'][:, group.index('distinct')] != m[:, group.index('distinct')]).any()), 'the update moved nothing'
  return seen


def test_the_shapes_reach_the_loop_trip_counts_the_docstring_states():
  assert set(TABLE) == set(SHAPES)
  for (K, H), (lp, wp, s0, s7) in TABLE.items():
    assert pc.trip_counts(K, H) == dict(lane_passes=lp, wave_passes=wp, steps_wave0=s0, steps_wave7=s7), (K, H)
  ks, hs = {k for k, _ in SHAPES}, {h for _, h in SHAPES}
  assert ks == {1, 2, 63, 64, 65, 511, 512, 513, 1100, 8192} and hs == {1, 8, 9, 19}
  assert all(any(h > 8 for k, h in SHAPES if k == K) for K in ks) and all(any(k > 512 for k, h in SHAPES if h == H) for H in hs)


@pytest.mark.parametrize('K,H', SHAPES)
@pytest.mark.parametrize('name', UNITS)
def test_update_kernel_on_crafted_returns(name, K, H):
  """every column, three envs per launch (n = 3, the remainder as it comes), and the first columns once more one env per launch (n = 1)"""
  seen = run_groups(name, K, H, 2.0)
  want = [c for c in pc.COLUMNS if not (K < 2 and c in ('tie 0 / K-1', 'NaN at the maximum', 'one weight', 'one ulp')) and not (K < 33 and c == 'tie 16 / 32') and not (K < 65 and c == 'tie 63 / 64')
          and not (K < 513 and c == 'tie 511 / 512')]
  assert seen == want, (seen, want)
  run_groups(name, K, H, 2.0, names=list(pc.COLUMNS)[:2], sizes=(1,))


@pytest.mark.parametrize('inv_t', [1e-6, 1e6])
@pytest.mark.parametrize('name', UNITS)
def test_inverse_temperature_at_both_ends(name, inv_t):
  """1e-6: every finite return keeps nearly the full weight; 1e6: only the ties for the maximum keep any"""
  for K, H in ((65, 9), (1100, 9)):
    run_groups(name, K, H, inv_t)
  unit = pc.UNITS[name]
  mean, act, m = pc.drawn(name, 65, 9, 1)
  ret = pc.columns(65, inv_t, ['distinct'])['distinct'][:, None]
  W = pc.expected(unit, mean, act, m, ret, inv_t)[0]['W'][:, 0]
  assert (W > pc.FULL - 64).all() if inv_t < 1 else (W != 0).sum() == 1


@pytest.mark.parametrize('name', UNITS)
def test_in_place_with_more_steps_than_two_rounds_of_waves(name):
  """plan == mean at H = 19: a wave reads row t of the mean before it writes row t of the plan, three rounds of the eight waves"""
  run_groups(name, 513, 19, 2.0, in_place=True)
  run_groups(name, 65, 9, 2.0, in_place=True)


@pytest.mark.parametrize('null', ['ret0', 'best_ret', 'best_k'])
@pytest.mark.parametrize('name', UNITS)
def test_each_optional_output_null_in_turn(name, null):
  run_groups(name, 65, 9, 2.0, null=(null,))


@pytest.mark.parametrize('name', UNITS)
def test_sums_at_their_stated_bound(name):
  """K = 8192, every return equal (W = 2^24 each), every candidate at the far end of the clip range from its mean: |D| = 2^21, so |A| = (K - 1) 2^24 2^21 = 2^58 less
  2^45 -- the int64 sums at the count the contract states, split over lanes whose partial sums pass 2^51.  Env 0: mean -1 (a NaN and a -3 among its words), candidates
  +1; env 1: mean +1, candidates -1; env 2: mean 0, candidates alternating.  ROW 0 OF THE CANDIDATES IS NOT THE MEAN here: branch 0 is the mean by item 5 (delta = 0)
  whatever the array holds, so the expectation is made with row 0 replaced by the clipped mean -- a kernel that adds row 0 as it stands differs"""
  unit = pc.UNITS[name]
  K, H, n, dim = 8192, 2, 3, unit.dim
  mean = np.zeros((H, n, dim), pc.F32)
  mean[:, 0], mean[:, 1] = -1.0, 1.0
  mean[0, 0, 0], mean[1, 0, 1], mean[0, 1, 2] = np.nan, -3.0, np.inf
  m = pc.sp.clip(mean)
  act = np.empty((K, H, n, dim), pc.F32)
  act[:, :, 0], act[:, :, 1] = 1.0, -1.0
  act[0::2, :, 2], act[1::2, :, 2] = 1.0, -1.0
  ret = np.full((K, n), -1.25)
  legit = act.copy()
  legit[0] = m
  want, twin = pc.expected(unit, mean, legit, m, ret, 2.0)
  assert (want['W'] == pc.FULL).all()
  D = np.rint((legit - m[None]).astype(np.float64) * 2.0**20).astype(np.int64)
  A = (want['W'][:, None, :, None] * D).sum(0)
  assert int(np.abs(A[:, :2]).min()) == (K - 1) * 2**24 * 2**21 and int(np.abs(A).max()) < 2**62
  assert (want['plan'][:, 0] == pc.F32(1 - 2.0 / K)).all() and (want['plan'][:, 1] == pc.F32(2.0 / K - 1)).all()
  pc.compare(twin, want, 'of the host twin')
  pc.compare(unit.helpers.host_update(pc._abi.load_host(), unit.cfg(n), unit.params(K, H, 2.0), pc.J, mean, act, ret), want, 'of the host twin with row 0 as it stands')
  got = pc.device_update(unit, mean, act, ret, 2.0)
  pc.compare(got, want, f'({name}: the sums at their bound)')

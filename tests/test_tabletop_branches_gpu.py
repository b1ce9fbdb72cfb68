"""earl_tabletop_branch_rollout / earl_tabletop3_branch_rollout (include/earl_tabletop.h) on the device: branch_kernel<NOBJ, GENERAL> of csrc/tabletop_branch.hip, one
lane per (branch, env), through tests/tabletop_branch_helpers.py -- every buffer inside guard bands, both fills, every output pre-filled with a pattern.

References and tolerances: the device library's own earl_tabletop[3]_rollout called K times on fresh copies of the state, reduced in numpy: every word bit-exact, both
rewards.  Device against host twin: sparse bit-exact; dense success_last / first_success / last_obs bit-exact and |d ret| <= 1e-6 * sum_t |r_t|.

The cases are those of tests/test_tabletop_branches.py (1 core, 2 general, 3 state / NULLs, 4 prediction through Python, 5 edges, 7 refusals) and
  6. large K         n = 64, K = 65,600 (beyond grid.y's 65,535), H = 1, no RNG in the step: against ONE earl_tabletop_rollout with T = 1 on 64 K envs whose state
                     rows tile the 64 rows, row by row
"""
import copy

import numpy as np
import pytest
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as h

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def side():
  return ta.Side('cuda')


@pytest.fixture(scope='module')
def host():
  return ta.Side('cpu')


# ---------------------------------------------------------------------------------------------------- 1-3
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_k_rollouts(side, host, nobj, rt):
  cs = h.case(nobj, rt)
  h.check_coverage(cs, h.reference(cs, side))
  full = h.check_case(side, cs)
  h.check_nulls(side, cs, full)
  h.check_device_vs_host(cs, full, h.check_case(host, cs))


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path_sees_the_draws_of_the_real_rollout(side, host, nobj, rt):
  cs = h.case(nobj, rt, general=True)
  h.check_general_coverage(cs, h.reference(cs, side))
  h.check_device_vs_host(cs, h.check_case(side, cs), h.check_case(host, cs))


def test_three_object_auto_reset_with_noise_draws(side):
  h.check_three_object_draws(side)


# ---------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('nobj', [1, 3])
@pytest.mark.parametrize('general', [False, True])
def test_edges_of_k_h_and_n(side, nobj, general):
  for kw in (dict(K=1), dict(H=1), dict(H=9), dict(n=1, K=2, H=9), dict(n=64, K=2, H=3), dict(n=65, K=2, H=3)):
    h.check_case(side, h.case(nobj, 'dense', general=general, **kw))


@pytest.mark.parametrize('nobj', [1, 3])
def test_stride_zero_replays_one_block(side, nobj):
  cs = h.case(nobj, 'dense', general=True)
  one = cs.act[2]
  ref = h.reference(cs, side, cs.sc, one[None], key=('stride 0', nobj))
  res = ta.both_fills(h.run_ok, side, cs.sc, one, what=cs.what + ' stride 0', K=3)
  h.state_untouched(res, cs.sc, cs.what)
  for k in h.OUTS:
    for j in range(3):
      ta.same(res['out.' + k][j].cpu(), ref['out.' + k][0], f'{cs.what} stride 0: row {j} of {k}')


@pytest.mark.parametrize('nobj', [1, 3])
def test_two_shards_equal_the_batch(side, nobj):
  cs = h.case(nobj, 'sparse', general=True, env_offset=0)
  whole = h.check_case(side, cs)
  for lo, hi in ((0, 33), (33, 70)):
    sc, act = h.shard(cs.sc, lo, hi), np.ascontiguousarray(cs.act[:, :, lo:hi])
    res = ta.both_fills(h.run_ok, side, sc, act, what=f'{cs.what} shard {lo}..{hi}')
    for k in h.OUTS:
      ta.same(res['out.' + k], whole['out.' + k][:, lo:hi].contiguous(), f'{cs.what} shard {lo}..{hi}: {k}')


# ---------------------------------------------------------------------------------------------------- 6
def test_more_branches_than_grid_y_holds(side):
  n, K = 64, 65600
  cs = h.case(1, 'sparse', n=n, K=1, H=1)
  assert not cs.sc.cfg().auto_reset and not cs.sc.cfg().goal_change_frequency            # no RNG in the step: the env id does not matter
  act = np.random.default_rng(6).uniform(-1, 1, (K, 1, n, 3)).astype(np.float32)
  act[..., 2] = np.abs(act[..., 2])
  big = copy.copy(cs.sc)
  big.n = n * K
  big.state = {k: np.tile(v, (K,) + (1,) * (v.ndim - 1)) for k, v in cs.sc.state.items()}
  big._cfg = cs.sc.cfg(n=n * K)
  ref, b = ta.run_rollout(side, big, act.reshape(1, n * K, 3), 0x00)
  b.check('the reference of large K')
  del b
  res, b = h.run_ok(side, cs.sc, act, 0xFF)
  b.check('large K')
  ta.assert_written(res, 'large K')
  h.state_untouched(res, cs.sc, 'large K')
  rew, succ = ref['out.reward'].reshape(K, n), ref['out.success'].reshape(K, n)
  assert bool(succ.any()) and not bool(succ.all()) and bool((rew[0] != rew[-1]).any())
  ta.same(res['out.ret'], rew.to(torch.float64), 'large K: ret')
  ta.same(res['out.success_last'], succ, 'large K: success_last')
  ta.same(res['out.first_success'], torch.where(succ != 0, 0, -1).to(torch.int32), 'large K: first_success')
  ta.same(res['out.last_obs'], ref['out.obs'].reshape(K, n, 12), 'large K: last_obs')


# ---------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  cs = h.case(nobj, 'sparse')
  h.check_refusals(side, cs)
  h.check_empty(side, cs)


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_branches_predict_the_next_rollout(nobj, general):
  dev = h.check_prediction(h.make_env(nobj, 'cuda', general=general))
  cpu = h.check_prediction(h.make_env(nobj, 'cpu', general=general))
  for k in dev:
    ta.same(dev[k], cpu[k], f'rollout_branches cuda vs cpu (sparse): {k}')

"""earl_tabletop_branch_rollout / earl_tabletop3_branch_rollout (include/earl_tabletop.h) without a GPU: the host twins of csrc/libearl_host.so -- branch_body
(csrc/tabletop_plan.h), the function the kernel runs -- through tests/tabletop_branch_helpers.py, the Python path on device='cpu', and the build of
csrc/tabletop_branch.hip.  The reference is the same library's earl_tabletop[3]_rollout_cpu called K times on fresh copies of the state and reduced in numpy;
every word is bit-exact, under both rewards.

  1. core case       n = 70 (a full tile and a ragged one), env_offset 3, K = 4, H = 12, horizon 50, both rewards, 1 and 3 objects; the coverage conditions
                     are asserted on the reference first
  2. general path    the same under horizon 7 + auto_reset (+ goal_change_frequency 3 with one object): done fires, goal_idx would change -- all branches must
                     see the draws of the real rollout (a wrong counter or env id shows here)
  3. state           after every call the state and every guard band are as before, under both fills; every output is overwritten; each of the four output
                     pointers NULL in turn
  4. prediction      env.rollout_branches(a)[k] == the summaries of the real env.rollout(a[k]) that follows, both env classes, under their wrappers
  5. edges           K = 1; H = 1; H = 9 (the prefetch's one-step second chunk); stride 0; n = 1, 64, 65; two shards == the batch, general
  7. refusals        every EARL_ERR_ARG of the header, buffers untouched; n = 0, K = 0, H = 0 return EARL_OK with buffers untouched
  8. build           csrc/tabletop_branch.hip: four kernels, no scratch, no LDS
(6, K = 65,600, needs the device: tests/test_tabletop_branches_gpu.py)
"""
import numpy as np
import pytest
import torch

import kernel_build
import tabletop_abi as ta
import tabletop_branch_helpers as h

CPU = 'cpu'


@pytest.fixture(scope='module')
def side():
  return ta.Side(CPU)


# ---------------------------------------------------------------------------------------------------- 1-3
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_k_rollouts(side, nobj, rt):
  cs = h.case(nobj, rt)
  h.check_coverage(cs, h.reference(cs, side))
  full = h.check_case(side, cs)
  h.check_nulls(side, cs, full)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path_sees_the_draws_of_the_real_rollout(side, nobj, rt):
  cs = h.case(nobj, rt, general=True)
  h.check_general_coverage(cs, h.reference(cs, side))
  h.check_case(side, cs)


def test_three_object_auto_reset_changes_the_results(side):
  """the coverage of the three-object auto-reset, from earl_tabletop3_rollout_cpu itself: with it the branches end elsewhere than without"""
  on = h.case(3, 'sparse', general=True)
  same_but_no_reset = h.with_cfg(on.sc, auto_reset=0)
  a, b = h.reference(on, side), h.reference(on, side, same_but_no_reset, on.act, key='3obj general without auto_reset')
  assert a['done'] and b['done']
  assert not torch.equal(a['out.last_obs'], b['out.last_obs']), 'auto_reset leaves the three-object rollout as it was'


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
      ta.same(res['out.' + k][j], ref['out.' + k][0], f'{cs.what} stride 0: row {j} of {k}')


@pytest.mark.parametrize('nobj', [1, 3])
def test_two_shards_equal_the_batch(side, nobj):
  cs = h.case(nobj, 'sparse', general=True, env_offset=0)
  whole = h.check_case(side, cs)
  for lo, hi in ((0, 33), (33, 70)):
    sc, act = h.shard(cs.sc, lo, hi), np.ascontiguousarray(cs.act[:, :, lo:hi])
    res = ta.both_fills(h.run_ok, side, sc, act, what=f'{cs.what} shard {lo}..{hi}')
    for k in h.OUTS:
      ta.same(res['out.' + k], whole['out.' + k][:, lo:hi].contiguous(), f'{cs.what} shard {lo}..{hi}: {k}')


def test_counter_high_word_changes_inside_a_branch():
  cs = h.case(1, 'sparse', general=True)
  c = cs.sc.counter
  assert c >> 32 == 0 and (c + cs.H - 1) >> 32 == 1


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
  env = h.make_env(nobj, CPU, general=general)
  h.check_prediction(env)


def test_python_arguments():
  env = h.make_env(1, CPU, n=5)
  u = env.unwrapped
  a = torch.zeros(2, 3, 5, 3)
  with pytest.raises(ValueError, match=r'\[K, H, N, 3\]'):
    env.rollout_branches(a[0])
  with pytest.raises(ValueError, match=r'\[K, H, N, 3\]'):
    env.rollout_branches(torch.zeros(2, 3, 4, 3))
  with pytest.raises(ValueError):
    env.rollout_branches(a, out={'reward': torch.empty(2, 5)})
  with pytest.raises(ValueError):
    env.rollout_branches(a, out={'ret': torch.empty(2, 5)})                       # float32
  with pytest.raises(ValueError):
    env.rollout_branches(a, out={'ret': None})
  with pytest.raises(ValueError):
    env.rollout_branches(a[:, :0])
  assert set(env.rollout_branches(a, last_obs=False)) == {'ret', 'success', 'first_success'}
  full = env.rollout_branches(a)
  ret = torch.full((2, 5), 7.0, dtype=torch.float64)
  before = h.snapshot(env)
  got = env.rollout_branches(a, out={'ret': ret, 'last_obs': None})
  assert set(got) == {'ret'} and got['ret'] is ret
  ta.same(ret, full['ret'], 'out={ret}')
  h.assert_env_as_found(env, before, 'out={ret}')
  assert u.total_step_count == before['total_step_count'] and int(u._cfg.counter) == before['rng_counter']


# ---------------------------------------------------------------------------------------------------- 8
def test_branch_kernels_use_no_scratch_and_no_lds():
  res = kernel_build.unit('tabletop_branch.hip').resources
  want = {f'branch_kernel<{nobj}, {g}>' for nobj in (1, 3) for g in ('true', 'false')}
  assert set(res) == want, set(res) ^ want
  for name, r in sorted(res.items()):
    print(name, r)
    assert r['scratch'] == 0 and r['lds'] == 0 and r['agpr'] == 0, (name, r)

"""earl_tabletop_plan_mppi / earl_tabletop3_plan_mppi / earl_tabletop_plan_candidates (include/earl_tabletop.h, "MPPI planning") without a GPU: the host twins of
csrc/libearl_host.so -- tabletop_plan.h's plan_* functions, the ones the kernels run -- through tests/tabletop_plan_helpers.py, the Python path on device='cpu',
and the build of csrc/tabletop_plan.hip.  The oracle (that module's docstring) uses none of the planner's code: a numpy Philox, the policy-math host build, the
library's EXISTING earl_tabletop[3]_branch_rollout_cpu for the returns, Python integers for the update.  Every output is bit-exact, under both rewards.

  0. the oracle's own arithmetic: the numpy Philox's known answers, fmaf32 against rationals
  1. core        n = 70 (a partial second wave), K = 5, H = 9 (crosses the eight-step unroll), I = 2, both envs, both rewards; the coverage conditions asserted on
                 the oracle first
  2. chaining    I = 3 in one call == three calls numbered 0, 1, 2; iterations 254, 255 accepted, 257 refused
  3. candidates  the entry point == the oracle's; branch 0 == the clipped mean; sigma = 0
  4. general     horizon 7 + auto-reset (+ a goal switch every 3 steps with one object)
  5. state and pointers   state, cfg and bands untouched under both fills, outputs overwritten; each optional pointer NULL in turn; plan aliasing mean; ret NULL refused
  6. edges       K = 1; H = 1; n = 1 / 64 / 65; two shards == the batch; noise_counter; non-finite input as the header states it
  7. Python      under the wrappers: the env as found, the plan scored by rollout_branches, `out=`
  8. refusals    every EARL_ERR_ARG of check_plan, and n == 0
  9. build       csrc/tabletop_plan.hip: six kernels, no scratch, the LDS DESIGN states
(K = 65536, device == twin and cuda == cpu need the device: tests/test_tabletop_plan_gpu.py)
"""
import numpy as np
import pytest

import kernel_build
import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_plan_helpers as h


@pytest.fixture(scope='module')
def side():
  return ta.Side('cpu')


# ---------------------------------------------------------------------------------------------------- 0
def test_the_oracles_philox_and_fmaf():
  kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
  for ctr, key, want in kat:
    assert tuple(int(w[0]) for w in h.philox4x32_10([np.array([c], np.uint64) for c in ctr], key)) == want
  rng = np.random.default_rng(0)
  a, b, c = (rng.uniform(-1, 1, 4000).astype(np.float32) for _ in range(3))
  b *= 5.5
  a[:8], b[:8], c[:8] = 0.5, np.float32(1 + 2**-23), np.float32(2**-25) * np.array([1, -1, 2, -2, 3, -3, 0, 1], np.float32)   # sums at and next to float32 half-way points
  # ... and sums 2^-64 off a half-way point, which float64 cannot hold: one rounding goes to the odd neighbour, two roundings tie to the even one
  a[8:12], b[8:12] = np.float32(2**-24 * (1 + 2**-20)), np.array([1, 1, -1, -1], np.float32) * np.float32(1 - 2**-20)
  c[8:12] = np.array([1 + 2**-23, 1, -1 - 2**-23, -1], np.float32)
  got = h.fmaf32(a, b, c)
  want = np.array([h.fmaf_exact(*v) for v in zip(a, b, c)], np.float32)
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
  naive = (a.astype(np.float64) * b + c).astype(np.float32)
  assert not np.array_equal(naive.view(np.uint32), want.view(np.uint32)), 'no element on which two roundings differ from one'


# ---------------------------------------------------------------------------------------------------- 1, 5
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_the_oracle(side, nobj, rt):
  cs = h.case(nobj, rt)
  h.check_coverage(cs, h.reference(cs, side))
  full = h.check_case(side, cs)
  h.check_pointers(side, cs, full)


# ---------------------------------------------------------------------------------------------------- 2, 3
@pytest.mark.parametrize('nobj', [1, 3])
def test_iterations_chain(side, nobj):
  h.check_chaining(side, h.case(nobj, 'dense'))


@pytest.mark.parametrize('nobj', [1, 3])
def test_candidates_entry_point(side, nobj):
  h.check_candidates(side, h.case(nobj, 'sparse'))


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path(side, nobj, rt):
  cs = h.case(nobj, rt, H=7, general=True)
  ref = h.reference(cs, side)
  tb.check_general_coverage(tb.case(nobj, rt, general=True), tb.reference(cs, side, cs.sc, ref['iters'][0]['act'], key=(id(cs), 'general')))
  h.check_case(side, cs)


# ---------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('nobj', [1, 3])
def test_edges(side, nobj):
  h.check_edges(side, nobj)
  h.check_shards(side, nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_non_finite_input(side, nobj):
  h.check_nonfinite(side, nobj)


# ---------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_plan_mppi(nobj, general):
  h.check_python(tb.make_env(nobj, 'cpu', general=general))


# ---------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  cs = h.case(nobj, 'sparse')
  h.check_refusals(side, cs)
  h.check_empty(side, cs)


# ---------------------------------------------------------------------------------------------------- 9
def test_build_of_the_plan_unit():
  kernel_build.need_hipcc()
  res = kernel_build.unit('tabletop_plan.hip').resources
  want = {f'plan_score_kernel<{nobj}, {g}>' for nobj in (1, 3) for g in ('true', 'false')} | {'plan_update_kernel', 'plan_candidates_kernel'}
  assert set(res) == want, set(res) ^ want
  for name, r in sorted(res.items()):
    print(name, r)
    assert r['scratch'] == 0 and r['agpr'] == 0, (name, r)
    assert r['lds'] == (22528 if name == 'plan_update_kernel' else 0), (name, r)        # [64][64] int32 weights + [8][64] (float64, int32) partial maxima

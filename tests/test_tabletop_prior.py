"""earl_tabletop[3]_plan_mppi_prior (include/earl_tabletop.h, "MPPI with policy-prior branches") on the host library -- csrc/tabletop_prior.h's functions, the ones the
kernels run -- through tests/tabletop_prior_helpers.py, the Python path on device='cpu', and the build of csrc/tabletop_prior.hip.  The oracle (that module's
docstring) uses none of the new code; every comparison is bit for bit.  No GPU is needed."""
import pytest

import kernel_build
import tabletop_abi as ta
import tabletop_plan_helpers as h
import tabletop_prior_helpers as p


@pytest.fixture(scope='module')
def side():
  return ta.Side('cpu')


@pytest.mark.parametrize('spec', p.CASES, ids=lambda s: '-'.join(map(str, s)))
def test_the_call_equals_the_oracle(side, spec):
  cs, prior, value = p.setup(*spec)
  ref = p.reference(cs, side, prior, value)
  if cs.general:
    p.check_trace(cs, ref)
  p.check_case(side, cs, prior, value)


def test_a_256_wide_policy(side):
  cs = h.case(1, 'sparse', n=3, K=3, H=2, I=1)
  p.check_case(side, cs, p.Prior(p.pnet(12, (256,), 'tanh', 'tanh'), 1))


@pytest.mark.parametrize('nobj', [1, 3])
def test_one_noiseless_prior_branch_is_the_closed_loop_rollout(nobj):
  p.check_closed_loop_identity('cpu', nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_no_prior_branches_is_the_planner(side, nobj):
  cs, prior, _ = p.setup(nobj, 'sparse', True, (16,), 'relu', 'none', False)
  p.check_identity(side, cs, prior)


def test_iterations_chain_and_shards_add_up(side):
  cs, prior, _ = p.setup(1, 'sparse', True, (32,), 'tanh', 'tanh', False)
  p.check_chaining(side, cs, prior)
  p.check_shards(side, cs, prior, p.check_case(side, cs, prior))


def test_optional_outputs_in_place_and_empty_work(side):
  cs, prior, _ = p.setup(3, 'sparse', False, (16,), 'relu', 'none', False)
  p.check_pointers(side, cs, prior, p.check_case(side, cs, prior))
  p.check_empty(side, cs, prior)


def test_non_finite_weights_mean_and_state(side):
  cs, prior, _ = p.setup(1, 'dense', False, (32,), 'tanh', 'tanh', False)
  p.check_nonfinite(side, cs, prior)
  p.check_nan_state(side, 1, prior)


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals(side, nobj):
  cs, prior, _ = p.setup(nobj, 'sparse', False, (16,), 'relu', 'none', False)
  p.check_refusals(side, cs, prior)


@pytest.mark.parametrize('nobj', [1, 3])
def test_the_prior_steers_where_the_noise_cannot(side, nobj):
  p.check_steering(side, nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_through_python(nobj):
  p.check_python('cpu', nobj)


def test_build_of_the_prior_unit():
  """the kernels of csrc/tabletop_prior.hip: no scratch, no AGPRs, no LDS in the score kernels, the update kernel's LDS no larger than plan_update_kernel's"""
  units = kernel_build.units(['tabletop_prior.hip', 'tabletop_plan.hip'])
  res = units['tabletop_prior.hip'].resources
  combos = [(nobj, g, val) for nobj in (1, 3) for g in ('true', 'false') for val in ('true', 'false')]
  want = {f'{k}<{nobj}, {g}, {val}>' for k in ('prior_noise_kernel', 'prior_score_kernel') for nobj, g, val in combos} | {'prior_update_kernel'}
  assert set(res) == want, sorted(set(res) ^ want)
  for k, r in sorted(res.items()):
    print(k, r)
    assert r['scratch'] == 0 and r['agpr'] == 0, (k, r)
    if k == 'prior_update_kernel':
      assert 0 < r['lds'] <= units['tabletop_plan.hip'].resources['plan_update_kernel']['lds'], (k, r)
    else:
      assert r['lds'] == 0, (k, r)

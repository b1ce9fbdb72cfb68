"""earl_tabletop_plan_cem / earl_tabletop3_plan_cem / earl_tabletop_cem_candidates (include/earl_tabletop.h, "CEM planning") without a GPU: the host twins of
csrc/libearl_host.so -- tabletop_cem.h's functions, the ones the kernels run -- through tests/tabletop_cem_helpers.py, the Python path on device='cpu', and the
build of csrc/tabletop_cem.hip and csrc/tabletop_cem_mpc.hip.  The oracle (that module's docstring) uses none of the new code; every output is bit-exact, under
both rewards.

  1. core        n = 70 (a 6-lane tail tile), K = 5, H = 9 (two update step-groups), I = 2, E = 2, alpha = 0.25, std in [0.05, 0.6], std0 given; both envs, both
                 rewards; the coverage conditions asserted on the oracle first; the optional pointers NULL in every combination; plan == mean and std == std0;
                 pv = {1.0, NULL} == pv NULL; with pv: a tanh value net D -> 16 -> 1 and discount 0.9
  3. E edges     E = 1 (std' = std_min), E = K, E = K with alpha = 0
  4. K mapping   n = 3, H = 2, E = 8, sigma 2.0: K in 1, 2, 63, 64, 65, 1024
  5. chaining, shards, iteration0 / noise_counter, word 0 against MPPI's
  6. general     auto-reset (+ lifelong goal switches with one object) inside the look-ahead, H = 7
  7. non-finite  NaN / +-Inf in mean and std0; some returns NaN (Ne < E); a NaN state under the dense reward (Ne = 0)
  8. cem_candidates
 10. Python      plan_cem / cem_candidates on device='cpu'
 11. refusals and empty work
 12. build       the two new units: their kernels, no scratch, the static LDS
(the fused loop: tests/test_tabletop_cem_mpc.py; the device: tests/test_tabletop_cem_gpu.py)
"""
import pytest

import kernel_build
import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_cem_helpers as c


@pytest.fixture(scope='module')
def side():
  return ta.Side('cpu')


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_the_oracle(side, nobj, rt):
  cs = c.case(nobj, rt)
  c.check_coverage(cs, c.reference(cs, side))
  full = c.check_case(side, cs)
  c.check_pointers(side, cs, full)
  c.check_value_identity(side, cs)
  c.check_value(side, cs)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_elite_count_edges(side, nobj, rt):
  c.check_e_edges(side, nobj, rt)


@pytest.mark.parametrize('K', [1, 2, 63, 64, 65, 1024])
@pytest.mark.parametrize('nobj', [1, 3])
def test_branch_count_mapping(side, nobj, K):
  c.check_k_mapping(side, nobj, K)


@pytest.mark.parametrize('nobj', [1, 3])
def test_chaining_shards_and_noise_words(side, nobj):
  c.check_chaining(side, c.case(nobj, 'dense'))
  c.check_shards(side, c.case(nobj, 'sparse', H=7, general=True))
  c.check_noise_words(side, c.case(nobj, 'sparse'))


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path(side, nobj, rt):
  cs = c.case(nobj, rt, H=7, general=True)
  ref = c.reference(cs, side)
  tb.check_general_coverage(tb.case(nobj, rt, general=True), tb.reference(cs, side, cs.sc, ref['iters'][0]['act'], key=(id(cs), 'cem general')))
  c.check_case(side, cs)


@pytest.mark.parametrize('nobj', [1, 3])
def test_non_finite_input(side, nobj):
  c.check_nonfinite(side, nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_candidates_entry_point(side, nobj):
  c.check_candidates(side, c.case(nobj, 'sparse'))


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_plan_cem(nobj, general):
  c.check_python_plan(tb.make_env(nobj, 'cpu', general=general))


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  cs = c.case(nobj, 'sparse')
  c.check_refusals(side, cs)
  c.check_empty(side, cs)


def test_build_of_the_cem_units():
  kernel_build.need_hipcc()
  units = kernel_build.units(['tabletop_cem.hip', 'tabletop_cem_mpc.hip'])
  combos = [(nobj, g) for nobj in (1, 3) for g in ('true', 'false')]
  want = {'tabletop_cem.hip': {f'cem_score_kernel<{nobj}, {g}, {v}>' for nobj, g in combos for v in ('true', 'false')} | {'cem_update_kernel', 'cem_candidates_kernel'},
          'tabletop_cem_mpc.hip': {f'cem_mpc_kernel<{nobj}, {g}>' for nobj, g in combos}}
  for name, unit in units.items():
    res = unit.resources
    assert set(res) == want[name], set(res) ^ want[name]
    for kernel, r in sorted(res.items()):
      print(name, kernel, r)
      assert r['scratch'] == 0 and r['agpr'] == 0, (kernel, r)
      assert r['lds'] == (14336 if kernel == 'cem_update_kernel' else 0), (kernel, r)    # [32][64] elite mask words + [8][64] (float64, int32) partial maxima

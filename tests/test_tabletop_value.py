"""earl_tabletop[3]_plan_mppi_value / earl_tabletop[3]_mpc_rollout_value (include/earl_tabletop.h, "discounted MPPI with a terminal value") without a GPU: the host
twins of csrc/libearl_host.so -- the kernels' per-lane functions of csrc/tabletop_value.h -- through tests/tabletop_value_helpers.py, the Python path on
device='cpu', and the build of csrc/tabletop_plan_value.hip and csrc/tabletop_mpc_value.hip.  The oracles (that module's docstring) use none of the new code: the
library's existing rollouts, a numpy float64 discounted sum, earl_mlp_policy_forward_cpu and the Python-integer update; every output is bit-exact, both rewards.

  1. core        n = 70, K = 5, H = 9, I = 2 (MPC: T = 6), both envs, both rewards, gamma = 0.9, V = D -> 16 -> 16 -> 1 tanh / none; coverage asserted on the oracle
  2. identity    gamma = 1 without a network and with an all-zero one == earl_tabletop[3]_plan_mppi / _mpc_rollout
  3. shapes      one hidden layer of 16, 48, 256; two of (16, 16), (EARL_PLAN_VALUE_MAX_H1, 80), (EARL_PLAN_VALUE_MAX_H1, 256); relu / tanh, none / tanh; K = 5, H = 3.
                 The issue's (48, 80) needs a first hidden layer of 48 in registers: EARL_PLAN_VALUE_MAX_H1 had to be lowered to 16 (include/earl_tabletop.h), so that
                 shape is REFUSED (case 8) and (16, 80) stands in for the unroll edge of the streamed second layer
  4. steering    sparse reward, nothing reachable within H = 2: the value-free planner is blind, V = -L1 distance to the goal turns every far env's plan towards it
  5. general     horizon 7, auto-reset, a goal switch every 3 steps, T = 9: the discount runs across the reset, V reads the re-read / terminal row
  6. chaining    I = 3 == three calls; T = 4 then 5 == 9; two shards == the batch; n = 1, 64, 65; K = 1; H = 1
  7. non-finite  a NaN bias, a +Inf last-layer bias, a NaN in one env's state
  8. refusals    every EARL_ERR_ARG leaves every buffer as it was; the widths that bracket EARL_PLAN_VALUE_MAX_H1; n = 0 / T = 0 write nothing; optional pointers
  9. Python      plan_mppi / rollout_mpc with discount / value == the ABI route; the defaults == the calls without the keywords; bad networks refused
  11. build      every new instantiation exists, none has scratch, the MPC ones hold at most 128 VGPRs, LDS as the value-free kernels'
(10, device == twin, graphs and the sixteen-wave launch need the device: tests/test_tabletop_value_gpu.py)
"""
import pytest

import kernel_build
import tabletop_abi as ta
import tabletop_plan_helpers as h
import tabletop_value_helpers as v


@pytest.fixture(scope='module')
def side():
  return ta.Side('cpu')


def core_net(cs):
  return v.net(cs.sc.obs_dim, (16, 16), 'tanh', 'none', seed=1)


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_the_oracle(side, nobj, rt):
  cs = h.case(nobj, rt)
  vnet = core_net(cs)
  v.check_candidates_entry(side, cs)
  v.check_coverage(side, cs, vnet, v.reference(side, cs, vnet))
  full = v.check_case(side, cs, vnet)
  v.check_pointers(side, cs, vnet, full)
  loop = v.check_mpc_case(side, cs, 6, vnet)
  v.check_mpc_pointers(side, cs, 6, vnet, loop)


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_unit_discount_without_a_value_is_the_value_free_call(side, nobj, rt):
  v.check_identity(side, h.case(nobj, rt))


# ---------------------------------------------------------------------------------------------------- 3
SHAPES = [((16,), 'relu', 'none'), ((48,), 'tanh', 'tanh'), ((256,), 'relu', 'tanh'), ((16, 16), 'relu', 'tanh'), ((v.MAX_H1, 80), 'tanh', 'none'),
          ((v.MAX_H1, 256), 'relu', 'none')]


@pytest.mark.parametrize('hidden,hact,oact', SHAPES)
@pytest.mark.parametrize('nobj', [1, 3])
def test_network_shapes(side, nobj, hidden, hact, oact):
  cs = h.case(nobj, 'dense', H=3)
  vnet = v.net(cs.sc.obs_dim, hidden, hact, oact, seed=2)
  v.check_case(side, cs, vnet)
  v.check_mpc_case(side, cs, 2, vnet)


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('nobj', [1, 3])
def test_the_value_steers_a_blind_planner(side, nobj):
  v.check_steering(side, nobj)


# ---------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path(side, nobj, rt):
  cs = h.case(nobj, rt, H=7, general=True)
  vnet = core_net(cs)
  v.check_case(side, cs, vnet)
  v.check_mpc_general_coverage(v.mpc_reference(side, cs, 9, vnet))
  v.check_mpc_case(side, cs, 9, vnet)


# ---------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('nobj', [1, 3])
def test_calls_chain_and_shards_equal_the_batch(side, nobj):
  cs = h.case(nobj, 'dense', H=7, general=True)
  vnet = core_net(cs)
  v.check_chaining(side, cs, vnet)
  v.check_mpc_chaining(side, cs, vnet)
  v.check_shards(side, h.case(nobj, 'sparse', general=True), vnet)


@pytest.mark.parametrize('nobj', [1, 3])
def test_edges_of_the_shapes(side, nobj):
  base = h.case(nobj, 'sparse')
  vnet = core_net(base)
  for n in (1, 64, 65):
    cs = h.case(nobj, 'sparse', n=n, K=3, H=2, I=1)
    v.check_case(side, cs, vnet)
    v.check_mpc_case(side, cs, 2, vnet)
  v.check_case(side, base, vnet, key=('K=1', nobj), K=1)
  v.check_mpc_case(side, base, 2, vnet, key=('K=1 mpc', nobj), K=1)
  one = h.case(nobj, 'sparse', H=1)
  v.check_case(side, one, vnet)
  v.check_mpc_case(side, one, 3, vnet)


# ---------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('nobj', [1, 3])
def test_non_finite_values(side, nobj):
  v.check_nonfinite(side, nobj)


# ---------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  v.check_refusals(side, h.case(nobj, 'sparse'))


# ---------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_keywords(nobj):
  v.check_python('cpu', nobj)


# ---------------------------------------------------------------------------------------------------- 11
def test_build_of_the_value_units():
  """resource counts only (the compiler's remarks)"""
  kernel_build.need_hipcc()
  built = kernel_build.units(['tabletop_plan.hip', 'tabletop_mpc.hip', 'tabletop_plan_value.hip', 'tabletop_mpc_value.hip'])
  for unit, kernel, free in (('tabletop_plan_value.hip', 'plan_score_kernel', 'tabletop_plan.hip'), ('tabletop_mpc_value.hip', 'mpc_kernel', 'tabletop_mpc.hip')):
    res, was = built[unit].resources, built[free].resources
    want = {f'value::{kernel}<{nobj}, {g}>' for nobj in (1, 3) for g in ('true', 'false')}
    assert set(res) == want, set(res) ^ want
    for name, r in sorted(res.items()):
      print(name, r)
      assert r['scratch'] == 0 and r['agpr'] == 0, (name, r)
      assert r['lds'] == was[name[len('value::'):]]['lds'], (name, r)
      if kernel == 'mpc_kernel':
        assert r['vgpr'] <= 128, (name, r)                  # sixteen waves of one workgroup on a CU: 512 / 4 registers per lane

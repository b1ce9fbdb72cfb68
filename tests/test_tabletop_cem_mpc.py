"""earl_tabletop_mpc_rollout_cem / earl_tabletop3_mpc_rollout_cem (include/earl_tabletop.h, "CEM planning") without a GPU: the host twins against the COMPOSED
route the header defines the call by -- per real step earl_tabletop[3]_plan_cem_cpu with std0 = NULL, the one-step rollout, the shift in numpy
(tests/tabletop_cem_helpers.py) -- bit for bit in every output, the final plan and the final state, under both rewards.

  9. core        n = 70, K = 5, H = 9, I = 2, E = 2, T = 6; each optional pointer NULL in turn
     shapes      T in 1, 6; H in 1, 2; n in 1, 70
     general     auto-reset inside the launch: the plan of a reset env is zeroed
     chaining    T1 + T2 == T1, then T2; two shards == the batch
     K mapping   K in 1, 2, 63, 64, 65, 1024
     value       pv != NULL is the documented refusal (the header: the kernel with the value network inside does not fit without scratch)
 10. Python      rollout_mpc(method='cem') == the loop on plan_cem and rollout; rollout_mpc() without a new keyword == the loop on plan_mppi and rollout
 11. refusals and empty work
"""
import pytest

import tabletop_abi as ta
import tabletop_cem_helpers as c


@pytest.fixture(scope='module')
def side():
  return ta.Side('cpu')


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_fused_loop_equals_the_composed_calls(side, nobj, rt):
  cs = c.case(nobj, rt, std0=False)
  c.check_mpc_coverage(cs, c.mpc_reference(side, cs, 6))
  full = c.check_mpc_case(side, cs, 6)
  c.check_mpc_pointers(side, cs, 6, full)


@pytest.mark.parametrize('nobj', [1, 3])
def test_shapes(side, nobj):
  for H in (1, 2):
    for n in (1, 70):
      for T in (1, 6):
        c.check_mpc_case(side, c.case(nobj, 'sparse', n=n, K=5, H=H, I=2, E=2, std0=False), T)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path_zeroes_the_plan_of_a_reset_env(side, nobj, rt):
  cs = c.case(nobj, rt, H=7, general=True, std0=False)
  c.check_mpc_coverage(cs, c.mpc_reference(side, cs, 6), general=True)
  c.check_mpc_case(side, cs, 6)


@pytest.mark.parametrize('nobj', [1, 3])
def test_chaining_and_shards(side, nobj):
  c.check_mpc_chaining(side, c.case(nobj, 'dense', std0=False))
  c.check_mpc_shards(side, c.case(nobj, 'sparse', H=7, general=True, std0=False), 4)


@pytest.mark.parametrize('K', [1, 2, 63, 64, 65, 1024])
@pytest.mark.parametrize('nobj', [1, 3])
def test_branch_count_mapping(side, nobj, K):
  c.check_k_mapping(side, nobj, K, mpc_T=2)


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_rollout_mpc_methods(nobj, general):
  c.check_python_mpc('cpu', nobj, general)


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  c.check_mpc_refusals(side, c.case(nobj, 'sparse', std0=False))

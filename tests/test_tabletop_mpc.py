"""earl_tabletop_mpc_rollout / earl_tabletop3_mpc_rollout (include/earl_tabletop.h, "receding-horizon MPPI control") without a GPU: the host twins of
csrc/libearl_host.so -- the kernel's per-lane functions (csrc/tabletop_mpc.h) -- through tests/tabletop_mpc_helpers.py, the Python path on device='cpu', and the build
of csrc/tabletop_mpc.hip.  The reference (that module's docstring) is the COMPOSED route through the library's existing plan_mppi and one-step rollout with the shift
in numpy; every output, the final plan and the final state are bit-exact, under both rewards.

  1. core        n = 70, K = 5, H = 9, I = 2, T = 6, both envs, both rewards; the coverage conditions asserted on the reference first; both fills; each optional
                 pointer NULL in turn
  2. general     horizon 7 + auto-reset (+ a goal switch every 3 steps with one object), T = 9: every env resets inside the launch and inside look-aheads
  3. K           1, 63, 64, 65, 130: the edges of the device's lane mapping (one wave, a full wave, two and three waves with idle lanes)
  4. H, T, n     H = 1, 2; H = 40 and 70 at K = 3 (the device's update walks the rows in one group, and in two passes); T = 1; n = 1, 65
  5. chaining    T = 4 then T = 5 == T = 9, the noise counter wrapping past 2^32 on the way
  6. shards      0..40 and 40..70 with env_offset == the batch
  7. sigma = 0; a NaN in one env's state under the dense reward
  8. refusals    every EARL_ERR_ARG of check_mpc leaves every buffer as it was; n == 0 and T == 0 write nothing
  9. Python      rollout_mpc == the hand-written loop on a second env; counters; `out=`
  10. build      csrc/tabletop_mpc.hip: four kernels, no scratch
(device == twin and cuda == cpu need the device: tests/test_tabletop_mpc_gpu.py)
"""
import pytest

import kernel_build
import tabletop_abi as ta
import tabletop_mpc_helpers as m
import tabletop_plan_helpers as h


@pytest.fixture(scope='module')
def side():
  return ta.Side('cpu')


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_the_composed_calls(side, nobj, rt):
  cs = h.case(nobj, rt)
  m.check_coverage(cs, m.reference(side, cs, 6))
  full = m.check_case(side, cs, 6)
  m.check_pointers(side, cs, 6, full)


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path(side, nobj, rt):
  cs = h.case(nobj, rt, H=7, general=True)
  m.check_coverage(cs, m.reference(side, cs, 9), general=True)
  m.check_case(side, cs, 9)


# ---------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('K', [1, 63, 64, 65, 130])
def test_branch_counts_across_the_lane_mapping(side, K):
  m.check_case(side, h.case(1, 'sparse', K=K, H=4), 3)


def test_three_waves_of_the_widest_kernel(side):
  m.check_case(side, h.case(3, 'dense', K=130, H=4, general=True), 3)


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('H,K', [(1, 5), (2, 5), (40, 3), (70, 3)])
def test_plan_lengths(side, H, K):
  m.check_case(side, h.case(1, 'dense', n=9 if H > 2 else 70, K=K, H=H, I=1 if H > 2 else 2), 3)


@pytest.mark.parametrize('nobj', [1, 3])
def test_one_step(side, nobj):
  m.check_case(side, h.case(nobj, 'sparse'), 1)


@pytest.mark.parametrize('n', [1, 65])
def test_batch_sizes(side, n):
  m.check_case(side, h.case(1, 'sparse', n=n, K=3, H=2, I=1), 3)


# ---------------------------------------------------------------------------------------------------- 5, 6
@pytest.mark.parametrize('nobj', [1, 3])
def test_calls_chain(side, nobj):
  m.check_chaining(side, h.case(nobj, 'dense', H=7, general=True), nc=0xFFFFFFFA)


@pytest.mark.parametrize('nobj', [1, 3])
def test_shards_equal_the_batch(side, nobj):
  m.check_shards(side, h.case(nobj, 'sparse', H=7, general=True), 9)


# ---------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('nobj', [1, 3])
def test_without_noise_and_with_a_nan_state(side, nobj):
  m.check_sigma_zero(side, h.case(nobj, 'sparse'), 4)
  m.check_nan_state(side, nobj)


# ---------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  cs = h.case(nobj, 'sparse')
  m.check_refusals(side, cs)
  m.check_empty(side, cs)


# ---------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_rollout_mpc(nobj, general):
  m.check_python('cpu', nobj, general=general)


# ---------------------------------------------------------------------------------------------------- 10
def test_build_of_the_mpc_unit():
  kernel_build.need_hipcc()
  res = kernel_build.unit('tabletop_mpc.hip').resources
  want = {f'mpc_kernel<{nobj}, {g}>' for nobj in (1, 3) for g in ('true', 'false')}
  assert set(res) == want, set(res) ^ want
  for name, r in sorted(res.items()):
    print(name, r)
    assert r['scratch'] == 0 and r['agpr'] == 0, (name, r)
    assert r['vgpr'] <= 128, (name, r)                    # sixteen waves of one workgroup on a CU: 512 / 4 registers per lane
    assert r['lds'] == 0, (name, r)                       # all of it dynamic: 36 H + 4 K + 200 bytes and the env (csrc/tabletop_mpc.hip)

"""earl_tabletop_mpc_rollout / earl_tabletop3_mpc_rollout (include/earl_tabletop.h, "receding-horizon MPPI control") on the device: mpc_kernel<NOBJ, GENERAL> of
csrc/tabletop_mpc.hip through tests/tabletop_mpc_helpers.py -- every buffer inside guard bands, both fills, every output pre-filled with a pattern.

The reference (that module's docstring) is the COMPOSED route through the device's own existing plan_mppi and one-step rollout: every output, the final plan and
the final state bit-exact, both rewards.  Device against host twin: bit-exact under the sparse reward, not compared under the dense one.

The cases are those of tests/test_tabletop_mpc.py (1 core, 2 general, 3 K, 4 H / T / n, 5 chaining, 6 shards, 7 sigma = 0 / NaN, 8 refusals, 9 Python) and
  1'. the fused call on the device == the fused call of the twin (sparse), core and general
  9'. rollout_mpc on 'cuda' == on 'cpu' (sparse)
  9''. the call captured into a HIP graph (no host synchronisation, no allocation inside it) replays to the eager call's bits
"""
import pytest
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_mpc_helpers as m
import tabletop_plan_helpers as h

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def side():
  return ta.Side('cuda')


@pytest.fixture(scope='module')
def host():
  return ta.Side('cpu')


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_the_composed_calls(side, host, nobj, rt):
  cs = h.case(nobj, rt)
  m.check_coverage(cs, m.reference(side, cs, 6))
  full = m.check_case(side, cs, 6)
  m.check_pointers(side, cs, 6, full)
  if rt == 'sparse':
    m.check_device_vs_host(cs, 6, side, host)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path(side, host, nobj, rt):
  cs = h.case(nobj, rt, H=7, general=True)
  m.check_coverage(cs, m.reference(side, cs, 9), general=True)
  m.check_case(side, cs, 9)
  if rt == 'sparse':
    m.check_device_vs_host(cs, 9, side, host)


@pytest.mark.parametrize('K', [1, 63, 64, 65, 130])
def test_branch_counts_across_the_lane_mapping(side, K):
  m.check_case(side, h.case(1, 'sparse', K=K, H=4), 3)


def test_three_waves_of_the_widest_kernel(side):
  m.check_case(side, h.case(3, 'dense', K=130, H=4, general=True), 3)


@pytest.mark.parametrize('H,K', [(1, 5), (2, 5), (40, 3), (70, 3)])
def test_plan_lengths(side, H, K):
  m.check_case(side, h.case(1, 'dense', n=9 if H > 2 else 70, K=K, H=H, I=1 if H > 2 else 2), 3)


@pytest.mark.parametrize('nobj', [1, 3])
def test_one_step(side, nobj):
  m.check_case(side, h.case(nobj, 'sparse'), 1)


@pytest.mark.parametrize('n', [1, 65])
def test_batch_sizes(side, n):
  m.check_case(side, h.case(1, 'sparse', n=n, K=3, H=2, I=1), 3)


@pytest.mark.parametrize('nobj', [1, 3])
def test_calls_chain(side, nobj):
  m.check_chaining(side, h.case(nobj, 'dense', H=7, general=True), nc=0xFFFFFFFA)


@pytest.mark.parametrize('nobj', [1, 3])
def test_shards_equal_the_batch(side, nobj):
  m.check_shards(side, h.case(nobj, 'sparse', H=7, general=True), 9)


@pytest.mark.parametrize('nobj', [1, 3])
def test_without_noise_and_with_a_nan_state(side, nobj):
  m.check_sigma_zero(side, h.case(nobj, 'sparse'), 4)
  m.check_nan_state(side, nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  cs = h.case(nobj, 'sparse')
  m.check_refusals(side, cs)
  m.check_empty(side, cs)


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_rollout_mpc_cuda_equals_the_loop_and_cpu(nobj, general):
  dev = m.check_python('cuda', nobj, general=general)
  cpu = m.check_python('cpu', nobj, general=general)
  for k in m.KEYS:
    ta.same(dev[k], cpu[k], f'rollout_mpc cuda vs cpu: {k}')


def test_rollout_mpc_replays_from_a_captured_graph():
  env, twin = tb.make_env(1, 'cuda'), tb.make_env(1, 'cuda')
  plan = torch.from_numpy(h.case(1, 'sparse').mean).cuda()
  kw = dict(K=5, iterations=2, sigma=(0.5, 0.5, 0.8), temperature=0.5, noise_counter=11)
  want = env.rollout_mpc(4, plan, **kw)
  out = {k: torch.zeros_like(v) for k, v in want.items()}
  out['plan'].copy_(plan)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    twin.rollout_mpc(4, out['plan'], out=out, **kw)
  torch.cuda.synchronize()
  assert not bool(out['reward'].any()) and not bool(out['actions'].any()), 'the captured launch ran during the capture'
  graph.replay()
  torch.cuda.synchronize()
  for k in m.KEYS:
    ta.same(out[k], want[k], f'graph replay vs the eager call: {k}')
  for k, v in tb.snapshot(env).items():
    if torch.is_tensor(v):
      ta.same(tb.snapshot(twin)[k], v, f'graph replay vs the eager call: env {k}')

"""earl_tabletop_mpc_rollout_cem / earl_tabletop3_mpc_rollout_cem (include/earl_tabletop.h, "CEM planning") on the device: cem_mpc_kernel<NOBJ, GENERAL> of
csrc/tabletop_cem_mpc.hip against the COMPOSED route on the device's own earl_tabletop[3]_plan_cem and one-step rollout (tests/tabletop_cem_helpers.py), bit for
bit in every output, the final plan and the final state, under both rewards; against the host twin under the sparse one.

The cases are those of tests/test_tabletop_cem_mpc.py (K = 1024: sixteen waves of the widest kernel) and
  9'.   device == host twin (sparse)
  10'.  rollout_mpc(method='cem') on 'cuda' == on 'cpu' (sparse)
  10''. the call captured into a HIP graph replays to the eager call's bits
"""
import pytest
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_cem_helpers as c
import tabletop_mpc_helpers as mh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def side():
  return ta.Side('cuda')


@pytest.fixture(scope='module')
def host():
  return ta.Side('cpu')


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_fused_loop_equals_the_composed_calls(side, host, nobj, rt):
  cs = c.case(nobj, rt, std0=False)
  c.check_mpc_coverage(cs, c.mpc_reference(side, cs, 6))
  full = c.check_mpc_case(side, cs, 6)
  c.check_mpc_pointers(side, cs, 6, full)
  if rt == 'sparse':
    c.check_mpc_device_vs_host(cs, 6, side, host)


@pytest.mark.parametrize('nobj', [1, 3])
def test_shapes(side, nobj):
  for H in (1, 2):
    for n in (1, 70):
      for T in (1, 6):
        c.check_mpc_case(side, c.case(nobj, 'sparse', n=n, K=5, H=H, I=2, E=2, std0=False), T)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path_zeroes_the_plan_of_a_reset_env(side, host, nobj, rt):
  cs = c.case(nobj, rt, H=7, general=True, std0=False)
  c.check_mpc_coverage(cs, c.mpc_reference(side, cs, 6), general=True)
  c.check_mpc_case(side, cs, 6)
  if rt == 'sparse':
    c.check_mpc_device_vs_host(cs, 6, side, host)


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
def test_python_rollout_mpc_cuda_equals_cpu(nobj, general):
  dev = c.check_python_mpc('cuda', nobj, general)
  cpu = c.check_python_mpc('cpu', nobj, general)
  for k in mh.KEYS:
    ta.same(dev[k], cpu[k], f"rollout_mpc(method='cem') cuda vs cpu: {k}")


def test_rollout_mpc_cem_replays_from_a_captured_graph():
  env, twin = tb.make_env(1, 'cuda'), tb.make_env(1, 'cuda')
  plan = torch.from_numpy(c.case(1, 'sparse', std0=False).mean).cuda()
  kw = dict(K=5, elites=2, iterations=2, sigma=(0.5, 0.5, 0.8), alpha=0.25, std_min=0.05, std_max=0.6, noise_counter=11, method='cem')
  want = twin.rollout_mpc(3, plan, **kw)
  out = {k: torch.zeros_like(v) for k, v in want.items()}
  out['plan'].copy_(plan)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    env.rollout_mpc(3, out['plan'], out=out, **kw)   # (in place on the plan: no copy inside the capture)
  torch.cuda.synchronize()
  assert not bool(out['actions'].any()) and not bool(out['obs'].any()),'the captured launch ran during the capture'
  graph.replay()
  torch.cuda.synchronize()
  for k in mh.KEYS:
    ta.same(out[k], want[k], f'graph replay vs the eager call: {k}')


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  c.check_mpc_refusals(side, c.case(nobj, 'sparse', std0=False))

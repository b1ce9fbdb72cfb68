"""earl_tabletop[3]_plan_mppi_value / earl_tabletop[3]_mpc_rollout_value (include/earl_tabletop.h, "discounted MPPI with a terminal value") on the device:
value::plan_score_kernel<NOBJ, GENERAL> of csrc/tabletop_plan_value.hip and value::mpc_kernel<NOBJ, GENERAL> of csrc/tabletop_mpc_value.hip through
tests/tabletop_value_helpers.py -- every buffer inside guard bands, both fills, every output pre-filled with a pattern.

The planner's oracle (that module's docstring) takes its rewards and last observations from the device's own EXISTING earl_tabletop[3]_rollout and V from
earl_mlp_policy_forward_cpu: every output bit-exact, both rewards.  The cases are those of tests/test_tabletop_value.py (1 - 9) and
  3'.  every network shape once more through the MPC kernel with K = 65 (two waves)
  9'.  plan_mppi / rollout_mpc with a value network on 'cuda' == on 'cpu' (sparse)
  10.  device == twin bit for bit under the sparse reward, both entry-point families; dense, one planner iteration: within 1e-6 * (sum |r| + |V|); the `_value` calls
       captured into a HIP graph replay to the eager bits; K = 1024 at n = 2, H = 2 through the MPC kernel with the widest allowed network (sixteen waves: the
       register-budget case)
"""
import numpy as np
import pytest
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_plan_helpers as h
import tabletop_value_helpers as v
from test_tabletop_value import SHAPES, core_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def side():
  return ta.Side('cuda')


@pytest.fixture(scope='module')
def host():
  return ta.Side('cpu')


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_core_case_equals_the_oracle(side, host, nobj, rt):
  cs = h.case(nobj, rt)
  vnet = core_net(cs)
  v.check_candidates_entry(side, cs)
  v.check_coverage(side, cs, vnet, v.reference(side, cs, vnet))
  full = v.check_case(side, cs, vnet)
  v.check_pointers(side, cs, vnet, full)
  loop = v.check_mpc_case(side, cs, 6, vnet)
  v.check_mpc_pointers(side, cs, 6, vnet, loop)
  v.check_device_vs_host(cs, vnet, side, host)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_unit_discount_without_a_value_is_the_value_free_call(side, nobj, rt):
  v.check_identity(side, h.case(nobj, rt))


@pytest.mark.parametrize('hidden,hact,oact', SHAPES)
@pytest.mark.parametrize('nobj', [1, 3])
def test_network_shapes(side, host, nobj, hidden, hact, oact):
  cs = h.case(nobj, 'dense', H=3)
  vnet = v.net(cs.sc.obs_dim, hidden, hact, oact, seed=2)
  v.check_case(side, cs, vnet)
  v.check_mpc_case(side, cs, 2, vnet)
  two = h.case(nobj, 'sparse', n=3, K=65, H=3, I=1)         # two waves of the MPC kernel
  v.check_mpc_case(side, two, 2, vnet)
  v.check_device_vs_host(two, vnet, side, host, T=2)


@pytest.mark.parametrize('nobj', [1, 3])
def test_the_value_steers_a_blind_planner(side, nobj):
  v.check_steering(side, nobj)


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path(side, host, nobj, rt):
  cs = h.case(nobj, rt, H=7, general=True)
  vnet = core_net(cs)
  v.check_case(side, cs, vnet)
  v.check_mpc_general_coverage(v.mpc_reference(side, cs, 9, vnet))
  v.check_mpc_case(side, cs, 9, vnet)
  if rt == 'sparse':
    v.check_device_vs_host(cs, vnet, side, host, T=9)


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


@pytest.mark.parametrize('nobj', [1, 3])
def test_non_finite_values(side, nobj):
  v.check_nonfinite(side, nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  v.check_refusals(side, h.case(nobj, 'sparse'))


@pytest.mark.parametrize('nobj', [1, 3])
def test_python_keywords_and_cuda_equals_cpu(nobj):
  plan_d, loop_d = v.check_python('cuda', nobj)
  plan_c, loop_c = v.check_python('cpu', nobj)
  for k in plan_d:
    ta.same(plan_d[k], plan_c[k], f'plan_mppi(discount, value) cuda vs cpu: {k}')
  for k in loop_d:
    ta.same(loop_d[k], loop_c[k], f'rollout_mpc(discount, value) cuda vs cpu: {k}')


@pytest.mark.parametrize('nobj', [1, 3])
def test_sixteen_waves_with_the_widest_network(side, host, nobj):
  """K = 1024 at n = 2, H = 2: every lane of the largest workgroup scores a branch and evaluates D -> EARL_PLAN_VALUE_MAX_H1 -> 256 -> 1"""
  cs = h.case(nobj, 'sparse', n=2, K=1024, H=2, I=1, general=nobj == 3)
  vnet = v.net(cs.sc.obs_dim, (v.MAX_H1, 256), 'tanh', 'none', seed=4)
  d, b = v.m.run_ok(side, cs.sc, cs.mean, cs.K, 2, 0x00, value=v.Value(vnet), **cs.kw)
  b.check('sixteen waves')
  hh, b = v.m.run_ok(host, cs.sc, cs.mean, cs.K, 2, 0xFF, value=v.Value(vnet), **cs.kw)
  v.m.compare(d, hh, 'sixteen waves: device vs host')
  p, b = h.run_ok(side, cs.sc, cs.mean, cs.K, 0x00, value=v.Value(vnet), **cs.kw)
  b.check('K = 1024, planner')
  ph, b = h.run_ok(host, cs.sc, cs.mean, cs.K, 0xFF, value=v.Value(vnet), **cs.kw)
  h.compare(p, ph, 'K = 1024, planner: device vs host')


def test_value_calls_replay_from_a_captured_graph():
  env = tb.make_env(1, 'cuda')
  vnet = v.net(12, (16, 16), 'tanh', 'none', seed=5)
  pi = v.python_net(vnet, env.unwrapped.device)
  mean = torch.from_numpy(h.case(1, 'sparse').mean).cuda()
  kw = dict(K=5, iterations=2, sigma=(0.5, 0.5, 0.8), temperature=0.5, noise_counter=11, discount=v.GAMMA, value=pi)
  want = env.plan_mppi(mean, **kw)
  out = {k: torch.zeros_like(t) for k, t in want.items()}
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    env.plan_mppi(mean, out=out, **kw)
  torch.cuda.synchronize()
  assert not bool(out['ret'].any()), 'the captured launches ran during the capture'
  graph.replay()
  torch.cuda.synchronize()
  for k in h.OUTS:
    ta.same(out[k], want[k], f'graph replay vs the eager call: {k}')
  # the loop: the eager call on one env, the captured one on a second env built alike (tests/test_tabletop_mpc_gpu.py)
  twin = tb.make_env(1, 'cuda')
  want = env.rollout_mpc(3, mean, **kw)
  out = {k: torch.zeros_like(t) for k, t in want.items()}
  out['plan'].copy_(mean)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    twin.rollout_mpc(3, out['plan'], out=out, **kw)
  torch.cuda.synchronize()
  assert not bool(out['reward'].any()) and not bool(out['actions'].any()), 'the captured launch ran during the capture'
  graph.replay()
  torch.cuda.synchronize()
  for k in want:
    ta.same(out[k], want[k], f'graph replay of the loop vs the eager call: {k}')

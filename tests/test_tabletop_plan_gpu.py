"""earl_tabletop_plan_mppi / earl_tabletop3_plan_mppi / earl_tabletop_plan_candidates (include/earl_tabletop.h, "MPPI planning") on the device: plan_score_kernel<NOBJ,
GENERAL>, plan_update_kernel and plan_candidates_kernel of csrc/tabletop_plan.hip through tests/tabletop_plan_helpers.py -- every buffer inside guard bands, both
fills, every output pre-filled with a pattern.

The oracle (that module's docstring) takes its returns from the device's own EXISTING earl_tabletop[3]_branch_rollout: every output bit-exact, both rewards.  Device
against host twin: bit-exact under the sparse reward; dense, one iteration: ret, ret0, best_ret within 1e-6 * sum_t |r_t|, plans not compared.

The cases are those of tests/test_tabletop_plan.py (1 core, 2 chaining, 3 candidates, 4 general, 5 state / pointers, 6 edges, 7 Python, 8 refusals) and
  6'. K = 65536 at n = 64, H = 1, I = 1: the top of the k field of the noise counter and of the int64 budget
  7'. plan_mppi on 'cuda' == on 'cpu' (sparse)
  7''. the call captured into a HIP graph (no host synchronisation, no allocation inside it) replays to the eager call's bits
"""
import numpy as np
import pytest
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
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
def test_core_case_equals_the_oracle(side, host, nobj, rt):
  cs = h.case(nobj, rt)
  h.check_coverage(cs, h.reference(cs, side))
  full = h.check_case(side, cs)
  h.check_pointers(side, cs, full)
  h.check_device_vs_host(cs, side, host)


@pytest.mark.parametrize('nobj', [1, 3])
def test_iterations_chain(side, nobj):
  h.check_chaining(side, h.case(nobj, 'dense'))


@pytest.mark.parametrize('nobj', [1, 3])
def test_candidates_entry_point(side, nobj):
  h.check_candidates(side, h.case(nobj, 'sparse'))


@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('nobj', [1, 3])
def test_general_path(side, host, nobj, rt):
  cs = h.case(nobj, rt, H=7, general=True)
  ref = h.reference(cs, side)
  tb.check_general_coverage(tb.case(nobj, rt, general=True), tb.reference(cs, side, cs.sc, ref['iters'][0]['act'], key=(id(cs), 'general')))
  h.check_case(side, cs)
  h.check_device_vs_host(cs, side, host)


@pytest.mark.parametrize('nobj', [1, 3])
def test_edges(side, nobj):
  h.check_edges(side, nobj)
  h.check_shards(side, nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_non_finite_input(side, nobj):
  h.check_nonfinite(side, nobj)


def test_the_top_of_the_branch_index(side):
  """K = 65536: k = 65535 fills the high half of the counter word, and 65536 weights of up to 2^24 times differences of up to 2^21 stay inside int64 (the sparse
  reward at a goal: many branches share the best return, so S is large).  The oracle's update runs in int64 here (its Python-integer form is held to it in the core
  case by the planner equalling both)"""
  cs = h.case(1, 'sparse', n=64, K=65536, H=1, I=1, sigma=(2.0, 2.0, 2.0))
  ref = h.oracle(side, cs.sc, cs.mean, cs.K, 1, cs.kw['sigma'], cs.kw['inv_t'], cs.kw['nc'], fast=True)
  W = ref['iters'][0]['W']
  assert int(W.sum(0).max()) > 2**36 and bool((np.abs(ref['iters'][0]['act'][65535]) == 1).any())
  res, b = h.run_ok(side, cs.sc, cs.mean, cs.K, 0xFF, **cs.kw)
  b.check('K = 65536')
  ta.assert_written(res, 'K = 65536')
  h.state_untouched(res, cs.sc, 'K = 65536')
  h.compare(res, ref, 'K = 65536')


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_plan_mppi_cuda_equals_cpu(nobj, general):
  dev = h.check_python(tb.make_env(nobj, 'cuda', general=general))
  cpu = h.check_python(tb.make_env(nobj, 'cpu', general=general))
  for k in h.OUTS:
    ta.same(dev[k], cpu[k], f'plan_mppi cuda vs cpu: {k}')


def test_plan_mppi_replays_from_a_captured_graph():
  env = tb.make_env(1, 'cuda')
  mean = torch.from_numpy(h.case(1, 'sparse').mean).cuda()
  kw = dict(K=5, iterations=2, sigma=(0.5, 0.5, 0.8), temperature=0.5, noise_counter=11)
  want = env.plan_mppi(mean, **kw)
  out = {k: torch.zeros_like(v) for k, v in want.items()}
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


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  cs = h.case(nobj, 'sparse')
  h.check_refusals(side, cs)
  h.check_empty(side, cs)

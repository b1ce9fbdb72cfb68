"""earl_tabletop_plan_cem / earl_tabletop3_plan_cem / earl_tabletop_cem_candidates (include/earl_tabletop.h, "CEM planning") on the device: cem_score_kernel<NOBJ,
GENERAL, VALUE>, cem_update_kernel and cem_candidates_kernel of csrc/tabletop_cem.hip through tests/tabletop_cem_helpers.py -- every buffer inside guard bands, both
fills, every output pre-filled with a pattern.

The oracle (that module's docstring) takes its returns from the device's own EXISTING earl_tabletop[3]_branch_rollout: every output bit-exact, both rewards.  Device
against host twin: bit-exact under the sparse reward; dense, one iteration: ret, ret0, best_ret within 1e-6 * sum_t |r_t|, plans not compared.

The cases are those of tests/test_tabletop_cem.py and
  1'.  device == host twin
  10'. plan_cem on 'cuda' == on 'cpu' (sparse)
  10''. the call captured into a HIP graph (no host synchronisation, no allocation inside it) replays to the eager call's bits
"""
import pytest
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_cem_helpers as c

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
  cs = c.case(nobj, rt)
  c.check_coverage(cs, c.reference(cs, side))
  full = c.check_case(side, cs)
  c.check_pointers(side, cs, full)
  c.check_value_identity(side, cs)
  c.check_value(side, cs)
  c.check_device_vs_host(cs, side, host)


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
def test_general_path(side, host, nobj, rt):
  cs = c.case(nobj, rt, H=7, general=True)
  ref = c.reference(cs, side)
  tb.check_general_coverage(tb.case(nobj, rt, general=True), tb.reference(cs, side, cs.sc, ref['iters'][0]['act'], key=(id(cs), 'cem general')))
  c.check_case(side, cs)
  c.check_device_vs_host(cs, side, host)


@pytest.mark.parametrize('nobj', [1, 3])
def test_non_finite_input(side, nobj):
  c.check_nonfinite(side, nobj)


@pytest.mark.parametrize('nobj', [1, 3])
def test_candidates_entry_point(side, nobj):
  c.check_candidates(side, c.case(nobj, 'sparse'))


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('nobj', [1, 3])
def test_python_plan_cem_cuda_equals_cpu(nobj, general):
  dev = c.check_python_plan(tb.make_env(nobj, 'cuda', general=general))
  cpu = c.check_python_plan(tb.make_env(nobj, 'cpu', general=general))
  for k in c.OUTS:
    ta.same(dev[k], cpu[k], f'plan_cem cuda vs cpu: {k}')


def test_plan_cem_replays_from_a_captured_graph():
  env = tb.make_env(1, 'cuda')
  cs = c.case(1, 'sparse')
  mean, std = torch.from_numpy(cs.mean).cuda(), torch.from_numpy(cs.std0).cuda()
  kw = dict(K=5, elites=2, iterations=2, sigma=(0.5, 0.5, 0.8), alpha=0.25, std_min=0.05, std_max=0.6, noise_counter=11)
  want = env.plan_cem(mean, std=std, **kw)
  out = {k: torch.zeros_like(v) for k, v in want.items()}
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    env.plan_cem(mean, std=std, out=out, **kw)
  torch.cuda.synchronize()
  assert not bool(out['ret'].any()), 'the captured launches ran during the capture'
  graph.replay()
  torch.cuda.synchronize()
  for k in c.OUTS:
    ta.same(out[k], want[k], f'graph replay vs the eager call: {k}')


@pytest.mark.parametrize('nobj', [1, 3])
def test_refusals_and_empty_work(side, nobj):
  cs = c.case(nobj, 'sparse')
  c.check_refusals(side, cs)
  c.check_empty(side, cs)

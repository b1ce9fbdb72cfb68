"""earl_tabletop[3]_plan_mppi_prior on the MI355X: prior_noise_kernel, prior_score_kernel and prior_update_kernel of csrc/tabletop_prior.hip through
tests/tabletop_prior_helpers.py -- every buffer inside guard bands, both fills -- against the oracle of that module (which uses none of the new code: on the device the
device's own one-step rollouts and branch launch), against the host twin, from a captured graph and through Python.  Every comparison is bit for bit."""
import pytest
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_plan_helpers as h
import tabletop_prior_helpers as p

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def side():
  return ta.Side('cuda')


@pytest.fixture(scope='module')
def host():
  return ta.Side('cpu')


@pytest.mark.parametrize('spec', p.CASES, ids=lambda s: '-'.join(map(str, s)))
def test_the_call_equals_the_oracle_and_the_twin(side, host, spec):
  cs, prior, value = p.setup(*spec)
  ref = p.reference(cs, side, prior, value)
  if cs.general:
    p.check_trace(cs, ref)
  dev = p.check_case(side, cs, prior, value)
  if cs.rt == 'sparse':                                     # (dense: the device's exp; the twin is held to its own oracle in tests/test_tabletop_prior.py)
    twin, b = p.run_ok(host, cs.sc, cs.mean, cs.K, 0x00, prior, value=value, **cs.kw)
    p.compare(dev, twin, cs.what + ' device vs host')


def test_a_256_wide_policy(side, host):
  cs = h.case(1, 'sparse', n=3, K=3, H=2, I=1)
  prior = p.Prior(p.pnet(12, (256,), 'tanh', 'tanh'), 1)
  dev = p.check_case(side, cs, prior)
  twin, b = p.run_ok(host, cs.sc, cs.mean, cs.K, 0x00, prior, **cs.kw)
  p.compare(dev, twin, cs.what + ' device vs host')


@pytest.mark.parametrize('nobj', [1, 3])
def test_one_noiseless_prior_branch_is_the_closed_loop_rollout(nobj):
  p.check_closed_loop_identity('cuda', nobj)


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


def test_the_call_replays_from_a_captured_graph():
  env = tb.make_env(1, 'cuda')
  mean = torch.from_numpy(h.case(1, 'sparse').mean).cuda()
  pi = p.python_net(p.pnet(12, (32,), 'tanh', 'tanh'), 'cuda')
  kw = dict(K=6, iterations=2, sigma=(0.5, 0.5, 0.8), temperature=0.5, noise_counter=11, prior=pi, prior_branches=2, prior_sigma=(0.2, 0.0, 0.4))
  want = env.plan_mppi(mean, **kw)
  out = {k: torch.zeros_like(x) for k, x in want.items()}
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    env.plan_mppi(mean, out=out, **kw)
  torch.cuda.synchronize()
  assert not bool(out['ret'].any()) and not bool(out['prior_actions'].any()), 'the captured launches ran during the capture'
  graph.replay()
  torch.cuda.synchronize()
  for k in p.OUTS:
    ta.same(out[k], want[k], f'graph replay vs the eager call: {k}')


@pytest.mark.parametrize('nobj', [1, 3])
def test_through_python_the_device_equals_the_host(nobj):
  dev, cpu = p.check_python('cuda', nobj), p.check_python('cpu', nobj)
  for what in dev:
    for k in p.OUTS:
      ta.same(dev[what][k], cpu[what][k], f"plan_mppi(prior) {what}: device='cuda' vs device='cpu': {k}")

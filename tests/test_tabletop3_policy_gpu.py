"""earl_tabletop3_policy_rollout on the MI355X (csrc/tabletop3_policy.hip: tabletop_policy_kernel.inc with NOBJ = 3), held to its host twin bit for bit:
  9.  every instantiation (NT2 x GENERAL x GAUSS, single policy and population) and every hidden width 16 .. 256 at both layer positions, sparse reward: obs, reward,
      done, success, act_out, eps_out, the summaries, the final state; under the dense reward everything but reward / ret bit for bit, those within the tolerance
      tests/test_tabletop_gpu.py uses for the three-object dense reward;
  10. the wide shapes against an exact integer reference (a wrong lane or k-step mapping shows independently of the host twin);
  11. closed loop = open loop on the device, both forms with auto-reset, and the coverage condition's run of tests/test_tabletop3_policy.py;
  12. the Python path on device='cuda' against device='cpu';
  13. banded buffers: guard bands of 0x00 and 0xFF round every output, every optional pointer NULL in turn, pre-filled outputs fully overwritten, n = 0.
Shapes: n = 40, env_offset = 3, T = 12 (tests/policy_width_cases.py): a workgroup that starts at a negative local index, a full one and a ragged one.
Observed (one MI355X): no difference on any of the 211 cases; the slowest case 0.30 s (the first, which loads the library), at most 0.16 s otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_width_cases as W
import tabletop3_policy_helpers as t3
import tabletop_abi as A
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import Packed
from policy_width_cases import N, OFFSET, T
from population_helpers import members_needed, summary_by_definition
from test_policy_rollout import assert_same_bits, assert_same_state, final_state
from test_tabletop_gpu import DENSE_ATOL, DENSE_RTOL

pytestmark = pytest.mark.gpu
GPU, CPU = 'cuda:0', 'cpu'
FORMS = {'evaluation': dict(horizon=T), 'continuing': dict(auto_reset=True, horizon=7)}      # GENERAL = auto-reset (the three-object env has no lifelong switch)
HEAD_KW = {'deterministic': None, 'sample': dict(mode='sample', log_std_map='tanh')}
G = 16


def name_of(hidden, form, head):
  return f'tabletop3_policy_kernel<NT2 = {W.nt2_of(hidden)}, GENERAL = {str(form == "continuing").lower()}, GAUSS = {str(head == "sample").lower()}>'


def one_run(device, s, hidden, head, form, rt='sparse', population=False):
  """one launch of the case on `device` -> (outputs, final state)"""
  reset_first = form == 'evaluation'
  hact, oact = ('relu', 'tanh')[s % 2], ('tanh', 'none')[(s // 2) % 2]
  h = t3.harness(device, reward_type=rt, reset_at_goal=True, seed=1000 + s, **FORMS[form])
  t3.start_somewhere(h)
  if population:
    net = t3.Population3(hidden, members_needed(OFFSET, N, G), G, gaussian=head == 'sample', hidden_act=hact, out_act=oact, seed0=11 + s, device=device)
  else:
    net = t3.net3(hidden, hact, oact, seed=1000 + s, gaussian=head == 'sample', device=device)
  res = t3.rollout3(h, net.struct, 2 if reset_first else 1, T, reset_first, pop=net.pop if population else None, head=HEAD_KW[head])
  return res, final_state(h)


def hold_to_host(what, got, want, keys, dense=False):
  for k in [k for k in ('eps', 'act') if k in keys]:                    # the actions first, with the kernel's name and the first differing value
    g, w = got[k].reshape(-1, N, 3), want[k].reshape(-1, N, 3)
    if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
      bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
      t, i, j = bad[0]
      raise AssertionError(f'{what}: {len(bad)} of {w.size} values of {k} differ; first at step {t} env {i} action {j}: device {g[t, i, j]!r} host {w[t, i, j]!r}')
  assert_same_bits(got, want, [k for k in keys if not (dense and k in ('reward', 'ret'))])
  if dense:
    for k in ('reward', 'ret'):
      np.testing.assert_allclose(got[k], want[k], rtol=DENSE_RTOL, atol=DENSE_ATOL, err_msg=f'{what} {k}')


SINGLE = [(s, hidden, head, form) for s, hidden in enumerate(W.SHAPES) for head in W.HEADS for form in W.FORMS]
POPULATION = [(s, hidden, head, form) for s, hidden in enumerate(W.POPULATION_SHAPES) for head in W.HEADS for form in W.FORMS]
IDS = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_the_case_tables_reach_every_instantiation_and_every_width():
  for table in (SINGLE, POPULATION):
    assert {(W.nt2_of(hidden), form, head) for _, hidden, head, form in table} == {(nt2, f, hd) for nt2 in range(5) for f in W.FORMS for hd in W.HEADS}
  for layer in (0, 1):
    assert {hidden[layer] for _, hidden, _, _ in SINGLE if len(hidden) > layer} == set(W.WIDTHS)


# ---------------------------------------------------------------------------------------------------------------- 9. device = host twin
@pytest.mark.parametrize('s,hidden,head,form', SINGLE, ids=IDS)
def test_device_equals_host_twin_bit_for_bit(s, hidden, head, form):
  (got, end_d), (want, end_h) = one_run(GPU, s, hidden, head, form), one_run(CPU, s, hidden, head, form)
  assert np.isfinite(want['act']).all()
  keys = ('act',) + (('eps',) if head == 'sample' else ()) + t3.OUT + t3.SUMMARY
  hold_to_host(f'{hidden} {head} {form} -> {name_of(hidden, form, head)}', got, want, keys)
  assert_same_state(end_d, end_h)
  assert want['done'].any()


@pytest.mark.parametrize('s,hidden,head,form', POPULATION, ids=IDS)
def test_population_device_equals_host_twin_bit_for_bit(s, hidden, head, form):
  (got, end_d), (want, end_h) = one_run(GPU, s, hidden, head, form, population=True), one_run(CPU, s, hidden, head, form, population=True)
  keys = ('act',) + (('eps',) if head == 'sample' else ()) + t3.OUT + t3.SUMMARY
  hold_to_host(f'population {hidden} {head} {form} -> {name_of(hidden, form, head)}', got, want, keys)
  assert_same_state(end_d, end_h)
  lead = (-1, T, N)
  ref = summary_by_definition(got['reward'].reshape(lead), got['success'].reshape(lead))
  for k in t3.SUMMARY:
    np.testing.assert_array_equal(got[k].view(np.uint8), ref[k].view(np.uint8), err_msg=k)
  members = [(OFFSET + i) // G for i in range(N)]
  first = want['act'].reshape(-1, N, 3)[0]
  assert len({tuple(first[members.index(m)]) for m in range(3)}) == 3                   # (three members, acting differently)


@pytest.mark.parametrize('s,hidden,head,form', [(1, (208,), 'sample', 'evaluation'), (2, (80, 112), 'deterministic', 'continuing'), (3, (48, 240), 'sample', 'continuing')], ids=IDS)
@pytest.mark.parametrize('population', [False, True], ids=['single', 'population'])
def test_dense_reward_everything_but_the_reward_bit_for_bit(s, hidden, head, form, population):
  (got, end_d), (want, end_h) = (one_run(dev, s, hidden, head, form, rt='dense', population=population) for dev in (GPU, CPU))
  keys = ('act',) + (('eps',) if head == 'sample' else ()) + t3.OUT + t3.SUMMARY
  hold_to_host(f'dense {hidden} {head} {form} -> {name_of(hidden, form, head)}', got, want, keys, dense=True)
  assert_same_state(end_d, end_h)
  assert (want['reward'] != 0).all()


# ---------------------------------------------------------------------------------------------------------------- 10. lane maps against an exact reference
@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian-mean'])
@pytest.mark.parametrize('hidden', W.EXACT_SHAPES, ids=IDS)
def test_lane_maps_against_an_exact_reference_at_the_wide_shapes(hidden, gaussian):
  """ReLU hidden layers, no output activation, weights in {-1, 0, 1}, integer biases in [-3, 3], observations that are multiples of 0.5 with |x| <= 3: every product
  and partial sum is exact in float32 (|layer 0| <= 63, |layer 1| <= 16131, |output| <= 4.2e6 = 8.3e6 half-units < 2^24), so the reference is numpy float64 in any
  order, and a swapped row / column, a permuted k-step of the five of layer 0 or a dropped tile shows as a wrong number, not as a rounding difference"""
  rng = np.random.default_rng(sum(hidden))
  dims = [t3.OBS] + list(hidden) + [6 if gaussian else 3]
  layers = [(rng.integers(-1, 2, (n, k)).astype(np.float32), rng.integers(-3, 4, n).astype(np.float32)) for k, n in zip(dims[:-1], dims[1:])]
  pol = Packed(layers, 'relu', 'none', device=GPU)
  goals = np.random.default_rng(2).integers(-6, 7, size=(4, 10)) / 2.0
  d = t3.harness(GPU, n=G + 5, reward_type='sparse', horizon=5, seed=1, goal_table=goals, n_sample_goals=4)
  d.reset()
  n = d.n
  q = np.random.default_rng(3).integers(-4, 5, size=(n, 8)) / 2.0          # 21 different rows of half-integers in [-2, 2]
  gi = (np.arange(n) % 4).astype(np.int32)
  d.qpos.copy_(torch.tensor(q))
  d.goal_idx.copy_(torch.tensor(gi))
  x = np.concatenate([q, np.full((n, 2), -1.0), goals[gi]], axis=1)       # _get_obs of that state: qpos, the free flag pair, the goal row
  assert x.shape == (n, t3.OBS) and (np.abs(x) <= 3).all() and len(np.unique(x, axis=0)) == n
  v, biggest = x, 0.0
  for l, (w, b) in enumerate(layers):
    v = v @ w.astype(np.float64).T + b.astype(np.float64)
    biggest = max(biggest, float(np.abs(v).max()))
    if l + 1 < len(layers):
      v = np.maximum(v, 0)
  assert biggest < 2 ** 23 and (v[:, :3] != 0).any() and len(np.unique(v[:, :3], axis=0)) > n // 2
  got = t3.rollout3(d, pol.struct, 1, 1, False, head=dict(mode='mean') if gaussian else None)
  act = got['act'][0].astype(np.float64)
  if not np.array_equal(act, v[:, :3]):
    bad = np.argwhere(act != v[:, :3])
    i, j = bad[0]
    raise AssertionError(f'{hidden} -> NT2 = {W.nt2_of(hidden)}: {len(bad)} of {act.size} actions differ; first at env {i} action {j}: device {act[i, j]!r} exact {v[i, j]!r}')


# ---------------------------------------------------------------------------------------------------------------- 11. closed = open on the device
@pytest.mark.parametrize('form', W.FORMS)
@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'sample'])
def test_closed_equals_open_on_the_device_with_auto_reset(gaussian, form):
  h = t3.harness(GPU, reward_type='dense', reset_at_goal=True, seed=6, auto_reset=True, horizon=7)
  t3.start_somewhere(h)
  pol = t3.net3((48, 32), 'tanh', seed=3, gaussian=gaussian, device=GPU)
  reset_first = form == 'evaluation'
  got, _ = t3.closed_equals_open3(h, pol.struct, 2 if reset_first else 1, T, reset_first, head=dict(mode='sample') if gaussian else None)
  assert got['done'].any()


def test_the_coverage_run_on_the_device():
  runs = {}
  for dev in (GPU, CPU):
    h = t3.coverage_harness(dev)
    att0 = h.host('attached').copy()
    pol = t3.coverage_policy(dev)
    got, _ = t3.closed_equals_open3(h, pol.struct, 1, t3.COVERAGE_T, False)
    runs[dev] = (got, final_state(h))
    latched, released, inside = t3.coverage_of(att0, got)
    assert latched == {0, 1, 2} and released >= 1 and all(inside), (dev, latched, released, inside)
  assert_same_bits(runs[GPU][0], runs[CPU][0], ('act',) + t3.OUT + t3.SUMMARY)
  assert_same_state(runs[GPU][1], runs[CPU][1])


# ---------------------------------------------------------------------------------------------------------------- 12. the Python path
def test_the_python_path_on_cuda_agrees_with_cpu():
  from test_tabletop3_policy import python_path
  dev, _ = python_path(GPU)
  host, _ = python_path(CPU)
  assert set(dev) == set(host)
  for name in host:
    assert len(dev[name]) == len(host[name])
    for a, b in zip(dev[name], host[name]):
      assert a.shape == b.shape and a.dtype == b.dtype, name
      assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), name


# ---------------------------------------------------------------------------------------------------------------- 13. banded buffers
OPTIONAL = ('obs', 'reward', 'done', 'success', 'act', 'eps', 'ret', 'success_last', 'first_success')


def run_banded(side, sc, net, E, Tn, reset_first, fill, head=None, pop=None, summary=True, null=(), n_call=None):
  """earl_tabletop3_policy_rollout on banded buffers (tests/tabletop_abi.py: Run) -> (results, Bands); names in `null` are passed as NULL"""
  n = sc.n
  lead = (E, Tn, n) if reset_first else (Tn, n)
  r = A.Run(side, fill, null)
  st = r.state(sc)
  params = r.put('in.params', net.params)
  ps = net.struct
  pol = _abi.MlpPolicy(n_layers=ps.n_layers, dims=ps.dims, hidden_act=ps.hidden_act, out_act=ps.out_act, precision=0, params=params.data_ptr())
  out = r.out(lead, t3.OBS)
  r.blank('out.act', lead + (3,), torch.float32, n * 3)
  hd = None
  if head is not None:
    r.blank('out.eps', lead + (3,), torch.float32, n * 3)
    hd = _abi.GaussianHead(mode=1, log_std_map=1, log_std_min=-5.0, log_std_max=2.0, eps_out=r.ptr('out.eps'))
  sm = None
  if summary:
    for k, dt in A.SUMMARY:
      r.blank('out.' + k, (E, n), dt, n)
    sm = _abi.EpisodeSummary(**{k: r.ptr('out.' + k) for k, _ in A.SUMMARY})
  cfg = sc.cfg() if n_call is None else sc.cfg(n=n_call)
  ref = lambda s: None if s is None else C.byref(s)
  rc = side.lib.earl_tabletop3_policy_rollout(C.byref(cfg), C.byref(st), C.byref(pol), ref(pop), ref(hd), E, Tn, int(reset_first), C.byref(out), r.ptr('out.act'),
                                              ref(sm), side.stream)
  return r.finish(rc, 'tabletop3_policy_rollout')


@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'sample'])
@pytest.mark.parametrize('form', W.FORMS)
def test_banded_buffers_optional_pointers_and_the_empty_batch(form, gaussian):
  reset_first = form == 'evaluation'
  E = 2 if reset_first else 1
  sc = A.Scene(N, nobj=3, reward_type='sparse', reset_at_goal=True, seed=3, env_offset=OFFSET, **FORMS[form])
  net = t3.Population3((48, 80), members_needed(OFFSET, N, G), G, gaussian=gaussian, seed0=5)
  head = {} if gaussian else None
  dev, host = A.Side(GPU), A.Side(CPU)
  kw = dict(head=head, pop=net.pop)
  full = A.both_fills(run_banded, dev, sc, net, E, T, reset_first, what=f'{form} all outputs', **kw)
  want, _ = run_banded(host, sc, net, E, T, reset_first, A.FILLS[0], **kw)
  A.agree(full, want, f'{form}: device vs host twin')
  for name in OPTIONAL:                                                 # every optional pointer NULL in turn: the others, and the state, unchanged
    if name == 'eps' and not gaussian:
      continue
    res = A.both_fills(run_banded, dev, sc, net, E, T, reset_first, what=f'{form} without {name}', null=(name,), **kw)
    A.agree(res, full, f'{form} without {name}', null=(name,))
  none = A.both_fills(run_banded, dev, sc, net, E, T, reset_first, what=f'{form} without a summary', summary=False, **kw)
  A.agree(none, {k: v for k, v in full.items() if k[4:] not in t3.SUMMARY}, f'{form} without a summary')
  single = t3.net3((48, 80), seed=5, gaussian=gaussian)                  # pop == NULL: one policy
  one = A.both_fills(run_banded, dev, sc, single, E, T, reset_first, what=f'{form} one policy', head=head)
  want1, _ = run_banded(host, sc, single, E, T, reset_first, A.FILLS[0], head=head)
  A.agree(one, want1, f'{form} one policy: device vs host twin')
  for fill in A.FILLS:                                                  # n = 0: EARL_OK, nothing written
    res, b = run_banded(dev, sc, net, E, T, reset_first, fill, n_call=0, **kw)
    b.check(f'{form} n = 0')
    A.assert_untouched(res, sc, f'{form} n = 0')

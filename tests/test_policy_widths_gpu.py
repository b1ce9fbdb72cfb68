"""The width and instantiation matrix of the tabletop policy kernels on the MI355X (csrc/tabletop_policy.h, tabletop_policy_kernel.inc, tabletop_pair_kernel.h):
every hidden width 16 .. 256 at every layer position and every one of the 46 instantiations (single 10 + Gaussian 10 + population 20 + pair 6) runs on the device
and is held to the host twin bit for bit -- actions, draws, observations, rewards, flags, the state left behind -- on the smallest launch that has a full, a middle
and a ragged workgroup (n = 40, env_offset = 3, T = 12).  tests/policy_width_cases.py holds the tables; tests/test_policy_math.py shows without a GPU that they
reach every instantiation and width, and that the host twin's actions change when the last N-tile of either hidden layer is zeroed (so a dropped or misplaced tail
tile shows here).  The wide shapes are also held to an independent exact reference (weights in {-1, 0, 1}: numpy float64, any summation order).
The instantiation a case dispatches to is part of its failure message and of the case's printed line (policy_width_cases.instantiation restates the launchers' rule)."""
import numpy as np
import pytest
import torch

import hip_harness as hx
import policy_width_cases as W
from gaussian_policy_helpers import Packed, gaussian_rollout
from population_helpers import OUT, SUMMARY, summary_by_definition
from test_policy_rollout import assert_same_bits, assert_same_state, final_state, policy_rollout

pytestmark = pytest.mark.gpu
GPU, CPU = 'cuda:0', 'cpu'


def hold_to_host(what, inst, got, want, keys, reset_first):
  """act (and eps) first, with the shape, the instantiation and the first differing (episode, step, env, action); then every other output bit for bit"""
  for k in [k for k in ('eps', 'act') if k in keys]:
    g, w = got[k], want[k]
    if not reset_first:
      g, w = g[None], w[None]
    if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
      bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
      e, t, i, j = bad[0]
      raise AssertionError(f'{what} -> {W.name_of(inst)}: {len(bad)} of {w.size} values of {k} differ; first at episode {e} step {t} env {i} action {j}: '
                           f'device {g[e, t, i, j]!r} host {w[e, t, i, j]!r}')
  assert_same_bits(got, want, keys)


# ---------------------------------------------------------------------------------------------------------------- 1. the single-policy kernels, 39 shapes x 2 heads x 2 forms
@pytest.mark.parametrize('case', W.CASES, ids=lambda c: c.id)
def test_device_equals_host_twin_bit_for_bit(case):
  """39 shapes x {deterministic, sampled} x {evaluation, continuing}.  Dispatch (policy_width_cases.instantiation, printed per case): policy_rollout_kernel<NT2,
  GENERAL, GAUSS> with NT2 = 0 for the 16 one-hidden-layer shapes, ceil(H2 / 64) otherwise (NT2 = 1: H2 16 .. 64, 2: 80 .. 128, 3: 144 .. 192, 4: 208 .. 256),
  GENERAL = the continuing form, GAUSS = the sampled head: all 20 instantiations, 6 to 10 shapes each.
  Observed (one MI355X): no difference on any of the 156 cases; the slowest case 0.19 s (the first, which loads the library), 0.02 .. 0.11 s otherwise"""
  d, h = case.harness(GPU), case.harness(CPU)
  got, want = case.run(d, case.policy(GPU)), case.run(h, case.policy(CPU))
  print(f'{case.id} {case.hact}/{case.oact} {case.cfg_kw} -> {W.name_of(case.inst)}')
  assert np.isfinite(want['act']).all()
  hold_to_host(f'{case.id} {case.hact}/{case.oact} {case.cfg_kw}', case.inst, got, want, case.keys(), case.reset_first)
  assert_same_state(final_state(d), final_state(h))
  if case.cfg_kw.get('auto_reset'):                                     # the reset fell inside the launch (goal_change_frequency = 5 < T: so does the switch)
    assert want['done'].any()


# ---------------------------------------------------------------------------------------------------------------- 2. the population kernel, its 20 instantiations
@pytest.mark.parametrize('hidden,head,form', W.POPULATION_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_population_device_equals_host_twin_bit_for_bit(hidden, head, form):
  """three workgroups, three members (G = 16, global ids 3 .. 42); the summaries too.  Dispatch: policy_population_kernel<NT2, GENERAL, GAUSS>, NT2 = 0 .. 4 from
  (208,), (144, 48), (80, 112), (112, 176), (48, 240): its 20 instantiations, one case each.  Observed (one MI355X): no difference; at most 0.07 s a case"""
  reset_first = form == 'evaluation'
  inst = W.instantiation('population', hidden, W.POPULATION_FORMS[form], head)
  (got, end_d), (want, end_h) = W.population_run(GPU, hidden, head, form), W.population_run(CPU, hidden, head, form)
  print(f'{hidden} {head} {form} -> {W.name_of(inst)}')
  keys = ('act',) + (('eps',) if head == 'sample' else ()) + OUT + SUMMARY
  hold_to_host(f'population {hidden} {head} {form}', inst, got, want, keys, reset_first)
  assert_same_state(end_d, end_h)
  if reset_first:
    ref = summary_by_definition(got['reward'], got['success'])
    for k in SUMMARY:
      np.testing.assert_array_equal(got[k].view(np.uint8), ref[k].view(np.uint8), err_msg=k)
  members = [(W.OFFSET + i) // W.POPULATION_G for i in range(W.N)]
  first = want['act'][0, 0] if reset_first else want['act'][0]
  assert len({tuple(first[members.index(m)]) for m in range(3)}) == 3                   # (three members, acting differently)


# ---------------------------------------------------------------------------------------------------------------- 3. the pair kernel, every width it takes
@pytest.mark.parametrize('hidden,head', W.PAIR_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_pair_device_equals_host_twin_bit_for_bit(hidden, head):
  """switch_every = (7, 5), switch_on_success = 1, T = 12: both clocks run out inside the launch.  Dispatch: pair_kernel<NOBJ = 1, NT2, GAUSS>, NT2 = 0 for the 16
  one-hidden-layer widths, 1 for H2 16 .. 64, 2 for H2 80 .. 128 and (128, 128): its 6 instantiations.  Observed (one MI355X): no difference on any of the 50 cases"""
  inst = W.instantiation('pair', hidden, {}, head)
  (got, end_d, ps_d), (want, end_h, ps_h) = W.pair_run(GPU, hidden, head), W.pair_run(CPU, hidden, head)
  print(f'{hidden} {head} -> {W.name_of(inst)}')
  keys = ('act',) + (('eps',) if head == 'sample' else ()) + OUT + ('agent', 'fs', 'bs')
  hold_to_host(f'pair {hidden} {head}', inst, got, want, keys, False)
  assert_same_state(end_d, end_h)
  np.testing.assert_array_equal(ps_d[0], ps_h[0])
  np.testing.assert_array_equal(ps_d[1], ps_h[1])
  assert (want['agent'] == 0).any() and (want['agent'] == 1).any() and (want['agent'][1:] != want['agent'][:-1]).any()      # both agents acted, and handovers happened


# ---------------------------------------------------------------------------------------------------------------- 4. lane maps against an exact reference
def exact_layers(hidden, nout, seed):
  """weights in {-1, 0, 1} with no symmetry in (j, k), integer biases in [-3, 3]"""
  rng = np.random.default_rng(seed)
  dims = [12] + list(hidden) + [nout]
  return [(rng.integers(-1, 2, (n, k)).astype(np.float32), rng.integers(-3, 4, n).astype(np.float32)) for k, n in zip(dims[:-1], dims[1:])]


@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian-mean'])
@pytest.mark.parametrize('hidden', W.EXACT_SHAPES, ids=lambda sh: 'x'.join(map(str, sh)))
def test_lane_maps_against_an_exact_reference_at_the_wide_shapes(hidden, gaussian):
  """ReLU hidden layers, no output activation, weights in {-1, 0, 1}, observations that are multiples of 0.5 with |x| <= 3: every product and partial sum is exact
  in float32 (|layer 0| <= 39, |layer 1| <= 9987, |output| <= 2.56e6 = 5.1e6 half-units < 2^24), so the reference is numpy float64 in any order and a swapped
  row / column, a permuted k or a dropped tile shows as a wrong number, not as a rounding difference.  Observed (one MI355X): exact on all 18 cases"""
  n = 16
  layers = exact_layers(hidden, 6 if gaussian else 3, seed=sum(hidden))
  pol = Packed(layers, 'relu', 'none', device=GPU)
  d = hx.HipTabletop(n, device=GPU, horizon=5, seed=1)
  d.reset()
  code = np.random.default_rng(3).choice(5 ** 4, n, replace=False)        # 16 different rows of small integers in [-2, 2] (the goal rows add -2.5)
  q = (code[:, None] // 5 ** np.arange(4) % 5 - 2).astype(np.float64)
  d.qpos.copy_(torch.tensor(q))
  x = d.observe()[0].astype(np.float64)
  assert (2 * x == np.round(2 * x)).all() and (np.abs(x) <= 3).all() and len(np.unique(x, axis=0)) == n
  v, biggest = x, 0.0
  for l, (w, b) in enumerate(layers):
    v = v @ w.astype(np.float64).T + b.astype(np.float64)
    biggest = max(biggest, float(np.abs(v).max()))
    if l + 1 < len(layers):
      v = np.maximum(v, 0)
  assert biggest < 2 ** 23
  assert (v[:, :3] != 0).any() and len(np.unique(v[:, :3], axis=0)) > n // 2
  inst = W.instantiation('single', hidden, {}, 'sample' if gaussian else 'deterministic')
  got = gaussian_rollout(d, pol, 1, 1, False, mode='mean') if gaussian else policy_rollout(d, pol, 1, 1, False)
  act = got['act'][0].astype(np.float64)
  if not np.array_equal(act, v[:, :3]):
    bad = np.argwhere(act != v[:, :3])
    i, j = bad[0]
    raise AssertionError(f'{hidden} -> {W.name_of(inst)}: {len(bad)} of {act.size} actions differ; first at env {i} action {j}: device {act[i, j]!r} exact {v[i, j]!r}')

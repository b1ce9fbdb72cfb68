"""earl_tabletop3_pair_rollout on the MI355X (csrc/tabletop3_pair.hip), held to its host twin bit for bit:
  10. every output, the state left behind and the pair state, over shape x hidden activation x head x goal x form, on the three paths of the kernel (every workgroup
      all-forward, all-reset, mixed -- asserted from agent_out in every form); the shapes hit every tile-ownership edge of every width class; under the dense reward everything but the reward;
  11. the widest shape of each class against an exact integer reference with different small-integer weights per agent (the lane maps and the LDS images of the
      output weights, the layer-0 weights and the two agents, independently of the host twin);
  12. the env state parked in LDS across the networks at NT2 = 2: a handover at every step with auto-reset;
  13. never switching equals earl_tabletop3_policy_rollout on the device; shards equal the batch and two launches equal one; NULL outputs leave the state alone;
  14. banded buffers: guard bands of 0x00 and 0xFF round every buffer, every optional pointer NULL in turn, n = 0;
  15. env.rollout_agents on device='cuda' equals the same call on device='cpu'.
Shapes: n = 40 envs at env_offset = 3 (three workgroups, the last one ragged), T = 12 .. 24, horizon = 7 where an auto-reset is wanted.
Observed (one MI355X): no difference on any of the 220 cases; the slowest case 0.48 s (the first, which loads the library), at most 0.16 s otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import tabletop3_pair_helpers as p3
import tabletop3_policy_helpers as t3
import tabletop_abi as A
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import Packed
from tabletop3_pair_helpers import INITIAL3, OUT, Pair3, PairState, assert_bits, keys_of, pair_rollout3, single_rollout3, workgroup_shares
from test_policy_rollout import assert_same_state, final_state, restore, snapshot
from test_tabletop3_pair import FORMS, HEADS, N, OFFSET, coverage_run
from test_tabletop_gpu import DENSE_ATOL, DENSE_RTOL

pytestmark = pytest.mark.gpu
GPU, CPU = 'cuda:0', 'cpu'
# NT2 = 0: (16,) only wave 0 owns a layer-0 tile, (80,) wave 0 owns two, (256,) every wave four; NT2 = 1 and 2: the narrowest and the widest of the class
SHAPES = [(16,), (80,), (256,), (48, 16), (256, 64), (16, 80), (256, 128)]
WIDEST = [(256,), (256, 64), (256, 128)]
IDS = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)
T = 14


def start_phases(path, reset_first=False):
  """-> (phase, clock, switch_every, switch_on_success): all envs forward resp. reset with clocks that never run out (an auto-reset sends every env forward at the
  same step: the workgroups stay uniform), or random phases and clocks with short clocks and handover on success.  The evaluation form (reset_first) starts every
  episode in the forward phase whatever the start phases are: there the reset path hands every env over after the episode's first step (switch_every = (1, never)),
  so that the workgroups are all-reset from the second step on, and the mixed path gets its mix from the handovers on success"""
  if path in ('forward', 'reset'):
    se = (1, 10**6) if reset_first and path == 'reset' else (10**6, 10**6)
    return np.full(N, path == 'reset', np.int8), np.zeros(N, np.int32), se, 0
  rng = np.random.default_rng(5)
  return rng.integers(0, 2, N).astype(np.int8), rng.integers(0, 3, N).astype(np.int32), (4, 3), 1


def one_run(device, hidden, hact, head, goal, form, path, reward='sparse'):
  E, reset_first, cfg_kw = FORMS[form]
  h = p3.prepared(device, reset_first, reward_type=reward, reset_at_goal=True, seed=9, **cfg_kw)
  pr = Pair3(hidden, gaussian=HEADS[head] is not None, hidden_act=hact, seed0=4, device=device)
  phase, sip, se, on_success = start_phases(path, reset_first)
  ps = PairState(N, device=device, phase=phase, sip=sip)
  got = pair_rollout3(h, pr, ps, E, T, reset_first, se, on_success, backward_goal=None if goal is None else INITIAL3, head=HEADS[head])
  return got, final_state(h), ps.host()


def hold_to_host(what, got, want, keys, skip=()):
  g, w = got['act'].reshape(-1, N, 3), want['act'].reshape(-1, N, 3)
  if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    t, i, j = bad[0]
    raise AssertionError(f'{what}: {len(bad)} of {w.size} actions differ; first at step {t} env {i} action {j}: device {g[t, i, j]!r} host {w[t, i, j]!r}, '
                         f'agent {want["agent"].reshape(-1, N)[t, i]}')
  assert_bits(got, want, [k for k in keys if k not in skip])


# ---------------------------------------------------------------------------------------------------------------- 10. device = host twin
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('goal', [None, 'initial'])
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('hact', ['relu', 'tanh'])
@pytest.mark.parametrize('hidden', SHAPES, ids=IDS)
def test_device_equals_host_twin_bit_for_bit_on_all_three_paths(hidden, hact, head, goal, form):
  reset_first = FORMS[form][1]
  for path in ('forward', 'reset', 'mixed'):
    (got, end_d, ps_d), (want, end_h, ps_h) = (one_run(dev, hidden, hact, head, goal, form, path) for dev in (GPU, CPU))
    assert np.isfinite(want['act']).all()
    hold_to_host(f'{hidden} {hact} {head} goal={goal} {form} {path}', got, want, keys_of(HEADS[head]) + ('agent', 'fs', 'bs'))
    assert_same_state(end_d, end_h)
    np.testing.assert_array_equal(ps_d[0], ps_h[0])
    np.testing.assert_array_equal(ps_d[1], ps_h[1])
    mixed, fwd, rst = workgroup_shares(got['agent'])
    if reset_first:                                            # (each episode's reset puts every env into the forward phase: the start phases are not used)
      assert (got['agent'][:, 0] == 0).all()
    if path == 'forward':
      assert (mixed, fwd, rst) == (0.0, 1.0, 0.0)
    elif path == 'reset' and reset_first:                      # forward at each episode's first step, the reset agent's from there on
      assert (got['agent'][:, 1:] == 1).all() and mixed == 0.0 and rst == (T - 1) / T
    elif path == 'reset':
      assert mixed == 0.0 and rst > 0.0 and (form == 'auto_reset' or rst == 1.0)
    elif reset_first:                                          # the handovers on success come at different steps inside a workgroup
      assert mixed > 0
    else:
      first = got['agent'][0]
      assert all(len(np.unique(first[i0:i0 + 16])) == 2 for i0 in range(0, N, 16)), 'a workgroup is uniform at the first step'
      assert mixed > 0


@pytest.mark.parametrize('form', ['continuing', 'auto_reset'])
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('hidden', WIDEST, ids=IDS)
def test_dense_reward_everything_but_the_reward_bit_for_bit(hidden, head, form):
  (got, end_d, ps_d), (want, end_h, ps_h) = (one_run(dev, hidden, 'tanh', head, 'initial', form, 'mixed', reward='dense') for dev in (GPU, CPU))
  hold_to_host(f'dense {hidden} {head} {form}', got, want, keys_of(HEADS[head]) + ('agent', 'fs', 'bs'), skip=('reward',))
  np.testing.assert_allclose(got['reward'], want['reward'], rtol=DENSE_RTOL, atol=DENSE_ATOL)
  assert (want['reward'] != 0).all()
  assert_same_state(end_d, end_h)
  np.testing.assert_array_equal(ps_d[0], ps_h[0])
  np.testing.assert_array_equal(ps_d[1], ps_h[1])


def test_the_coverage_run_on_the_device():
  """the host tests' run with every handover cause, an auto-reset and a held object (tests/test_tabletop3_pair.py), on the device"""
  for head in ('deterministic', 'sample_clamp'):
    (got, ps_d, _, hd), (want, ps_h, _, hh) = coverage_run(GPU, head), coverage_run(CPU, head)
    hold_to_host(f'coverage {head}', got, want, keys_of(HEADS[head]) + ('agent', 'fs', 'bs'))
    assert_same_state(final_state(hd), final_state(hh))
    np.testing.assert_array_equal(ps_d.host()[0], ps_h.host()[0])
    np.testing.assert_array_equal(ps_d.host()[1], ps_h.host()[1])
    assert got['fs'].sum() > 0 and got['bs'].sum() > 0 and got['done'].any() and (got['obs'][..., 8] >= 0).any()


# ---------------------------------------------------------------------------------------------------------------- 11. lane maps against an exact reference
@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian-mean'])
@pytest.mark.parametrize('hidden', WIDEST, ids=IDS)
def test_lane_maps_against_an_exact_integer_reference_at_the_widest_shapes(hidden, gaussian):
  """ReLU hidden layers, no output activation, weights in {-1, 0, 1} that differ between the two agents and have no symmetry in (n, k), integer biases in [-3, 3],
  observations that are multiples of 0.5 with |x| <= 3: every product and partial sum is exact in float32 (|layer 0| <= 63, |layer 1| <= 16131, |output| <=
  2.1e6 = 4.2e6 half-units < 2^24), so the reference is numpy float64 in any order, and a wrong LDS index of the output or layer-0 image, a permuted k-step, a dropped
  tile or a swap of the agents' images changes an integer.  Random phases: every workgroup runs both networks"""
  nout = 6 if gaussian else 3
  dims = [p3.OBS] + list(hidden) + [nout]
  layers = []
  for ag in range(2):
    rng = np.random.default_rng(sum(hidden) + 1000 * ag)
    layers.append([(rng.integers(-1, 2, (n, k)).astype(np.float32), rng.integers(-3, 4, n).astype(np.float32)) for k, n in zip(dims[:-1], dims[1:])])
  assert all((a[0] != b[0]).mean() > 0.5 for a, b in zip(*layers))
  pr = Pair3(gaussian=gaussian, device=GPU, members=[Packed(l, 'relu', 'none', GPU) for l in layers])
  goals = np.random.default_rng(2).integers(-6, 7, size=(4, 10)) / 2.0
  back = np.random.default_rng(4).integers(-6, 7, size=10) / 2.0
  d = t3.harness(GPU, reward_type='sparse', horizon=5, seed=1, goal_table=goals, n_sample_goals=4)
  d.reset()
  q = np.random.default_rng(3).integers(-4, 5, size=(N, 8)) / 2.0          # different rows of half-integers in [-2, 2]
  gi = (np.arange(N) % 4).astype(np.int32)
  phase = np.random.default_rng(6).integers(0, 2, N).astype(np.int8)
  d.qpos.copy_(torch.tensor(q))
  d.goal_idx.copy_(torch.tensor(gi))
  x = np.concatenate([q, np.full((N, 2), -1.0), np.where(phase[:, None] == 1, back[None], goals[gi])], axis=1)      # _get_obs with the goal in force
  assert x.shape == (N, p3.OBS) and (np.abs(x) <= 3).all() and len(np.unique(x, axis=0)) == N
  want, biggest = np.zeros((N, 3)), 0.0
  for ag in range(2):
    v = x
    for l, (w, b) in enumerate(layers[ag]):
      v = v @ w.astype(np.float64).T + b.astype(np.float64)
      biggest = max(biggest, float(np.abs(v).max()))
      if l + 1 < len(layers[ag]):
        v = np.maximum(v, 0)
    want[phase == ag] = v[phase == ag, :3]
  assert biggest < 2 ** 23 and (want != 0).any() and len(np.unique(want, axis=0)) > N // 2
  ps = PairState(N, device=GPU, phase=phase)
  got = pair_rollout3(d, pr, ps, 1, 1, False, 10, 0, backward_goal=back, head=dict(mode='mean') if gaussian else None)
  np.testing.assert_array_equal(got['agent'][0], phase)
  act = got['act'][0].astype(np.float64)
  if not np.array_equal(act, want):
    bad = np.argwhere(act != want)
    i, j = bad[0]
    raise AssertionError(f'{hidden}: {len(bad)} of {act.size} actions differ; first at env {i} (agent {phase[i]}) action {j}: device {act[i, j]!r} exact {want[i, j]!r}')


# ---------------------------------------------------------------------------------------------------------------- 12. the parked state at NT2 = 2
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('hidden', [(16, 80), (256, 128)], ids=IDS)
def test_the_state_parked_in_lds_survives_a_handover_at_every_step_with_auto_reset(hidden, head):
  """NT2 = 2 keeps q[8] and g[10] of the env lanes in LDS while the networks run: with switch_every = (1, 1) the goal in force changes at every step, and horizon 7
  resets every env inside the launch, so a stale or unrestored copy shows in qpos, attached or goal_idx left behind"""
  Tn = 24
  runs = []
  for dev in (GPU, CPU):
    h = p3.prepared(dev, False, reward_type='sparse', seed=13, auto_reset=True, horizon=7)
    rng = np.random.default_rng(1)
    ps = PairState(N, device=dev, phase=rng.integers(0, 2, N), sip=np.zeros(N))
    pr = Pair3(hidden, gaussian=HEADS[head] is not None, hidden_act='tanh', seed0=8, device=dev)
    got = pair_rollout3(h, pr, ps, 1, Tn, False, (1, 1), 1, backward_goal=INITIAL3, head=HEADS[head])
    runs.append((got, final_state(h), ps.host()))
  (got, end_d, ps_d), (want, end_h, ps_h) = runs
  assert want['done'].any() and ((want['agent'][1:] != want['agent'][:-1]) | want['done'][:-1].astype(bool)).all()
  for k in ('qpos', 'attached', 'goal_idx'):
    np.testing.assert_array_equal(end_d[0][k].view(np.uint8), end_h[0][k].view(np.uint8), err_msg=k)
  hold_to_host(f'parked {hidden} {head}', got, want, keys_of(HEADS[head]) + ('agent', 'fs', 'bs'))
  assert_same_state(end_d, end_h)
  np.testing.assert_array_equal(ps_d[0], ps_h[0])
  np.testing.assert_array_equal(ps_d[1], ps_h[1])
  assert len(np.unique(end_h[0]['goal_idx'])) > 1


# ---------------------------------------------------------------------------------------------------------------- 13. never switching, shards, split launches, NULLs
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('hidden', [(80,), (48, 16), (256, 128)], ids=IDS)
def test_never_switching_equals_the_single_policy_launch_on_the_device(hidden, head, form):
  E, reset_first, cfg_kw = FORMS[form]
  pr = Pair3(hidden, gaussian=HEADS[head] is not None, hidden_act='tanh', seed0=9, device=GPU)
  d = p3.prepared(GPU, reset_first, reward_type='dense', reset_at_goal=True, seed=5, **cfg_kw)
  snap = snapshot(d)
  ps = PairState(N, device=GPU)
  got = pair_rollout3(d, pr, ps, E, T, reset_first, T + 1, 0, head=HEADS[head])
  end = final_state(d)
  assert not np.isnan(got['act']).any() and (got['agent'] == 0).all()
  restore(d, snap)
  want = single_rollout3(d, pr.members[0], E, T, reset_first, head=HEADS[head])
  assert_bits(got, want, keys_of(HEADS[head]))
  assert_same_state(end, final_state(d))


@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('hidden', [(64,), (32, 112)], ids=IDS)
def test_shards_equal_the_batch_and_two_launches_equal_one_on_the_device(hidden, head):
  T1, T2 = 11, 13
  kw = dict(reward_type='sparse', reset_at_goal=True, seed=21, auto_reset=True, horizon=7)
  pr = Pair3(hidden, gaussian=HEADS[head] is not None, seed0=5, device=GPU)
  args = dict(switch_every=(4, 3), switch_on_success=1, backward_goal=INITIAL3, head=HEADS[head])
  whole = p3.prepared(GPU, False, **kw)
  snap = snapshot(whole)
  ps = PairState(N, device=GPU)
  got = pair_rollout3(whole, pr, ps, 1, T1 + T2, False, **args)
  end = final_state(whole)
  keys = keys_of(HEADS[head]) + ('agent',)
  restore(whole, snap)
  ps2 = PairState(N, device=GPU)
  a = pair_rollout3(whole, pr, ps2, 1, T1, False, **args)
  b = pair_rollout3(whole, pr, ps2, 1, T2, False, **args)
  assert_bits({k: np.concatenate([a[k], b[k]], axis=0) for k in keys}, got, keys)
  np.testing.assert_array_equal(a['fs'] + b['fs'], got['fs'])
  np.testing.assert_array_equal(a['bs'] + b['bs'], got['bs'])
  assert_same_state(final_state(whole), end)
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])
  np.testing.assert_array_equal(ps2.host()[1], ps.host()[1])
  parts, states, pss = [], [], []
  for i0, m in ((0, 25), (25, 15)):                           # the cut is inside a workgroup of the batch
    hs = p3.harness(GPU, n=m, env_offset=OFFSET + i0, **kw)
    for k, v in snap[0].items():
      getattr(hs, k).copy_(v[i0:i0 + m])
    hs.cfg.counter = snap[1]
    p = PairState(m, device=GPU)
    parts.append(pair_rollout3(hs, pr, p, 1, T1 + T2, False, **args))
    states.append(final_state(hs))
    pss.append(p.host())
  assert_bits({k: np.concatenate([p[k] for p in parts], axis=1) for k in keys + ('fs', 'bs')}, got, keys + ('fs', 'bs'))
  for k in end[0]:
    np.testing.assert_array_equal(np.concatenate([s[0][k] for s in states], axis=0).view(np.uint8), end[0][k].view(np.uint8), err_msg=k)
  np.testing.assert_array_equal(np.concatenate([p[0] for p in pss]), ps.host()[0])
  np.testing.assert_array_equal(np.concatenate([p[1] for p in pss]), ps.host()[1])


def test_null_outputs_leave_the_state_what_it_was_on_the_device():
  Tn = 16
  kw = dict(reward_type='sparse', reset_at_goal=True, seed=2, horizon=10**6)
  pr = Pair3((64, 128), gaussian=True, seed0=1, device=GPU)
  args = dict(switch_every=(4, 3), switch_on_success=1, backward_goal=INITIAL3, head=HEADS['sample_clamp'])
  d = p3.prepared(GPU, False, **kw)
  snap = snapshot(d)
  ps = PairState(N, device=GPU)
  pair_rollout3(d, pr, ps, 1, Tn, False, **args)
  end = final_state(d)
  restore(d, snap)
  ps2 = PairState(N, device=GPU)
  bare = pair_rollout3(d, pr, ps2, 1, Tn, False, null=OUT + ('act', 'eps', 'agent', 'fs', 'bs'), **args)
  for k in OUT + ('act', 'eps'):
    assert np.isnan(bare[k]).all() if bare[k].dtype == np.float32 else (bare[k] == 7).all()
  assert (bare['agent'] == 7).all() and (bare['fs'] == -7).all() and (bare['bs'] == -7).all()
  assert_same_state(end, final_state(d))
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])
  np.testing.assert_array_equal(ps2.host()[1], ps.host()[1])


# ---------------------------------------------------------------------------------------------------------------- 14. banded buffers
OPTIONAL = ('obs', 'reward', 'done', 'success', 'act', 'eps', 'agent', 'fs', 'bs')


def run_banded(side, sc, net, E, Tn, reset_first, fill, pair, head=None, null=(), n_call=None):
  """earl_tabletop3_pair_rollout on banded buffers (tests/tabletop_abi.py: Run) -> (results, Bands); names in `null` are passed as NULL"""
  n = sc.n
  lead = (E, Tn, n) if reset_first else (Tn, n)
  r = A.Run(side, fill, null)
  st = r.state(sc)
  params = r.put('in.params', net.params)
  ps = net.struct
  pol = _abi.MlpPolicy(n_layers=ps.n_layers, dims=ps.dims, hidden_act=ps.hidden_act, out_act=ps.out_act, precision=0, params=params.data_ptr())
  out = r.out(lead, p3.OBS)
  r.blank('out.act', lead + (3,), torch.float32, n * 3)
  hd = None
  if head is not None:
    r.blank('out.eps', lead + (3,), torch.float32, n * 3)
    hd = _abi.GaussianHead(mode=1, log_std_map=1, log_std_min=-5.0, log_std_max=2.0, eps_out=r.ptr('out.eps'))
  r.put('st.phase', np.asarray(pair['phase'], np.int8))
  r.put('st.sip', np.asarray(pair['sip'], np.int32))
  r.put('in.backward_goal', pair.get('backward_goal'))
  r.blank('out.agent', lead, torch.int8, n)
  r.blank('out.fs', (E, n), torch.int32, n)
  r.blank('out.bs', (E, n), torch.int32, n)
  pst = _abi.AgentPair(switch_every=(C.c_int32 * 2)(*pair['switch_every']), switch_on_success=int(pair['switch_on_success']), pad_=0,
                       param_stride=net.params.shape[1], backward_goal=r.ptr('in.backward_goal'), phase=r.ptr('st.phase'), steps_in_phase=r.ptr('st.sip'),
                       agent_out=r.ptr('out.agent'), forward_success=r.ptr('out.fs'), backward_success=r.ptr('out.bs'))
  cfg = sc.cfg() if n_call is None else sc.cfg(n=n_call)
  rc = side.lib.earl_tabletop3_pair_rollout(C.byref(cfg), C.byref(st), C.byref(pol), C.byref(pst), None if hd is None else C.byref(hd), E, Tn, int(reset_first),
                                            C.byref(out), r.ptr('out.act'), side.stream)
  return r.finish(rc, 'tabletop3_pair_rollout')


@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'sample'])
@pytest.mark.parametrize('form', ['evaluation', 'auto_reset'])
def test_banded_buffers_optional_pointers_and_the_empty_batch(form, gaussian):
  E, reset_first, cfg_kw = FORMS[form]
  sc = A.Scene(N, nobj=3, reward_type='sparse', reset_at_goal=True, seed=3, env_offset=OFFSET, **cfg_kw)
  net = Pair3((48, 80), gaussian=gaussian, seed0=5)
  rng = np.random.default_rng(2)
  pair = dict(switch_every=(3, 2), switch_on_success=1, phase=rng.integers(0, 2, size=N), sip=rng.integers(0, 2, size=N), backward_goal=INITIAL3)
  head = {} if gaussian else None
  dev, host = A.Side(GPU), A.Side(CPU)
  full = A.both_fills(run_banded, dev, sc, net, E, T, reset_first, pair=pair, head=head, what=f'{form} all outputs')
  want, _ = run_banded(host, sc, net, E, T, reset_first, A.FILLS[0], pair=pair, head=head)
  A.agree(full, want, f'{form}: device vs host twin')
  for name in OPTIONAL:                                                 # every optional pointer NULL in turn: the others, and the state, unchanged
    if name == 'eps' and not gaussian:
      continue
    res = A.both_fills(run_banded, dev, sc, net, E, T, reset_first, pair=pair, head=head, what=f'{form} without {name}', null=(name,))
    A.agree(res, full, f'{form} without {name}', null=(name,))
  nogoal = dict(pair, backward_goal=None)                               # the backward goal is optional too
  res = A.both_fills(run_banded, dev, sc, net, E, T, reset_first, pair=nogoal, head=head, what=f'{form} without a backward goal')
  want0, _ = run_banded(host, sc, net, E, T, reset_first, A.FILLS[0], pair=nogoal, head=head)
  A.agree(res, want0, f'{form} without a backward goal: device vs host twin')
  for fill in A.FILLS:                                                  # n = 0: EARL_OK, nothing written
    res, b = run_banded(dev, sc, net, E, T, reset_first, fill, pair=pair, head=head, n_call=0)
    b.check(f'{form} n = 0')
    A.assert_untouched(res, sc, f'{form} n = 0')


# ---------------------------------------------------------------------------------------------------------------- 15. the Python surface
@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian'])
def test_rollout_agents_on_cuda_equals_the_same_call_on_the_host(gaussian):
  from earl_benchmark_amd.policy import AgentPair
  from test_tabletop3_pair import agents_of, env3
  _, agents = agents_of(gaussian)
  pair_h = AgentPair(agents[0], agents[1], switch_every=(4, 3), obs_dim=20, act_dim=3)
  pair_d = AgentPair(agents[0], agents[1], switch_every=(4, 3), obs_dim=20, act_dim=3, device=GPU)
  assert pair_d.params.is_cuda and torch.equal(pair_d.params.cpu(), pair_h.params)
  env_d, env_h = env3(GPU), env3(CPU)
  env_d.reset()
  env_h.reset()
  extra = dict(return_noise=True) if gaussian else {}
  for _ in range(2):                                          # the second launch continues from the pair state the first left on the device
    outs, want = env_d.rollout_agents(pair_d, 20, **extra), env_h.rollout_agents(pair_h, 20, **extra)
    for a, b in zip(outs, want):
      assert a.is_cuda and tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(env_d.agent_phase.cpu(), env_h.agent_phase) and torch.equal(env_d.steps_in_phase.cpu(), env_h.steps_in_phase)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(env_d.pair_counts, env_h.pair_counts)) and torch.equal(env_d.goal_idx.cpu(), env_h.goal_idx)
    assert 0 < float(outs[5].float().mean()) < 1
  assert env_d._cfg.counter == env_h._cfg.counter
  o2, w2 = env_d.rollout_agents(pair_d, 6, episodes=2, reset_first=True), env_h.rollout_agents(pair_h, 6, episodes=2, reset_first=True)
  assert all(torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8)) for a, b in zip(o2, w2))
  with pytest.raises(ValueError):
    env_d.rollout_agents(pair_h, 6)

"""earl_tabletop_pair_rollout on the MI355X: the pair kernel (csrc/tabletop_policy_pair.hip: both agents' weights in registers, the per-step ballot of the phase, the
uniform and the mixed path) held to its host twin bit for bit on inputs that take all three paths, to the open-loop kernels, to itself across shards and split
launches, and the Python surface on the device.
The width matrix of the pair kernel (every width it takes, its 6 instantiations) lives in tests/test_policy_widths_gpu.py."""
import numpy as np
import pytest
import torch

import hip_harness as hx
from pair_helpers import INITIAL, OUT, Pair, PairState, assert_bits, pair_rollout, workgroup_shares
from test_policy_pair import FORMS, HEADS, OFFSET, keys_of, prepared
from test_policy_rollout import Policy, assert_same_bits, assert_same_state, final_state, open_loop, restore, snapshot

pytestmark = pytest.mark.gpu
GPU, CPU = 'cuda:0', 'cpu'
SHAPES = {'NT2=0': (64,), 'NT2=1': (48, 32), 'NT2=2': (64, 128)}          # every shipped class of the hidden -> hidden layer


def initial_phase(n, seed=0):
  """workgroups (16 consecutive envs) alternately all-forward, all-reset and random, the random ones with random clocks: with fixed clocks the first two kinds stay
  uniform until a success, the third is mixed from the first step on"""
  rng = np.random.default_rng(seed)
  ph, sip = rng.integers(0, 2, n), rng.integers(0, 4, n)
  wg = np.arange(n) // 16
  ph[wg % 3 == 0], ph[wg % 3 == 1] = 0, 1
  sip[wg % 3 != 2] = 0
  return ph.astype(np.int8), sip.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- 11. device = host twin
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('goal', [None, 'initial'])
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('hact', ['relu', 'tanh'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_device_equals_host_twin_bit_for_bit_on_all_three_paths(shape, hact, head, goal, form):
  E, reset_first, cfg_kw = FORMS[form]
  T, se = 40, (7, 5)
  cfg_kw = dict(cfg_kw, horizon=T) if form == 'evaluation' else cfg_kw
  counts = np.zeros(3)
  for n in (1, 16, 100, 4096, 5000):
    kw = dict(reward_type='sparse', reset_at_goal=True, wide_init=True, seed=9, env_offset=OFFSET, **cfg_kw)
    args = dict(gaussian=HEADS[head] is not None, hidden_act=hact, seed0=4)
    pd, ph = Pair(SHAPES[shape], device=GPU, **args), Pair(SHAPES[shape], device=CPU, **args)
    d, h = prepared(n, reset_first, device=GPU, **kw), prepared(n, reset_first, device=CPU, **kw)
    p0, s0 = initial_phase(n)
    psd, psh = PairState(n, device=GPU, phase=p0, sip=s0), PairState(n, device=CPU, phase=p0, sip=s0)
    run = dict(switch_every=se, switch_on_success=1, backward_goal=None if goal is None else INITIAL, head=HEADS[head])
    got = pair_rollout(d, pd, psd, E, T, reset_first, **run)
    want = pair_rollout(h, ph, psh, E, T, reset_first, **run)
    if not np.array_equal(got['act'].view(np.uint32), want['act'].view(np.uint32)):
      bad = np.argwhere(got['act'].view(np.uint32) != want['act'].view(np.uint32))
      raise AssertionError(f'{shape} {hact} {head} {form} n={n}: {len(bad)} of {want["act"].size} actions differ; first at {tuple(bad[0])}: device '
                           f'{got["act"][tuple(bad[0])]!r} host {want["act"][tuple(bad[0])]!r}, agent {want["agent"][tuple(bad[0][:-1])]}')
    assert_bits(got, want, keys_of(HEADS[head]) + ('agent', 'fs', 'bs'))
    assert_same_state(final_state(d), final_state(h))
    np.testing.assert_array_equal(psd.host()[0], psh.host()[0])
    np.testing.assert_array_equal(psd.host()[1], psh.host()[1])
    counts += np.array(workgroup_shares(got['agent'])) * ((n + 15) // 16 * E * T)
  share = counts / counts.sum()
  print(f'{shape} {hact} {head} goal={goal} {form}: (workgroup, step) pairs mixed {share[0]:.4f}, uniform-forward {share[1]:.4f}, uniform-reset {share[2]:.4f}')
  assert (share >= 0.01).all(), share


# ---------------------------------------------------------------------------------------------------------------- 12. closed = open, shards, split launches
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_never_switching_launch_equals_the_open_loop_rollout_fed_with_its_actions(head, form):
  E, reset_first, cfg_kw = FORMS[form]
  n, T = 1000, 60
  kw = dict(reward_type='dense', seed=5, env_offset=OFFSET, **cfg_kw)
  pr = Pair((48, 32), gaussian=HEADS[head] is not None, hidden_act='tanh', seed0=9, device=GPU)
  d = prepared(n, reset_first, device=GPU, **kw)
  snap = snapshot(d)
  ps = PairState(n, device=GPU)
  got = pair_rollout(d, pr, ps, E, T, reset_first, T + 1, 0, head=HEADS[head])
  end = final_state(d)
  assert not np.isnan(got['act']).any() and (got['agent'] == 0).all()
  restore(d, snap)
  want = open_loop(d, got['act'], reset_first)
  assert_same_bits(got, want)
  assert_same_state(end, final_state(d))


@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_shards_equal_the_batch_and_two_launches_equal_one_on_the_device(head):
  n, T1, T2 = 100, 23, 31
  kw = dict(reward_type='sparse', reset_at_goal=True, wide_init=True, seed=21, horizon=10**6)
  pr = Pair((64,), gaussian=HEADS[head] is not None, seed0=5, device=GPU)
  args = dict(switch_every=(7, 5), switch_on_success=1, backward_goal=INITIAL, head=HEADS[head])
  whole = prepared(n, False, device=GPU, env_offset=OFFSET, **kw)
  snap = snapshot(whole)
  ps = PairState(n, device=GPU)
  got = pair_rollout(whole, pr, ps, 1, T1 + T2, False, **args)
  end = final_state(whole)
  keys = keys_of(HEADS[head]) + ('agent',)
  restore(whole, snap)
  ps2 = PairState(n, device=GPU)
  a = pair_rollout(whole, pr, ps2, 1, T1, False, **args)
  b = pair_rollout(whole, pr, ps2, 1, T2, False, **args)
  assert_bits({k: np.concatenate([a[k], b[k]], axis=0) for k in keys}, got, keys)
  np.testing.assert_array_equal(a['fs'] + b['fs'], got['fs'])
  np.testing.assert_array_equal(a['bs'] + b['bs'], got['bs'])
  assert_same_state(final_state(whole), end)
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])
  np.testing.assert_array_equal(ps2.host()[1], ps.host()[1])
  parts, states, pss = [], [], []
  for i0, m in ((0, 60), (60, 40)):                           # the cut is inside a workgroup of the batch
    hs = hx.HipTabletop(m, device=GPU, env_offset=OFFSET + i0, **kw)
    for k, v in snap[0].items():
      getattr(hs, k).copy_(v[i0:i0 + m])
    hs.cfg.counter = snap[1]
    p = PairState(m, device=GPU)
    parts.append(pair_rollout(hs, pr, p, 1, T1 + T2, False, **args))
    states.append(final_state(hs))
    pss.append(p.host())
  assert_bits({k: np.concatenate([p[k] for p in parts], axis=1) for k in keys + ('fs', 'bs')}, got, keys + ('fs', 'bs'))
  for k in end[0]:
    np.testing.assert_array_equal(np.concatenate([s[0][k] for s in states], axis=0).view(np.uint8), end[0][k].view(np.uint8), err_msg=k)
  np.testing.assert_array_equal(np.concatenate([p[0] for p in pss]), ps.host()[0])
  np.testing.assert_array_equal(np.concatenate([p[1] for p in pss]), ps.host()[1])


def test_null_outputs_leave_the_state_what_it_was_on_the_device():
  n, T = 1000, 30
  kw = dict(reward_type='sparse', reset_at_goal=True, wide_init=True, seed=2, env_offset=OFFSET, horizon=10**6)
  pr = Pair((64, 128), gaussian=True, seed0=1, device=GPU)
  args = dict(switch_every=(7, 5), switch_on_success=1, backward_goal=INITIAL, head=HEADS['sample_clamp'])
  d = prepared(n, False, device=GPU, **kw)
  snap = snapshot(d)
  ps = PairState(n, device=GPU)
  pair_rollout(d, pr, ps, 1, T, False, **args)
  end = final_state(d)
  restore(d, snap)
  ps2 = PairState(n, device=GPU)
  bare = pair_rollout(d, pr, ps2, 1, T, False, null=OUT + ('act', 'eps', 'agent', 'fs', 'bs'), **args)
  for k in OUT + ('act', 'eps'):
    assert np.isnan(bare[k]).all() if bare[k].dtype == np.float32 else (bare[k] == 7).all()
  assert (bare['agent'] == 7).all() and (bare['fs'] == -7).all()
  assert_same_state(end, final_state(d))
  np.testing.assert_array_equal(ps2.host()[0], ps.host()[0])


# ---------------------------------------------------------------------------------------------------------------- 13. the Python surface
@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian'])
def test_rollout_agents_on_cuda_equals_the_same_call_on_the_host(gaussian):
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy
  from gaussian_policy_helpers import GaussPolicy
  if gaussian:
    agents = [GaussianMLPPolicy(GaussPolicy((48, 32), seed=s, log_std_gain=1.0).layers, 'relu') for s in range(2)]
  else:
    agents = [MLPPolicy(Policy((48, 32), seed=s).layers, 'relu', 'tanh') for s in range(2)]
  pair_h = AgentPair(agents[0], agents[1], switch_every=(7, 5))
  pair_d = AgentPair(agents[0], agents[1], switch_every=(7, 5), device=GPU)
  assert pair_d.params.is_cuda and pair_d.device == torch.device(GPU) and torch.equal(pair_d.params.cpu(), pair_h.params)
  n, T = 500, 60
  kw = dict(reward_type='sparse', reset_train_env_at_goal=True, wide_init_distr=True, num_envs=n, seed=3, env_offset=OFFSET)
  env_d, _ = eb.EARLEnvs('tabletop_manipulation', device=GPU, **kw).get_envs()
  env_h, _ = eb.EARLEnvs('tabletop_manipulation', device=CPU, **kw).get_envs()
  extra = dict(return_noise=True) if gaussian else {}
  for _ in range(2):                                          # the second launch continues from the pair state the first left on the device
    outs, want = env_d.rollout_agents(pair_d, T, **extra), env_h.rollout_agents(pair_h, T, **extra)
    for a, b in zip(outs, want):
      assert a.is_cuda and tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8))
    ud, uh = env_d.unwrapped, env_h.unwrapped
    assert torch.equal(ud.agent_phase.cpu(), uh.agent_phase) and torch.equal(ud.steps_in_phase.cpu(), uh.steps_in_phase)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(ud.pair_counts, uh.pair_counts)) and torch.equal(ud.goal_idx.cpu(), uh.goal_idx)
    assert 0 < float(outs[5].float().mean()) < 1
  assert env_d.total_steps == 2 * T and env_d.unwrapped._cfg.counter == env_h.unwrapped._cfg.counter
  o2, w2 = env_d.rollout_agents(pair_d, 20, episodes=2, reset_first=True), env_h.rollout_agents(pair_h, 20, episodes=2, reset_first=True)
  assert all(torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8)) for a, b in zip(o2, w2))
  if not gaussian:
    torch.testing.assert_close(pair_d(outs[0][:-1], outs[5][1:]), outs[4][1:], rtol=1e-4, atol=1e-4)
  with pytest.raises(ValueError):
    env_d.rollout_agents(pair_h, T)

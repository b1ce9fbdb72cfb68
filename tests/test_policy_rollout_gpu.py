"""earl_tabletop_policy_rollout on the MI355X: the kernel of csrc/tabletop_policy.h (v_mfma_f32_16x16x4_f32 beside the fp64 recurrence) held to its host
twin bit for bit -- the test of the MFMA lane maps, of the k order of the accumulation and of tanh_f32 on the device -- and to the open-loop kernels.
The width and instantiation matrix (every hidden width, every NT2 x GENERAL instantiation) lives in tests/test_policy_widths_gpu.py."""
import numpy as np
import pytest
import torch

import hip_harness as hx
from test_policy_rollout import (Policy, assert_same_bits, assert_same_state, closed_equals_open, final_state, policy_rollout, restore, snapshot)

pytestmark = pytest.mark.gpu
GPU, CPU = 'cuda:0', 'cpu'


def twin(n, **kw):
  return hx.HipTabletop(n, device=GPU, **kw), hx.HipTabletop(n, device=CPU, **kw)


# ---------------------------------------------------------------------------------------------------------------- 7. device = host
@pytest.mark.parametrize('oact', ['tanh', 'none'])
@pytest.mark.parametrize('hact', ['relu', 'tanh'])
@pytest.mark.parametrize('hidden', [(16,), (64,), (48, 32), (256, 256)], ids=str)
def test_device_equals_host_bit_for_bit(hidden, hact, oact):
  T = 40 if hidden == (256, 256) else 200
  seed = len(hidden) * 100 + hidden[0] + (hact == 'tanh') * 7 + (oact == 'tanh') * 13
  for n in (1, 16, 100, 4096, 5000):
    kw = dict(reward_type='sparse', wide_init=n == 100, horizon=T, seed=seed, env_offset=3)
    d, h = twin(n, **kw)
    pd, ph = Policy(hidden, hact, oact, seed=seed, device=GPU), Policy(hidden, hact, oact, seed=seed, device=CPU)
    got, want = policy_rollout(d, pd, 2, T, True), policy_rollout(h, ph, 2, T, True)
    a = np.abs(want['act'])
    if n >= 100:                                             # some actions saturate the env's clip (tanh output: its own saturation), some do not
      assert ((a > 1).any() if oact == 'none' else (a > 0.99).any()) and (a < 0.5).any()
    if not np.array_equal(got['act'].view(np.uint32), want['act'].view(np.uint32)):
      bad = np.argwhere(got['act'].view(np.uint32) != want['act'].view(np.uint32))
      e, t, i, j = bad[0]
      raise AssertionError(f'{hidden} {hact}/{oact} n={n}: {len(bad)} of {a.size} actions differ; first at episode {e} step {t} env {i} action {j}: '
                           f'device {got["act"][e, t, i, j]!r} host {want["act"][e, t, i, j]!r}')
    assert_same_bits(got, want)
    assert_same_state(final_state(d), final_state(h))


def test_identity_activation_path_against_an_asymmetric_matrix():
  """the guide's lane-map check: out_act none, ReLU on a positive chain is the identity -- weights W0[j][k] = 1 + j + 20 k and W1[j][k] = 1 + j + 3 k are asymmetric in (j, k), and with
  observations that are multiples of 0.5 every product and partial sum is exact in float32 (below 2^24 half-units), so a swapped row/column or a permuted k shows as a wrong INTEGER, not as a rounding difference"""
  n, T = 16, 1
  pol = Policy((16,), 'relu', 'none', seed=0, device=GPU)
  w0 = np.array([[1 + j + 20 * k for k in range(12)] for j in range(16)], np.float32)
  w1 = np.array([[1 + j + 3 * k for k in range(16)] for j in range(3)], np.float32)
  flat = np.concatenate([w0.reshape(-1), np.arange(16, dtype=np.float32), w1.reshape(-1), np.zeros(3, np.float32)])
  pol.params.copy_(torch.tensor(flat))
  d = hx.HipTabletop(n, device=GPU, horizon=5, seed=1)
  d.reset()
  q = (np.arange(n * 4).reshape(n, 4) % 5 - 2).astype(np.float64)          # small integers (the goal rows add -2.5)
  d.qpos.copy_(torch.tensor(q))
  x = d.observe()[0].astype(np.float64)
  assert (2 * x == np.round(2 * x)).all() and (np.abs(x) <= 3).all()
  hdn = x @ w0.astype(np.float64).T + np.arange(16)
  want = np.maximum(hdn, 0) @ w1.astype(np.float64).T
  got = policy_rollout(d, pol, 1, T, False)
  np.testing.assert_array_equal(got['act'][0].astype(np.float64), want)


# ---------------------------------------------------------------------------------------------------------------- 8. closed = open on the device
@pytest.mark.parametrize('T', [200, 37])
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('wide', [False, True])
def test_closed_equals_open_on_the_device_evaluation_form(T, rt, wide):
  pol = Policy((64,), seed=T, device=GPU)
  closed_equals_open(GPU, pol, 1000, 3, T, True, reward_type=rt, wide_init=wide, horizon=T)


@pytest.mark.parametrize('kw', [dict(goal_change_frequency=50, horizon=10**6), dict(auto_reset=True, horizon=13), dict(horizon=10**6)], ids=['lifelong', 'auto_reset', 'plain'])
def test_closed_equals_open_on_the_device_continuing_form(kw):
  pol = Policy((48, 32), hidden_act='tanh', seed=3, device=GPU)
  closed_equals_open(GPU, pol, 1000, 1, 200, False, reward_type='dense', **kw)


# ---------------------------------------------------------------------------------------------------------------- 9. shards, repeats, NULLs, the Python surface
def test_two_shards_equal_the_batch_and_two_launches_equal_each_other():
  n, T, E = 100, 64, 2
  kw = dict(reward_type='sparse', wide_init=True, horizon=T, seed=21)
  pol = Policy((64,), seed=5, device=GPU)
  whole = hx.HipTabletop(n, device=GPU, **kw)
  snap = snapshot(whole)
  got = policy_rollout(whole, pol, E, T, True)
  end = final_state(whole)
  restore(whole, snap)
  again = policy_rollout(whole, pol, E, T, True)
  assert_same_bits(got, again, ('obs', 'reward', 'done', 'success', 'act'))
  assert_same_state(end, final_state(whole))
  parts = [policy_rollout(hx.HipTabletop(m, device=GPU, env_offset=off, **kw), pol, E, T, True) for off, m in ((0, 60), (60, 40))]
  for k in ('obs', 'reward', 'done', 'success', 'act'):
    np.testing.assert_array_equal(np.concatenate([p[k] for p in parts], axis=2).view(np.uint8), got[k].view(np.uint8), err_msg=k)


def test_null_outputs_leave_the_others_unchanged():
  n, T = 100, 24
  kw = dict(reward_type='sparse', horizon=T, seed=2)
  pol = Policy((32,), seed=5, device=GPU)
  d = hx.HipTabletop(n, device=GPU, **kw)
  snap = snapshot(d)
  full = policy_rollout(d, pol, 1, T, True)
  end = final_state(d)
  for null in (('obs',), ('reward', 'done'), ('success', 'act'), ('obs', 'reward', 'done', 'success', 'act')):
    restore(d, snap)
    part = policy_rollout(d, pol, 1, T, True, null=null)
    assert_same_bits(part, full, [k for k in ('obs', 'reward', 'done', 'success', 'act') if k not in null])
    for k in null:                                     # (the harness's fill pattern: nothing was written)
      assert np.isnan(part[k]).all() if part[k].dtype == np.float32 else (part[k] == 7).all()
    assert_same_state(final_state(d), end)


def test_rollout_policy_through_the_loader_and_the_wrappers():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import MLPPolicy
  ref = Policy((64,), seed=6)
  pi = MLPPolicy(ref.layers, 'relu', 'tanh', device=GPU)
  n, T = 512, 40
  _, eval_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=GPU, seed=3).get_envs()
  _, host_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=CPU, seed=3).get_envs()
  outs = eval_env.rollout_policy(pi, T, episodes=2)
  want = host_env.rollout_policy(MLPPolicy(ref.layers, 'relu', 'tanh', device=CPU), T, episodes=2)
  for a, b in zip(outs, want):
    assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8))
  assert eval_env.total_steps == 2 * T and int(eval_env.num_interventions.sum()) == 2 * n
  assert eval_env.unwrapped._cfg.counter == host_env.unwrapped._cfg.counter
  # the same object serves the captured step loop: torch's matmul order, so close to the fused launch, not identical
  a_torch = pi(outs[0][0, 0])
  assert float((a_torch - outs[4][0, 1]).abs().max()) < 1e-5
  train_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', setup_as_lifelong_learning=True, num_envs=n, device=GPU, seed=3).get_envs()
  train_env.unwrapped._cfg.goal_change_frequency = 7
  train_env.reset()
  sd = train_env.unwrapped.state_dict()
  obs, rew, done, succ, act = train_env.rollout_policy(pi, T, reset_first=False)
  lret = train_env.lifelong_return.clone()
  train_env.unwrapped.load_state_dict(sd)
  o2, r2, d2, s2 = train_env.rollout(act)
  assert torch.equal(obs.view(torch.int32), o2.view(torch.int32)) and torch.equal(rew, r2) and torch.equal(lret, train_env.lifelong_return)
  with pytest.raises(ValueError):
    eval_env.rollout_policy(MLPPolicy(ref.layers, device=CPU), T)

"""earl_tabletop_policy_rollout_gaussian on the MI355X: the GAUSS instantiations of csrc/tabletop_policy.h's kernel held to the host twin bit for bit -- the test of
the lane = (env, dimension) hand-over through LDS, of the 6-column output tile and of the float32 sqrt and / of normal_quantile_f32 on the device -- and to the
open-loop kernels.
The width and instantiation matrix of the GAUSS instantiations lives in tests/test_policy_widths_gpu.py; the head's scalar functions are swept in tests/test_policy_math_gpu.py."""
import numpy as np
import pytest
import torch

import hip_harness as hx
from gaussian_policy_helpers import GaussPolicy, gaussian_closed_equals_open, gaussian_rollout
from test_policy_rollout import assert_same_bits, assert_same_state, final_state, restore, snapshot

pytestmark = pytest.mark.gpu
GPU, CPU = 'cuda:0', 'cpu'
KEYS = ('obs', 'reward', 'done', 'success', 'act', 'eps')


def device_equals_host(hidden, hact, oact, **head_kw):
  T = 40 if hidden == (256, 256) else 200
  seed = len(hidden) * 100 + hidden[0] + (hact == 'tanh') * 7 + (oact == 'tanh') * 13
  for n in (1, 16, 100, 4096, 5000):
    kw = dict(reward_type='sparse', wide_init=n == 100, horizon=T, seed=seed, env_offset=3)
    d, h = hx.HipTabletop(n, device=GPU, **kw), hx.HipTabletop(n, device=CPU, **kw)
    pd, ph = GaussPolicy(hidden, hact, oact, seed=seed, device=GPU), GaussPolicy(hidden, hact, oact, seed=seed, device=CPU)
    got, want = gaussian_rollout(d, pd, 2, T, True, **head_kw), gaussian_rollout(h, ph, 2, T, True, **head_kw)
    for k in ('eps', 'act'):                                 # the draws first: a difference there is the quantile's (sqrt, /), one in the actions alone the head's or the tile's
      if not np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)):
        bad = np.argwhere(got[k].view(np.uint32) != want[k].view(np.uint32))
        e, t, i, j = bad[0]
        raise AssertionError(f'{hidden} {hact}/{oact} {head_kw} n={n}: {len(bad)} of {want[k].size} values of {k} differ; first at episode {e} step {t} env {i} '
                             f'dimension {j}: device {got[k][e, t, i, j]!r} host {want[k][e, t, i, j]!r}')
    assert_same_bits(got, want, KEYS)
    assert_same_state(final_state(d), final_state(h))


# ---------------------------------------------------------------------------------------------------------------- 10. device = host
@pytest.mark.parametrize('oact', ['tanh', 'none'])
@pytest.mark.parametrize('hact', ['relu', 'tanh'])
@pytest.mark.parametrize('hidden', [(16,), (64,), (48, 32), (256, 256)], ids=str)
def test_device_equals_host_bit_for_bit_sampling_with_the_tanh_map(hidden, hact, oact):
  device_equals_host(hidden, hact, oact, mode='sample', log_std_map='tanh')


@pytest.mark.parametrize('head_kw', [dict(mode='sample', log_std_map='clamp'), dict(mode='mean', log_std_map='tanh')], ids=['clamp', 'mean'])
@pytest.mark.parametrize('hidden', [(64,), (48, 32)], ids=str)
def test_device_equals_host_bit_for_bit_clamp_map_and_mean_mode(hidden, head_kw):
  device_equals_host(hidden, 'relu', 'tanh' if hidden == (64,) else 'none', **head_kw)


# ---------------------------------------------------------------------------------------------------------------- 11. closed = open, shards, NULLs, the Python surface
def fresh(n, reset_first, **kw):
  h = hx.HipTabletop(n, device=GPU, seed=5, env_offset=2, **kw)
  h.reset()
  if not reset_first:
    h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, n, 3)).astype(np.float32))
  return h


@pytest.mark.parametrize('T', [200, 37])
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
def test_closed_equals_open_on_the_device_evaluation_form(T, rt):
  pol = GaussPolicy((64,), seed=T, device=GPU)
  gaussian_closed_equals_open(fresh(1000, True, reward_type=rt, wide_init=T == 37, horizon=T), pol, 3, T, True)


@pytest.mark.parametrize('kw', [dict(goal_change_frequency=50, horizon=10**6), dict(auto_reset=True, horizon=13), dict(horizon=10**6)], ids=['lifelong', 'auto_reset', 'plain'])
def test_closed_equals_open_on_the_device_continuing_form(kw):
  pol = GaussPolicy((48, 32), hidden_act='tanh', out_act='none', seed=3, device=GPU)
  gaussian_closed_equals_open(fresh(1000, False, reward_type='dense', **kw), pol, 1, 200, False, log_std_map='clamp')


def test_two_shards_equal_the_batch_and_two_launches_equal_each_other():
  n, T, E = 100, 64, 2
  kw = dict(reward_type='sparse', wide_init=True, horizon=T, seed=21)
  pol = GaussPolicy((64,), seed=5, device=GPU)
  whole = hx.HipTabletop(n, device=GPU, **kw)
  snap = snapshot(whole)
  got = gaussian_rollout(whole, pol, E, T, True)
  end = final_state(whole)
  restore(whole, snap)
  again = gaussian_rollout(whole, pol, E, T, True)
  assert_same_bits(got, again, KEYS)
  assert_same_state(end, final_state(whole))
  parts = [gaussian_rollout(hx.HipTabletop(m, device=GPU, env_offset=off, **kw), pol, E, T, True) for off, m in ((0, 60), (60, 40))]
  for k in KEYS:
    np.testing.assert_array_equal(np.concatenate([p[k] for p in parts], axis=2).view(np.uint8), got[k].view(np.uint8), err_msg=k)


def test_null_outputs_leave_the_others_unchanged():
  n, T = 100, 24
  kw = dict(reward_type='sparse', horizon=T, seed=2)
  pol = GaussPolicy((32,), seed=5, device=GPU)
  d = hx.HipTabletop(n, device=GPU, **kw)
  snap = snapshot(d)
  full = gaussian_rollout(d, pol, 1, T, True)
  end = final_state(d)
  for null in (('eps',), ('obs', 'eps'), ('reward', 'done'), ('success', 'act'), KEYS):
    restore(d, snap)
    part = gaussian_rollout(d, pol, 1, T, True, null=null)
    assert_same_bits(part, full, [k for k in KEYS if k not in null])
    for k in null:                                     # (the harness's fill pattern: nothing was written)
      assert np.isnan(part[k]).all() if part[k].dtype == np.float32 else (part[k] == 7).all()
    assert_same_state(final_state(d), end)


def test_rollout_policy_through_the_loader_and_the_wrappers():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import GaussianMLPPolicy
  ref = GaussPolicy((64,), seed=6, log_std_gain=1.0)
  pi = GaussianMLPPolicy(ref.layers, 'relu', device=GPU)
  ph = GaussianMLPPolicy(ref.layers, 'relu', device=CPU)
  n, T = 512, 40
  _, eval_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=GPU, seed=3).get_envs()
  _, host_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device=CPU, seed=3).get_envs()
  for kw in (dict(return_noise=True), dict(sample=False)):
    outs = eval_env.rollout_policy(pi, T, episodes=2, **kw)
    want = host_env.rollout_policy(ph, T, episodes=2, **kw)
    assert len(outs) == len(want) == (6 if 'return_noise' in kw else 5)
    for a, b in zip(outs, want):
      assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8))
    assert eval_env.unwrapped._cfg.counter == host_env.unwrapped._cfg.counter
  assert eval_env.total_steps == 4 * T and int(eval_env.num_interventions.sum()) == 4 * n
  outs = eval_env.rollout_policy(pi, T, episodes=1, return_noise=True)
  assert float((pi.sample(outs[0][0, 0], outs[5][0, 1]) - outs[4][0, 1]).abs().max()) < 1e-4           # torch's statement of the contract: close, not identical
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
    eval_env.rollout_policy(ph, T)

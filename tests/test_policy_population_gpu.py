"""earl_tabletop_population_rollout on the MI355X: the population kernel (csrc/tabletop_policy.h with POP: workgroups aligned to global env ids, per-workgroup
weights, summaries on the env lanes) held to its host twin bit for bit, to per-policy launches of the existing kernels, to the open-loop kernels, to itself
across shards and with its outputs switched off, and the Python surface on the device.
The width and instantiation matrix (all 20 population instantiations) lives in tests/test_policy_widths_gpu.py."""
import numpy as np
import pytest
import torch

import hip_harness as hx
from population_helpers import (OUT, SUMMARY, Population, assert_bits, members_needed, per_policy_launches, population_rollout, summary_by_definition)
from test_policy_population import FORMS, HEADS, OFFSET, prepared
from test_policy_rollout import Policy, assert_same_bits, assert_same_state, final_state, open_loop, restore, snapshot

pytestmark = pytest.mark.gpu
GPU, CPU = 'cuda:0', 'cpu'


def keys_of(head):
  return OUT + ('act',) + (('eps',) if HEADS[head] is not None else ()) + SUMMARY


# ---------------------------------------------------------------------------------------------------------------- 1. device = host
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
@pytest.mark.parametrize('G', [16, 64])
@pytest.mark.parametrize('hidden', [(16,), (64,), (48, 32), (256, 256)], ids=str)
def test_device_equals_host_bit_for_bit(hidden, G, head):
  T, E = (40 if hidden == (256, 256) else 200), 2
  for n in (1, 16, 100, 4096, 5000):
    kw = dict(reward_type='sparse', wide_init=n == 100, reset_at_goal=n == 4096, horizon=T, seed=len(hidden) * 100 + hidden[0] + G, env_offset=OFFSET)
    P = members_needed(OFFSET, n, G)
    args = dict(gaussian=HEADS[head] is not None, hidden_act='tanh' if hidden == (48, 32) else 'relu', seed0=7)
    pd, ph = Population(hidden, P, G, device=GPU, **args), Population(hidden, P, G, device=CPU, **args)
    d, h = prepared(n, True, device=GPU, **kw), prepared(n, True, device=CPU, **kw)
    got = population_rollout(d, pd.struct, pd.pop, E, T, True, head=HEADS[head])
    want = population_rollout(h, ph.struct, ph.pop, E, T, True, head=HEADS[head])
    if not np.array_equal(got['act'].view(np.uint32), want['act'].view(np.uint32)):
      bad = np.argwhere(got['act'].view(np.uint32) != want['act'].view(np.uint32))
      e, t, i, j = bad[0]
      raise AssertionError(f'{hidden} G={G} {head} n={n}: {len(bad)} of {want["act"].size} actions differ; first at episode {e} step {t} env {i} (member {(OFFSET + i) // G}) '
                           f'action {j}: device {got["act"][e, t, i, j]!r} host {want["act"][e, t, i, j]!r}')
    assert_bits(got, want, keys_of(head))
    assert_same_state(final_state(d), final_state(h))
    assert_bits(got, summary_by_definition(got['reward'], got['success']), SUMMARY)


@pytest.mark.parametrize('form', ['lifelong', 'auto_reset'])
def test_device_equals_host_in_the_continuing_form(form):
  E, reset_first, cfg_kw = FORMS[form]
  n, T, G = 1000, 200, 48
  kw = dict(reward_type='sparse', seed=12, env_offset=OFFSET, **cfg_kw)
  P = members_needed(OFFSET, n, G)
  pd, ph = Population((48, 32), P, G, gaussian=True, hidden_act='tanh', device=GPU), Population((48, 32), P, G, gaussian=True, hidden_act='tanh', device=CPU)
  d, h = prepared(n, False, device=GPU, **kw), prepared(n, False, device=CPU, **kw)
  got = population_rollout(d, pd.struct, pd.pop, E, T, False, head=HEADS['sample_clamp'])
  want = population_rollout(h, ph.struct, ph.pop, E, T, False, head=HEADS['sample_clamp'])
  assert_bits(got, want, keys_of('sample_clamp'))
  assert_same_state(final_state(d), final_state(h))


# ---------------------------------------------------------------------------------------------------------------- 2. population = per-policy launches
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh', 'mean'])
@pytest.mark.parametrize('hidden,G', [((64,), 16), ((48, 32), 48), ((256, 256), 16)], ids=str)
def test_population_equals_per_policy_launches_on_the_device(hidden, G, head):
  n, E, T = 100, 2, 40
  kw = dict(reward_type='dense', wide_init=True, horizon=T, seed=31)
  popn = Population(hidden, members_needed(OFFSET, n, G), G, gaussian=HEADS[head] is not None, seed0=2, device=GPU)
  d = prepared(n, True, device=GPU, env_offset=OFFSET, **kw)
  snap = snapshot(d)
  got = population_rollout(d, popn.struct, popn.pop, E, T, True, head=HEADS[head])
  end = final_state(d)
  want, want_state, want_counter = per_policy_launches(d, snap, popn, E, T, True, head=HEADS[head], **kw)
  assert_bits(got, want, OUT + ('act',) + (('eps',) if HEADS[head] is not None else ()))
  for k, v in want_state.items():
    np.testing.assert_array_equal(end[0][k].view(np.uint8), v.view(np.uint8), err_msg=k)
  assert end[1] == want_counter


# ---------------------------------------------------------------------------------------------------------------- 3. closed = open
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_closed_equals_open_on_the_device(head, form):
  E, reset_first, cfg_kw = FORMS[form]
  n, T, G = 1000, 60, 32
  kw = dict(reward_type='dense', seed=5, env_offset=OFFSET, **cfg_kw)
  popn = Population((64,), members_needed(OFFSET, n, G), G, gaussian=HEADS[head] is not None, seed0=9, device=GPU)
  d = prepared(n, reset_first, device=GPU, **kw)
  snap = snapshot(d)
  got = population_rollout(d, popn.struct, popn.pop, E, T, reset_first, head=HEADS[head])
  end = final_state(d)
  assert not np.isnan(got['act']).any()
  restore(d, snap)
  want = open_loop(d, got['act'], reset_first)
  assert_same_bits(got, want)
  assert_same_state(end, final_state(d))


# ---------------------------------------------------------------------------------------------------------------- 4. shards = batch
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_two_ragged_shards_equal_the_batch_on_the_device(head):
  E, T, G, n = 2, 64, 16, 100
  kw = dict(reward_type='sparse', wide_init=True, horizon=T, seed=21)
  popn = Population((64,), members_needed(OFFSET, n, G), G, gaussian=HEADS[head] is not None, seed0=5, device=GPU)
  whole = prepared(n, True, device=GPU, env_offset=OFFSET, **kw)
  snap = snapshot(whole)
  got = population_rollout(whole, popn.struct, popn.pop, E, T, True, head=HEADS[head])
  end = final_state(whole)
  parts, states = [], []
  for i0, m in ((0, 60), (60, 40)):                           # cut at global id 63: inside a member and inside a workgroup
    h = hx.HipTabletop(m, device=GPU, env_offset=OFFSET + i0, **kw)
    for k, v in snap[0].items():
      getattr(h, k).copy_(v[i0:i0 + m])
    h.cfg.counter = snap[1]
    parts.append(population_rollout(h, popn.struct, popn.pop, E, T, True, head=HEADS[head]))
    states.append(final_state(h))
  for k in OUT + ('act',) + (('eps',) if HEADS[head] is not None else ()):
    np.testing.assert_array_equal(np.concatenate([p[k] for p in parts], axis=2).view(np.uint8), got[k].view(np.uint8), err_msg=k)
  for k in SUMMARY:
    np.testing.assert_array_equal(np.concatenate([p[k] for p in parts], axis=1).view(np.uint8), got[k].view(np.uint8), err_msg=k)
  for k in end[0]:
    np.testing.assert_array_equal(np.concatenate([s[0][k] for s in states], axis=0).view(np.uint8), end[0][k].view(np.uint8), err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- 5. summary only = full launch
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('head', ['deterministic', 'sample_clamp'])
def test_summary_only_equals_the_full_launch_on_the_device(head, rt):
  n, E, T, G = 4096, 2, 200, 16
  kw = dict(reward_type=rt, reset_at_goal=True, wide_init=head != 'deterministic', horizon=T, seed=7, env_offset=OFFSET)
  popn = Population((64,), members_needed(OFFSET, n, G), G, gaussian=HEADS[head] is not None, seed0=0, device=GPU)
  d = prepared(n, True, device=GPU, **kw)
  snap = snapshot(d)
  full = population_rollout(d, popn.struct, popn.pop, E, T, True, head=HEADS[head])
  end = final_state(d)
  assert_bits(full, summary_by_definition(full['reward'], full['success']), SUMMARY)
  print(f'{head} {rt}: rows with a success {(full["first_success"] >= 0).mean():.4f}, successful at the last step {(full["success_last"] == 1).mean():.4f}')
  restore(d, snap)
  bare = population_rollout(d, popn.struct, popn.pop, E, T, True, head=HEADS[head], null=OUT + ('act', 'eps'))
  assert_bits(bare, full, SUMMARY)
  for k in OUT + ('act', 'eps'):                            # (the harness's fill pattern: nothing was written)
    assert np.isnan(bare[k]).all() if bare[k].dtype == np.float32 else (bare[k] == 7).all()
  assert_same_state(end, final_state(d))
  restore(d, snap)
  none = population_rollout(d, popn.struct, popn.pop, E, T, True, head=HEADS[head], summary=False)
  assert_bits(none, full, OUT + ('act',))
  assert np.isnan(none['ret']).all()


def test_null_population_is_the_existing_kernel_on_the_device():
  from test_policy_rollout import policy_rollout
  n, E, T = 1000, 2, 50
  kw = dict(reward_type='sparse', horizon=T, seed=8, env_offset=OFFSET)
  pol = Policy((256, 256), seed=2, device=GPU)
  d = prepared(n, True, device=GPU, **kw)
  snap = snapshot(d)
  got = population_rollout(d, pol.struct, None, E, T, True)
  end = final_state(d)
  restore(d, snap)
  want = policy_rollout(d, pol, E, T, True)
  assert_bits(got, want, OUT + ('act',))
  assert_same_state(end, final_state(d))


# ---------------------------------------------------------------------------------------------------------------- 6. the Python surface
@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian'])
def test_evaluate_policy_and_rollout_policy_on_cuda(gaussian):
  import earl_benchmark_amd as eb
  from earl_benchmark_amd import sharding
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  from gaussian_policy_helpers import GaussPolicy
  if gaussian:
    members = [GaussianMLPPolicy(GaussPolicy((64,), seed=s, log_std_gain=1.0).layers, 'relu') for s in range(8)]
  else:
    members = [MLPPolicy(Policy((64,), seed=s).layers, 'relu', 'tanh') for s in range(8)]
  pop_h = PolicyPopulation(members, envs_per_policy=64)
  pop_d = PolicyPopulation(members, envs_per_policy=64, device=GPU)
  assert pop_d.params.is_cuda and pop_d.device == torch.device(GPU) and torch.equal(pop_d.params.cpu(), pop_h.params)
  n, T, E = 500, 40, 2
  kw = dict(reward_type='sparse', wide_init_distr=True, num_envs=n, seed=3, env_offset=OFFSET)
  _, env_d = eb.EARLEnvs('tabletop_manipulation', device=GPU, **kw).get_envs()
  _, env_h = eb.EARLEnvs('tabletop_manipulation', device=CPU, **kw).get_envs()
  sd = env_d.unwrapped.state_dict()
  extra = dict(return_noise=True) if gaussian else {}
  outs, want = env_d.rollout_policy(pop_d, T, episodes=E, **extra), env_h.rollout_policy(pop_h, T, episodes=E, **extra)
  for a, b in zip(outs, want):
    assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8))
  assert env_d.total_steps == E * T and env_d.unwrapped._cfg.counter == env_h.unwrapped._cfg.counter
  if not gaussian:
    torch.testing.assert_close(pop_d(outs[0][0, :-1], env_offset=OFFSET), outs[4][0, 1:], rtol=1e-4, atol=1e-4)
  env_d.unwrapped.load_state_dict(sd)
  s = env_d.evaluate_policy(pop_d, T, episodes=E, sample=gaussian)
  ref = summary_by_definition(outs[1].cpu().numpy(), outs[3].cpu().numpy())
  assert all(v.is_cuda and tuple(v.shape) == (E, n) for v in s.values())
  np.testing.assert_array_equal(s['ret'].cpu().numpy().view(np.uint64), ref['ret'].view(np.uint64))
  np.testing.assert_array_equal(s['success'].cpu().numpy(), ref['success_last'].astype(bool))
  np.testing.assert_array_equal(s['first_success'].cpu().numpy(), ref['first_success'])
  assert env_d.unwrapped._cfg.counter == env_h.unwrapped._cfg.counter and env_d.total_steps == E * T      # (the state dict holds both counters: restored, then advanced again)
  # an in-place write to .params is what the next launch reads: member 1 overwritten with member 0 = the population built with member 0 twice
  pop_d.params[1].copy_(pop_d.params[0])
  env_d.unwrapped.load_state_dict(sd)
  s2 = env_d.evaluate_policy(pop_d, T, episodes=E, sample=gaussian)
  env_d.unwrapped.load_state_dict(sd)
  s3 = env_d.evaluate_policy(PolicyPopulation([members[0]] + members[:1] + members[2:], envs_per_policy=64, device=GPU), T, episodes=E, sample=gaussian)
  assert all(torch.equal(s2[k], s3[k]) for k in s2) and torch.equal(s2['ret'][:, :64 - OFFSET], s['ret'][:, :64 - OFFSET])
  fit = sharding.population_fitness(s, OFFSET, 64, 8)
  assert fit.is_cuda and tuple(fit.shape) == (8, 3) and float(fit[:, 2].sum()) == E * n
  with pytest.raises(ValueError):
    env_d.evaluate_policy(pop_h, T)

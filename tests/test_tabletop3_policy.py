"""earl_tabletop3_policy_rollout (include/earl_tabletop.h): the closed-loop rollout of the three-object tabletop -- a float32 MLP policy 20 -> hidden (-> hidden) -> 3
(6 with a Gaussian head), one policy or a population, with per-episode summaries.  Without a GPU, through csrc/libearl_host.so (the kernel's own headers compiled for
the host), the Python path on device='cpu' and the cross-compiled unit:
  1. closed = open, bit for bit: the launch equals earl_tabletop3_reset + earl_tabletop3_rollout fed with the actions it recorded, both forms, auto-reset off and on;
  2. pinned to the reference: OracleTabletop(nobj=3) stepped with the recorded actions reproduces observations and flags exactly;
  3. the coverage condition of the run the device test repeats: every object latched, a release, unsaturated actions in every dimension;
  4. the actions are the k-ascending fmaf chain, exactly (fractions.Fraction), and every input column of layer 0 reaches them;
  5. population = per-member launches, summary = its definitions, EARL_HEAD_MEAN = the deterministic launch on rows 0..2, eps_out = the specified draws;
  6. argument errors from both libraries;
  7. rollout_policy / evaluate_policy of the three-object env on device='cpu', and the refusals that stay;
  8. the unit holds exactly the 20 kernels, none with scratch, each with the waves per SIMD of its single-object twin, as recorded.
tests/test_tabletop3_policy_gpu.py holds the device to the host twin bit for bit.
Shapes: N = 40 envs from global id 3 (a workgroup that starts at a negative local index, a full one, a ragged one), T = 12 (tests/policy_width_cases.py)."""
import ctypes as C
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import kernel_build
import tabletop3_policy_helpers as t3
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import expected_uniform_index
from oracle import tabletop_oracle as orc
from policy_width_cases import N, OFFSET, T
from population_helpers import assert_bits, members_needed, pieces, summary_by_definition
from test_policy_rollout import assert_same_bits, final_state, restore, round_f32, snapshot

CPU = 'cpu'
GOALS = np.random.default_rng(5).uniform(-2.0, 2.0, size=(3, 10))      # goal rows without a zero in them: every observation column carries something
AUTO = dict(auto_reset=True, horizon=7)                                # horizon < T: the auto-reset fires inside the launch


# ---------------------------------------------------------------------------------------------------------------- 1. closed = open
@pytest.mark.parametrize('auto', [False, True], ids=['plain', 'auto_reset'])
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
def test_closed_equals_open_evaluation_form(rt, auto):
  h = t3.harness(CPU, reward_type=rt, reset_at_goal=True, seed=5, **(AUTO if auto else dict(horizon=T)))
  h.reset()
  pol = t3.net3((64,), seed=1)
  got, _ = t3.closed_equals_open3(h, pol.struct, 2, T, True)
  assert got['done'].any()
  assert h.host('num_interventions').min() >= 3                        # the constructor's reset and one per episode (auto-reset: more)


@pytest.mark.parametrize('auto', [False, True], ids=['plain', 'auto_reset'])
@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'sample'])
def test_closed_equals_open_continuing_form(gaussian, auto):
  h = t3.harness(CPU, reward_type='dense', reset_at_goal=True, seed=6, **(AUTO if auto else dict(horizon=10**6)))
  t3.start_somewhere(h)
  pol = t3.net3((48, 32), 'tanh', seed=3, gaussian=gaussian)
  got, _ = t3.closed_equals_open3(h, pol.struct, 1, T, False, head=dict(mode='sample') if gaussian else None)
  assert bool(got['done'].any()) == auto


# ---------------------------------------------------------------------------------------------------------------- 2. pinned to the reference
def test_oracle_stepped_with_the_recorded_actions_reproduces_the_closed_loop():
  E = 2                                                                # (the oracle's three-object step has no auto-reset: the reference class has none)
  kw = dict(reward_type='sparse', reset_at_goal=True, seed=9, env_offset=OFFSET, horizon=T)
  h, o = t3.harness(CPU, **{k: v for k, v in kw.items() if k != 'env_offset'}), orc.OracleTabletop(N, nobj=3, **kw)
  pol = t3.net3((32,), seed=11)
  got = t3.rollout3(h, pol.struct, E, T, True)
  for e in range(E):
    o.reset()
    obs, rew, done, succ = o.rollout(np.ascontiguousarray(got['act'][e]))
    np.testing.assert_array_equal(got['obs'][e].view(np.uint32), obs.view(np.uint32))
    np.testing.assert_array_equal(got['reward'][e], rew)
    np.testing.assert_array_equal(got['done'][e], done)
    np.testing.assert_array_equal(got['success'][e], succ)
  np.testing.assert_array_equal(h.host('qpos'), o.qpos)
  np.testing.assert_array_equal(h.host('attached'), o.attached)
  assert h.cfg.counter == o.cfg.counter


# ---------------------------------------------------------------------------------------------------------------- 3. the coverage condition
def test_the_coverage_run_latches_every_object_releases_and_leaves_actions_unsaturated():
  h = t3.coverage_harness(CPU)
  att0 = h.host('attached').copy()
  pol = t3.coverage_policy(CPU)
  got, _ = t3.closed_equals_open3(h, pol.struct, 1, t3.COVERAGE_T, False)
  latched, released, inside = t3.coverage_of(att0, got)
  print('latched', latched, 'envs that released', released, 'unsaturated', inside)
  assert latched == {0, 1, 2} and released >= 1 and all(inside)


# ---------------------------------------------------------------------------------------------------------------- 4. exact arithmetic
def small_case(pol, n=4, steps=2):
  """a continuing launch of a few rows from a state with nothing at zero -> (the observation each step consumed [steps, n, 20], the actions [steps, n, 3])"""
  h = t3.harness(CPU, n=n, reward_type='sparse', horizon=10**6, seed=1, goal_table=GOALS, n_sample_goals=3, reset_at_goal=True)
  t3.start_somewhere(h, steps=3)
  o = orc.OracleTabletop(n, nobj=3, reward_type='sparse', horizon=10**6, seed=1, goal_table=GOALS, n_sample_goals=3, reset_at_goal=True, env_offset=OFFSET)
  o.reset()
  x0 = o.rollout(np.random.default_rng(1).uniform(-1, 1, size=(3, n, 3)).astype(np.float32))[0][-1]      # the observation the scripted steps ended on
  got = t3.rollout3(h, pol.struct, 1, steps, False)
  x = np.concatenate([x0[None], got['obs'][:-1]])
  assert (x != 0).all()
  return x, got['act']


def test_small_case_exactly_against_the_fmaf_chain_in_fractions():
  pol = t3.net3((16,), 'relu', 'none', seed=8)
  x, act = small_case(pol)
  for t in range(x.shape[0]):
    for i in range(x.shape[1]):
      v = [Fraction(float(a)) for a in x[t, i]]
      for l, (w, b) in enumerate(pol.layers):
        nxt = []
        for j in range(w.shape[0]):
          acc = Fraction(float(b[j]))
          for k in range(w.shape[1]):
            acc = round_f32(v[k] * Fraction(float(w[j, k])) + acc)          # fmaf: one rounding
          nxt.append(max(acc, Fraction(0)) if l == 0 else acc)
        v = nxt
      want = np.array([float(a) for a in v], np.float32)
      np.testing.assert_array_equal(act[t, i].view(np.uint32), want.view(np.uint32))


def test_every_input_column_of_layer_0_reaches_the_actions():
  base = t3.net3((16,), 'tanh', 'none', seed=8)                        # (tanh: no hidden unit is dead)
  _, act = small_case(base, steps=1)
  for k in range(t3.OBS):
    pol = t3.net3((16,), 'tanh', 'none', seed=8)
    pol.params[(k % 16) * t3.OBS + k] += 0.25                          # W0[k % 16][k]
    _, moved = small_case(pol, steps=1)
    assert (moved.view(np.uint32) != act.view(np.uint32)).any(), k


# ---------------------------------------------------------------------------------------------------------------- 5. relations
G = 16                                                                 # global ids 3 .. 42: members 0, 1, 2, one per workgroup


@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'sample'])
@pytest.mark.parametrize('form', ['evaluation', 'continuing'])
def test_population_equals_the_per_member_launches_and_the_summary_its_definitions(form, gaussian):
  reset_first = form == 'evaluation'
  E = 2 if reset_first else 1
  kw = dict(reward_type='sparse', reset_at_goal=True, seed=77, **(dict(horizon=T) if reset_first else AUTO))
  head = dict(mode='sample', log_std_map='clamp') if gaussian else None
  popn = t3.Population3((48, 80), members_needed(OFFSET, N, G), G, gaussian=gaussian, seed0=11)
  h = t3.harness(CPU, **kw)
  t3.start_somewhere(h)
  snap = snapshot(h)
  got = t3.rollout3(h, popn.struct, E, T, reset_first, pop=popn.pop, head=head)
  end = final_state(h)
  keys = t3.OUT + ('act',) + (('eps',) if gaussian else ())
  outs, states = [], []
  for i0, m, member in pieces(OFFSET, N, G):
    hp = t3.harness(CPU, n=m, env_offset=OFFSET + i0, **kw)
    for k, v in snap[0].items():
      getattr(hp, k).copy_(v[i0:i0 + m])
    hp.cfg.counter = snap[1]
    outs.append(t3.rollout3(hp, popn.members[member].struct, E, T, reset_first, head=head))
    states.append(final_state(hp))
    assert states[-1][1] == end[1]
  axis = 2 if reset_first else 1
  assert_bits(got, {k: np.concatenate([o[k] for o in outs], axis=axis) for k in keys}, keys)
  for k in t3.SUMMARY:
    np.testing.assert_array_equal(got[k], np.concatenate([o[k] for o in outs], axis=1), err_msg=k)
  for k in end[0]:
    np.testing.assert_array_equal(end[0][k], np.concatenate([s[0][k] for s in states]), err_msg=k)
  # summary = its definitions applied to the [T] outputs, with and without them
  lead = (E, T, N)
  want = summary_by_definition(got['reward'].reshape(lead), got['success'].reshape(lead))
  np.testing.assert_array_equal(got['ret'].view(np.uint64), want['ret'].view(np.uint64))
  np.testing.assert_array_equal(got['success_last'], want['success_last'])
  np.testing.assert_array_equal(got['first_success'], want['first_success'])
  restore(h, snap)
  bare = t3.rollout3(h, popn.struct, E, T, reset_first, pop=popn.pop, head=head, null=t3.OUT + ('act', 'eps'))
  assert_bits(bare, got, t3.SUMMARY)


@pytest.mark.parametrize('hidden', [(32,), (48, 208)])
def test_head_mean_equals_the_deterministic_launch_and_eps_out_the_specified_draws(hidden):
  kw = dict(reward_type='sparse', reset_at_goal=True, horizon=T, seed=(1 << 40) + 12345)
  pol = t3.net3(hidden, 'relu', 'tanh', seed=4, gaussian=True)
  h = t3.harness(CPU, **kw)
  h.reset()
  h.cfg.counter = (1 << 32) - 5                                        # (the high word of the Philox counter changes inside the launch)
  snap = snapshot(h)
  mean = t3.rollout3(h, pol.struct, 2, T, True, head=dict(mode='mean'))
  restore(h, snap)
  twin = t3.mean_twin(pol)
  det = t3.rollout3(h, twin.struct, 2, T, True)
  assert_same_bits(mean, det, t3.OUT + ('act',) + t3.SUMMARY)
  restore(h, snap)
  smp = t3.rollout3(h, pol.struct, 2, T, True, head=dict(mode='sample'))
  np.testing.assert_array_equal(smp['eps'].view(np.uint32), mean['eps'].view(np.uint32))      # the draws do not depend on the mode
  assert (smp['act'] != mean['act']).any()
  counters = [snap[1] + e * (T + 1) + 1 + t for e in range(2) for t in range(T)]
  k24 = expected_uniform_index(kw['seed'], np.arange(N) + OFFSET, counters).reshape(2, T, N, 3)
  q = _abi.load_host().earl_normal_quantile_f32
  want = np.array([q(int(k)) for k in k24.reshape(-1)], np.float32).reshape(k24.shape)
  np.testing.assert_array_equal(smp['eps'].view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 6. argument errors
def _edge_calls(lib, host):
  h = t3.harness(CPU, n=8, env_offset=0)
  st = h._state()
  arrs, out = h._outs((3, 4, 8))                                       # (room for the good call with three episodes)
  pol, gpol = t3.net3((16,)), t3.net3((16,), gaussian=True)
  head = _abi.GaussianHead(mode=1, log_std_map=0, log_std_min=-5.0, log_std_max=2.0, eps_out=None)
  pop = _abi.PolicyPopulation(n_policies=1, envs_per_policy=16, param_stride=pol.params.numel())

  def call(cfg=h.cfg, state=st, p=pol.struct, pp=None, hd=None, E=1, T=4, rf=1, o=out):
    ref = lambda s: None if s is None else C.byref(s)
    args = [ref(cfg), ref(state), ref(p), ref(pp), ref(hd), E, T, rf, ref(o), None, None]
    return lib.earl_tabletop3_policy_rollout_cpu(*args) if host else lib.earl_tabletop3_policy_rollout(*args, None)

  def variant(base=pol, **kw):
    s = base.struct
    d = dict(n_layers=s.n_layers, dims=tuple(s.dims), hidden_act=s.hidden_act, out_act=s.out_act, precision=0, params=s.params)
    d.update(kw)
    d['dims'] = (C.c_int32 * 4)(*d['dims'])
    return _abi.MlpPolicy(**d)

  def cfg_with(**kw):
    c = _abi.TabletopCfg.from_buffer_copy(h.cfg)
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def pop_with(**kw):
    d = dict(n_policies=1, envs_per_policy=16, param_stride=pol.params.numel())
    d.update(kw)
    return _abi.PolicyPopulation(**d)

  bad = [dict(cfg=None), dict(state=None), dict(p=None), dict(o=None), dict(p=variant(params=None)),
         dict(p=variant(dims=(12, 16, 3, 0))), dict(p=variant(dims=(19, 16, 3, 0))), dict(p=variant(dims=(24, 16, 3, 0))),      # dims[0] is 20 and nothing else
         dict(p=variant(precision=_abi.PRECISION_BF16)), dict(p=variant(precision=1)),
         dict(p=variant(dims=(20, 16, 4, 0))), dict(p=variant(dims=(20, 16, 6, 0))), dict(p=variant(gpol, dims=(20, 16, 3, 0)), hd=head),      # 6 goes with a head, 3 without
         dict(p=variant(n_layers=1)), dict(p=variant(n_layers=4)), dict(p=variant(dims=(20, 24, 3, 0))), dict(p=variant(dims=(20, 272, 3, 0))),
         dict(p=variant(dims=(20, 0, 3, 0))), dict(p=variant(dims=(20, 16, 3, 5))), dict(p=variant(n_layers=3, dims=(20, 16, 8, 3))),
         dict(p=variant(hidden_act=0)), dict(p=variant(hidden_act=3)), dict(p=variant(out_act=1)),
         dict(T=0), dict(T=-1), dict(E=0), dict(E=2, rf=0), dict(rf=2),
         dict(p=gpol.struct, hd=_abi.GaussianHead(mode=2, log_std_map=0, log_std_min=-5.0, log_std_max=2.0, eps_out=None)),
         dict(p=gpol.struct, hd=_abi.GaussianHead(mode=1, log_std_map=0, log_std_min=-21.0, log_std_max=2.0, eps_out=None)),
         dict(pp=pop_with(n_policies=0)), dict(pp=pop_with(envs_per_policy=8)), dict(pp=pop_with(envs_per_policy=24)),
         dict(pp=pop_with(param_stride=pol.params.numel() - 1)), dict(pp=pop, cfg=cfg_with(env_offset=-1)), dict(pp=pop, cfg=cfg_with(env_offset=9)),      # ids 9 .. 16: member 1 of 1
         dict(cfg=cfg_with(wide_init=1)), dict(cfg=cfg_with(goal_change_frequency=5)), dict(cfg=cfg_with(n=-1))]
  for kw in bad:
    assert call(**kw) == -1, kw
    assert (lib.earl_host_last_error if host else lib.earl_last_error)(), kw
  assert call(cfg=cfg_with(n=0)) == 0                                  # nothing to do, before any HIP call
  call.keep = (h, arrs, pol, gpol)                                     # the buffers the structs point into
  call.good = [dict(), dict(pp=pop), dict(p=gpol.struct, hd=head), dict(E=3), dict(rf=0)]
  return call


def test_argument_errors_from_the_host_library():
  call = _edge_calls(_abi.load_host()._cdll, True)
  for kw in call.good:
    assert call(**kw) == 0, kw                                         # the good calls run (host pointers)


def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  _edge_calls(lib, False)
  assert lib.earl_tabletop3_policy_rollout(None, None, None, None, None, 1, 1, 1, None, None, None, None) == -1
  assert b'NULL' in lib.earl_last_error()


# ---------------------------------------------------------------------------------------------------------------- 7. Python on device='cpu'
def layers_of(pol):
  return [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in pol.layers]


def env3(device=CPU, **kw):
  from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  env = TabletopManipulation(reward_type='sparse', reset_at_goal=True, num_envs=N, device=device, seed=5, env_offset=OFFSET, **kw)
  env._cfg.horizon = T
  return env


def python_path(device):
  """every documented call of the three-object env's closed loop on `device` -> {name: tuple of host tensors}"""
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  kw = dict(device=device, obs_dim=20, act_dim=3)
  pi = MLPPolicy(layers_of(t3.net3((64,), seed=1)), 'relu', 'tanh', **kw)
  gp = GaussianMLPPolicy(layers_of(t3.net3((32, 48), seed=2, gaussian=True)), 'relu', **kw)
  pop = PolicyPopulation([MLPPolicy(layers_of(t3.net3((16,), seed=s)), 'relu', 'tanh', **kw) for s in range(4)], envs_per_policy=16, **kw)
  env, got = env3(device), {}
  sd = env.state_dict()
  got['policy'] = env.rollout_policy(pi, T, episodes=2)
  got['continuing'] = env.rollout_policy(pi, T, reset_first=False)
  got['sample'] = env.rollout_policy(gp, T, episodes=2, return_noise=True)
  got['mean'] = env.rollout_policy(gp, T, episodes=2, sample=False)
  got['population'] = env.rollout_policy(pop, T, episodes=2)
  assert env._cfg.counter == sd['rng_counter'] + 4 * 2 * (T + 1) + T and env.total_step_count == sd['total_step_count'] + 9 * T
  assert env._last_success.data_ptr() == got['population'][3][-1, -1].data_ptr()
  for name, p, sample in (('evaluate', pi, False), ('evaluate_sample', gp, True), ('evaluate_population', pop, False)):
    s = env.evaluate_policy(p, T, episodes=2, sample=sample)
    assert set(s) == {'ret', 'success', 'first_success'}
    got[name] = (s['ret'], s['success'], s['first_success'])
  return {k: tuple(t.cpu() for t in v) for k, v in got.items()}, (pi, gp, pop)


def test_rollout_policy_and_evaluate_policy_of_the_three_object_env_on_the_host():
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  got, (pi, gp, pop) = python_path(CPU)
  assert pop.stride == pop.n_params and pop.params.dtype == torch.float32          # packed as the tabletop's: stride piece 1
  lead = (2, T, N)
  assert [tuple(t.shape) for t in got['policy']] == [lead + (20,), lead, lead, lead, lead + (3,)]
  assert [tuple(t.shape) for t in got['continuing']] == [lead[1:] + (20,), lead[1:], lead[1:], lead[1:], lead[1:] + (3,)]
  assert [tuple(t.shape) for t in got['sample']] == [lead + (20,), lead, lead, lead, lead + (3,), lead + (3,)]
  assert all(tuple(t.shape) == (2, N) for k in ('evaluate', 'evaluate_sample', 'evaluate_population') for t in got[k])
  # the bits of test 1's procedure: the harness from the env's own start, the same packed network, the open loop fed with the actions
  env = env3()
  h = t3.harness(CPU, reward_type='sparse', reset_at_goal=True, horizon=T, seed=5)
  for k in h.STATE:
    if k not in ('steps_since_goal_change', 'lifelong_return', 'num_interventions'):
      getattr(h, k).copy_(getattr(env, k))
  h.cfg.counter = env._cfg.counter
  obs, rew, done, succ, act = got['policy']
  want = t3.open_loop3(h, act.numpy(), True)
  np.testing.assert_array_equal(obs.numpy().view(np.uint32), want['obs'].view(np.uint32))
  np.testing.assert_array_equal(rew.numpy(), want['reward'])
  np.testing.assert_array_equal(done.numpy(), want['done'].astype(bool))
  np.testing.assert_array_equal(succ.numpy(), want['success'].astype(bool))
  # evaluate_policy = the summary of what rollout_policy returns from the same start
  env = env3()
  s = env.evaluate_policy(pi, T, episodes=2)
  d = summary_by_definition(rew.numpy(), succ.numpy())
  np.testing.assert_array_equal(s['ret'].numpy().view(np.uint64), d['ret'].view(np.uint64))
  np.testing.assert_array_equal(s['success'].numpy(), d['success_last'].astype(bool))
  np.testing.assert_array_equal(s['first_success'].numpy(), d['first_success'])
  # the refusals that stay
  env = env3()
  narrow = MLPPolicy(layers_of(_twelve_wide()), 'relu', 'tanh')
  for method in ('rollout_policy', 'evaluate_policy'):
    with pytest.raises(NotImplementedError, match=re.escape(f'{method}: single-object env only')):
      getattr(env, method)(narrow, T)
    with pytest.raises(NotImplementedError, match=re.escape(f'{method}: single-object env only')):
      getattr(env, method)(PolicyPopulation([narrow] * 3), T)
    with pytest.raises(ValueError, match='observation width 14 and action width 4; the tabletop takes 12 and 3'):
      getattr(env, method)(MLPPolicy([(torch.zeros(16, 14), torch.zeros(16)), (torch.zeros(4, 16), torch.zeros(4))], obs_dim=14, act_dim=4), T)
    with pytest.raises(ValueError, match=re.escape('.widened()')):
      getattr(env, method)(MLPPolicy(layers_of(t3.net3((16,))), obs_dim=20, act_dim=3, param_dtype=torch.bfloat16), T)
  from earl_benchmark_amd.policy import AgentPair
  with pytest.raises(NotImplementedError, match=re.escape('rollout_agents: single-object env only')):
    env.rollout_agents(AgentPair(narrow, narrow), T)
  from earl_benchmark_amd.envs.tabletop import TabletopManipulation as OneObject
  one = OneObject(reward_type='sparse', num_envs=4, device=CPU)
  with pytest.raises(ValueError, match='observation width 20 and action width 3; the tabletop takes 12 and 3'):
    one.rollout_policy(pi, T)
  assert env._cfg.counter == env3()._cfg.counter and env.total_step_count == 0          # a refused call leaves the bookkeeping alone


def _twelve_wide():
  from test_policy_rollout import Policy
  return Policy((16,), seed=0)


# ---------------------------------------------------------------------------------------------------------------- 8. kernel resources
def test_the_unit_holds_the_twenty_kernels_without_scratch_and_with_the_recorded_figures():
  built = kernel_build.units(('tabletop3_policy.hip', 'tabletop_policy.hip', 'tabletop_policy_gaussian.hip'))
  now = built['tabletop3_policy.hip'].figures
  twins = {**built['tabletop_policy.hip'].figures, **built['tabletop_policy_gaussian.hip'].figures}
  want = {f'_ZN4earl23tabletop3_policy_kernelILi{nt2}ELb{g}ELb{s}EEEvNS_14PopulationArgsE' for nt2 in range(5) for g in (0, 1) for s in (0, 1)}
  assert set(now) == want, sorted(set(now) ^ want)
  recorded = kernel_build.recorded_figures()
  for name, fig in sorted(now.items()):
    twin = re.sub(r'^_ZN4earl23tabletop3_policy_kernel(I\w+?EEE)vNS_14PopulationArgsE$', r'_ZN4earl21policy_rollout_kernel\1vNS_12PolicyArgsOfIXT1_EE4typeE', name)
    assert twin in twins, (name, twin)
    print(name, fig, 'beside', twins[twin])
    assert fig[3] == 0, (name, 'scratch', fig[3])
    assert fig[1] + fig[2] <= 512, (name, 'registers', fig[1] + fig[2])
    assert fig[4] >= twins[twin][4], (name, 'waves per SIMD', fig[4], twins[twin][4])
    assert recorded.get(name) == [fig], (name, fig, recorded.get(name))

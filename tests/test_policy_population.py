"""earl_tabletop_population_rollout (include/earl_tabletop.h): the closed-loop tabletop rollout for a population of policies, with per-episode summaries.
Without a GPU, through csrc/libearl_host.so (the host twin) -- and csrc/libearl_hip.so for the argument errors, which come before any HIP call:
  1. population = per-policy launches of the EXISTING `_cpu` entry points on the shard cut at the multiples of G, bit for bit: outputs, actions, eps, state;
  2. two ragged shards whose cut is not a member boundary equal the batch;
  3. pop = NULL equals the existing entry point of the same head;
  4. each summary array equals its definition applied to the launch's own outputs, exactly, with and without the outputs, dense and sparse reward;
  5. every new argument error from both libraries;
  6. PolicyPopulation, evaluate_policy, rollout_policy(pop) and sharding.population_fitness on the host;
  7. the twenty existing kernels keep their recorded register / LDS / occupancy figures, the twenty new ones have no scratch (cross-compiled).
tests/test_policy_population_gpu.py holds the device to the host twin bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hip_harness as hx
import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import GaussPolicy, gaussian_rollout, head_struct
from population_helpers import (OUT, SUMMARY, Population, assert_bits, members_needed, per_policy_launches, population_rollout, summary_by_definition)
from test_policy_rollout import Policy, final_state, policy_rollout, restore, snapshot

CPU = 'cpu'
OFFSET = 3
HEADS = {'deterministic': None, 'sample_tanh': dict(mode='sample', log_std_map='tanh'), 'sample_clamp': dict(mode='sample', log_std_map='clamp'),
         'mean': dict(mode='mean', log_std_map='tanh')}
FORMS = {'evaluation': (2, True, dict(horizon=60)), 'lifelong': (1, False, dict(goal_change_frequency=17, horizon=10**6)),
         'auto_reset': (1, False, dict(auto_reset=True, horizon=13))}


def prepared(n, reset_first, device=CPU, **kw):
  """a harness in the state a launch starts from: a continuing rollout starts somewhere (a reset and a few scripted steps)"""
  h = hx.HipTabletop(n, device=device, **kw)
  h.reset()
  if not reset_first:
    h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, n, 3)).astype(np.float32))
  return h


# ---------------------------------------------------------------------------------------------------------------- 1. population = per-policy launches
@pytest.mark.parametrize('head', list(HEADS))
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('G', [16, 48])
@pytest.mark.parametrize('hidden', [(16,), (64,), (48, 32)], ids=str)
def test_population_equals_per_policy_launches_of_the_existing_entry_points(hidden, G, form, head):
  E, reset_first, cfg_kw = FORMS[form]
  T = 60
  for n in (1, 16, 100, 333):
    kw = dict(reward_type='sparse', wide_init=n == 100, seed=11, **cfg_kw)
    popn = Population(hidden, members_needed(OFFSET, n, G), G, gaussian=HEADS[head] is not None, hidden_act='tanh' if len(hidden) == 2 else 'relu', seed0=len(hidden) * 10)
    h = prepared(n, reset_first, env_offset=OFFSET, **kw)
    snap = snapshot(h)
    got = population_rollout(h, popn.struct, popn.pop, E, T, reset_first, head=HEADS[head])
    end = final_state(h)
    keys = OUT + ('act',) + (('eps',) if HEADS[head] is not None else ())
    assert not any(np.isnan(got[k]).any() for k in keys if got[k].dtype == np.float32), (n, 'an output was not written, or a read left the member\'s parameters')
    want, want_state, want_counter = per_policy_launches(h, snap, popn, E, T, reset_first, head=HEADS[head], **kw)
    assert_bits(got, want, keys)
    for k, v in want_state.items():
      np.testing.assert_array_equal(end[0][k].view(np.uint8), v.view(np.uint8), err_msg=f'n={n} state {k}')
    assert end[1] == want_counter == snap[1] + (E * (T + 1) if reset_first else T)
    if form == 'auto_reset':
      assert got['done'].any()


def test_the_member_depends_on_the_global_id_only():
  """the same 40 global ids as a batch of their own and inside a larger batch at another offset: same rows"""
  E, T, G = 2, 40, 16
  kw = dict(reward_type='sparse', horizon=T, seed=4)
  popn = Population((64,), members_needed(0, 200, G), G, seed0=3)
  big = prepared(150, True, env_offset=7, **kw)                # ids 7 .. 156
  small = prepared(40, True, env_offset=50, **kw)              # ids 50 .. 89 = rows 43 .. 82 of `big`
  a = population_rollout(big, popn.struct, popn.pop, E, T, True)
  b = population_rollout(small, popn.struct, popn.pop, E, T, True)
  for k in OUT + ('act',) + SUMMARY:
    np.testing.assert_array_equal(np.ascontiguousarray(a[k][..., 43:83, :] if a[k].ndim > 3 else a[k][..., 43:83]).view(np.uint8), b[k].view(np.uint8), err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- 2. shards = batch
@pytest.mark.parametrize('head', ['deterministic', 'sample_tanh'])
def test_two_ragged_shards_cut_inside_a_member_equal_the_batch(head):
  E, T, G, n = 2, 50, 16, 100
  kw = dict(reward_type='sparse', wide_init=True, horizon=T, seed=21)
  popn = Population((64,), members_needed(OFFSET, n, G), G, gaussian=HEADS[head] is not None, seed0=5)
  whole = prepared(n, True, env_offset=OFFSET, **kw)
  snap = snapshot(whole)
  got = population_rollout(whole, popn.struct, popn.pop, E, T, True, head=HEADS[head])
  end = final_state(whole)
  parts, states = [], []
  for i0, m in ((0, 60), (60, 40)):                           # the cut is at global id 63: inside member 3 (ids 48 .. 63), and not a multiple of 16
    h = hx.HipTabletop(m, device=CPU, env_offset=OFFSET + i0, **kw)
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
  assert states[0][1] == states[1][1] == end[1]


# ---------------------------------------------------------------------------------------------------------------- 3. pop = NULL
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('head', list(HEADS))
def test_null_population_is_the_existing_entry_point(head, form):
  E, reset_first, cfg_kw = FORMS[form]
  n, T = 70, 60
  kw = dict(reward_type='dense', seed=8, env_offset=OFFSET, **cfg_kw)
  pol = GaussPolicy((48, 32), 'tanh', seed=2) if HEADS[head] is not None else Policy((48, 32), 'tanh', seed=2)
  h = prepared(n, reset_first, **kw)
  snap = snapshot(h)
  got = population_rollout(h, pol.struct, None, E, T, reset_first, head=HEADS[head])
  end = final_state(h)
  restore(h, snap)
  want = gaussian_rollout(h, pol, E, T, reset_first, **HEADS[head]) if HEADS[head] is not None else policy_rollout(h, pol, E, T, reset_first)
  assert_bits(got, want, OUT + ('act',) + (('eps',) if HEADS[head] is not None else ()))
  again = final_state(h)
  for k in end[0]:
    np.testing.assert_array_equal(end[0][k].view(np.uint8), again[0][k].view(np.uint8), err_msg=k)
  assert end[1] == again[1]


# ---------------------------------------------------------------------------------------------------------------- 4. the summary
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('cfg', ['reset_at_goal', 'reset_at_goal_wide_init'])
def test_summary_equals_its_definition_on_the_launch_s_own_outputs(cfg, rt):
  """n = 512 at offset 3, seed 7, E = 2, T = 200, the four members Policy((64,), seed=0..3) (G = 144: global ids 3 .. 514 are members 0 .. 3).  Measured on the
  host twin with ONE of those policies on all 512 envs: reset_at_goal -- envs with any success 0 / 23.5 % / 49.1 % / 0, none successful at the last step;
  reset_at_goal + wide_init -- every env succeeds at some step, 100 % / 100 % / 100 % / 72 % at the last.  So the first configuration exercises both branches of
  first_success and the second both values of success_last; each is asserted to hold in at least 1 % of the rows."""
  n, E, T, G = 512, 2, 200, 144
  kw = dict(reward_type=rt, reset_at_goal=True, wide_init=cfg.endswith('wide_init'), horizon=T, seed=7, env_offset=OFFSET)
  popn = Population((64,), 4, G, seed0=0)
  assert members_needed(OFFSET, n, G) == 4
  h = prepared(n, True, **kw)
  snap = snapshot(h)
  got = population_rollout(h, popn.struct, popn.pop, E, T, True)
  end = final_state(h)
  want = summary_by_definition(got['reward'], got['success'])
  rows = E * n
  frac_first = (got['first_success'] >= 0).sum() / rows
  frac_last = (got['success_last'] == 1).sum() / rows
  print(f'{cfg} {rt}: rows with a success {frac_first:.4f}, rows successful at the last step {frac_last:.4f}, return in [{got["ret"].min():.4g}, {got["ret"].max():.4g}]')
  assert_bits(got, want, SUMMARY)
  assert set(np.unique(got['success_last'])) <= {0, 1} and got['first_success'].min() >= -1 and got['first_success'].max() < T
  if cfg == 'reset_at_goal':
    assert 0.01 <= frac_first <= 0.99
  else:
    assert 0.01 <= frac_last <= 0.99
  # the same summary with nothing else requested, and the same state left behind
  restore(h, snap)
  bare = population_rollout(h, popn.struct, popn.pop, E, T, True, null=OUT + ('act',))
  assert_bits(bare, got, SUMMARY)
  for k in OUT + ('act',):                                  # (the harness's fill pattern: nothing was written)
    assert np.isnan(bare[k]).all() if bare[k].dtype == np.float32 else (bare[k] == 7).all()
  again = final_state(h)
  for k in end[0]:
    np.testing.assert_array_equal(end[0][k].view(np.uint8), again[0][k].view(np.uint8), err_msg=k)
  # each summary pointer may be NULL on its own, and a NULL summary leaves the outputs what they were
  restore(h, snap)
  none = population_rollout(h, popn.struct, popn.pop, E, T, True, summary=False)
  assert_bits(none, got, OUT + ('act',))
  assert np.isnan(none['ret']).all() and (none['success_last'] == 7).all() and (none['first_success'] == -7).all()


def test_summary_with_a_gaussian_head_and_single_null_pointers():
  n, E, T, G = 100, 2, 50, 48
  kw = dict(reward_type='dense', reset_at_goal=True, wide_init=True, horizon=T, seed=7, env_offset=OFFSET)
  popn = Population((16,), members_needed(OFFSET, n, G), G, gaussian=True, seed0=1)
  h = prepared(n, True, **kw)
  snap = snapshot(h)
  got = population_rollout(h, popn.struct, popn.pop, E, T, True, head=HEADS['sample_clamp'])
  assert_bits(got, summary_by_definition(got['reward'], got['success']), SUMMARY)
  for keep in SUMMARY:
    restore(h, snap)
    lead = (E, T, n)
    arrs, out = h._outs(lead)
    bufs = {'ret': torch.full((E, n), float('nan'), dtype=torch.float64), 'success_last': torch.full((E, n), 7, dtype=torch.uint8),
            'first_success': torch.full((E, n), -7, dtype=torch.int32)}
    sm = _abi.EpisodeSummary(**{k: (bufs[k].data_ptr() if k == keep else None) for k in SUMMARY})
    hd = head_struct(**HEADS['sample_clamp'])
    st = h._state()
    rc = h.lib.earl_tabletop_population_rollout(C.byref(h.cfg), C.byref(st), C.byref(popn.struct), C.byref(popn.pop), C.byref(hd), E, T, 1, C.byref(out), None, C.byref(sm), None)
    assert rc == 0
    np.testing.assert_array_equal(bufs[keep].numpy().view(np.uint8), got[keep].view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- 5. argument errors
def _edge_calls(lib, host):
  n = 40
  h = hx.HipTabletop(n, device=CPU, env_offset=OFFSET)
  st = h._state()
  arrs, out = h._outs((1, 4, n))
  det, gau = Population((16,), 3, 16), Population((16,), 3, 16, gaussian=True)
  good_head = head_struct()
  bufs = (torch.zeros(1, n, dtype=torch.float64), torch.zeros(1, n, dtype=torch.uint8), torch.zeros(1, n, dtype=torch.int32))
  sm = _abi.EpisodeSummary(*(b.data_ptr() for b in bufs))

  def call(cfg=h.cfg, state=st, p=det.struct, pop=det.pop, hd=None, E=1, T=4, rf=1, o=out, s=sm):
    ref = lambda x: C.byref(x) if x is not None else None
    args = [ref(cfg), ref(state), ref(p), ref(pop), ref(hd), E, T, rf, ref(o), None, ref(s)]
    return lib.earl_tabletop_population_rollout_cpu(*args) if host else lib.earl_tabletop_population_rollout(*args, None)

  def popv(P=3, G=16, stride=det.n_params + 5):
    return _abi.PolicyPopulation(n_policies=P, envs_per_policy=G, param_stride=stride)

  def cfgv(**kw):
    c = _abi.TabletopCfg.from_buffer_copy(h.cfg)
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def variant(base, **kw):
    d = dict(n_layers=base.n_layers, dims=tuple(base.dims), hidden_act=base.hidden_act, out_act=base.out_act, precision=0, params=base.params)
    d.update(kw)
    d['dims'] = (C.c_int32 * 4)(*d['dims'])
    return _abi.MlpPolicy(**d)

  bad = [dict(pop=popv(G=24)), dict(pop=popv(G=8)), dict(pop=popv(G=0)), dict(pop=popv(G=-16)), dict(pop=popv(P=0)), dict(pop=popv(P=-1)),   # G % 16, G < 16, P < 1
         dict(pop=popv(stride=det.n_params - 1)), dict(pop=popv(stride=0)), dict(pop=popv(stride=-1)),                                           # stride below the parameter count
         dict(pop=popv(P=2)), dict(cfg=cfgv(env_offset=9)), dict(cfg=cfgv(env_offset=-1)),                                                      # ids 3 .. 42 need member 2; 9 .. 48 member 3
         dict(hd=good_head), dict(p=gau.struct, pop=gau.pop),                                                                                   # head and dims[n_layers] disagree
         dict(p=gau.struct, pop=gau.pop, hd=head_struct(mode=2)), dict(p=gau.struct, pop=gau.pop, hd=head_struct(bounds=(1.0, -1.0))),
         # what the single-policy entry points refuse
         dict(cfg=None), dict(state=None), dict(p=None), dict(o=None), dict(p=variant(det.struct, params=None)), dict(p=variant(det.struct, precision=1)),
         dict(p=variant(det.struct, dims=(12, 24, 3, 0))), dict(p=variant(det.struct, hidden_act=0)), dict(T=0), dict(E=0), dict(E=2, rf=0), dict(rf=2)]
  for kw in bad:
    assert call(**kw) == -1, kw
    assert (lib.earl_host_last_error if host else lib.earl_last_error)(), kw
  call.keep = (h, arrs, det, gau, bufs)
  return call, gau, good_head, popv


def test_argument_errors_from_the_host_library():
  lib = _abi.load_host()
  call, gau, good_head, popv = _edge_calls(lib._cdll, True)
  assert call() == 0                                                       # the good call runs (host pointers)
  assert call(p=gau.struct, pop=gau.pop, hd=good_head) == 0
  assert call(pop=None) == 0 and call(s=None) == 0 and call(pop=popv(P=7)) == 0 and call(pop=popv(G=48, P=1)) == 0
  assert call(cfg=None, pop=None) == -1


def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  _edge_calls(lib, False)
  assert lib.earl_tabletop_population_rollout(None, None, None, None, None, 1, 1, 1, None, None, None, None) == -1
  assert b'NULL' in lib.earl_last_error()


def test_struct_layouts_match_what_gcc_sees(tmp_path):
  src = '#include <stdio.h>\n#include <stddef.h>\n#include "earl_tabletop.h"\nint main(void) {\n'
  want = []
  for cname, cls in (('earl_policy_population', _abi.PolicyPopulation), ('earl_episode_summary', _abi.EpisodeSummary)):
    src += f'printf("%zu ", sizeof({cname}));\n' + ''.join(f'printf("%zu ", offsetof({cname}, {f[0]}));\n' for f in cls._fields_)
    want += [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src + 'return 0; }\n')
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  assert [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == want
  assert C.sizeof(_abi.PolicyPopulation) == 16 and C.sizeof(_abi.EpisodeSummary) == 24


# ---------------------------------------------------------------------------------------------------------------- 6. the Python surface on the host
def test_policy_population_packs_indexes_and_rejects():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  refs = [Policy((64,), seed=s) for s in range(4)]
  pis = [MLPPolicy(r.layers, 'relu', 'tanh') for r in refs]
  pop = PolicyPopulation(pis, envs_per_policy=32)
  assert eb.PolicyPopulation is PolicyPopulation and pop.n_policies == 4 and pop.stride == pop.n_params == refs[0].params.numel() and not pop.gaussian
  np.testing.assert_array_equal(pop.params.numpy(), np.stack([r.params.numpy() for r in refs]))
  assert pop.params.dtype == torch.float32 and pop.params.is_contiguous() and pop.struct.params == pop.params.data_ptr()
  assert (pop.pop_struct.n_policies, pop.pop_struct.envs_per_policy, pop.pop_struct.param_stride) == (4, 32, pop.n_params)
  np.testing.assert_array_equal(pop.policy_index(torch.tensor([0, 31, 32, 95, 96, 127])).numpy(), [0, 0, 1, 2, 3, 3])
  np.testing.assert_array_equal(pop.member(2).params.numpy(), refs[2].params.numpy())
  assert isinstance(pop.member(2), MLPPolicy) and pop.member(2).dims == [12, 64, 3]
  # the batched torch evaluation: each env through its own member, close to the member's own torch evaluation
  x = torch.randn(3, 100, 12)
  y = pop(x, env_offset=OFFSET)
  for i in (0, 28, 29, 60, 61, 99):
    torch.testing.assert_close(y[:, i], pis[(OFFSET + i) // 32](x[:, i]), rtol=1e-5, atol=1e-6)
  with pytest.raises(ValueError):
    pop(torch.randn(200, 12), env_offset=OFFSET)               # global ids up to 202 need member 6
  # a template and a [P, n_params (+ padding)] tensor; in-place writes reach the kernel's view
  theta = torch.cat([pop.params, torch.zeros(4, 3)], 1)
  tp = PolicyPopulation(pis[0], envs_per_policy=16, params=theta)
  assert tp.n_policies == 4 and tp.stride == pop.n_params + 3 and tp.envs_per_policy == 16
  ptr = tp.params.data_ptr()
  tp.params.mul_(2.0)
  assert tp.params.data_ptr() == ptr == tp.struct.params
  np.testing.assert_array_equal(tp.member(1).params.numpy(), 2.0 * refs[1].params.numpy())
  # rejections name the member
  with pytest.raises(ValueError, match='member 2'):
    PolicyPopulation([pis[0], pis[1], MLPPolicy(Policy((32,), seed=0).layers), pis[3]])
  with pytest.raises(ValueError, match='member 1'):
    PolicyPopulation([pis[0], MLPPolicy(refs[1].layers, 'tanh', 'tanh')])
  with pytest.raises(ValueError, match='member 1'):
    PolicyPopulation([pis[0], MLPPolicy(refs[1].layers, 'relu', 'none')])
  g = [GaussPolicy((64,), seed=s) for s in range(3)]
  gp = [GaussianMLPPolicy(r.layers, 'relu') for r in g]
  assert PolicyPopulation(gp).gaussian and PolicyPopulation(gp).dims == [12, 64, 6]
  with pytest.raises(ValueError, match='member 1'):
    PolicyPopulation([pis[0], gp[1]])
  for kw in (dict(squash=False), dict(log_std_bounds=(-4.0, 2.0)), dict(log_std_map='clamp')):
    with pytest.raises(ValueError, match='member 2'):
      PolicyPopulation([gp[0], gp[1], GaussianMLPPolicy(g[2].layers, 'relu', **kw)])
  for G in (0, 8, 24, -16):
    with pytest.raises(ValueError):
      PolicyPopulation(pis, envs_per_policy=G)
  with pytest.raises(ValueError):
    PolicyPopulation(pis[0])
  with pytest.raises(ValueError):
    PolicyPopulation(pis[0], params=torch.zeros(4, pop.n_params - 1))
  with pytest.raises(ValueError):
    PolicyPopulation([])


@pytest.mark.parametrize('gaussian', [False, True], ids=['deterministic', 'gaussian'])
def test_evaluate_policy_and_rollout_policy_agree_on_the_host_through_the_loader_and_the_wrappers(gaussian):
  import earl_benchmark_amd as eb
  from earl_benchmark_amd import sharding
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  if gaussian:
    members = [GaussianMLPPolicy(GaussPolicy((64,), seed=s, log_std_gain=1.0).layers, 'relu') for s in range(4)]
  else:
    members = [MLPPolicy(Policy((64,), seed=s).layers, 'relu', 'tanh') for s in range(4)]
  pop = PolicyPopulation(members, envs_per_policy=32)
  n, T, E = 100, 30, 2
  kw = dict(reward_type='dense', wide_init_distr=True, num_envs=n, device='cpu', seed=3, env_offset=OFFSET)
  _, env = eb.EARLEnvs('tabletop_manipulation', **kw).get_envs()
  sd = env.unwrapped.state_dict()
  outs = env.rollout_policy(pop, T, episodes=E, **(dict(return_noise=True) if gaussian else {}))
  obs, rew, done, succ, act = outs[:5]
  assert tuple(obs.shape) == (E, T, n, 12) and tuple(act.shape) == (E, T, n, 3) and env.total_steps == E * T and int(env.num_interventions.sum()) == E * n
  end = env.unwrapped.state_dict()
  # rollout_policy(pop) = the open loop fed with its actions, and each env's actions are its member's (torch: close)
  env.unwrapped.load_state_dict(sd)
  o2, r2, d2, s2 = env.rollout_episodes(act)
  assert torch.equal(obs.view(torch.int32), o2.view(torch.int32)) and torch.equal(rew, r2) and torch.equal(succ, s2)
  if not gaussian:
    torch.testing.assert_close(pop(obs[0, :-1], env_offset=OFFSET), act[0, 1:], rtol=1e-4, atol=1e-4)
  # evaluate_policy: the summary of the same launch, no [T] array, the same bookkeeping
  env.unwrapped.load_state_dict(sd)
  steps0 = env.total_steps
  s = env.evaluate_policy(pop, T, episodes=E, sample=gaussian)
  assert set(s) == {'ret', 'success', 'first_success'}
  assert s['ret'].dtype == torch.float64 and s['success'].dtype == torch.bool and s['first_success'].dtype == torch.int32
  assert all(tuple(v.shape) == (E, n) for v in s.values())
  want = summary_by_definition(rew.numpy(), succ.numpy())
  np.testing.assert_array_equal(s['ret'].numpy().view(np.uint64), want['ret'].view(np.uint64))
  np.testing.assert_array_equal(s['success'].numpy(), want['success_last'].astype(bool))
  np.testing.assert_array_equal(s['first_success'].numpy(), want['first_success'])
  after = env.unwrapped.state_dict()
  assert after['rng_counter'] == end['rng_counter'] == sd['rng_counter'] + E * (T + 1) and env.total_steps == steps0 + E * T
  assert torch.equal(after['qpos'], end['qpos']) and torch.equal(after['interventions'], end['interventions'])
  # one policy through the same method = the population whose members are all that policy
  env.unwrapped.load_state_dict(sd)
  one = env.evaluate_policy(members[1], T, episodes=E, sample=gaussian)
  env.unwrapped.load_state_dict(sd)
  same = env.evaluate_policy(PolicyPopulation([members[1]] * 4, envs_per_policy=32), T, episodes=E, sample=gaussian)
  assert all(torch.equal(one[k], same[k]) for k in one)
  if not gaussian:
    with pytest.raises(ValueError):
      env.evaluate_policy(pop, T, sample=True)
  # population_fitness: additive over two shards cut inside a member
  whole = sharding.population_fitness(s, OFFSET, 32, 4)
  assert tuple(whole.shape) == (4, 3) and whole.dtype == torch.float64
  np.testing.assert_array_equal(whole[:, 2].numpy(), [E * 29, E * 32, E * 32, E * 7])
  parts = []
  for i0, m in ((0, 45), (45, 55)):
    _, shard = eb.EARLEnvs('tabletop_manipulation', **dict(kw, num_envs=m, env_offset=OFFSET + i0)).get_envs()
    u = shard.unwrapped
    for name, key in (('qpos', 'qpos'), ('attached', 'attached'), ('goal_idx', 'goal_idx'), ('steps_since_reset', 'steps_since_reset'), ('interventions', 'interventions')):
      getattr(u, name).copy_(sd[key][i0:i0 + m])
    u._cfg.counter = sd['rng_counter']
    ps = shard.evaluate_policy(pop, T, episodes=E, sample=gaussian)
    assert all(torch.equal(ps[k], s[k][:, i0:i0 + m]) for k in ps)
    parts.append(sharding.population_fitness(ps, OFFSET + i0, 32, 4))
  np.testing.assert_array_equal((parts[0] + parts[1])[:, 1:].numpy(), whole[:, 1:].numpy())
  torch.testing.assert_close(parts[0] + parts[1], whole, rtol=1e-13, atol=0)             # (float64 sums of the same terms in another order)
  for p in range(4):
    lo, hi = max(p * 32 - OFFSET, 0), min((p + 1) * 32 - OFFSET, n)
    torch.testing.assert_close(whole[p, 0], s['ret'][:, lo:hi].sum(), rtol=1e-13, atol=0)
    assert int(whole[p, 1]) == int(s['success'][:, lo:hi].sum())
  with pytest.raises(ValueError):
    sharding.population_fitness(s, OFFSET, 16, 4)


def test_the_three_object_env_has_no_population_entry():
  from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation as TabletopManipulation3Obj
  from earl_benchmark_amd.policy import MLPPolicy, PolicyPopulation
  env = TabletopManipulation3Obj(num_envs=4, device='cpu')
  pop = PolicyPopulation([MLPPolicy(Policy((16,), seed=0).layers)])
  with pytest.raises(NotImplementedError):
    env.evaluate_policy(pop, 5)
  with pytest.raises(NotImplementedError):
    env.rollout_policy(pop, 5)


# ---------------------------------------------------------------------------------------------------------------- 7. kernel resources
def test_existing_kernels_keep_their_recorded_figures_and_the_new_ones_have_no_scratch():
  now = {}
  for unit in kernel_build.units(('tabletop_policy.hip', 'tabletop_policy_gaussian.hip', 'tabletop_policy_population.hip')).values():
    now.update(unit.figures)
  old = {k: v for k, v in now.items() if 'policy_rollout_kernel' in k}
  new = {k: v for k, v in now.items() if 'policy_population_kernel' in k}
  assert len(old) == 20 and len(new) == 20 and len(now) == 40, sorted(now)
  # every line on record of a kernel that still exists says what the compiler says now (the record was written before this feature and appended to after)
  recorded = kernel_build.recorded_figures()
  for name, fig in old.items():
    assert len(recorded.get(name, [])) >= 2 and all(r == fig for r in recorded[name]), (name, fig, recorded.get(name))
  for name, fig in new.items():
    assert recorded.get(name) == [fig], (name, fig, recorded.get(name))
    twin = re.sub(r'^_ZN4earl24policy_population_kernel(I\w+?EEE)vNS_14PopulationArgsE$', r'_ZN4earl21policy_rollout_kernel\1vNS_12PolicyArgsOfIXT1_EE4typeE', name)
    assert twin in old, (name, twin)
    print(name, fig, 'beside', old[twin])
    assert fig[3] == 0, (name, 'scratch', fig[3])
    assert fig[4] >= old[twin][4], (name, 'waves per SIMD', fig[4], old[twin][4])

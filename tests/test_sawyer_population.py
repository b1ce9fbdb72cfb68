"""earl_sawyer_population_rollout (include/earl_physics.h): the Sawyer door / peg closed loop for a POPULATION of policies, with per-env episode summaries and
without any [T] array.  What can be held without a GPU:
  1. PolicyPopulation(obs_dim=14, act_dim=4): packing, member(p) round trip, pop(obs, env_offset) against earl_mlp_policy_forward_cpu per member, the mismatch
     messages, and the tabletop's paths refusing such a population;
  2. the entry point is declared, bound and exported, and every new argument error comes back before any HIP call;
  3. compile time: the kernels that can run a population keep their timestep loops free of scratch and the occupancy / LDS of the plain instantiation, and the
     new arguments live in SawyerPolicyArgs only.
tests/test_sawyer_population_gpu.py holds the launches."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, head as head_of, variant as variant_of
from test_sawyer_policy_rollout import forward_cpu, pack, random_layers

CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')


def members_of(dims, P, head=False, seed0=0):
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  layers = [random_layers(dims, seed=seed0 + p, last_gain=1.5) for p in range(P)]
  if head:
    return [GaussianMLPPolicy(l, 'tanh', squash=True, log_std_map='clamp', obs_dim=14, act_dim=4) for l in layers], layers
  return [MLPPolicy(l, 'relu', 'tanh', obs_dim=14, act_dim=4) for l in layers], layers


# ---------------------------------------------------------------------------------------------------------------- 1. the container
@pytest.mark.parametrize('head', [False, True])
def test_population_of_sawyer_widths_packs_its_members_and_gives_them_back(head):
  from earl_benchmark_amd.policy import PolicyPopulation
  dims = [14, 32, 16, 8 if head else 4]
  P, G = 3, 16
  members, layers = members_of(dims, P, head)
  pop = PolicyPopulation(members, envs_per_policy=G, obs_dim=14, act_dim=4)
  n_params = sum(n * (k + 1) for k, n in zip(dims[:-1], dims[1:]))
  assert (pop.obs_dim, pop.act_dim, pop.n_policies, pop.envs_per_policy, pop.n_params) == (14, 4, P, G, n_params)
  assert pop.stride >= n_params and pop.stride % 4 == 0 and tuple(pop.params.shape) == (P, pop.stride)
  assert list(pop.struct.dims) == dims and (pop.pop_struct.n_policies, pop.pop_struct.envs_per_policy, pop.pop_struct.param_stride) == (P, G, pop.stride)
  for p in range(P):
    flat = np.concatenate([a.reshape(-1) for wb in layers[p] for a in wb])                  # W0, b0, W1, b1, ...
    np.testing.assert_array_equal(pop.params[p, :n_params].numpy(), flat)
    m = pop.member(p)
    assert type(m) is type(members[p]) and (m.obs_dim, m.act_dim) == (14, 4) and m.dims == dims
    np.testing.assert_array_equal(m.params.numpy(), members[p].params.numpy())
  # one template and a table of rows; a row length that is no multiple of four floats is padded to one (the kernel reads 16-byte pieces)
  theta = torch.cat([pop.params[:, :n_params], torch.zeros(P, 3)], 1)
  pop2 = PolicyPopulation(members[0], params=theta, envs_per_policy=G, obs_dim=14, act_dim=4)
  assert pop2.stride == (n_params + 3 + 3) // 4 * 4 and pop2.stride % 4 == 0
  np.testing.assert_array_equal(pop2.params[:, :n_params].numpy(), pop.params[:, :n_params].numpy())
  np.testing.assert_array_equal(pop2.member(2).params.numpy(), members[2].params.numpy())


@pytest.mark.parametrize('head', [False, True])
def test_population_forward_against_the_host_contract_per_member(head):
  """pop(obs, env_offset): every env through the member of its GLOBAL id; torch's summation order, so close to the contract (atol 1e-5, as the existing container
  test), not bit-identical"""
  from earl_benchmark_amd.policy import PolicyPopulation
  dims = [14, 32, 8 if head else 4]
  P, G, off, N = 4, 16, 8, 50                                             # global ids 8 .. 57: members 0 (partial) .. 3 (partial)
  members, layers = members_of(dims, P, head, seed0=10)
  pop = PolicyPopulation(members, envs_per_policy=G, obs_dim=14, act_dim=4)
  x = torch.as_tensor(np.random.default_rng(1).uniform(-1, 1, size=(2, N, 14)).astype(np.float32))
  got = pop(x, env_offset=off)
  assert tuple(got.shape) == (2, N, 4)
  member = (np.arange(N) + off) // G
  np.testing.assert_array_equal(pop.policy_index(torch.arange(N) + off).numpy(), member)
  hd = (_abi.HEAD_MEAN, _abi.LOGSTD_CLAMP, -5.0, 2.0) if head else None
  for p in range(P):
    rows = np.nonzero(member == p)[0]
    want = forward_cpu(layers[p], 'tanh' if head else 'relu', 'tanh', x[:, rows].reshape(-1, 14).numpy(), head=hd).reshape(2, len(rows), 4)
    np.testing.assert_allclose(got[:, rows].numpy(), want, rtol=0, atol=1e-5)
  assert not np.allclose(got[0, 0].numpy(), pop.member(1)(x[0, :1])[0].numpy(), atol=1e-3)      # (the members differ: env 0 is member 0's)
  with pytest.raises(ValueError, match='need members'):
    pop(x, env_offset=P * G - N + 1)


def test_population_width_mismatches_are_refused_by_name():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import MLPPolicy, PolicyPopulation
  (pi14, pj14), _ = members_of([14, 16, 4], 2)
  pi12 = MLPPolicy(random_layers([12, 16, 3], seed=0))
  with pytest.raises(ValueError, match='observation width 14 and action width 4; the tabletop takes 12 and 3'):
    PolicyPopulation([pi14, pj14])                                       # the defaults stay the tabletop's
  with pytest.raises(ValueError, match='observation width 12 and action width 3; 14 and 4 were declared'):
    PolicyPopulation([pi12, pi12], obs_dim=14, act_dim=4)
  with pytest.raises(ValueError, match='observation width 12 and action width 3; 14 and 4 were declared'):
    PolicyPopulation([pi14, pi12], obs_dim=14, act_dim=4)
  with pytest.raises(ValueError, match='observation width 12 and action width 3; 14 and 4 were declared'):
    PolicyPopulation(pi12, params=torch.zeros(2, pi12.params.numel()), obs_dim=14, act_dim=4)
  with pytest.raises(ValueError, match='member 1 has dims'):
    PolicyPopulation([pi14, members_of([14, 32, 4], 1)[0][0]], obs_dim=14, act_dim=4)
  with pytest.raises(ValueError, match='a multiple of 16'):
    PolicyPopulation([pi14, pj14], envs_per_policy=24, obs_dim=14, act_dim=4)
  # the tabletop keeps refusing a 14 / 4 population
  pop = PolicyPopulation([pi14, pj14], obs_dim=14, act_dim=4)
  _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=4, device='cpu', seed=3).get_envs()
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    env.rollout_policy(pop, 5)
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    env.evaluate_policy(pop, 5)


# ---------------------------------------------------------------------------------------------------------------- 2. declared, bound, exported; argument errors
def test_entry_point_is_declared_bound_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'int\s+earl_sawyer_population_rollout\s*\((.*?)\)\s*;', src, flags=re.S)
  assert m, 'earl_sawyer_population_rollout is not declared'
  assert len(m.group(1).split(',')) == len(_abi.SIGNATURES['earl_sawyer_population_rollout']) == 15
  assert 'const earl_policy_population* pop' in m.group(1) and 'const earl_episode_summary* summary' in m.group(1)      # earl_tabletop.h's structs, as they are
  assert hasattr(_abi.load(), 'earl_sawyer_population_rollout') and not hasattr(C.CDLL(_abi.HOST_LIB_PATH), 'earl_sawyer_population_rollout')


def test_new_argument_errors_need_no_gpu():
  """every refusal comes back before any HIP call (the pointers are host stand-ins that are never read), and an accepted call with n = 0 returns EARL_OK"""
  lib = _abi.load()
  layers = random_layers([14, 16, 4], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  count = keep.size                                                       # 14 * 16 + 16 + 16 * 4 + 4 = 308
  assert count == 308 and count % 4 == 0
  aligned = aligned_params(pol, keep, rows=4)                               # a 16-byte aligned home for four members
  buf = np.zeros(4096, np.float64)
  p = buf.ctypes.data
  st = _abi.SawyerState(qpos=p, qvel=p, mocap_pos=p, goal=p, last_obs=p)
  st_no_last = _abi.SawyerState(qpos=p, qvel=p, mocap_pos=p, goal=p)
  out, out_no_obs = _abi.SawyerOut(obs=p), _abi.SawyerOut()
  summ = _abi.EpisodeSummary(ret=p, success_last=p, first_success=p)

  def cfg(n, env_offset=0):
    return _abi.SawyerCfg(n=n, env_offset=env_offset, frame_skip=5)

  def pop(P=4, G=16, stride=count):
    return _abi.PolicyPopulation(n_policies=P, envs_per_policy=G, param_stride=stride)

  def variant(**kw):
    return variant_of(pol, **kw)

  def call(model=p, nv=10, cfg=cfg(0), st=st, pol=pol, pop=pop(), head=None, obs0=p, T=4, actions=p, out=out, summary=summ):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_sawyer_population_rollout(model, None, nv, ref(cfg), ref(st), ref(pol), ref(pop), ref(head), obs0, T, None, actions, ref(out), ref(summary), None)

  # accepted with n = 0: one policy or a population, with and without a summary, with and without actions / any `out` pointer (last_obs then carries the row)
  for kw in (dict(), dict(pop=None), dict(summary=None), dict(actions=None), dict(out=out_no_obs), dict(out=out_no_obs, actions=None, pop=None, summary=None),
             dict(pop=pop(stride=count + 4)), dict(pop=pop(G=1040)), dict(cfg=cfg(0, env_offset=7)), dict(summary=_abi.EpisodeSummary()), dict(nv=15)):
    assert call(**kw) == _abi.EARL_OK, kw
  head = head_of()
  assert call(pol=variant(dims=(14, 16, 8, 0)), head=head, pop=pop(stride=376)) == _abi.EARL_OK
  bad = [dict(pop=pop(G=24)), dict(pop=pop(G=8)), dict(pop=pop(G=0)), dict(pop=pop(G=-16)),                              # G % 16, G < 16
         dict(pop=pop(P=0)), dict(pop=pop(P=-1)),                                                                        # P < 1
         dict(pop=pop(stride=count - 4)), dict(pop=pop(stride=0)),                                                       # a stride below the parameter count
         dict(pop=pop(stride=count + 1)), dict(pop=pop(stride=count + 2)), dict(pop=pop(stride=count + 3)),              # param_stride % 4
         dict(pol=variant(dims=(14, 16, 8, 0)), head=head, pop=pop(stride=372)),                                         # (the count is that of the network given: 376)
         dict(cfg=cfg(0, env_offset=-1)), dict(cfg=cfg(8, env_offset=-16)),                                              # env_offset < 0 with pop
         dict(cfg=cfg(8, env_offset=57)), dict(cfg=cfg(1, env_offset=64)), dict(cfg=cfg(65)), dict(cfg=cfg(17), pop=pop(P=1)),      # (env_offset + n - 1) / G >= P
         dict(out=out_no_obs, st=st_no_last), dict(out=out_no_obs, st=st_no_last, pop=None, summary=None),               # out->obs == NULL needs st->last_obs
         # ... and what earl_sawyer_policy_rollout already refuses
         dict(out=None), dict(pol=None), dict(obs0=None), dict(model=None), dict(cfg=None), dict(st=None), dict(T=0), dict(nv=23),
         dict(pol=variant(dims=(12, 16, 4, 0))), dict(pol=variant(dims=(14, 24, 4, 0))), dict(pol=variant(precision=1)), dict(pol=variant(params=pol.params + 4)),
         dict(pol=variant(dims=(14, 16, 8, 0))), dict(head=head)]
  for kw in bad:
    assert call(**kw) == -1, kw
  # the last global id decides: ids 0 .. 63 fit four members of 16, id 64 does not; a negative offset is refused with a population only
  assert call(cfg=cfg(0, env_offset=-1), pop=None) == _abi.EARL_OK
  # the single-policy entry point keeps requiring what it required
  one = lambda actions, out: lib.earl_sawyer_policy_rollout(p, None, 10, C.byref(cfg(0)), C.byref(st), C.byref(pol), None, p, 4, None, actions, C.byref(out), None)
  assert one(p, out) == _abi.EARL_OK and one(None, out) == -1 and one(p, out_no_obs) == -1
  del aligned, buf


# ---------------------------------------------------------------------------------------------------------------- 3. compile time
def test_the_kernels_that_run_a_population_keep_the_timestep_loop_free_of_scratch_and_the_occupancy():
  """A population and a summary are wave-uniform runtime branches inside the four existing sawyer_policy_rollout_kernel instantiations (no new instantiation, no
  sibling kernel): each has zero scratch instructions inside its timestep loop (tools/scratch_in_loops.py's count) and the occupancy and LDS of the
  sawyer_rollout_kernel instantiation of the same template arguments in the same unit.  That these ARE the kernels a population runs: the member offset and the
  summary pointers are fields of SawyerPolicyArgs, read by sawyer_policy_action and the rollout body, and no other kernel takes that struct."""
  tool = kernel_build.tool()
  hdr = open(os.path.join(CSRC, 'physics_env_sawyer.h')).read()
  from population_no_gpu import policy_fields
  plain, policy, shared_hdr = policy_fields('physics_env_sawyer.h', 'SawyerPolicyArgs', 'SawyerArgs')
  for field in ('pop_G', 'pop_stride', 'sum_ret', 'sum_last', 'sum_first'):
    assert re.search(r'\b%s;' % field, policy) and field not in plain, field
  body = open(os.path.join(CSRC, 'physics_env_sawyer_rollout.inc')).read()
  # (the member's rows and the summary update are csrc/policy_closed_loop.h's, which sawyer_policy_action and the rollout body call)
  assert 'ka->pop_G' in shared_hdr and 'ka->sum_ret' in shared_hdr and 'cl_policy_weights(ka' in hdr and 'cl_episode_summary(' in body
  assert not re.search(r'\ba\.(pop_|sum_)\w+', hdr + body + shared_hdr.split('// ---')[1])      # never as a member of the kernel's argument
  kernels = set(re.findall(r'void (\w+)\(const SawyerPolicyArgs a\)', hdr))
  assert kernels == {'sawyer_policy_rollout_kernel'} and 'sawyer_policy_rollout_kernel' in tool.KERNELS
  want = {'physics.hip': {'<10, 16, false>', '<15, 16, false>', '<15, 16, true>'}, 'physics_w8.hip': {'<10, 16, false>'}}
  for unit_name, insts in want.items():
    unit = kernel_build.unit(unit_name)
    lines = [ln for ln in unit.scratch_report() if 'sawyer_policy_rollout_kernel' in ln]
    assert {re.search(r'sawyer_policy_rollout_kernel(<[^>]*>)', ln).group(1) for ln in lines} == insts, lines
    kernel_build.check_scratch_lines(lines, otherwise=('no scratch at all',))
    res = {k: (v['occupancy'], v['lds']) for k, v in unit.resources.items() if 'rollout_kernel<' in k}
    for inst in insts:
      assert res['sawyer_policy_rollout_kernel' + inst] == res['sawyer_rollout_kernel' + inst], (unit_name, inst, res)

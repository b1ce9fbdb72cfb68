"""earl_sawyer_pair_rollout (include/earl_physics.h): the forward / reset agent pair inside the Sawyer door / peg rollout kernel.  What can be held without a GPU:
  1. AgentPair(obs_dim=14, act_dim=4): packing, the stride of whole 16-byte pieces, agent(k) round trip, pair(obs, phase) against earl_mlp_policy_forward_cpu per
     phase, the 7-wide backward goal, the mismatch messages, no width limit, and the defaults still the tabletop's;
  2. the entry point is declared, bound and exported, and every new argument error comes back before any HIP call;
  3. compile time: the kernels that run a pair keep their timestep loops free of scratch and the occupancy / LDS of the plain instantiation, and the pair's
     arguments live in SawyerPolicyArgs only.
tests/test_sawyer_pair_gpu.py holds the launches."""
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


def agents_of(dims, head=False, seed0=0):
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  layers = [random_layers(dims, seed=seed0 + p, last_gain=1.5) for p in range(2)]
  if head:
    return [GaussianMLPPolicy(l, 'tanh', squash=True, log_std_map='clamp', obs_dim=14, act_dim=4) for l in layers], layers
  return [MLPPolicy(l, 'relu', 'tanh', obs_dim=14, act_dim=4) for l in layers], layers


# ---------------------------------------------------------------------------------------------------------------- 1. the container
@pytest.mark.parametrize('head', [False, True])
def test_pair_of_sawyer_widths_packs_its_agents_and_gives_them_back(head):
  from earl_benchmark_amd.policy import AgentPair
  dims = [14, 32, 16, 8 if head else 4]
  (f, b), layers = agents_of(dims, head)
  pair = AgentPair(f, b, switch_every=(5, 3), switch_on_success=False, backward_goal=None, obs_dim=14, act_dim=4)
  n_params = sum(n * (k + 1) for k, n in zip(dims[:-1], dims[1:]))
  assert (pair.obs_dim, pair.act_dim, pair.n_params, pair.switch_every, pair.switch_on_success) == (14, 4, n_params, (5, 3), False)
  assert pair.stride >= n_params and pair.stride % 4 == 0 and tuple(pair.params.shape) == (2, pair.stride)
  assert list(pair.struct.dims) == dims
  for k, m in enumerate((f, b)):
    flat = np.concatenate([a.reshape(-1) for wb in layers[k] for a in wb])                  # W0, b0, W1, b1, ...
    np.testing.assert_array_equal(pair.params[k, :n_params].numpy(), flat)
    np.testing.assert_array_equal(pair.params[k, :n_params].numpy(), m.params.numpy())
    a = pair.agent(k)
    assert type(a) is type(m) and (a.obs_dim, a.act_dim) == (14, 4) and a.dims == dims
    np.testing.assert_array_equal(a.params.numpy(), m.params.numpy())


def test_the_stride_is_whole_16_byte_pieces():
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  # the kernel reads both rows in 16-byte pieces (hidden widths are multiples of 16, so every legal count is one of four already: the padding rule is
  # PolicyPopulation's and costs nothing)
  for dims, count in (([14, 16, 4], 308), ([14, 48, 16, 4], 1572), ([14, 256, 256, 4], 70660)):
    (f, b), _ = agents_of(dims)
    pair = AgentPair(f, b, backward_goal=None, obs_dim=14, act_dim=4)
    assert pair.n_params == count and pair.stride == (count + 3) // 4 * 4
    np.testing.assert_array_equal(pair.agent(1).params.numpy(), b.params.numpy())
    assert not pair.params[:, count:].any()


@pytest.mark.parametrize('head', [False, True])
def test_pair_forward_against_the_host_contract_per_phase(head):
  """pair(obs, phase): every env through the agent of its phase; torch's summation order, so close to the contract (atol 1e-5), not bit-identical"""
  from earl_benchmark_amd.policy import AgentPair
  dims = [14, 32, 8 if head else 4]
  (f, b), layers = agents_of(dims, head, seed0=10)
  pair = AgentPair(f, b, backward_goal=None, obs_dim=14, act_dim=4)
  N = 50
  x = torch.as_tensor(np.random.default_rng(1).uniform(-1, 1, size=(2, N, 14)).astype(np.float32))
  phase = torch.as_tensor(np.arange(N) % 2, dtype=torch.int8)
  got = pair(x, phase)
  assert tuple(got.shape) == (2, N, 4)
  hd = (_abi.HEAD_MEAN, _abi.LOGSTD_CLAMP, -5.0, 2.0) if head else None
  for k in range(2):
    rows = np.nonzero(phase.numpy() == k)[0]
    want = forward_cpu(layers[k], 'tanh' if head else 'relu', 'tanh', x[:, rows].reshape(-1, 14).numpy(), head=hd).reshape(2, len(rows), 4)
    np.testing.assert_allclose(got[:, rows].numpy(), want, rtol=0, atol=1e-5)
  other = forward_cpu(layers[1], 'tanh' if head else 'relu', 'tanh', x[0, :1].numpy(), head=hd)
  assert not np.allclose(got[0, 0].numpy(), other[0], atol=1e-3)        # (the agents differ: env 0 is the forward agent's)


def test_backward_goal_widths_mismatches_and_the_width_limit():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  (pi14, pj14), _ = agents_of([14, 16, 4])
  pi12 = MLPPolicy(random_layers([12, 16, 3], seed=0))
  # the defaults stay the tabletop's: the message tests/test_sawyer_policy_rollout.py matches
  with pytest.raises(ValueError, match='observation width 14 and action width 4; the tabletop takes 12 and 3'):
    AgentPair(pi14, pj14)
  dflt = AgentPair(pi12, pi12)
  assert (dflt.obs_dim, dflt.act_dim, dflt.stride) == (12, 3, dflt.n_params) and dflt.backward_goal == 'initial'
  with pytest.raises(ValueError, match='ONE goal row of 6 values, got 7'):
    AgentPair(pi12, pi12, backward_goal=np.zeros(7))
  with pytest.raises(ValueError, match='observation width 12 and action width 3; 14 and 4 were declared'):
    AgentPair(pi12, pi12, obs_dim=14, act_dim=4)
  with pytest.raises(ValueError, match='observation width 12 and action width 3; 14 and 4 were declared'):
    AgentPair(pi14, pi12, obs_dim=14, act_dim=4)
  with pytest.raises(ValueError, match='member 1 has dims'):
    AgentPair(pi14, agents_of([14, 32, 4])[0][0], obs_dim=14, act_dim=4)
  # a 7-wide goal row is accepted, a 6-wide one refused
  g = np.arange(7, dtype=np.float64) / 10
  pair = AgentPair(pi14, pj14, backward_goal=g, obs_dim=14, act_dim=4)
  np.testing.assert_array_equal(pair.goal_row(None).numpy(), g)
  with pytest.raises(ValueError, match='ONE goal row of 7 values, got 6'):
    AgentPair(pi14, pj14, backward_goal=np.zeros(6), obs_dim=14, act_dim=4)
  # no EARL_PAIR_MAX_H2 here: the weights are read from memory; the tabletop pair keeps its limit
  (w0, w1), _ = agents_of([14, 32, 256, 4])
  wide = AgentPair(w0, w1, backward_goal=None, obs_dim=14, act_dim=4)
  assert wide.dims == [14, 32, 256, 4] and wide.stride % 4 == 0
  t256 = MLPPolicy(random_layers([12, 32, 256, 3], seed=0))
  with pytest.raises(ValueError, match='EARL_PAIR_MAX_H2'):
    AgentPair(t256, t256)
  # 'initial' resolves against the env: one row on the door, fifteen on the peg -- the caller picks
  from earl_benchmark_amd.envs import sawyer_door, sawyer_peg

  class Rows:
    def __init__(self, rows):
      self.initial_states = rows
  init = AgentPair(pi14, pj14, obs_dim=14, act_dim=4)
  np.testing.assert_array_equal(init.goal_row(Rows(sawyer_door.initial_states)).numpy(), sawyer_door.initial_states[0])
  with pytest.raises(ValueError, match=r'env\.initial_states has 15 rows'):
    init.goal_row(Rows(sawyer_peg.initial_states))
  # the tabletop refuses a 14 / 4 pair by name
  _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=4, device='cpu', seed=3).get_envs()
  with pytest.raises(ValueError, match='observation width 14 and action width 4; the tabletop takes 12 and 3'):
    env.rollout_agents(pair, 5)


def test_check_policy_no_longer_says_pairs_are_tabletop_only():
  src = open(os.path.join(REPO, 'earl_benchmark_amd', 'envs', 'sawyer_door.py')).read()
  assert 'agent pairs are tabletop only' not in src and 'def rollout_agents(self, pair, T, reset_first=False, sample=True, return_noise=False, out=None)' in src


# ---------------------------------------------------------------------------------------------------------------- 2. declared, bound, exported; argument errors
def test_entry_point_is_declared_bound_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'int\s+earl_sawyer_pair_rollout\s*\((.*?)\)\s*;', src, flags=re.S)
  assert m, 'earl_sawyer_pair_rollout is not declared'
  assert len(m.group(1).split(',')) == len(_abi.SIGNATURES['earl_sawyer_pair_rollout']) == 14
  assert 'const earl_agent_pair* pair' in m.group(1)                    # earl_tabletop.h's struct, as it is
  assert hasattr(_abi.load(), 'earl_sawyer_pair_rollout') and not hasattr(C.CDLL(_abi.HOST_LIB_PATH), 'earl_sawyer_pair_rollout')


def test_new_argument_errors_need_no_gpu():
  """every refusal comes back before any HIP call (the pointers are host stand-ins that are never read), and an accepted call with n = 0 returns EARL_OK"""
  lib = _abi.load()
  layers = random_layers([14, 16, 4], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  count = keep.size                                                       # 308
  assert count == 308 and count % 4 == 0
  aligned = aligned_params(pol, keep, rows=2)                               # a 16-byte aligned home for two agents
  buf = np.zeros(4096, np.float64)
  p = buf.ctypes.data
  st = _abi.SawyerState(qpos=p, qvel=p, mocap_pos=p, goal=p, last_obs=p, steps_since_goal_change=p)
  st_no_last = _abi.SawyerState(qpos=p, qvel=p, mocap_pos=p, goal=p)
  out, out_no_obs = _abi.SawyerOut(obs=p), _abi.SawyerOut()

  def cfg(n=0, rows=1, gcf=0):
    return _abi.SawyerCfg(n=n, env_offset=0, frame_skip=5, n_goal_rows=rows, goal_table=p if rows else None, goal_change_frequency=gcf)

  def pair(se=(5, 3), sos=1, stride=count, goal=None, phase=p, sip=p, agent=p, fs=p, bs=p):
    return _abi.AgentPair(switch_every=(C.c_int32 * 2)(*se), switch_on_success=sos, pad_=0, param_stride=stride, backward_goal=goal, phase=phase, steps_in_phase=sip,
                          agent_out=agent, forward_success=fs, backward_success=bs)

  def variant(**kw):
    return variant_of(pol, **kw)

  def call(model=p, nv=10, cfg=cfg(), st=st, pol=pol, pair=pair(), head=None, obs0=p, T=4, actions=p, out=out):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_sawyer_pair_rollout(model, None, nv, ref(cfg), ref(st), ref(pol), ref(pair), ref(head), obs0, T, None, actions, ref(out), None)

  head = head_of()
  for kw in (dict(), dict(nv=15), dict(actions=None), dict(out=out_no_obs), dict(out=out_no_obs, actions=None, pair=pair(agent=None, fs=None, bs=None)),
             dict(pair=pair(stride=count + 4)), dict(pair=pair(se=(1, 1), sos=0)), dict(pair=pair(goal=p)), dict(cfg=cfg(rows=0)), dict(cfg=cfg(rows=15), pair=pair(goal=p)),
             dict(pol=variant(dims=(14, 16, 8, 0)), head=head, pair=pair(stride=376)), dict(pol=variant(dims=(14, 16, 256, 4), n_layers=3), pair=pair(stride=8192))):
    assert call(**kw) == _abi.EARL_OK, kw
  bad = [dict(pair=None), dict(pair=pair(phase=None)), dict(pair=pair(sip=None)),                                         # NULL pair / phase / steps_in_phase
         dict(pair=pair(se=(0, 3))), dict(pair=pair(se=(5, 0))), dict(pair=pair(se=(-1, -1))),                            # switch_every[k] < 1
         dict(pair=pair(sos=2)), dict(pair=pair(sos=-1)),                                                                 # switch_on_success not 0 or 1
         dict(pair=pair(stride=count - 4)), dict(pair=pair(stride=0)),                                                    # a stride below the parameter count
         dict(pair=pair(stride=count + 1)), dict(pair=pair(stride=count + 2)), dict(pair=pair(stride=count + 3)),         # param_stride % 4
         dict(pol=variant(dims=(14, 16, 8, 0)), head=head, pair=pair(stride=372)),                                        # (the count is that of the network given: 376)
         dict(cfg=cfg(gcf=5)),                                                                                            # the pair IS the lifelong mechanism
         dict(cfg=cfg(rows=0), pair=pair(goal=p)),                                                                        # the forward goal could not be restored
         dict(out=out_no_obs, st=st_no_last),                                                                             # out->obs == NULL needs st->last_obs
         # ... and what earl_sawyer_population_rollout refuses with pop = NULL
         dict(out=None), dict(pol=None), dict(obs0=None), dict(model=None), dict(cfg=None), dict(st=None), dict(T=0), dict(nv=23),
         dict(pol=variant(dims=(12, 16, 4, 0))), dict(pol=variant(dims=(14, 24, 4, 0))), dict(pol=variant(precision=1)), dict(pol=variant(params=pol.params + 4)),
         dict(pol=variant(dims=(14, 16, 8, 0))), dict(head=head)]
  for kw in bad:
    assert call(**kw) == -1, kw
  del aligned, buf


# ---------------------------------------------------------------------------------------------------------------- 3. compile time
def test_the_kernels_that_run_a_pair_keep_the_timestep_loop_free_of_scratch_and_the_occupancy():
  """The pair is a set of runtime branches inside the four existing sawyer_policy_rollout_kernel instantiations (no new instantiation, no sibling kernel): each has zero
  scratch instructions inside its timestep loop (tools/scratch_in_loops.py's count) and the occupancy and LDS of the sawyer_rollout_kernel instantiation of the same
  template arguments in the same unit.  That these ARE the kernels a pair runs: its fields are in SawyerPolicyArgs (and not in SawyerArgs), read by
  sawyer_policy_action and the rollout body, and no other kernel takes that struct."""
  tool = kernel_build.tool()
  hdr = open(os.path.join(CSRC, 'physics_env_sawyer.h')).read()
  from population_no_gpu import policy_fields
  plain, policy, shared_hdr = policy_fields('physics_env_sawyer.h', 'SawyerPolicyArgs', 'SawyerArgs')
  for field in ('pair_phase', 'pair_sip', 'pair_stride', 'pair_goal', 'pair_se', 'pair_sos', 'pair_agent', 'pair_fs', 'pair_bs'):
    assert re.search(r'\b%s(\[2\])?;' % field, policy) and field not in plain, field
  body = open(os.path.join(CSRC, 'physics_env_sawyer_rollout.inc')).read()
  # (the weight rows of the phase and the handover decision are csrc/policy_closed_loop.h's, which sawyer_policy_action and the rollout body call)
  assert 'ka->pair_phase' in shared_hdr and 'ka->pair_stride' in shared_hdr and 'cl_policy_weights(ka' in hdr and 'ka->pair_phase' in body and 'ka->pair_goal' in body
  assert not re.search(r'\ba\.pair_\w+', hdr + body + shared_hdr.split('// ---')[1])      # never as a member of the kernel's argument
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

"""bf16 as a STORAGE format of the policy parameters on the stepper envs (earl_mlp_policy.precision == EARL_PRECISION_BF16; include/earl_tabletop.h), what can be
held without a GPU:
  1. packing: `param_dtype=torch.bfloat16` rounds every parameter once (round to nearest even, pinned on bit patterns), `.params` is the bf16 tensor,
     `.widened()` the float32 policy of exactly those values, the containers' strides are whole 16-byte pieces, a mixed list is refused by member;
  2. the host statement: earl_mlp_policy_forward_cpu with precision = 16 on the bf16 buffer == the same call with precision = 0 on the widened buffer, as bit
     patterns, for every shape of tests/policy_width_cases.py at the three env widths, without a head and in both head modes;
  3. the refusals, each EARL_ERR_ARG before any HIP call: every other precision value at every stepper entry point, precision = 16 at every tabletop entry point,
     misaligned params, strides that are a multiple of 4 but not of 8 elements; the well-formed row is accepted (n = 0); the tabletop's Python methods name widened();
  4. compile time: the four units that hold the bf16 kernels have no scratch instruction inside a timestep loop and the occupancy and LDS of the float32 kernel of
     the same form (the float32 units' own figures and the plain functions' digests are held by tests/test_closed_loop_args.py and its neighbours).
tests/test_policy_bf16_gpu.py holds the launches."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import kernel_build
import policy_bf16_cases as B
from earl_benchmark_amd import _abi
from policy_struct_helpers import variant
from test_sawyer_policy_rollout import random_layers

BF16 = torch.bfloat16
EARL_ERR_ARG = -1


def net(kind, hidden, seed=0, head=False, param_dtype=torch.float32, hact='tanh', specials=False):
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  O, A = B.WIDTHS[kind]
  layers = random_layers([O] + list(hidden) + [2 * A if head else A], seed=seed)
  if specials:
    B.plant_specials(layers)
  if head:
    return GaussianMLPPolicy(layers, hact, obs_dim=O, act_dim=A, param_dtype=param_dtype), layers
  return MLPPolicy(layers, hact, 'tanh', obs_dim=O, act_dim=A, param_dtype=param_dtype), layers


# ---------------------------------------------------------------------------------------------------------------- 1. packing
def test_rounding_is_to_nearest_even_on_the_pinned_bit_patterns():
  got = B.bits16(torch.from_numpy(B.special_f32()).to(BF16))
  np.testing.assert_array_equal(got, B.special_bf16_bits())


@pytest.mark.parametrize('kind', ['door', 'minitaur', 'kitchen'])
def test_packing_rounds_once_and_widened_holds_the_stored_values(kind):
  pi, layers = net(kind, (16, 32), seed=3, param_dtype=BF16, specials=True)
  flat = torch.cat([torch.from_numpy(a).reshape(-1) for wb in layers for a in wb])
  assert pi.params.dtype == BF16 and pi.param_dtype == BF16 and pi.struct.precision == 16 == _abi.PRECISION_BF16
  np.testing.assert_array_equal(B.bits16(pi.params), B.bits16(flat.to(BF16)))
  k = len(B.SPECIAL)
  np.testing.assert_array_equal(B.bits16(pi.params)[:k], B.special_bf16_bits())      # the first row of W0 carries the special values
  assert pi.struct.params == pi.params.data_ptr() and pi.params.data_ptr() % 16 == 0
  w = pi.widened()
  assert type(w) is type(pi) and w.params.dtype == torch.float32 and w.param_dtype == torch.float32 and w.struct.precision == 0
  np.testing.assert_array_equal(w.params.numpy().view(np.uint32), pi.params.float().numpy().view(np.uint32))
  np.testing.assert_array_equal(w.params.numpy().view(np.uint32), B.bits16(pi.params).astype(np.uint32) << 16)      # the value of an element: u << 16
  # .layers hold the widened values: pi(obs) is the network the kernel evaluates
  for (wa, ba), (wb, bb) in zip(pi.layers, w.layers):
    assert wa.dtype == torch.float32 and torch.equal(wa.view(torch.int32), wb.view(torch.int32)) and torch.equal(ba.view(torch.int32), bb.view(torch.int32))
  # a round trip, and the float32 default stays what it was
  again = w.with_param_dtype(BF16)
  np.testing.assert_array_equal(B.bits16(again.params), B.bits16(pi.params))
  plain, _ = net(kind, (16, 32), seed=3)
  assert plain.params.dtype == torch.float32 and plain.struct.precision == 0 and plain.param_dtype == torch.float32
  np.testing.assert_array_equal(plain.params.numpy().view(np.uint32), net(kind, (16, 32), seed=3)[0].widened().params.numpy().view(np.uint32))
  with pytest.raises(ValueError, match='param_dtype'):
    net(kind, (16,), param_dtype=torch.float16)


def test_gaussian_policy_takes_the_dtype():
  pi, _ = net('door', (16,), head=True, param_dtype=BF16)
  assert pi.params.dtype == BF16 and pi.struct.precision == 16 and pi.widened().log_std_bounds == pi.log_std_bounds and pi.widened().squash == pi.squash
  obs = torch.linspace(-1, 1, 5 * 14).reshape(5, 14)
  assert torch.equal(pi(obs), pi.widened()(obs)) and torch.equal(pi.sample(obs, torch.ones(5, 4)), pi.widened().sample(obs, torch.ones(5, 4)))


@pytest.mark.parametrize('kind', ['door', 'minitaur', 'kitchen'])
def test_containers_take_the_members_dtype_and_pad_to_whole_pieces(kind):
  from earl_benchmark_amd.policy import AgentPair, PairPopulation, PolicyPopulation
  O, A = B.WIDTHS[kind]
  mk = lambda seed, dt=BF16: net(kind, (16,), seed=seed, param_dtype=dt)[0]
  members = [mk(0), mk(1), mk(2)]
  count = members[0].params.numel()
  pop = PolicyPopulation(members, envs_per_policy=16, obs_dim=O, act_dim=A)
  assert pop.params.dtype == BF16 and pop.param_dtype == BF16 and pop.struct.precision == 16
  assert pop.stride % 8 == 0 and pop.stride >= count == pop.n_params and pop.pop_struct.param_stride == pop.stride
  for p, m in enumerate(members):
    np.testing.assert_array_equal(B.bits16(pop.params[p, :count]), B.bits16(m.params))
    assert pop.member(p).param_dtype == BF16
    np.testing.assert_array_equal(B.bits16(pop.member(p).params), B.bits16(m.params))
  assert not pop.params[:, count:].float().any()
  obs = torch.linspace(-1, 1, 40 * O).reshape(40, O)
  assert torch.equal(pop(obs, env_offset=5), pop.widened()(obs, env_offset=5))           # the torch statement widens first
  assert pop.widened().params.dtype == torch.float32 and pop.widened().struct.precision == 0
  # the template form: params of the template's dtype, a stride with padding beyond the rounded count
  wide = torch.zeros(3, pop.stride + 16, dtype=BF16)
  wide[:, :pop.stride] = pop.params
  tp = PolicyPopulation(members[0], envs_per_policy=16, params=wide, obs_dim=O, act_dim=A)
  assert tp.stride == pop.stride + 16 and tp.params.dtype == BF16 and tp.struct.precision == 16
  with pytest.raises(ValueError, match='params is torch.float32, the template policy stores torch.bfloat16'):
    PolicyPopulation(members[0], envs_per_policy=16, params=wide.float(), obs_dim=O, act_dim=A)
  with pytest.raises(ValueError, match='params is torch.bfloat16, the template policy stores torch.float32'):
    PolicyPopulation(members[0].widened(), envs_per_policy=16, params=wide, obs_dim=O, act_dim=A)
  with pytest.raises(ValueError, match=r'PolicyPopulation: member 2 has param_dtype = torch.float32, member 0 has torch.bfloat16'):
    PolicyPopulation([mk(0), mk(1), mk(2, torch.float32)], envs_per_policy=16, obs_dim=O, act_dim=A)
  # the pair and the population of pairs
  pair = AgentPair(mk(3), mk(4), switch_every=(2, 3), backward_goal=None, obs_dim=O, act_dim=A)
  assert pair.params.dtype == BF16 and pair.struct.precision == 16 and pair.stride % 8 == 0 and pair.stride >= count and pair.pair_stride == pair.stride
  assert pair.agent(1).param_dtype == BF16
  np.testing.assert_array_equal(B.bits16(pair.agent(1).params), B.bits16(mk(4).params))
  phase = torch.arange(7) % 2
  assert torch.equal(pair(obs[:7], phase), pair.widened()(obs[:7], phase))
  with pytest.raises(ValueError, match=r'AgentPair: member 1 has param_dtype = torch.float32, member 0 has torch.bfloat16'):
    AgentPair(mk(3), mk(4, torch.float32), backward_goal=None, obs_dim=O, act_dim=A)
  pairs = PairPopulation([pair, AgentPair(mk(5), mk(6), switch_every=(2, 3), backward_goal=None, obs_dim=O, act_dim=A)], envs_per_policy=16)
  assert pairs.params.dtype == BF16 and pairs.struct.precision == 16 and pairs.pair_stride % 8 == 0 and pairs.stride == 2 * pairs.pair_stride >= 2 * count
  assert pairs.pair(1).param_dtype == BF16 and pairs.widened().params.dtype == torch.float32
  np.testing.assert_array_equal(B.bits16(pairs.pair(1).params), B.bits16(pairs.params[1]))
  with pytest.raises(ValueError, match=r'PairPopulation: member 1 has param_dtype = torch.float32, member 0 has torch.bfloat16'):
    PairPopulation([pair, pair.widened()], envs_per_policy=16)


# ---------------------------------------------------------------------------------------------------------------- 2. the host statement
def host_forward(pol_struct, n, obs, A, head=None, eps=None):
  host = _abi.load_host()
  act = np.full((n, A), np.nan, np.float32)
  rc = host.earl_mlp_policy_forward_cpu(C.byref(pol_struct), None if head is None else C.byref(head), n, obs.ctypes.data, None if eps is None else eps.ctypes.data,
                                        act.ctypes.data)
  assert rc == 0, host.earl_host_last_error()
  return act


def aligned16(a):
  """a 16-byte aligned copy of a 1-d array -> (the view, the array to keep alive)"""
  raw = np.zeros(a.nbytes + 16, np.uint8)
  off = -raw.ctypes.data % 16
  raw[off:off + a.nbytes] = a.view(np.uint8)
  return raw[off:off + a.nbytes].view(a.dtype), raw


def host_cases():
  import policy_width_cases as W
  return [(O, A, hidden, head) for (O, A) in ((14, 4), (32, 8), (46, 9)) for hidden in W.SAWYER_SHAPES for head in (None, 'mean', 'sample')]


def test_host_forward_bf16_equals_fp32_on_the_widened_values():
  n, seen = 6, 0
  rng = np.random.default_rng(5)
  for s, (O, A, hidden, head) in enumerate(host_cases()):
    dims = [O] + list(hidden) + [2 * A if head else A]
    layers = random_layers(dims, seed=s)
    special = s % 5 == 0                                  # (under a tanh hidden layer, which bounds the row that carries bf16's largest value)
    if special:
      B.plant_specials(layers)
    flat = torch.cat([torch.from_numpy(a).reshape(-1) for wb in layers for a in wb])
    stored, keep16 = aligned16(B.bits16(flat.to(BF16)))
    widened, keep32 = aligned16((stored.astype(np.uint32) << 16).view(np.float32))
    d = dims + [0] * (4 - len(dims))
    hact = _abi.ACTIVATIONS['tanh'] if special else (_abi.ACTIVATIONS['relu'], _abi.ACTIVATIONS['tanh'])[s % 2]
    base = _abi.MlpPolicy(n_layers=len(dims) - 1, dims=(C.c_int32 * 4)(*d), hidden_act=hact, out_act=_abi.ACTIVATIONS['tanh'], precision=0, params=widened.ctypes.data)
    hd = None if head is None else _abi.GaussianHead(mode=_abi.HEAD_SAMPLE if head == 'sample' else _abi.HEAD_MEAN, log_std_map=(s // 2) % 2, log_std_min=-5.0,
                                                      log_std_max=2.0, eps_out=None)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    eps = rng.standard_normal((n, A)).astype(np.float32) if head == 'sample' else None
    want = host_forward(base, n, obs, A, hd, eps)
    got = host_forward(variant(base, precision=16, params=stored.ctypes.data), n, obs, A, hd, eps)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str((O, A, hidden, head)))
    assert not np.isnan(want).any() and len(np.unique(want)) > n
    # the rounding is in the values: the float32 call on the UNROUNDED parameters gives other bits
    unrounded, keep = aligned16(flat.numpy())
    assert (host_forward(variant(base, params=unrounded.ctypes.data), n, obs, A, hd, eps).view(np.uint32) != want.view(np.uint32)).any()
    seen += 1
    del keep16, keep32, keep
  assert seen == 3 * 34 * 3


def test_host_forward_refuses_what_the_contract_refuses():
  host = _abi.load_host()
  layers = random_layers([14, 16, 4], seed=0)
  flat = torch.cat([torch.from_numpy(a).reshape(-1) for wb in layers for a in wb])
  stored, keep = aligned16(np.concatenate([B.bits16(flat.to(BF16)), np.zeros(16, np.uint16)]))
  pol = _abi.MlpPolicy(n_layers=2, dims=(C.c_int32 * 4)(14, 16, 4, 0), hidden_act=1, out_act=2, precision=16, params=stored.ctypes.data)
  obs, act = np.zeros((2, 14), np.float32), np.zeros((2, 4), np.float32)
  call = lambda p: host.earl_mlp_policy_forward_cpu(C.byref(p), None, 2, obs.ctypes.data, None, act.ctypes.data)
  assert call(pol) == 0
  for precision in (1, -1, 8, 17, 32):
    assert call(variant(pol, precision=precision)) == EARL_ERR_ARG, precision
  for off in (2, 4, 8):
    assert call(variant(pol, params=stored.ctypes.data + off)) == EARL_ERR_ARG, off
  assert call(variant(pol, precision=0, params=stored.ctypes.data + 4)) == 0      # (float32 on the host keeps taking any address)
  del keep


# ---------------------------------------------------------------------------------------------------------------- 3. the refusals
_buf = np.zeros(4096, np.float64)                                          # state / output stand-in: an address, never read
P = _buf.ctypes.data
_params = np.zeros(64, np.float32)
PARAMS = _params.ctypes.data + (-_params.ctypes.data % 16)                 # 16-byte aligned, never read


def ref(s):
  return None if s is None else C.byref(s)


def sawyer_args():
  cfg = _abi.SawyerCfg(n=0, env_offset=0, frame_skip=5, n_goal_rows=1, goal_table=P, goal_change_frequency=0)
  st = _abi.SawyerState(qpos=P, qvel=P, mocap_pos=P, goal=P, last_obs=P, steps_since_goal_change=P)
  return cfg, st, _abi.SawyerOut(obs=P)


def minitaur_args():
  cfg = _abi.MinitaurCfg(n=0, env_offset=0, num_substeps=5, n_goals=12, goal_table=P, goal_change_frequency=0)
  st = _abi.MinitaurState(qpos=P, qvel=P, goal=P, motor_param=P, observed_torque=P, overheat=P, motor_enabled=P, steps_since_goal_change=P, last_obs=P)
  return cfg, st, _abi.MinitaurOut(obs=P, reward=P, done=P, success=P)


def kitchen_args():
  cfg = _abi.KitchenCfg(n=0, frame_skip=40, n_att=12, mocap_quat_dev=P)
  cfg.site_att[:] = [0, 1, 2, 3, 4, 5, 6, 7]
  st = _abi.KitchenState(qpos=P, qvel=P, mocap_pos=P, goal=P, last_qp_robot=P, att_xpos=P, steps_since_reset=P, last_obs=P)
  return _abi.KitchenParams(), cfg, st, _abi.KitchenOut(obs=P, reward=P, done=P, success=P)


def tabletop_args():
  cfg = _abi.TabletopCfg(n=0, env_offset=0, reward_type=0, goal_change_frequency=0, n_goals=4, n_sample_goals=4)
  st = _abi.TabletopState(qpos=P, attached=P, goal_idx=P, goal_table=P, steps_since_reset=P, num_interventions=P, steps_since_goal_change=P, lifelong_return=P)
  return cfg, st, _abi.TabletopOut(obs=P, reward=P, done=P, success=P)


def _sw(name):
  def call(lib, pol, pop, pair):
    cfg, st, out = sawyer_args()
    f = getattr(lib, name)
    if name == 'earl_sawyer_policy_rollout':
      return f(P, None, 10, ref(cfg), ref(st), ref(pol), None, P, 4, None, P, ref(out), None)
    if name == 'earl_sawyer_population_rollout':
      return f(P, None, 10, ref(cfg), ref(st), ref(pol), ref(pop), None, P, 4, None, P, ref(out), None, None)
    if name == 'earl_sawyer_pair_rollout':
      return f(P, None, 10, ref(cfg), ref(st), ref(pol), ref(pair), None, P, 4, None, P, ref(out), None)
    return f(P, None, 10, ref(cfg), ref(st), ref(pol), ref(pair), ref(pop), None, None, P, 4, None, P, ref(out), None, None)
  return call


def _mt(name):
  def call(lib, pol, pop, pair):
    cfg, st, out = minitaur_args()
    f = getattr(lib, name)
    if name == 'earl_minitaur_policy_rollout':
      return f(P, None, ref(cfg), ref(st), ref(pol), None, P, 4, None, P, ref(out), None)
    if name == 'earl_minitaur_population_rollout':
      return f(P, None, ref(cfg), ref(st), ref(pol), ref(pop), None, P, 4, None, P, ref(out), None, None)
    return f(P, None, ref(cfg), ref(st), ref(pol), ref(pair), ref(pop), None, None, P, 4, None, P, ref(out), None, None)
  return call


def _kt(name):
  def call(lib, pol, pop, pair):
    params, cfg, st, out = kitchen_args()
    f = getattr(lib, name)
    if name == 'earl_kitchen_policy_rollout':
      return f(P, None, ref(params), ref(cfg), ref(st), ref(pol), None, P, 4, None, P, ref(out), None)
    if name == 'earl_kitchen_population_rollout':
      return f(P, None, ref(params), ref(cfg), ref(st), ref(pol), ref(pop), None, P, 4, None, P, ref(out), None, None)
    return f(P, None, ref(params), ref(cfg), ref(st), ref(pol), ref(pair), ref(pop), None, None, 0, None, P, 4, None, P, ref(out), None, None)
  return call


def _tt(name):
  def call(lib, pol, pop, pair):
    cfg, st, out = tabletop_args()
    f = getattr(lib, name)
    if name == 'earl_tabletop_policy_rollout':
      return f(ref(cfg), ref(st), ref(pol), 1, 4, 1, ref(out), P, None)
    if name == 'earl_tabletop_population_rollout':
      return f(ref(cfg), ref(st), ref(pol), ref(pop), None, 1, 4, 1, ref(out), P, None, None)
    return f(ref(cfg), ref(st), ref(pol), ref(pair), None, 1, 4, 1, ref(out), P, None)
  return call


# name -> (observation width, action width, takes a population, takes a pair, the call)
STEPPER = {name: (O, A, 'population' in name or 'agents' in name, 'pair' in name or 'agents' in name, maker(name))
           for maker, O, A, names in ((_sw, 14, 4, ('earl_sawyer_policy_rollout', 'earl_sawyer_population_rollout', 'earl_sawyer_pair_rollout', 'earl_sawyer_agents_rollout')),
                                      (_mt, 32, 8, ('earl_minitaur_policy_rollout', 'earl_minitaur_population_rollout', 'earl_minitaur_agents_rollout')),
                                      (_kt, 46, 9, ('earl_kitchen_policy_rollout', 'earl_kitchen_population_rollout', 'earl_kitchen_agents_rollout')))
           for name in names}
TABLETOP = {name: (12, 3, 'population' in name, 'pair' in name, _tt(name))
            for name in ('earl_tabletop_policy_rollout', 'earl_tabletop_population_rollout', 'earl_tabletop_pair_rollout')}


def run(entry, precision=16, params=PARAMS, pop_stride=None, pair_stride=None):
  """one call with otherwise valid arguments of the entry point's widths, n = 0 -> (return code, the policy's parameter count)"""
  O, A, takes_pop, takes_pair, call = entry
  count = 16 * (O + 1) + A * 17
  piece = 8 if precision == 16 else 4
  rounded = (count + piece - 1) // piece * piece
  pol = _abi.MlpPolicy(n_layers=2, dims=(C.c_int32 * 4)(O, 16, A, 0), hidden_act=1, out_act=2, precision=precision, params=params)
  pstride = rounded if pair_stride is None else pair_stride(count)
  pair = _abi.AgentPair(switch_every=(C.c_int32 * 2)(5, 3), switch_on_success=1, pad_=0, param_stride=pstride, backward_goal=None, phase=P, steps_in_phase=P,
                        agent_out=None, forward_success=None, backward_success=None) if takes_pair else None
  base = 2 * pstride if takes_pair else rounded              # (a population of pairs: a member is two rows)
  pop = _abi.PolicyPopulation(n_policies=4, envs_per_policy=16, param_stride=base if pop_stride is None else pop_stride(count)) if takes_pop else None
  return call(_abi.load(), pol, pop, pair)


@pytest.mark.parametrize('name', sorted(STEPPER))
def test_every_stepper_entry_point_takes_bf16_and_refuses_every_other_precision(name):
  entry = STEPPER[name]
  assert run(entry, precision=0) == _abi.EARL_OK and run(entry, precision=16) == _abi.EARL_OK
  for precision in (8, 32, 17, 1, -1):
    assert run(entry, precision=precision) == EARL_ERR_ARG, precision
  for off in (4, 8):
    assert run(entry, params=PARAMS + off) == EARL_ERR_ARG, off
  r8 = lambda c: (c + 7) // 8 * 8
  if entry[2]:
    assert run(entry, pop_stride=lambda c: 2 * r8(c) + 4) == EARL_ERR_ARG       # a multiple of 4, not of 8
    assert run(entry, pop_stride=lambda c: 2 * r8(c) + 16) == _abi.EARL_OK      # padding beyond the rounded count
    assert run(entry, precision=0, pop_stride=lambda c: 2 * r8(c) + 4) == _abi.EARL_OK      # (float32: whole pieces are 4 elements, as before)
    if not entry[3]:
      assert run(entry, pop_stride=lambda c: r8(c) - 8) == EARL_ERR_ARG         # below the parameter count
  if entry[3]:
    assert run(entry, pair_stride=lambda c: r8(c) + 4) == EARL_ERR_ARG
    assert run(entry, pair_stride=lambda c: r8(c) + 8) == _abi.EARL_OK
    assert run(entry, precision=0, pair_stride=lambda c: r8(c) + 4) == _abi.EARL_OK
    assert run(entry, pair_stride=lambda c: r8(c) - 8) == EARL_ERR_ARG


@pytest.mark.parametrize('name', sorted(TABLETOP) + ['earl_tabletop_policy_rollout_gaussian'])
def test_every_tabletop_entry_point_refuses_bf16(name):
  lib = _abi.load()
  if name.endswith('gaussian'):
    cfg, st, out = tabletop_args()
    hd = _abi.GaussianHead(mode=_abi.HEAD_SAMPLE, log_std_map=_abi.LOGSTD_TANH, log_std_min=-5.0, log_std_max=2.0, eps_out=None)
    for precision, want in ((0, _abi.EARL_OK), (16, EARL_ERR_ARG)):
      pol = _abi.MlpPolicy(n_layers=2, dims=(C.c_int32 * 4)(12, 16, 6, 0), hidden_act=1, out_act=2, precision=precision, params=PARAMS)
      assert lib.earl_tabletop_policy_rollout_gaussian(ref(cfg), ref(st), ref(pol), ref(hd), 1, 4, 1, ref(out), P, None) == want
    return
  assert run(TABLETOP[name], precision=0) == _abi.EARL_OK
  assert run(TABLETOP[name], precision=16) == EARL_ERR_ARG
  assert 'bf16' in lib.earl_last_error().decode()


def test_the_host_twins_of_the_tabletop_refuse_bf16_too():
  host = _abi.load_host()
  cfg, st, out = tabletop_args()
  for precision, want in ((0, _abi.EARL_OK), (16, EARL_ERR_ARG)):
    pol = _abi.MlpPolicy(n_layers=2, dims=(C.c_int32 * 4)(12, 16, 3, 0), hidden_act=1, out_act=2, precision=precision, params=PARAMS)
    assert host.earl_tabletop_policy_rollout_cpu(ref(cfg), ref(st), ref(pol), 1, 4, 1, ref(out), P) == want


def test_the_tabletop_methods_name_widened():
  from earl_benchmark_amd.envs.tabletop import TabletopManipulation
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy, PolicyPopulation
  mk = lambda seed: MLPPolicy(random_layers([12, 16, 3], seed=seed), 'relu', 'tanh', param_dtype=BF16)
  pi = mk(0)
  pop = PolicyPopulation([mk(0), mk(1), mk(2)], envs_per_policy=16)
  pair = AgentPair(mk(3), mk(4), backward_goal=None)
  env = TabletopManipulation.__new__(TabletopManipulation)                # (the env itself may need a device; its checks do not)
  env.device, env.num_envs = torch.device('cpu'), 40
  for call in (lambda: env.rollout_policy(pi, 4), lambda: env.rollout_policy(pop, 4), lambda: env.evaluate_policy(pi, 4), lambda: env.evaluate_policy(pop, 4),
               lambda: env.rollout_agents(pair, 4)):
    with pytest.raises(ValueError, match=r'widened\(\)'):
      call()


# ---------------------------------------------------------------------------------------------------------------- 4. compile time
BF16_UNITS = {'physics_bf16.hip': 'physics.hip', 'physics_w8_bf16.hip': 'physics_w8.hip', 'physics_mt_bf16.hip': 'physics_mt.hip',
              'physics_kitchen_policy_bf16.hip': 'physics_kitchen_policy.hip'}


def test_the_bf16_units_keep_occupancy_and_lds_and_have_no_scratch_in_a_timestep_loop():
  import json
  import os
  from conftest import GOLDEN
  want = json.load(open(os.path.join(GOLDEN, 'closed_loop_parent_build.json')))['policy_kernel_resources']      # the float32 policy kernels (tests/test_closed_loop_args.py holds them to it)
  built, tool = kernel_build.units(BF16_UNITS), kernel_build.tool()
  seen = 0
  for unit, twin in BF16_UNITS.items():
    res = built[unit].resources
    kernels = {k: v for k, v in res.items() if 'policy' in k}
    assert all(k.startswith('bf16::') for k in kernels), sorted(kernels)             # a kernel trace tells the two forms apart
    assert {k.replace('bf16::', '') for k in kernels} == set(want[twin]), (unit, sorted(kernels))
    assert not [k for k in res if 'policy' not in k and ('rollout_kernel' in k or 'minitaur' in k or 'physics_kernel' in k)], sorted(res)      # the policy kernels only
    for k, now in sorted(kernels.items()):
      fp32 = want[twin][k.replace('bf16::', '')]
      print(unit, k, now, 'float32:', fp32)
      assert (now['occupancy'], now['lds']) == (fp32['occupancy'], fp32['lds']), (k, now, fp32)
      seen += 1
    lines = [ln for ln in built[unit].scratch_report(tool.KERNELS + tool.POLICY_DUO) if 'policy' in ln]
    assert len(lines) == len(kernels), lines
    # (the two-wave minitaur kernel has one slot loop and no timestep loop, like its float32 form)
    kernel_build.check_scratch_lines(lines, otherwise=('no scratch at all', 'slot loop'))
  assert seen == 9      # door, peg, peg time-sliced, door eight-wave, minitaur one-wave and two-wave, kitchen x 3
  # the weight path: 16-byte loads in the function that evaluates the policy
  for unit in BF16_UNITS:
    asm = built[unit].asm
    start = next(i for i, ln in enumerate(asm) if re.match(r'^_Z\w*policy_action\w*:', ln))
    end = next(i for i in range(start, len(asm)) if asm[i].startswith('.Lfunc_end'))
    body = '\n'.join(asm[start:end])
    assert 'global_load_dwordx4' in body, unit

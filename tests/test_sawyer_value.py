"""Discount and a terminal value net in the Sawyer door / peg planners (include/earl_physics.h, "discount and a terminal value on the door and the peg":
earl_sawyer_branch_rollout_value, earl_sawyer_plan_mppi_value, earl_sawyer_plan_cem_value, earl_sawyer_value_ws_bytes, earl_sawyer_value_terminal_cpu), what can be held
without a GPU:
  1. the host twin of the value kernel (earl_sawyer_value_terminal_cpu: csrc/sawyer_value.h, the header the kernel uses) against numpy float64 and
     earl_mlp_policy_forward_cpu on the float32 rows -- 14 -> 16 -> 1, 14 -> 256 -> 1, 14 -> 64 -> 64 -> 1, both activations, both output activations, rows = 7 with one NaN
     row (which gives NaN whatever the network) -- and d_H for H = 1, 7, 300 against the Python recurrence;
  2. the three entry points' refusals before the device (host stand-in pointers, as tests/test_sawyer_plan.py does): wrong widths, a head's width, precision != 0, a bad
     discount, a small or misaligned workspace; pv = NULL and {1.0, NULL} are the value-free calls;
  3. earl_sawyer_value_ws_bytes: 0 without work, monotone in K, H and n, at least earl_sawyer_plan_ws_bytes;
  4. the Python front end: its argument errors, and the minitaur and the kitchen still refuse when the new keywords are passed;
  5. the build: the value kernel without scratch, the discounted rollout kernels with no more VGPRs, LDS or scratch than the branch kernels they copy and none of it in a
     timestep loop.
The GPU side is tests/test_sawyer_value_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import kernel_build
import sawyer_cem_helpers as sc
import sawyer_plan_helpers as sp
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, variant
from test_physics_abi import EARL_ERR_ARG, host_ptr, sawyer_args
from test_sawyer_policy_rollout import forward_cpu, pack, random_layers

F32, F64 = np.float32, np.float64
GAMMA = 0.9                      # inexact in binary: the order of operations shows
NETS = [(14, 16, 1), (14, 256, 1), (14, 64, 64, 1)]


def discount_H(gamma, H):
  d = 1.0
  for _ in range(H):
    d = d * gamma
  return d


def value_struct(layers, hidden_act, out_act):
  """(struct earl_mlp_policy over 16-byte aligned host memory, what to keep alive)"""
  st, flat = pack(layers, hidden_act, out_act)
  return st, aligned_params(st, flat)


def rows_with_a_nan(rows, seed):
  obs = np.random.default_rng(seed).uniform(-1.0, 1.0, (rows, 14))
  obs[:, 7:] += 0.25                                                         # (doubles that are no float32: the rounding shows)
  obs[rows // 2, 5] = np.nan
  return obs


def expected_terminal(layers, hidden_act, out_act, gamma, H, obs, ret):
  """ret + d_H * (double)V in numpy float64, V from earl_mlp_policy_forward_cpu on the float32 rows; a row that holds a NaN gives NaN"""
  V = forward_cpu(layers, hidden_act, out_act, obs.astype(F32))[:, 0]
  term = F64(discount_H(gamma, H)) * V.astype(F64)
  want = ret + term
  want[np.isnan(obs).any(1)] = np.nan
  return want, V


# ---------------------------------------------------------------------------------------------------------------- 1. the host twin
@pytest.mark.parametrize('dims', NETS, ids=lambda d: '-'.join(map(str, d)))
@pytest.mark.parametrize('hidden_act', ['relu', 'tanh'])
@pytest.mark.parametrize('out_act', ['none', 'tanh'])
def test_host_twin_equals_numpy_and_the_policy_contract(dims, hidden_act, out_act):
  host = _abi.load_host()
  rows, H = 7, 6
  layers = random_layers(dims, 3, gain=1.5)
  obs = rows_with_a_nan(rows, 4)
  ret0 = np.random.default_rng(5).uniform(0.0, 3.0, rows)
  want, V = expected_terminal(layers, hidden_act, out_act, GAMMA, H, obs, ret0)
  assert len(np.unique(V[~np.isnan(obs).any(1)])) == rows - 1 and np.isnan(want).sum() == 1      # the rows differ; exactly the NaN row is NaN
  st, keep = value_struct(layers, hidden_act, out_act)
  pv = _abi.PlanValue(discount=GAMMA, value=C.pointer(st))
  ret = ret0.copy()
  assert host.earl_sawyer_value_terminal_cpu(C.byref(pv), H, rows, obs.ctypes.data, ret.ctypes.data) == _abi.EARL_OK, host.earl_last_error()
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(ret), nan)
  sp.same_bits(ret[~nan], want[~nan], f'ret of {dims} {hidden_act} {out_act}')
  assert not np.array_equal(ret[~nan], ret0[~nan])
  del keep


@pytest.mark.parametrize('H', [1, 7, 300])
def test_the_discount_of_the_terminal_term_is_the_recurrence(H):
  """ret = 0 and V = 1 exactly (a network of zero weights and an output bias of 1): the twin returns d_H itself"""
  host = _abi.load_host()
  layers = [(np.zeros((16, 14), F32), np.zeros(16, F32)), (np.zeros((1, 16), F32), np.ones(1, F32))]
  st, keep = value_struct(layers, 'relu', 'none')
  pv = _abi.PlanValue(discount=GAMMA, value=C.pointer(st))
  obs, ret = np.zeros((3, 14)), np.zeros(3)
  assert host.earl_sawyer_value_terminal_cpu(C.byref(pv), H, 3, obs.ctypes.data, ret.ctypes.data) == _abi.EARL_OK
  want = discount_H(GAMMA, H)
  assert want != GAMMA ** H or H == 1                                        # (pow rounds once: the recurrence is what is defined)
  sp.same_bits(ret, np.full(3, want), f'd_H for H = {H}')
  del keep


def test_host_twin_without_a_network_and_its_refusals():
  host = _abi.load_host()
  obs, ret = np.zeros((2, 14)), np.array([1.5, 2.5])
  pv = _abi.PlanValue(discount=GAMMA, value=None)
  assert host.earl_sawyer_value_terminal_cpu(C.byref(pv), 4, 2, obs.ctypes.data, ret.ctypes.data) == _abi.EARL_OK and ret.tolist() == [1.5, 2.5]
  assert host.earl_sawyer_value_terminal_cpu(None, 4, 2, obs.ctypes.data, ret.ctypes.data) == EARL_ERR_ARG
  assert host.earl_sawyer_value_terminal_cpu(C.byref(pv), 4, 2, None, ret.ctypes.data) == EARL_ERR_ARG
  assert host.earl_sawyer_value_terminal_cpu(C.byref(pv), 4, 2, obs.ctypes.data, None) == EARL_ERR_ARG
  assert host.earl_sawyer_value_terminal_cpu(C.byref(pv), -1, 2, obs.ctypes.data, ret.ctypes.data) == EARL_ERR_ARG
  assert host.earl_sawyer_value_terminal_cpu(C.byref(pv), 4, -1, obs.ctypes.data, ret.ctypes.data) == EARL_ERR_ARG
  for bad in (0.0, -0.5, 1.5, float('nan'), float('inf')):
    assert host.earl_sawyer_value_terminal_cpu(C.byref(_abi.PlanValue(discount=bad, value=None)), 4, 2, obs.ctypes.data, ret.ctypes.data) == EARL_ERR_ARG, bad
  st, keep = value_struct(random_layers((14, 16, 4), 1), 'relu', 'none')     # a policy, not a value network
  assert host.earl_sawyer_value_terminal_cpu(C.byref(_abi.PlanValue(discount=1.0, value=C.pointer(st))), 4, 2, obs.ctypes.data, ret.ctypes.data) == EARL_ERR_ARG
  del keep


# ---------------------------------------------------------------------------------------------------------------- 2. refusals of the three entry points
MEAN = host_ptr(1 << 16)


def value_ws_bytes(lib, nv, K, H, n):
  need = C.c_int64(-1)
  rc = lib.earl_sawyer_value_ws_bytes(nv, K, H, n, C.byref(need))
  return rc, need.value


def ws_of(ws, ws_bytes_, ws_base=None):
  return None if ws is None else _abi.SawyerBranchWs(base=(host_ptr() if ws_base is None else ws_base) if ws == 'given' else None, bytes=ws_bytes_)


def call_branch(lib, nv, cfg, st, pv, K=2, H=3, ws='given', ws_bytes_=1 << 40, ws_base=None, ret=True):
  w = ws_of(ws, ws_bytes_, ws_base)
  summary = _abi.EpisodeSummary(ret=host_ptr() if ret else None, success_last=host_ptr(), first_success=host_ptr())
  return lib.earl_sawyer_branch_rollout_value(host_ptr(), None, nv, C.byref(cfg), C.byref(st), K, H, host_ptr(), H * cfg.n * 4, None, None if pv is None else C.byref(pv),
                                              None if w is None else C.byref(w), C.byref(summary), host_ptr(), host_ptr(), None)


def call_mppi(lib, nv, cfg, st, pv, ws='given', ws_bytes_=1 << 40, ws_base=None):
  w = ws_of(ws, ws_bytes_, ws_base)
  pp = sp.params(2, 3, I=1, sigma=0.3, inv_t=1.0)
  return lib.earl_sawyer_plan_mppi_value(host_ptr(), None, nv, C.byref(cfg), C.byref(st), C.byref(pp), None if pv is None else C.byref(pv), MEAN, host_ptr(1 << 16),
                                         host_ptr(), host_ptr(), host_ptr(), host_ptr(), host_ptr(), None, None if w is None else C.byref(w), None)


def call_cem(lib, nv, cfg, st, pv, ws='given', ws_bytes_=1 << 40, ws_base=None):
  w = ws_of(ws, ws_bytes_, ws_base)
  cp = sc.params(2, 3, I=1, E=1)
  al = lambda q: q + (-q % 16)
  return lib.earl_sawyer_plan_cem_value(host_ptr(), None, nv, C.byref(cfg), C.byref(st), C.byref(cp), None if pv is None else C.byref(pv), MEAN, None,
                                        al(host_ptr(1 << 16)), al(host_ptr(1 << 16)), host_ptr(), host_ptr(), host_ptr(), host_ptr(), host_ptr(), host_ptr(), None,
                                        None if w is None else C.byref(w), None)


CALLS = {'branch': call_branch, 'mppi': call_mppi, 'cem': call_cem}


@pytest.mark.parametrize('which', sorted(CALLS))
@pytest.mark.parametrize('nv', [10, 15])
def test_every_refusal_fires_before_the_device(which, nv):
  """n = 4 and K = 2: an accepted call would launch, so every EARL_ERR_ARG below was decided on the host"""
  lib, call = _abi.load(), CALLS[which]
  cfg, st, _ = sawyer_args(n=4, nv=nv)
  good, keep = value_struct(random_layers((14, 64, 64, 1), 2), 'tanh', 'none')
  nan, inf = float('nan'), float('inf')
  for bad in (0.0, -0.9, 1.0000001, nan, inf, -inf):
    assert call(lib, nv, cfg, st, _abi.PlanValue(discount=bad, value=None)) == EARL_ERR_ARG, bad
    assert call(lib, nv, cfg, st, _abi.PlanValue(discount=bad, value=C.pointer(good))) == EARL_ERR_ARG, bad
  nets = dict(a_policy=variant(good, dims=(14, 64, 64, 4)), a_head=variant(good, dims=(14, 64, 64, 2)), wide_input=variant(good, dims=(12, 64, 64, 1)),
              odd_hidden=variant(good, dims=(14, 24, 64, 1)), too_wide=variant(good, dims=(14, 272, 64, 1)), too_narrow=variant(good, dims=(14, 64, 0, 1)),
              bf16=variant(good, precision=_abi.PRECISION_BF16), precision_7=variant(good, precision=7), four_layers=variant(good, n_layers=4),
              one_layer=variant(good, n_layers=1), hidden_act=variant(good, hidden_act=_abi.ACTIVATIONS['none']), out_act=variant(good, out_act=9),
              no_params=variant(good, params=None), misaligned=variant(good, params=good.params + 4), unused_dim=variant(good, n_layers=2, dims=(14, 64, 1, 5)))
  for name, net in nets.items():
    for gamma in (1.0, GAMMA):
      assert call(lib, nv, cfg, st, _abi.PlanValue(discount=gamma, value=C.pointer(net))) == EARL_ERR_ARG, (name, gamma)
  # the workspace block is earl_sawyer_value_ws_bytes': too small, NULL, misaligned
  H = 0 if which == 'branch' else 3
  need = value_ws_bytes(lib, nv, 2, H, 4)[1]
  for pv in (_abi.PlanValue(discount=GAMMA, value=None), _abi.PlanValue(discount=1.0, value=C.pointer(good)), _abi.PlanValue(discount=GAMMA, value=C.pointer(good))):
    assert need > 0 and call(lib, nv, cfg, st, pv, ws_bytes_=need - 1) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, pv, ws='null base') == EARL_ERR_ARG and call(lib, nv, cfg, st, pv, ws=None) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, pv, ws_base=host_ptr(1 << 16) + 4) == EARL_ERR_ARG
  if which == 'branch':
    assert call(lib, nv, cfg, st, _abi.PlanValue(discount=GAMMA, value=C.pointer(good)), ret=False) == EARL_ERR_ARG      # a network with nothing to add to
  # what the value-free entry point refuses is still refused
  c2, s2, _ = sawyer_args(n=4, nv=nv)
  s2.qpos = None
  assert call(lib, nv, c2, s2, _abi.PlanValue(discount=GAMMA, value=C.pointer(good))) == EARL_ERR_ARG
  assert call(lib, 12, cfg, st, _abi.PlanValue(discount=GAMMA, value=C.pointer(good))) == EARL_ERR_ARG
  # the 64-lane switch refuses, as it refuses the value-free calls
  assert lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
  try:
    assert call(lib, nv, cfg, st, _abi.PlanValue(discount=GAMMA, value=C.pointer(good))) == EARL_ERR_ARG
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK
  del keep


@pytest.mark.parametrize('which', sorted(CALLS))
def test_the_empty_call_and_the_value_free_forms(which):
  lib, call = _abi.load(), CALLS[which]
  good, keep = value_struct(random_layers((14, 16, 1), 2), 'relu', 'tanh')
  zero, zst, _ = sawyer_args(n=0, nv=10)
  for pv in (None, _abi.PlanValue(discount=1.0, value=None), _abi.PlanValue(discount=GAMMA, value=C.pointer(good))):
    assert call(lib, 10, zero, zst, pv) == _abi.EARL_OK
    assert call(lib, 10, zero, zst, pv, ws='null base', ws_bytes_=0) == _abi.EARL_OK       # (no virtual env: no block needed)
  # pv = NULL and {1.0, NULL} ARE the value-free call: its workspace size is enough for them, and not for a call that discounts
  cfg, st, _ = sawyer_args(n=4, nv=10)
  need = C.c_int64(0)
  if which == 'branch':
    assert lib.earl_sawyer_branch_ws_bytes(10, 2, 4, C.byref(need)) == _abi.EARL_OK
    assert call(lib, 10, cfg, st, _abi.PlanValue(discount=GAMMA, value=None), H=0, ws_bytes_=1 << 40) == _abi.EARL_OK     # H == 0: nothing launched
  else:
    assert lib.earl_sawyer_plan_ws_bytes(10, 2, 3, 4, C.byref(need)) == _abi.EARL_OK
  assert call(lib, 10, cfg, st, _abi.PlanValue(discount=GAMMA, value=None), ws_bytes_=need.value) == EARL_ERR_ARG
  del keep


# ---------------------------------------------------------------------------------------------------------------- 3. the size function
def test_value_workspace_size_is_monotone_and_holds_the_planner_block():
  lib = _abi.load()
  for nv in (10, 15):
    for g in ((0, 3, 7), (7, 3, 0), (0, 0, 0), (0, 0, 5)):
      assert value_ws_bytes(lib, nv, *g) == (_abi.EARL_OK, 0)
    grid = [(K_, H_, n_) for K_ in (1, 2, 65, 8192) for H_ in (0, 1, 2, 20) for n_ in (1, 5, 64)]
    sizes = {g: value_ws_bytes(lib, nv, *g) for g in grid}
    assert all(rc == _abi.EARL_OK and b > 0 for rc, b in sizes.values())
    for a, (_, b) in sizes.items():
      plan, branch = C.c_int64(-1), C.c_int64(-1)
      assert lib.earl_sawyer_plan_ws_bytes(nv, *a, C.byref(plan)) == _abi.EARL_OK and lib.earl_sawyer_branch_ws_bytes(nv, a[0], a[2], C.byref(branch)) == _abi.EARL_OK
      assert b >= plan.value and b >= branch.value + a[0] * a[2] * 8 + a[0] * a[1] * a[2] * 16 and b % 8 == 0, (nv, a, b)
      for a2, (_, b2) in sizes.items():
        if all(x2 >= x for x2, x in zip(a2, a)) and a2 != a:
          assert b2 > b, (nv, a, a2)
    assert value_ws_bytes(lib, nv, 1 << 15, 1, 1 << 16)[0] == EARL_ERR_ARG and value_ws_bytes(lib, nv, -1, 1, 4)[0] == EARL_ERR_ARG
    assert value_ws_bytes(lib, nv, 1, -1, 4)[0] == EARL_ERR_ARG and value_ws_bytes(lib, nv, 1, 1, -4)[0] == EARL_ERR_ARG
    assert lib.earl_sawyer_value_ws_bytes(nv, 1, 1, 1, None) == EARL_ERR_ARG
  assert value_ws_bytes(lib, 12, 3, 2, 5)[0] == EARL_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- 4. the Python front end
def bare(cls, n=3):
  import torch
  env = object.__new__(cls)                                                # (no GPU here: the argument errors need no state)
  env.num_envs, env.device, env.total_step_count = n, torch.device('cpu'), 0
  return env


def test_python_argument_errors():
  import torch
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  t = lambda layers: [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in layers]
  good = MLPPolicy(t(random_layers((14, 16, 1), 1)), 'relu', 'none', obs_dim=14, act_dim=1)
  bad_values = (MLPPolicy(t(random_layers((14, 16, 4), 1)), 'relu', 'none', obs_dim=14, act_dim=4),          # a policy of the env: width 14 -> 4
                MLPPolicy(t(random_layers((12, 16, 1), 1)), 'relu', 'none', obs_dim=12, act_dim=1),          # the tabletop's observation
                GaussianMLPPolicy(t(random_layers((14, 16, 2), 1)), obs_dim=14, act_dim=1),                  # a head
                MLPPolicy(t(random_layers((14, 16, 1), 1)), 'relu', 'none', obs_dim=14, act_dim=1, param_dtype=torch.bfloat16), 'a string')
  for cls in (SawyerDoor, SawyerPeg):
    env = bare(cls)
    mean, acts = torch.zeros(4, 3, 4), torch.zeros(2, 4, 3, 4)
    for name, args in (('rollout_branches', (acts,)), ('plan_mppi', (mean,)), ('plan_cem', (mean,))):
      for d in (0.0, -1.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match=name + '.*discount'):
          getattr(env, name)(*args, discount=d)
        with pytest.raises(ValueError, match=name + '.*discount'):
          getattr(env, name)(*args, discount=d, value=good)
      for v in bad_values:
        with pytest.raises(ValueError, match=name):
          getattr(env, name)(*args, discount=GAMMA, value=v)
    for method in ('mppi', 'cem'):
      with pytest.raises(ValueError, match='mpc_rollout.*discount'):
        env.mpc_rollout(2, horizon=4, method=method, discount=0.0)
      with pytest.raises(ValueError, match='mpc_rollout'):
        env.mpc_rollout(2, horizon=4, method=method, value=bad_values[0])
  cuda_like = bare(SawyerDoor)
  cuda_like.device = torch.device('meta')
  with pytest.raises(ValueError, match='rollout_branches.*the env on meta'):                                   # the env's device
    cuda_like.rollout_branches(torch.zeros(2, 4, 3, 4, device='meta'), value=good)


def test_the_envs_without_a_planner_refuse_the_new_keywords_too():
  from earl_benchmark_amd.envs.kitchen import Kitchen
  from earl_benchmark_amd.envs.minitaur import Minitaur
  from earl_benchmark_amd.envs.physics_env import PhysicsEnv
  for cls in (Minitaur, Kitchen):
    env = object.__new__(cls)
    for name in ('rollout_branches', 'plan_mppi', 'plan_cem', 'mpc_rollout'):
      assert getattr(cls, name) is getattr(PhysicsEnv, name)
      for kw in (dict(discount=GAMMA), dict(value=object()), dict(discount=GAMMA, value=object())):
        with pytest.raises(NotImplementedError, match=name + '.*' + cls.ENV):
          getattr(env, name)(None, **kw)


# ---------------------------------------------------------------------------------------------------------------- 5. the build
def test_resources_of_the_new_kernels():
  """the value kernel: no scratch, no LDS.  The discounted rollout kernels: the VGPRs, AGPRs, LDS, occupancy and scratch bytes of the branch kernels they copy, at most, and
  no scratch instruction inside a timestep loop (the branch kernels' own bar: tests/test_sawyer_branches.py).  The peg forms and the eight-wave door form of the BRANCH
  kernels hold scratch outside the timestep loop (156 / 264 / 196 bytes per lane on record); the discounted builds may hold as much and not a byte more."""
  got = kernel_build.units(['sawyer_value.hip', 'physics_branch_value.hip', 'physics_branch_value_w8.hip', 'physics_branch.hip', 'physics_branch_w8.hip'])
  val = got['sawyer_value.hip'].resources
  print(val)
  assert sorted(val) == ['sawyer_value_kernel'], sorted(val)
  assert val['sawyer_value_kernel']['scratch'] == 0 and val['sawyer_value_kernel']['lds'] == 0 and val['sawyer_value_kernel']['agpr'] == 0, val
  pairs = [('physics_branch_value.hip', 'physics_branch.hip', '<10, 16, false>'), ('physics_branch_value.hip', 'physics_branch.hip', '<15, 16, false>'),
           ('physics_branch_value.hip', 'physics_branch.hip', '<15, 16, true>'), ('physics_branch_value_w8.hip', 'physics_branch_w8.hip', '<10, 16, false>')]
  for unit, plain_unit, inst in pairs:
    now, was = got[unit].resources['sawyer_branch_rollout_kernel' + inst], got[plain_unit].resources['sawyer_branch_rollout_kernel' + inst]
    print(unit, inst, was, '->', now)
    assert now['vgpr'] <= was['vgpr'] and now['vgpr'] + now['agpr'] <= was['vgpr'] + was['agpr'], (unit, inst, was, now)
    assert now['lds'] <= was['lds'] and now['occupancy'] >= was['occupancy'] and now['scratch'] <= was['scratch'], (unit, inst, was, now)
  assert got['physics_branch_value.hip'].resources['sawyer_branch_rollout_kernel<10, 16, false>']['scratch'] == 0
  for unit, n_kernels in (('physics_branch_value.hip', 3), ('physics_branch_value_w8.hip', 1)):
    assert sorted(k.split('<')[0] for k in got[unit].resources) == ['sawyer_branch_rollout_kernel'] * n_kernels, sorted(got[unit].resources)
    lines = got[unit].scratch_report(('sawyer_branch_rollout_kernel',))
    assert len(lines) == n_kernels
    kernel_build.check_scratch_lines(lines, otherwise=('no scratch at all',))

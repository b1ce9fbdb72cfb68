"""Policy-prior branches of the Sawyer door / peg planners without a GPU (include/earl_physics.h, "policy-prior branches on the door and the peg"):
  1. the host twin earl_sawyer_prior_actions_cpu against numpy Philox + earl_mlp_policy_forward_cpu + clip (tests/sawyer_prior_helpers.py), widths 16 and 256-256,
     one and two hidden layers, sigma 0 and non-zero, MPPI's and CEM's draw word;
  2. every refusal of the three `_prior` entry points fires before the device (n = 4: an accepted call would launch); the empty call; branches == 0 forwards;
  3. the one size function;
  4. the Python front end's argument errors, and the envs without a planner;
  5. the build: the new units hold only the prior kernels, each within the figures of the closed-loop policy kernel of the same form, no scratch in a timestep loop.
The device side: tests/test_sawyer_prior_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import kernel_build
import sawyer_cem_helpers as sc
import sawyer_plan_helpers as sp
import sawyer_prior_helpers as spr
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, variant
from test_physics_abi import EARL_ERR_ARG, host_ptr, sawyer_args
from test_sawyer_policy_rollout import forward_cpu, pack, random_layers

F32, F64 = np.float32, np.float64
GAMMA = 0.9
NETS = [(14, 16, 4), (14, 256, 4), (14, 16, 16, 4), (14, 256, 256, 4)]


def policy_struct(layers, hidden_act, out_act):
  st, flat = pack(layers, hidden_act, out_act)
  return st, aligned_params(st, flat)


def prior_struct(policy, P, sigma=0.2, obs0='given', act=None):
  return _abi.SawyerPlanPrior(policy=None if policy is None else C.pointer(policy), branches=P, sigma=(C.c_float * 4)(*[float(v) for v in sp.sigma4(sigma)]),
                              obs0=host_ptr() if obs0 == 'given' else None, act=act)


# ---------------------------------------------------------------------------------------------------------------- 1. the host twin
@pytest.mark.parametrize('dims', NETS, ids=lambda d: '-'.join(map(str, d)))
@pytest.mark.parametrize('sigma', [0.0, (0.2, 0.1, 0.3, 0.5)], ids=['sigma0', 'sigma'])
@pytest.mark.parametrize('cem', [0, 1], ids=['mppi', 'cem'])
def test_host_twin_equals_numpy_philox_forward_cpu_and_clip(dims, sigma, cem):
  host = _abi.load_host()
  n, H, k, j, nc, seed, off = 7, 5, 6, 3, 0x9E3779B9, 0x0123456789ABCDEF, 3
  layers = random_layers(dims, 4, gain=1.5, last_gain=3.0)                   # (outputs beyond +-1: the clip shows)
  obs = np.random.default_rng(5).uniform(-1.0, 1.0, (H, n, 14))
  obs[..., 7:] += 0.25                                                       # (doubles that are no float32: the rounding shows)
  want = spr.rows_actions(layers, 'relu', 'none', obs, seed, off, k, j, nc, sigma, cem=bool(cem))
  st, keep = policy_struct(layers, 'relu', 'none')
  pr = prior_struct(st, 2, sigma)
  cfg = sp.cfg_of(n, off, seed)
  got = np.full((H, n, 4), np.nan, F32)
  assert host.earl_sawyer_prior_actions_cpu(C.byref(cfg), C.byref(pr), H, k, j, nc, cem, obs.ctypes.data, got.ctypes.data) == _abi.EARL_OK, host.earl_last_error()
  sp.same_bits(got, want, f'prior actions of {dims}')
  u = forward_cpu(layers, 'relu', 'none', obs.astype(F32).reshape(-1, 14)).reshape(H, n, 4)
  assert (np.abs(u) > 1).any() and (np.abs(got) <= 1).all()
  if np.all(np.asarray(sigma) == 0):
    sp.same_bits(got, np.clip(u, -1, 1), 'sigma = 0: the clipped policy output')
  else:
    other = np.full((H, n, 4), np.nan, F32)
    assert host.earl_sawyer_prior_actions_cpu(C.byref(cfg), C.byref(pr), H, k + 1, j, nc, cem, obs.ctypes.data, other.ctypes.data) == _abi.EARL_OK
    assert not np.array_equal(other, got)                                    # (the noise is keyed by the branch)
    flip = np.full((H, n, 4), np.nan, F32)
    assert host.earl_sawyer_prior_actions_cpu(C.byref(cfg), C.byref(pr), H, k, j, nc, 1 - cem, obs.ctypes.data, flip.ctypes.data) == _abi.EARL_OK
    assert not np.array_equal(flip, got)                                     # (and by the planner's draw word)
  del keep


def test_host_twin_refusals():
  host = _abi.load_host()
  st, keep = policy_struct(random_layers((14, 16, 4), 1), 'relu', 'tanh')
  cfg, obs, act = sp.cfg_of(2, 0, 1), np.zeros((3, 2, 14)), np.zeros((3, 2, 4), F32)
  call = lambda cfg_=cfg, pr=prior_struct(st, 1), H=3, k=1, j=0, o=obs.ctypes.data, a=act.ctypes.data: host.earl_sawyer_prior_actions_cpu(
      None if cfg_ is None else C.byref(cfg_), None if pr is None else C.byref(pr), H, k, j, 7, 0, o, a)
  assert call() == _abi.EARL_OK
  assert call(cfg_=None) == EARL_ERR_ARG and call(pr=None) == EARL_ERR_ARG and call(pr=prior_struct(None, 1)) == EARL_ERR_ARG
  assert call(o=None) == EARL_ERR_ARG and call(a=None) == EARL_ERR_ARG
  assert call(H=-1) == EARL_ERR_ARG and call(k=0) == EARL_ERR_ARG and call(k=8192) == EARL_ERR_ARG and call(j=-1) == EARL_ERR_ARG and call(j=256) == EARL_ERR_ARG
  assert call(pr=prior_struct(st, 1, sigma=-0.1)) == EARL_ERR_ARG and call(pr=prior_struct(st, 1, sigma=float('nan'))) == EARL_ERR_ARG
  assert call(pr=prior_struct(variant(st, dims=(14, 16, 3, 0)), 1)) == EARL_ERR_ARG and call(pr=prior_struct(variant(st, dims=(12, 16, 4, 0)), 1)) == EARL_ERR_ARG
  del keep


# ---------------------------------------------------------------------------------------------------------------- 2. refusals of the three entry points
MEAN = host_ptr(1 << 16)
al = lambda q: q + (-q % 16)
ACT = al(host_ptr(1 << 16))


def prior_ws_bytes(lib, nv, K, H, n):
  need = C.c_int64(-1)
  rc = lib.earl_sawyer_prior_ws_bytes(nv, K, H, n, C.byref(need))
  return rc, need.value


def ws_of(ws, ws_bytes_, ws_base=None):
  return None if ws is None else _abi.SawyerBranchWs(base=(host_ptr() if ws_base is None else ws_base) if ws == 'given' else None, bytes=ws_bytes_)


def ref(x):
  return None if x is None else C.byref(x)


def call_branch(lib, nv, cfg, st, pr, pv=None, K=3, H=3, ws='given', ws_bytes_=1 << 40, ws_base=None, act=ACT, stride=None, j=0):
  w = ws_of(ws, ws_bytes_, ws_base)
  summary = _abi.EpisodeSummary(ret=host_ptr(), success_last=host_ptr(), first_success=host_ptr())
  return lib.earl_sawyer_branch_rollout_prior(host_ptr(), None, nv, C.byref(cfg), C.byref(st), K, H, act, H * cfg.n * 4 if stride is None else stride, None, ref(pv), ref(pr),
                                              j, 7, ref(w), C.byref(summary), host_ptr(), host_ptr(), None)


def call_mppi(lib, nv, cfg, st, pr, pv=None, K=3, H=3, ws='given', ws_bytes_=1 << 40, ws_base=None, **_):
  w = ws_of(ws, ws_bytes_, ws_base)
  pp = sp.params(K, H, I=1, sigma=0.3, inv_t=1.0)
  return lib.earl_sawyer_plan_mppi_prior(host_ptr(), None, nv, C.byref(cfg), C.byref(st), C.byref(pp), ref(pv), ref(pr), MEAN, host_ptr(1 << 16),
                                         host_ptr(), host_ptr(), host_ptr(), host_ptr(), host_ptr(), None, ref(w), None)


def call_cem(lib, nv, cfg, st, pr, pv=None, K=3, H=3, ws='given', ws_bytes_=1 << 40, ws_base=None, **_):
  w = ws_of(ws, ws_bytes_, ws_base)
  cp = sc.params(K, H, I=1, E=1)
  return lib.earl_sawyer_plan_cem_prior(host_ptr(), None, nv, C.byref(cfg), C.byref(st), C.byref(cp), ref(pv), ref(pr), MEAN, None,
                                        al(host_ptr(1 << 16)), al(host_ptr(1 << 16)), host_ptr(), host_ptr(), host_ptr(), host_ptr(), host_ptr(), host_ptr(), None,
                                        ref(w), None)


CALLS = {'branch': call_branch, 'mppi': call_mppi, 'cem': call_cem}


@pytest.mark.parametrize('which', sorted(CALLS))
@pytest.mark.parametrize('nv', [10, 15])
def test_every_refusal_fires_before_the_device(which, nv):
  """n = 4, K = 3 and P = 1: an accepted call would launch, so every EARL_ERR_ARG below was decided on the host"""
  lib, call = _abi.load(), CALLS[which]
  cfg, st, _ = sawyer_args(n=4, nv=nv)
  good, keep = policy_struct(random_layers((14, 64, 64, 4), 2), 'tanh', 'tanh')
  assert call(lib, nv, cfg, st, None) == EARL_ERR_ARG and call(lib, nv, cfg, st, prior_struct(None, 1)) == EARL_ERR_ARG
  for P in (-1, 3, 4, 1 << 20):                                              # 0 .. K - 1 = 2
    assert call(lib, nv, cfg, st, prior_struct(good, P)) == EARL_ERR_ARG, P
  nets = dict(a_value_net=variant(good, dims=(14, 64, 64, 1)), a_head=variant(good, dims=(14, 64, 64, 8)), wide_input=variant(good, dims=(12, 64, 64, 4)),
              odd_hidden=variant(good, dims=(14, 24, 64, 4)), too_wide=variant(good, dims=(14, 272, 64, 4)), too_narrow=variant(good, dims=(14, 64, 0, 4)),
              bf16=variant(good, precision=_abi.PRECISION_BF16), precision_7=variant(good, precision=7), four_layers=variant(good, n_layers=4),
              one_layer=variant(good, n_layers=1), hidden_act=variant(good, hidden_act=_abi.ACTIVATIONS['none']), out_act=variant(good, out_act=9),
              no_params=variant(good, params=None), misaligned=variant(good, params=good.params + 4), unused_dim=variant(good, n_layers=2, dims=(14, 64, 4, 5)))
  for name, net in nets.items():
    for P in (0, 1):                                                         # (the struct's own rules hold with no prior branch too)
      assert call(lib, nv, cfg, st, prior_struct(net, P)) == EARL_ERR_ARG, (name, P)
  for bad in (-0.1, float('nan'), float('inf')):
    for P in (0, 1):
      assert call(lib, nv, cfg, st, prior_struct(good, P, sigma=(0.1, 0.1, bad, 0.1))) == EARL_ERR_ARG, bad
  assert call(lib, nv, cfg, st, prior_struct(good, 1, obs0=None)) == EARL_ERR_ARG
  # prior->act: misaligned, or over an input of the call
  assert call(lib, nv, cfg, st, prior_struct(good, 1, act=al(host_ptr()) + 4)) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, prior_struct(good, 1, act=MEAN if which != 'branch' else ACT + 16)) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, prior_struct(good, 1, act=al(good.params))) == EARL_ERR_ARG
  # what the `_value` call refuses
  for bad in (0.0, -0.9, 1.0000001, float('nan')):
    for P in (0, 1):
      assert call(lib, nv, cfg, st, prior_struct(good, P), pv=_abi.PlanValue(discount=bad, value=None)) == EARL_ERR_ARG, (bad, P)
  assert call(lib, nv, cfg, st, prior_struct(good, 1), pv=_abi.PlanValue(discount=GAMMA, value=C.pointer(good))) == EARL_ERR_ARG      # (a policy is no value network)
  # the workspace block is earl_sawyer_prior_ws_bytes': too small (the `_value` size is), NULL, misaligned
  H = 0 if which == 'branch' else 3
  need = prior_ws_bytes(lib, nv, 3, H, 4)[1]
  value_need = C.c_int64(0)
  assert lib.earl_sawyer_value_ws_bytes(nv, 3, H, 4, C.byref(value_need)) == _abi.EARL_OK and 0 < value_need.value < need
  for pv in (None, _abi.PlanValue(discount=GAMMA, value=None)):
    assert call(lib, nv, cfg, st, prior_struct(good, 1), pv=pv, ws_bytes_=need - 1) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, prior_struct(good, 1), pv=pv, ws_bytes_=value_need.value) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, prior_struct(good, 1), pv=pv, ws='null base') == EARL_ERR_ARG and call(lib, nv, cfg, st, prior_struct(good, 1), pv=pv, ws=None) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, prior_struct(good, 1), pv=pv, ws_base=host_ptr(1 << 16) + 4) == EARL_ERR_ARG
  if which == 'branch':
    assert call(lib, nv, cfg, st, prior_struct(good, 1), stride=0) == EARL_ERR_ARG                   # one block for all branches cannot take the prior's rows
    assert call(lib, nv, cfg, st, prior_struct(good, 1), stride=3 * 4 * 4 + 2) == EARL_ERR_ARG       # rows are 16-byte stores
    assert call(lib, nv, cfg, st, prior_struct(good, 1), stride=3 * 4 * 4 - 4) == EARL_ERR_ARG       # the branch launch's own rule
    assert call(lib, nv, cfg, st, prior_struct(good, 1), act=ACT + 4) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, prior_struct(good, 1), act=None) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, prior_struct(good, 1), j=-1) == EARL_ERR_ARG and call(lib, nv, cfg, st, prior_struct(good, 1), j=256) == EARL_ERR_ARG
    assert call(lib, nv, cfg, st, prior_struct(good, 1), K=-1) == EARL_ERR_ARG and call(lib, nv, cfg, st, prior_struct(good, 1), H=-1) == EARL_ERR_ARG
  # what the underlying call refuses is still refused
  c2, s2, _ = sawyer_args(n=4, nv=nv)
  s2.qpos = None
  assert call(lib, nv, c2, s2, prior_struct(good, 1)) == EARL_ERR_ARG
  assert call(lib, 12, cfg, st, prior_struct(good, 1)) == EARL_ERR_ARG
  # the 64-lane switch refuses, as it refuses the branch launch -- in either launch shape
  for shape in (2, 1):
    assert lib.earl_debug_set_sawyer_prior_launches(shape) == _abi.EARL_OK and lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
    try:
      assert call(lib, nv, cfg, st, prior_struct(good, 1)) == EARL_ERR_ARG
    finally:
      assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK and lib.earl_debug_set_sawyer_prior_launches(1) == _abi.EARL_OK
  del keep


@pytest.mark.parametrize('which', sorted(CALLS))
def test_the_empty_call_and_no_prior_branch_forwards(which):
  lib, call = _abi.load(), CALLS[which]
  good, keep = policy_struct(random_layers((14, 16, 4), 2), 'relu', 'tanh')
  zero, zst, _ = sawyer_args(n=0, nv=10)
  for P in (0, 1, 2):
    for pv in (None, _abi.PlanValue(discount=1.0, value=None), _abi.PlanValue(discount=GAMMA, value=None)):
      assert call(lib, 10, zero, zst, prior_struct(good, P), pv=pv) == _abi.EARL_OK
      assert call(lib, 10, zero, zst, prior_struct(good, P), pv=pv, ws='null base', ws_bytes_=0) == _abi.EARL_OK      # (no virtual env: no block needed)
  # branches == 0 IS the `_value` call (the plain call for pv NULL or {1.0, NULL}): that call's workspace is enough for it, and not for a call with a prior branch
  cfg, st, _ = sawyer_args(n=4, nv=10)
  need = C.c_int64(0)
  if which == 'branch':
    assert lib.earl_sawyer_branch_ws_bytes(10, 3, 4, C.byref(need)) == _abi.EARL_OK
    for pv in (None, _abi.PlanValue(discount=1.0, value=None)):
      assert call(lib, 10, cfg, st, prior_struct(good, 0, obs0=None), pv=pv, H=0, ws_bytes_=need.value) == _abi.EARL_OK      # H == 0: nothing launched
      assert call(lib, 10, cfg, st, prior_struct(good, 0, obs0=None), pv=pv, H=0, stride=0, ws_bytes_=need.value) == _abi.EARL_OK
    assert call(lib, 10, cfg, st, prior_struct(good, 0), pv=_abi.PlanValue(discount=GAMMA, value=None), H=0, ws_bytes_=need.value) == EARL_ERR_ARG      # the `_value` call's size rule
    assert lib.earl_sawyer_value_ws_bytes(10, 3, 0, 4, C.byref(need)) == _abi.EARL_OK
    assert call(lib, 10, cfg, st, prior_struct(good, 0), pv=_abi.PlanValue(discount=GAMMA, value=None), H=0, ws_bytes_=need.value) == _abi.EARL_OK
    assert call(lib, 10, cfg, st, prior_struct(good, 1), pv=_abi.PlanValue(discount=GAMMA, value=None), H=0, ws_bytes_=need.value) == EARL_ERR_ARG
    assert call(lib, 10, cfg, st, prior_struct(good, 1), H=0) == _abi.EARL_OK                          # H == 0 with a prior branch: checked, nothing launched
  else:
    assert lib.earl_sawyer_value_ws_bytes(10, 3, 3, 4, C.byref(need)) == _abi.EARL_OK
    assert call(lib, 10, cfg, st, prior_struct(good, 1), ws_bytes_=need.value) == EARL_ERR_ARG
    # (an accepted planner call launches: the forwarding itself is held on the device, tests/test_sawyer_prior_gpu.py)
    assert call(lib, 10, cfg, st, prior_struct(good, 0), pv=_abi.PlanValue(discount=0.0, value=None)) == EARL_ERR_ARG
  del keep


# ---------------------------------------------------------------------------------------------------------------- 3. the size function
def test_prior_workspace_size_is_monotone_and_holds_the_planner_block():
  lib = _abi.load()
  for nv in (10, 15):
    for g in ((0, 3, 7), (7, 3, 0), (0, 0, 0), (0, 0, 5)):
      assert prior_ws_bytes(lib, nv, *g) == (_abi.EARL_OK, 0)
    grid = [(K_, H_, n_) for K_ in (1, 2, 65, 8192) for H_ in (0, 1, 2, 20) for n_ in (1, 5, 64)]
    sizes = {g: prior_ws_bytes(lib, nv, *g) for g in grid}
    assert all(rc == _abi.EARL_OK and b > 0 for rc, b in sizes.values())
    for a, (_, b) in sizes.items():
      value, plan, branch = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
      assert lib.earl_sawyer_value_ws_bytes(nv, *a, C.byref(value)) == _abi.EARL_OK and lib.earl_sawyer_plan_ws_bytes(nv, *a, C.byref(plan)) == _abi.EARL_OK
      assert lib.earl_sawyer_branch_ws_bytes(nv, a[0], a[2], C.byref(branch)) == _abi.EARL_OK
      V = a[0] * a[2]
      # the `_value` block, a second work queue (two words per group of four virtual envs) and the planner's candidates
      assert b >= value.value + 8 * ((V + 3) // 4) and b >= plan.value and b % 8 == 0, (nv, a, b)
      assert b >= branch.value + V * 8 + 8 * ((V + 3) // 4) + a[0] * a[1] * a[2] * 16, (nv, a, b)
      for a2, (_, b2) in sizes.items():
        if all(x2 >= x for x2, x in zip(a2, a)) and a2 != a:
          assert b2 > b, (nv, a, a2)
    assert prior_ws_bytes(lib, nv, 1 << 15, 1, 1 << 16)[0] == EARL_ERR_ARG and prior_ws_bytes(lib, nv, -1, 1, 4)[0] == EARL_ERR_ARG
    assert prior_ws_bytes(lib, nv, 1, -1, 4)[0] == EARL_ERR_ARG and prior_ws_bytes(lib, nv, 1, 1, -4)[0] == EARL_ERR_ARG
    assert lib.earl_sawyer_prior_ws_bytes(nv, 1, 1, 1, None) == EARL_ERR_ARG
  assert prior_ws_bytes(lib, 12, 3, 2, 5)[0] == EARL_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- 4. the Python front end
def bare(cls, n=3):
  import torch
  env = object.__new__(cls)                                                  # (no GPU here: the argument errors need no state)
  env.num_envs, env.device, env.total_step_count = n, torch.device('cpu'), 0
  return env


def test_python_argument_errors():
  import torch
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  t = lambda layers: [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in layers]
  good = MLPPolicy(t(random_layers((14, 16, 4), 1)), 'relu', 'tanh', obs_dim=14, act_dim=4)
  bad_priors = (MLPPolicy(t(random_layers((14, 16, 1), 1)), 'relu', 'none', obs_dim=14, act_dim=1),          # a value network
                MLPPolicy(t(random_layers((12, 16, 3), 1)), 'relu', 'none', obs_dim=12, act_dim=3),          # the tabletop's policy
                GaussianMLPPolicy(t(random_layers((14, 16, 8), 1)), obs_dim=14, act_dim=4),                  # a head
                MLPPolicy(t(random_layers((14, 16, 4), 1)), 'relu', 'none', obs_dim=14, act_dim=4, param_dtype=torch.bfloat16), 'a string')
  for cls in (SawyerDoor, SawyerPeg):
    env = bare(cls)
    mean, acts = torch.zeros(4, 3, 4), torch.zeros(2, 4, 3, 4)
    cases = (('rollout_branches', (acts,), {}, 3), ('plan_mppi', (mean,), dict(K=4), 4), ('plan_cem', (mean,), dict(K=4, elites=2), 4),
             ('mpc_rollout', (2,), dict(horizon=4, K=4), 4), ('mpc_rollout', (2,), dict(horizon=4, K=4, method='cem', elites=2), 4))
    for name, args, kw, K in cases:
      with pytest.raises(ValueError, match=name + '.*prior_branches = 1 without a prior'):
        getattr(env, name)(*args, prior_branches=1, **kw)
      for p in bad_priors:
        with pytest.raises(ValueError, match=name):
          getattr(env, name)(*args, prior=p, prior_branches=1, **kw)
      for P in (-1,) if name == 'rollout_branches' else (-1, K, K + 3):          # (rollout_branches: K is len(actions) + P, so only a negative P is out of range)
        with pytest.raises(ValueError, match=name + '.*prior_branches'):
          getattr(env, name)(*args, prior=good, prior_branches=P, **kw)
      for s in (-0.1, float('nan'), float('inf'), (0.1, 0.2), (0.1, 0.1, 0.1, -1.0)):
        with pytest.raises(ValueError, match=name + '.*prior_sigma'):
          getattr(env, name)(*args, prior=good, prior_branches=1, prior_sigma=s, **kw)
    with pytest.raises(ValueError, match='rollout_branches.*K='):
      env.rollout_branches(torch.zeros(4, 3, 4), K=3, prior=good, prior_branches=1)
    with pytest.raises(ValueError, match='rollout_branches.*iteration'):
      env.rollout_branches(acts, prior=good, prior_branches=1, iteration=256)
    with pytest.raises(ValueError, match=r'rollout_branches.*\[K - P, H, N, 4\]'):
      env.rollout_branches(torch.zeros(2, 4, 5, 4), prior=good, prior_branches=1)
  cuda_like = bare(SawyerDoor)
  cuda_like.device = torch.device('meta')
  with pytest.raises(ValueError, match='plan_mppi.*the env on meta'):                                          # the env's device
    cuda_like.plan_mppi(torch.zeros(4, 3, 4, device='meta'), K=4, prior=good, prior_branches=1)


def test_the_envs_without_a_planner_refuse_the_new_keywords_too():
  from earl_benchmark_amd.envs.kitchen import Kitchen
  from earl_benchmark_amd.envs.minitaur import Minitaur
  from earl_benchmark_amd.envs.physics_env import PhysicsEnv
  for cls in (Minitaur, Kitchen):
    env = object.__new__(cls)
    for name in ('rollout_branches', 'plan_mppi', 'plan_cem', 'mpc_rollout'):
      assert getattr(cls, name) is getattr(PhysicsEnv, name)
      for kw in (dict(prior=object()), dict(prior_branches=2), dict(prior=object(), prior_branches=2, prior_sigma=0.1), dict(noise_counter=3, iteration=1)):
        with pytest.raises(NotImplementedError, match=name + '.*' + cls.ENV):
          getattr(env, name)(None, **kw)


def test_entry_points_are_declared_bound_and_exported():
  lib, host = _abi.load(), _abi.load_host()
  for name in ('earl_sawyer_prior_ws_bytes', 'earl_sawyer_branch_rollout_prior', 'earl_sawyer_plan_mppi_prior', 'earl_sawyer_plan_cem_prior'):
    assert name in _abi.SIGNATURES and getattr(lib, name).argtypes is not None
  assert 'earl_sawyer_prior_actions_cpu' in _abi.HOST_EXTRA_SIGNATURES and host.earl_sawyer_prior_actions_cpu.argtypes is not None
  assert C.sizeof(_abi.SawyerPlanPrior) == 48                                # pointer, int32, four floats (4 bytes of padding), two pointers
  # the launch-shape switch: 1 (the default) or 2 launches, nothing else
  assert 'earl_debug_set_sawyer_prior_launches' in _abi.SIGNATURES
  for bad in (0, 3, -1):
    assert lib.earl_debug_set_sawyer_prior_launches(bad) == EARL_ERR_ARG
  assert lib.earl_debug_set_sawyer_prior_launches(2) == _abi.EARL_OK and lib.earl_debug_set_sawyer_prior_launches(1) == _abi.EARL_OK


# ---------------------------------------------------------------------------------------------------------------- 5. the build
def test_resources_of_the_prior_kernels():
  """The prior kernels are the branch kernels with the closed loop's policy phase in the place of the action load: each form stays within the VGPRs + AGPRs, LDS and
  scratch bytes of sawyer_policy_rollout_kernel of the same form (physics.hip / physics_w8.hip, built from this tree), at no lower occupancy, and holds no scratch
  instruction inside a timestep loop.  On record (bytes of scratch per lane, prior <- policy): door 204 <- 252, peg 364 <- 492, peg time-sliced 492 <- 572, eight-wave
  door 448 <- 516; the one-wave door kernel's scratch is never touched by an instruction."""
  got = kernel_build.units(['physics_branch_prior.hip', 'physics_branch_prior_w8.hip', 'physics.hip', 'physics_w8.hip'])
  pairs = [('physics_branch_prior.hip', 'physics.hip', '<10, 16, false>'), ('physics_branch_prior.hip', 'physics.hip', '<15, 16, false>'),
           ('physics_branch_prior.hip', 'physics.hip', '<15, 16, true>'), ('physics_branch_prior_w8.hip', 'physics_w8.hip', '<10, 16, false>')]
  for unit, policy_unit, inst in pairs:
    now, was = got[unit].resources['sawyer_prior_rollout_kernel' + inst], got[policy_unit].resources['sawyer_policy_rollout_kernel' + inst]
    print(unit, inst, was, '->', now)
    assert now['vgpr'] <= was['vgpr'] and now['vgpr'] + now['agpr'] <= was['vgpr'] + was['agpr'], (unit, inst, was, now)
    assert now['lds'] <= was['lds'] and now['occupancy'] >= was['occupancy'] and now['scratch'] <= was['scratch'], (unit, inst, was, now)
  for unit, n_kernels in (('physics_branch_prior.hip', 3), ('physics_branch_prior_w8.hip', 1)):
    assert sorted(k.split('<')[0] for k in got[unit].resources) == ['sawyer_prior_rollout_kernel'] * n_kernels, sorted(got[unit].resources)
    lines = got[unit].scratch_report(('sawyer_prior_rollout_kernel',))
    assert len(lines) == n_kernels
    kernel_build.check_scratch_lines(lines, otherwise=('no scratch at all',))

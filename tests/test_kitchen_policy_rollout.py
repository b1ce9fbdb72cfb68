"""earl_kitchen_policy_rollout (include/earl_physics.h): the kitchen rollout with a float32 MLP policy 46 -> hidden (-> hidden) -> 9 evaluated inside the fused
rollout kernel.  What can be held without a GPU:
  1. the entry point is declared, bound and exported where it belongs;
  2. every argument error comes back before any HIP call;
  3. the Python refusals that need no launch;
  4. compile time: the plain kitchen kernels (kitchen_rollout_kernel<0 | 1 | 2>, the per-step kernels, physics_kernel<23, 32, *>) are byte-identical to the build
     before the policy kernels existed (tests/golden/kitchen_plain_kernels_asm.json: a digest per function of that build's gfx950 assembly, comment lines and label
     numbers aside); the policy kernels keep the plain kernels' occupancy and LDS and have no scratch instruction inside their timestep loops.
tests/test_kitchen_policy_rollout_gpu.py holds the launch itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, head, variant as variant_of
from test_sawyer_policy_rollout import pack, random_layers

CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')


# ---------------------------------------------------------------------------------------------------------------- 1. declared, bound, exported
def test_entry_point_is_declared_bound_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'int\s+earl_kitchen_policy_rollout\s*\((.*?)\)\s*;', src, flags=re.S)
  assert m, 'earl_kitchen_policy_rollout is not declared'
  assert len(m.group(1).split(',')) == len(_abi.SIGNATURES['earl_kitchen_policy_rollout']) == 13
  # the bound argument list is the clocked entry point's with `action` replaced by policy, head, obs0 and `actions` put before `out`
  clocked = _abi.SIGNATURES['earl_kitchen_rollout_clocked']
  bound = _abi.SIGNATURES['earl_kitchen_policy_rollout']
  assert bound[:5] == clocked[:5] and bound[8:10] == clocked[6:8] and bound[11:] == clocked[8:]
  assert bound[5]._type_ is _abi.MlpPolicy and bound[6]._type_ is _abi.GaussianHead and bound[7] is C.c_void_p and bound[10] is C.c_void_p
  assert src.index('earl_kitchen_rollout_clocked') < m.start() < src.index('earl_minitaur_rollout')      # next to the clocked entry point
  lib, host = _abi.load(), C.CDLL(_abi.HOST_LIB_PATH)
  assert hasattr(lib, 'earl_kitchen_policy_rollout') and not hasattr(host, 'earl_kitchen_policy_rollout')
  tt = open(os.path.join(REPO, 'include', 'earl_tabletop.h')).read()
  assert 'earl_kitchen_policy_rollout' in tt[tt.index('THE ARGUMENT CONTRACT'):tt.index('enum { EARL_ACT_NONE')]


# ---------------------------------------------------------------------------------------------------------------- 2. argument errors, no GPU
def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  layers = random_layers([46, 16, 9], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  aligned = aligned_params(pol, keep)
  buf = np.zeros(4096, np.float64)                                       # never read: every call below returns before any HIP call
  p = buf.ctypes.data
  params = _abi.KitchenParams()

  def cfg_of(**kw):
    d = dict(n=8, frame_skip=40, n_att=12, mocap_quat_dev=p)
    d.update(kw)
    site = d.pop('site_att', [0, 1, 2, 3, 4, 5, 6, 7])
    cfg = _abi.KitchenCfg(**d)
    cfg.site_att[:] = site
    return cfg

  def st_of(**kw):
    d = dict(qpos=p, qvel=p, mocap_pos=p, goal=p, last_qp_robot=p, att_xpos=p, steps_since_reset=p, last_obs=p)      # (fail_count and the step's scratch may be NULL)
    d.update(kw)
    return _abi.KitchenState(**d)

  def out_of(**kw):
    d = dict(obs=p, reward=p, done=p, success=p)                         # (status may be NULL)
    d.update(kw)
    return _abi.KitchenOut(**d)

  def variant(base=pol, **kw):
    return variant_of(base, **kw)

  cfg, st, out = cfg_of(), st_of(), out_of()

  def call(model=p, params=params, cfg=cfg, st=st, pol=pol, head=None, obs0=p, T=4, actions=p, out=out):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_kitchen_policy_rollout(model, None, ref(params), ref(cfg), ref(st), ref(pol), ref(head), obs0, T, None, actions, ref(out), None)

  pol18 = variant(dims=(46, 16, 18, 0))
  bad = [dict(pol=None), dict(obs0=None), dict(actions=None),
         # everything earl_kitchen_rollout_clocked refuses
         dict(model=None), dict(params=None), dict(cfg=None), dict(st=None), dict(out=None), dict(T=-1), dict(cfg=cfg_of(n=-1)),
         dict(cfg=cfg_of(n_att=9)), dict(cfg=cfg_of(n_att=33)), dict(cfg=cfg_of(frame_skip=-1)), dict(cfg=cfg_of(mocap_quat_dev=None)),
         dict(cfg=cfg_of(site_att=[0, 1, 2, 3, 4, 5, 6, 12])), dict(cfg=cfg_of(site_att=[-1, 1, 2, 3, 4, 5, 6, 7])),
         dict(st=st_of(qpos=None)), dict(st=st_of(qvel=None)), dict(st=st_of(mocap_pos=None)), dict(st=st_of(goal=None)), dict(st=st_of(last_qp_robot=None)),
         dict(st=st_of(att_xpos=None)), dict(st=st_of(steps_since_reset=None)), dict(st=st_of(last_obs=None)),
         dict(out=out_of(obs=None)), dict(out=out_of(reward=None)), dict(out=out_of(done=None)), dict(out=out_of(success=None)),
         # check_policy(*policy, 46, 9, head, kParamsAligned16)
         dict(pol=variant(dims=(45, 16, 9, 0))), dict(pol=variant(dims=(47, 16, 9, 0))), dict(pol=variant(dims=(32, 16, 9, 0))), dict(pol=variant(dims=(48, 16, 9, 0))),   # dims[0] != 46
         dict(pol=variant(dims=(46, 16, 8, 0))), dict(pol=variant(dims=(46, 16, 10, 0))), dict(pol=pol18), dict(pol=pol, head=head()),
         dict(pol=variant(dims=(46, 16, 16, 0)), head=head()),                                                           # the last layer
         dict(pol=variant(dims=(46, 24, 9, 0))), dict(pol=variant(dims=(46, 272, 9, 0))), dict(pol=variant(dims=(46, 0, 9, 0))), dict(pol=variant(dims=(46, 8, 9, 0))),
         dict(pol=variant(n_layers=3, dims=(46, 16, 24, 9))),                                                            # hidden widths
         dict(pol=variant(n_layers=1)), dict(pol=variant(n_layers=4)), dict(pol=variant(dims=(46, 16, 9, 1))),
         dict(pol=variant(precision=1)), dict(pol=variant(params=None)), dict(pol=variant(params=pol.params + 4)),      # (+ 4: no longer 16-byte aligned)
         dict(pol=variant(hidden_act=0)), dict(pol=variant(hidden_act=3)), dict(pol=variant(out_act=_abi.ACTIVATIONS['relu'])), dict(pol=variant(out_act=3)),
         dict(pol=pol18, head=head(mode=2)), dict(pol=pol18, head=head(m=2)), dict(pol=pol18, head=head(lo=-21.0)), dict(pol=pol18, head=head(hi=4.5)),
         dict(pol=pol18, head=head(lo=1.0, hi=0.0)), dict(pol=pol18, head=head(lo=float('nan')))]
  for kw in bad:
    assert call(**kw) == -1, kw
  cfg0 = cfg_of(n=0)
  assert call(cfg=cfg0) == 0 and call(cfg=cfg0, pol=pol18, head=head()) == 0     # n = 0: every check passed and nothing was launched (the arguments above are otherwise good)
  assert call(T=0) == 0 and call(T=0, pol=pol18, head=head()) == 0               # T = 0: as the plain entry point
  assert call(cfg=cfg0, pol=variant(n_layers=3, dims=(46, 144, 256, 9))) == 0
  # the reference clips silently: an unbounded policy is taken (the minitaur refuses it)
  assert call(cfg=cfg0, pol=variant(out_act=_abi.ACTIVATIONS['none'])) == 0
  assert call(cfg=cfg0, pol=variant(pol18, out_act=_abi.ACTIVATIONS['none']), head=head()) == 0
  # fail_count, status and the per-step scratch may be NULL, as for the plain entry point
  assert call(cfg=cfg0, st=st_of(fail_count=None), out=out_of(status=None)) == 0
  # the plain clocked entry point refuses the same env arguments
  for kw in bad[3:28]:
    a = dict(model=p, params=params, cfg=cfg, st=st, T=4, out=out)
    a.update(kw)
    ref = lambda s: None if s is None else C.byref(s)
    assert lib.earl_kitchen_rollout_clocked(a['model'], None, ref(a['params']), ref(a['cfg']), ref(a['st']), p, a['T'], None, ref(a['out']), None) == -1, kw
  del aligned, buf


# ---------------------------------------------------------------------------------------------------------------- 3. the Python surface without a launch
def test_python_refusals_need_no_gpu():
  from earl_benchmark_amd.envs.kitchen import Kitchen, _Cfg
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  layers = random_layers([46, 48, 9], seed=4)
  pi = MLPPolicy(layers, 'relu', 'none', obs_dim=46, act_dim=9)          # unbounded: taken
  assert pi.dims == [46, 48, 9] and list(pi.struct.dims) == [46, 48, 9, 0] and pi.params.numel() == 47 * 48 + 49 * 9
  g = GaussianMLPPolicy(random_layers([46, 16, 80, 18], seed=6), 'tanh', squash=False, obs_dim=46, act_dim=9)
  assert list(g.struct.dims) == [46, 16, 80, 18]
  env = Kitchen.__new__(Kitchen)                                         # (the env itself needs a GPU; its checks do not)
  env.device, env.scalar_api, env.num_envs, env._cfg = torch.device('cpu'), False, 4, _Cfg(n=4)
  assert env._check_policy(pi, 'rollout_policy') is False and env._check_policy(g, 'rollout_policy') is True
  with pytest.raises(ValueError, match='observation width 32 and action width 8; this env takes 46 and 9'):
    env._check_policy(MLPPolicy(random_layers([32, 16, 8], seed=0), obs_dim=32, act_dim=8), 'rollout_policy')
  with pytest.raises(ValueError, match='observation width 12 and action width 3; this env takes 46 and 9'):
    env.rollout_policy(MLPPolicy(random_layers([12, 16, 3], seed=0)), 3)
  with pytest.raises(ValueError, match='an MLPPolicy, a GaussianMLPPolicy'):
    env.rollout_policy(lambda obs: obs, 3)
  with pytest.raises(NotImplementedError, match='PolicyPopulation on the kitchen'):
    env.rollout_policy(PolicyPopulation([pi, pi], envs_per_policy=16, obs_dim=46, act_dim=9), 3)
  pair = AgentPair(pi, pi, backward_goal=None, obs_dim=46, act_dim=9)
  with pytest.raises(NotImplementedError, match='AgentPair on the kitchen'):
    env.rollout_policy(pair, 3)
  with pytest.raises(NotImplementedError, match='AgentPair on the kitchen'):
    env.rollout_agents(pair, 3)
  with pytest.raises(NotImplementedError, match='evaluate_policy.*on the kitchen'):
    env.evaluate_policy(pi, 3)
  with pytest.raises(ValueError, match='need a GaussianMLPPolicy'):
    env.rollout_policy(pi, 3, sample=False)
  with pytest.raises(ValueError, match='need a GaussianMLPPolicy'):
    env.rollout_policy(pi, 3, return_noise=True)
  with pytest.raises(ValueError, match='T = 0'):
    env.rollout_policy(pi, 0)
  env.scalar_api = True
  with pytest.raises(ValueError, match='scalar_api'):
    env.rollout_policy(pi, 3)
  env.scalar_api = False
  env._cfg.goal_change_frequency = 5
  with pytest.raises(ValueError, match='goal switch runs on the host'):
    env.rollout_policy(pi, 3)
  env._cfg.goal_change_frequency = 0
  env.device = torch.device('cuda', 0)
  with pytest.raises(ValueError, match='the policy is on cpu'):
    env.rollout_policy(pi, 3)
  # the other envs refuse the kitchen's widths by name
  from earl_benchmark_amd.envs.minitaur import Minitaur
  mt = Minitaur.__new__(Minitaur)
  mt.device = torch.device('cpu')
  with pytest.raises(ValueError, match='observation width 46 and action width 9; this env takes 32 and 8'):
    mt._check_policy(pi, 'rollout_policy')


# ---------------------------------------------------------------------------------------------------------------- 4. compile time
def test_plain_kitchen_kernels_are_byte_identical_to_the_build_before():
  want = kernel_build.recorded('kitchen_plain_kernels_asm.json', what='the digests')
  got = kernel_build.unit('physics_kitchen.hip').digests
  assert set(got) == set(want['functions']), sorted(set(got) ^ set(want['functions']))      # no policy kernel, no policy function in this unit
  names = ' '.join(want['functions'])
  for k in ('kitchen_rollout_kernelILi0E', 'kitchen_rollout_kernelILi1E', 'kitchen_rollout_kernelILi2E', 'kitchen_pre_kernel', 'kitchen_guard_kernel',
            'kitchen_finish_kernel', 'physics_kernelILi23ELi32ELb1E', 'physics_kernelILi23ELi32ELb0E'):
    assert k in names, k
  for name, lines_and_sha in want['functions'].items():
    assert got[name] == lines_and_sha, name


def test_policy_kernels_keep_the_plain_kernels_occupancy_lds_and_scratch_free_timestep_loops():
  """Measured: every form occupancy 1 and LDS 162,048 bytes; <1> and <2> no scratch instruction in the kernel at all, <0> none inside its timestep
  loop (the plain <0> likewise keeps a few outside it)"""
  plain_unit, policy_unit = kernel_build.unit('physics_kitchen.hip'), kernel_build.unit('physics_kitchen_policy.hip')
  assert 'kitchen_policy_rollout_kernel' in kernel_build.tool().KERNELS
  plain, policy = plain_unit.resources, policy_unit.resources
  for duo in (0, 1, 2):
    a, b = plain[f'kitchen_rollout_kernel<{duo}>'], policy[f'kitchen_policy_rollout_kernel<{duo}>']
    print(duo, a, b)
    assert (b['occupancy'], b['lds']) == (a['occupancy'], a['lds']), (duo, a, b)
    assert b['vgpr'] <= 256 and b['agpr'] <= 256
  assert not any('kitchen_rollout_kernel' in k for k in policy) and not any('policy' in k for k in plain)
  listing = policy_unit.scratch_report()
  assert len(listing) == 3 and all('kitchen_policy_rollout_kernel' in ln for ln in listing), listing
  # the rules of tests/test_no_scratch_in_timestep_loops.py
  kernel_build.check_scratch_lines(listing + plain_unit.scratch_report(), otherwise=('no scratch at all', 'no inner loop', 'no loop'))
  # the policy phase is a called function (nothing of it is live across a timestep) and adds no LDS
  asm = policy_unit.asm
  assert sum('s_swappc_b64' in ln for ln in asm) == 3                    # one call per kernel, in the env-step loop
  assert any(re.match(r'^_ZN\w*kitchen_policy_action\w*:', ln) for ln in asm)


def test_makefile_lists_the_units_and_the_inc():
  mk = open(os.path.join(CSRC, 'Makefile')).read()
  src = re.search(r'^SRC\s*=(.*)$', mk, flags=re.M).group(1).split()
  assert 'physics_kitchen.hip' in src and 'physics_kitchen_policy.hip' in src
  kitchen = re.search(r'^KITCHEN\s*=(.*)$', mk, flags=re.M).group(1).split()
  assert {'physics_env_kitchen.h', 'physics_env_kitchen_rollout.inc', 'policy_lane_group.h', 'policy_math.h', 'policy_check.h'} <= set(kitchen)
  for unit in ('physics_kitchen', 'physics_kitchen_policy'):
    assert re.search(rf'^{unit}\.o: {unit}\.hip \$\(PHYS\) \$\(KITCHEN\)$', mk, flags=re.M), unit

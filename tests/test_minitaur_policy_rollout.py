"""earl_minitaur_policy_rollout (include/earl_physics.h): the minitaur rollout with a float32 MLP policy 32 -> hidden (-> hidden) -> 8 evaluated inside either
rollout kernel.  What can be held without a GPU:
  1. the entry point is declared, bound and exported where it belongs;
  2. every argument error comes back before any HIP call;
  3. MLPPolicy / GaussianMLPPolicy with obs_dim=32, act_dim=8, and the tabletop and Sawyer paths refusing such a policy by its widths;
  4. compile time: the one-wave policy kernel keeps its timestep loop free of scratch and has the occupancy and LDS of minitaur_kernel<false, true>; the two-wave
     policy kernel has the occupancy and LDS of minitaur_duo_kernel and slot-loop scratch counts within the plain two-wave kernel's bounds.
tests/test_minitaur_policy_rollout_gpu.py holds the launch itself."""
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
from test_sawyer_policy_rollout import forward_cpu, pack, random_layers


# ---------------------------------------------------------------------------------------------------------------- 1. declared, bound, exported
def test_entry_point_is_declared_bound_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'int\s+earl_minitaur_policy_rollout\s*\((.*?)\)\s*;', src, flags=re.S)
  assert m, 'earl_minitaur_policy_rollout is not declared'
  assert len(m.group(1).split(',')) == len(_abi.SIGNATURES['earl_minitaur_policy_rollout']) == 12
  assert src.index('earl_minitaur_rollout_clocked') < m.start() < src.index('earl_minitaur_reset')      # next to the clocked entry point
  lib, host = _abi.load(), C.CDLL(_abi.HOST_LIB_PATH)
  assert hasattr(lib, 'earl_minitaur_policy_rollout') and not hasattr(host, 'earl_minitaur_policy_rollout')


# ---------------------------------------------------------------------------------------------------------------- 2. argument errors, no GPU
def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  layers = random_layers([32, 16, 8], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  aligned = aligned_params(pol, keep)
  buf = np.zeros(4096, np.float64)                                       # never read: every call below returns before any HIP call
  p = buf.ctypes.data

  def cfg_of(**kw):
    d = dict(n=8, num_substeps=5, n_goals=12, goal_table=p)
    d.update(kw)
    return _abi.MinitaurCfg(**d)

  def st_of(**kw):
    d = dict(qpos=p, qvel=p, goal=p, motor_param=p, observed_torque=p, overheat=p, motor_enabled=p)
    d.update(kw)
    return _abi.MinitaurState(**d)

  def out_of(**kw):
    d = dict(obs=p, reward=p, done=p, success=p)
    d.update(kw)
    return _abi.MinitaurOut(**d)

  def variant(base=pol, **kw):
    return variant_of(base, **kw)

  cfg, st, out = cfg_of(), st_of(), out_of()

  def call(model=p, cfg=cfg, st=st, pol=pol, head=None, obs0=p, T=4, actions=p, out=out):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_minitaur_policy_rollout(model, None, ref(cfg), ref(st), ref(pol), ref(head), obs0, T, None, actions, ref(out), None)

  pol16 = variant(dims=(32, 16, 16, 0))
  bad = [dict(pol=None), dict(obs0=None), dict(actions=None),
         # everything earl_minitaur_rollout_clocked refuses
         dict(model=None), dict(cfg=None), dict(st=None), dict(out=None), dict(T=-1), dict(cfg=cfg_of(n=-1)),
         dict(st=st_of(qpos=None)), dict(st=st_of(qvel=None)), dict(st=st_of(goal=None)), dict(st=st_of(motor_param=None)), dict(st=st_of(observed_torque=None)),
         dict(st=st_of(overheat=None)), dict(st=st_of(motor_enabled=None)),
         dict(out=out_of(obs=None)), dict(out=out_of(reward=None)), dict(out=out_of(done=None)), dict(out=out_of(success=None)),
         dict(cfg=cfg_of(goal_table=None)), dict(cfg=cfg_of(n_goals=0)), dict(cfg=cfg_of(num_substeps=-1)), dict(cfg=cfg_of(goal_change_frequency=5)),
         dict(pol=variant(dims=(30, 16, 8, 0))), dict(pol=variant(dims=(14, 16, 8, 0))), dict(pol=variant(dims=(33, 16, 8, 0))),               # dims[0] != 32
         dict(pol=variant(dims=(32, 16, 4, 0))), dict(pol=pol16), dict(pol=pol, head=head()), dict(pol=variant(dims=(32, 16, 12, 0)), head=head()),   # the last layer
         dict(pol=variant(dims=(32, 24, 8, 0))), dict(pol=variant(dims=(32, 272, 8, 0))), dict(pol=variant(dims=(32, 0, 8, 0))), dict(pol=variant(dims=(32, 8, 8, 0))),
         dict(pol=variant(n_layers=3, dims=(32, 16, 24, 8))),                                                            # hidden widths
         dict(pol=variant(n_layers=1)), dict(pol=variant(n_layers=4)), dict(pol=variant(dims=(32, 16, 8, 1))),
         dict(pol=variant(precision=1)), dict(pol=variant(params=None)), dict(pol=variant(params=pol.params + 4)),
         dict(pol=variant(hidden_act=0)), dict(pol=variant(hidden_act=3)),
         dict(pol=variant(out_act=_abi.ACTIVATIONS['none'])), dict(pol=variant(out_act=_abi.ACTIVATIONS['relu'])), dict(pol=variant(out_act=3)),   # bounded policies only
         dict(pol=variant(pol16, out_act=_abi.ACTIVATIONS['none']), head=head()),
         dict(pol=pol16, head=head(mode=2)), dict(pol=pol16, head=head(m=2)), dict(pol=pol16, head=head(lo=-21.0)), dict(pol=pol16, head=head(hi=4.5)),
         dict(pol=pol16, head=head(lo=1.0, hi=0.0)), dict(pol=pol16, head=head(lo=float('nan')))]                        # the head errors of the tabletop entry point
  for kw in bad:
    assert call(**kw) == -1, kw
  cfg0 = cfg_of(n=0)
  assert call(cfg=cfg0) == 0 and call(cfg=cfg0, pol=pol16, head=head()) == 0     # n = 0: every check passed and nothing was launched (the arguments above are otherwise good)
  assert call(T=0) == 0                                                          # T = 0: as the plain entry point
  assert call(cfg=cfg0, pol=variant(n_layers=3, dims=(32, 144, 256, 8))) == 0
  # the generic-stepper comparison build has no policy form
  assert lib.earl_debug_set_minitaur_stepper(0) == 0
  try:
    assert call(cfg=cfg0) == -1
  finally:
    assert lib.earl_debug_set_minitaur_stepper(1) == 0
  assert call(cfg=cfg0) == 0
  del aligned, buf


# ---------------------------------------------------------------------------------------------------------------- 3. the Python policy classes
def test_policy_classes_take_the_minitaur_widths_and_the_other_envs_refuse_them():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  layers = random_layers([32, 48, 8], seed=4)
  pi = MLPPolicy(layers, 'relu', 'tanh', obs_dim=32, act_dim=8)
  assert pi.dims == [32, 48, 8] and (pi.obs_dim, pi.act_dim) == (32, 8) and pi.params.numel() == 32 * 48 + 48 + 48 * 8 + 8
  assert list(pi.struct.dims) == [32, 48, 8, 0] and pi.macs == 32 * 48 + 48 * 8
  x = torch.as_tensor(np.random.default_rng(0).uniform(-1, 1, size=(6, 32)).astype(np.float32))
  np.testing.assert_allclose(pi(x).numpy(), forward_cpu(layers, 'relu', 'tanh', x.numpy()), rtol=0, atol=1e-5)      # (torch's summation order: close, not bit-identical)
  glayers = random_layers([32, 16, 144, 16], seed=6)
  g = GaussianMLPPolicy(glayers, 'tanh', squash=True, log_std_map='clamp', obs_dim=32, act_dim=8)
  assert g.dims == [32, 16, 144, 16] and list(g.struct.dims) == [32, 16, 144, 16] and g.params.numel() == 33 * 16 + 17 * 144 + 145 * 16
  assert tuple(g(x).shape) == (6, 8) and tuple(g.sample(x, torch.zeros(6, 8)).shape) == (6, 8)
  np.testing.assert_allclose(g(x).numpy(), forward_cpu(glayers, 'tanh', 'tanh', x.numpy(), head=(_abi.HEAD_MEAN, _abi.LOGSTD_CLAMP, -5.0, 2.0)), rtol=0, atol=1e-5)
  with pytest.raises(ValueError, match='the output is the 8-wide action, got width 7'):
    MLPPolicy(random_layers([32, 48, 7], seed=4), obs_dim=32, act_dim=8)
  with pytest.raises(ValueError, match='the output is the 16-wide mean and raw log_std of the action, got width 8'):
    GaussianMLPPolicy(layers, obs_dim=32, act_dim=8)
  # the tabletop's paths take 12 / 3 only, the Sawyer's 14 / 4, and say which widths they were given
  with pytest.raises(ValueError, match='observation width 32 and action width 8'):
    PolicyPopulation([pi, pi])
  with pytest.raises(ValueError, match='observation width 32 and action width 8'):
    AgentPair(pi, pi)
  _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=4, device='cpu', seed=3).get_envs()
  with pytest.raises(ValueError, match='observation width 32 and action width 8'):
    env.rollout_policy(pi, 5)
  with pytest.raises(ValueError, match='observation width 32 and action width 8'):
    env.evaluate_policy(pi, 5)
  door = SawyerDoor.__new__(SawyerDoor)                                  # (the Sawyer env itself needs a GPU; its width check does not)
  door.device = torch.device('cpu')
  with pytest.raises(ValueError, match='observation width 32 and action width 8; this env takes 14 and 4'):
    door._check_policy(pi, 'rollout_policy')


# ---------------------------------------------------------------------------------------------------------------- 4. compile time
def test_policy_kernels_keep_the_plain_kernels_occupancy_lds_and_scratch_bounds():
  """physics_mt.hip cross-compiled once with the tool's flags: register, LDS and scratch counts only.
  Measured: one-wave policy kernel no scratch instruction at all, occupancy 1, LDS 88,208; two-wave policy kernel 8 loads and 2 stores in its slot
  loop (plain: 12 and 3), occupancy 2, LDS 158,512"""
  unit, tool = kernel_build.unit('physics_mt.hip'), kernel_build.tool()
  assert 'minitaur_policy_kernel' in tool.KERNELS and not any('duo' in k and 'policy' in k for k in tool.KERNELS)
  default = unit.scratch_report()
  assert not any('minitaur_policy_duo_kernel' in ln for ln in default)   # the default listing keeps ONE slot-loop line
  assert sum('slot loop' in ln for ln in default) == 1
  one = [ln for ln in default if 'minitaur_policy_kernel<false, true>' in ln]
  assert len(one) == 1, default
  kernel_build.check_scratch_lines(one, otherwise=('no scratch at all',))
  duo = [ln for ln in unit.scratch_report(tool.KERNELS + tool.POLICY_DUO) if 'minitaur_policy_duo_kernel' in ln]
  assert len(duo) == 1 and 'slot loop' in duo[0], duo
  print(duo[0])
  m = re.search(r': (\d+) loads, (\d+) stores$', duo[0].rstrip())
  assert m and int(m.group(1)) <= 64 and int(m.group(2)) <= 8, duo[0]     # the bounds of tests/test_no_scratch_in_timestep_loops.py for the plain two-wave kernel
  res = {k: (v['occupancy'], v['lds']) for k, v in unit.resources.items()}
  assert res['minitaur_policy_kernel<false, true>'] == res['minitaur_kernel<false, true>'], res
  assert res['minitaur_policy_duo_kernel'] == res['minitaur_duo_kernel'], res

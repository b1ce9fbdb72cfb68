"""earl_minitaur_population_rollout (include/earl_physics.h) and Minitaur.rollout_population / evaluate_population, what can be held without a GPU:
  1. the entry point is declared, bound and exported where it belongs;
  2. every argument error, the population rows included, comes back before any HIP call, and the well-formed combinations (pop / summary / head / actions / out
     pointers each NULL or given) are accepted with n = 0;
  3. the Python refusals, by member and field, and the pinned refusals of rollout_policy(PolicyPopulation) / evaluate_policy;
  4. compile time: the plain minitaur kernels are byte-identical to the build before (tests/golden/population_parent_build.json), the policy kernels keep that build's
     occupancy and LDS, and have no scratch instruction inside a timestep loop (two-wave form: within the plain two-wave kernel's bounds).
tests/test_minitaur_population_gpu.py holds the launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_build
import population_no_gpu as shared
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, head, variant
from test_sawyer_policy_rollout import pack, random_layers

NAME = 'earl_minitaur_population_rollout'


def test_entry_point_is_declared_bound_and_exported():
  shared.declared(NAME, 14, 'earl_minitaur_policy_rollout', 'earl_minitaur_reset')


def test_argument_errors_and_well_formed_combinations_need_no_gpu():
  lib = _abi.load()
  layers = random_layers([32, 16, 8], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  aligned = aligned_params(pol, keep)
  count = 33 * 16 + 17 * 8
  buf = np.zeros(4096, np.float64)                                       # never read: every call below returns before any HIP call
  p = buf.ctypes.data

  def cfg_of(**kw):
    d = dict(n=40, num_substeps=5, n_goals=12, goal_table=p)
    d.update(kw)
    return _abi.MinitaurCfg(**d)

  def st_of(**kw):
    d = dict(qpos=p, qvel=p, goal=p, motor_param=p, observed_torque=p, overheat=p, motor_enabled=p, last_obs=p)
    d.update(kw)
    return _abi.MinitaurState(**d)

  def out_of(**kw):
    d = dict(obs=p, reward=p, done=p, success=p)
    d.update(kw)
    return _abi.MinitaurOut(**d)

  cfg, st, out = cfg_of(), st_of(), out_of()
  count16 = 33 * 16 + 17 * 16                                            # with the head's 16-wide last layer
  good_pop = shared.pop_struct(3, 16, count16)

  def call(model=p, cfg=cfg, st=st, pol=pol, pop=good_pop, head=None, obs0=p, T=4, actions=p, out=out, summary=None):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_minitaur_population_rollout(model, None, ref(cfg), ref(st), ref(pol), ref(pop), ref(head), obs0, T, None, actions, ref(out), ref(summary), None)

  pol16 = variant(pol, dims=(32, 16, 16, 0))
  bad = [dict(pol=None), dict(obs0=None),
         # everything earl_minitaur_policy_rollout refuses, but NULL actions / out pointers
         dict(model=None), dict(cfg=None), dict(st=None), dict(out=None), dict(T=-1), dict(cfg=cfg_of(n=-1)),
         dict(st=st_of(qpos=None)), dict(st=st_of(qvel=None)), dict(st=st_of(goal=None)), dict(st=st_of(motor_param=None)), dict(st=st_of(observed_torque=None)),
         dict(st=st_of(overheat=None)), dict(st=st_of(motor_enabled=None)),
         dict(cfg=cfg_of(goal_table=None)), dict(cfg=cfg_of(n_goals=0)), dict(cfg=cfg_of(num_substeps=-1)), dict(cfg=cfg_of(goal_change_frequency=5)),
         dict(pol=variant(pol, dims=(30, 16, 8, 0))), dict(pol=variant(pol, dims=(46, 16, 8, 0))), dict(pol=variant(pol, dims=(32, 16, 9, 0))), dict(pol=pol16),
         dict(pol=pol, head=head()), dict(pol=variant(pol, dims=(32, 24, 8, 0))), dict(pol=variant(pol, dims=(32, 272, 8, 0))),
         dict(pol=variant(pol, n_layers=3, dims=(32, 16, 24, 8))), dict(pol=variant(pol, n_layers=1)), dict(pol=variant(pol, n_layers=4)),
         dict(pol=variant(pol, precision=1)), dict(pol=variant(pol, params=None)), dict(pol=variant(pol, params=pol.params + 4)),
         dict(pol=variant(pol, hidden_act=0)), dict(pol=variant(pol, out_act=_abi.ACTIVATIONS['none'])), dict(pol=variant(pol, out_act=_abi.ACTIVATIONS['relu'])),
         dict(pol=pol16, head=head(mode=2)), dict(pol=pol16, head=head(m=2)), dict(pol=pol16, head=head(lo=-21.0)), dict(pol=pol16, head=head(lo=float('nan'))),
         # the carried row needs st->last_obs
         dict(out=out_of(obs=None), st=st_of(last_obs=None)),
         # the member range against the GLOBAL ids: 40 envs from id 9 on end in member 3 of 3
         dict(cfg=cfg_of(env_offset=9)), dict(cfg=cfg_of(env_offset=-1))]
  bad += [dict(pop=q) for q in shared.population_rows(count, 40)]
  for kw in bad:
    assert call(**kw) == -1, kw
  # well-formed: pop / summary / head / actions / every pointer of out, each NULL or given, n = 0 (nothing is launched)
  cfg0, none_out = cfg_of(n=0), _abi.MinitaurOut()
  for pop in (None, good_pop, shared.pop_struct(1, 32, count16 + 8)):
    for sm in shared.summaries(p):
      for hd, pl in ((None, pol), (head(), pol16)):
        for actions in (p, None):
          for o in (out, none_out, out_of(obs=None), out_of(reward=None, success=None), out_of(done=None, status=p)):
            assert call(cfg=cfg0, pop=pop, summary=sm, head=hd, pol=pl, actions=actions, out=o) == 0
  assert call(T=0) == 0 and call(T=0, out=none_out, actions=None) == 0
  assert call(cfg=cfg0, st=st_of(last_obs=None)) == 0                    # with out->obs the minitaur's last_obs may be NULL as ever
  assert call(cfg=cfg_of(n=0, env_offset=9)) == 0                        # (no env, no member needed)
  # the single-policy entry point keeps its own NULL checks
  ref = C.byref
  for a, o in ((None, out), (p, out_of(obs=None)), (p, out_of(reward=None)), (p, out_of(done=None)), (p, out_of(success=None))):
    assert lib.earl_minitaur_policy_rollout(p, None, ref(cfg0), ref(st), ref(pol), None, p, 4, None, a, ref(o), None) == -1
  # the generic-stepper comparison build has no policy form
  assert lib.earl_debug_set_minitaur_stepper(0) == 0
  try:
    assert call(cfg=cfg0) == -1
  finally:
    assert lib.earl_debug_set_minitaur_stepper(1) == 0
  assert call(cfg=cfg0) == 0
  del aligned, buf


def test_python_refusals_by_member_and_field():
  from earl_benchmark_amd.envs.minitaur import Minitaur, _Cfg
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  mk = lambda seed, **kw: MLPPolicy(random_layers([32, 16, 8], seed=seed), kw.pop('hact', 'relu'), kw.pop('out', 'tanh'), obs_dim=32, act_dim=8)
  pi = mk(0)
  pop = PolicyPopulation([mk(0), mk(1), mk(2)], envs_per_policy=16, obs_dim=32, act_dim=8)
  assert pop.stride % 4 == 0 and pop.n_policies == 3
  env = Minitaur.__new__(Minitaur)                                       # (the env itself needs a GPU; its checks do not)
  env.device, env.num_envs, env._cfg = torch.device('cpu'), 40, _Cfg(n=40, env_offset=3)
  assert env._check_policy(pop, 'rollout_population', population=True) is False and env._check_policy(pi, 'evaluate_population', population=True) is False
  # the pinned refusals stay
  with pytest.raises(NotImplementedError, match='PolicyPopulation on the minitaur'):
    env.rollout_policy(pop, 3)
  with pytest.raises(NotImplementedError, match='evaluate_policy.*on the minitaur'):
    env.evaluate_policy(pi, 3)
  with pytest.raises(ValueError, match='pop is a PolicyPopulation'):
    env.rollout_population(pi, 3)
  # a member range short of the global ids: 40 envs from id 9 on need member 3
  env._cfg.env_offset = 9
  with pytest.raises(ValueError, match='global env ids 9 .. 48 need members up to 3 of 3'):
    env.rollout_population(pop, 3)
  with pytest.raises(ValueError, match='need members up to 3 of 3'):
    env.evaluate_population(pop, 3)
  env._cfg.env_offset = 3
  # by field: a member of another architecture, activation or width
  with pytest.raises(ValueError, match='member 1 has hidden_act'):
    PolicyPopulation([mk(0), mk(1, hact='tanh')], obs_dim=32, act_dim=8)
  with pytest.raises(ValueError, match='member 2 has dims'):
    PolicyPopulation([mk(0), mk(1), MLPPolicy(random_layers([32, 48, 8], seed=3), 'relu', 'tanh', obs_dim=32, act_dim=8)], obs_dim=32, act_dim=8)
  with pytest.raises(ValueError, match='observation width 46 and action width 9'):
    PolicyPopulation([MLPPolicy(random_layers([46, 16, 9], seed=0), obs_dim=46, act_dim=9)], obs_dim=32, act_dim=8)
  with pytest.raises(ValueError, match='observation width 46 and action width 9; this env takes 32 and 8'):
    env.rollout_population(PolicyPopulation([MLPPolicy(random_layers([46, 16, 9], seed=0), obs_dim=46, act_dim=9)] * 3, obs_dim=46, act_dim=9), 3)
  with pytest.raises(ValueError, match='envs_per_policy = 8'):
    PolicyPopulation([mk(0)], envs_per_policy=8, obs_dim=32, act_dim=8)
  # bounded outputs only
  unb = PolicyPopulation([mk(0, out='none'), mk(1, out='none'), mk(2, out='none')], obs_dim=32, act_dim=8)
  with pytest.raises(ValueError, match='unbounded'):
    env.rollout_population(unb, 3)
  with pytest.raises(ValueError, match='unbounded'):
    env.evaluate_population(unb, 3)
  # sample / return_noise / T / episodes
  with pytest.raises(ValueError, match='population of GaussianMLPPolicy'):
    env.rollout_population(pop, 3, sample=False)
  with pytest.raises(ValueError, match='population of GaussianMLPPolicy'):
    env.rollout_population(pop, 3, return_noise=True)
  with pytest.raises(ValueError, match='T = 0'):
    env.rollout_population(pop, 0)
  with pytest.raises(ValueError, match='sample=True needs a Gaussian policy'):
    env.evaluate_population(pop, 3, sample=True)
  with pytest.raises(ValueError, match='both >= 1'):
    env.evaluate_population(pop, 0)
  with pytest.raises(ValueError, match='both >= 1'):
    env.evaluate_population(pi, 3, episodes=0)
  with pytest.raises(ValueError, match='one episode'):
    env.evaluate_population(pop, 3, episodes=2, reset_first=False)
  g = GaussianMLPPolicy(random_layers([32, 16, 16], seed=1), 'tanh', squash=True, obs_dim=32, act_dim=8)
  assert env._check_policy(PolicyPopulation([g, g, g], obs_dim=32, act_dim=8), 'evaluate_population', population=True) is True
  env.device = torch.device('cuda', 0)
  with pytest.raises(ValueError, match='the policy is on cpu'):
    env.evaluate_population(pop, 3)


def test_plain_kernels_are_byte_identical_and_the_policy_kernels_keep_their_resources():
  """physics_mt.hip cross-compiled once.  Measured: one-wave policy kernel 256 VGPR / 172 AGPR, no scratch instruction in the kernel, occupancy 1,
  LDS 88,208; two-wave policy kernel 10 loads and 3 stores in its slot loop (plain: 12 and 3), occupancy 2, LDS 158,512"""
  unit, tool = kernel_build.unit('physics_mt.hip'), kernel_build.tool()
  want = kernel_build.recorded('population_parent_build.json')
  got, res = unit.digests, unit.resources
  for name, lines_and_sha in want['minitaur_plain_functions'].items():
    assert got[name] == lines_and_sha, name
  assert {k for k in got if 'policy' not in k} == set(want['minitaur_plain_functions'])
  for k in ('minitaur_policy_kernel<false, true>', 'minitaur_policy_duo_kernel'):
    was, now = want['policy_kernel_resources'][k], res[k]
    print(k, was, '->', now)
    assert (now['occupancy'], now['lds']) == (was['occupancy'], was['lds']) and now['vgpr'] <= 256 and now['agpr'] <= 256
  lines = unit.scratch_report(tool.KERNELS + tool.POLICY_DUO)
  one = [ln for ln in lines if 'minitaur_policy_kernel<false, true>' in ln]
  duo = [ln for ln in lines if 'minitaur_policy_duo_kernel' in ln]
  assert len(one) == 1 and len(duo) == 1, lines
  print(duo[0])
  kernel_build.check_scratch_lines(one, otherwise=('no scratch at all',))
  import re
  m = re.search(r': (\d+) loads, (\d+) stores$', duo[0].rstrip())
  assert m and int(m.group(1)) <= 64 and int(m.group(2)) <= 8, duo[0]     # the bounds of tests/test_no_scratch_in_timestep_loops.py for the plain two-wave kernel

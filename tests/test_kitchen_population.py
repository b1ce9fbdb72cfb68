"""earl_kitchen_population_rollout (include/earl_physics.h) and Kitchen.rollout_population / evaluate_population, what can be held without a GPU:
  1. the entry point is declared, bound and exported where it belongs;
  2. every argument error, the population rows included, comes back before any HIP call, and the well-formed combinations (pop / summary / head / actions / out
     pointers each NULL or given) are accepted with n = 0;
  3. the Python refusals, by member and field, and the pinned refusals of rollout_policy(PolicyPopulation) / evaluate_policy;
  4. compile time: the policy kernels keep the occupancy and LDS of the build before (tests/golden/population_parent_build.json) and have no scratch instruction
     inside a timestep loop.  (The plain kernels' digests are tests/test_kitchen_policy_rollout.py's.)
tests/test_kitchen_population_gpu.py holds the launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_build
import population_no_gpu as shared
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, head, variant
from test_sawyer_policy_rollout import pack, random_layers

NAME = 'earl_kitchen_population_rollout'


def test_entry_point_is_declared_bound_and_exported():
  shared.declared(NAME, 15, 'earl_kitchen_policy_rollout', 'earl_minitaur_rollout')


def test_argument_errors_and_well_formed_combinations_need_no_gpu():
  lib = _abi.load()
  layers = random_layers([46, 16, 9], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  aligned = aligned_params(pol, keep)
  count, count18 = 47 * 16 + 17 * 9, 47 * 16 + 17 * 18
  buf = np.zeros(4096, np.float64)                                       # never read: every call below returns before any HIP call
  p = buf.ctypes.data
  params = _abi.KitchenParams()

  def cfg_of(**kw):
    d = dict(n=40, frame_skip=40, n_att=12, mocap_quat_dev=p)
    d.update(kw)
    site = d.pop('site_att', [0, 1, 2, 3, 4, 5, 6, 7])
    cfg = _abi.KitchenCfg(**d)
    cfg.site_att[:] = site
    return cfg

  def st_of(**kw):
    d = dict(qpos=p, qvel=p, mocap_pos=p, goal=p, last_qp_robot=p, att_xpos=p, steps_since_reset=p, last_obs=p)
    d.update(kw)
    return _abi.KitchenState(**d)

  def out_of(**kw):
    d = dict(obs=p, reward=p, done=p, success=p)
    d.update(kw)
    return _abi.KitchenOut(**d)

  cfg, st, out = cfg_of(), st_of(), out_of()
  good_pop = shared.pop_struct(3, 16, (count18 + 3) // 4 * 4)

  def call(model=p, params=params, cfg=cfg, st=st, pol=pol, pop=good_pop, head=None, obs0=p, T=4, actions=p, out=out, summary=None):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_kitchen_population_rollout(model, None, ref(params), ref(cfg), ref(st), ref(pol), ref(pop), ref(head), obs0, T, None, actions, ref(out),
                                               ref(summary), None)

  pol18 = variant(pol, dims=(46, 16, 18, 0))
  bad = [dict(pol=None), dict(obs0=None),
         # everything earl_kitchen_policy_rollout refuses, but NULL actions / out pointers
         dict(model=None), dict(params=None), dict(cfg=None), dict(st=None), dict(out=None), dict(T=-1), dict(cfg=cfg_of(n=-1)),
         dict(cfg=cfg_of(n_att=9)), dict(cfg=cfg_of(n_att=33)), dict(cfg=cfg_of(frame_skip=-1)), dict(cfg=cfg_of(mocap_quat_dev=None)),
         dict(cfg=cfg_of(site_att=[0, 1, 2, 3, 4, 5, 6, 12])), dict(cfg=cfg_of(site_att=[-1, 1, 2, 3, 4, 5, 6, 7])),
         dict(st=st_of(qpos=None)), dict(st=st_of(qvel=None)), dict(st=st_of(mocap_pos=None)), dict(st=st_of(goal=None)), dict(st=st_of(last_qp_robot=None)),
         dict(st=st_of(att_xpos=None)), dict(st=st_of(steps_since_reset=None)), dict(st=st_of(last_obs=None)), dict(st=st_of(last_obs=None), out=out_of(obs=None)),
         dict(pol=variant(pol, dims=(45, 16, 9, 0))), dict(pol=variant(pol, dims=(32, 16, 9, 0))), dict(pol=variant(pol, dims=(46, 16, 8, 0))), dict(pol=pol18),
         dict(pol=pol, head=head()), dict(pol=variant(pol, dims=(46, 24, 9, 0))), dict(pol=variant(pol, dims=(46, 272, 9, 0))),
         dict(pol=variant(pol, n_layers=3, dims=(46, 16, 24, 9))), dict(pol=variant(pol, n_layers=1)), dict(pol=variant(pol, n_layers=4)),
         dict(pol=variant(pol, precision=1)), dict(pol=variant(pol, params=None)), dict(pol=variant(pol, params=pol.params + 4)),
         dict(pol=variant(pol, hidden_act=0)), dict(pol=variant(pol, out_act=_abi.ACTIVATIONS['relu'])),
         dict(pol=pol18, head=head(mode=2)), dict(pol=pol18, head=head(m=2)), dict(pol=pol18, head=head(lo=-21.0)), dict(pol=pol18, head=head(lo=float('nan'))),
         # the member range against the GLOBAL ids: 40 envs from id 9 on end in member 3 of 3
         dict(cfg=cfg_of(env_offset=9)), dict(cfg=cfg_of(env_offset=-1))]
  bad += [dict(pop=q) for q in shared.population_rows(count, 40)]
  for kw in bad:
    assert call(**kw) == -1, kw
  # well-formed: pop / summary / head / actions / every pointer of out, each NULL or given, n = 0 (nothing is launched)
  cfg0, none_out = cfg_of(n=0), _abi.KitchenOut()
  for pop in (None, good_pop, shared.pop_struct(1, 32, count18 + 9 + 3 - (count18 + 9 + 3) % 4)):
    for sm in shared.summaries(p):
      for hd, pl in ((None, pol), (head(), pol18), (None, variant(pol, out_act=_abi.ACTIVATIONS['none']))):
        for actions in (p, None):
          for o in (out, none_out, out_of(obs=None), out_of(reward=None, success=None), out_of(done=None, status=p)):
            assert call(cfg=cfg0, pop=pop, summary=sm, head=hd, pol=pl, actions=actions, out=o) == 0
  assert call(T=0) == 0 and call(T=0, out=none_out, actions=None) == 0
  assert call(cfg=cfg_of(n=0, env_offset=9)) == 0                        # (no env, no member needed)
  assert call(cfg=cfg0, st=st_of(fail_count=None)) == 0
  # the single-policy entry point keeps its own NULL checks
  ref = C.byref
  for a, o in ((None, out), (p, out_of(obs=None)), (p, out_of(reward=None)), (p, out_of(done=None)), (p, out_of(success=None))):
    assert lib.earl_kitchen_policy_rollout(p, None, ref(params), ref(cfg0), ref(st), ref(pol), None, p, 4, None, a, ref(o), None) == -1
  del aligned, buf


def test_python_refusals_by_member_and_field():
  from earl_benchmark_amd.envs.kitchen import Kitchen, _Cfg
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  mk = lambda seed, **kw: MLPPolicy(random_layers([46, 16, 9], seed=seed), kw.pop('hact', 'relu'), kw.pop('out', 'none'), obs_dim=46, act_dim=9)
  pi = mk(0)
  pop = PolicyPopulation([mk(0), mk(1), mk(2)], envs_per_policy=16, obs_dim=46, act_dim=9)
  assert pop.stride % 4 == 0 and pop.stride > pop.n_params == 47 * 16 + 17 * 9      # 905 parameters: the row is padded to whole 16-byte pieces
  env = Kitchen.__new__(Kitchen)                                         # (the env itself needs a GPU; its checks do not)
  env.device, env.scalar_api, env.num_envs, env._cfg = torch.device('cpu'), False, 40, _Cfg(n=40, env_offset=3)
  assert env._check_policy(pop, 'rollout_population', population=True) is False and env._check_policy(pi, 'evaluate_population', population=True) is False
  # the pinned refusals stay
  with pytest.raises(NotImplementedError, match='PolicyPopulation on the kitchen'):
    env.rollout_policy(pop, 3)
  with pytest.raises(NotImplementedError, match='evaluate_policy.*on the kitchen'):
    env.evaluate_policy(pi, 3)
  with pytest.raises(ValueError, match='pop is a PolicyPopulation'):
    env.rollout_population(pi, 3)
  # a member range short of the global ids
  env._cfg.env_offset = 9
  with pytest.raises(ValueError, match='global env ids 9 .. 48 need members up to 3 of 3'):
    env.rollout_population(pop, 3)
  with pytest.raises(ValueError, match='need members up to 3 of 3'):
    env.evaluate_population(pop, 3)
  env._cfg.env_offset = 3
  # by field
  with pytest.raises(ValueError, match='member 1 has out_act'):
    PolicyPopulation([mk(0), mk(1, out='tanh')], obs_dim=46, act_dim=9)
  with pytest.raises(ValueError, match='member 2 has dims'):
    PolicyPopulation([mk(0), mk(1), MLPPolicy(random_layers([46, 48, 9], seed=3), 'relu', 'none', obs_dim=46, act_dim=9)], obs_dim=46, act_dim=9)
  with pytest.raises(ValueError, match='observation width 32 and action width 8; this env takes 46 and 9'):
    env.rollout_population(PolicyPopulation([MLPPolicy(random_layers([32, 16, 8], seed=0), obs_dim=32, act_dim=8)] * 3, obs_dim=32, act_dim=8), 3)
  # the env's own refusals
  env.scalar_api = True
  with pytest.raises(ValueError, match='scalar_api'):
    env.rollout_population(pop, 3)
  with pytest.raises(ValueError, match='scalar_api'):
    env.evaluate_population(pop, 3)
  env.scalar_api = False
  env._cfg.goal_change_frequency = 5
  with pytest.raises(ValueError, match='goal switch runs on the host'):
    env.rollout_population(pop, 3)
  with pytest.raises(ValueError, match='goal switch runs on the host'):
    env.evaluate_population(pi, 3)
  env._cfg.goal_change_frequency = 0
  # sample / return_noise / T / episodes
  with pytest.raises(ValueError, match='population of GaussianMLPPolicy'):
    env.rollout_population(pop, 3, sample=False)
  with pytest.raises(ValueError, match='T = 0'):
    env.rollout_population(pop, 0)
  with pytest.raises(ValueError, match='sample=True needs a Gaussian policy'):
    env.evaluate_population(pop, 3, sample=True)
  with pytest.raises(ValueError, match='both >= 1'):
    env.evaluate_population(pop, 3, episodes=0)
  with pytest.raises(ValueError, match='one episode'):
    env.evaluate_population(pop, 3, episodes=2, reset_first=False)
  g = GaussianMLPPolicy(random_layers([46, 16, 18], seed=1), 'tanh', squash=False, obs_dim=46, act_dim=9)
  assert env._check_policy(PolicyPopulation([g, g, g], obs_dim=46, act_dim=9), 'evaluate_population', population=True) is True
  env.device = torch.device('cuda', 0)
  with pytest.raises(ValueError, match='the policy is on cpu'):
    env.evaluate_population(pop, 3)


def test_policy_kernels_keep_their_occupancy_lds_and_scratch_free_timestep_loops():
  """physics_kitchen_policy.hip cross-compiled once.  Measured: every form occupancy 1 and LDS 162,048 bytes, no scratch instruction inside a
  timestep loop; <1> and <2> none in the kernel at all"""
  unit = kernel_build.unit('physics_kitchen_policy.hip')
  want, res = kernel_build.recorded('population_parent_build.json'), unit.resources
  for duo in (0, 1, 2):
    k = f'kitchen_policy_rollout_kernel<{duo}>'
    was, now = want['policy_kernel_resources'][k], res[k]
    print(k, was, '->', now)
    assert (now['occupancy'], now['lds']) == (was['occupancy'], was['lds']) and now['vgpr'] <= 256 and now['agpr'] <= 256
  listing = unit.scratch_report()
  assert len(listing) == 3, listing
  kernel_build.check_scratch_lines(listing, otherwise=('no scratch at all',))

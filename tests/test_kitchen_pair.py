"""earl_kitchen_agents_rollout (include/earl_physics.h) and Kitchen.rollout_pair / evaluate_pair, what can be held without a GPU:
  1. the entry point is declared after earl_kitchen_population_rollout, bound and exported from libearl_hip.so only; earl_kitchen_state.goal lost its const;
  2. every argument error comes back before any HIP call, and the well-formed combinations (pair with pop / goals / forward table / summary / head / actions / out
     pointers each NULL or given) are accepted with n = 0;
  3. the Python refusals by field, AgentPair / PairPopulation with the kitchen's widths and goal width, and the pinned refusal of rollout_agents;
  4. compile time: the plain kernels of physics_kitchen.hip are byte-identical to the build before (tests/golden/pair_parent_build.json); the policy kernels of
     physics_kitchen_policy.hip, which run the pair, keep that build's occupancy and LDS and have no scratch instruction inside a timestep loop.
tests/test_kitchen_pair_gpu.py holds the launches."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kernel_build
import population_no_gpu as shared
from conftest import REPO
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, head, variant
from test_minitaur_pair import declared, goals_struct, pair_rows, pair_struct
from test_sawyer_policy_rollout import pack, random_layers

NAME = 'earl_kitchen_agents_rollout'


def test_entry_point_is_declared_bound_and_exported():
  declared(NAME, 19, 'earl_kitchen_population_rollout', 'earl_minitaur_rollout')
  src = open(os.path.join(REPO, 'include', 'earl_physics.h')).read()
  assert re.search(r'\n  double\* goal; +/\* \[n, 23\].*written by earl_kitchen_agents_rollout only', src) and '23 on the kitchen' in src
  assert dict(_abi.KitchenState._fields_)['goal'] is C.c_void_p           # the layout is what it was


def test_argument_errors_and_well_formed_combinations_need_no_gpu():
  lib = _abi.load()
  layers = random_layers([46, 16, 9], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  aligned = aligned_params(pol, keep)
  count, count18 = 47 * 16 + 17 * 9, 47 * 16 + 17 * 18
  stride = (count18 + 3) // 4 * 4
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
  good_pair, good_pop = pair_struct(p, stride), shared.pop_struct(3, 16, 2 * stride)

  def call(model=p, params=params, cfg=cfg, st=st, pol=pol, pair=good_pair, pop=None, goals=None, fwd=p, n_fwd=2, head=None, obs0=p, T=4, actions=p, out=out, summary=None):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_kitchen_agents_rollout(model, None, ref(params), ref(cfg), ref(st), ref(pol), ref(pair), ref(pop), ref(goals), fwd, n_fwd, ref(head), obs0, T, None,
                                           actions, ref(out), ref(summary), None)

  pol18 = variant(pol, dims=(46, 16, 18, 0))
  with_goal = pair_struct(p, stride, goal=p)
  bad = [dict(pair=None),                                                # not an alias of the population entry point
         dict(pol=None), dict(obs0=None),
         # everything earl_kitchen_population_rollout refuses
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
         # the population of pairs: the member range against the GLOBAL ids, a member is two rows
         dict(pop=good_pop, cfg=cfg_of(env_offset=9)), dict(pop=good_pop, cfg=cfg_of(env_offset=-1)), dict(pop=shared.pop_struct(3, 16, 2 * stride - 4)),
         dict(pop=shared.pop_struct(3, 16, stride)),
         # the table of backward goals
         dict(goals=goals_struct(p, table=False)), dict(goals=goals_struct(p, n_rows=0)), dict(goals=goals_struct(p, n_rows=-3)), dict(goals=goals_struct(p), pair=with_goal),
         # a backward goal or table without a forward table: the forward goal could not be restored
         dict(pair=with_goal, fwd=None), dict(pair=with_goal, n_fwd=0), dict(pair=with_goal, fwd=None, n_fwd=0), dict(goals=goals_struct(p), fwd=None),
         dict(goals=goals_struct(p), n_fwd=0), dict(n_fwd=-1), dict(fwd=None, n_fwd=-1)]
  bad += [dict(pair=q) for q in pair_rows(p, count)]
  bad += [dict(pop=q) for q in shared.population_rows(2 * stride, 40)]
  for kw in bad:
    assert call(**kw) == -1, kw
  # well-formed: pair with pop / goals / forward table / summary / head / actions / every pointer of out / the pair's outputs, each NULL or given, n = 0
  cfg0, none_out = cfg_of(n=0), _abi.KitchenOut()
  backward = ((None, good_pair, None, 0), (None, good_pair, p, 2), (None, good_pair, None, 3), (None, with_goal, p, 1), (goals_struct(p), good_pair, p, 2),
              (goals_struct(p, n_rows=1, outs=False), pair_struct(p, stride, outs=False), p, 7))
  for pop in (None, good_pop, shared.pop_struct(1, 32, 2 * stride + 8)):
    for goals, pair, fwd, n_fwd in backward:
      for sm in shared.summaries(p):
        for hd, pl in ((None, pol), (head(), pol18), (None, variant(pol, out_act=_abi.ACTIVATIONS['none']))):
          for actions, o in ((p, out), (None, none_out), (p, out_of(obs=None)), (None, out_of(reward=None, success=None)), (p, out_of(done=None, status=p))):
            assert call(cfg=cfg0, pop=pop, goals=goals, pair=pair, fwd=fwd, n_fwd=n_fwd, summary=sm, head=hd, pol=pl, actions=actions, out=o) == 0
  assert call(T=0) == 0 and call(T=0, out=none_out, actions=None) == 0
  assert call(cfg=cfg_of(n=0, env_offset=9), pop=good_pop) == 0          # (no env, no member needed)
  assert call(cfg=cfg0, st=st_of(fail_count=None)) == 0
  del aligned, buf


def test_python_refusals_and_the_pair_classes():
  from earl_benchmark_amd.envs.kitchen import Kitchen, _Cfg
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy, PairPopulation
  mk = lambda seed, **kw: MLPPolicy(random_layers([46, 16, 9], seed=seed), kw.pop('hact', 'relu'), kw.pop('out', 'none'), obs_dim=46, act_dim=9)
  pair = AgentPair(mk(0), mk(1), switch_every=(3, 2), backward_goal='initial_states', obs_dim=46, act_dim=9)
  assert pair.goal_dim == 23 and pair.stride % 4 == 0 and pair.stride > pair.n_params == 47 * 16 + 17 * 9 and pair.backward_goal == 'initial_states'
  one = AgentPair(mk(0), mk(1), backward_goal=np.arange(23.0), obs_dim=46, act_dim=9)
  assert tuple(one.backward_goal.shape) == (23,) and one.backward_goals is None
  tab = AgentPair(mk(0), mk(1), backward_goal=np.zeros((4, 23)), obs_dim=46, act_dim=9)
  assert tab.backward_goal is None and tuple(tab.backward_goals.shape) == (4, 23)
  with pytest.raises(ValueError, match='ONE goal row of 23 values, got 7'):
    AgentPair(mk(0), mk(1), backward_goal=np.zeros(7), obs_dim=46, act_dim=9)
  with pytest.raises(ValueError, match='observation width 32 and action width 8'):
    AgentPair(MLPPolicy(random_layers([32, 16, 8], seed=0), obs_dim=32, act_dim=8), MLPPolicy(random_layers([32, 16, 8], seed=1), obs_dim=32, act_dim=8), obs_dim=46, act_dim=9)
  pop = PairPopulation([pair] + [AgentPair(mk(2 * k), mk(2 * k + 1), switch_every=(3, 2), backward_goal='initial_states', obs_dim=46, act_dim=9) for k in (1, 2)])
  assert (pop.obs_dim, pop.act_dim, pop.n_policies) == (46, 9, 3) and pop.stride == 2 * pop.pair_stride
  member = pop.pair(2)
  assert (member.obs_dim, member.act_dim, member.goal_dim) == (46, 9, 23) and torch.equal(member.params, pop.params[2])
  with pytest.raises(ValueError, match='member 1 has switch_every'):
    PairPopulation([pair, AgentPair(mk(2), mk(3), switch_every=(4, 2), backward_goal='initial_states', obs_dim=46, act_dim=9)])
  env = Kitchen.__new__(Kitchen)                                         # (the env itself needs a GPU; its checks do not)
  env.device, env.scalar_api, env.num_envs, env._cfg = torch.device('cpu'), False, 40, _Cfg(n=40, env_offset=3)
  env._initial_states = np.arange(6 * 23, dtype=np.float64).reshape(6, 23)
  assert env._check_pair(pair, 'rollout_pair') is False and env._check_pair(pop, 'evaluate_pair') is False
  # 'initial_states': the rows of get_init_states(); 'initial': its one row when there is one, else an error naming initial_states
  assert np.array_equal(pair.goal_table(env).numpy(), env.get_init_states()) and np.array_equal(pop.goal_table(env).numpy(), env.get_init_states())
  initial = AgentPair(mk(0), mk(1), backward_goal='initial', obs_dim=46, act_dim=9)
  with pytest.raises(ValueError, match='initial_states has 6 rows'):
    initial.goal_row(env)
  env._initial_states = env._initial_states[2:3]
  assert initial.goal_table(env) is None and np.array_equal(initial.goal_row(env).numpy(), np.arange(46.0, 69.0))
  assert pair.goal_table(env) is None and np.array_equal(pair.goal_row(env).numpy(), np.arange(46.0, 69.0))      # a table of one row behaves as 'initial'
  assert tuple(tab.goal_table(env).shape) == (4, 23) and np.array_equal(one.goal_row(env).numpy(), np.arange(23.0))
  # the pinned refusals stay, and point at the new methods
  with pytest.raises(NotImplementedError, match='AgentPair on the kitchen.*rollout_pair'):
    env.rollout_agents(pair, 3)
  with pytest.raises(NotImplementedError, match='AgentPair on the kitchen.*rollout_pair'):
    env.rollout_policy(pair, 3)
  # by field
  with pytest.raises(ValueError, match='pair is an AgentPair or a PairPopulation'):
    env.rollout_pair(mk(0), 3)
  with pytest.raises(ValueError, match='observation width 14 and action width 4; this env takes 46 and 9'):
    env.rollout_pair(AgentPair(MLPPolicy(random_layers([14, 16, 4], seed=0), obs_dim=14, act_dim=4), MLPPolicy(random_layers([14, 16, 4], seed=1), obs_dim=14, act_dim=4),
                               obs_dim=14, act_dim=4), 3)
  env._cfg.env_offset = 9
  with pytest.raises(ValueError, match='global env ids 9 .. 48 need members up to 3 of 3'):
    env.evaluate_pair(pop, 3)
  env._cfg.env_offset = 3
  env.scalar_api = True
  with pytest.raises(ValueError, match='scalar_api'):
    env.rollout_pair(pair, 3)
  with pytest.raises(ValueError, match='scalar_api'):
    env.evaluate_pair(pop, 3)
  env.scalar_api = False
  env._cfg.goal_change_frequency = 5
  with pytest.raises(ValueError, match='goal switch runs on the host'):
    env.rollout_pair(pair, 3)
  with pytest.raises(ValueError, match='goal switch runs on the host'):
    env.evaluate_pair(pair, 3)
  env._cfg.goal_change_frequency = 0
  with pytest.raises(ValueError, match='Gaussian agents'):
    env.rollout_pair(pair, 3, sample=False)
  with pytest.raises(ValueError, match='T = 0'):
    env.rollout_pair(pair, 0)
  with pytest.raises(ValueError, match='sample=False needs Gaussian agents'):
    env.evaluate_pair(pair, 3, sample=False)
  g = lambda seed: GaussianMLPPolicy(random_layers([46, 16, 18], seed=seed), 'tanh', squash=False, obs_dim=46, act_dim=9)
  assert env._check_pair(AgentPair(g(0), g(1), obs_dim=46, act_dim=9), 'rollout_pair') is True      # unbounded agents are taken: the env clips
  env.device = torch.device('cuda', 0)
  with pytest.raises(ValueError, match='the pair is on cpu'):
    env.rollout_pair(pair, 3)


def test_plain_kernels_are_byte_identical_and_the_kernels_that_run_the_pair_keep_their_resources():
  """physics_kitchen.hip and physics_kitchen_policy.hip cross-compiled once each.  Measured: every form occupancy 1 and LDS 162,048 bytes, 256 VGPR,
  AGPR 256 / 232 / 234 for <0> / <1> / <2> (before: 256 / 230 / 232), no scratch instruction inside a timestep loop; <1> and <2> none in the kernel at all"""
  want = kernel_build.recorded('pair_parent_build.json')
  got = kernel_build.unit('physics_kitchen.hip').digests
  plain = want['plain_functions']['physics_kitchen.hip']
  for name, lines_and_sha in plain.items():
    assert got[name] == lines_and_sha, name
  assert set(got) == set(plain)
  unit = kernel_build.unit('physics_kitchen_policy.hip')
  res = unit.resources
  assert {k for k in res if 'policy' in k} == {f'kitchen_policy_rollout_kernel<{duo}>' for duo in (0, 1, 2)}      # one kernel per form: no instantiation of its own
  for duo in (0, 1, 2):
    k = f'kitchen_policy_rollout_kernel<{duo}>'
    was, now = want['policy_kernel_resources'][k], res[k]
    print(k, was, '->', now)
    assert (now['occupancy'], now['lds']) == (was['occupancy'], was['lds']) and now['vgpr'] <= 256 and now['agpr'] <= 256
  listing = unit.scratch_report()
  assert len(listing) == 3, listing
  kernel_build.check_scratch_lines(listing, otherwise=('no scratch at all',))

"""earl_minitaur_agents_rollout (include/earl_physics.h) and Minitaur.rollout_pair / evaluate_pair, what can be held without a GPU:
  1. the entry point is declared after earl_minitaur_population_rollout, bound and exported from libearl_hip.so only;
  2. every argument error comes back before any HIP call, and the well-formed combinations (pair with pop / goals / summary / head / actions / out pointers each NULL or
     given) are accepted with n = 0;
  3. the Python refusals by field, AgentPair / PairPopulation with the minitaur's widths and goal width, and the pinned refusal of rollout_agents;
  4. compile time: the plain kernels of physics_mt.hip are byte-identical to the build before (tests/golden/pair_parent_build.json); the policy kernels, which run the
     pair, keep that build's occupancy and LDS, the one-wave kernel has no scratch instruction at all and the two-wave kernel stays within the plain one's bounds.
tests/test_minitaur_pair_gpu.py holds the launches."""
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
from test_sawyer_policy_rollout import pack, random_layers

NAME = 'earl_minitaur_agents_rollout'


def declared(name, n_args, after, before):
  """population_no_gpu.declared for an entry point that also takes earl_agent_pair and earl_backward_goals"""
  shared.declared(name, n_args, after, before)
  sig = _abi.SIGNATURES[name]
  assert any(getattr(a, '_type_', None) is _abi.AgentPair for a in sig) and any(getattr(a, '_type_', None) is _abi.BackwardGoals for a in sig)


def pair_struct(p, stride, se=(3, 2), sos=1, goal=None, phase=True, sip=True, outs=True):
  return _abi.AgentPair(switch_every=(C.c_int32 * 2)(*se), switch_on_success=sos, pad_=0, param_stride=stride, backward_goal=goal, phase=p if phase else None,
                        steps_in_phase=p if sip else None, agent_out=p if outs else None, forward_success=p if outs else None, backward_success=p if outs else None)


def pair_rows(p, count):
  """malformed pairs for agents of `count` parameters (check_pair of csrc/policy_check.h, stride multiple 4)"""
  stride = (count + 3) // 4 * 4
  return [pair_struct(p, stride, phase=False), pair_struct(p, stride, sip=False), pair_struct(p, stride, se=(0, 2)), pair_struct(p, stride, se=(3, 0)),
          pair_struct(p, stride, se=(-1, -1)), pair_struct(p, stride, sos=2), pair_struct(p, stride, sos=-1), pair_struct(p, count - 1), pair_struct(p, stride + 1),
          pair_struct(p, stride + 2), pair_struct(p, 0)]


def goals_struct(p, n_rows=5, table=True, outs=True):
  return _abi.BackwardGoals(table=p if table else None, n_rows=n_rows, pad_=0, row=p if outs else None, row_out=p if outs else None)


def test_entry_point_is_declared_bound_and_exported():
  declared(NAME, 16, 'earl_minitaur_population_rollout', 'earl_minitaur_reset')
  src = open(os.path.join(REPO, 'include', 'earl_physics.h')).read()
  assert re.search(r'W = 7 on the Sawyer door and peg.*2 on the minitaur', src) and 'goal_change_frequency > 0 is refused' in src


def test_argument_errors_and_well_formed_combinations_need_no_gpu():
  lib = _abi.load()
  layers = random_layers([32, 16, 8], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  aligned = aligned_params(pol, keep)
  count = 33 * 16 + 17 * 8
  count16 = 33 * 16 + 17 * 16                                            # with the head's 16-wide last layer
  stride = count16
  buf = np.zeros(4096, np.float64)                                       # never read: every call below returns before any HIP call
  p = buf.ctypes.data

  def cfg_of(**kw):
    d = dict(n=40, num_substeps=5, n_goals=12, goal_table=p)
    d.update(kw)
    return _abi.MinitaurCfg(**d)

  def st_of(**kw):
    d = dict(qpos=p, qvel=p, goal=p, motor_param=p, observed_torque=p, overheat=p, motor_enabled=p, last_obs=p, steps_since_goal_change=p)
    d.update(kw)
    return _abi.MinitaurState(**d)

  def out_of(**kw):
    d = dict(obs=p, reward=p, done=p, success=p)
    d.update(kw)
    return _abi.MinitaurOut(**d)

  cfg, st, out = cfg_of(), st_of(), out_of()
  good_pair, good_pop = pair_struct(p, stride), shared.pop_struct(3, 16, 2 * stride)

  def call(model=p, cfg=cfg, st=st, pol=pol, pair=good_pair, pop=None, goals=None, head=None, obs0=p, T=4, actions=p, out=out, summary=None):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_minitaur_agents_rollout(model, None, ref(cfg), ref(st), ref(pol), ref(pair), ref(pop), ref(goals), ref(head), obs0, T, None, actions, ref(out),
                                            ref(summary), None)

  pol16 = variant(pol, dims=(32, 16, 16, 0))
  bad = [dict(pair=None),                                                # not an alias of the population entry point
         dict(pol=None), dict(obs0=None),
         # everything earl_minitaur_population_rollout refuses
         dict(model=None), dict(cfg=None), dict(st=None), dict(out=None), dict(T=-1), dict(cfg=cfg_of(n=-1)),
         dict(st=st_of(qpos=None)), dict(st=st_of(qvel=None)), dict(st=st_of(goal=None)), dict(st=st_of(motor_param=None)), dict(st=st_of(observed_torque=None)),
         dict(st=st_of(overheat=None)), dict(st=st_of(motor_enabled=None)),
         dict(cfg=cfg_of(goal_table=None)), dict(cfg=cfg_of(n_goals=0)), dict(cfg=cfg_of(num_substeps=-1)),
         dict(pol=variant(pol, dims=(30, 16, 8, 0))), dict(pol=variant(pol, dims=(46, 16, 9, 0))), dict(pol=variant(pol, dims=(32, 16, 9, 0))), dict(pol=pol16),
         dict(pol=pol, head=head()), dict(pol=variant(pol, dims=(32, 24, 8, 0))), dict(pol=variant(pol, dims=(32, 272, 8, 0))),
         dict(pol=variant(pol, n_layers=3, dims=(32, 16, 24, 8))), dict(pol=variant(pol, n_layers=1)), dict(pol=variant(pol, n_layers=4)),
         dict(pol=variant(pol, precision=1)), dict(pol=variant(pol, params=None)), dict(pol=variant(pol, params=pol.params + 4)),
         dict(pol=variant(pol, hidden_act=0)), dict(pol=variant(pol, out_act=_abi.ACTIVATIONS['none'])), dict(pol=variant(pol, out_act=_abi.ACTIVATIONS['relu'])),
         dict(pol=pol16, head=head(mode=2)), dict(pol=pol16, head=head(m=2)), dict(pol=pol16, head=head(lo=-21.0)), dict(pol=pol16, head=head(lo=float('nan'))),
         dict(out=out_of(obs=None), st=st_of(last_obs=None)),
         # the lifelong switch inside a pair launch is not offered, with or without its counter
         dict(cfg=cfg_of(goal_change_frequency=5)), dict(cfg=cfg_of(goal_change_frequency=5), st=st_of(steps_since_goal_change=None)),
         # the population of pairs: the member range against the GLOBAL ids, a member is two rows
         dict(pop=good_pop, cfg=cfg_of(env_offset=9)), dict(pop=good_pop, cfg=cfg_of(env_offset=-1)), dict(pop=shared.pop_struct(3, 16, 2 * stride - 4)),
         dict(pop=shared.pop_struct(3, 16, stride)),
         # the table of backward goals
         dict(goals=goals_struct(p, table=False)), dict(goals=goals_struct(p, n_rows=0)), dict(goals=goals_struct(p, n_rows=-3)),
         dict(goals=goals_struct(p), pair=pair_struct(p, stride, goal=p))]
  bad += [dict(pair=q) for q in pair_rows(p, count)]
  bad += [dict(pop=q) for q in shared.population_rows(2 * stride, 40)]
  for kw in bad:
    assert call(**kw) == -1, kw
  # well-formed: pair with pop / goals / summary / head / actions / every pointer of out / the pair's outputs, each NULL or given, n = 0 (nothing is launched)
  cfg0, none_out = cfg_of(n=0), _abi.MinitaurOut()
  for pop in (None, good_pop, shared.pop_struct(1, 32, 2 * stride + 8)):
    for goals, pair in ((None, good_pair), (None, pair_struct(p, stride, goal=p)), (goals_struct(p), good_pair), (goals_struct(p, n_rows=1, outs=False), pair_struct(p, stride, outs=False))):
      for sm in shared.summaries(p):
        for hd, pl in ((None, pol), (head(), pol16)):
          for actions, o in ((p, out), (None, none_out), (p, out_of(obs=None)), (None, out_of(reward=None, success=None)), (p, out_of(done=None, status=p))):
            assert call(cfg=cfg0, pop=pop, goals=goals, pair=pair, summary=sm, head=hd, pol=pl, actions=actions, out=o) == 0
  assert call(T=0) == 0 and call(T=0, out=none_out, actions=None) == 0
  assert call(cfg=cfg0, st=st_of(last_obs=None)) == 0 and call(cfg=cfg0, st=st_of(steps_since_goal_change=None)) == 0
  assert call(cfg=cfg_of(n=0, env_offset=9), pop=good_pop) == 0          # (no env, no member needed)
  # the generic-stepper comparison build has no pair form
  assert lib.earl_debug_set_minitaur_stepper(0) == 0
  try:
    assert call(cfg=cfg0) == -1
  finally:
    assert lib.earl_debug_set_minitaur_stepper(1) == 0
  assert call(cfg=cfg0) == 0
  del aligned, buf


def test_python_refusals_and_the_pair_classes():
  from earl_benchmark_amd.envs.minitaur import Minitaur, _Cfg
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy, PairPopulation
  mk = lambda seed, **kw: MLPPolicy(random_layers([32, 16, 8], seed=seed), kw.pop('hact', 'relu'), kw.pop('out', 'tanh'), obs_dim=32, act_dim=8)
  pair = AgentPair(mk(0), mk(1), switch_every=(3, 2), backward_goal='initial', obs_dim=32, act_dim=8)
  assert pair.goal_dim == 2 and pair.stride % 4 == 0 and pair.backward_goal == 'initial'
  # the goal widths by env: 6 tabletop, 7 Sawyer, 2 minitaur, 23 kitchen
  tt = lambda: MLPPolicy(random_layers([12, 16, 3], seed=0))
  sw = lambda: MLPPolicy(random_layers([14, 16, 4], seed=0), obs_dim=14, act_dim=4)
  kt = lambda: MLPPolicy(random_layers([46, 16, 9], seed=0), obs_dim=46, act_dim=9)
  assert AgentPair(tt(), tt()).goal_dim == 6 and AgentPair(sw(), sw(), obs_dim=14, act_dim=4).goal_dim == 7 and AgentPair(kt(), kt(), obs_dim=46, act_dim=9).goal_dim == 23
  # one row, a table, and the wrong widths
  one = AgentPair(mk(0), mk(1), backward_goal=[0.5, -0.5], obs_dim=32, act_dim=8)
  assert tuple(one.backward_goal.shape) == (2,) and one.backward_goals is None
  tab = AgentPair(mk(0), mk(1), backward_goal=np.zeros((5, 2)), obs_dim=32, act_dim=8)
  assert tab.backward_goal is None and tuple(tab.backward_goals.shape) == (5, 2)
  with pytest.raises(ValueError, match='ONE goal row of 2 values, got 7'):
    AgentPair(mk(0), mk(1), backward_goal=np.zeros(7), obs_dim=32, act_dim=8)
  with pytest.raises(ValueError, match='ONE goal row of 2 values'):
    AgentPair(mk(0), mk(1), backward_goal=np.zeros((5, 7)), obs_dim=32, act_dim=8)
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    AgentPair(sw(), sw(), obs_dim=32, act_dim=8)
  pop = PairPopulation([pair, AgentPair(mk(2), mk(3), switch_every=(3, 2), backward_goal='initial', obs_dim=32, act_dim=8),
                        AgentPair(mk(4), mk(5), switch_every=(3, 2), backward_goal='initial', obs_dim=32, act_dim=8)])
  assert (pop.obs_dim, pop.act_dim, pop.n_policies) == (32, 8, 3) and pop.stride == 2 * pop.pair_stride
  member = pop.pair(2)
  assert (member.obs_dim, member.act_dim, member.goal_dim) == (32, 8, 2) and torch.equal(member.params, pop.params[2])
  with pytest.raises(ValueError, match='PairPopulation: .* of observation width 12 and action width 3'):
    PairPopulation([AgentPair(tt(), tt())])                               # the tabletop's pair launch takes ONE pair
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    PairPopulation([pair, AgentPair(sw(), sw(), switch_every=(3, 2), obs_dim=14, act_dim=4)])
  env = Minitaur.__new__(Minitaur)                                       # (the env itself needs a GPU; its checks do not)
  env.device, env.num_envs, env._cfg = torch.device('cpu'), 40, _Cfg(n=40, env_offset=3)
  env._reset_qpos = torch.arange(23, dtype=torch.float64) + 0.25
  assert env._check_pair(pair, 'rollout_pair') is False and env._check_pair(pop, 'evaluate_pair') is False
  assert np.array_equal(pair.goal_row(env).numpy(), [0.25, 1.25]) and pair.goal_table(env) is None and tab.goal_row(env) is None      # 'initial': reset_qpos[:2]
  assert tuple(tab.goal_table(env).shape) == (5, 2) and pop.goal_table(env) is None and np.array_equal(pop.goal_row(env).numpy(), [0.25, 1.25])
  # the pinned refusals stay, and point at the new methods
  with pytest.raises(NotImplementedError, match='AgentPair on the minitaur.*rollout_pair'):
    env.rollout_agents(pair, 3)
  with pytest.raises(NotImplementedError, match='AgentPair on the minitaur.*rollout_pair'):
    env.rollout_policy(pair, 3)
  # by field
  with pytest.raises(ValueError, match='pair is an AgentPair or a PairPopulation'):
    env.rollout_pair(mk(0), 3)
  with pytest.raises(ValueError, match='observation width 46 and action width 9; this env takes 32 and 8'):
    env.rollout_pair(AgentPair(kt(), kt(), obs_dim=46, act_dim=9), 3)
  with pytest.raises(ValueError, match='unbounded'):
    env.rollout_pair(AgentPair(mk(0, out='none'), mk(1, out='none'), obs_dim=32, act_dim=8), 3)
  with pytest.raises(ValueError, match='unbounded'):
    env.evaluate_pair(AgentPair(mk(0, out='none'), mk(1, out='none'), obs_dim=32, act_dim=8), 3)
  env._cfg.env_offset = 9
  with pytest.raises(ValueError, match='global env ids 9 .. 48 need members up to 3 of 3'):
    env.rollout_pair(pop, 3)
  env._cfg.env_offset = 3
  env._cfg.goal_change_frequency = 5
  with pytest.raises(ValueError, match='the agent pair IS the lifelong mechanism'):
    env.rollout_pair(pair, 3)
  with pytest.raises(ValueError, match='the agent pair IS the lifelong mechanism'):
    env.evaluate_pair(pop, 3)
  env._cfg.goal_change_frequency = 0
  with pytest.raises(ValueError, match='Gaussian agents'):
    env.rollout_pair(pair, 3, sample=False)
  with pytest.raises(ValueError, match='Gaussian agents'):
    env.rollout_pair(pair, 3, return_noise=True)
  with pytest.raises(ValueError, match='T = 0'):
    env.rollout_pair(pair, 0)
  with pytest.raises(ValueError, match='sample=False needs Gaussian agents'):
    env.evaluate_pair(pair, 3, sample=False)
  with pytest.raises(ValueError, match='T = 0'):
    env.evaluate_pair(pair, 0)
  g = lambda seed: GaussianMLPPolicy(random_layers([32, 16, 16], seed=seed), 'tanh', squash=True, obs_dim=32, act_dim=8)
  assert env._check_pair(AgentPair(g(0), g(1), obs_dim=32, act_dim=8), 'rollout_pair') is True
  env.device = torch.device('cuda', 0)
  with pytest.raises(ValueError, match='the pair is on cpu'):
    env.rollout_pair(pair, 3)


def test_plain_kernels_are_byte_identical_and_the_kernels_that_run_the_pair_keep_their_resources():
  """physics_mt.hip cross-compiled once.  Measured: one-wave policy kernel 256 VGPR / 178 AGPR (before: 172), no scratch instruction in the kernel,
  occupancy 1, LDS 88,208; two-wave policy kernel 12 loads and 6 stores in its slot loop (before: 10 and 3), occupancy 2, LDS 158,512"""
  unit, tool = kernel_build.unit('physics_mt.hip'), kernel_build.tool()
  want = kernel_build.recorded('pair_parent_build.json')
  got, res = unit.digests, unit.resources
  plain = want['plain_functions']['physics_mt.hip']
  for name, lines_and_sha in plain.items():
    assert got[name] == lines_and_sha, name
  assert {k for k in got if 'policy' not in k} == set(plain)
  assert {k for k in res if 'policy' in k} == {'minitaur_policy_kernel<false, true>', 'minitaur_policy_duo_kernel'}      # one kernel per form: no instantiation of its own
  for k in ('minitaur_policy_kernel<false, true>', 'minitaur_policy_duo_kernel'):
    was, now = want['policy_kernel_resources'][k], res[k]
    print(k, was, '->', now)
    assert (now['occupancy'], now['lds']) == (was['occupancy'], was['lds']) and now['vgpr'] <= 256 and now['agpr'] <= 256
  lines = unit.scratch_report(tool.KERNELS + tool.POLICY_DUO)
  one = [ln for ln in lines if 'minitaur_policy_kernel<false, true>' in ln]
  duo = [ln for ln in lines if 'minitaur_policy_duo_kernel' in ln]
  assert len(one) == 1 and len(duo) == 1, lines
  print(one[0]); print(duo[0])
  assert 'no scratch at all' in one[0], one[0]
  m = re.search(r': (\d+) loads, (\d+) stores$', duo[0].rstrip())
  assert m and int(m.group(1)) <= 64 and int(m.group(2)) <= 8, duo[0]     # the bounds of tests/test_no_scratch_in_timestep_loops.py for the plain two-wave kernel

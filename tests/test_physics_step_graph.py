"""CPU side of make_step_graph on the physics envs: the clocked rollout entry points are declared in include/earl_physics.h and bound in
earl_benchmark_amd/_abi.py with the same argument types (the old entry point's list with the clock pointer before `out`), exported by the library,
every physics env class offers make_step_graph, and PhysicsStepGraph refuses what it cannot capture before it touches a GPU."""
import ctypes as C
import os
import re
import types

import pytest

from conftest import REPO
from earl_benchmark_amd import _abi

CLOCKED = {'earl_sawyer_rollout_clocked': 'earl_sawyer_rollout', 'earl_kitchen_rollout_clocked': 'earl_kitchen_rollout',
           'earl_minitaur_rollout_clocked': 'earl_minitaur_rollout'}


def declaration(name):
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'^int\s+' + name + r'\s*\(([^;]*)\)\s*;', src, flags=re.M)
  assert m, name
  return [a.strip() for a in ' '.join(m.group(1).split()).split(',')]


@pytest.mark.parametrize('name', sorted(CLOCKED))
def test_clocked_entry_points_are_declared_and_bound_like_the_old_ones(name):
  old = CLOCKED[name]
  new_args, old_args = declaration(name), declaration(old)
  # the old parameter list with `const uint64_t* clock` inserted before `out`
  assert new_args[-3] == 'const uint64_t* clock', new_args
  assert new_args[:-3] + new_args[-2:] == old_args
  assert name in _abi.SIGNATURES
  sig, old_sig = _abi.SIGNATURES[name], _abi.SIGNATURES[old]
  assert len(sig) == len(new_args)
  assert sig[-3] is C.c_void_p and sig[:-3] + sig[-2:] == old_sig


def test_library_exports_the_clocked_entry_points():
  lib = _abi.load()
  for name in CLOCKED:
    assert hasattr(lib, name), name


def test_every_physics_env_has_make_step_graph():
  from earl_benchmark_amd.envs.kitchen import Kitchen
  from earl_benchmark_amd.envs.minitaur import Minitaur
  from earl_benchmark_amd.envs.physics_step_graph import PhysicsStepGraph
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  for cls in (SawyerDoor, SawyerPeg, Kitchen, Minitaur):
    assert callable(getattr(cls, 'make_step_graph', None)), cls
    for hook in ('_graph_check', '_new_graph_out', '_graph_capture', '_graph_step', '_graph_clock', '_graph_advance', '_graph_info'):
      assert callable(getattr(cls, hook, None)), (cls, hook)
  assert Minitaur._graph_bounds == (-1.01, 1.01) and SawyerDoor._graph_bounds is None and Kitchen._graph_bounds is None
  assert PhysicsStepGraph.check_actions and PhysicsStepGraph.replay


def fake_env(**kw):
  import torch
  d = dict(scalar_api=False, device=torch.device('cuda', 0), num_envs=2)
  d.update(kw)
  e = types.SimpleNamespace(**d)
  e.unwrapped = e
  return e


@pytest.mark.parametrize('kw,T,match', [({'scalar_api': True}, 2, 'batched'), ({'device': 'cpu'}, 2, 'cuda'), ({}, 0, 'T >= 1')])
def test_graph_arguments_are_checked_before_any_capture(kw, T, match):
  import torch
  from earl_benchmark_amd.envs.physics_step_graph import PhysicsStepGraph
  if 'device' in kw:
    kw = {'device': torch.device(kw['device'])}
  with pytest.raises(ValueError, match=match):
    PhysicsStepGraph(fake_env(**kw), T)


def test_kitchen_refuses_lifelong_goal_switching_before_any_capture():
  from earl_benchmark_amd.envs.kitchen import Kitchen, _Cfg
  from earl_benchmark_amd.envs.physics_step_graph import PhysicsStepGraph
  e = fake_env(_cfg=_Cfg())
  e._cfg.goal_change_frequency = 3
  e._graph_check = types.MethodType(Kitchen._graph_check, e)
  with pytest.raises(ValueError, match='goal'):
    PhysicsStepGraph(e, 2)

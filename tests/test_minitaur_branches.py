"""The minitaur's branch launch (include/earl_physics.h: earl_minitaur_branch_rollout, earl_minitaur_branch_ws_bytes; Minitaur.branch_rollout), what can be held without
a GPU:
  1. the workspace size query: refusals, 0 without a virtual env, monotone in K and n;
  2. every refusal of the header's list returns EARL_ERR_ARG, with a message, before the entry point touches the device (host stand-in pointers, as
     tests/test_sawyer_branches.py does), and the empty calls return EARL_OK;
  3. the structs as gcc sees them; the Python front end's argument errors; the names of their own beside the six base-class refusals;
  4. csrc/physics_mt_branch.hip compiles for gfx950 to exactly the two branch kernels and the replicate kernel, with the policy kernels' occupancy and LDS.
The GPU side is tests/test_minitaur_branches_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from test_physics_abi import EARL_ERR_ARG, host_ptr, minitaur_args


def ws_bytes(lib, K, n):
  need = C.c_int64(-1)
  rc = lib.earl_minitaur_branch_ws_bytes(K, n, C.byref(need))
  return rc, need.value


def test_workspace_size():
  lib = _abi.load()
  for K, n in ((0, 7), (7, 0), (0, 0)):
    assert ws_bytes(lib, K, n) == (_abi.EARL_OK, 0)
  grid = [(K, n) for K in (1, 2, 65, 8192) for n in (1, 5, 64)]
  sizes = {g: ws_bytes(lib, *g) for g in grid}
  assert all(rc == _abi.EARL_OK and b > 0 for rc, b in sizes.values())
  for a, (_, b) in sizes.items():
    # what a branch mutates: qpos 23, qvel 22, goal 2, observed torque 8 and the carried row 32 in float64, eight int32 counters, the goal-switch counter, eight flags
    assert b >= a[0] * a[1] * ((23 + 22 + 2 + 8 + 32) * 8 + 9 * 4 + 8), (a, b)
    for a2, (_, b2) in sizes.items():
      if all(x2 >= x for x2, x in zip(a2, a)) and a2 != a:
        assert b2 > b, (a, a2)
  assert ws_bytes(lib, 1 << 15, 1 << 16)[0] == EARL_ERR_ARG and ws_bytes(lib, -1, 4)[0] == EARL_ERR_ARG and ws_bytes(lib, 1, -4)[0] == EARL_ERR_ARG
  assert lib.earl_minitaur_branch_ws_bytes(1, 1, None) == EARL_ERR_ARG


ACT = host_ptr(1 << 16)


def call(lib, cfg, st, model='given', K=2, H=3, act=ACT, stride=None, ws='given', ws_bytes_=1 << 40, ws_base=None, summary='given', last_obs='given', fail='given'):
  """earl_minitaur_branch_rollout on host stand-in pointers: only for calls that return before anything reads through them"""
  w = None if ws is None else _abi.MinitaurBranchWs(base=(host_ptr() if ws_base is None else ws_base) if ws == 'given' else None, bytes=ws_bytes_)
  sm = {'given': _abi.EpisodeSummary(ret=host_ptr(), success_last=host_ptr(), first_success=host_ptr()), 'empty': _abi.EpisodeSummary(), None: None}[summary]
  return lib.earl_minitaur_branch_rollout(host_ptr() if model == 'given' else None, None, None if cfg is None else C.byref(cfg), None if st is None else C.byref(st), K, H, act,
                                          H * cfg.n * 8 if stride is None and cfg is not None else (stride or 0), None, None if w is None else C.byref(w),
                                          None if sm is None else C.byref(sm), host_ptr() if last_obs == 'given' else None, host_ptr() if fail == 'given' else None, None)


def test_every_refusal_fires_before_the_device():
  """n = 4 and K = 2: an accepted call would launch, so every EARL_ERR_ARG below was decided on the host"""
  lib = _abi.load()
  cfg, st, _ = minitaur_args(n=4)

  def refused(*a, **kw):
    rc = call(lib, *a, **kw)
    return rc == EARL_ERR_ARG and b'minitaur_branch_rollout' in lib.earl_last_error()

  # everything earl_minitaur_rollout_clocked refuses in model / cfg / st
  assert refused(cfg, st, model=None) and refused(None, st) and refused(cfg, None)
  assert refused(*minitaur_args(n=-1)[:2]) and refused(*minitaur_args(n=4, gcf=2, with_sgc=False)[:2])
  for field in ('qpos', 'qvel', 'goal', 'motor_param', 'observed_torque', 'overheat', 'motor_enabled'):
    c2, s2, _ = minitaur_args(n=4)
    setattr(s2, field, None)
    assert refused(c2, s2), field
  for kw in (dict(goal_table=None), dict(n_goals=0), dict(num_substeps=-1)):
    c2, s2, _ = minitaur_args(n=4)
    for k, v in kw.items():
      setattr(c2, k, v)
    assert refused(c2, s2), kw
  # the launch's own
  for kw in (dict(act=None), dict(ws=None), dict(K=-1), dict(H=-1), dict(stride=-1), dict(stride=3 * 4 * 8 - 1), dict(stride=1),
             dict(summary=None, last_obs=None, fail=None), dict(summary='empty', last_obs=None, fail=None)):
    assert refused(cfg, st, **kw), kw
  big, bst, _ = minitaur_args(n=1 << 19)
  assert refused(big, bst, K=4096)                                                       # K n = 2^31
  need = ws_bytes(lib, 2, 4)[1]
  assert need > 0 and refused(cfg, st, ws_bytes_=need - 1)                               # too small
  assert refused(cfg, st, ws='null base') and refused(cfg, st, ws_base=host_ptr(1 << 16) + 4)      # NULL, misaligned
  # the generic-stepper comparison build has no branch form
  assert lib.earl_debug_set_minitaur_stepper(0) == 0
  try:
    assert refused(cfg, st)
  finally:
    assert lib.earl_debug_set_minitaur_stepper(1) == 0


def test_the_empty_calls_launch_nothing():
  lib = _abi.load()
  cfg, st, _ = minitaur_args(n=4)
  zero, zst, _ = minitaur_args(n=0)
  assert call(lib, zero, zst) == _abi.EARL_OK and call(lib, zero, zst, ws='null base', ws_bytes_=0) == _abi.EARL_OK      # (no virtual env: no block needed)
  assert call(lib, cfg, st, K=0, ws='null base', ws_bytes_=0) == _abi.EARL_OK
  assert call(lib, cfg, st, H=0) == _abi.EARL_OK and call(lib, cfg, st, H=0, stride=0) == _abi.EARL_OK
  # every combination of outputs but none at all; steps_since_reset, fail_count and last_obs of `st` are not needed
  for kw in (dict(summary=None), dict(last_obs=None), dict(fail=None), dict(summary=None, last_obs=None), dict(summary='empty', fail=None)):
    assert call(lib, cfg, st, H=0, **kw) == _abi.EARL_OK, kw
  c2, s2, _ = minitaur_args(n=4)
  s2.steps_since_reset = s2.fail_count = s2.last_obs = None
  assert call(lib, c2, s2, H=0) == _abi.EARL_OK
  assert call(lib, cfg, st, H=0, stride=2 * 3 * 4 * 8) == _abi.EARL_OK                  # a stride beyond H n 8


def test_structs_match_what_gcc_sees(tmp_path):
  probes = (('earl_minitaur_branch_ws', _abi.MinitaurBranchWs), ('earl_minitaur_plan_params', _abi.MinitaurPlanParams))
  body = ''
  for cname, cls in probes:
    body += f'printf("%zu", sizeof({cname}));\n' + '\n'.join(f'printf(" %zu", offsetof({cname}, {f[0]}));' for f in cls._fields_) + '\nprintf("\\n");\n'
  src = '#include <stdio.h>\n#include <stddef.h>\n#include "earl_physics.h"\nint main(void) {\n' + body + 'printf("%d\\n", EARL_MINITAUR_PLAN_MAX_K);\nreturn 0; }\n'
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src)
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
  for (cname, cls), line in zip(probes, lines):
    tok = [int(x) for x in line.split()]
    assert tok[0] == C.sizeof(cls) and tok[1:] == [getattr(cls, f[0]).offset for f in cls._fields_], cname
  assert int(lines[2]) == _abi.MINITAUR_PLAN_MAX_K


def bare(n=3):
  import torch
  from earl_benchmark_amd.envs.minitaur import Minitaur
  env = object.__new__(Minitaur)                                          # (no GPU here: the argument errors need no state)
  env.num_envs, env.device, env.total_step_count = n, torch.device('cpu'), 0
  return env


def test_python_argument_errors():
  import torch
  env = bare()
  ok = torch.zeros(2, 4, 3, 8)
  for args, kw in (((torch.zeros(2, 4, 3, 4),), {}), ((torch.zeros(2, 4, 2, 8),), {}), ((torch.zeros(4, 3, 8),), {}), ((ok,), dict(K=2)), ((torch.zeros(4, 3, 8),), dict(K=0)),
                   ((torch.zeros(0, 4, 3, 8),), {}), ((torch.zeros(2, 0, 3, 8),), {})):
    with pytest.raises(ValueError, match='branch_rollout'):
      env.branch_rollout(*args, **kw)
  # the reference's bound, as rollout raises it: the dimension that is out of bounds, NaN included
  for bad, dim in ((1.02, 5), (-1.5, 0), (float('nan'), 7)):
    a = ok.clone()
    a[1, 2, 0, dim] = bad
    with pytest.raises(ValueError, match=f'^{dim}th action out of bounds.$'):
      env.branch_rollout(a)
    with pytest.raises(ValueError, match=f'^{dim}th action out of bounds.$'):
      env.branch_rollout(a[1], K=3)


def test_names_of_their_own_beside_the_base_class_refusals():
  from earl_benchmark_amd.envs.kitchen import Kitchen
  from earl_benchmark_amd.envs.minitaur import Minitaur
  from earl_benchmark_amd.envs.physics_env import PhysicsEnv
  for name in ('branch_rollout', 'mppi_plan', 'mppi_candidates', 'mppi_control'):
    assert callable(getattr(Minitaur, name)) and not hasattr(PhysicsEnv, name) and not hasattr(Kitchen, name), name
  # the six base-class names still refuse on the minitaur (tests/test_sawyer_{branches,plan,cem,value,prior}.py hold the messages)
  assert all(getattr(Minitaur, name) is getattr(PhysicsEnv, name) for name in ('rollout_branches', 'plan_mppi', 'plan_candidates', 'mpc_rollout', 'plan_cem', 'cem_candidates'))
  with pytest.raises(NotImplementedError, match='rollout_branches.*the minitaur'):
    object.__new__(Minitaur).rollout_branches(None)


def test_the_unit_holds_the_two_branch_kernels_and_the_replicate_kernel():
  """physics_mt_branch.hip and physics_mt.hip cross-compiled once each.  Measured: one-wave branch kernel 256 VGPR / 164 AGPR, no scratch, occupancy 1, LDS 88,208;
  two-wave branch kernel occupancy 2, LDS 158,512.  That physics_mt.hip itself is unchanged is tests/test_minitaur_population.py's and tests/test_minitaur_pair.py's."""
  built = kernel_build.units(['physics_mt_branch.hip', 'physics_mt.hip'])
  unit, parent, tool = built['physics_mt_branch.hip'], built['physics_mt.hip'], kernel_build.tool()
  res, was = unit.resources, parent.resources
  print(res)
  assert sorted(res) == ['minitaur_branch_duo_kernel', 'minitaur_branch_kernel<false, true>', 'minitaur_branch_replicate_kernel'], sorted(res)
  assert not any('branch' in k for k in was), sorted(was)
  one, pol = res['minitaur_branch_kernel<false, true>'], was['minitaur_policy_kernel<false, true>']
  assert (one['occupancy'], one['lds']) == (pol['occupancy'], pol['lds']) and one['vgpr'] <= 256 and one['agpr'] <= 256 and one['scratch'] == 0, (one, pol)
  duo, pduo = res['minitaur_branch_duo_kernel'], was['minitaur_policy_duo_kernel']
  assert (duo['occupancy'], duo['lds']) == (pduo['occupancy'], pduo['lds']) and duo['vgpr'] <= 256 and duo['agpr'] <= 256, (duo, pduo)
  assert res['minitaur_branch_replicate_kernel']['scratch'] == 0 and res['minitaur_branch_replicate_kernel']['lds'] == 0
  # the slot loop of the two-wave kernel: within the plain two-wave kernel's bounds (tests/test_no_scratch_in_timestep_loops.py)
  # (counted as tools/scratch_in_loops.py counts them for the kernels it knows by name: the scratch instructions inside the function's widest loop)
  asm = unit.asm
  start = next(i for i, ln in enumerate(asm) if re.match(r'^_Z\w*minitaur_branch_duo_kernel\w*:\s', ln))
  body = asm[start:next(j for j in range(start, len(asm)) if asm[j].startswith('.Lfunc_end'))]
  a, b = tool.loops_of(body)[0]
  loads = sum('scratch_load' in ln for ln in body[a:b + 1])
  stores = sum('scratch_store' in ln for ln in body[a:b + 1])
  print(f'minitaur_branch_duo_kernel: slot loop lines {a}-{b}: {loads} loads, {stores} stores')
  assert b - a > len(body) // 2 and loads <= 64 and stores <= 8, (a, b, len(body), loads, stores)
  # the object list gains exactly this unit; the two kernel bodies are included where they were, once more each
  mk = open(os.path.join(kernel_build.CSRC, 'Makefile')).read()
  src = re.search(r'^SRC\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
  assert src.count('physics_mt_branch.hip') == 1 and len(src) == len(set(src))
  assert re.search(r'^physics_mt_branch\.o: physics_mt_branch\.hip \$\(PHYS\) \$\(MINITAUR\)$', mk, flags=re.M)
  header = open(os.path.join(kernel_build.CSRC, 'physics_env_minitaur.h')).read()
  assert header.count('#include "physics_env_minitaur_rollout.inc"') == 3 and header.count('#include "physics_env_minitaur_duo.inc"') == 3

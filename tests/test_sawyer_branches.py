"""The Sawyer door / peg branch launch (include/earl_physics.h: earl_sawyer_branch_rollout), what can be held without a GPU:
  1. every refusal of the header's list returns EARL_ERR_ARG before the entry point touches the device (host stand-in pointers, as tests/test_physics_abi.py does),
     and n == 0, K == 0, H == 0 return EARL_OK;
  2. the workspace size query: 0 without a virtual env, monotone in K and in n, its own refusals; the struct is what gcc sees in the header;
  3. the resource bar: each branch kernel of csrc/physics_branch.hip / physics_branch_w8.hip has the occupancy and the LDS of the plain sawyer_rollout_kernel of the
     same (NV, LPE, SLICED) in the same build (physics.hip / physics_w8.hip), no more scratch bytes, and no scratch instruction inside a timestep loop;
  4. the Python front end refuses on the envs that have no branch launch.
The GPU side is tests/test_sawyer_branches_gpu.py; that physics.hip and physics_w8.hip still compile to the recorded build is tests/test_closed_loop_args.py."""
import ctypes as C
import os
import subprocess

import pytest

import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from test_physics_abi import EARL_ERR_ARG, host_ptr, sawyer_args

INT32_MAX = 2**31 - 1


def ws_bytes(lib, nv, K, n):
  need = C.c_int64(-1)
  rc = lib.earl_sawyer_branch_ws_bytes(nv, K, n, C.byref(need))
  return rc, need.value


def call(lib, nv, cfg, st, K=2, H=3, act='given', stride=None, clock=None, ws='given', outputs=('ret', 'last', 'first', 'last_obs', 'fail'), model='given', ws_bytes_=1 << 40):
  """earl_sawyer_branch_rollout on host stand-in pointers: only for calls that return before anything reads through them"""
  stride = H * cfg.n * 4 if stride is None else stride
  summary = _abi.EpisodeSummary(ret=host_ptr() if 'ret' in outputs else None, success_last=host_ptr() if 'last' in outputs else None,
                                first_success=host_ptr() if 'first' in outputs else None)
  w = _abi.SawyerBranchWs(base=host_ptr() if ws == 'given' else None, bytes=ws_bytes_) if ws is not None else None
  return lib.earl_sawyer_branch_rollout(host_ptr() if model == 'given' else None, None, nv, C.byref(cfg), C.byref(st), K, H, host_ptr() if act == 'given' else None,
                                        stride, clock, None if w is None else C.byref(w), C.byref(summary) if outputs != 'no summary' else None,
                                        host_ptr() if 'last_obs' in outputs else None, host_ptr() if 'fail' in outputs else None, None)


@pytest.mark.parametrize('nv', [10, 15])
def test_zero_work_returns_ok_and_launches_nothing(nv):
  lib = _abi.load()
  cfg, st, _ = sawyer_args(n=0, nv=nv)
  assert call(lib, nv, cfg, st) == _abi.EARL_OK                                # n == 0
  assert call(lib, nv, cfg, st, ws='null base', ws_bytes_=0) == _abi.EARL_OK   # (no virtual env: no block needed)
  cfg, st, _ = sawyer_args(n=4, nv=nv)
  assert call(lib, nv, cfg, st, K=0) == _abi.EARL_OK
  assert call(lib, nv, cfg, st, K=0, ws='null base', ws_bytes_=0) == _abi.EARL_OK
  assert call(lib, nv, cfg, st, H=0) == _abi.EARL_OK
  assert call(lib, nv, cfg, st, H=0, stride=0) == _abi.EARL_OK


@pytest.mark.parametrize('nv', [10, 15])
def test_every_refusal_fires_before_the_device(nv):
  """n = 4 and K = 2: an accepted call would launch, so every EARL_ERR_ARG below was decided on the host"""
  lib = _abi.load()
  ok = lambda **kw: sawyer_args(n=4, nv=nv, **kw)[:2]
  cfg, st = ok()
  assert call(lib, nv, cfg, st, model=None) == EARL_ERR_ARG
  assert call(lib, 12, cfg, st) == EARL_ERR_ARG and call(lib, 23, cfg, st) == EARL_ERR_ARG            # nv not 10 or 15
  assert call(lib, nv, cfg, st, act=None) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, ws=None) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, ws='null base') == EARL_ERR_ARG
  need = ws_bytes(lib, nv, 2, 4)[1]
  assert need > 0 and call(lib, nv, cfg, st, ws_bytes_=need - 1) == EARL_ERR_ARG                      # a block that is too small
  assert call(lib, nv, cfg, st, K=-1) == EARL_ERR_ARG and call(lib, nv, cfg, st, H=-1) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, stride=-1) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, H=3, stride=3 * 4 * 4 - 1) == EARL_ERR_ARG                             # neither 0 nor >= H n 4
  assert call(lib, nv, cfg, st, outputs=()) == EARL_ERR_ARG and call(lib, nv, cfg, st, outputs='no summary') == EARL_ERR_ARG      # all five outputs NULL
  big, bst = sawyer_args(n=1 << 16, nv=nv)[:2]
  assert call(lib, nv, big, bst, K=1 << 15) == EARL_ERR_ARG                                            # K n = 2^31
  # what earl_sawyer_rollout_clocked refuses in cfg / st
  cfg, st = ok(gcf=3, with_sgc=False)
  assert call(lib, nv, cfg, st) == EARL_ERR_ARG                                                        # goal switching without its counter
  cfg, st = ok(n_goal_rows=2)
  assert call(lib, nv, cfg, st) == EARL_ERR_ARG                                                        # a goal count without its table
  cfg, st = ok()
  st.qpos = None
  assert call(lib, nv, cfg, st) == EARL_ERR_ARG
  if nv == 15:
    cfg, st = ok(reward_type=1, att_grasp=4, att_lpad=5, att_rpad=6)
    st.obj_init = None
    assert call(lib, nv, cfg, st) == EARL_ERR_ARG                                                      # peg dense reward without obj_init
  neg, nst = sawyer_args(n=-1, nv=nv)[:2]
  assert call(lib, nv, neg, nst) == EARL_ERR_ARG


def test_each_single_output_is_enough():
  """the five outputs may be NULL in any combination but all: with n = 0 an accepted call returns EARL_OK before the device"""
  lib = _abi.load()
  cfg, st, _ = sawyer_args(n=0, nv=10)
  for one in ('ret', 'last', 'first', 'last_obs', 'fail'):
    assert call(lib, 10, cfg, st, outputs=(one,)) == _abi.EARL_OK, one
  assert call(lib, 10, cfg, st, outputs=()) == EARL_ERR_ARG


def test_the_64_lane_measurement_builds_have_no_branch_form():
  lib = _abi.load()
  cfg, st, _ = sawyer_args(n=4, nv=10)
  assert lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
  try:
    assert call(lib, 10, cfg, st) == EARL_ERR_ARG
    zero, zst, _ = sawyer_args(n=0, nv=10)
    assert call(lib, 10, zero, zst) == EARL_ERR_ARG
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK


def test_workspace_size_is_zero_without_work_and_monotone():
  lib = _abi.load()
  for nv in (10, 15):
    assert ws_bytes(lib, nv, 0, 7) == (_abi.EARL_OK, 0) and ws_bytes(lib, nv, 7, 0) == (_abi.EARL_OK, 0) and ws_bytes(lib, nv, 0, 0) == (_abi.EARL_OK, 0)
    sizes = {(K, n): ws_bytes(lib, nv, K, n) for K in (1, 2, 3, 64, 65, 4096) for n in (1, 2, 5, 64, 1024)}
    assert all(rc == _abi.EARL_OK and b > 0 for rc, b in sizes.values())
    for (K, n), (_, b) in sizes.items():
      for (K2, n2), (_, b2) in sizes.items():
        if K2 >= K and n2 >= n and (K2, n2) != (K, n):
          assert b2 > b, (nv, K, n, K2, n2)
    # a virtual env keeps qpos (nv + 1 at most), qvel, mocap, goal, one observation row and a counter; four of them share two words of the queue
    assert sizes[(3, 5)][1] >= 15 * ((nv + 1 + nv + 3 + 7 + 14) * 8 + 4) + 2 * 4 * 4
    assert ws_bytes(lib, nv, 1 << 15, 1 << 16)[0] == EARL_ERR_ARG and ws_bytes(lib, nv, 1, INT32_MAX)[0] == _abi.EARL_OK
    assert ws_bytes(lib, nv, -1, 4)[0] == EARL_ERR_ARG and ws_bytes(lib, nv, 4, -1)[0] == EARL_ERR_ARG
    assert lib.earl_sawyer_branch_ws_bytes(nv, 1, 1, None) == EARL_ERR_ARG
  assert ws_bytes(lib, 15, 3, 5)[1] > ws_bytes(lib, 10, 3, 5)[1]
  assert ws_bytes(lib, 12, 3, 5)[0] == EARL_ERR_ARG


def test_workspace_struct_matches_what_gcc_sees(tmp_path):
  """tests/test_abi.py's probe, for the struct this header gained"""
  fields = [f[0] for f in _abi.SawyerBranchWs._fields_]
  src = ('#include <stdio.h>\n#include <stddef.h>\n#include "earl_physics.h"\nint main(void) {\nprintf("%zu", sizeof(earl_sawyer_branch_ws));\n'
         + '\n'.join(f'printf(" %zu", offsetof(earl_sawyer_branch_ws, {f}));' for f in fields) + '\nprintf("\\n");\nreturn 0; }\n')
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src)
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  tok = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
  assert tok[0] == C.sizeof(_abi.SawyerBranchWs) and tok[1:] == [getattr(_abi.SawyerBranchWs, f).offset for f in fields]


def test_branch_kernels_keep_the_plain_kernels_resources():
  """the resource bar: same occupancy and LDS as the plain kernel of the same instantiation in the same build, no more scratch, none of it in a timestep loop"""
  got = kernel_build.units(['physics_branch.hip', 'physics_branch_w8.hip', 'physics.hip', 'physics_w8.hip'])
  pairs = [('physics_branch.hip', 'physics.hip', '<10, 16, false>'), ('physics_branch.hip', 'physics.hip', '<15, 16, false>'),
           ('physics_branch.hip', 'physics.hip', '<15, 16, true>'), ('physics_branch_w8.hip', 'physics_w8.hip', '<10, 16, false>')]
  for unit, plain_unit, inst in pairs:
    now, was = got[unit].resources['sawyer_branch_rollout_kernel' + inst], got[plain_unit].resources['sawyer_rollout_kernel' + inst]
    print(unit, inst, was, '->', now)
    assert (now['occupancy'], now['lds']) == (was['occupancy'], was['lds']), (unit, inst, was, now)
    assert now['scratch'] <= was['scratch'], (unit, inst, was, now)
  for unit, n_kernels in (('physics_branch.hip', 3), ('physics_branch_w8.hip', 1)):
    assert sum('sawyer_branch_rollout_kernel' in k for k in got[unit].resources) == n_kernels, sorted(got[unit].resources)
    assert not any('sawyer_rollout_kernel' in k or 'policy' in k for k in got[unit].resources), sorted(got[unit].resources)      # only the branch kernels live here
    lines = got[unit].scratch_report(('sawyer_branch_rollout_kernel',))
    assert len(lines) == n_kernels
    kernel_build.check_scratch_lines(lines, otherwise=('no scratch at all',))
  # the replicate kernel in front: a copy, one wave per four virtual envs, no LDS and no scratch
  rep = got['physics_branch.hip'].resources['sawyer_branch_replicate_kernel']
  assert rep['scratch'] == 0 and rep['lds'] == 0, rep


def test_the_base_class_refuses_where_no_branch_launch_is_built():
  from earl_benchmark_amd.envs.kitchen import Kitchen
  from earl_benchmark_amd.envs.minitaur import Minitaur
  from earl_benchmark_amd.envs.physics_env import PhysicsEnv
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  for cls in (Minitaur, Kitchen):
    assert cls.rollout_branches is PhysicsEnv.rollout_branches
    env = object.__new__(cls)                                            # (no GPU here: the refusal needs no state)
    with pytest.raises(NotImplementedError, match='rollout_branches.*' + cls.ENV):
      env.rollout_branches(None)
  assert SawyerPeg.rollout_branches is SawyerDoor.rollout_branches is not PhysicsEnv.rollout_branches

"""What the Sawyer door / peg MPPI and CEM planners share (csrc/sawyer_shoot.h), what can be held without a GPU:
  1. the workspace layout: the three public size functions (earl_sawyer_plan_ws_bytes, earl_sawyer_value_ws_bytes, earl_sawyer_prior_ws_bytes) against ONE Python
     statement of the block, built on earl_sawyer_branch_ws_bytes -- the byte counts are public contract, so this part holds on the commits before the header too;
  2. the structure: each planner unit names one scoring callee in its iteration loop, the Philox draw of a candidate is stated in the shared header alone, and the
     helpers both units used to define are defined once.
The planners' bits are held by tests/test_sawyer_{plan,cem,value,prior}.py and their `_gpu` files."""
import ctypes as C
import os
import re

import pytest

import kernel_build
from earl_benchmark_amd import _abi
from test_physics_abi import EARL_ERR_ARG

SIZE_FUNCTIONS = ('earl_sawyer_plan_ws_bytes', 'earl_sawyer_value_ws_bytes', 'earl_sawyer_prior_ws_bytes')


def round8(v):
  return (v + 7) // 8 * 8


def layout(branch, K, H, n):
  """the block of a planner call: the branch launch's workspace rounded up to 8 bytes; `_value` and `_prior`: the [K n] discounts; `_prior`: the second work queue,
  2 ceil(K n / 4) int32 rounded up to 8 bytes; then the [K, H, n, 4] candidates behind 8 bytes of slack -- always for the plain block, for H > 0 otherwise"""
  if K * n == 0:
    return 0, 0, 0
  cand = 8 + 16 * K * H * n
  value = round8(branch) + 8 * K * n + (cand if H > 0 else 0)
  return round8(branch) + cand, value, value + round8(8 * ((K * n + 3) // 4))


def size(lib, name, *args):
  need = C.c_int64(-1)
  return getattr(lib, name)(*args, C.byref(need)), need.value


@pytest.mark.parametrize('nv', [10, 15])
def test_the_three_size_functions_state_one_layout(nv):
  lib = _abi.load()
  for K in (1, 2, 65, 8192):
    for H in (0, 1, 7):
      for n in (0, 1, 5):
        rc, branch = size(lib, 'earl_sawyer_branch_ws_bytes', nv, K, n)
        assert rc == _abi.EARL_OK
        got = tuple(size(lib, name, nv, K, H, n) for name in SIZE_FUNCTIONS)
        assert got == tuple((_abi.EARL_OK, b) for b in layout(branch, K, H, n)), (nv, K, H, n, branch, got)
  for name in SIZE_FUNCTIONS:
    assert size(lib, name, 12, 2, 3, 4)[0] == EARL_ERR_ARG and size(lib, name, nv, 2, -1, 4)[0] == EARL_ERR_ARG
    assert getattr(lib, name)(nv, 2, 3, 4, None) == EARL_ERR_ARG


def read(*files):
  return ''.join(open(os.path.join(kernel_build.CSRC, f)).read() for f in files)


def code(text):
  """the text without its // comments"""
  return re.sub(r'//[^\n]*', '', text)


def test_each_planner_names_one_scoring_callee_and_the_shared_pieces_stand_once():
  for unit in ('sawyer_plan.hip', 'sawyer_cem.hip'):
    text = code(read(unit))
    loop = text[text.index('params->iterations; ++it'):]
    callees = re.findall(r'\b(earl_sawyer_branch_rollout\w*|earl_unit_sawyer_branch_\w+|sawyer_shoot_score)\s*\(', loop)
    assert len(callees) == 1, (unit, callees)                                # (no three-way choice of a callee per iteration)
    assert 'earl_sawyer_branch_rollout_value' not in text, unit
    assert not re.search(r'#include\s+"physics_', read(unit, 'sawyer_shoot.h'))
  assert 'philox4x32_10' in read('sawyer_shoot.h')
  assert 'philox4x32_10' not in read('sawyer_plan.h') and 'philox4x32_10' not in read('sawyer_cem.h')
  sawyer = code(read(*sorted(f for f in os.listdir(kernel_build.CSRC) if re.fullmatch(r'sawyer_\w+\.(hip|h)', f))))
  for name in ('round_up', 'wave_sum', 'launched', 'misaligned16', 'sawyer_ws_layout'):
    assert len(re.findall(r'^[\w: ]*\b' + name + r'\((?:const )?\w+[*&]? \w+[,)].*\{', sawyer, flags=re.M)) == 1, name

"""tests/kernel_build.py itself: a unit is compiled once, with the Makefile's flags, and the compile call and the readers of its output exist once under tests/."""
import collections
import os
import re

import pytest

import kernel_build
from conftest import REPO

TESTS = os.path.join(REPO, 'tests')


def test_a_unit_is_compiled_once_and_handed_out_again():
  first = kernel_build.unit('physics_w8.hip')                            # (the cheapest unit)
  assert kernel_build.unit('physics_w8.hip') is first and kernel_build.units(['physics_w8.hip'])['physics_w8.hip'] is first
  assert first.asm and 'Function Name: ' in first.remarks and first.digests and first.resources and first.figures
  assert all(len(fig) == len(kernel_build.FIGURES) for fig in first.figures.values())


def test_no_unit_was_handed_to_the_compiler_twice():
  """holds whenever it is asked: whatever the tests before it compiled, and nothing if none did"""
  assert [k for k, n in collections.Counter(kernel_build.COMPILED).items() if n > 1] == []


def test_the_flags_are_the_makefiles():
  mk = open(os.path.join(kernel_build.CSRC, 'Makefile')).read()
  hipflags = re.search(r'^HIPFLAGS\s*\?=\s*(.*)$', mk, flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
  assert {'-Wall', '-Wextra'} <= set(hipflags) and {'--cuda-device-only', '-S'} <= set(kernel_build.tool().FLAGS)
  assert [f for f in kernel_build.tool().FLAGS if f not in ('--cuda-device-only', '-S')] == [f for f in hipflags if f not in ('-Wall', '-Wextra')]


def texts():
  out = {}
  for d, _, files in os.walk(TESTS):
    for f in files:
      if '__pycache__' not in d and not f.endswith(('.so', '.npz', '.npy', '.pyc')):
        try:
          out[os.path.relpath(os.path.join(d, f), TESTS)] = open(os.path.join(d, f), encoding='utf-8').read()
        except UnicodeDecodeError:
          pass
  return out


def test_the_compile_call_and_the_readers_exist_once():
  src = texts()
  # (each pattern is written so that this file does not hold the text it looks for)
  for pattern in (r'kernel-resource-usag[e]', r'def normalised_function[s]', r'def digest[(]', r'def resources[(]'):
    assert [f for f, text in src.items() if re.search(pattern, text)] == ['kernel_build.py'], pattern
  crossing = re.compile(r'from test_\w+ import .*\b(digest|normalised_functions|resources)\b')
  assert [f for f, text in src.items() if crossing.search(text)] == []


def test_the_scratch_rule():
  line = 'physics.hip: sawyer_rollout_kernel<15, 16, true>: 4 scratch instructions in 9 lines; outermost loop (env steps) lines 0-8: 2; timestep loop lines 1-2 (1 lines): '
  kernel_build.check_scratch_lines([line + '0', 'physics.hip: physics_kernel<10>: no scratch at all (5 lines)'], otherwise=('no scratch at all',))
  with pytest.raises(AssertionError):
    kernel_build.check_scratch_lines([line + '1'], otherwise=('no scratch at all',))
  with pytest.raises(AssertionError):                                    # a timestep loop is held to the count, whatever phrase the line also holds
    kernel_build.check_scratch_lines([line + '1'], otherwise=('timestep loop',))
  with pytest.raises(AssertionError):
    kernel_build.check_scratch_lines(['physics.hip: physics_kernel<10>: 3 scratch instructions, no loop'], otherwise=('no scratch at all', 'slot loop'))

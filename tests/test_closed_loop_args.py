"""The closed-loop kernel arguments of the stepper envs (csrc/policy_closed_loop.h: ClosedLoopArgs, its host-side fill and its device pieces), what can be held
without a GPU:
  1. the plain functions of physics.hip and physics_w8.hip (sawyer_rollout_kernel in every instantiation, reset / observe / reward / info, physics_kernel) are
     byte-identical to the build before the shared header (tests/golden/closed_loop_parent_build.json; the minitaur's and the kitchen's are held by
     tests/test_minitaur_pair.py and tests/test_kitchen_pair.py);
  2. every policy kernel of the five units keeps that build's occupancy, LDS and scratch bytes, takes no more VGPRs, AGPRs or SGPRs, and has no scratch
     instruction inside a timestep loop;
  3. the closed-loop fields are declared once under csrc/, and no *_closed_loop body assigns one itself.
The golden was recorded by `golden_of()` below on the parent commit's csrc, with the flags of tools/scratch_in_loops.py."""
import os
import re

import pytest

import kernel_build

UNITS = ('physics.hip', 'physics_w8.hip', 'physics_mt.hip', 'physics_kitchen.hip', 'physics_kitchen_policy.hip')
PLAIN_UNITS = ('physics.hip', 'physics_w8.hip')
FIELDS = ('pol', 'head', 'gauss', 'obs0', 'act_out', 'pop_G', 'pop_stride', 'sum_ret', 'sum_last', 'sum_first', 'pair_phase', 'pair_sip', 'pair_stride', 'pair_goal',
          'pair_fwd', 'pair_goal_rows', 'pair_fwd_rows', 'pair_se', 'pair_sos', 'pair_agent', 'pair_fs', 'pair_bs', 'pair_row', 'pair_row_out')


def golden_of(units, compiler):
  """the golden of `units` (kernel_build.units(UNITS) on the parent commit's csrc) under kernel_build.compiler_version()'s name `compiler`"""
  return {'compiler': compiler,
          'what': 'the build before csrc/policy_closed_loop.h, cross-compiled with the flags of tools/scratch_in_loops.py: a digest per plain function of physics.hip and '
                  'physics_w8.hip (gfx950 assembly, comment lines and label numbers aside: [lines, sha256]) and the resources of every policy kernel of the five units '
                  '(tests/test_closed_loop_args.py)',
          'plain_functions': {u: {k: v for k, v in units[u].digests.items() if 'policy' not in k} for u in PLAIN_UNITS},
          'policy_kernel_resources': {u: {k: v for k, v in units[u].resources.items() if 'policy' in k} for u in UNITS}}


@pytest.fixture(scope='module')
def units():
  return kernel_build.recorded('closed_loop_parent_build.json'), kernel_build.units(UNITS)


def test_plain_sawyer_functions_are_byte_identical_to_the_build_before(units):
  want, got = units
  for unit in PLAIN_UNITS:
    plain = want['plain_functions'][unit]
    fns = {k: v for k, v in got[unit].digests.items() if 'policy' not in k}
    assert set(fns) == set(plain), sorted(set(fns) ^ set(plain))
    for name, lines_and_sha in plain.items():
      assert fns[name] == lines_and_sha, (unit, name)
  names = ' '.join(want['plain_functions']['physics.hip'])
  for k in ('sawyer_rollout_kernelILi10ELi16ELb0E', 'sawyer_rollout_kernelILi10ELi16ELb1E', 'sawyer_rollout_kernelILi15ELi16ELb0E', 'sawyer_rollout_kernelILi15ELi16ELb1E',
            'sawyer_reset_kernelILi10E', 'sawyer_reset_kernelILi15E', 'sawyer_door_reward_kernel', 'sawyer_door_info_kernel', 'physics_kernelILi10E', 'physics_kernelILi15E'):
    assert k in names, k
  assert any('sawyer_rollout_kernel' in k for k in want['plain_functions']['physics_w8.hip'])


def test_every_policy_kernel_keeps_its_resources(units):
  want, got = units
  tool = kernel_build.tool()
  seen = 0
  for unit in UNITS:
    res = got[unit].resources
    was_unit = want['policy_kernel_resources'][unit]
    assert {k for k in res if 'policy' in k} == set(was_unit), unit
    for k, was in sorted(was_unit.items()):
      now = res[k]
      print(unit, k, was, '->', now)
      assert (now['occupancy'], now['lds'], now['scratch']) == (was['occupancy'], was['lds'], was['scratch']), (k, was, now)
      assert now['vgpr'] <= was['vgpr'] and now['agpr'] <= was['agpr'] and now['sgpr'] <= was['sgpr'], (k, was, now)
      seen += 1
    # (the two-wave minitaur kernel has one slot loop and no timestep loop: its scratch bytes are held above)
    kernel_build.check_scratch_lines([ln for ln in got[unit].scratch_report(tool.KERNELS + tool.POLICY_DUO) if 'policy' in ln],
                                     otherwise=('no scratch at all', 'no inner loop', 'slot loop'))
  assert seen >= 9      # door, peg, peg time-sliced, door eight-wave, minitaur one-wave and two-wave, kitchen x 3


def sources():
  return {f: open(os.path.join(kernel_build.CSRC, f)).read() for f in sorted(os.listdir(kernel_build.CSRC)) if f.endswith(('.h', '.hip', '.inc', '.cpp'))}


def test_the_fields_are_declared_once_and_filled_once():
  src = sources()
  for field in ('pair_phase', 'pop_G', 'sum_ret'):
    decl = [f for f, text in src.items() for _ in re.finditer(r'^\s*(?:const\s+)?[\w:]+\s*\*?\s*' + field + r'\s*;', text, flags=re.M)]
    assert decl == ['policy_closed_loop.h'], (field, decl)
  header = src['policy_closed_loop.h']
  body = re.search(r'struct ClosedLoopArgs : Plain \{(.*?)\n\};', header, flags=re.S).group(1)
  declared = re.findall(r'^\s*(?:const\s+)?[\w:]+\s*\*?\s*(\w+)(?:\[\d+\])?\s*;', body, flags=re.M)
  assert sorted(declared) == sorted(FIELDS), declared
  assert len(re.findall(r'\bfill_closed_loop\s*\(', header)) == 1
  for unit, fn, struct, plain in (('physics.hip', 'sawyer_closed_loop', 'SawyerPolicyArgs', 'SawyerArgs'), ('physics_mt.hip', 'minitaur_closed_loop', 'MinitaurPolicyArgs', 'MinitaurArgs'),
                                  ('physics_kitchen.hip', 'kitchen_closed_loop', 'KitchenPolicyArgs', 'KitchenRolloutArgs')):
    text = src[unit]
    start = text.index('static int ' + fn)
    fn_body = text[start:text.index('\n}\n', start)]
    for field in FIELDS:
      assert not re.search(r'\b\w+\.' + field + r'\b(?:\[\d\])?\s*=[^=]', fn_body), (fn, field)
    assert fn_body.count('fill_closed_loop(') == 1 and fn_body.count('check_closed_loop(') == 1, fn
    assert not re.search(r'contract::check_(policy|population|pair|pair_population|backward_goals)\b', fn_body), fn
    # the policy struct declares no field of its own
    assert re.search(r'struct ' + struct + r' : ClosedLoopArgs<' + plain + r'> \{\};', ''.join(src.values())), struct

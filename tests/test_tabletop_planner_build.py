"""The planner's header of its own (csrc/tabletop_plan.h), what can be held without a GPU: every function of the step / rollout unit and of the five planner units
compiles to the assembly of the build before the move, when csrc/tabletop_step.h held the branch body and the MPPI contract
(tests/golden/tabletop_planner_parent_build.json: `kernel_build.units(UNITS)[u].digests` on the parent commit's csrc, with the flags of tools/scratch_in_loops.py).
The policy and pair units, which include tabletop_step.h as well, are held by tests/test_tabletop3_pair.py and profiles/policy_kernel_resources.txt."""
import pytest

import kernel_build

UNITS = ('tabletop.hip', 'tabletop_branch.hip', 'tabletop_plan.hip', 'tabletop_plan_value.hip', 'tabletop_mpc.hip', 'tabletop_mpc_value.hip')


@pytest.fixture(scope='module')
def builds():
  return kernel_build.recorded('tabletop_planner_parent_build.json')['units'], kernel_build.units(UNITS)


def test_the_recorded_build_holds_every_function_of_the_six_units(builds):
  want, _ = builds
  assert set(want) == set(UNITS)
  assert sum(len(fns) for fns in want.values()) == 49
  names = ' '.join(k for fns in want.values() for k in fns)
  for k in ('rollout_kernel', 'branch_kernel', 'plan_score_kernel', 'plan_update_kernel', 'plan_candidates_kernel', 'mpc_kernel', '5value17plan_score_kernel', '5value10mpc_kernel'):
    assert k in names, k


@pytest.mark.parametrize('unit', UNITS)
def test_every_function_is_byte_identical_to_the_build_before(builds, unit):
  want, got = builds
  now = got[unit].digests
  assert set(now) == set(want[unit]), sorted(set(now) ^ set(want[unit]))
  differ = sorted(k for k, lines_and_sha in want[unit].items() if now[k] != lines_and_sha)
  for k in differ:
    print(unit, k, want[unit][k], '->', now[k])
  assert not differ, (unit, differ)

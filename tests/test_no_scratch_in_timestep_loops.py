""""no scratch inside any timestep loop".  tools/scratch_in_loops.py compiles the stepper units to gfx950 assembly (device only, no GPU needed) and counts the
scratch_load / scratch_store instructions of every rollout kernel inside its timestep loop; this test pins the count at zero (the one-wave kernels) or bounds it (the minitaur's two-wave kernel)."""
import kernel_build


def test_timestep_loops_hold_no_scratch_instruction():
  tool = kernel_build.tool()
  kernel_build.units(tool.UNITS)
  lines = [ln for ln in tool.listing(lambda u: kernel_build.unit(u).asm, tool.KERNELS) if ln.strip()]
  assert len(lines) >= 20                                               # every stepper kernel of the five units is listed
  names = ' '.join(lines)
  for k in ('sawyer_rollout_kernel<10, 16, false>', 'sawyer_rollout_kernel<15, 16, true>', 'kitchen_rollout_kernel', 'minitaur_kernel<false, true>'):
    assert k in names, k
  duo = [ln for ln in lines if 'minitaur_duo_kernel' in ln]
  assert len(duo) == 1 and 'slot loop' in duo[0]                        # the two-waves-per-SIMD kernel (round 6): at the 256-register cap its dynamics half keeps a few spills -- bounded here,
  import re                                                             # stated in DESIGN.md 4.5 (their write-through is the launch's extra HBM traffic)
  m = re.search(r': (\d+) loads, (\d+) stores$', duo[0].rstrip())
  assert m and int(m.group(1)) <= 64 and int(m.group(2)) <= 8, duo[0]
  lines = [ln for ln in lines if 'minitaur_duo_kernel' not in ln]
  kernel_build.check_scratch_lines(lines, otherwise=('no scratch at all', 'no inner loop', 'no loop'))
  # the kitchen and door kernels spill nothing at all
  assert any('kitchen_rollout_kernel' in ln and 'no scratch at all' in ln for ln in lines)
  assert any(ln.startswith('physics.hip') and 'sawyer_rollout_kernel<10, 16, false>' in ln and 'no scratch at all' in ln for ln in lines)      # (the four-workgroups-per-CU door build; the eight-wave one spills outside the loop)

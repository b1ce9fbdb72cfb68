"""What the device sweeps of csrc/policy_math.h and the width matrix of the in-kernel policies rest on, held without a GPU:
  1. tests/policy_math_probe.hip cross-compiles for gfx950 in both contexts (the tabletop units', the stepper units' `fp contract(fast)`), with the Makefile's
     HIPFLAGS (that the pragma reaches the code is shown on the device: tests/test_policy_math_gpu.py's multiply-add outside the header fuses in that build alone);
  2. the host helper (the same file, g++, the flags of the existing host sweeps) builds, and equals earl_tanh_f32 / earl_exp_f32 / earl_normal_quantile_f32 of
     libearl_host.so on a handful of values; the special values the GPU test pins are the host's;
  3. the case tables of tests/policy_width_cases.py reach all 10 + 10 + 20 + 6 tabletop instantiations and every hidden width at every layer position;
  4. the sensitivity condition on the host twin, every case: zeroing the last 16 rows (the last N-tile) of either hidden layer changes the actions, the actions
     are finite, and a tanh output does not saturate everywhere.
tests/test_policy_math_gpu.py, tests/test_policy_widths_gpu.py and tests/test_sawyer_policy_widths_gpu.py hold the device."""
import ctypes as C
import re
import shutil

import numpy as np
import pytest

import policy_math_ref as R
import policy_width_cases as W
from earl_benchmark_amd import _abi

needs_hipcc = pytest.mark.skipif(shutil.which('hipcc') is None, reason='no hipcc')


# ---------------------------------------------------------------------------------------------------------------- 1. the probe unit
def test_probe_flags_are_the_makefiles_hipflags():
  assert R.HIPFLAGS == R.makefile_hipflags()
  for build in R.BUILDS:
    cmd = R.device_command(build, 'out.so')
    assert cmd[1:1 + len(R.HIPFLAGS)] == R.makefile_hipflags() and cmd[-1] == R.SRC
    assert [a for a in cmd if a.startswith('-D')] == ([R.STEPPER_DEFINE] if build == 'stepper' else [])
    assert not any(a.startswith('-ffp-contract') for a in cmd[1 + len(R.HIPFLAGS):])                       # nothing after the product's flags changes the contraction mode
  host = R.host_command('out.so')
  for flag in ('-ffp-contract=off', '-fno-fast-math', '-mfma', '-fopenmp', '-DEARL_HOST_BUILD'):
    assert flag in host


@needs_hipcc
@pytest.mark.parametrize('build', R.BUILDS)
def test_probe_cross_compiles_for_gfx950_in_both_contexts(tmp_path, build):
  out = R.compile_unit(build, out=str(tmp_path / 'libprobe.so'))
  syms = open(out, 'rb').read()
  for name in (b'probe_tanh', b'probe_exp', b'probe_quantile', b'probe_head', b'probe_muladd', b'probe_stepper_context', b'k_tanh', b'k_head'):
    assert name in syms, name
  assert C.CDLL(out).probe_stepper_context() == int(build == 'stepper')


def test_the_stepper_context_places_the_pragma_before_the_header():
  """the define puts `#pragma clang fp contract(fast)` at file scope before policy_math.h, as physics_stepper.h precedes it in physics.hip and physics_w8.hip"""
  src = open(R.SRC).read()
  m = re.search(r'#ifdef EARL_PROBE_STEPPER_CONTEXT\s*\n#pragma clang fp contract\(fast\)\s*\n#endif', src)
  assert m and m.end() < src.index('policy_math.h"')
  for unit in ('physics.hip', 'physics_w8.hip'):
    text = open(f'{R.CSRC}/{unit}').read()
    assert text.index('#include "physics_stepper.h"') < text.index('#include "policy_math.h"')
  stepper = open(f'{R.CSRC}/physics_stepper.h').read()
  assert re.search(r'^#pragma clang fp contract\(fast\)', stepper, flags=re.M)


# ---------------------------------------------------------------------------------------------------------------- 2. the host helper
@pytest.fixture(scope='module')
def host():
  return R.load_host()


def test_host_helper_equals_the_host_library_on_a_handful_of_values(host):
  lib = _abi.load_host()
  rng = np.random.default_rng(0)
  xs = np.concatenate([rng.standard_normal(200) * 3, [0.0, -0.0, 2.0 ** -6, 10.0, -10.0, 16.0, 2.0 ** -12, 1e-30, 1e-45, 88.9, -103.9, 4.0, -20.0]]).astype(np.float32)
  bits = xs.view(np.uint32)
  for fn, ref in (('tanh', lib.earl_tanh_f32), ('exp', lib.earl_exp_f32)):
    got = R.host_fill(host, fn, bits=bits)
    want = np.array([ref(float(x)) for x in xs], np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=fn)
  ks = np.concatenate([rng.integers(0, 1 << 24, 200), [0, 1, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 14260633 // 2 + (1 << 23), 14260633 // 2 + (1 << 23) + 1]]).astype(np.uint32)
  got = R.host_fill(host, 'quantile', bits=ks)
  want = np.array([lib.earl_normal_quantile_f32(int(k)) for k in ks], np.float32)
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  # the range form and the list form are the same elements
  first, count = R.RANGES[('tanh', 'negative')]
  np.testing.assert_array_equal(R.host_fill(host, 'tanh', first=first + 12345, count=1000).view(np.uint32),
                                R.host_fill(host, 'tanh', bits=np.arange(first + 12345, first + 13345, dtype=np.uint64).astype(np.uint32)).view(np.uint32))


def test_special_values_and_the_input_tables(host):
  assert R.host_fill(host, 'tanh', bits=[0, 0x80000000, 0x7f800000, 0xff800000, 1, 0x7f7fffff]).view(np.uint32).tolist() == [0, 0x80000000, 0x3f800000, 0xbf800000, 1, 0x3f800000]
  assert R.host_fill(host, 'exp', bits=[0, 0x80000000, 0x7f800000, 0xff800000, R.f32_bits(89.0), R.f32_bits(-104.0)]).view(np.uint32).tolist() == [0x3f800000, 0x3f800000, 0x7f800000, 0, 0x7f800000, 0]
  for points, n_finite in (R.tanh_points(), R.exp_points()):
    assert np.isnan(points[n_finite:].view(np.float32)).all() and not np.isnan(points[:n_finite].view(np.float32)).any()
  assert R.RANGES[('tanh', 'positive')] == (0x39800000, 0x41800000 - 0x39800000 + 1) and R.RANGES[('exp', 'negative')] == (0xb9800000, 0x41a00000 - 0x39800000 + 1)
  assert sum(c for (fn, _), (_, c) in R.RANGES.items() if fn == 'tanh') > 2.6e8
  q = R.host_fill(host, 'quantile', first=0, count=1 << 24).view(np.uint32)
  assert np.array_equal(q, q[::-1] ^ np.uint32(0x80000000))
  # the head's rows do what their docstring says: raw on both sides of the bounds and at them, NaN in the clamp map only, eps from both tails
  for lmap in (0, 1):
    rows = R.head_rows(host, lmap, (-5.0, 2.0), seed=1, count=1 << 14)
    raw = rows[:, 1]
    assert (raw < -5).any() and (raw > 2).any() and (raw == -5).any() and (raw == 2).any() and ((raw > -5) & (raw < 2)).any()
    assert np.isnan(raw).any() == (lmap == 0) and not np.isnan(rows[:, [0, 2]]).any()
    assert rows[0, 2] == np.float32(-5.4199834) and rows[1, 2] == np.float32(5.4199834)
    out = R.host_head(host, 1, lmap, -5.0, 2.0, 0, rows)
    assert not np.isnan(out).any() and (out != rows[:, 0]).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------- 3. coverage of the dispatch
def test_case_tables_reach_every_instantiation_and_every_width():
  single = {c.inst for c in W.CASES}
  want_single = {('single', nt2, general, gauss) for nt2 in range(5) for general in (False, True) for gauss in (False, True)}
  assert single == want_single and len(single) == 20                                  # 10 deterministic + 10 Gaussian
  # every shape runs in all four (head, form) combinations
  assert len(W.CASES) == 4 * len(W.SHAPES) == 4 * 39
  for sh in W.SHAPES:
    assert {(c.head, c.form) for c in W.CASES if c.hidden == sh} == {(h, f) for h in W.HEADS for f in W.FORMS}
  # both continuing forms occur in every NT2 class, and every alternating setting takes both values
  for nt2 in range(5):
    kinds = {tuple(sorted(c.cfg_kw)) for c in W.CASES if c.form == 'continuing' and W.nt2_of(c.hidden) == nt2}
    assert kinds == {('auto_reset', 'horizon'), ('goal_change_frequency', 'horizon')}, (nt2, kinds)
    for attr in ('hact', 'oact', 'log_std_map'):
      assert len({getattr(c, attr) for c in W.CASES if W.nt2_of(c.hidden) == nt2}) == 2, (nt2, attr)
  population = {W.instantiation('population', hidden, W.POPULATION_FORMS[form], head) for hidden, head, form in W.POPULATION_CASES}
  assert population == {('population', nt2, general, gauss) for nt2 in range(5) for general in (False, True) for gauss in (False, True)} and len(population) == 20
  pair = {W.instantiation('pair', hidden, {}, head) for hidden, head in W.PAIR_CASES}
  assert pair == {('pair', nt2, True, gauss) for nt2 in range(3) for gauss in (False, True)} and len(pair) == 6
  assert len(single | population | pair) == 46
  # every hidden width at every layer position: the only hidden layer, the first of two, the second of two
  widths = set(W.WIDTHS)
  assert widths == set(range(16, 257, 16))
  assert {sh[0] for sh in W.SHAPES if len(sh) == 1} == widths
  assert {sh[0] for sh in W.SHAPES if len(sh) == 2} == widths and {sh[1] for sh in W.SHAPES if len(sh) == 2} == widths
  assert all(sh[0] != sh[1] for sh in W.ANTI_DIAGONAL)
  assert {sh[0] for sh in W.PAIR_SHAPES if len(sh) == 1} == widths
  assert {sh[1] for sh in W.PAIR_SHAPES if len(sh) == 2} == {w for w in widths if w <= W.PAIR_MAX_H2} and max(sh[1] for sh in W.PAIR_SHAPES if len(sh) == 2) == 128
  assert {W.nt2_of(sh) for sh in W.EXACT_SHAPES} == set(range(5)) and {(256,), (128, 192), (192, 128), (256, 256)} <= set(W.EXACT_SHAPES)
  # the launch has a full workgroup, a middle one and a ragged one; the population's three workgroups run three members
  assert W.N // 16 == 2 and W.N % 16 != 0
  assert {(W.OFFSET + i) // W.POPULATION_G for i in range(W.N)} == {0, 1, 2}
  # the Sawyer table: every width in every layer position on the door, a partial group after a full one among them, the group edges on the peg
  cases = W.sawyer_cases()
  door = [c[1] for c in cases if c[0] == 'door']
  assert {sh[0] for sh in door if len(sh) == 1} == widths and {sh[0] for sh in door if len(sh) == 2} >= widths and {sh[1] for sh in door if len(sh) == 2} == widths
  assert {W.sawyer_groups(w) for sh in door for w in sh} >= {(g, r) for g in (1, 2, 3) for r in (16, 32, 48)}
  peg = [c[1] for c in cases if c[0] == 'peg']
  assert {sh[-1] for sh in peg} == set(W.SAWYER_PEG_WIDTHS) and {len(sh) for sh in peg} == {1, 2}
  for kind in ('door', 'peg'):
    assert {c[4] for c in cases if c[0] == kind} == set(W.SAWYER_HEADS)
  assert {(c[2], c[3]) for c in cases} == {(h, o) for h in ('relu', 'tanh') for o in ('tanh', 'none')}


# ---------------------------------------------------------------------------------------------------------------- 4. sensitivity, on the host twin
@pytest.mark.parametrize('shape', W.SHAPES, ids=lambda sh: 'x'.join(map(str, sh)))
def test_host_twin_meets_the_sensitivity_condition(shape):
  """a kernel that drops or misplaces the last N-tile of a layer must show: the host twin's actions change when that tile's rows are zeroed.  Observed: all 40 envs
  change, at the first step already, on every one of the 124 (case, hidden layer) pairs of the single-policy table, the 18 of the population's and the 68 of the
  pair's; actions finite everywhere; no tanh output saturated on every row (Policy at its own gain 1, GaussPolicy with log_std_gain = 2)"""
  for case in (c for c in W.CASES if c.hidden == shape and c.form == 'evaluation'):
    base = case.run(case.harness('cpu'), case.policy('cpu'))['act']
    assert np.isfinite(base).all(), case.id
    if case.oact == 'tanh':
      assert not (np.abs(base) > 0.99).all(), case.id
    for layer in range(len(shape)):
      pol = case.policy('cpu')
      W.zero_last_tile(pol.params, shape, layer)
      got = case.run(case.harness('cpu'), pol)['act']
      changed = (got.view(np.uint32) != base.view(np.uint32)).any(axis=(0, 1, 3))
      first = (got[0, 0].view(np.uint32) != base[0, 0].view(np.uint32)).any(axis=1)
      print(f'{case.id} layer {layer}: envs whose actions change {int(changed.sum())} of {W.N}, at the first step {int(first.sum())}')
      assert first.any(), (case.id, layer)                               # at the first step already: not through a diverged trajectory


def first_step_changes(base, got, reset_first):
  a, b = (base[0, 0], got[0, 0]) if reset_first else (base[0], got[0])
  return (a.view(np.uint32) != b.view(np.uint32)).any(axis=1)


@pytest.mark.parametrize('shape', W.POPULATION_SHAPES, ids=lambda sh: 'x'.join(map(str, sh)))
def test_host_twin_meets_the_sensitivity_condition_on_the_population_shapes(shape):
  """the same condition through the population entry point (every member's last tile zeroed): envs of all three members change at the first step"""
  for head in W.HEADS:
    base = W.population_run('cpu', shape, head, 'evaluation')[0]['act']
    assert np.isfinite(base).all() and not (np.abs(base) > 0.99).all()
    for layer in range(len(shape)):
      got = W.population_run('cpu', shape, head, 'evaluation', mutate=lambda p: W.zero_last_tile(p, shape, layer))[0]['act']
      first = first_step_changes(base, got, True)
      members = (W.OFFSET + np.arange(W.N)) // W.POPULATION_G
      print(f'population {shape} {head} layer {layer}: envs whose first action changes {int(first.sum())} of {W.N}')
      assert all(first[members == m].any() for m in range(3)), (shape, head, layer)


@pytest.mark.parametrize('shape', W.PAIR_SHAPES, ids=lambda sh: 'x'.join(map(str, sh)))
def test_host_twin_meets_the_sensitivity_condition_on_the_pair_shapes(shape):
  """the same condition through the pair entry point (both agents' last tile zeroed)"""
  for head in W.HEADS:
    base = W.pair_run('cpu', shape, head)[0]
    assert np.isfinite(base['act']).all() and not (np.abs(base['act']) > 0.99).all()
    for layer in range(len(shape)):
      got = W.pair_run('cpu', shape, head, mutate=lambda p: W.zero_last_tile(p, shape, layer))[0]['act']
      first = first_step_changes(base['act'], got, False)
      agent = base['agent'][0]
      print(f'pair {shape} {head} layer {layer}: envs whose first action changes {int(first.sum())} of {W.N}')
      assert first[agent == 0].any() and first[agent == 1].any(), (shape, head, layer)      # envs of both agents

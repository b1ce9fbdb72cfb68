"""CPU side of the primitive tests (tests/test_physics_primitives_gpu.py): the test unit cross-compiles with the product's flags, the references agree with each
other where two exist, and the input generators meet the conditions the GPU assertions rest on BY THE REFERENCE ALONE -- so that a bound missed on the device
says something about the kernel and not about the inputs."""
import os
import re
import shutil

import mpmath
import numpy as np
import pytest

import primitives_ref as R

U, LD = R.U, R.LD


def test_fixture_flags_are_the_makefiles_hipflags():
  assert R.HIPFLAGS == R.makefile_hipflags()


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='no hipcc')
@pytest.mark.parametrize('packed', [False, True])
def test_unit_cross_compiles_for_gfx950_with_the_product_flags(tmp_path, packed):
  out = R.compile_unit(packed, out=str(tmp_path / 'libprim.so'))
  assert os.path.getsize(out) > 0
  syms = open(out, 'rb').read()
  for name in (b'prim_rcp_nr', b'prim_solve_rows_22', b'prim_solve_schur_15', b'prim_chol_small_6', b'prim_lane_moves'):
    assert name in syms


def _calls(text, name):
  """template argument lists of the calls of `name<...>(` in a source text, comments stripped"""
  text = re.sub(r'//[^\n]*', '', text)
  return {m.group(1).replace(' ', '') for m in re.finditer(r'\b' + name + r'<([^<>()]*(?:\([^()]*\))?[^<>()]*)>\s*\(', text)}


def test_instantiation_lists_match_the_call_sites():
  """a new instantiation in the product without a wrapper in tests/physics_primitives.hip fails here"""
  stepper = open(os.path.join(R.CSRC, 'physics_stepper.h')).read()
  mt = open(os.path.join(R.CSRC, 'minitaur_stepper.h')).read()
  solve = open(os.path.join(R.CSRC, 'physics_solve.h')).read()
  # the generic call sites are written in NV / NA: which NV reach them is decided by Lim<NV>; the literal argument lists must be the ones the wrappers repeat
  assert _calls(stepper, 'chol_regs') == {'NA,NA,true', 'NV,NV,(NV>10)', 'NV,NA,(NV>10)'}
  assert _calls(stepper, 'solve_regs') == {'NA,NA', 'NV,NV', 'NV,NA'}
  assert _calls(stepper, 'load_tri') == {'NV,NV', 'NV,NA'}
  assert _calls(stepper, 'chol_coop') == {'NV'} and _calls(stepper, 'solve_lds') == {'NV'}
  assert _calls(stepper, 'chol_coop_loop') == {'NV'} and _calls(stepper, 'solve_lds_loop') == {'NV'}
  assert _calls(stepper, 'chol_solve_rows') == {'NV'}
  assert _calls(stepper, 'solve_lead_regs') == {'NV,NA'} and _calls(stepper, 'solve_schur_regs') == {'NV,NA'}
  assert _calls(stepper, 'scan_anc') == {'NV'} and _calls(stepper, 'scan_desc') == {'NV,10', 'NV,6'}
  assert _calls(solve, 'chol_regs') == {'N,N,true', 'NP,NP,true', 'NA,NA,true'} and _calls(solve, 'solve_regs') == {'N,N', 'NA,NA'}
  assert {f'{n}' for n in R.SMALL_N} == _calls(mt, 'chol_small') and _calls(mt, 'solve_regs') == {'6,6'}
  quads = set(re.findall(r'dpp_quad<(QP_\w+|qp_bcast<\w+>\(\))>\(', re.sub(r'//[^\n]*', '', mt)))
  assert quads == {'QP_PARENT', 'QP_CHILD', 'QP_SWAP1', 'QP_SWAP2'} | {f'qp_bcast<{k}>()' for k in range(4)}
  assert _calls(solve, 'group_bcast') == {'J'}
  # the forms that no call site names any more stay deleted (physics_solve.h: solve_lead_regs is the only leading-block form)
  assert 'chol_coop_lead' not in stepper + solve and 'solve_lds_lead' not in stepper + solve
  # the models behind NV, and the wrappers that exist for them
  lds = open(os.path.join(R.CSRC, 'physics_lds.h')).read()
  assert 'static constexpr int NA = (NV == 15 || NV == 23) ? 9 : NV;' in lds and 'static constexpr int LPE = NV > 16 ? 32 : 16;' in lds
  assert 'static constexpr bool ARMSCAN = (NV == 15 || NV == 23) && !EARL_NO_ARMSCAN;' in lds
  unit = open(R.SRC).read()
  for form, sizes in R.SOLVE_FORMS.items():
    for nv in sizes:
      assert re.search(rf'PRIM_SOLVE\({form}_{nv}, {nv}, F_{form.upper()}\)', unit), (form, nv)
  for nv in (15, 23):
    assert nv in R.SCAN_NV


def test_newton_bounds_hold_for_every_seed_the_comment_allows():
  """where A's bounds come from: the iterations restated with exactly rounded operations, from seeds with ANY relative error up to 2^-26 and up to 2^-20, stay
  within rcp_nr 1 ulp, rsq_nr / rsq2 2 ulp -- and rsq2 with one step lost does not (so the GPU assertion sees a lost step)"""
  rng = np.random.default_rng(5)
  xs = np.concatenate([np.exp2(rng.uniform(-200, 200, 500)), 10.0 ** rng.uniform(-8, 4, 500)])
  worst = {'rcp': 0.0, 'rsq3': 0.0, 'rsq2': 0.0, 'rsq1': 0.0}
  for x in xs.tolist():
    for amp in (2.0 ** -26, 2.0 ** -20):
      e = float(rng.uniform(-1, 1)) * amp
      for key, got, root in (('rcp', R.restate_rcp(x, e), False), ('rsq3', R.restate_rsq(x, e, 3), True), ('rsq2', R.restate_rsq(x, e, 2), True)):
        worst[key] = max(worst[key], float(R.ulp_err_mp(np.array([x]), np.array([got]), root)[0]))
    e = (1 if rng.random() < 0.5 else -1) * 2.0 ** -26
    worst['rsq1'] = max(worst['rsq1'], float(R.ulp_err_mp(np.array([x]), np.array([R.restate_rsq(x, e, 1)]), True)[0]))
  print(worst)
  assert worst['rcp'] <= 1.0 and worst['rsq3'] <= 2.0 and worst['rsq2'] <= 2.0
  assert worst['rsq1'] > 2.0


def test_ulp_measure_longdouble_agrees_with_mpmath():
  rng = np.random.default_rng(6)
  x = np.exp2(rng.uniform(-200, 200, 2000))
  for root in (False, True):
    got = (1 / np.sqrt(x) if root else 1 / x) * (1 + rng.integers(-3, 4, len(x)) * 2.0 ** -52)
    a, b = R.ulp_err(got, R.recip_ref_ld(x, root)), R.ulp_err_mp(x, got, root)
    assert np.abs(a - b).max() <= 2.0 ** -9        # (longdouble's 2^-64 against the double's 2^-53 ulp: 2^-11, and the same again for the difference)


def test_sincos_references_agree_to_2_pow_minus_60():
  x, special = R.sincos_inputs(n_random=4000)
  xs = x[~special]
  s, c = np.sin(xs), np.cos(xs)
  es_l, ec_l = R.sincos_err_ld(xs, s, c)
  es_m, ec_m = R.sincos_err_mp(xs, s, c)
  assert max(np.abs(es_l - es_m).max(), np.abs(ec_l - ec_m).max()) <= 2.0 ** -60


def test_sincos_restatement_meets_the_absolute_bound():
  """the kernel's operations with exactly rounded steps: absolute error <= 2^-52 on the documented range (the bound the GPU test asserts), multiples of pi/2 included"""
  x, special = R.sincos_inputs(n_random=3000)
  pick = np.concatenate([x[special][::37], x[~special]])
  got = np.array([R.restate_sincos(v) for v in pick.tolist()])
  es, ec = R.sincos_err_mp(pick, got[:, 0], got[:, 1])
  print('restated sincos_mod: max abs error', max(es.max(), ec.max()))
  assert max(es.max(), ec.max()) <= 2.0 ** -52


def test_impedance_cases_cover_what_the_issue_lists():
  c = R.impedance_cases()
  refs, imps = R.model_sol_rows()
  assert len(refs) >= 3 and len(imps) >= 10
  have = {tuple(r) for r in c[:, 2:7].tolist()}
  assert all(tuple(i) in have for i in imps)
  p, d0, dw, width, mid, r, dt = c[:, 6], c[:, 2], c[:, 3], c[:, 4], c[:, 5], c[:, 7], c[:, 8]
  for power in (1, 2, 3, 2.5):
    assert (p == power).any()
  assert (d0 == dw).any() and (width == 0).any() and (r == 0).any() and (np.abs(r) >= width).any() and (c[:, 0] < 2 * dt).any()
  assert ((np.abs(r) == mid * width) & (width > 0)).any() and (mid == 0.05).any() and (mid == 0.95).any()
  # the reference at a few hand-worked points: power 2, mid 0.5: y(0.25) = 0.125, y(0.75) = 0.875; power 1: y = x
  assert abs(R.impedance_ref((0.0, 1.0, 1.0, 0.5, 2.0), 0.25) - mpmath.mpf(0.125)) < 1e-60
  assert abs(R.impedance_ref((0.0, 1.0, 1.0, 0.5, 2.0), -0.75) - mpmath.mpf(0.875)) < 1e-60
  assert abs(R.impedance_ref((0.2, 0.6, 2.0, 0.5, 1.0), 0.5) - mpmath.mpf('0.3')) < 1e-16
  assert R.impedance_ref((0.9, 0.95, 0.0, 0.5, 2.0), 0.1) == mpmath.mpf(0.95)


def test_cone_zone_left_out_share_and_reference():
  c = R.cone_zone_inputs()
  zone, decided = R.cone_zone_ref(c)
  assert len(c) >= 1_000_000 and 1 - decided.mean() <= 0.01, 1 - decided.mean()
  assert (c[:, 3] == 0).any() and (c[:, 0] == 0).any() and ((c[:, 1] == 0) & (c[:, 2] == 0)).any()
  assert all((zone[decided] == z).sum() > 10000 for z in (0, 1, 2))
  for i in np.flatnonzero(decided)[:3000].tolist():            # longdouble against mpmath
    r0, r1, r2, mu = (mpmath.mpf(v) for v in c[i].tolist())
    rho = mpmath.sqrt(r1 * r1 + r2 * r2)
    assert zone[i] == (0 if r0 >= mu * rho else (1 if rho <= -mu * r0 else 2))
  b, want = R.cone_zone_boundary()
  zb, _ = R.cone_zone_ref(b)
  assert (zb == want).all()


@pytest.mark.parametrize('kind,nv', [('dense', 10), ('dense', 15), ('dense', 22), ('dense', 23), ('blocks', 15), ('lead', 23), ('dense', 4), ('dense', 6)])
def test_solver_inputs_are_fair_by_the_reference_alone(kind, nv):
  """the plain fp64 statement of the inverted-diagonal Cholesky reaches eta <= 2 u on every system (the GPU bound is 16 u), the longdouble reference is far
  below that, and the equilibrated condition is within a factor 10 of the nominal one"""
  fam = R.family(kind, nv)
  A, b = R.active(fam)
  assert len(A) >= 2048 and len(A) % 4 == 0
  blocks = [(0, A.shape[1])] if kind != 'blocks' else [(0, R.NA_OF[nv]), (R.NA_OF[nv], nv)]
  for lo, hi in blocks:
    As, bs = A[:, lo:hi, lo:hi], b[:, lo:hi]
    eta = R.backward_error(As, R.chol_solve(As, bs, np.float64), bs)
    assert eta.max() <= 2 * U, eta.max() / U
    assert R.backward_error(As, R.solve_ld(As, bs), bs).max() <= U / 256
    ratio = R.cond2_equilibrated(As) / fam['nominal']
    assert ratio.min() >= 0.1 and ratio.max() <= 10, (ratio.min(), ratio.max())
  assert np.array_equal(fam['H0'], fam['H0'].transpose(0, 2, 1))
  if kind == 'blocks':
    na = R.NA_OF[nv]
    assert np.isnan(fam['H'][:, na:, :na]).all() and np.isnan(fam['H'][:, :na, na:]).all() and not np.isnan(fam['A']).any()


@pytest.mark.parametrize('name,nv', [('door', 10), ('peg', 15)])
def test_recorded_hessians_are_fair_by_the_reference_alone(name, nv):
  fam = R.recorded_family(name)
  A, b = R.active(fam)
  assert A.shape == (160, nv, nv) and len(A) % 4 == 0 and np.array_equal(fam['H'], fam['H'].transpose(0, 2, 1))
  assert R.backward_error(A, R.chol_solve(A, b, np.float64), b).max() <= 2 * U
  assert R.backward_error(A, R.solve_ld(A, b), b).max() <= U / 256
  assert np.abs(fam['H'][:, :9, 9:]).max() > 0 or nv == 15          # (the door couples all ten dofs; the recorded peg systems are block diagonal)


def test_spoiled_systems_have_the_pivot_they_claim():
  fam = R.family('dense', 10)
  H, bad, which = R.spoil(fam, fam['H'])
  assert bad.sum() == len(H) // 4 and set(which[bad].tolist()) == {0, 1, 2, 3, 4}
  assert all(bad[w * 4:(w + 1) * 4].sum() == 1 for w in range(len(H) // 4))
  A = H.copy()
  d = np.arange(10)
  A[:, d, d] += fam['dl']
  for e in np.flatnonzero(bad & (which <= 2)).tolist():
    j = (0, 5, 9)[which[e]]
    sc = 1 / np.sqrt(np.abs(A[e, d, d]))
    Ae = A[e] * sc[:, None] * sc[None, :]                           # (signs of pivots and definiteness do not change under a diagonal scaling; eigvalsh needs it)
    lead = Ae[:j, :j]
    assert j == 0 or np.linalg.eigvalsh(lead).min() > 0            # the columns before it factorise ...
    piv = Ae[j, j] - (Ae[j, :j] @ np.linalg.solve(lead, Ae[:j, j]) if j else 0.0)
    assert piv < 0                                                  # ... and column j's pivot is negative


def test_scan_reference_chains():
  anc, desc = R.chains(15)
  assert anc[8] == [0, 1, 2, 3, 4, 5, 6, 8] and desc[6] == [6, 7, 8] and desc[0] == list(range(9)) and anc[12] == [9, 10, 11, 12] and desc[12] == [12, 13, 14] and anc[15] is None
  assert R.chains(10)[0][9] is None and R.chains(23)[1][9] is None

"""The stepper's device primitives, each on its own, against plain high-precision references (tests/primitives_ref.py: mpmath, numpy.longdouble; nothing from
oracle/, nothing from the library under test) at inputs chosen to hurt them.  The kernels are the wrappers of tests/physics_primitives.hip, built on demand with the
product's flags in the door's two storage layouts.  u = 2^-53.  Every test prints the figure it asserts on (DESIGN.md "primitive accuracy on MI355X" quotes them).

Bounds are the ones the references give, never what the device returned: A from the exactly rounded restatement of the Newton iterations under any seed the comment
in physics_math.h allows (test_physics_primitives.py), B from the restated kernel, D from the plain fp64 Cholesky's own backward error (<= 1.03 u measured, asserted
<= 2 u on the same inputs) times 16 for the 1.6-ulp root, fused against separate rounding and CholRows' two partial sums."""
import numpy as np
import pytest

import primitives_ref as R

pytestmark = pytest.mark.gpu
U, LD = R.U, R.LD


class Dev:
  """a test library plus the device-buffer plumbing (torch only moves bytes)"""

  def __init__(self, packed):
    import torch
    self.torch, self.lib, self.packed = torch, R.load(packed), packed
    assert self.lib.prim_door_packed() == int(packed)

  def call(self, name, ins, out_shapes, n, out_dtype=None):
    t = self.torch
    d_in = [t.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in ins]
    d_out = [t.full(sh, float('nan'), dtype=t.float64, device='cuda') if out_dtype is None else t.full(sh, -1, dtype=out_dtype, device='cuda') for sh in out_shapes]
    rc = getattr(self.lib, 'prim_' + name)(*[a.data_ptr() for a in d_in], *[a.data_ptr() for a in d_out], n, t.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, rc)
    t.cuda.synchronize()
    return [a.cpu().numpy() for a in d_out]

  def solve(self, form, nv, H, dl, b):
    return self.call(f'solve_{form}_{nv}', [H, dl, b], [b.shape], len(H))[0]


@pytest.fixture(scope='module')
def dev():
  return Dev(False)


@pytest.fixture(scope='module')
def dev_packed():
  return Dev(True)


def fig(*a):
  print('PRIM-FIG', *a)


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ================================================================================================================ A
@pytest.mark.parametrize('name,root,bound', [('rcp_nr', False, 1.0), ('rsq_nr', True, 2.0), ('rsq2', True, 2.0)])
def test_reciprocal_and_root_iterations(dev, name, root, bound):
  """>= 1e6 inputs: log-uniform over 2^-200 ... 2^200, every power of two, 1 +- a few ulp, the models' pivot range.  Error in ulps of the correctly rounded result:
  rcp_nr <= 1, rsq_nr / rsq2 <= 2 (longdouble on all, mpmath on >= 1e5).  A lost Newton step is about 3 ulp from a 2^-26 seed."""
  x = R.recip_inputs()
  assert len(x) >= 1_000_000
  y = dev.call(name, [x], [x.shape], len(x))[0]
  assert np.isfinite(y).all()
  e_ld = R.ulp_err(y, R.recip_ref_ld(x, root))
  rng = np.random.default_rng(7)
  sub = np.unique(np.concatenate([rng.choice(len(x), 100_000, replace=False), np.arange(len(x) - 450, len(x)), np.argsort(e_ld)[-2000:]]))
  e_mp = R.ulp_err_mp(x[sub], y[sub], root)
  fig(name, 'max ulp error (longdouble, all)', e_ld.max(), '(mpmath,', len(sub), ')', e_mp.max(), 'bound', bound)
  assert e_ld.max() <= bound and e_mp.max() <= bound


@pytest.mark.parametrize('name', ['rsq_nr', 'rsq2'])
def test_roots_of_nonpositive_nan_and_inf_are_not_finite(dev, name):
  """a non-positive pivot must poison the solve, never pass as a number (the rollback guard keys on non-finite values)"""
  x = np.array([0.0, -0.0, -1.0, -1e-300, -5e-324, -1e300, -np.inf, np.nan, np.inf, -2.5, -1e-8])
  y = dev.call(name, [x], [x.shape], len(x))[0]
  assert not np.isfinite(y).any(), y


# ================================================================================================================ B
def test_sincos_mod_and_kc(dev):
  """>= 1e6 arguments: |x| <= 4, |x| <= 1e3, k pi/2 (1 +- few ulp) for |k| <= 636, zeros, denormals, the tie points of rint(x 2 / pi).  ABSOLUTE error of both outputs
  <= 2^-52 against mpmath (>= 1e5 arguments, all special ones among them; longdouble libm on the rest), |sn^2 + cs^2 - 1| <= 8 u, sincos_kc == sincos_mod bit for
  bit.  RELATIVE accuracy next to multiples of pi/2 is not promised by a two-word reduction (the restated kernel is off by 1e9 ulp of the tiny result there) and is
  not asserted.  Beyond 1e3 the first |x| at which the absolute bound fails is printed: information, not an assertion."""
  x, special = R.sincos_inputs()
  assert len(x) >= 1_000_000
  sn, cs = dev.call('sincos_mod', [x], [x.shape, x.shape], len(x))
  sk, ck = dev.call('sincos_kc', [x], [x.shape, x.shape], len(x))
  assert np.array_equal(bits(sn), bits(sk)) and np.array_equal(bits(cs), bits(ck)), 'sincos_kc is not sincos_mod bit for bit'
  es, ec = R.sincos_err_ld(x, sn, cs)
  rng = np.random.default_rng(8)
  mp = special.copy()
  mp[rng.choice(np.flatnonzero(~special), 80_000, replace=False)] = True
  mp[np.argsort(np.maximum(es, ec))[-2000:]] = True
  assert mp.sum() >= 100_000
  ms, mc = R.sincos_err_mp(x[mp], sn[mp], cs[mp])
  es[mp], ec[mp] = ms, mc
  ident = np.abs(sn.astype(LD) ** 2 + cs.astype(LD) ** 2 - 1).astype(np.float64)
  fig('sincos_mod max abs error', max(es.max(), ec.max()), '= 2^-52 x', max(es.max(), ec.max()) * 2.0 ** 52, '; at the special arguments', max(ms[:special.sum()].max(), mc[:special.sum()].max()),
      '; |sn^2+cs^2-1| / u', ident.max() / U)
  big = np.sort(np.concatenate([10.0 ** np.linspace(3, 12, 3000), -10.0 ** np.linspace(3, 12, 1000)]))
  big = big[np.argsort(np.abs(big))]
  bs, bc = dev.call('sincos_mod', [big], [big.shape, big.shape], len(big))
  eb = np.maximum(*R.sincos_err_mp(big, bs, bc))
  fails = np.flatnonzero(eb > 2.0 ** -52)
  fig('sincos_mod beyond 1e3: first |x| with abs error > 2^-52:', abs(big[fails[0]]) if len(fails) else None, 'error there', eb[fails[0]] if len(fails) else None)
  assert max(es.max(), ec.max()) <= 2.0 ** -52
  assert ident.max() <= 8 * U


# ================================================================================================================ C
def test_impedance_and_kb_against_mujocos_formula(dev):
  """kb_of, kbimp, imp_of, imp_p2 against MuJoCo's documented impedance d(r) and (k, b) written out in mpmath (primitives_ref.impedance_ref / kb_ref): powers 1, 2, 3,
  2.5, d0 == dw, width == 0, r = 0, |r| >= width, x == mid, mid 0.05 / 0.95, solref[0] < 2 dt, and every solref / solimp row of earl_benchmark_amd/models.
  |d - d_ref| <= 16 u, k and b relative <= 8 u, imp_p2 == imp_of bit for bit at powers 1 and 2.
  (Observation, not asserted: some Sawyer rows are the 3-number legacy form padded with mid = power = 0, for which this formula -- and the kernels -- give d = d0 at every r;
  MuJoCo's own runtime would first clamp such a row to power 1 and mid 1e-4.  Likewise width = 0 is taken as the limit x = 1 here.  Parity with MuJoCo on whole
  models is not pinned by this project: DESIGN.md.)"""
  import mpmath
  c = R.impedance_cases()
  out = dev.call('impedance', [c], [(len(c), 7)], len(c))[0]
  ed = ek = 0.0
  for row, o in zip(c.tolist(), out.tolist()):
    d_ref = R.impedance_ref(row[2:7], row[7])
    k_ref, b_ref = R.kb_ref(row[0:2], row[2:7], row[8])
    ed = max(ed, *[float(abs(mpmath.mpf(v) - d_ref)) for v in ((o[4], o[5]) + ((o[6],) if row[6] in (1.0, 2.0) else ()))])
    ek = max(ek, *[float(abs(mpmath.mpf(v) / ref - 1)) for v, ref in ((o[0], k_ref), (o[2], k_ref), (o[1], b_ref), (o[3], b_ref))])
  fig('impedance: max |d - d_ref| / u', ed / U, 'max relative error of k, b / u', ek / U)
  p12 = (c[:, 6] == 1) | (c[:, 6] == 2)
  assert np.array_equal(bits(out[p12, 6]), bits(out[p12, 5])), 'imp_p2 differs from imp_of at powers 1 / 2'
  assert ed <= 16 * U and ek <= 8 * U


def test_cone_apply_against_the_explicit_matrix(dev):
  """cone_apply<false> / <true> = W j with the 3 x 3 matrix of the comment in physics_lds.h, longdouble; error relative to ||W||_F ||j||_2 <= 16 u"""
  rng = np.random.default_rng(9)
  n = 200_000
  mu = 10.0 ** rng.uniform(-2, 0.5, n)
  w_ell = np.stack([10.0 ** rng.uniform(-3, 6, n), rng.standard_normal(n) * mu, rng.standard_normal(n) * mu, 10.0 ** rng.uniform(-3, 6, n), 1 / (mu * mu)], 1)
  w_ell[::7, 1:3] = 0.0; w_ell[::11, 0] = 0.0; w_ell[::13] = 0.0            # bottom zone (D, 0, 0, D, .), K = 0, top zone
  w_pyr = rng.standard_normal((n, 5)) * 10.0 ** rng.uniform(-3, 6, (n, 1))
  j = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
  worst = {}
  for ell, w in ((False, w_pyr), (True, w_ell)):
    out = dev.call('cone_apply', [np.concatenate([w, j], 1)], [(n, 6)], n)[0][:, 3:] if ell else dev.call('cone_apply', [np.concatenate([w, j], 1)], [(n, 6)], n)[0][:, :3]
    W = R.cone_matrix(w, ell)
    ref = np.einsum('nij,nj->ni', W, j.astype(LD))
    scale = np.sqrt((W * W).sum((1, 2))) * np.sqrt((j.astype(LD) ** 2).sum(1))
    err = np.abs(out.astype(LD) - ref).max(1)
    ok = scale > 0
    assert (err[~ok] == 0).all()
    worst[ell] = float((err[ok] / scale[ok]).max())
  fig('cone_apply max error / (u ||W|| ||j||): pyramid', worst[False] / U, 'elliptic', worst[True] / U)
  assert worst[False] <= 16 * U and worst[True] <= 16 * U


def test_cone_zone_three_way_rule(dev):
  """1e6 random (r0, r1, r2, mu) incl. mu = 0, rho = 0, r0 = 0: every case whose two margins exceed 8 u (|r0| + mu rho + rho) is classified exactly (<= 1 % are
  left out: checked on the CPU); exactly representable boundary cases come out as the >= / <= of the source says"""
  c = R.cone_zone_inputs()
  import torch
  got = dev.call('cone_zone', [c], [(len(c),)], len(c), out_dtype=torch.int32)[0]
  zone, decided = R.cone_zone_ref(c)
  assert 1 - decided.mean() <= 0.01
  wrong = int((got[decided] != zone[decided]).sum())
  b, want = R.cone_zone_boundary()
  gb = dev.call('cone_zone', [b], [(len(b),)], len(b), out_dtype=torch.int32)[0]
  fig('cone_zone: misclassified', wrong, 'of', int(decided.sum()), '; boundary cases wrong', int((gb != want).sum()), 'of', len(b))
  assert wrong == 0
  assert np.array_equal(gb, want), (gb, want)


# ================================================================================================================ D
# (form, nv, family kind): the product's forms on the structure each one meets (physics_stepper.h K9 / K10; coop_15 is the peg's measurement switch and the dense
# statement solve_schur_regs is compared with; coop_23 the unrolled form chol_coop_loop<23> is compared with)
SOLVE_CASES = [('regs', 10, 'dense'), ('coop', 10, 'dense'), ('regs', 15, 'blocks'), ('coop', 15, 'dense'), ('schur', 15, 'dense'), ('schur', 15, 'blocks'),
               ('coop', 22, 'dense'), ('loop', 22, 'dense'), ('rows', 22, 'dense'), ('coop', 23, 'dense'), ('loop', 23, 'dense'),
               ('lead_regs', 23, 'lead'), ('lead_split', 23, 'lead')]
_fams = {}


def fam_of(kind, nv):
  if (kind, nv) not in _fams:
    _fams[kind, nv] = R.family(kind, nv)
  return _fams[kind, nv]


def inputs_for(form, fam):
  """H as the form may see it: the NaN of the never-read block stays only for the block-diagonal register form, whose claim it tests"""
  return fam['H' if form == 'regs' else 'H0']


def check_accuracy(tag, fam, x):
  """assertions D.1 (backward error, equilibrated, <= 16 u; the plain fp64 reference <= 2 u on the same systems) and D.2 (forward error <= 16 u cond2)"""
  k = fam['act']
  A, b = R.active(fam)
  blocks = [(0, k)] if fam['kind'] != 'blocks' else [(0, R.NA_OF[fam['nv']]), (R.NA_OF[fam['nv']], k)]
  assert np.isfinite(x).all(), tag
  eta = eta_ref = fwd = 0.0
  for lo, hi in blocks:
    As, bs, xs = A[:, lo:hi, lo:hi], b[:, lo:hi], x[:, lo:hi]
    eta = max(eta, R.backward_error(As, xs, bs).max())
    eta_ref = max(eta_ref, R.backward_error(As, R.chol_solve(As, bs, np.float64), bs).max())
    xl = R.solve_ld(As, bs)
    rel = (np.abs(xs.astype(LD) - xl).max(1) / np.abs(xl).max(1)).astype(np.float64)
    fwd = max(fwd, (rel / (U * R.cond2_equilibrated(As))).max())
  fig(tag, 'eta / u', eta / U, '(fp64 reference', eta_ref / U, ') forward error / (u cond)', fwd)
  assert eta_ref <= 2 * U
  assert eta <= 16 * U, (tag, eta / U)
  assert fwd <= 16, (tag, fwd)


@pytest.mark.parametrize('form,nv,kind', SOLVE_CASES)
def test_solve_forms_backward_and_forward_error(dev, dev_packed, form, nv, kind):
  """every factorisation / solve form at the instantiations the product uses, 2304 systems per family (conditions 1e2, 1e8, 1e12, each also with rows / columns
  scaled by 10^U(-3, 3)), different systems in the envs that share a wave; block-diagonal families carry NaN in the off-diagonal block the register form claims
  never to read.  nv 10 runs on both storage layouts of the door."""
  fam = fam_of(kind, nv)
  for d in ((dev, dev_packed) if nv == 10 else (dev,)):
    x = d.solve(form, nv, inputs_for(form, fam), fam['dl'], fam['b'])
    check_accuracy(f'{form}<{nv}> {kind}{" packed" if d.packed else ""}', fam, x)
    if fam['act'] < nv:                                            # a leading-block form leaves the other entries alone
      assert np.array_equal(bits(x[:, fam['act']:]), bits(fam['b'][:, fam['act']:]))


@pytest.mark.parametrize('name', ['door', 'peg'])
def test_solve_forms_on_recorded_hessians(dev, dev_packed, name):
  """Hessians and right-hand sides of real timesteps in contact (tests/golden/primitive_hessians.npz: door and peg reset at the goal under random actions, from this
  project's CPU statement of the stepper -- a data file; nothing of oracle/ is imported here): D.1 and D.2 on every form the model can meet, and the door's
  register = in-LDS identity on both layouts.  None of the recorded peg systems couples arm and peg, so all of them also go to chol_regs<15, 9> with NaN in the block
  it claims not to read."""
  fam = R.recorded_family(name)
  nv = fam['nv']
  xs = {}
  for form in ('regs', 'coop') + (('schur',) if nv == 15 else ()):
    for d in ((dev, dev_packed) if nv == 10 else (dev,)):
      H = fam['H']
      if form == 'regs' and nv == 15:
        assert not fam['joined'].any()
        H = H.copy()
        H[:, 9:, :9] = np.nan; H[:, :9, 9:] = np.nan
      xs[form, d.packed] = d.solve(form, nv, H, fam['dl'], fam['b'])
      check_accuracy(f'recorded {name}: {form}<{nv}>{" packed" if d.packed else ""}', fam, xs[form, d.packed])
  if nv == 10:
    assert all(np.array_equal(bits(v), bits(xs['regs', False])) for v in xs.values()), 'the door forms differ on recorded Hessians'


@pytest.mark.parametrize('n', R.SMALL_N)
def test_chol_small_is_chol_regs_fast_and_accurate(dev, n):
  """the minitaur's per-lane blocks: chol_small<N> == chol_regs<N, N, true> bit for bit (factor and solution: the comment in minitaur_stepper.h), D.1 and D.2"""
  fam = fam_of('dense', n)
  A64 = (fam['H'] + np.einsum('mi,ij->mij', fam['dl'], np.eye(n)))
  tri = np.tril_indices(n)
  Lin = A64[:, tri[0], tri[1]]
  m = len(Lin)
  Ls, xs = dev.call(f'chol_small_{n}', [Lin, fam['b']], [Lin.shape, fam['b'].shape], m)
  Lr, xr = dev.call(f'chol_regs_{n}', [Lin, fam['b']], [Lin.shape, fam['b'].shape], m)
  same = np.array_equal(bits(Ls), bits(Lr)) and np.array_equal(bits(xs), bits(xr))
  fig(f'chol_small<{n}> == chol_regs<{n},{n},true> bit for bit:', same)
  assert same
  fam2 = dict(fam, A=A64.astype(LD))                               # (the diagonal sum was formed on the host here: the system is the rounded one)
  check_accuracy(f'chol_small<{n}> + solve_regs', fam2, xs)


def test_bit_identities_of_the_solve_forms(dev, dev_packed):
  """the identities launch forms rest on, where they live (they broke three times under contraction and were found by bisecting whole rollouts):
  chol_regs<10,10,false> + solve_regs == chol_coop<10> + solve_lds, each on square == packed storage (the door's two builds, chosen by batch size);
  chol_coop_loop<NV> + solve_lds_loop == chol_coop<NV> + solve_lds (nv 22, 23: measurement switches of the same kernels);
  solve_lead_regs<23,9> == the helper wave's chol_regs<9,9,true> handed over through LDS + the owner's solve_regs<9,9> (the kitchen's one-wave and four-wave launches)."""
  f10 = fam_of('dense', 10)
  x = {(form, d.packed): d.solve(form, 10, f10['H0'], f10['dl'], f10['b']) for form in ('regs', 'coop') for d in (dev, dev_packed)}
  ref = x['regs', False]
  res = {f'{form}<10>{" packed" if pk else ""} == regs<10>': np.array_equal(bits(v), bits(ref)) for (form, pk), v in x.items()}
  for nv in (22, 23):
    f = fam_of('dense', nv)
    res[f'loop<{nv}> == coop<{nv}>'] = np.array_equal(bits(dev.solve('loop', nv, f['H0'], f['dl'], f['b'])), bits(dev.solve('coop', nv, f['H0'], f['dl'], f['b'])))
  f = fam_of('lead', 23)
  res['lead_regs<23,9> == lead_split<23,9>'] = np.array_equal(bits(dev.solve('lead_regs', 23, f['H0'], f['dl'], f['b'])), bits(dev.solve('lead_split', 23, f['H0'], f['dl'], f['b'])))
  fig('bit identities:', res)
  assert all(res.values()), res


@pytest.mark.parametrize('form,nv,dense', [('rows', 22, 'coop'), ('schur', 15, 'coop')])
def test_reordered_forms_agree_with_the_dense_form(dev, form, nv, dense):
  """chol_solve_rows<22> and solve_schur_regs<15,9> are different orders of operations by design: agreement with the dense in-LDS form to 16 u cond2"""
  f = fam_of('dense', nv)
  a, b = dev.solve(form, nv, f['H0'], f['dl'], f['b']), dev.solve(dense, nv, f['H0'], f['dl'], f['b'])
  rel = np.abs(a - b).max(1) / np.abs(b).max(1) / (U * R.cond2_equilibrated(R.active(f)[0]))
  fig(f'{form}<{nv}> vs {dense}<{nv}>: max difference / (u cond)', rel.max())
  assert rel.max() <= 16


@pytest.mark.parametrize('form,nv,kind', SOLVE_CASES)
def test_bad_system_poisons_its_own_env_only(dev, dev_packed, form, nv, kind):
  """one env of every wave gets an indefinite matrix (negative pivot at column 0, in the middle, last), a NaN or an Inf entry; its wave neighbours get good systems.
  The neighbours' results are bit-identical to the run with a good neighbour, and the bad env's solution holds a non-finite entry in EVERY case -- never a finite
  wrong answer: the rollback guard !(fabs(qp) < EARL_BAD_VALUE && fabs(qv) < EARL_BAD_VALUE) sees a NaN or an overflow and nothing else."""
  fam = fam_of(kind, nv)
  Hs, bad, which = R.spoil(fam, inputs_for(form, fam))
  for d in ((dev, dev_packed) if nv == 10 else (dev,)):
    good = d.solve(form, nv, inputs_for(form, fam), fam['dl'], fam['b'])
    got = d.solve(form, nv, Hs, fam['dl'], fam['b'])
    assert np.array_equal(bits(got[~bad]), bits(good[~bad])), 'a neighbour of the bad env changed'
    k = fam['act']
    finite_bad = np.isfinite(got[bad][:, :k]).all(1)
    fig(f'{form}<{nv}> {kind}: bad envs', int(bad.sum()), 'with a finite answer', int(finite_bad.sum()), 'kinds', sorted(set(which[bad][finite_bad].tolist())))
    assert not finite_bad.any(), ('finite answer from a bad system, kinds (neg0, negmid, neglast, nan, inf) =', sorted(set(which[bad][finite_bad].tolist())))


# ================================================================================================================ E
@pytest.mark.parametrize('nv', R.SCAN_NV)
def test_scans_along_the_chains(dev, nv):
  """scan_anc<NV> and scan_desc<NV, 6 / 10> against plain tree sums over the chain membership of the comments (arm 0 ... 6, fingers 7 and 8 on link 6, free body
  9 ... 14 for nv 15), integer-valued doubles so that == is the comparison; four different rows per wave; the lanes outside the chains preloaded with ordinary
  numbers, NaN and 1e300 in turn: the chain results do not change and those lanes come back untouched, bit for bit"""
  rng = np.random.default_rng(10 + nv)
  rows = 256
  outside = [s for s in range(16) if R.chains(nv)[0][s] is None]
  for fill in (None, np.nan, 1e300):
    for which, N in (('anc', 6), ('desc', 6), ('desc', 10)):
      x = rng.integers(-1000, 1001, (rows, 16, N)).astype(np.float64)
      if fill is not None:
        x[:, outside] = fill
        if R.LPE_OF[nv] == 32:
          x[1::2] = fill                                           # the env's second row of lanes
      want = R.scan_ref(x, nv, which)
      got = dev.call(f'scan_anc_{nv}' if which == 'anc' else f'scan_desc_{nv}_{N}', [x.reshape(rows * 16, N)], [(rows * 16, N)], rows)[0].reshape(rows, 16, N)
      assert np.array_equal(bits(got), bits(want)), (nv, which, N, fill)
  fig(f'scans nv {nv}: exact')


def test_lane_moves_stay_inside_their_row_quad_and_group(dev):
  """dpp_row<SHR / SHL k> returns 0 at the row edges, never the neighbour row's value; dpp_quad's patterns read inside the aligned quad; group_bcast<J> for
  J = 0, 21, 31 returns lane J of the lane's OWN 32-lane group (distinct data in the two groups)"""
  waves = 8
  lanes = 64 * waves
  v = np.arange(1, lanes + 1, dtype=np.float64) * 1.5 + 1000.0
  out = dev.call('lane_moves', [v], [(dev.lib.prim_n_moves(), lanes)], lanes)[0]
  lane = np.arange(lanes)
  want = []
  for k in (1, 2, 4):
    want.append(np.where(lane % 16 >= k, v[np.maximum(lane - k, 0)], 0.0))
  for k in (1, 2, 4):
    want.append(np.where(lane % 16 + k <= 15, v[np.minimum(lane + k, lanes - 1)], 0.0))
  base = lane - lane % 4
  for sel in ((0, 0, 2, 2), (1, 1, 3, 3), (1, 0, 3, 2), (2, 3, 0, 1), (0,) * 4, (1,) * 4, (2,) * 4, (3,) * 4):
    want.append(v[base + np.array(sel)[lane % 4]])
  for J in (0, 21, 31):
    want.append(v[lane - lane % 32 + J])
  want = np.array(want)
  assert out.shape == want.shape
  assert np.array_equal(bits(out), bits(want)), np.flatnonzero((out != want).any(1))
  fig('lane moves: exact')


# ================================================================================================================ F
def test_small_algebra(dev):
  """qmul, qmat, mulv, mulvT, cross, iapply against longdouble, 16 u relative to the operand norms; qmat of a unit quaternion orthogonal to 16 u; selv / selq / pick3
  exact.  Pins the conventions: w-first quaternions, I10 = {m, h (3), Io xx yy zz xy xz yz}."""
  rng = np.random.default_rng(11)
  n = 200_000
  qa, qb = rng.standard_normal((n, 4)), rng.standard_normal((n, 4))
  qa /= np.linalg.norm(qa, axis=1, keepdims=True)
  qb *= 10.0 ** rng.uniform(-2, 2, (n, 1))
  v, w = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1)) for _ in range(2))
  I = rng.standard_normal((n, 10)) * 10.0 ** rng.uniform(-3, 2, (n, 1))
  o = dev.call('algebra', [np.concatenate([qa, qb, v, w, I], 1)], [(n, 36)], n)[0]
  l = lambda a: a.astype(LD)
  nrm = lambda a: np.sqrt((l(a) ** 2).sum(tuple(range(1, a.ndim))))
  worst = {}

  def rel(name, got, ref, scale):
    worst[name] = float((np.abs(l(got) - ref).reshape(n, -1).max(1) / scale).max()) / U

  a, b = l(qa), l(qb)
  aw, ax, ay, az = (a[:, k] for k in range(4)); bw, bx, by, bz = (b[:, k] for k in range(4))
  rel('qmul', o[:, 0:4], np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1), nrm(qa) * nrm(qb))
  Rm = np.stack([1 - 2 * (ay * ay + az * az), 2 * (ax * ay - aw * az), 2 * (ax * az + aw * ay), 2 * (ax * ay + aw * az), 1 - 2 * (ax * ax + az * az), 2 * (ay * az - aw * ax),
                 2 * (ax * az - aw * ay), 2 * (ay * az + aw * ax), 1 - 2 * (ax * ax + ay * ay)], 1)
  rel('qmat', o[:, 4:13], Rm, np.maximum(nrm(qa) ** 2, 1))
  Rg = l(o[:, 4:13]).reshape(n, 3, 3)                              # the operand of mulv / mulvT is the matrix the device made
  # R(q) R(q)' = |q|^4 I for ANY q: the quaternion normalised in fp64 is unit to a few u only, and that is the input's share, not qmat's -- measured against the
  # norm the numbers handed in really have (rounding of the nine entries alone gives at most 2 sqrt(3) x 2 u = 7 u)
  n4 = ((a * a).sum(1) ** 2)[:, None, None]
  worst['qmat orthogonality'] = float(np.abs(np.einsum('nij,nkj->nik', Rg, Rg) - n4 * np.eye(3, dtype=LD)).max()) / U
  rel('mulv', o[:, 13:16], np.einsum('nij,nj->ni', Rg, l(v)), nrm(o[:, 4:13]) * nrm(v))
  rel('mulvT', o[:, 16:19], np.einsum('nji,nj->ni', Rg, l(v)), nrm(o[:, 4:13]) * nrm(v))
  rel('cross', o[:, 19:22], np.cross(l(v), l(w)), nrm(v) * nrm(w))
  Il = l(I)
  h = Il[:, 1:4]
  Io = np.stack([Il[:, 4], Il[:, 7], Il[:, 8], Il[:, 7], Il[:, 5], Il[:, 9], Il[:, 8], Il[:, 9], Il[:, 6]], 1).reshape(n, 3, 3)
  rel('iapply n', o[:, 22:25], np.einsum('nij,nj->ni', Io, l(w)) + np.cross(h, l(v)), nrm(Io) * nrm(w) + nrm(h) * nrm(v))
  rel('iapply f', o[:, 25:28], l(v) * Il[:, :1] - np.cross(h, l(w)), np.abs(Il[:, 0]) * nrm(v) + nrm(h) * nrm(w))
  fig('small algebra, max error / (u operand norms):', worst)
  odd = (np.arange(n) & 1).astype(bool)[:, None]
  assert np.array_equal(bits(o[:, 28:31]), bits(np.where(odd, v, w))) and np.array_equal(bits(o[:, 31:35]), bits(np.where(odd, qa, qb)))
  assert np.array_equal(bits(o[:, 35]), bits(v[np.arange(n), np.arange(n) % 3]))
  assert all(x <= 16 for x in worst.values()), worst

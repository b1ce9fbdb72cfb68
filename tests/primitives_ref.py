"""References, input generators and the build recipe for the stepper's device primitives (tests/physics_primitives.hip).

Shared by tests/test_physics_primitives.py (CPU: the references against each other, the generators against their stated conditions) and
tests/test_physics_primitives_gpu.py (the kernels against the references).  Nothing here imports oracle/ or loads the library under test: the
references are mpmath (>= 200 bits) for scalars and numpy.longdouble (64-bit mantissa on x86) for linear algebra."""
import ctypes as C
import glob
import os
import re
import subprocess

import mpmath
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')
SRC = os.path.join(REPO, 'tests', 'physics_primitives.hip')
U = 2.0 ** -53
LD = np.longdouble
mpmath.mp.prec = 240

# the product's flags, spelled out (test_physics_primitives.py asserts that this IS the HIPFLAGS line of csrc/Makefile with ARCH = gfx950)
HIPFLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fno-fast-math', '-fhip-fp32-correctly-rounded-divide-sqrt', '-fPIC', '-Wall', '-Wextra']


def makefile_hipflags():
  text = open(os.path.join(CSRC, 'Makefile')).read()
  arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
  return re.search(r'^HIPFLAGS\s*\?=\s*(.*)$', text, re.M).group(1).replace('$(ARCH)', arch).split()


def so_path(packed):
  return os.path.join(REPO, 'tests', 'libphysics_primitives_packed.so' if packed else 'libphysics_primitives.so')


def compile_unit(packed, out=None, extra=()):
  """hipcc with the product's flags -> the shared object (packed: the door's eight-wave storage layout, -DEARL_DOOR_PACKED=1)"""
  out = out or so_path(packed)
  cmd = ['hipcc', *HIPFLAGS, *(['-DEARL_DOOR_PACKED=1'] if packed else []), *extra, '-shared', '-o', out, SRC]
  subprocess.check_call(cmd)
  return out


def build_if_stale(packed):
  so = so_path(packed)
  deps = [SRC] + glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(REPO, 'include', '*.h'))
  if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
    compile_unit(packed)
  return so


# ---------------------------------------------------------------------------------------------------------------- instantiation lists
# (form -> the sizes the GPU test runs it at; test_physics_primitives.py greps the call sites of csrc/physics_stepper.h and minitaur_stepper.h against these)
SOLVE_FORMS = {'regs': (10, 15), 'coop': (10, 15, 22, 23), 'loop': (22, 23), 'rows': (22,), 'lead_regs': (23,), 'lead_split': (23,), 'schur': (15,)}
NA_OF = {4: 4, 6: 6, 10: 10, 15: 9, 22: 22, 23: 9}      # Lim<NV>::NA (4, 6: the minitaur's per-lane leg and root blocks, dense)
LPE_OF = {4: 16, 6: 16, 10: 16, 15: 16, 22: 32, 23: 32}   # Lim<NV>::LPE
SMALL_N = (4, 6)                             # chol_small<N>; solve_regs<6, 6>
SCAN_NV = (10, 15, 23)                       # (the product's ARMSCAN models are nv 15 and 23; nv 10 has the same chain rule without a free body)
SCAN_DESC_N = (6, 10)


def load(packed=False):
  lib = C.CDLL(build_if_stale(packed))
  p, L = C.c_void_p, C.c_long
  for name in ('rcp_nr', 'rsq_nr', 'rsq2', 'impedance', 'cone_apply', 'cone_zone', 'algebra', 'lane_moves',
               *[f'scan_anc_{nv}' for nv in SCAN_NV], *[f'scan_desc_{nv}_{n}' for nv in SCAN_NV for n in SCAN_DESC_N]):
    getattr(lib, 'prim_' + name).argtypes = [p, p, L, p]
  for name in ('sincos_mod', 'sincos_kc'):
    getattr(lib, 'prim_' + name).argtypes = [p, p, p, L, p]
  for form, sizes in SOLVE_FORMS.items():
    for nv in sizes:
      getattr(lib, f'prim_solve_{form}_{nv}').argtypes = [p, p, p, p, L, p]
  for n in SMALL_N:
    for k in ('small', 'regs'):
      getattr(lib, f'prim_chol_{k}_{n}').argtypes = [p, p, p, p, L, p]
  return lib


# ---------------------------------------------------------------------------------------------------------------- A: reciprocal / root
def recip_inputs(seed=0, n_random=1_000_000):
  rng = np.random.default_rng(seed)
  parts = [np.exp2(rng.uniform(-200, 200, n_random // 2)),                          # log-uniform over 2^-200 ... 2^200
           np.ldexp(rng.uniform(1, 2, n_random // 4), rng.integers(-200, 201, n_random // 4)),
           10.0 ** rng.uniform(-8, 4, n_random // 4 + 1000),                        # the pivot range of the models
           np.exp2(np.arange(-200, 201, dtype=np.float64))]                         # every power of two
  one = [1.0]
  for _ in range(8):
    one = [np.nextafter(one[0], 0.0)] + one + [np.nextafter(one[-1], 2.0)]          # 1 +- up to 8 ulp
  parts.append(np.array(one))
  parts.append(np.array([2.0, 3.0, 4.0, 0.5, 0.25]) * (1 + 2 ** -52))
  return np.concatenate(parts)


def ulp_err(got, ref_ld):
  """|got - ref| in ulps of the correctly rounded double (ref: longdouble or float array of exact-enough references)"""
  cr = ref_ld.astype(np.float64)
  return (np.abs(got.astype(LD) - ref_ld) / np.spacing(np.abs(cr)).astype(LD)).astype(np.float64)


def recip_ref_ld(x, root):
  x = x.astype(LD)
  return 1 / np.sqrt(x) if root else 1 / x


def ulp_err_mp(x, got, root):
  """the same in mpmath, exactly (a python loop: subsamples only)"""
  out = np.empty(len(x))
  for i, (xi, gi) in enumerate(zip(x.tolist(), got.tolist())):
    ref = 1 / mpmath.sqrt(mpmath.mpf(xi)) if root else 1 / mpmath.mpf(xi)
    out[i] = float(abs(mpmath.mpf(gi) - ref) / float(np.spacing(abs(float(ref)))))
  return out


# the two Newton iterations of csrc/physics_math.h restated in exact arithmetic with one rounding per operation (an fma rounds once): what any seed within the
# stated accuracy can lead to.  Used on the CPU to show where the bounds of the GPU test come from.
def _rnd(v):
  return mpmath.mpf(float(v))     # mpf -> nearest double (prec 240 holds every product of two doubles exactly)


def restate_rcp(x, seed_rel, steps=2):
  x = mpmath.mpf(x)
  r = _rnd((1 / x) * (1 + seed_rel))
  for _ in range(steps):
    e = _rnd(-x * r + 1)
    r = _rnd(e * r + r)
  return float(r)


def restate_rsq(x, seed_rel, steps):
  x = mpmath.mpf(x)
  y = _rnd((1 / mpmath.sqrt(x)) * (1 + seed_rel))
  for _ in range(steps):
    t = _rnd(_rnd(mpmath.mpf(-0.5) * x) * y)          # -0.5 * x is exact (a power of two), then one rounded product
    y = _rnd(y * _rnd(t * y + mpmath.mpf(1.5)))
  return float(y)


# ---------------------------------------------------------------------------------------------------------------- B: sincos
def sincos_inputs(seed=1, n_random=1_000_000):
  """-> (x, special): special marks the arguments that always go to mpmath (multiples of pi/2, tie points, zeros, denormals)"""
  rng = np.random.default_rng(seed)
  half_pi = mpmath.pi / 2
  ks = np.arange(-636, 637)
  near = lambda centres: np.concatenate([_step_ulps(centres, d) for d in range(-4, 5)])
  mult = np.array([float(k * half_pi) for k in ks.tolist()])
  tie = np.array([float((k + mpmath.mpf(0.5)) * half_pi) for k in ks.tolist()])      # rint(x 2 / pi) flips here
  edge = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-310, 1e-300, -1e-300, 1e-160, 1e-20, -1e-20, 4.0, -4.0, 1e3, -1e3])
  special = np.concatenate([near(mult), near(tie), edge])
  rand = np.concatenate([rng.uniform(-4, 4, n_random // 2), rng.uniform(-1e3, 1e3, n_random // 2)])
  x = np.concatenate([special, rand])
  mark = np.zeros(len(x), bool)
  mark[:len(special)] = True
  return x, mark


def _step_ulps(x, d):
  x = x.copy()
  for _ in range(abs(d)):
    x = np.nextafter(x, np.inf if d > 0 else -np.inf)
  return x


def sincos_err_mp(x, sn, cs):
  """absolute errors against mpmath, as floats (the difference is formed in mpmath)"""
  es, ec = np.empty(len(x)), np.empty(len(x))
  for i, (xi, si, ci) in enumerate(zip(x.tolist(), sn.tolist(), cs.tolist())):
    c, s = mpmath.cos_sin(mpmath.mpf(xi))
    es[i], ec[i] = float(abs(mpmath.mpf(si) - s)), float(abs(mpmath.mpf(ci) - c))
  return es, ec


def sincos_err_ld(x, sn, cs):
  xl = x.astype(LD)
  return np.abs(sn.astype(LD) - np.sin(xl)).astype(np.float64), np.abs(cs.astype(LD) - np.cos(xl)).astype(np.float64)


def restate_sincos(x):
  """csrc/physics_math.h sincos_mod in exact arithmetic with one rounding per operation (fma: one rounding) -- the CPU statement of what the kernel should return"""
  m, r_ = mpmath.mpf, _rnd
  x = m(x)
  k = m(float(np.rint(float(r_(x * m(6.36619772367581382433e-01))))))
  r = r_(-k * m(1.57079632673412561417e+00) + x)
  r = r_(-k * m(6.07710050650619224932e-11) + r)
  z = r_(r * r)
  ps = r_(z * m(1.58969099521155010221e-10) + m(-2.50507602534068634195e-08))
  for c in (2.75573137070700676789e-06, -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01):
    ps = r_(z * ps + m(c))
  sr = r_(r_(r * z) * ps + r)
  pc = r_(z * m(-1.13596475577881948265e-11) + m(2.08757232129817482790e-09))
  for c in (-2.75573143513906633035e-07, 2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02):
    pc = r_(z * pc + m(c))
  cr = r_(r_(z * z) * pc + r_(m(-0.5) * z + 1))
  q = int(k) & 3
  sn = (sr, cr, -sr, -cr)[q]
  cs = (cr, -sr, -cr, sr)[q]
  return float(sn), float(cs)


# ---------------------------------------------------------------------------------------------------------------- C: impedance and cone
def model_sol_rows():
  """every distinct solref and solimp row that earl_benchmark_amd/models/*.npz hold"""
  refs, imps = set(), set()
  for f in sorted(glob.glob(os.path.join(REPO, 'earl_benchmark_amd', 'models', '*.npz'))):
    with np.load(f) as z:
      for k in z.files:
        if k.endswith('solref'):
          refs |= {tuple(r) for r in np.asarray(z[k], float).reshape(-1, 2).tolist()}
        if k.endswith('solimp'):
          imps |= {tuple(r) for r in np.asarray(z[k], float).reshape(-1, 5).tolist()}
  return sorted(refs), sorted(imps)


def impedance_ref(solimp, r):
  """MuJoCo's impedance d(r) (documentation, "Solver parameters": x = |r| / width clipped to 1; y(x) = x for power 1, else x^p / mid^(p - 1) below the midpoint and
  1 - (1 - x)^p / (1 - mid)^(p - 1) above it; d = d0 + y (dwidth - d0)), in mpmath.  width = 0 is taken as the limit width -> 0+ (x = 1, d = dwidth), which is what
  the kernels and the model tables mean by it.  The quotients are written as products with the exponent 1 - p so that mid = 0 (rows of the 3-number legacy form,
  padded with mid = power = 0) is the limit 0 and not a division by zero."""
  d0, dw, width, mid, power = (mpmath.mpf(v) for v in solimp)
  x = min(abs(mpmath.mpf(r)) / width, mpmath.mpf(1)) if width > 0 else mpmath.mpf(1)
  if power == 1 or d0 == dw:
    y = x
  elif x <= mid:
    y = (x ** power) * (mid ** (1 - power)) if mid > 0 else mpmath.mpf(0)
  else:
    y = 1 - ((1 - x) ** power) * ((1 - mid) ** (1 - power))
  return d0 + y * (dw - d0)


def kb_ref(solref, solimp, dt):
  tc, dr, dw = max(mpmath.mpf(solref[0]), 2 * mpmath.mpf(dt)), mpmath.mpf(solref[1]), mpmath.mpf(solimp[1])
  return 1 / (dw * dw * tc * tc * dr * dr), 2 / (dw * tc)


def impedance_cases(seed=2):
  """rows of 9: solref (2), solimp (5), r, dt"""
  rng = np.random.default_rng(seed)
  refs, imps = model_sol_rows()
  rows = []
  rs_of = lambda width, mid: [0.0, -0.0, width, -width, 2 * width, 1e3, mid * width, -mid * width, np.nextafter(mid * width, 0), np.nextafter(mid * width, 1), 0.25 * width, 0.75 * width, 1e-12, 0.999 * width]
  for ref in refs:                                                # the models' own rows, every pairing, at the models' timesteps (0.0025 Sawyer, 0.002 kitchen / minitaur) and at one that clamps
    for imp in imps:
      for dt in (0.0025, 0.002, 0.02):
        for r in rs_of(imp[2], imp[3]) + (rng.uniform(-1.5, 1.5, 6) * imp[2]).tolist():
          rows.append([*ref, *imp, r, dt])
  for power in (1.0, 2.0, 3.0, 2.5):                              # the pow branches
    for mid in (0.5, 0.05, 0.95, 0.25):
      for d0, dw in ((0.9, 0.95), (0.5, 0.5), (0.0001, 0.9999), (0.95, 0.9)):
        for width in (0.001, 0.0, 1.0, 0.0625):
          for ref in ((0.02, 1.0), (0.001, 1.0), (0.004, 0.7), (0.5, 2.0)):      # solref[0] < 2 dt: the clamp
            w = width if width > 0 else 1.0
            for r in rs_of(w, mid) + (rng.uniform(-1.2, 1.2, 4) * w).tolist():
              rows.append([*ref, d0, dw, width, mid, power, r, 0.0025])
  return np.array(rows, dtype=np.float64)


def cone_matrix(w, ell):
  """the explicit 3 x 3 matrix of csrc/physics_lds.h cone_apply's comment, longdouble; w: [n][5]"""
  w = w.astype(LD)
  W = np.zeros((len(w), 3, 3), LD)
  if ell:
    K, m1, m2, q, i2 = (w[:, k] for k in range(5))
    m = np.stack([np.ones_like(K), m1, m2], 1)
    W = K[:, None, None] * m[:, :, None] * m[:, None, :]
    mt = m[:, 1:]
    W[:, 1:, 1:] += q[:, None, None] * (np.eye(2, dtype=LD)[None] - mt[:, :, None] * mt[:, None, :] * i2[:, None, None])
  else:
    W[:, 0, 0], W[:, 0, 1], W[:, 0, 2], W[:, 1, 1], W[:, 2, 2] = (w[:, k] for k in range(5))
    W[:, 1, 0], W[:, 2, 0] = w[:, 1], w[:, 2]
  return W


def cone_zone_inputs(seed=3, n=1_000_000):
  rng = np.random.default_rng(seed)
  r = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-6, 3, (n, 1))
  mu = np.where(rng.random(n) < 0.05, 0.0, 10.0 ** rng.uniform(-2, 0.5, n))
  r[rng.random(n) < 0.03, 0] = 0.0                      # r0 = 0
  z = rng.random(n) < 0.03
  r[z, 1] = 0.0; r[z, 2] = 0.0                          # rho = 0
  return np.concatenate([r, mu[:, None]], 1)


def cone_zone_ref(c):
  """-> (zone, decided): the three-way rule in longdouble with the margins of the two comparisons; decided = both margins beyond 8 u (|r0| + mu rho + rho).
  (longdouble: its 2^-64 is 2^-8 of the margin asked for; test_physics_primitives.py checks a subsample against mpmath)"""
  r0, r1, r2, mu = (c[:, k].astype(LD) for k in range(4))
  rho = np.sqrt(r1 * r1 + r2 * r2)
  m_top, m_bot = r0 - mu * rho, -mu * r0 - rho          # top: m_top >= 0; bottom: m_bot >= 0
  zone = np.where(m_top >= 0, 0, np.where(m_bot >= 0, 1, 2))
  tol = 8 * LD(U) * (np.abs(r0) + mu * rho + rho)
  decided = (np.abs(m_top) > tol) & (np.abs(m_bot) > tol)
  return zone.astype(np.int32), decided


def cone_zone_boundary():
  """exactly representable boundary cases: (r1, r2) = (3, 4) -> rho = 5, mu = 0.5 -> mu rho = 2.5 and rho = -mu r0 at r0 = -10.  The source says `r0 >= mu rho` -> top
  and `rho <= -mu r0` -> bottom, so both boundaries belong to the outer zones."""
  rows, want = [], []
  for s in (1.0, 2.0, 0.5, 2.0 ** -30, 2.0 ** 40):
    rows += [[2.5 * s, 3 * s, 4 * s, 0.5], [-2.5 * s, 3 * s, 4 * s, 0.5], [-10 * s, 3 * s, 4 * s, 0.5], [np.nextafter(2.5 * s, 0), 3 * s, 4 * s, 0.5],
             [np.nextafter(-10 * s, 0), 3 * s, 4 * s, 0.5], [0.0, 0.0, 0.0, 0.5], [0.0, 3 * s, 4 * s, 0.0], [s, 3 * s, 4 * s, 0.0], [-s, 3 * s, 4 * s, 0.0], [-s, 0.0, 0.0, 0.0]]
    want += [0, 2, 1, 2, 2, 0, 0, 0, 2, 1]
  return np.array(rows), np.array(want, np.int32)


# ---------------------------------------------------------------------------------------------------------------- D: SPD systems
CONDS = (1e2, 1e8, 1e12)
PER_SUB = 384        # 3 conditions x plain / scaled x 384 = 2304 >= 2048 systems per family and size (a multiple of 4: whole wavefronts)


def spd_batch(n, cond, m, rng, scaled):
  """m matrices Q diag(lambda) Q' with lambda log-spaced over [1, cond]; scaled: rows and columns times 10^U(-3, 3)"""
  Q = np.linalg.qr(rng.standard_normal((m, n, n)))[0]
  lam = cond ** (np.arange(n) / (n - 1))
  lam = np.stack([rng.permutation(lam) for _ in range(m)])
  A = np.einsum('mik,mk,mjk->mij', Q, lam, Q)
  A = 0.5 * (A + A.transpose(0, 2, 1))
  # what the bounds speak of is the condition of the EQUILIBRATED matrix (unit diagonal), which for small n can fall well below lambda's: draw again until it is
  # within a factor 4 of the nominal one (the CPU test asserts a factor 10 on every system)
  for _ in range(200):
    c = cond2_equilibrated(A) / cond
    redo = np.flatnonzero((c < 0.25) | (c > 4))
    if not len(redo):
      break
    Qr = np.linalg.qr(rng.standard_normal((len(redo), n, n)))[0]
    Ar = np.einsum('mik,mk,mjk->mij', Qr, lam[redo], Qr)
    A[redo] = 0.5 * (Ar + Ar.transpose(0, 2, 1))
  if scaled:
    s = 10.0 ** rng.uniform(-3, 3, (m, n))
    A = A * s[:, :, None] * s[:, None, :]
  return A


def family(kind, nv, seed=4):
  """-> dict(H [n][nv][nv], dl [n][nv], b [n][nv], A [n][nv][nv] longdouble = the system the kernels are asked to solve (H + diag dl, zeros where nothing is read),
  act = number of leading unknowns the form solves, nominal [n] condition numbers).  kind: 'dense' | 'blocks' (block diagonal [0, NA) + [NA, NV), the off-diagonal
  block NaN in H) | 'lead' (arm block + decoupled positive diagonal; only the arm block is solved)"""
  rng = np.random.default_rng(seed * 1000 + nv * 10 + {'dense': 0, 'blocks': 1, 'lead': 2}[kind])
  na = NA_OF[nv]
  Hs, noms = [], []
  for cond in CONDS:
    for scaled in (False, True):
      if kind == 'dense':
        A = spd_batch(nv, cond, PER_SUB, rng, scaled)
      else:
        A = np.zeros((PER_SUB, nv, nv))
        A[:, :na, :na] = spd_batch(na, cond, PER_SUB, rng, scaled)
        if kind == 'blocks':
          A[:, na:, na:] = spd_batch(nv - na, cond, PER_SUB, rng, scaled)
        else:
          idx = np.arange(na, nv)
          A[:, idx, idx] = 10.0 ** rng.uniform(-3, 3, (PER_SUB, nv - na))
      Hs.append(A); noms.append(np.full(PER_SUB, cond))
  A = np.concatenate(Hs)
  il = np.tril_indices(nv, -1)
  A[:, il[1], il[0]] = A[:, il[0], il[1]]              # exactly symmetric (the scaling rounds (i, j) and (j, i) differently): forms that read different triangles see the same numbers
  nom = np.concatenate(noms)
  perm = rng.permutation(len(A))                       # different kinds of systems side by side in a wave
  A, nom = A[perm], nom[perm]
  n = len(A)
  d = np.arange(nv)
  dl = rng.uniform(0, 0.5, (n, nv)) * A[:, d, d]
  H = A.copy()
  H[:, d, d] = A[:, d, d] - dl
  b = rng.standard_normal((n, nv)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
  Aeff = H.astype(LD)
  Aeff[:, d, d] = H[:, d, d].astype(LD) + dl.astype(LD)
  H0 = H.copy()                                        # for the forms that read the whole matrix: zeros there
  if kind == 'blocks':
    H[:, na:, :na] = np.nan; H[:, :na, na:] = np.nan   # the claim: never read
  act = na if kind == 'lead' else nv
  return dict(H=H, H0=H0, dl=dl, b=b, A=Aeff, act=act, nominal=nom, nv=nv, kind=kind)


def chol_solve(A, b, dtype):
  """the inverted-diagonal Cholesky and the two substitutions, plainly, batched over the first axis in `dtype` (float64: the fp64 reference the issue measures the
  bound against; longdouble: the reference solution)"""
  A = A.astype(dtype); x = b.astype(dtype).copy()
  n = A.shape[1]
  L = np.zeros_like(A)
  for j in range(n):
    d = A[:, j, j] - np.einsum('mp,mp->m', L[:, j, :j], L[:, j, :j])
    inv = 1 / np.sqrt(d)
    L[:, j, j] = inv
    if j + 1 < n:
      L[:, j + 1:, j] = (A[:, j + 1:, j] - np.einsum('mip,mp->mi', L[:, j + 1:, :j], L[:, j, :j])) * inv[:, None]
  for i in range(n):
    x[:, i] = (x[:, i] - np.einsum('mp,mp->m', L[:, i, :i], x[:, :i])) * L[:, i, i]
  for i in range(n - 1, -1, -1):
    x[:, i] = (x[:, i] - np.einsum('mp,mp->m', L[:, i + 1:, i], x[:, i + 1:])) * L[:, i, i]
  return x


def solve_ld(A, b):
  """longdouble solution with two steps of iterative refinement (residuals in longdouble)"""
  x = chol_solve(A, b, LD)
  for _ in range(2):
    r = b.astype(LD) - np.einsum('mij,mj->mi', A.astype(LD), x)
    x = x + chol_solve(A, r, LD)
  return x


def equilibrated(A):
  d = np.sqrt(A[:, np.arange(A.shape[1]), np.arange(A.shape[1])])
  return A / d[:, :, None] / d[:, None, :], d


def backward_error(A, xhat, b):
  """eta = ||b~ - A~ x~||inf / (||A~||inf ||x~||inf + ||b~||inf) with D = diag(A)^1/2, A~ = D^-1 A D^-1, x~ = D xhat, b~ = D^-1 b, in longdouble; per system"""
  A = A.astype(LD)
  At, d = equilibrated(A)
  xt, bt = d * xhat.astype(LD), b.astype(LD) / d
  res = np.abs(bt - np.einsum('mij,mj->mi', At, xt)).max(1)
  return (res / (np.abs(At).sum(2).max(1) * np.abs(xt).max(1) + np.abs(bt).max(1))).astype(np.float64)


def cond2_equilibrated(A):
  return np.linalg.cond(equilibrated(A)[0].astype(np.float64))


def active(fam):
  """the leading block the form solves: (A, b) restricted to it"""
  k = fam['act']
  return fam['A'][:, :k, :k], fam['b'][:, :k]


def spoil(fam, H, kinds=('neg0', 'negmid', 'neglast', 'nan', 'inf')):
  """a copy of the family's inputs in which ONE env of every wavefront (which one rotates) gets a bad matrix: a negative pivot at column 0 / in the middle / last
  (A_jj lowered by twice its pivot), a NaN entry, an Inf entry -- within the block the form reads.  H: the family's H or H0.  -> (H, bad mask, kind index per system)"""
  nv, k = fam['nv'], fam['act']
  epw = 64 // LPE_OF[nv]
  H = H.copy()
  n = len(H)
  bad = np.zeros(n, bool)
  which = np.full(n, -1)
  A = fam['A'].astype(np.float64)
  for w in range(n // epw):
    e = w * epw + w % epw
    kind = kinds[w % len(kinds)]
    bad[e], which[e] = True, w % len(kinds)
    if kind.startswith('neg'):
      j = {'neg0': 0, 'negmid': k // 2, 'neglast': k - 1}[kind]
      Aj = np.nan_to_num(A[e, :j + 1, :j + 1])
      piv = Aj[j, j] - (Aj[j, :j] @ np.linalg.solve(Aj[:j, :j], Aj[:j, j]) if j else 0.0)
      H[e, j, j] -= 2 * piv
    elif kind == 'nan':
      H[e, 1, 0] = H[e, 0, 1] = np.nan
    else:
      H[e, 2, 2] = np.inf
  return H, bad, which


# ---------------------------------------------------------------------------------------------------------------- E: scans
def chains(nv):
  """-> (anc, desc): per lane of a 16-lane row the lanes its inclusive ancestor / subtree sum runs over; None = the lane is outside every chain (untouched).
  Arm 0 ... 6 in series, fingers 7 and 8 on link 6; nv 15: the free body's chain 9 ... 14."""
  anc, desc = [None] * 16, [None] * 16
  for s in range(7):
    anc[s] = list(range(s + 1))
    desc[s] = list(range(s, 9))
  for f in (7, 8):
    anc[f] = list(range(7)) + [f]
    desc[f] = [f]
  if nv == 15:
    for s in range(9, 15):
      anc[s] = list(range(9, s + 1))
      desc[s] = list(range(s, 15))
  return anc, desc


def scan_ref(x, nv, which):
  """x: [rows][16][N] integer-valued doubles -> the tree sums, lane by lane in plain Python; lanes outside the chains keep their value"""
  table = chains(nv)[0 if which == 'anc' else 1]
  out = x.copy()
  rows = slice(0, None, 2) if LPE_OF[nv] == 32 else slice(None)      # 32 lanes per env: the chains sit in the env's first row, its second row is outside
  for s in range(16):
    if table[s] is not None:
      out[rows, s] = sum(x[rows, t] for t in table[s])
  return out


def recorded_family(name):
  """Hessians and right-hand sides of real door (nv 10) / peg (nv 15) timesteps in contact, recorded from this project's CPU statement of the stepper by
  tests/golden/make_primitive_hessians.py, in the shape of family(): a quarter of the diagonal goes through dl.  'joined' marks the peg systems in which a contact
  couples arm and peg (the others are block diagonal and can go to chol_regs<15, 9>)"""
  with np.load(os.path.join(REPO, 'tests', 'golden', 'primitive_hessians.npz')) as z:
    A, b = z[name + '_H'], z[name + '_g']
  n, nv = b.shape
  d = np.arange(nv)
  dl = 0.25 * A[:, d, d]
  H = A.copy()
  H[:, d, d] = A[:, d, d] - dl
  Aeff = H.astype(LD)
  Aeff[:, d, d] = H[:, d, d].astype(LD) + dl.astype(LD)
  na = NA_OF[nv]
  joined = np.abs(A[:, na:, :na]).max((1, 2)) > 0 if na < nv else np.zeros(n, bool)
  return dict(H=H, H0=H, dl=dl, b=b, A=Aeff, act=nv, nominal=None, nv=nv, kind='dense', joined=joined)

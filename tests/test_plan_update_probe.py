"""CPU side of the update-kernel tests (tests/test_plan_update_gpu.py), no GPU:
  A. the probe (tests/plan_update_probe.hip) is built with the Makefile's HIPFLAGS, both builds cross-compile for gfx950, and the update kernel inside each probe is,
     instruction for instruction, the one csrc/<unit>.hip compiles to on its own (whole normalised function bodies compared: kernel_build.Unit.functions);
  B. the crafted return columns are what their names say BY THE ORACLE ALONE at every shape the GPU test runs, and the host twin equals the Python integers on them
     (so that a difference on the device says something about the kernel);
  C. the integer contract against MPPI itself in mpmath: how far the contract's new mean lies from the softmax-weighted mean it stands for, under a derived bound."""
import shutil
import subprocess

import mpmath
import numpy as np
import pytest

import kernel_build
import plan_update_cases as pc
import primitives_ref as R
from earl_benchmark_amd import _abi
from tabletop_plan_helpers import exp_f32

F32, F64 = np.float32, np.float64
mpf = mpmath.mpf


# ---------------------------------------------------------------------------------------------------------------- A. the probe
def test_probe_flags_are_the_makefiles_hipflags(monkeypatch):
  assert pc.HIPFLAGS == R.makefile_hipflags()
  seen = []
  monkeypatch.setattr(subprocess, 'check_call', lambda cmd: seen.append(cmd))
  for unit in pc.UNITS.values():
    pc.compile_probe(unit, out='x.so')
  flags = R.makefile_hipflags()
  assert seen == [['hipcc', *flags, '-DEARL_PROBE_SAWYER=1', '-shared', '-o', 'x.so', pc.SRC], ['hipcc', *flags, '-shared', '-o', 'x.so', pc.SRC]]


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='no hipcc')
@pytest.mark.parametrize('name', list(pc.UNITS))
def test_probe_cross_compiles_for_gfx950_with_the_product_flags(tmp_path, name):
  unit = pc.UNITS[name]
  out = pc.compile_probe(unit, out=str(tmp_path / 'libprobe.so'))
  blob = open(out, 'rb').read()
  assert unit.launcher.encode() in blob and unit.kernel.encode() in blob
  other = [u for u in pc.UNITS.values() if u is not unit][0]
  assert other.launcher.encode() not in blob, 'one unit per build: the two cannot share a translation unit'


@pytest.mark.parametrize('name', list(pc.UNITS))
def test_the_kernel_inside_the_probe_is_the_products(tmp_path, name):
  """the probe's device code, compiled as kernel_build compiles a unit, holds the unit's two kernels under their own names with bodies equal line for line"""
  kernel_build.need_hipcc()
  unit = pc.UNITS[name]
  asm = str(tmp_path / 'probe.s')
  subprocess.run([kernel_build.HIPCC, *kernel_build.tool().FLAGS, *unit.defines, '-o', asm, pc.SRC], check=True, capture_output=True)
  probe = kernel_build.normalised_functions(open(asm).read().split('\n'))
  product = kernel_build.unit(unit.source).functions
  mine = [k for k in product if unit.kernel in k]
  assert len(mine) == 1 and sorted(probe) == sorted(product), (sorted(probe), sorted(product))
  for k, body in product.items():
    assert len(body) > 100 and probe[k] == body, f'{k}: the probe compiles another body than csrc/{unit.source}'
  text = open(pc.SRC).read()
  assert f'#include "../earl_benchmark_amd/csrc/{unit.source}"' in text and '__global__' not in text, 'the probe holds no kernel text of its own'


# ---------------------------------------------------------------------------------------------------------------- B. the columns, on the oracle
@pytest.mark.parametrize('K,H', [(1, 9), (2, 19), (65, 9), (513, 1), (1100, 8)])
@pytest.mark.parametrize('name', list(pc.UNITS))
def test_columns_are_what_their_names_say_and_the_twin_equals_python_integers(name, K, H):
  unit = pc.UNITS[name]
  host = _abi.load_host()
  for inv_t in (2.0, 1e-6, 1e6):
    cols = pc.columns(K, inv_t)
    assert set(cols) >= {'distinct', 'all NaN', 'all -Inf', 'one +Inf', 'all equal', 'near 1e300'}
    assert ('tie 511 / 512' in cols) == (K >= 513) and ('tie 16 / 32' in cols) == (K >= 33) and ('tie 63 / 64' in cols) == (K >= 65) and ('one weight' in cols) == (K >= 2)
    for group, ret in pc.groups(cols):
      mean, act, m = pc.drawn(name, K, H, len(group))
      want, twin = pc.expected(unit, mean, act, m, ret, inv_t, host)
      pc.check_columns(group, ret, want, inv_t)
      pc.compare(twin, want, f'({name}, K = {K}, H = {H}, 1/T = {inv_t}, {group})')
      for i, c in enumerate(group):
        if c in ('all NaN', 'all -Inf', 'one +Inf'):
          pc.mp.same_bits(want['plan'][:, i], m[:, i], c + ': S == 0, the plan is the clipped mean')


def test_every_finite_column_is_in_part_c():
  cols = pc.columns(8192, 2.0)
  finite = [k for k, r in cols.items() if np.isfinite(r).all()]
  assert finite == list(pc.FINITE) and len(cols) == len(pc.COLUMNS)


# ---------------------------------------------------------------------------------------------------------------- C. the contract against MPPI
X_LOW = -18.0                 # exp(-18) < 2^-25: below it a weight is 0 in the contract and below half a quantum in MPPI; the relative error of exp_f32 is measured above it


def exp_f32_error(x):
  """max |exp_f32(x) / exp(x) - 1| over float32 x, exp_f32 from the policy-math host build (what the oracle calls), exp in mpmath"""
  x = np.unique(np.asarray(x, F32))
  e = exp_f32(x)
  return max((abs(mpf(float(ev)) / mpmath.exp(mpf(float(xv))) - 1) for xv, ev in zip(x.tolist(), e.tolist())), default=mpf(0))


def contract_bound(K, delta, X, eta):
  """|contract - MPPI| per word of the new mean, as the docstring of test_contract_against_mppi_in_high_precision derives it"""
  u32, u64 = mpf(2)**-24, mpf(2)**-53
  theta = (1 + u64)**2 * (1 + u32) - 1
  tau = X * theta / (1 - theta) + mpf(2)**-149
  rho = (1 + eta) * mpmath.exp(tau) - 1
  eps_d = mpf(2)**-21 + u32 * delta
  weights = 2 * delta * (K * mpf(2)**-25 + rho) / (1 - rho)
  mu = delta + eps_d
  final = mu * ((1 + u64)**2 - 1) + (u32 * mu * (1 + mpf(2)**-51) + mpf(2)**-150) + u32 * (1 + mu * (1 + mpf(2)**-23))
  return eps_d + weights + final


def mppi_reference(act, m, r, inv_t):
  """one env: act [K, H, dim] and m [H, dim] float32, r [K] finite float64 -> clip(m + sum_k w_k (c_k - m) / sum_k w_k), w_k = exp((r_k - beta) inv_t), in mpmath"""
  beta, it = mpf(float(r.max())), mpf(float(inv_t))
  w = [mpmath.exp((mpf(v) - beta) * it) for v in r.tolist()]
  sw = mpmath.fsum(w)
  out = np.empty(m.shape, object)
  for t in range(m.shape[0]):
    for d in range(m.shape[1]):
      mm = mpf(float(m[t, d]))
      v = mm + mpmath.fdot(w, [mpf(c) - mm for c in act[:, t, d].tolist()]) / sw
      out[t, d] = min(max(v, mpf(-1)), mpf(1))
  return out


@pytest.mark.parametrize('K', [2, 65, 1100, 8192])
def test_contract_against_mppi_in_high_precision(K):
  """What the integer MPPI update costs in accuracy: the Python-integer oracle and the host twin against
      new* = clip(m + sum_k w_k (c_k - m) / sum_k w_k),   w_k = exp((r_k - beta) inv_t)
  in mpmath (240 bits) on the same float32 candidates c_k and clipped mean m, for EVERY finite return column of the GPU test (plan_update_cases.FINITE) at inv_t = 2
  and, where the GPU test runs them (K = 65 and 1100), at inv_t = 1e-6 and 1e6; eight action dimensions (the Sawyer twin on dimensions 0 .. 3 of the same arrays).

  The contract: x_k = fl32(fl64(fl64(r_k - beta) inv_t)), a_k = W_k 2^-24 = rint(exp_f32(x_k) 2^24) 2^-24, D_k 2^-20 = rint(fl32(c_k - m) 2^20) 2^-20,
  new = clip(fl32(m + fl32(fl64(fl64(A) / (S 2^20))))) with A = sum W_k D_k and S = sum W_k exact integers (S 2^20 < 2^53 is exact).
  With Delta = max |c_k - m|, X = max |x_k| over x_k >= -18, eta = max |exp_f32(x) / exp(x) - 1| over those x, u32 = 2^-24, u64 = 2^-53:
    deltas    |D_k 2^-20 - (c_k - m)| <= 2^-21 (half the delta quantum) + u32 Delta (the float32 subtraction) =: eps_D; D_0 = 0 = c_0 - m.  A weighted mean of the D_k 2^-20
              lies within eps_D of the same weighted mean of the c_k - m.
    weights   y_k = (r_k - beta) inv_t exactly; x_k = y_k (1 + e), |e| <= theta = (1 + u64)^2 (1 + u32) - 1 (two double roundings, one float32 rounding), so
              |x_k - y_k| <= tau = X theta / (1 - theta) + 2^-149 (a subnormal x_k).  For x_k >= -18:
              |a_k - w_k| <= 2^-25 (half the weight quantum) + w_k rho, rho = (1 + eta) e^tau - 1.  For x_k < -18 (-Inf included): a_k = 0 (asserted on the oracle) and
              w_k < e^(-18 / (1 + theta)) < 2^-25.  So sum |a_k - w_k| =: E <= K 2^-25 + rho sum w_k, and with sum w_k <= sum a_k + E: E <= (K 2^-25 + rho sum a_k) / (1 - rho).
              Two weighted means of the same values of size <= Delta under weights a and w differ by at most Delta * 2 E / sum a_k, and sum a_k >= 1 (the best
              candidate has x = 0 and a = 1):  <= 2 Delta (K 2^-25 + rho) / (1 - rho).
    the end   mu = A / (S 2^20), |mu| <= Delta + eps_D =: M.  fl64(A) and the division: M ((1 + u64)^2 - 1); to float32: u32 M (1 + 2^-51) + 2^-150; the float32
              sum with m: u32 (1 + M (1 + 2^-23)).  The clip moves two numbers no further apart.
    bound     eps_D + 2 Delta (K 2^-25 + rho) / (1 - rho) + the end's three terms  (contract_bound above; dominated by K 2^-24 Delta: every weight may be off by half
              a quantum while the sum of the weights is only known to be >= 1).
  eta is MEASURED here, on the host build of exp_f32 against mpmath, over every x_k >= -18 of the test's own columns and 4096 more float32 in [-18, 0]: a property of
  the reference side, printed and recorded in DESIGN.md, never hard-coded.  Asserted: oracle <= bound and twin <= bound per word; printed: the observed worst distance."""
  host = _abi.load_host()
  unit, saw = pc.UNITS['minitaur'], pc.UNITS['sawyer']
  H = 2 if K <= 1100 else 1
  mean, act, m = pc.drawn('minitaur', K, H, 1)
  delta = float(np.abs(act.astype(F64) - m[None].astype(F64)).max()) * (1 + 2.0**-50)
  grid = np.concatenate([np.random.default_rng(K).uniform(X_LOW, 0.0, 4094), [X_LOW, 0.0]]).astype(F32)
  cases, xs = [], [grid]
  temps = (2.0, 1e-6, 1e6) if K in (65, 1100) else (2.0,)
  for inv_t in temps:
    for name, r in pc.columns(K, inv_t, pc.FINITE).items():
      assert np.isfinite(r).all()
      with np.errstate(over='ignore'):
        x = ((r - r.max()) * F64(inv_t)).astype(F32)
      xs.append(x[x >= X_LOW])
      cases.append((inv_t, name, r, x))
  assert {c[1] for c in cases} == set(pc.columns(K, 2.0, pc.FINITE)) and len(cases) == len(temps) * len(pc.columns(K, 2.0, pc.FINITE))
  used = np.concatenate(xs)
  eta = exp_f32_error(used)
  X = float(np.abs(used).max())
  bound = contract_bound(K, mpf(delta), mpf(X), eta)
  print(f'PLAN-FIG K = {K}: exp_f32 relative error eta = {float(eta):.3e} over {len(np.unique(used))} x in [{X_LOW}, 0]; Delta = {delta:.6f}, X = {X:.4f}, bound = {float(bound):.3e}')
  worst = {'oracle': mpf(0), 'twin': mpf(0), 'sawyer twin': mpf(0)}
  for inv_t, name, r, x in cases:
    ret = r[:, None]
    want, twin = pc.expected(unit, mean, act, m, ret, inv_t, host)
    assert (want['W'][x < X_LOW, 0] == 0).all() and want['W'][int(np.argmax(r)), 0] == pc.FULL
    ref = mppi_reference(act[:, :, 0], m[:, 0], r, inv_t)
    a4, mean4 = np.ascontiguousarray(act[..., :4]), np.ascontiguousarray(mean[..., :4])
    stwin = saw.helpers.host_update(host, saw.cfg(1), saw.params(K, H, inv_t), pc.J, mean4, a4, ret)
    dist = lambda plan, ref: max(abs(mpf(float(p)) - q) for p, q in zip(plan.reshape(-1).tolist(), ref.reshape(-1).tolist()))
    d = {'oracle': dist(want['plan'][:, 0], ref), 'twin': dist(twin['plan'][:, 0], ref), 'sawyer twin': dist(stwin['plan'][:, 0], ref[:, :4])}
    for k, v in d.items():
      worst[k] = max(worst[k], v)
      assert v <= bound, f'K = {K}, 1/T = {inv_t}, {name}: {k} is {float(v):.3e} from MPPI, the derived bound is {float(bound):.3e}'
  print(f'PLAN-FIG K = {K}: worst |contract - MPPI| over {len(cases)} columns: ' + ', '.join(f'{k} {float(v):.3e}' for k, v in worst.items()) + f' (bound {float(bound):.3e})')

"""The probe around the two MPPI update kernels, its build recipe, and the crafted inputs of tests/test_plan_update_gpu.py (the kernels on the device) and
tests/test_plan_update_probe.py (no GPU: the build, the kernel text, the contract against MPPI in high precision); a plain module.

THE PROBE is tests/plan_update_probe.hip: it includes csrc/sawyer_plan.hip (-DEARL_PROBE_SAWYER=1) or csrc/minitaur_plan.hip and adds one launcher with the host
twin's arguments plus a stream.  Built on demand with the Makefile's HIPFLAGS, as tests/primitives_ref.py builds its unit; libearl_hip.so is loaded RTLD_GLOBAL first, so
that the public calls the included unit refers to resolve.

THE EXPECTATIONS use nothing the device returned: the numpy Philox candidates of tests/sawyer_plan_helpers.py / minitaur_plan_helpers.py, items 4 - 7 in Python integers
(tests/tabletop_plan_helpers.py: weights / update, update_fast in int64 where K is large) and the host twin earl_*_plan_update_cpu on the same arrays.

THE RETURN COLUMNS (COLUMNS below: name -> maker and the check, ON THE ORACLE, that the column is what its name says) are one env each.  The ties: (0, K - 1) the
first and the last candidate; (16, 32) two lanes of one wave that the shuffle butterfly of block_best joins in an order other than ascending k (lane 0 meets lane 32
before lane 16: without the `k < bk` rule the wave reports 32); (63, 64) the last lane of wave 0 and the first of wave 1; (511, 512) the last lane of the workgroup and
lane 0's second pass."""
import ctypes as C
import functools
import glob
import os
import subprocess

import numpy as np

import minitaur_plan_helpers as mp
import sawyer_plan_helpers as sp
from earl_benchmark_amd import _abi
from primitives_ref import CSRC, HIPFLAGS, REPO

F32, F64 = np.float32, np.float64
SRC = os.path.join(REPO, 'tests', 'plan_update_probe.hip')
UPDATE_THREADS, UPDATE_WAVES = 512, 8      # kUpdateThreads / kUpdateWaves of both units (the probe reports the first: `load` asserts it)
SEED, OFF, NC, J = 0x1234567890ABCDEF, 5, 0x9E3779B9, 4
SIGMA = (0.5, 0.0, 0.8, 0.3, 0.2, 0.6, 0.4, 0.7)
FULL = 2**24                                # the weight of a return equal to beta
PLAN_FILL, RET_FILL, K_FILL = 7.0, -12345.0, -7      # sentinels no output can equal: a plan word lies in +-1, the returns of every case differ from RET_FILL, best_k >= 0


class Unit:
  def __init__(self, name, dim, helpers, defines, source, kernel, max_k):
    self.name, self.dim, self.helpers, self.defines, self.source, self.kernel, self.max_k = name, dim, helpers, defines, source, kernel, max_k
    self.launcher = f'probe_{name}_plan_update'
    self.so = os.path.join(REPO, 'tests', f'libplan_update_probe_{name}.so')

  def candidates(self, n, K, H, mean):
    """items 1 - 2 -> (act [K, H, n, dim], m [H, n, dim]) with this module's seed, offset, iteration and counters"""
    return self.helpers.candidates(SEED, OFF, n, K, H, J, SIGMA[:self.dim], NC, mean)[:2]

  def cfg(self, n):
    return self.helpers.cfg_of(n, OFF, SEED)

  def params(self, K, H, inv_t):
    return self.helpers.params(K, H, sigma=SIGMA[:self.dim], inv_t=inv_t, nc=NC)


UNITS = {'sawyer': Unit('sawyer', 4, sp, ['-DEARL_PROBE_SAWYER=1'], 'sawyer_plan.hip', 'sawyer_plan_update_kernel', _abi.SAWYER_PLAN_MAX_K),
         'minitaur': Unit('minitaur', 8, mp, [], 'minitaur_plan.hip', 'minitaur_plan_update_kernel', _abi.MINITAUR_PLAN_MAX_K)}


# ---------------------------------------------------------------------------------------------------------------- the build
def compile_probe(unit, out=None, extra=()):
  """hipcc with the product's flags -> the probe's shared object (extra: e.g. --cuda-device-only -S for the assembly)"""
  out = out or unit.so
  subprocess.check_call(['hipcc', *HIPFLAGS, *unit.defines, *extra, *([] if '-S' in extra else ['-shared']), '-o', out, SRC])
  return out


def build_if_stale(unit):
  deps = [SRC] + glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(REPO, 'include', '*.h'))
  if not os.path.exists(unit.so) or os.path.getmtime(unit.so) < max(os.path.getmtime(d) for d in deps):
    compile_probe(unit)
  return unit.so


@functools.lru_cache(None)
def load(name):
  """the probe of one unit, its launcher typed; the product library first and RTLD_GLOBAL: the included unit's public calls resolve there"""
  unit = UNITS[name]
  _abi.load()
  C.CDLL(_abi.LIB_PATH, mode=C.RTLD_GLOBAL)
  lib = C.CDLL(build_if_stale(unit))
  cfg_t, pp_t = type(unit.cfg(1)), type(unit.params(1, 1, 1.0))
  fn = getattr(lib, unit.launcher)
  fn.argtypes = [C.POINTER(cfg_t), C.POINTER(pp_t), C.c_int32] + [C.c_void_p] * 8
  fn.restype = C.c_int32
  assert lib.probe_plan_update_threads() == UPDATE_THREADS
  return lib


# ---------------------------------------------------------------------------------------------------------------- the means and the candidates
def nasty_mean(H, n, dim, seed):
  """entries beyond +-1, a NaN and both infinities (item 1 clips: NaN -> -1)"""
  mean = np.random.default_rng(seed).uniform(-1.15, 1.15, (H, n, dim)).astype(F32)
  mean[0, 1 % n, 0], mean[1 % H, 2 % n, dim - 1], mean[2 % H, 0, dim - 3] = np.nan, np.inf, -np.inf
  return mean


@functools.lru_cache(None)
def drawn(name, K, H, n):
  """(mean, act, m) of one shape: the oracle's real draws around a nasty mean, made once per process and never written"""
  unit = UNITS[name]
  mean = nasty_mean(H, n, unit.dim, 1000 * K + 10 * H + n)
  act, m = unit.candidates(n, K, H, mean)
  assert bool((np.abs(mean) > 1).any()) and bool(np.isnan(mean).any()) and np.isfinite(act).all() and float(np.abs(act).max()) <= 1.0
  for a in (mean, act, m):
    a.setflags(write=False)
  return mean, act, m


# ---------------------------------------------------------------------------------------------------------------- the return columns
def _base(K, rng):
  """distinct, negative like the envs' dense returns, the maximum away from index 0 where K allows"""
  r = -rng.uniform(0.1, 3.0, K)
  assert len(np.unique(r)) == K
  if K > 1 and int(np.argmax(r)) == 0:
    r[[0, K - 1]] = r[[K - 1, 0]]
  return r


def _tie(a, b):
  def make(K, rng, inv_t):
    i, j = (0, K - 1) if a is None else (a, b)
    if not 0 <= i < j < K:
      return None
    r = _base(K, rng)
    r[[i, j]] = -0.05
    return r

  def check(r, W, beta, bk, inv_t):
    i, j = (0, len(r) - 1) if a is None else (a, b)
    assert beta == -0.05 == r[i] == r[j] and (r == beta).sum() == 2 and bk == i and W[i] == W[j] == FULL, 'the lowest index of a tie wins'
  return make, check


def _distinct(K, rng, inv_t):
  return _base(K, rng)


def _distinct_ok(r, W, beta, bk, inv_t):
  assert len(np.unique(r)) == len(r) and bk == int(np.argmax(r)) and beta == r.max() and W[bk] == FULL and (len(r) == 1 or bk > 0)


def _nan_at_max(K, rng, inv_t):
  if K < 2:
    return None
  r = _base(K, rng)
  r[int(np.argmax(r))] = np.nan
  if int(np.nanargmax(r)) == 0:                                # (the runner-up is not index 0 either where K allows)
    r[[0, 1]] = r[[1, 0]]
  return r


def _nan_at_max_ok(r, W, beta, bk, inv_t):
  nan = np.isnan(r)
  assert nan.sum() == 1 and W[nan].tolist() == [0] and bk == int(np.nanargmax(r)) and beta == np.nanmax(r) and W[bk] == FULL


def _const(v):
  return lambda K, rng, inv_t: np.full(K, v, F64)


def _no_weight_ok(r, W, beta, bk, inv_t):
  assert (W == 0).all() and beta == -np.inf and bk == 0, 'all NaN / all -Inf: no weight, beta = -Inf, best_k = 0'


def _one_pinf(K, rng, inv_t):
  r = _base(K, rng)
  r[K // 2] = np.inf
  return r


def _one_pinf_ok(r, W, beta, bk, inv_t):
  assert np.isinf(r).sum() == 1 and beta == np.inf and bk == len(r) // 2 and (W == 0).all(), '+Inf is beta; every x is NaN or -Inf: S == 0'


def _all_equal_ok(r, W, beta, bk, inv_t):
  assert (r == -1.25).all() and (W == FULL).all() and beta == -1.25 and bk == 0


def _wide(K, rng, inv_t):
  """every other return so far below the best that x < -104, exp_f32's zero threshold"""
  if K < 2:
    return None
  r = -0.5 - rng.uniform(200.0, 400.0, K) / inv_t
  r[K // 2] = -0.5
  return r


def _wide_ok(r, W, beta, bk, inv_t):
  x = ((r - beta) * inv_t).astype(F32)
  others = np.arange(len(r)) != bk
  assert bk == len(r) // 2 and W[bk] == FULL and (W[others] == 0).all() and (x[others] < -104).all()


def _ulp(K, rng, inv_t):
  """-1 and its neighbour towards zero, one ulp above: the first of the larger ones wins, not at index 0"""
  if K < 2:
    return None
  r = np.full(K, -1.0)
  r[1::2] = np.nextafter(-1.0, 0.0)
  return r


def _ulp_ok(r, W, beta, bk, inv_t):
  assert r.max() - r.min() == np.spacing(abs(r.max())) and bk == 1 and beta == r[1] > r[0] and (W[1::2] == FULL).all() and (W >= FULL - 1).all()


def _huge(K, rng, inv_t):
  """magnitudes near 1e300 and the double's top: r - beta overflows to -Inf for the lowest, and (r - beta) * inv_temperature leaves the float32 range for the rest"""
  r = np.array([(-1.5e308, 1e300, -1e300, 1.5e308, 1.2e308, -3e299)[k % 6] * (1 + (k // 6) * 2.0**-20) for k in range(K)])
  return r if K > 1 else np.array([1.5e308])


def _huge_ok(r, W, beta, bk, inv_t):
  with np.errstate(over='ignore'):
    d = r - beta
  assert np.isfinite(r).all() and beta == r.max() and W[bk] == FULL and (len(r) < 4 or (np.isinf(d).any() and (W == 0).sum() >= len(r) // 6))


COLUMNS = {'distinct': (_distinct, _distinct_ok), 'tie 0 / K-1': _tie(None, None), 'tie 16 / 32': _tie(16, 32), 'tie 63 / 64': _tie(63, 64), 'tie 511 / 512': _tie(511, 512),
           'NaN at the maximum': (_nan_at_max, _nan_at_max_ok), 'all NaN': (_const(np.nan), _no_weight_ok), 'all -Inf': (_const(-np.inf), _no_weight_ok),
           'one +Inf': (_one_pinf, _one_pinf_ok), 'all equal': (_const(-1.25), _all_equal_ok), 'one weight': (_wide, _wide_ok), 'one ulp': (_ulp, _ulp_ok),
           'near 1e300': (_huge, _huge_ok)}
FINITE = ('distinct', 'tie 0 / K-1', 'tie 16 / 32', 'tie 63 / 64', 'tie 511 / 512', 'all equal', 'one weight', 'one ulp', 'near 1e300')      # (part C: every column without NaN / Inf)


def columns(K, inv_t, names=None):
  """{name: the column [K]} of every case K allows, in COLUMNS' order"""
  out = {}
  for idx, name in enumerate(COLUMNS if names is None else names):
    r = COLUMNS[name][0](K, np.random.default_rng(100 * K + idx), inv_t)
    if r is not None:
      out[name] = np.asarray(r, F64)
  return out


def groups(cols, size=3):
  """the columns `size` envs at a time -> [(names, ret [K, n])]"""
  names = list(cols)
  return [(names[i:i + size], np.stack([cols[k] for k in names[i:i + size]], 1)) for i in range(0, len(names), size)]


def trip_counts(K, H):
  """what a shape reaches in the update kernel: passes of the workgroup's 512 lanes over the returns / the weights, passes of a wave's 64 lanes over the candidates of a
  step, and the plan steps of wave 0 and of wave 7"""
  steps = lambda w: len(range(w, H, UPDATE_WAVES))
  return dict(lane_passes=-(-K // UPDATE_THREADS), wave_passes=-(-K // 64), steps_wave0=steps(0), steps_wave7=steps(UPDATE_WAVES - 1))


# ---------------------------------------------------------------------------------------------------------------- expectations
def expected(unit, mean, act, m, ret, inv_t, host=None):
  """(the oracle's dict with W, the host twin's dict) of one call; every named column checked on the oracle by the caller"""
  K = act.shape[0]
  with np.errstate(over='ignore', invalid='ignore'):
    want = unit.helpers.oracle_update(act, m, ret, inv_t, fast=K > 512)
  want['best_k'] = want['best_k'].astype(np.int32)
  twin = unit.helpers.host_update(host or _abi.load_host(), unit.cfg(ret.shape[1]), unit.params(K, act.shape[1], inv_t), J, mean, act, ret)
  return want, twin


def check_columns(names, ret, want, inv_t):
  for i, name in enumerate(names):
    COLUMNS[name][1](ret[:, i], want['W'][:, i], want['best_ret'][i], int(want['best_k'][i]), inv_t)


def compare(got, want, what, keys=('plan', 'best_k', 'best_ret', 'ret0')):
  """bit for bit; NaN payloads count as equal in ret0 (minitaur_plan_helpers.same)"""
  for k in keys:
    if k == 'ret0':
      mp.same(got[k], want[k], f'{k} {what}')
    else:
      mp.same_bits(got[k], want[k], f'{k} {what}')


# ---------------------------------------------------------------------------------------------------------------- the device call
def bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def device_update(unit, mean, act, ret, inv_t, in_place=False, null=()):
  """the probe's launcher on device copies -> dict(plan, ret0, best_ret, best_k) without the outputs named in `null`.  Every output is sentinel-filled, a guard row
  stands after the plan; the guard row, the candidates, the returns and (out of place) the mean are asserted unchanged"""
  import torch
  lib = load(unit.name)
  K, H, n, dim = act.shape
  assert mean.shape == (H, n, dim) and ret.shape == (K, n) and act.dtype == F32 and ret.dtype == F64 and 1 <= K <= unit.max_k
  dev = lambda a: torch.from_numpy(np.array(a, order='C')).cuda()      # (a copy: the cached arrays are read-only)
  d_act, d_ret, d_mean = dev(act), dev(ret), dev(mean)
  buf = torch.full((H + 1, n, dim), PLAN_FILL, dtype=torch.float32, device='cuda')
  if in_place:
    buf[:H] = d_mean
    d_mean = buf
  outs = {'ret0': torch.full((n,), RET_FILL, dtype=torch.float64, device='cuda'), 'best_ret': torch.full((n,), RET_FILL, dtype=torch.float64, device='cuda'),
          'best_k': torch.full((n,), K_FILL, dtype=torch.int32, device='cuda')}
  ptr = lambda k: None if k in null else outs[k].data_ptr()
  cfg, pp = unit.cfg(n), unit.params(K, H, inv_t)
  assert d_act.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0 and d_mean.data_ptr() % 16 == 0
  rc = getattr(lib, unit.launcher)(C.byref(cfg), C.byref(pp), J, d_mean.data_ptr(), d_act.data_ptr(), d_ret.data_ptr(), buf.data_ptr(), ptr('ret0'), ptr('best_ret'),
                                   ptr('best_k'), torch.cuda.current_stream().cuda_stream)
  assert rc == _abi.EARL_OK, (unit.launcher, rc, _abi.load().earl_last_error())
  torch.cuda.synchronize()
  host = buf.cpu().numpy()
  assert (host[H] == F32(PLAN_FILL)).all(), 'the guard row after the plan was written'
  assert np.array_equal(bits(d_act.cpu().numpy()), bits(act)), 'the candidates were written'
  assert np.array_equal(bits(d_ret.cpu().numpy()), bits(ret)), 'the returns were written'
  if not in_place:
    assert np.array_equal(bits(d_mean.cpu().numpy()), bits(mean)), 'the mean was written'
  return {'plan': np.ascontiguousarray(host[:H]), **{k: v.cpu().numpy() for k, v in outs.items() if k not in null}}

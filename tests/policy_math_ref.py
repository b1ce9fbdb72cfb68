"""The build recipe, the loaders and the input tables of tests/policy_math_probe.hip: the scalar functions of csrc/policy_math.h one element per thread on the
device (two builds: the tabletop units' context, and under the stepper's file-scope `fp contract(fast)`), and the same file compiled for the host with the flags of
the existing host sweeps (bulk OpenMP fills: the expected values of tests/test_policy_math_gpu.py).  Shared with tests/test_policy_math.py (no GPU)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

from primitives_ref import HIPFLAGS, REPO, CSRC, makefile_hipflags     # the product's flags, spelled out there and held to csrc/Makefile (HIPFLAGS is re-asserted for this unit in test_policy_math.py)

SRC = os.path.join(REPO, 'tests', 'policy_math_probe.hip')
STEPPER_DEFINE = '-DEARL_PROBE_STEPPER_CONTEXT'
# the flags of the host sweeps of tests/test_policy_rollout.py / test_policy_gaussian.py
HOSTFLAGS = ['-O2', '-std=c++17', '-mavx2', '-mfma', '-ffp-contract=off', '-fno-fast-math', '-fopenmp', '-DEARL_HOST_BUILD']
BUILDS = ('plain', 'stepper')
CHUNK = 1 << 24


def so_path(build):
  return os.path.join(REPO, 'tests', {'plain': 'libpolicy_math_probe.so', 'stepper': 'libpolicy_math_probe_stepper.so', 'host': 'libpolicy_math_host.so'}[build])


def device_command(build, out):
  return ['hipcc', *HIPFLAGS, *([STEPPER_DEFINE] if build == 'stepper' else []), '-shared', '-o', out, SRC]


def host_command(out):
  return ['g++', *HOSTFLAGS, '-Wno-unknown-pragmas', '-fPIC', '-shared', '-x', 'c++', '-o', out, SRC]


def compile_unit(build, out=None):
  out = out or so_path(build)
  subprocess.check_call(host_command(out) if build == 'host' else device_command(build, out))
  return out


def build_if_stale(build):
  so = so_path(build)
  deps = [SRC] + glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(REPO, 'include', '*.h'))
  if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
    compile_unit(build)
  return so


def load_host():
  lib = C.CDLL(build_if_stale('host'))
  p, u, L, f, i = C.c_void_p, C.c_uint32, C.c_long, C.c_float, C.c_int
  for name in ('fill_tanh', 'fill_exp', 'fill_quantile'):
    getattr(lib, name).argtypes, getattr(lib, name).restype = [p, u, p, L], None
  lib.fill_head.argtypes, lib.fill_head.restype = [i, i, f, f, i, p, p, L], None
  lib.fill_muladd.argtypes, lib.fill_muladd.restype = [p, p, L], None
  assert lib.probe_is_host() == 1
  return lib


def load_device(build):
  lib = C.CDLL(build_if_stale(build))
  p, u, L, f, i = C.c_void_p, C.c_uint32, C.c_long, C.c_float, C.c_int
  for name in ('probe_tanh', 'probe_exp', 'probe_quantile'):
    getattr(lib, name).argtypes, getattr(lib, name).restype = [p, u, p, L, p], i
  lib.probe_head.argtypes, lib.probe_head.restype = [i, i, f, f, i, p, p, L, p], i
  lib.probe_muladd.argtypes, lib.probe_muladd.restype = [p, p, L, p], i
  assert lib.probe_is_host() == 0 and lib.probe_stepper_context() == int(build == 'stepper')
  return lib


# ---------------------------------------------------------------------------------------------------------------- the host side
def host_fill(host, fn, first=0, count=None, bits=None):
  """fill_<fn> over the bit patterns first .. first + count - 1, or over the uint32 array `bits` -> float32 array"""
  if bits is not None:
    bits = np.ascontiguousarray(bits, np.uint32)
    count = len(bits)
  out = np.empty(count, np.float32)
  getattr(host, 'fill_' + fn)(None if bits is None else bits.ctypes.data, first, out.ctypes.data, count)
  return out


def host_head(host, mode, log_std_map, lo, hi, out_act, rows):
  rows = np.ascontiguousarray(rows, np.float32)
  out = np.empty(len(rows), np.float32)
  host.fill_head(mode, log_std_map, lo, hi, out_act, rows.ctypes.data, out.ctypes.data, len(rows))
  return out


# ---------------------------------------------------------------------------------------------------------------- the input tables
def f32_bits(x):
  return int(np.array(x, np.float32).view(np.uint32))


def both_signs(bits):
  bits = np.asarray(bits, np.uint32)
  return np.concatenate([bits, bits | np.uint32(0x80000000)])


def log_spaced(a, b, count=1_000_000):
  """`count` bit patterns from a to b (bit patterns of positive floats are log-spaced), both ends included"""
  k = np.arange(count, dtype=np.uint64)
  return (np.uint64(a) + (np.uint64(b - a) * k) // np.uint64(count - 1)).astype(np.uint32)


def neighbours(x, width=2):
  """the float32 x and its `width` neighbours on each side, as bit patterns (x != 0)"""
  b = f32_bits(x)
  return np.array([b + d for d in range(-width, width + 1)], np.uint32)


P2M12, SIXTEEN, FLT_MAX, INF = f32_bits(2.0 ** -12), f32_bits(16.0), 0x7f7fffff, 0x7f800000
NANS = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0xff812345, 0x7fa00000], np.uint32)

# (function, name) -> (first bit pattern, count): the contiguous ranges, every float32 of them
RANGES = {
    ('tanh', 'positive'): (P2M12, SIXTEEN - P2M12 + 1),                                   # 2^-12 <= x <= 16
    ('tanh', 'negative'): (P2M12 | 0x80000000, SIXTEEN - P2M12 + 1),
    ('exp', 'negative'): (P2M12 | 0x80000000, f32_bits(20.0) - P2M12 + 1),                # [-20, -2^-12]
    ('exp', 'positive'): (P2M12, f32_bits(4.0) - P2M12 + 1),                              # [2^-12, 4]
    ('quantile', 'all'): (0, 1 << 24),
}


def tanh_points():
  """the log-spaced samples outside the swept range and the special values: (bit patterns, the index from which the entries are NaN)"""
  parts = [both_signs(log_spaced(1, P2M12)), both_signs(log_spaced(SIXTEEN, FLT_MAX)), both_signs([0, INF, 0x007fffff, 1]),
           both_signs(neighbours(2.0 ** -6)), both_signs(neighbours(10.0))]
  finite = np.concatenate(parts)
  return np.concatenate([finite, NANS]), len(finite)


def exp_points():
  parts = [both_signs(log_spaced(1, P2M12)), both_signs([0]), neighbours(89.0), neighbours(-104.0), neighbours(4.0), neighbours(-20.0), both_signs([INF])]
  finite = np.concatenate(parts)
  return np.concatenate([finite, NANS]), len(finite)


HEAD_BOUNDS = ((-5.0, 2.0), (-20.0, 4.0), (1.5, 1.5))          # the usual bounds, the extremes the entry points accept, lo == hi
HEAD_COMBOS = [(mode, lmap, oact, b) for mode in (0, 1) for lmap in (0, 1) for oact in (0, 2) for b in range(len(HEAD_BOUNDS))]     # EARL_ACT_NONE = 0, EARL_ACT_TANH = 2


def head_rows(host, lmap, bounds, seed, count=1 << 20):
  """[count, 3] float32 rows (mean, raw, eps): means of a few units and some large; raw across and well beyond the bounds and around 0, some exactly at the bounds, and NaN in the
  clamp map (which defines NaN -> lo; the tanh map would carry a NaN payload, which is compared nowhere); eps from the quantile table"""
  rng = np.random.default_rng(seed)
  lo, hi = bounds
  mean = (rng.standard_normal(count) * np.where(rng.random(count) < 0.1, 30.0, 1.5)).astype(np.float32)
  raw = np.where(rng.random(count) < 0.5, rng.uniform(lo - 12.0, hi + 12.0, count), rng.uniform(-3.0, 3.0, count)).astype(np.float32)     # (half of them where tanh_f32 is not saturated)
  sel = rng.random(count)
  raw[sel < 0.02] = np.float32(lo)
  raw[(sel >= 0.02) & (sel < 0.04)] = np.float32(hi)
  raw[(sel >= 0.04) & (sel < 0.08)] *= np.float32(1e-3)                                  # the tanh map's small-argument branch
  if lmap == 0:
    raw[(sel >= 0.08) & (sel < 0.10)] = np.float32('nan')
  k = rng.integers(0, 1 << 24, count, dtype=np.uint32)
  k[:4] = (0, (1 << 24) - 1, 1 << 23, (1 << 23) - 1)                                     # both tails and the two innermost
  eps = host_fill(host, 'quantile', bits=k)
  return np.stack([mean, raw, eps], axis=1)

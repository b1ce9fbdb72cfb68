"""The scalar functions of csrc/policy_math.h swept on the MI355X: tanh_f32, exp_f32, normal_quantile_f32 and gaussian_head_action, one element per thread
(tests/policy_math_probe.hip), in BOTH contexts the product compiles them in -- the tabletop units' (-ffp-contract=off) and the stepper units' (a file-scope
`#pragma clang fp contract(fast)` before the header, where only the functions' own in-body contract(off) pragmas keep them exact) -- against the host statement of
the same header filled in bulk with the flags of the existing host sweeps.  The host header is held to tanh / exp / ndtri in double by tests/test_policy_rollout.py
and tests/test_policy_gaussian.py; this file is the missing link, device == host, so there is no tolerance: equality of bit patterns (NaN-ness for NaN inputs).
What each test sweeps, per build:
  tanh_f32     134 217 729 float32 per sign (every float32 with 2^-12 <= |x| <= 16), 4 000 028 log-spaced and special points outside, 6 NaN payloads
  exp_f32      136 314 881 (every float32 of [-20, -2^-12]) + 117 440 513 (every float32 of [2^-12, 4]), 2 000 024 points outside, 6 NaN payloads
  quantile     all 16 777 216 inputs, and the device array exactly odd in k <-> 2^24 - 1 - k
  head         2^20 rows for each of 24 combinations of mode x log_std_map x out_act x bounds
Observed (one MI355X, 16 host threads): no difference in either build on any sweep; 0.6 s for the largest (tanh_f32, one sign, both builds), 5.5 s for the file.
tests/test_policy_math.py (no GPU) holds the build recipe and the host helper."""
import numpy as np
import pytest
import torch

import policy_math_ref as R

pytestmark = pytest.mark.gpu
GPU = 'cuda:0'


@pytest.fixture(scope='module')
def host():
  return R.load_host()


@pytest.fixture(scope='module')
def devs():
  return {b: R.load_device(b) for b in R.BUILDS}


def device_fill(lib, fn, first=0, count=None, bits=None):
  d_in = None if bits is None else torch.from_numpy(np.ascontiguousarray(bits, np.uint32).view(np.int32)).to(GPU)
  count = count if bits is None else len(bits)
  out = torch.empty(count, dtype=torch.float32, device=GPU)
  rc = getattr(lib, 'probe_' + fn)(None if d_in is None else d_in.data_ptr(), first, out.data_ptr(), count, torch.cuda.current_stream().cuda_stream)
  assert rc == 0, f'probe_{fn} refused the launch'
  return out.cpu().numpy()


def assert_bits(got, want, build, what, arg_of):
  """equality of bit patterns; on failure: the first differing input, both outputs, the build and the count"""
  g, w = got.view(np.uint32), want.view(np.uint32)
  if not np.array_equal(g, w):
    bad = np.flatnonzero(g != w)
    i = int(bad[0])
    raise AssertionError(f'{what}, {build} build: {len(bad)} of {len(g)} values differ; first at {arg_of(i)}: device {got[i]!r} (0x{int(g[i]):08x}) host {want[i]!r} (0x{int(w[i]):08x})')


def f32_of(b):
  return float(np.array(b, np.uint32).view(np.float32))


def sweep_range(host, devs, fn, name):
  first, count = R.RANGES[(fn, name)]
  done = 0
  while done < count:                                                          # chunks of 2^24: one host array, both device builds against it
    m = min(R.CHUNK, count - done)
    f = (first + done) & 0xffffffff
    want = R.host_fill(host, fn, first=f, count=m)
    for build in R.BUILDS:
      got = device_fill(devs[build], fn, first=f, count=m)
      assert_bits(got, want, build, f'{fn} {name}', lambda i: f'input 0x{f + i:08x}' + (f' ({f32_of(f + i)!r})' if fn != 'quantile' else ''))
    done += m
  return count


def sweep_points(host, devs, fn, points, n_finite):
  want = R.host_fill(host, fn, bits=points)
  assert not np.isnan(want[:n_finite]).any() and np.isnan(want[n_finite:]).all()
  for build in R.BUILDS:
    got = device_fill(devs[build], fn, bits=points)
    assert_bits(got[:n_finite], want[:n_finite], build, f'{fn} points', lambda i: f'input 0x{int(points[i]):08x} ({f32_of(points[i])!r})')
    assert np.isnan(got[n_finite:]).all(), (build, got[n_finite:])             # NaN in, NaN out (the payload is not part of the contract)


# ---------------------------------------------------------------------------------------------------------------- the two contexts are two
def test_the_stepper_context_build_contracts_and_the_plain_build_does_not(host, devs):
  """a * b + c written in the probe unit itself (no pragma of its own): the plain build rounds the product (= the host, -ffp-contract=off), the stepper-context
  build fuses it -- so the sweeps below run policy_math.h where only its in-body contract(off) pragmas keep it exact.  a, b in [1, 2), c in [1, 4): the exact
  a b + c has at most 50 significant bits, so float64 holds it and one rounding to float32 is the fused result"""
  rng = np.random.default_rng(5)
  rows = np.stack([rng.uniform(1, 2, 1 << 16), rng.uniform(1, 2, 1 << 16), rng.uniform(1, 4, 1 << 16)], axis=1).astype(np.float32)
  separate = np.empty(len(rows), np.float32)
  host.fill_muladd(rows.ctypes.data, separate.ctypes.data, len(rows))
  np.testing.assert_array_equal(separate, (rows[:, 0] * rows[:, 1]) + rows[:, 2])
  r64 = rows.astype(np.float64)
  fused = (r64[:, 0] * r64[:, 1] + r64[:, 2]).astype(np.float32)
  assert (fused != separate).mean() > 0.1
  d_rows = torch.from_numpy(rows).to(GPU)
  for build, want in (('plain', separate), ('stepper', fused)):
    out = torch.empty(len(rows), dtype=torch.float32, device=GPU)
    assert devs[build].probe_muladd(d_rows.data_ptr(), out.data_ptr(), len(rows), torch.cuda.current_stream().cuda_stream) == 0
    assert_bits(out.cpu().numpy(), want, build, 'a * b + c outside the header', lambda i: f'row {i} = {tuple(rows[i].tolist())}')


# ---------------------------------------------------------------------------------------------------------------- tanh_f32
@pytest.mark.parametrize('sign', ['positive', 'negative'])
def test_tanh_f32_every_float32_of_the_swept_range(host, devs, sign):
  """134 217 729 values per sign and per build"""
  assert sweep_range(host, devs, 'tanh', sign) == 0x41800000 - 0x39800000 + 1


def test_tanh_f32_outside_the_swept_range_and_at_its_branch_edges(host, devs):
  """10^6 log-spaced bit patterns from the smallest subnormal to 2^-12 and 10^6 from 16 to FLT_MAX, both signs, both ends; +-0, +-Inf, the largest and the smallest
  subnormal, +-2^-6 and +-10 with two neighbours on each side; six NaN payloads"""
  points, n_finite = R.tanh_points()
  assert n_finite == 4_000_028 and {1, 0x39800000, 0x41800000, 0x7f7fffff, 0x80000001, 0xff7fffff, 0x3c800000 - 1, 0x41200000 + 2} <= set(points.tolist())
  sweep_points(host, devs, 'tanh', points, n_finite)
  for build in R.BUILDS:                                                       # the special values themselves, not only "what the host says"
    got = device_fill(devs[build], 'tanh', bits=[0, 0x80000000, 0x7f800000, 0xff800000, 1, 0x7f7fffff]).view(np.uint32)
    assert got.tolist() == [0, 0x80000000, 0x3f800000, 0xbf800000, 1, 0x3f800000], (build, got)


# ---------------------------------------------------------------------------------------------------------------- exp_f32
@pytest.mark.parametrize('sign', ['negative', 'positive'])
def test_exp_f32_every_float32_of_the_log_std_range(host, devs, sign):
  """136 314 881 values of [-20, -2^-12], 117 440 513 of [2^-12, 4], per build"""
  assert sweep_range(host, devs, 'exp', sign) == {'negative': 0x41a00000, 'positive': 0x40800000}[sign] - 0x39800000 + 1


def test_exp_f32_below_the_swept_range_and_at_its_branch_edges(host, devs):
  """10^6 log-spaced bit patterns of each sign below 2^-12 (subnormals included), +-0, the neighbours of 89, -104, 4 and -20, +-Inf; six NaN payloads"""
  points, n_finite = R.exp_points()
  assert n_finite == 2_000_024
  sweep_points(host, devs, 'exp', points, n_finite)
  for build in R.BUILDS:
    got = device_fill(devs[build], 'exp', bits=[0, 0x80000000, 0x7f800000, 0xff800000, R.f32_bits(89.0), R.f32_bits(-104.0)]).view(np.uint32)
    assert got.tolist() == [0x3f800000, 0x3f800000, 0x7f800000, 0, 0x7f800000, 0], (build, got)


# ---------------------------------------------------------------------------------------------------------------- normal_quantile_f32
def test_normal_quantile_f32_all_inputs_and_exactly_odd(host, devs):
  """all 2^24 inputs per build; the device array is odd in k <-> 2^24 - 1 - k as bit patterns"""
  assert sweep_range(host, devs, 'quantile', 'all') == 1 << 24
  for build in R.BUILDS:
    got = device_fill(devs[build], 'quantile', first=0, count=1 << 24).view(np.uint32)
    assert np.array_equal(got, got[::-1] ^ np.uint32(0x80000000)), build


# ---------------------------------------------------------------------------------------------------------------- gaussian_head_action
@pytest.mark.parametrize('mode,lmap,oact,b', R.HEAD_COMBOS, ids=[f'{("mean", "sample")[m]}-{("clamp", "tanh")[l]}-{("none", "", "tanh")[o]}-{R.HEAD_BOUNDS[b]}' for m, l, o, b in R.HEAD_COMBOS])
def test_gaussian_head_action_rows(host, devs, mode, lmap, oact, b):
  """2^20 rows per combination and per build: raw across and beyond the bounds and exactly at them, NaN raw in the clamp map, eps from the quantile table"""
  lo, hi = R.HEAD_BOUNDS[b]
  rows = R.head_rows(host, lmap, (lo, hi), seed=17 * b + 4 * mode + 2 * lmap + oact)
  want = R.host_head(host, mode, lmap, lo, hi, oact, rows)
  assert not np.isnan(want).any()
  if mode == 1:
    mean_only = R.host_head(host, 0, lmap, lo, hi, oact, rows)
    assert (want != mean_only).mean() > 0.25                                             # a condition on the inputs (host alone): the noise is in the actions of at least a quarter of the rows
  d_rows = torch.from_numpy(rows).to(GPU)
  for build in R.BUILDS:
    out = torch.empty(len(rows), dtype=torch.float32, device=GPU)
    assert devs[build].probe_head(mode, lmap, lo, hi, oact, d_rows.data_ptr(), out.data_ptr(), len(rows), torch.cuda.current_stream().cuda_stream) == 0
    assert_bits(out.cpu().numpy(), want, build, f'head mode={mode} map={lmap} out_act={oact} bounds=({lo}, {hi})',
                lambda i: f'row {i} (mean, raw, eps) = {tuple(rows[i].tolist())}')

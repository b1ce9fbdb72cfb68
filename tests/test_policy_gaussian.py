"""earl_tabletop_policy_rollout_gaussian (include/earl_tabletop.h): the closed-loop tabletop rollout with a Gaussian-head MLP sampled inside the launch.
Without a GPU, through csrc/libearl_host.so (the kernel's own header, csrc/tabletop_policy.h, compiled for the host):
  1. the draws are the specified ones (numpy Philox4x32-10 + the 24-bit uniform + the double quantile), whatever n, the shard split, E or the mode;
  2. normal_quantile_f32 over all 2^24 inputs and exp_f32 over every float32 of [-20, 4], in ulp against double references;
  3. the distribution of the recorded draws (moments, correlations, Kolmogorov-Smirnov);
  4. closed = open, bit for bit, and the oracle stepped with the recorded actions;
  5. MEAN mode == earl_tabletop_policy_rollout on the 3-output twin, bit for bit;
  6. the actions are the contract's: a-priori bound against float64, and one small case exactly in fractions.Fraction;
  7. ABI edges from both libraries, struct layout against gcc;
  8. no scratch in any instantiation of the new unit, the one-hidden-layer ones at two waves per SIMD;
  9. the Python surface on the host.
tests/test_policy_gaussian_gpu.py holds the device to the host bit for bit."""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import hip_harness as hx
import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import (EXP_ULP_BOUND, QUANTILE_ULP_BOUND, GaussPolicy, Packed, expected_eps, gaussian_closed_equals_open, gaussian_rollout,
                                     head_struct, ndtri64, ulp32)
from oracle import tabletop_oracle as orc
from test_policy_rollout import (CSRC, TANH_ULP_BOUND, U, Policy, assert_same_bits, assert_same_state, consumed_observations, f64_policy_with_bound,
                                 final_state, policy_rollout, round_f32)

CPU = 'cpu'
SEEDS = (5, 21, 2024)
HOSTCC = ['g++', '-O2', '-std=c++17', '-mavx2', '-mfma', '-ffp-contract=off', '-fno-fast-math', '-fopenmp', '-DEARL_HOST_BUILD', '-I', CSRC]


# ---------------------------------------------------------------------------------------------------------------- 1. the draws
@functools.lru_cache(maxsize=None)
def recorded(seed):
  """eps_out of the host twin: n = 4096, env_offset = 3, T = 200, E = 2, cfg.counter starting at 0"""
  h = hx.HipTabletop(4096, device=CPU, seed=seed, env_offset=3, horizon=200)
  return gaussian_rollout(h, GaussPolicy((16,), seed=1), 2, 200, True)['eps']


@pytest.mark.parametrize('seed', SEEDS)
def test_draws_are_the_specified_ones(seed):
  got = recorded(seed)
  want = expected_eps(seed, 3, 4096, 2, 200)
  err = np.abs(got.astype(np.float64) - want) / ulp32(want)
  print(f'seed {seed}: max error {err.max():.3f} ulp, max |eps| {np.abs(got).max()!r}')
  assert np.isfinite(got).all() and err.max() <= QUANTILE_ULP_BOUND
  if seed == 2024:
    assert np.abs(got).max() > 5.41                                                    # (this seed contains the extreme value)


def test_draws_depend_on_seed_global_env_and_counter_only():
  seed, T = 21, 200
  full = recorded(seed)
  pol = GaussPolicy((16,), seed=1)

  def run(n, off, E, counter0=0, pol=pol, **kw):
    h = hx.HipTabletop(n, device=CPU, seed=seed, env_offset=off, horizon=T)
    h.cfg.counter = counter0
    return gaussian_rollout(h, pol, E, T, True, **kw)['eps']

  np.testing.assert_array_equal(run(100, 3, 1).view(np.uint32), full[:1, :, :100].view(np.uint32))                      # n, E
  np.testing.assert_array_equal(run(40, 63, 2).view(np.uint32), full[:, :, 60:100].view(np.uint32))                     # the shard split
  np.testing.assert_array_equal(run(100, 3, 1, mode='mean').view(np.uint32), full[:1, :, :100].view(np.uint32))         # mode
  np.testing.assert_array_equal(run(64, 3, 1, counter0=T + 1).view(np.uint32), full[1:, :, :64].view(np.uint32))        # episode 1 = the counter
  other = run(64, 3, 1, pol=GaussPolicy((48, 32), 'tanh', 'none', seed=9), log_std_map='clamp')                          # ... and not on the policy
  np.testing.assert_array_equal(other.view(np.uint32), full[:1, :, :64].view(np.uint32))
  # the continuing form: counters cfg.counter + t
  h = hx.HipTabletop(50, device=CPU, seed=seed, env_offset=3, horizon=T)
  h.reset()
  got = gaussian_rollout(h, pol, 1, 30, False)['eps']
  want = expected_eps(seed, 3, 50, 1, 30, reset_first=False, counter0=1)[0]
  assert (np.abs(got - want) / ulp32(want)).max() <= QUANTILE_ULP_BOUND


# ---------------------------------------------------------------------------------------------------------------- 2. the quantile and exp, exhaustively
SWEEP = r'''
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "tabletop_policy.h"
using earl::exp_f32;
using earl::normal_quantile_f32;
static float f(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }
static uint32_t u(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<float> q(1u << 24);
#pragma omp parallel for schedule(static)
  for (long long k = 0; k < (1ll << 24); ++k) q[(size_t)k] = normal_quantile_f32((uint32_t)k);
  FILE* fp = fopen(argv[1], "wb");
  if (!fp || fwrite(q.data(), 4, q.size(), fp) != q.size()) return 3;
  fclose(fp);
  // exp_f32 over every float32 of [-20, 4]: bit patterns 0 .. 4.0f and -0 .. -20.0f
  double worst = 0; uint32_t worst_at = 0; long long count = 0, bad = 0;
  for (int part = 0; part < 2; ++part) {
    const uint32_t lo = part ? 0x80000000u : 0u, hi = part ? u(-20.0f) : u(4.0f);
#pragma omp parallel
    {
      double w = 0; uint32_t at = 0; long long c = 0, b = 0;
#pragma omp for schedule(static, 1 << 18) nowait
      for (long long k = lo; k <= (long long)hi; ++k) {
        const float x = f((uint32_t)k), y = exp_f32(x);
        const double ref = std::exp((double)x);
        int e; std::frexp(ref, &e);
        const double er = std::fabs((double)y - ref) / std::ldexp(1.0, e - 1 - 23);
        if (!(y > 0.0f) || !std::isfinite(y)) ++b;
        if (er > w) { w = er; at = (uint32_t)k; }
        ++c;
      }
#pragma omp critical
      { count += c; bad += b; if (w > worst) { worst = w; worst_at = at; } }
    }
  }
  printf("exp_count %lld bad %lld\n", count, bad);
  printf("exp_worst_ulp %.9f at %a\n", worst, (double)f(worst_at));
  printf("exp_special %08x %08x %08x %08x %d\n", u(exp_f32(0.0f)), u(exp_f32(-0.0f)), u(exp_f32(INFINITY)), u(exp_f32(-INFINITY)), (int)std::isnan(exp_f32(NAN)));
  return 0;
}
'''


def test_quantile_over_all_inputs_and_exp_over_every_float32_of_its_range(tmp_path):
  src, exe, qbin = tmp_path / 'gauss_sweep.cpp', tmp_path / 'gauss_sweep', tmp_path / 'q.bin'
  src.write_text(SWEEP)
  subprocess.run(HOSTCC + ['-o', str(exe), str(src)], check=True)
  out = subprocess.run([str(exe), str(qbin)], check=True, capture_output=True, text=True, timeout=3000).stdout
  print(out)
  q = np.fromfile(qbin, np.float32)
  assert q.size == 1 << 24 and np.isfinite(q).all()
  assert np.array_equal(q.view(np.uint32), q[::-1].view(np.uint32) ^ np.uint32(0x80000000))                 # exactly odd: eps(k) == -eps(2^24 - 1 - k)
  k = np.arange(1 << 24, dtype=np.float64)
  ref = ndtri64((k + 0.5) * 2.0 ** -24)
  err = np.abs(q.astype(np.float64) - ref)
  ulps = err / ulp32(ref)
  central = np.abs(2 * k + 1 - 2 ** 24) * 2.0 ** -25 <= 0.425
  print(f'quantile: max {ulps.max():.4f} ulp at k = {ulps.argmax()} (central {ulps[central].max():.4f}, tails {ulps[~central].max():.4f}, 99.9 % below '
        f'{np.quantile(ulps, 0.999):.4f}); largest value {np.abs(q).max()!r}; adjacent pairs out of order {int((np.diff(q) < 0).sum())}; '
        f'max absolute error for |eps| < 2^-6: {err[np.abs(ref) < 2.0 ** -6].max():.3e}')
  assert ulps.max() <= QUANTILE_ULP_BOUND <= 8.0                                                            # measured 4.934 (central 4.728)
  assert abs(float(np.abs(q).max()) - 5.41998) < 1e-5 and abs(float(q[-1]) - ref[-1]) <= QUANTILE_ULP_BOUND * ulp32(ref[-1]) and q[-1] == np.abs(q).max()
  ln = dict(line.split(' ', 1) for line in out.strip().splitlines())
  count, _, bad = ln['exp_count'].split()
  assert int(count) == (0x40800000 + 1) + (0xC1A00000 - 0x80000000 + 1) and bad == '0'                      # every float32 of [-20, 4], both zeros
  assert float(ln['exp_worst_ulp'].split()[0]) <= EXP_ULP_BOUND                                             # measured 0.5000000 (one rounding of a 1e-15-accurate value)
  assert ln['exp_special'] == '3f800000 3f800000 7f800000 00000000 1'


# ---------------------------------------------------------------------------------------------------------------- 3. the distribution
@pytest.mark.parametrize('seed', SEEDS)
def test_recorded_draws_are_standard_normal_and_uncorrelated(seed):
  x = recorded(seed).astype(np.float64)                                 # [E = 2, T, n, 3]
  N = x.size
  assert N == 4915200
  z = {'mean': x.mean() * np.sqrt(N), 'var': (x.var() - 1) / np.sqrt(2 / N), 'm4': ((x ** 4).mean() - 3) / np.sqrt(96 / N)}

  def corr(a, b):
    return float(np.corrcoef(a.ravel(), b.ravel())[0, 1]) * np.sqrt(a.size)

  for a, b in ((0, 1), (0, 2), (1, 2)):
    z[f'dim{a}{b}'] = corr(x[..., a], x[..., b])
  z['lag_t'], z['lag_env'], z['episodes'] = corr(x[:, :-1], x[:, 1:]), corr(x[:, :, :-1], x[:, :, 1:]), corr(x[0], x[1])
  s = np.sort(x.ravel())
  cdf = torch.special.ndtr(torch.from_numpy(s)).numpy()
  i = np.arange(1, N + 1, dtype=np.float64)
  ks = max(float((i / N - cdf).max()), float((cdf - (i - 1) / N).max())) * np.sqrt(N)
  print(f'seed {seed}: ' + ', '.join(f'{k} {v:+.2f}' for k, v in z.items()) + f', KS D sqrt(N) {ks:.3f}')
  assert all(abs(v) <= 4.5 for v in z.values()), z
  assert ks <= 1.95


# ---------------------------------------------------------------------------------------------------------------- 4. closed = open
def fresh(n, reset_first, **kw):
  h = hx.HipTabletop(n, device=CPU, seed=5, env_offset=2, **kw)
  h.reset()
  if not reset_first:
    h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, n, 3)).astype(np.float32))
  return h


@pytest.mark.parametrize('T', [200, 37])
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('wide', [False, True])
def test_closed_equals_open_evaluation_form(T, rt, wide):
  pol = GaussPolicy((64,), seed=T)
  got, _ = gaussian_closed_equals_open(fresh(70, True, reward_type=rt, wide_init=wide, horizon=T), pol, 3, T, True)
  a = np.abs(got['act'])
  assert (a > 0.99).any() and (a < 0.5).any()


@pytest.mark.parametrize('kw', [dict(goal_change_frequency=50, horizon=10**6), dict(auto_reset=True, horizon=13), dict(goal_change_frequency=50, auto_reset=True, horizon=31, wide_init=True)],
                         ids=['lifelong', 'auto_reset', 'both'])
def test_closed_equals_open_continuing_form(kw):
  pol = GaussPolicy((48, 32), hidden_act='tanh', out_act='none', seed=3)
  got, _ = gaussian_closed_equals_open(fresh(70, False, reward_type='dense', **kw), pol, 1, 200, False, log_std_map='clamp')
  if kw.get('auto_reset'):
    assert got['done'].any()


@pytest.mark.parametrize('wide', [False, True])
def test_oracle_stepped_with_the_recorded_actions_reproduces_the_closed_loop(wide):
  n, E, T = 50, 3, 40
  kw = dict(reward_type='sparse', wide_init=wide, horizon=T, seed=9, env_offset=1)
  h, o = hx.HipTabletop(n, device=CPU, **kw), orc.OracleTabletop(n, **kw)
  got = gaussian_rollout(h, GaussPolicy((32,), seed=11), E, T, True)
  for e in range(E):
    o.reset()
    obs, rew, done, succ = o.rollout(np.ascontiguousarray(got['act'][e]))
    np.testing.assert_array_equal(got['obs'][e].view(np.uint32), obs.view(np.uint32))
    np.testing.assert_array_equal(got['reward'][e], rew)
    np.testing.assert_array_equal(got['done'][e], done)
    np.testing.assert_array_equal(got['success'][e], succ)
  np.testing.assert_array_equal(h.host('qpos'), o.qpos)
  assert h.cfg.counter == o.cfg.counter


# ---------------------------------------------------------------------------------------------------------------- 5. MEAN mode
@pytest.mark.parametrize('oact', ['tanh', 'none'])
@pytest.mark.parametrize('hidden', [(16,), (64,), (48, 32), (256, 256)], ids=str)
def test_mean_mode_is_the_existing_entry_point_on_the_three_output_twin(hidden, oact):
  n, E, T = 40, 2, 30
  kw = dict(reward_type='dense', horizon=T, seed=4, env_offset=1)
  pol = GaussPolicy(hidden, 'relu' if len(hidden) == 1 else 'tanh', oact, seed=hidden[0])
  a, b = hx.HipTabletop(n, device=CPU, **kw), hx.HipTabletop(n, device=CPU, **kw)
  got = gaussian_rollout(a, pol, E, T, True, mode='mean')
  want = policy_rollout(b, pol.mean_twin(), E, T, True)
  assert_same_bits(got, want, ('obs', 'reward', 'done', 'success', 'act'))
  assert_same_state(final_state(a), final_state(b))


# ---------------------------------------------------------------------------------------------------------------- 6. the actions are the contract's
def f64_head_with_bound(pol, x, eps, log_std_map, bounds):
  """float64 evaluation of the contract from the recorded float32 eps, and the a-priori bound on what the float32 evaluation can differ from it.  The network's
  six outputs and their bounds are test_policy_rollout.f64_policy_with_bound's (no activation on the last layer).  Then, with u = 2^-24 per float32 operation:
    clamp   1-Lipschitz: e_ls = e_raw
    tanh    t = tanh_f32(raw): e_t = e_raw + its asserted ulp bound; ls = lo + h (t + 1) with h = 0.5 (hi - lo): four roundings (hi - lo, t + 1, the product, the sum), each
            of a value of magnitude <= |lo| + h (|t| + 1 + e_t): e_ls = h e_t + 4 u' (|lo| + h (|t| + 1 + e_t)), u' = u / (1 - 4 u)
    sigma   exp is e^x-Lipschitz: e_sigma = sigma (exp(e_ls) - 1) + EXP_ULP_BOUND ulp of a value <= sigma exp(e_ls)
    fmaf    e_u = e_mean + |eps| e_sigma + u (|mean + sigma eps| + e_mean + |eps| e_sigma)
    out_act tanh is 1-Lipschitz, plus tanh_f32's asserted bound"""
  net = Packed(pol.layers, pol.hidden_act, 'none')
  y, e = f64_policy_with_bound(net, x)
  mean, raw, e_mean, e_raw = y[..., :3], y[..., 3:], e[..., :3], e[..., 3:]
  lo, hi = (float(np.float32(b)) for b in bounds)
  if log_std_map == 'clamp':
    ls, e_ls = np.clip(raw, lo, hi), e_raw
  else:
    t = np.tanh(raw)
    e_t = e_raw + TANH_ULP_BOUND * 2.0 ** -23 * (np.abs(t) + e_raw) + 2.0 ** -149
    h = 0.5 * (hi - lo)
    ls = lo + h * (t + 1)
    e_ls = h * e_t + 4 * U / (1 - 4 * U) * (abs(lo) + h * (np.abs(t) + 1 + e_t))
  sigma = np.exp(ls)
  e_sigma = sigma * np.expm1(e_ls) + EXP_ULP_BOUND * 2.0 ** -23 * sigma * np.exp(e_ls)
  eps = eps.astype(np.float64)
  u = mean + sigma * eps
  e_u = e_mean + np.abs(eps) * e_sigma
  e_u = e_u + U * (np.abs(u) + e_u) + 2.0 ** -149
  if pol.out_act == 'tanh':
    u = np.tanh(u)
    e_u = e_u + TANH_ULP_BOUND * 2.0 ** -23 * (np.abs(u) + e_u) + 2.0 ** -149
  return u, e_u, ls


@pytest.mark.parametrize('hidden,hact,oact,lmap', [((64,), 'relu', 'tanh', 'tanh'), ((48, 32), 'tanh', 'none', 'clamp'), ((256, 256), 'relu', 'tanh', 'clamp'),
                                                   ((16,), 'relu', 'none', 'tanh')])
def test_actions_are_the_contract_within_the_a_priori_bound(hidden, hact, oact, lmap):
  n, E, T = 40, 2, 25
  kw = dict(reward_type='sparse', horizon=T, seed=4)
  pol = GaussPolicy(hidden, hact, oact, seed=2)
  got = gaussian_rollout(hx.HipTabletop(n, device=CPU, **kw), pol, E, T, True, log_std_map=lmap)
  x = consumed_observations(kw, n, E, T, got)
  want, bound, ls = f64_head_with_bound(pol, x, got['eps'], lmap, (-5.0, 2.0))
  err = np.abs(got['act'].astype(np.float64) - want)
  print(f'{hidden} {hact}/{oact} {lmap}: max |error| {err.max():.3e}, max error / bound {np.max(err / bound):.3f}, bound <= {bound.max():.3e}, '
        f'log_std in [{ls.min():.3f}, {ls.max():.3f}]')
  assert (err <= bound).all()
  assert np.median(bound) < 1e-2                                               # the bound says something for the typical action (its tail: sigma up to e^2 = 7.4 times |eps| up to 5.4 amplifies the network's own worst case)
  if lmap == 'clamp':                                                          # both clamp ends and the interior occur
    assert (ls == -5.0).any() and (ls == 2.0).any() and ((ls > -5.0) & (ls < 2.0)).any()
  else:
    assert ls.min() < -4.9 and ls.max() > 1.9 and ((ls > -3) & (ls < 0)).any()
  # sigma eps changes which side of the env's clip some actions fall on
  mean_act = f64_head_with_bound(pol, x, np.zeros_like(got['eps']), lmap, (-5.0, 2.0))[0]
  if oact == 'none':
    assert ((np.abs(mean_act) < 1) & (np.abs(want) > 1)).any() and ((np.abs(mean_act) > 1) & (np.abs(want) < 1)).any()


def round_to(fr, bits, emin):
  """a Fraction rounded ONCE to the nearest binary floating-point number with `bits` significant bits and minimum exponent emin (ties to even)"""
  if fr == 0:
    return Fraction(0)
  a, e = abs(fr), 0
  while a >= 2:
    a /= 2; e += 1
  while a < 1:
    a *= 2; e -= 1
  q = Fraction(2) ** (max(e, emin) - (bits - 1))
  return (1 if fr > 0 else -1) * round(abs(fr) / q) * q


def r64(v):
  return round_to(v, 53, -1022)


def exp_core_in_fractions(y, half):
  """the fp64 exp shared by exp_f32 and tanh_f32 in csrc/tabletop_policy.h, operation by operation (fma / * / + with one rounding each): e^y, NOT yet rounded to float32"""
  k = int(r64(r64(y * Fraction(1.4426950408889634)) + half))                                               # (int) truncates toward zero
  s = r64(k * Fraction(-6.93147180369123816490e-01) + y)
  s = r64(k * Fraction(-1.90821492927058770002e-10) + s)
  fact = [1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0]
  p = Fraction(fact[0])
  for c in fact[1:]:
    p = r64(s * p + Fraction(c))
  return p, k


def exp_f32_in_fractions(x):
  """exp_f32: the fp64 exp, p 2^k rounded ONCE to float32"""
  p, k = exp_core_in_fractions(Fraction(x), Fraction(-1, 2) if x < 0 else Fraction(1, 2))
  return round_f32(p * Fraction(2) ** k)


def tanh_f32_in_fractions(x):
  """tanh_f32 of a finite float32, operation by operation in fp64, rounded ONCE to float32; the sign is copied"""
  a = abs(Fraction(x))
  if a >= 10:
    v = Fraction(1)
  elif a < Fraction(1, 64):
    z = r64(a * a)
    p = Fraction(62.0 / 2835.0)
    for c in (-17.0 / 315.0, 2.0 / 15.0, -1.0 / 3.0):
      p = r64(z * p + Fraction(c))
    v = r64(a * r64(z * p) + a)
  else:
    p, k = exp_core_in_fractions(-2 * a, Fraction(-1, 2))
    t = r64(p * Fraction(2) ** k)
    v = r64(r64(1 - t) / r64(1 + t))
  v = round_f32(v)
  return -v if x < 0 else v


def test_small_case_exactly_in_fractions():
  """out_act none and the clamp map: every operation of the contract after the recorded eps (the fmaf chains, the clamp, exp_f32, the head's fmaf) in exact
  rational arithmetic with the roundings the contract names"""
  n, T = 4, 3
  kw = dict(reward_type='sparse', horizon=T, seed=1, wide_init=True)
  pol = GaussPolicy((16,), 'relu', 'none', seed=8, log_std_gain=3.0)
  got = gaussian_rollout(hx.HipTabletop(n, device=CPU, **kw), pol, 1, T, True, log_std_map='clamp', bounds=(-1.5, 0.75))
  x = consumed_observations(kw, n, 1, T, got)
  seen = set()
  for t in range(T):
    for i in range(n):
      v = [Fraction(float(a)) for a in x[0, t, i]]
      for l, (w, b) in enumerate(pol.layers):
        nxt = []
        for j in range(w.shape[0]):
          acc = Fraction(float(b[j]))
          for k in range(w.shape[1]):
            acc = round_f32(v[k] * Fraction(float(w[j, k])) + acc)
          nxt.append(max(acc, Fraction(0)) if l == 0 else acc)
        v = nxt
      want = []
      for d in range(3):
        ls = min(max(v[3 + d], Fraction(-1.5)), Fraction(0.75))
        seen.add('lo' if ls == Fraction(-1.5) else 'hi' if ls == Fraction(0.75) else 'in')
        sigma = exp_f32_in_fractions(float(ls))
        want.append(float(round_f32(sigma * Fraction(float(got['eps'][0, t, i, d])) + v[d])))
      np.testing.assert_array_equal(got['act'][0, t, i].view(np.uint32), np.array(want, np.float32).view(np.uint32))
  assert seen == {'lo', 'hi', 'in'}


def test_small_case_exactly_in_fractions_with_the_tanh_map_and_the_squashing():
  """out_act tanh and the tanh log_std map: as the case above, with tanh_f32 evaluated in Fractions too (both of its branches below 10 and its saturation occur)"""
  n, T = 4, 3
  kw = dict(reward_type='sparse', horizon=T, seed=1, wide_init=True)
  pol = GaussPolicy((16,), 'relu', 'tanh', seed=8, log_std_gain=3.0)
  lo, hi = -5.0, 2.0
  got = gaussian_rollout(hx.HipTabletop(n, device=CPU, **kw), pol, 1, T, True, log_std_map='tanh', bounds=(lo, hi))
  x = consumed_observations(kw, n, 1, T, got)
  h = round_f32(Fraction(1, 2) * round_f32(Fraction(hi) - Fraction(lo)))
  branches = set()
  for t in range(T):
    for i in range(n):
      v = [Fraction(float(a)) for a in x[0, t, i]]
      for l, (w, b) in enumerate(pol.layers):
        nxt = []
        for j in range(w.shape[0]):
          acc = Fraction(float(b[j]))
          for k in range(w.shape[1]):
            acc = round_f32(v[k] * Fraction(float(w[j, k])) + acc)
          nxt.append(max(acc, Fraction(0)) if l == 0 else acc)
        v = nxt
      want = []
      for d in range(3):
        th = tanh_f32_in_fractions(float(v[3 + d]))
        ls = round_f32(Fraction(lo) + round_f32(h * round_f32(th + 1)))
        sigma = exp_f32_in_fractions(float(ls))
        u = round_f32(sigma * Fraction(float(got['eps'][0, t, i, d])) + v[d])
        for a in (abs(v[3 + d]), abs(u)):
          branches.add('series' if a < Fraction(1, 64) else 'exp' if a < 10 else 'one')
        want.append(float(tanh_f32_in_fractions(float(u))))
      np.testing.assert_array_equal(got['act'][0, t, i].view(np.uint32), np.array(want, np.float32).view(np.uint32))
  assert 'exp' in branches
  # tanh_f32's other two branches, against the compiled function through the head itself: a policy whose last layer is zero weights and chosen biases
  for raw, mean in ((0.01, 0.003), (-0.004, -12.5), (11.0, 0.5)):
    w, b = pol.layers[-1]
    flat = Packed(pol.layers[:-1] + [(np.zeros_like(w), np.array([mean] * 3 + [raw] * 3, np.float32))], 'relu', 'tanh')
    got = gaussian_rollout(hx.HipTabletop(2, device=CPU, **kw), flat, 1, 2, True, log_std_map='tanh', bounds=(lo, hi))
    th = tanh_f32_in_fractions(float(np.float32(raw)))
    sigma = exp_f32_in_fractions(float(round_f32(Fraction(lo) + round_f32(h * round_f32(th + 1)))))
    want = np.array([[float(tanh_f32_in_fractions(float(round_f32(sigma * Fraction(float(e)) + Fraction(float(np.float32(mean))))))) for e in row] for row in got['eps'].reshape(-1, 3)],
                    np.float32)
    np.testing.assert_array_equal(got['act'].reshape(-1, 3).view(np.uint32), want.view(np.uint32))


def test_the_stamped_profiling_build_links_every_unit_of_the_library():
  """tools/build_policy_stamped.sh rebuilds the policy units with stamps and links them with the shipped objects, whose list it takes from the Makefile
  (`make print-objects`): every unit of the Makefile's SRC must be on its link line, or tools/prof_policy.py's load of the stamped library fails on the first missing
  symbol.  The script runs here with the compiler replaced by `echo`: the lines it would run are read, nothing is built"""
  src = re.search(r'^SRC\s*=\s*(.*)$', open(os.path.join(CSRC, 'Makefile')).read(), flags=re.M).group(1).split()
  r = subprocess.run(['bash', os.path.join(REPO, 'tools', 'build_policy_stamped.sh')], env={**os.environ, 'HIPCC': 'echo'}, capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  script = r.stdout
  link = next(line for line in script.splitlines() if '-shared' in line)
  for unit in src:
    stem = unit[:-len('.hip')]
    assert (f' {stem}.o' in link) != (f'/{stem}_stamped.o' in link), unit                # (once: the shipped object or the stamped one)
  for unit in ('tabletop_policy', 'tabletop_policy_gaussian'):
    assert f'{unit}_stamped.o' in link and f'-o ../../tools/ubench/{unit}_stamped.o {unit}.hip' in script
  assert 'earl_debug_read_policy_gaussian_profile' in open(os.path.join(CSRC, 'tabletop_policy_gaussian.hip')).read()
  assert 'earl_debug_read_policy_gaussian_profile' in open(os.path.join(REPO, 'tools', 'prof_policy.py')).read()


# ---------------------------------------------------------------------------------------------------------------- 7. ABI edges
def _edge_calls(lib, host):
  h = hx.HipTabletop(8, device=CPU)
  st = h._state()
  arrs, out = h._outs((1, 4, 8))
  pol = GaussPolicy((16,))
  good = head_struct()

  def call(cfg=h.cfg, state=st, p=pol.struct, hd=good, E=1, T=4, rf=1, o=out):
    ref = lambda s: C.byref(s) if s is not None else None
    args = [ref(cfg), ref(state), ref(p), ref(hd), E, T, rf, ref(o), None]
    return lib.earl_tabletop_policy_rollout_gaussian_cpu(*args) if host else lib.earl_tabletop_policy_rollout_gaussian(*args, None)

  def variant(**kw):
    d = dict(n_layers=pol.struct.n_layers, dims=tuple(pol.struct.dims), hidden_act=pol.struct.hidden_act, out_act=pol.struct.out_act, precision=0,
             params=pol.struct.params)
    d.update(kw)
    d['dims'] = (C.c_int32 * 4)(*d['dims'])
    return _abi.MlpPolicy(**d)

  nan, inf = float('nan'), float('inf')
  bad = [dict(hd=None), dict(hd=head_struct(mode=2)), dict(hd=head_struct(mode=-1)), dict(hd=head_struct(log_std_map=2)), dict(hd=head_struct(bounds=(1.0, -1.0))),
         dict(hd=head_struct(bounds=(nan, 2.0))), dict(hd=head_struct(bounds=(-5.0, nan))), dict(hd=head_struct(bounds=(-inf, 2.0))), dict(hd=head_struct(bounds=(-5.0, inf))),
         dict(hd=head_struct(bounds=(-20.5, 2.0))), dict(hd=head_struct(bounds=(-5.0, 4.5))),
         dict(p=variant(dims=(12, 16, 3, 0))), dict(p=variant(dims=(12, 16, 7, 0))),
         # the existing entry point's whole list
         dict(cfg=None), dict(state=None), dict(p=None), dict(o=None), dict(p=variant(params=None)), dict(p=variant(precision=1)),
         dict(p=variant(n_layers=1)), dict(p=variant(n_layers=4)), dict(p=variant(dims=(13, 16, 6, 0))), dict(p=variant(dims=(12, 16, 4, 0))),
         dict(p=variant(dims=(12, 24, 6, 0))), dict(p=variant(dims=(12, 272, 6, 0))), dict(p=variant(dims=(12, 0, 6, 0))),
         dict(p=variant(n_layers=3, dims=(12, 16, 8, 6))), dict(p=variant(hidden_act=0)), dict(p=variant(hidden_act=3)), dict(p=variant(out_act=1)),
         dict(T=0), dict(T=-1), dict(E=0), dict(E=2, rf=0), dict(rf=2)]
  for kw in bad:
    assert call(**kw) == -1, kw
    assert (lib.earl_host_last_error if host else lib.earl_last_error)(), kw
  # the existing entry point still refuses a 6-wide output
  args = [C.byref(h.cfg), C.byref(st), C.byref(pol.struct), 1, 4, 1, C.byref(out), None]
  assert (lib.earl_tabletop_policy_rollout_cpu(*args) if host else lib.earl_tabletop_policy_rollout(*args, None)) == -1
  call.keep = (h, arrs, pol)
  return call


def test_argument_errors_from_the_host_library():
  lib = _abi.load_host()
  call = _edge_calls(lib._cdll, True)
  assert call() == 0                                                       # the good call runs (host pointers)
  assert call(hd=head_struct(bounds=(-20.0, 4.0))) == 0 and call(hd=head_struct(bounds=(0.5, 0.5), log_std_map='clamp', mode='mean')) == 0


def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  _edge_calls(lib, False)
  assert lib.earl_tabletop_policy_rollout_gaussian(None, None, None, None, 1, 1, 1, None, None, None) == -1
  assert b'NULL' in lib.earl_last_error()


def test_gaussian_head_layout_matches_what_gcc_sees(tmp_path):
  fields = [f[0] for f in _abi.GaussianHead._fields_]
  src = ('#include <stdio.h>\n#include <stddef.h>\n#include "earl_tabletop.h"\nint main(void) {\nprintf("%zu", sizeof(earl_gaussian_head));\n'
         + '\n'.join(f'printf(" %zu", offsetof(earl_gaussian_head, {f}));' for f in fields)
         + '\nprintf(" %d %d %d %d\\n", EARL_HEAD_MEAN, EARL_HEAD_SAMPLE, EARL_LOGSTD_CLAMP, EARL_LOGSTD_TANH);\nreturn 0; }\n')
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src)
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  tok = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
  assert tok[0] == C.sizeof(_abi.GaussianHead) == 24
  assert tok[1:1 + len(fields)] == [getattr(_abi.GaussianHead, f).offset for f in fields]
  assert tok[-4:] == [_abi.HEAD_MEAN, _abi.HEAD_SAMPLE, _abi.LOGSTD_CLAMP, _abi.LOGSTD_TANH]


# ---------------------------------------------------------------------------------------------------------------- 8. no scratch, occupancy kept
def test_no_gaussian_instantiation_uses_scratch_and_one_hidden_layer_keeps_two_waves():
  figures = {k: fig for k, fig in kernel_build.unit('tabletop_policy_gaussian.hip').figures.items() if 'policy_rollout_kernel' in k}
  assert len(figures) == 10, figures                                    # NT2 = 0..4 x GENERAL, all with GAUSS = true
  for name, (_, vgpr, agpr, scratch, occ, _) in figures.items():
    print(name, vgpr, agpr, scratch, occ)
    assert 'Lb1EEE' in name, name                                       # (the third template argument)
    assert scratch == 0, (name, scratch)
    if 'ILi0E' in name:
      assert vgpr + agpr <= 256 and occ >= 2, (name, vgpr, agpr, occ)


# ---------------------------------------------------------------------------------------------------------------- 9. the Python surface on the host
def test_gaussian_mlp_policy_and_rollout_policy_on_the_host():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  ref = GaussPolicy((64,), seed=6, log_std_gain=1.0)
  pi = GaussianMLPPolicy(ref.layers, 'relu', squash=True, log_std_bounds=(-5.0, 2.0), log_std_map='tanh', device='cpu')
  assert eb.GaussianMLPPolicy is GaussianMLPPolicy and pi.dims == [12, 64, 6] and pi.out_act == 'tanh'
  np.testing.assert_array_equal(pi.params.numpy(), ref.params.numpy())
  n, T = 33, 20
  _, eval_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=n, device='cpu', seed=3).get_envs()
  sd = eval_env.unwrapped.state_dict()
  obs, rew, done, succ, act, eps = eval_env.rollout_policy(pi, T, episodes=2, return_noise=True)
  assert tuple(obs.shape) == (2, T, n, 12) and tuple(act.shape) == tuple(eps.shape) == (2, T, n, 3) and eval_env.total_steps == 2 * T
  assert int(eval_env.num_interventions.sum()) == 2 * n and 0.8 < float(eps.std()) < 1.2
  end = eval_env.unwrapped.state_dict()
  # the torch statement of the contract: observation consumed at step t + 1 is row t
  torch.testing.assert_close(pi.sample(obs[0, :-1], eps[0, 1:]), act[0, 1:], rtol=1e-4, atol=1e-4)
  eval_env.unwrapped.load_state_dict(sd)
  o2, r2, d2, s2 = eval_env.rollout_episodes(act)
  assert torch.equal(obs.view(torch.int32), o2.view(torch.int32)) and torch.equal(rew, r2) and torch.equal(done, d2) and torch.equal(succ, s2)
  assert eval_env.unwrapped.state_dict()['rng_counter'] == end['rng_counter']
  # five outputs without return_noise, and the same draws; sample=False is the mean, == MLPPolicy on the 3-output twin
  eval_env.unwrapped.load_state_dict(sd)
  again = eval_env.rollout_policy(pi, T, episodes=2)
  assert len(again) == 5 and torch.equal(again[4], act)
  eval_env.unwrapped.load_state_dict(sd)
  m = eval_env.rollout_policy(pi, T, episodes=2, sample=False)
  twin = ref.mean_twin()
  eval_env.unwrapped.load_state_dict(sd)
  d = eval_env.rollout_policy(MLPPolicy(twin.layers, 'relu', 'tanh', device='cpu'), T, episodes=2)
  assert len(m) == len(d) == 5 and all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(m, d))
  torch.testing.assert_close(pi(m[0][0, :-1]), m[4][0, 1:], rtol=1e-4, atol=1e-4)
  with pytest.raises(ValueError):
    eval_env.rollout_policy(MLPPolicy(twin.layers, device='cpu'), T, sample=False)
  with pytest.raises(ValueError):
    eval_env.rollout_policy(MLPPolicy(twin.layers, device='cpu'), T, return_noise=True)
  # the train env: lifelong wrapper, continuing form, clamp map, no squashing
  pc = GaussianMLPPolicy(ref.layers, 'relu', squash=False, log_std_bounds=(-2.0, 0.5), log_std_map='clamp')
  train_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', setup_as_lifelong_learning=True, num_envs=n, device='cpu', seed=3).get_envs()
  train_env.unwrapped._cfg.goal_change_frequency = 7
  train_env.reset()
  sd = train_env.unwrapped.state_dict()
  obs, rew, done, succ, act, eps = train_env.rollout_policy(pc, T, reset_first=False, return_noise=True)
  assert tuple(obs.shape) == (T, n, 12) and tuple(eps.shape) == (T, n, 3) and float(act.abs().max()) > 1
  torch.testing.assert_close(pc.sample(obs[:5], eps[1:6]), act[1:6], rtol=1e-4, atol=1e-4)       # (before the first goal switch at step 7)
  lret = train_env.lifelong_return.clone()
  train_env.unwrapped.load_state_dict(sd)
  o2, r2, d2, s2 = train_env.rollout(act)
  assert torch.equal(obs.view(torch.int32), o2.view(torch.int32)) and torch.equal(rew, r2) and torch.equal(lret, train_env.lifelong_return)


def test_gaussian_mlp_policy_rejects_what_the_kernel_cannot_take():
  from earl_benchmark_amd.policy import GaussianMLPPolicy

  def net(*dims):
    return [(np.zeros((n, k), np.float32), np.zeros(n, np.float32)) for k, n in zip(dims[:-1], dims[1:])]

  GaussianMLPPolicy(net(12, 16, 6))
  GaussianMLPPolicy(net(12, 256, 256, 6), log_std_bounds=(-20, 4), log_std_map='clamp', squash=False)
  for dims, what in (((12, 16, 3), 'width 3'), ((12, 16, 7), 'width 7'), ((12, 24, 6), 'width 24'), ((13, 16, 6), 'width 13'), ((12, 16, 16, 16, 6), '3 hidden layers')):
    with pytest.raises(ValueError, match=what):
      GaussianMLPPolicy(net(*dims))
  for kw in (dict(log_std_map='softplus'), dict(log_std_bounds=(2.0, -5.0)), dict(log_std_bounds=(-21.0, 2.0)), dict(log_std_bounds=(-5.0, 4.5)),
             dict(log_std_bounds=(float('nan'), 2.0)), dict(hidden_act='gelu')):
    with pytest.raises(ValueError):
      GaussianMLPPolicy(net(12, 16, 6), **kw)
  seq = torch.nn.Sequential(torch.nn.Linear(12, 32), torch.nn.ReLU(), torch.nn.Linear(32, 32), torch.nn.ReLU(), torch.nn.Linear(32, 6))
  pi = GaussianMLPPolicy(seq)
  assert pi.dims == [12, 32, 32, 6] and pi.hidden_act == 'relu' and pi.squash and pi.log_std_map == 'tanh' and pi.log_std_bounds == (-5.0, 2.0)
  x = torch.randn(5, 12)
  y = seq(x)
  torch.testing.assert_close(pi(x), torch.tanh(y[:, :3]))
  eps = torch.randn(5, 3)
  torch.testing.assert_close(pi.sample(x, eps), torch.tanh(y[:, :3] + torch.exp(-5.0 + 3.5 * (torch.tanh(y[:, 3:]) + 1)) * eps))
  with pytest.raises(ValueError):
    GaussianMLPPolicy(torch.nn.Sequential(torch.nn.Linear(12, 32), torch.nn.ReLU(), torch.nn.Linear(32, 6), torch.nn.Tanh()))

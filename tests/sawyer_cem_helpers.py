"""The oracle and the drivers of the Sawyer door / peg CEM planner (include/earl_physics.h, "CEM planning on the door and the peg": earl_sawyer_plan_cem,
earl_sawyer_cem_candidates, earl_sawyer_cem_update) for tests/test_sawyer_cem.py (no GPU: the host twins of libearl_host.so) and tests/test_sawyer_cem_gpu.py; a plain
module.

THE ORACLE uses none of the planner's code: `candidates` below is item 2 of the contract with FOUR words of the Philox block and word 0 = CEM_DRAW | j, on
tests/tabletop_plan_helpers.py's numpy Philox, host-built normal_quantile_f32, exact fmaf and clip, with the per-row clamped std; items 4 - 5 are
tests/tabletop_cem_helpers.py's `elites` (a Python sort on (is-NaN, -ret, k)) and `update` (Python integers), which are generic in the action dimension; beta and best_k
are tests/tabletop_plan_helpers.py's `weights`; the returns are the existing rollout_branches' (GPU tests) or crafted (`patterns`)."""
import ctypes as C

import numpy as np

from earl_benchmark_amd import _abi
from sawyer_plan_helpers import cfg_of, ptr, sigma4  # noqa: F401  (re-exported for the tests)
from tabletop_cem_helpers import CEM_DRAW, elites, sclamp, update
from tabletop_plan_helpers import clip, fmaf32, philox4x32_10, quantile, weights

F32, F64 = np.float32, np.float64
MAX_K, MAX_E = 8192, 1024


def std_rows(std0, sigma, H, n):
  """the std entering an iteration before its clamp: std0, or sigma in every row"""
  return np.broadcast_to(sigma4(sigma), (H, n, 4)).copy() if std0 is None else np.asarray(std0, F32)


def candidates(seed, env_offset, n, K, H, j, nc, mean, s):
  """items 1 - 2 with the clamped std s [H, n, 4] -> (act [K, H, n, 4], m [H, n, 4])"""
  m = clip(mean)
  k = np.arange(K, dtype=np.uint64)[:, None, None]
  t = np.arange(H, dtype=np.uint64)[None, :, None]
  g = ((np.arange(n, dtype=np.int64) + int(env_offset)) & 0xFFFFFFFF).astype(np.uint64)[None, None, :]
  shape = (K, H, n)
  ctr = (np.full(shape, CEM_DRAW | j, np.uint64), np.broadcast_to(g, shape), np.broadcast_to((k << np.uint64(16)) | t, shape), np.full(shape, nc & 0xFFFFFFFF, np.uint64))
  words = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
  eps = quantile(np.stack([(w >> np.uint64(8)).astype(np.uint32) for w in words], -1))
  act = clip(fmaf32(np.broadcast_to(s[None], eps.shape), eps, np.broadcast_to(m[None], eps.shape)))
  act[0] = m
  return act, m


def params(K, H, I=1, E=2, sigma=0.3, alpha=0.0, lo=0.0, hi=2.0, nc=7, iteration0=0):
  return _abi.SawyerCemParams(K=K, H=H, iterations=I, iteration0=iteration0, elites=E, sigma=(C.c_float * 4)(*[float(v) for v in sigma4(sigma)]),
                              noise_counter=nc & 0xFFFFFFFF, alpha=float(alpha), std_min=float(lo), std_max=float(hi))


def oracle_update(act, m, s, ret, E, alpha, lo, hi):
  """items 4 - 7 on given candidates and returns -> dict(plan, std, ret0, best_ret, best_k, elite [K, n] uint8, el: per env the elites, best first)"""
  ret = np.asarray(ret, F64)
  el = elites(ret, E)
  plan, std, _ = update(act, m, s, el, alpha, lo, hi)
  with np.errstate(over='ignore'):                                             # (the weights of huge returns overflow float32: they are not used here)
    _, beta, bk = weights(ret, 1.0)
  beta = np.where(beta > -np.inf, ret[bk, np.arange(ret.shape[1])], beta)      # beta IS ret[best_k]: where +0 and -0 tie for the maximum, numpy's max leaves the sign open
  mask = np.zeros(ret.shape, np.uint8)
  for i, ks in enumerate(el):
    mask[ks, i] = 1
  return dict(plan=plan, std=std, ret0=ret[0].copy(), best_ret=beta, best_k=bk, elite=mask, el=el)


def same_bits(got, want, what):
  """sawyer_plan_helpers.same_bits for words of any width (the elite bytes too)"""
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
  view = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
  bad = np.nonzero(got.view(view) != want.view(view))
  assert len(bad[0]) == 0, f'{what}: {len(bad[0])} words differ, first at {tuple(int(b[0]) for b in bad)}: {got[tuple(b[0] for b in bad)]!r} vs {want[tuple(b[0] for b in bad)]!r}'


def compare_update(got, want, what):
  for k in ('plan', 'std', 'best_ret', 'best_k', 'elite'):
    same_bits(got[k], want[k], f'{k} {what}')
  nan = np.isnan(want['ret0'])                                 # (a NaN return is copied, whatever its payload)
  assert np.array_equal(np.isnan(got['ret0']), nan), f'ret0 {what}'
  same_bits(got['ret0'][~nan], want['ret0'][~nan], f'ret0 {what}')


def host_candidates(host, cfg, pp, j, mean, std):
  """earl_sawyer_cem_candidates_cpu -> act [K, H, n, 4] (NaN-filled before the call: every word must be written)"""
  act = np.full((pp.K, pp.H, cfg.n, 4), np.nan, F32)
  mean = np.ascontiguousarray(mean, F32)
  std = None if std is None else np.ascontiguousarray(std, F32)
  rc = host.earl_sawyer_cem_candidates_cpu(C.byref(cfg), C.byref(pp), j, ptr(mean), ptr(std), ptr(act))
  assert rc == _abi.EARL_OK, host.earl_last_error()
  return act


def host_update(host, cfg, pp, j, mean, std_in, act, ret, in_place=False):
  """earl_sawyer_cem_update_cpu -> dict(plan, std [H, n, 4], ret0, best_ret, best_k [n], elite [K, n]); in_place: plan is mean and std is std_in (std_in given)"""
  n = cfg.n
  mean = np.array(mean, F32, order='C')                       # (copies: the in-place call writes them)
  std_in = None if std_in is None else np.array(std_in, F32, order='C')
  act, ret = np.ascontiguousarray(act, F32), np.ascontiguousarray(ret, F64)
  plan = mean if in_place else np.full(mean.shape, np.nan, F32)
  std = std_in if in_place and std_in is not None else np.full(mean.shape, np.nan, F32)
  ret0, best_ret, best_k, elite = np.full(n, np.nan, F64), np.full(n, np.nan, F64), np.full(n, -7, np.int32), np.full((pp.K, n), 9, np.uint8)
  rc = host.earl_sawyer_cem_update_cpu(C.byref(cfg), C.byref(pp), j, ptr(mean), ptr(std_in), ptr(act), ptr(ret), ptr(plan), ptr(std), ptr(ret0), ptr(best_ret), ptr(best_k),
                                       ptr(elite))
  assert rc == _abi.EARL_OK, host.earl_last_error()
  return dict(plan=plan, std=std, ret0=ret0, best_ret=best_ret, best_k=best_k, elite=elite)


def device_update(lib, cfg, pp, j, mean, std_in, act, ret, in_place=False):
  """earl_sawyer_cem_update on the current device -> host_update's dict as numpy arrays"""
  import torch
  n = cfg.n
  dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
  mean, act, ret = dev(mean, F32), dev(act, F32), dev(ret, F64)
  std_in = None if std_in is None else dev(std_in, F32)
  plan = mean if in_place else torch.full_like(mean, float('nan'))
  std = std_in if in_place and std_in is not None else torch.full_like(mean, float('nan'))
  ret0, best_ret = torch.full((n,), float('nan'), dtype=torch.float64, device='cuda'), torch.full((n,), float('nan'), dtype=torch.float64, device='cuda')
  best_k, elite = torch.full((n,), -7, dtype=torch.int32, device='cuda'), torch.full((pp.K, n), 9, dtype=torch.uint8, device='cuda')
  p = lambda t: None if t is None else t.data_ptr()
  rc = lib.earl_sawyer_cem_update(C.byref(cfg), C.byref(pp), j, p(mean), p(std_in), p(act), p(ret), p(plan), p(std), p(ret0), p(best_ret), p(best_k), p(elite),
                                  torch.cuda.current_stream().cuda_stream)
  assert rc == _abi.EARL_OK, lib.earl_last_error()
  torch.cuda.synchronize()
  return {k: v.cpu().numpy() for k, v in dict(plan=plan, std=std, ret0=ret0, best_ret=best_ret, best_k=best_k, elite=elite).items()}


# ---------------------------------------------------------------------------------------------------- crafted returns
def _bits(u):
  return np.asarray(u, np.uint64).view(F64)


def pattern(name, K, E, rng):
  """one env's K returns of the named pattern, and `holds(el, ret)`: the pattern's own condition on the ORACLE's elites el (best first) -- asserted wherever K lets the
  pattern exist, so that a case that stops exercising its path fails loudly"""
  if name == 'equal':                        # the sparse reward's real case
    return np.zeros(K), lambda el, r: sorted(el) == list(range(E))
  if name == 'tie':                          # two values, rank E - 1 inside a tie: G < E < G + ties (E == K: the tie ends with the branches)
    n_hi = E // 2 if E >= 2 else min(3, K)
    r = np.full(K, 1.5)
    r[rng.permutation(K)[:n_hi]] = 2.5
    def holds(el, r):
      v = r[el[-1]]
      G, ties = int((r > v).sum()), int((r == v).sum())
      first = [int(x) for x in np.nonzero(r == v)[0][:E - G]]
      return G < E and (E < G + ties or E == K) and sorted(x for x in el if r[x] == v) == first
    return r, holds
  if name == 'distinct':
    r = rng.permutation(K) * 0.37 - 11.0
    return r, lambda el, r: len(np.unique(r)) == K and el == [int(x) for x in np.argsort(-r)[:E]]
  if name == 'nans':                         # fewer numbers than E: Ne < E
    nn = E // 2
    r = np.full(K, np.nan)
    r[rng.permutation(K)[:nn]] = rng.normal(0.0, 1.0, nn)
    return r, lambda el, r: len(el) == nn < E
  if name == 'all_nan':
    return np.full(K, np.nan), lambda el, r: el == []
  if name == 'zeros':                        # +0 and -0 are one value: the tie goes by k, not by sign
    r = np.where(rng.integers(0, 2, K) == 1, 0.0, -0.0)
    r[rng.permutation(K)[:K // 3]] = -1.0
    def holds(el, r):
      z = [int(x) for x in np.nonzero(r == 0)[0]]
      return [x for x in el if r[x] == 0] == z[:E] and (K < 65 or E < 8 or len({bool(np.signbit(r[x])) for x in el if r[x] == 0}) == 2)
    return r, holds
  if name == 'infs':
    r = rng.normal(0.0, 1.0, K)
    idx = rng.permutation(K)
    r[idx[:K // 5]], r[idx[K // 5:2 * (K // 5)]], r[idx[2 * (K // 5):2 * (K // 5) + K // 7]] = np.inf, -np.inf, np.nan
    def holds(el, r):
      pinf = [int(x) for x in np.nonzero(r == np.inf)[0]]
      return el[:min(E, len(pinf))] == pinf[:E] and not any(np.isnan(r[x]) for x in el) and (K < 65 or len(pinf) > 1)
    return r, holds
  if name == 'low_byte':                     # keys that differ in their lowest byte only
    r = _bits(np.uint64(0x3FF0000000000000) | rng.integers(0, 256, K).astype(np.uint64))
    return r, lambda el, r: K < 65 or (len(np.unique(r)) > min(K, 256) // 2 and float(r.max() - r.min()) < 1e-13)
  if name == 'high_byte':                    # keys that differ in their highest byte only (positive numbers: the key is the bits with the sign set)
    r = _bits((rng.integers(0, 128, K).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000123456789ABCD))
    return r, lambda el, r: bool(np.isfinite(r).all()) and (K < 65 or len(np.unique(r)) > 40) and len(np.unique(r.view(np.uint64) & np.uint64((1 << 56) - 1))) == 1
  raise KeyError(name)


PATTERNS = (('equal', 'tie', 'distinct'), ('nans', 'all_nan', 'zeros'), ('infs', 'low_byte', 'high_byte'))


def crafted(names, K, E, H, seed):
  """one update call's inputs for n = len(names) envs, env i with pattern names[i] -> (mean, std_in, act, ret, holds): a mean beyond the box, a std with a NaN and
  entries outside [lo, hi], candidates anywhere in the box with branch 0 the clipped mean -- the update READS them, it cannot make them again"""
  rng = np.random.default_rng(seed)
  n = len(names)
  mean = rng.uniform(-1.15, 1.15, (H, n, 4)).astype(F32)
  std_in = rng.uniform(-0.1, 0.9, (H, n, 4)).astype(F32)
  std_in[0, 0, 1] = np.nan
  act = rng.uniform(-1.0, 1.0, (K, H, n, 4)).astype(F32)
  act[rng.integers(0, K, 8), rng.integers(0, H, 8), rng.integers(0, n, 8), rng.integers(0, 4, 8)] = rng.choice(np.array([-1.0, 1.0], F32), 8)
  act[0] = clip(mean)
  cols, holds = zip(*(pattern(nm, K, E, rng) for nm in names))
  return mean, std_in, act, np.stack(cols, 1).astype(F64), holds

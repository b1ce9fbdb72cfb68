"""The oracle and the drivers of the minitaur's MPPI planner (include/earl_physics.h: earl_minitaur_plan_mppi, earl_minitaur_plan_candidates) for
tests/test_minitaur_plan.py (no GPU: the host twins of libearl_host.so) and tests/test_minitaur_plan_gpu.py; a plain module.

THE ORACLE uses none of the planner's code: `candidates` below is item 2 of the contract with EIGHT words out of two Philox blocks -- the Sawyer oracle's block and
the block with bit 31 of word 2 set -- on tests/tabletop_plan_helpers.py's numpy Philox, host-built normal_quantile_f32, exact fmaf and clip, all imported through
tests/sawyer_plan_helpers.py; items 4 - 5 are that module's `oracle_update` (Python integers), generic in the action dimension."""
import ctypes as C

import numpy as np

from earl_benchmark_amd import _abi
from sawyer_plan_helpers import F32, F64, oracle_update, ptr, same_bits      # noqa: F401  (re-exported to the two test files)
from tabletop_plan_helpers import PLAN_DRAW, clip, fmaf32, philox4x32_10, quantile


def sigma8(sigma):
  return np.broadcast_to(np.asarray(sigma, F32), (8,)).copy()


def candidates(seed, env_offset, n, K, H, j, sigma, nc, mean):
  """items 1 - 2 -> (act [K, H, n, 8], m [H, n, 8])"""
  m = clip(mean)
  k = np.arange(K, dtype=np.uint64)[:, None, None]
  t = np.arange(H, dtype=np.uint64)[None, :, None]
  g = ((np.arange(n, dtype=np.int64) + int(env_offset)) & 0xFFFFFFFF).astype(np.uint64)[None, None, :]
  shape = (K, H, n)
  key = (int(seed) & 0xFFFFFFFF, int(seed) >> 32)
  words = []
  for hi in (0, 0x80000000):
    ctr = (np.full(shape, PLAN_DRAW | j, np.uint64), np.broadcast_to(g, shape), np.broadcast_to(np.uint64(hi) | (k << np.uint64(16)) | t, shape),
           np.full(shape, nc & 0xFFFFFFFF, np.uint64))
    words += list(philox4x32_10(ctr, key))
  k24 = np.stack([(w >> np.uint64(8)).astype(np.uint32) for w in words], -1)
  eps = quantile(k24)
  sg = sigma8(sigma).reshape(1, 1, 1, 8)
  act = clip(fmaf32(np.broadcast_to(sg, eps.shape), eps, np.broadcast_to(m[None], eps.shape)))
  act[0] = m
  return act, m


def params(K, H, I=1, sigma=0.3, inv_t=1.0, nc=7, iteration0=0):
  return _abi.MinitaurPlanParams(K=K, H=H, iterations=I, iteration0=iteration0, sigma=(C.c_float * 8)(*[float(v) for v in sigma8(sigma)]), noise_counter=nc & 0xFFFFFFFF,
                                 inv_temperature=float(inv_t))


def cfg_of(n, env_offset=0, seed=0):
  """the three words of earl_minitaur_cfg the planner's own arithmetic reads"""
  return _abi.MinitaurCfg(n=n, env_offset=env_offset, seed=seed)


def host_candidates(host, cfg, pp, j, mean):
  """earl_minitaur_plan_candidates_cpu -> act [K, H, n, 8] (NaN-filled before the call: every word must be written)"""
  act = np.full((pp.K, pp.H, cfg.n, 8), np.nan, F32)
  mean = np.ascontiguousarray(mean, F32)
  rc = host.earl_minitaur_plan_candidates_cpu(C.byref(cfg), C.byref(pp), j, ptr(mean), ptr(act))
  assert rc == _abi.EARL_OK, host.earl_last_error()
  return act


def host_update(host, cfg, pp, j, mean, act, ret, in_place=False):
  """earl_minitaur_plan_update_cpu -> dict(plan [H, n, 8], ret0 [n], best_ret [n], best_k [n])"""
  n = cfg.n
  mean = np.array(mean, F32, order='C')                       # (a copy: the in-place call writes it)
  act, ret = np.ascontiguousarray(act, F32), np.ascontiguousarray(ret, F64)
  plan = mean if in_place else np.full(mean.shape, np.nan, F32)
  ret0, best_ret, best_k = np.full(n, np.nan, F64), np.full(n, np.nan, F64), np.full(n, -7, np.int32)
  rc = host.earl_minitaur_plan_update_cpu(C.byref(cfg), C.byref(pp), j, ptr(mean), ptr(act), ptr(ret), ptr(plan), ptr(ret0), ptr(best_ret), ptr(best_k))
  assert rc == _abi.EARL_OK, host.earl_last_error()
  return dict(plan=plan, ret0=ret0, best_ret=best_ret, best_k=best_k)


def same(got, want, what):
  """same_bits with NaNs of any payload equal to each other (ret0 rows copied from returns that hold a NaN)"""
  got, want = np.asarray(got), np.asarray(want)
  assert np.array_equal(np.isnan(got), np.isnan(want)), what
  same_bits(np.where(np.isnan(got), 0, got).astype(got.dtype), np.where(np.isnan(want), 0, want).astype(want.dtype), what)

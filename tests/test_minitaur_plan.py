"""The minitaur's MPPI planner (include/earl_physics.h: earl_minitaur_plan_mppi, earl_minitaur_plan_candidates, earl_minitaur_plan_ws_bytes), what can be held without a
GPU:
  1. the candidates twin (earl_minitaur_plan_candidates_cpu) equals the Python oracle of tests/minitaur_plan_helpers.py bit for bit, and its words 0 .. 3 equal the
     Sawyer twin's for the same scalars;
  2. the update twin (earl_minitaur_plan_update_cpu) equals items 4 - 7 in Python integers on synthetic returns -- ties, one NaN, all equal -- at K = 4 and K = 65, in
     place and out of place; overlap without equality is refused;
  3. every refusal of the header's list returns EARL_ERR_ARG before the entry point touches the device; the workspace size query;
  4. the Python front end's argument errors;
  5. both kernels of csrc/minitaur_plan.hip compile for gfx950 without scratch, and the unit holds nothing else.
The GPU side is tests/test_minitaur_plan_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_build
import minitaur_plan_helpers as mp
import sawyer_plan_helpers as sp
from earl_benchmark_amd import _abi
from test_physics_abi import EARL_ERR_ARG, host_ptr, minitaur_args

F32, F64 = np.float32, np.float64
N, OFF, K, H, SEED, NC = 3, 5, 5, 4, 0x1234567890ABCDEF, 0x9E3779B9
SIGMA = (0.5, 0.0, 0.8, 0.3, 0.2, 0.6, 0.4, 0.7)


def nasty_mean(seed=2, H=H, n=N):
  """entries beyond +-1, a NaN and both infinities"""
  mean = np.random.default_rng(seed).uniform(-1.15, 1.15, (H, n, 8)).astype(F32)
  mean[0, 1 % n, 0], mean[1 % H, 2 % n, 7], mean[2 % H, 0, 5] = np.nan, np.inf, -np.inf
  return mean


# ---------------------------------------------------------------------------------------------------------------- 1. candidates
@pytest.mark.parametrize('j', [0, 1])
def test_candidates_twin_equals_the_oracle(j):
  host = _abi.load_host()
  mean = nasty_mean()
  want, m = mp.candidates(SEED, OFF, N, K, H, j, SIGMA, NC, mean)
  assert bool((np.abs(mean) > 1).any()) and np.isfinite(want).all() and float(np.abs(want).max()) <= 1.0
  mp.same_bits(want[0], sp.clip(mean), 'row 0 is the clipped mean')
  assert m[0, 1, 0] == -1 and m[1, 2, 7] == 1 and m[2, 0, 5] == -1                      # NaN -> -1, +-Inf -> +-1
  mp.same_bits(want[:, :, :, 1], np.broadcast_to(m[None, :, :, 1], (K, H, N)), 'sigma = 0 in one dimension: the clipped mean')
  for d in (0, 2, 3, 4, 5, 6, 7):
    assert bool((want[1:, :, :, d] != m[None, :, :, d]).any()), d                       # every other dimension is drawn, the second block's included
  got = mp.host_candidates(host, mp.cfg_of(N, OFF, SEED), mp.params(K, H, sigma=SIGMA, nc=NC), j, mean)
  assert not np.isnan(got).any(), 'a word was not written'
  mp.same_bits(got, want, f'candidates of iteration {j}')


def test_words_0_to_3_are_the_sawyer_candidates():
  host = _abi.load_host()
  mean = nasty_mean()
  for j in (0, 1):
    got = mp.host_candidates(host, mp.cfg_of(N, OFF, SEED), mp.params(K, H, sigma=SIGMA, nc=NC), j, mean)
    twin = sp.host_candidates(host, sp.cfg_of(N, OFF, SEED), sp.params(K, H, sigma=SIGMA[:4], nc=NC), j, np.ascontiguousarray(mean[..., :4]))
    mp.same_bits(np.ascontiguousarray(got[..., :4]), twin, f'words 0 .. 3 of iteration {j}')
    # the second block is another block: same sigma and mean in dimensions 0 and 4 give other words
    eq = mp.host_candidates(host, mp.cfg_of(N, OFF, SEED), mp.params(K, H, sigma=0.5, nc=NC), j, np.zeros((H, N, 8), F32))
    assert not np.array_equal(eq[1:, ..., 0], eq[1:, ..., 4])


def test_candidates_depend_on_the_global_id_and_the_counters_only():
  host = _abi.load_host()
  mean = nasty_mean()
  full = mp.host_candidates(host, mp.cfg_of(N, OFF, SEED), mp.params(K, H, sigma=0.5, nc=NC), 1, mean)
  part = mp.host_candidates(host, mp.cfg_of(2, OFF + 1, SEED), mp.params(K, H, sigma=0.5, nc=NC), 1, mean[:, 1:])
  mp.same_bits(part, full[:, :, 1:], 'a shard of two envs')
  for other in (mp.host_candidates(host, mp.cfg_of(N, OFF, SEED), mp.params(K, H, sigma=0.5, nc=NC + 1), 1, mean),
                mp.host_candidates(host, mp.cfg_of(N, OFF, SEED), mp.params(K, H, sigma=0.5, nc=NC), 2, mean),
                mp.host_candidates(host, mp.cfg_of(N, OFF, SEED + 1), mp.params(K, H, sigma=0.5, nc=NC), 1, mean)):
    mp.same_bits(other[0], full[0], 'row 0')
    assert not np.array_equal(other[1:, ..., :4], full[1:, ..., :4]) and not np.array_equal(other[1:, ..., 4:], full[1:, ..., 4:])


# ---------------------------------------------------------------------------------------------------------------- 2. update
def synthetic_returns(K, rng):
  """[K, 4], negative like the env's: env 0 distinct, 1 ties for the maximum, 2 one NaN (where the maximum would have been), 3 all equal"""
  ret = -rng.uniform(0.1, 3.0, (K, 4))
  ret[[1, K - 2], 1] = -0.05
  ret[int(np.argmax(ret[:, 2])), 2] = np.nan
  ret[:, 3] = -1.25
  return ret


@pytest.mark.parametrize('K', [4, 65])
@pytest.mark.parametrize('in_place', [False, True])
def test_update_twin_equals_python_integers(K, in_place):
  host = _abi.load_host()
  H, n, inv_t = 3, 4, 2.0
  mean = nasty_mean(3, H, n)
  act, m = mp.candidates(SEED, OFF, n, K, H, 4, SIGMA, NC, mean)
  ret = synthetic_returns(K, np.random.default_rng(5))
  want = mp.oracle_update(act, m, ret, inv_t)
  W = want['W']
  # the cases, on the oracle
  assert want['best_k'].tolist() == [int(np.argmax(ret[:, 0])), 1, int(np.nanargmax(ret[:, 2])), 0]
  assert (W[:, 2] == 0).sum() >= 1 and W[np.isnan(ret[:, 2]), 2].tolist() == [0] and (W[:, 3] == 2**24).all() and W[1, 1] == W[K - 2, 1] == 2**24
  assert want['best_ret'][1] == -0.05 and want['best_ret'][3] == -1.25 and bool((want['plan'][:, 0] != m[:, 0]).any())
  got = mp.host_update(host, mp.cfg_of(n, OFF, SEED), mp.params(K, H, inv_t=inv_t), 4, mean, act, ret, in_place=in_place)
  for k in ('plan', 'best_ret', 'best_k', 'ret0'):
    mp.same(got[k], want[k], f'{k} (K = {K}, in place: {in_place})')


def test_update_refuses_overlap_without_equality_and_the_rest():
  host = _abi.load_host()
  nan = float('nan')
  mean, act, ret, other = host_ptr(1 << 16), host_ptr(1 << 16), host_ptr(), host_ptr(1 << 16)
  cfg, pp = mp.cfg_of(4), mp.params(2, 3)
  upd = lambda cfg, pp, j, mean, a, ret, plan: host.earl_minitaur_plan_update_cpu(None if cfg is None else C.byref(cfg), None if pp is None else C.byref(pp), j, mean, a, ret,
                                                                                  plan, None, None, None)
  for args in ((cfg, pp, 0, mean, act, ret, mean + 32), (cfg, pp, 0, mean, act, ret, mean - 32), (cfg, pp, 0, mean, act, ret, mean + 3 * 4 * 32 - 4),
               (None, pp, 0, mean, act, ret, other), (cfg, None, 0, mean, act, ret, other), (cfg, pp, 0, None, act, ret, other), (cfg, pp, 0, mean, None, ret, other),
               (cfg, pp, 0, mean, act, None, other), (cfg, pp, 0, mean, act, ret, None), (cfg, pp, 256, mean, act, ret, other), (cfg, pp, -1, mean, act, ret, other),
               (cfg, mp.params(2, 3, inv_t=0.0), 0, mean, act, ret, other), (cfg, mp.params(2, 3, inv_t=nan), 0, mean, act, ret, other),
               (cfg, mp.params(_abi.MINITAUR_PLAN_MAX_K + 1, 3), 0, mean, act, ret, other)):
    assert upd(*args) == EARL_ERR_ARG and host.earl_last_error(), args
  assert upd(mp.cfg_of(0), pp, 0, mean, act, ret, other) == _abi.EARL_OK


# ---------------------------------------------------------------------------------------------------------------- 3. refusals and sizes
def ws_bytes(lib, K, H, n):
  need = C.c_int64(-1)
  rc = lib.earl_minitaur_plan_ws_bytes(K, H, n, C.byref(need))
  return rc, need.value


MEAN = host_ptr(1 << 16)


def call(lib, cfg, st, tell=None, model='given', params='given', mean=MEAN, plan='other', ret='given', ws='given', ws_bytes_=1 << 40, ws_base=None):
  """earl_minitaur_plan_mppi on host stand-in pointers: only for calls that return before anything reads through them.  tell: fields of earl_minitaur_plan_params"""
  pp = mp.params(2, 3, I=1, sigma=0.3, inv_t=1.0)
  for k, v in (tell or {}).items():
    setattr(pp, k, (C.c_float * 8)(*v) if k == 'sigma' else v)
  w = None if ws is None else _abi.MinitaurBranchWs(base=(host_ptr() if ws_base is None else ws_base) if ws == 'given' else None, bytes=ws_bytes_)
  pl = {'other': host_ptr(1 << 16), 'same': mean, None: None}.get(plan, plan)
  return lib.earl_minitaur_plan_mppi(host_ptr() if model == 'given' else None, None, None if cfg is None else C.byref(cfg), None if st is None else C.byref(st),
                                     C.byref(pp) if params == 'given' else None, mean, pl, host_ptr() if ret == 'given' else None, host_ptr(), host_ptr(), host_ptr(), host_ptr(),
                                     None, None if w is None else C.byref(w), None)


def test_every_refusal_fires_before_the_device():
  """n = 4 and K = 2: an accepted call would launch, so every EARL_ERR_ARG below was decided on the host"""
  lib = _abi.load()
  nan, inf = float('nan'), float('inf')
  cfg, st, _ = minitaur_args(n=4)

  def refused(*a, **kw):
    return call(lib, *a, **kw) == EARL_ERR_ARG and bool(lib.earl_last_error())

  # what earl_minitaur_branch_rollout refuses in model / cfg / st
  assert refused(cfg, st, model=None) and refused(None, st) and refused(cfg, None)
  assert refused(*minitaur_args(n=-1)[:2]) and refused(*minitaur_args(n=4, gcf=2, with_sgc=False)[:2])
  c2, s2, _ = minitaur_args(n=4)
  s2.overheat = None
  assert refused(c2, s2)
  c2, s2, _ = minitaur_args(n=4)
  c2.n_goals = 0
  assert refused(c2, s2)
  # the planner's own
  for kw in (dict(params=None), dict(mean=None), dict(plan=None), dict(ret=None), dict(ws=None)):
    assert refused(cfg, st, **kw), kw
  s8 = lambda d, v: tuple(v if i == d else 0.1 for i in range(8))
  for tell in (dict(K=0), dict(K=-1), dict(K=_abi.MINITAUR_PLAN_MAX_K + 1), dict(H=0), dict(H=-1), dict(H=65537), dict(iterations=0), dict(iteration0=-1),
               dict(iteration0=250, iterations=7), dict(iteration0=2**31 - 1, iterations=2**31 - 1), dict(sigma=s8(1, -0.1)), dict(sigma=s8(7, -0.1)), dict(sigma=s8(4, nan)),
               dict(sigma=s8(0, inf)), dict(inv_temperature=0.0), dict(inv_temperature=-1.0), dict(inv_temperature=nan), dict(inv_temperature=inf)):
    assert refused(cfg, st, tell=tell), tell
  assert refused(cfg, st, plan=MEAN + 32) and refused(cfg, st, plan=MEAN - 32) and refused(cfg, st, plan=MEAN + 3 * 4 * 32 - 4)      # a partial overlap (H n 32 = 384 bytes)
  big, bst, _ = minitaur_args(n=1 << 19)
  assert refused(big, bst, tell=dict(K=4096))                                            # K n = 2^31
  need = ws_bytes(lib, 2, 3, 4)[1]
  assert need > 0 and refused(cfg, st, ws_bytes_=need - 1)                               # too small
  assert refused(cfg, st, ws='null base') and refused(cfg, st, ws_base=host_ptr(1 << 16) + 4)
  # the empty call, and the generic-stepper comparison build
  zero, zst, _ = minitaur_args(n=0)
  assert call(lib, zero, zst) == _abi.EARL_OK and call(lib, zero, zst, ws='null base', ws_bytes_=0) == _abi.EARL_OK and call(lib, zero, zst, plan='same') == _abi.EARL_OK
  assert call(lib, zero, zst, tell=dict(K=0)) == EARL_ERR_ARG                            # (the parameter rules hold for an empty batch too)
  assert lib.earl_debug_set_minitaur_stepper(0) == 0
  try:
    assert refused(cfg, st)
  finally:
    assert lib.earl_debug_set_minitaur_stepper(1) == 0


def test_candidates_refusals_on_both_libraries():
  lib, host = _abi.load(), _abi.load_host()
  nan = float('nan')
  act = host_ptr(1 << 16)
  act += act % 16

  def both(cfg, pp, j, mean, out):
    a = lib.earl_minitaur_plan_candidates(None if cfg is None else C.byref(cfg), None if pp is None else C.byref(pp), j, mean, out, None)
    b = host.earl_minitaur_plan_candidates_cpu(None if cfg is None else C.byref(cfg), None if pp is None else C.byref(pp), j, mean, out)
    assert a == b, (a, b)
    return a

  cfg, pp = mp.cfg_of(4), mp.params(2, 3)
  for args in ((None, pp, 0, MEAN, act), (cfg, None, 0, MEAN, act), (cfg, pp, 0, None, act), (cfg, pp, 0, MEAN, None), (cfg, pp, -1, MEAN, act), (cfg, pp, 256, MEAN, act),
               (mp.cfg_of(-1), pp, 0, MEAN, act), (cfg, mp.params(0, 3), 0, MEAN, act), (cfg, mp.params(_abi.MINITAUR_PLAN_MAX_K + 1, 3), 0, MEAN, act),
               (cfg, mp.params(2, 0), 0, MEAN, act), (cfg, mp.params(2, 65537), 0, MEAN, act), (cfg, mp.params(2, 3, sigma=(0.1,) * 7 + (nan,)), 0, MEAN, act),
               (cfg, mp.params(2, 3, sigma=-0.5), 0, MEAN, act), (mp.cfg_of(1 << 19), mp.params(4096, 3), 0, MEAN, act)):
    assert both(*args) == EARL_ERR_ARG, args
  assert lib.earl_minitaur_plan_candidates(C.byref(cfg), C.byref(pp), 0, MEAN, act + 4, None) == EARL_ERR_ARG      # the device call stores 16 bytes at a time
  assert both(mp.cfg_of(0), pp, 0, MEAN, act) == _abi.EARL_OK                                                       # n == 0: nothing written


def test_workspace_size_holds_the_branch_block_and_the_candidates():
  lib = _abi.load()
  for K_, H_, n_ in ((0, 3, 7), (7, 3, 0), (0, 0, 0)):
    assert ws_bytes(lib, K_, H_, n_) == (_abi.EARL_OK, 0)
  grid = [(K_, H_, n_) for K_ in (1, 2, 65, 8192) for H_ in (1, 2, 20) for n_ in (1, 5, 64)]
  sizes = {g: ws_bytes(lib, *g) for g in grid}
  assert all(rc == _abi.EARL_OK and b > 0 for rc, b in sizes.values())
  for a, (_, b) in sizes.items():
    branch = C.c_int64(-1)
    assert lib.earl_minitaur_branch_ws_bytes(a[0], a[2], C.byref(branch)) == _abi.EARL_OK
    assert b >= branch.value + a[0] * a[1] * a[2] * 32 and b % 8 == 0, (a, b)
    for a2, (_, b2) in sizes.items():
      if all(x2 >= x for x2, x in zip(a2, a)) and a2 != a:
        assert b2 > b, (a, a2)
  assert ws_bytes(lib, 1 << 15, 1, 1 << 16)[0] == EARL_ERR_ARG and ws_bytes(lib, -1, 1, 4)[0] == EARL_ERR_ARG
  assert ws_bytes(lib, 1, -1, 4)[0] == EARL_ERR_ARG and ws_bytes(lib, 1, 1, -4)[0] == EARL_ERR_ARG
  assert lib.earl_minitaur_plan_ws_bytes(1, 1, 1, None) == EARL_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- 4. the Python front end
def test_python_argument_errors():
  import torch
  from test_minitaur_branches import bare
  env = bare()
  mean = torch.zeros(4, 3, 8)
  for kw in (dict(), dict(mean=torch.zeros(4, 3, 4)), dict(mean=torch.zeros(4, 2, 8)), dict(mean=mean, horizon=5), dict(mean=mean, sigma=(0.1, 0.2, 0.3, 0.4)),
             dict(mean=mean, temperature=0.0), dict(mean=mean, K=0), dict(mean=mean, K=_abi.MINITAUR_PLAN_MAX_K + 1), dict(mean=mean, iterations=0),
             dict(mean=mean, out={'nope': mean}), dict(mean=mean, out={'ret0': torch.zeros(1, 3, dtype=torch.float64)}), dict(mean=mean, out={'plan': torch.zeros(4, 3, 4)}),
             dict(mean=mean, K=4, out={'plan': mean, 'ret': torch.zeros(4, 3)}), dict(mean=mean, K=4, out={'plan': mean, 'fail': torch.zeros(4, 3, dtype=torch.int64)})):
    with pytest.raises(ValueError, match='mppi_plan|out\\['):
      env.mppi_plan(**kw)
  for args, kw in (((torch.zeros(4, 3, 4), 4), {}), ((mean, 0), {}), ((mean, 4), dict(sigma=(1.0, 2.0)))):
    with pytest.raises(ValueError, match='mppi_candidates'):
      env.mppi_candidates(*args, **kw)
  for kw in (dict(T=0, horizon=4), dict(T=2), dict(T=2, plan=torch.zeros(4, 3, 4)), dict(T=2, horizon=4, K=0), dict(T=2, horizon=4, temperature=-1.0),
             dict(T=2, horizon=4, sigma=(0.1,) * 4)):
    with pytest.raises(ValueError, match='mppi_control'):
      env.mppi_control(**kw)


# ---------------------------------------------------------------------------------------------------------------- 5. the build
def test_the_two_kernels_compile_without_scratch_and_the_unit_holds_nothing_else():
  unit = kernel_build.unit('minitaur_plan.hip')
  res = unit.resources
  print(res)
  assert sorted(res) == ['minitaur_plan_candidates_kernel', 'minitaur_plan_update_kernel'], sorted(res)
  for name, r in res.items():
    assert r['scratch'] == 0, (name, r)
  assert res['minitaur_plan_candidates_kernel']['lds'] == 0
  assert _abi.MINITAUR_PLAN_MAX_K * 4 <= res['minitaur_plan_update_kernel']['lds'] <= 40 * 1024      # one env's int32 weights, and the waves' maxima
  mk = open(os.path.join(kernel_build.CSRC, 'Makefile')).read()
  src = re.search(r'^SRC\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
  assert src.count('minitaur_plan.hip') == 1 and len(src) == len(set(src))
  text = ''.join(open(os.path.join(kernel_build.CSRC, f)).read() for f in ('minitaur_plan.hip', 'minitaur_plan.h', 'minitaur_branch_ws.h'))
  assert not re.search(r'#include\s+"(physics_|minitaur_stepper|minitaur_device)', text), 'the planner reaches the branch launch through the public ABI only'

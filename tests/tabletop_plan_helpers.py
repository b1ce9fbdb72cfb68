"""Drivers and the oracle of earl_tabletop[3]_plan_mppi / earl_tabletop_plan_candidates (include/earl_tabletop.h, "MPPI planning") for tests/test_tabletop_plan.py
(libearl_host.so) and tests/test_tabletop_plan_gpu.py (libearl_hip.so); a plain module on tests/tabletop_abi.py's banded buffers and tests/tabletop_branch_helpers.py's
scenes (a few steps off a reset at the goal, dirty last rows; `general`: horizon 7 + auto-reset, + a goal switch every 3 steps with one object).

THE ORACLE uses none of the planner's code:
  candidates   a numpy Philox4x32-10 (restated below), normal_quantile_f32 from the policy-math host build (tests/policy_math_ref.py), fmaf in exact arithmetic
               (`fmaf32`: the float64 product of two float32 is exact, the sum by TwoSum, one rounding to float32)
  returns      the SAME library's existing earl_tabletop[3]_branch_rollout fed with those candidates (on the device: the device's own)
  weights      exp_f32 from the policy-math host build; items 4-5 of the contract in numpy float32 / float64 and Python integers
The planner must equal it bit for bit in every output, under both rewards.  Device against twin: bit for bit under the sparse reward; under the dense one ret, ret0
and best_ret within the branch launch's bound |d ret| <= 1e-6 * sum_t |r_t| and the plans not compared.
"""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import torch

import policy_math_ref as pm
import tabletop_abi as ta
import tabletop_branch_helpers as tb
from earl_benchmark_amd import _abi

OUTS = ('plan', 'ret', 'ret0', 'best_ret', 'best_k')
OPTIONAL = ('ret0', 'best_ret', 'best_k')
PLAN_DRAW = 0x504C4E00
M32 = np.uint64(0xFFFFFFFF)
F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------- arithmetic of the oracle
def philox4x32_10(ctr, key):
  """Philox4x32-10 (Salmon et al., SC'11): ctr = four uint64 arrays holding 32-bit words, key = two words -> four arrays of words"""
  c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in ctr)
  k0, k1 = np.uint64(key[0]), np.uint64(key[1])
  for _ in range(10):
    p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
  return c0, c1, c2, c3


@functools.lru_cache(None)
def math_host():
  return pm.load_host()


def quantile(k24):
  return pm.host_fill(math_host(), 'quantile', bits=np.ascontiguousarray(k24, np.uint32).reshape(-1)).reshape(np.shape(k24))


def exp_f32(x):
  x = np.ascontiguousarray(x, F32)
  return pm.host_fill(math_host(), 'exp', bits=x.view(np.uint32).reshape(-1)).reshape(x.shape)


def clip(x):
  """the contract's clip: two compare-and-selects, NaN -> -1"""
  x = np.asarray(x, F32)
  y = np.where(x > F32(-1), x, F32(-1))
  return np.where(y < F32(1), y, F32(1)).astype(F32)


def fmaf32(a, b, c):
  """fmaf on float32 arrays (finite, no overflow): a * b is exact in float64; TwoSum gives the sum's error, which decides the one case a second rounding gets
  wrong -- the float64 sum exactly half way between two float32"""
  p, c = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64), np.asarray(c, F32).astype(F64)
  s = p + c
  bb = s - p
  e = (p - (s - bb)) + (c - bb)
  f = s.astype(F32)
  d = s - f.astype(F64)
  nb = np.nextafter(f, np.where(d > 0, np.inf, -np.inf).astype(F32))
  tie = (d != 0) & ((f.astype(F64) + nb.astype(F64)) * 0.5 == s)
  return np.where(tie & (e != 0) & (np.sign(e) == np.sign(d)), nb, f).astype(F32)


def fmaf_exact(a, b, c):
  """one element, in rationals: the float32 nearest (ties to even) to a * b + c"""
  v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
  f = F32(float(v))                                        # (float(Fraction) is correctly rounded; the second rounding is repaired below)
  lo, hi = sorted((f, np.nextafter(f, F32(np.inf) if Fraction(float(f)) < v else F32(-np.inf))))
  dl, dh = v - Fraction(float(lo)), Fraction(float(hi)) - v
  if dl != dh:
    return lo if dl < dh else hi
  return lo if (int(lo.view(np.uint32)) & 1) == 0 else hi


# ---------------------------------------------------------------------------------------------------- the oracle
def candidates(cfg, K, H, j, sigma, nc, mean):
  """item 1-2 -> (act [K, H, n, 3], m [H, n, 3], tail: whether a draw took the quantile's tail branch (|q| > 0.425))"""
  n = int(cfg.n)
  m = clip(mean)
  k = np.arange(K, dtype=np.uint64)[:, None, None]
  t = np.arange(H, dtype=np.uint64)[None, :, None]
  g = ((np.arange(n, dtype=np.int64) + int(cfg.env_offset)) & 0xFFFFFFFF).astype(np.uint64)[None, None, :]
  shape = (K, H, n)
  ctr = (np.full(shape, PLAN_DRAW | j, np.uint64), np.broadcast_to(g, shape), np.broadcast_to((k << np.uint64(16)) | t, shape), np.full(shape, nc, np.uint64))
  words = philox4x32_10(ctr, (int(cfg.seed) & 0xFFFFFFFF, int(cfg.seed) >> 32))
  k24 = np.stack([(w >> np.uint64(8)).astype(np.uint32) for w in words[:3]], -1)
  eps = quantile(k24)
  sg = np.broadcast_to(np.asarray(sigma, F32), (3,)).reshape(1, 1, 1, 3)
  act = clip(fmaf32(np.broadcast_to(sg, eps.shape), eps, np.broadcast_to(m[None], eps.shape)))
  act[0] = m
  q = np.abs((2.0 * k24[1:] + 1.0) / 2.0**25 - 0.5)
  return act, m, q > 0.425


def weights(ret, inv_t):
  """item 4 and 7 on ret [K, n] -> (W int64 [K, n], beta [n], best_k int32 [n])"""
  fin = np.where(np.isnan(ret), -np.inf, ret)
  beta = fin.max(0)
  with np.errstate(invalid='ignore'):
    x = ((ret - beta[None]) * F64(inv_t)).astype(F32)
  w = exp_f32(np.where(np.isnan(x), F32(0), x)).astype(F64)
  W = np.where(np.isnan(x), 0, np.rint(w * 2.0**24)).astype(np.int64)
  bk = np.where(beta > -np.inf, (ret == beta[None]).argmax(0), 0).astype(np.int32)
  return W, beta, bk


def update(act, m, W):
  """item 5 in Python integers -> mean' [H, n, 3]"""
  D = np.rint((act - m[None]).astype(F64) * 2.0**20).astype(np.int64)                         # (act - m: one float32 subtraction)
  A = (W.astype(object)[:, None, :, None] * D.astype(object)).sum(0)
  S = W.astype(object).sum(0)
  assert max(abs(int(v)) for v in A.reshape(-1)) < 2**62
  out = m.copy()
  for i in range(m.shape[1]):
    if S[i] != 0:
      a = np.array([float(int(v)) for v in A[:, i].reshape(-1)], F64).reshape(A[:, i].shape)   # (float(int): round to nearest)
      out[:, i] = clip(m[:, i] + (a / (F64(float(S[i])) * 2.0**20)).astype(F32))
  return out


def update_fast(act, m, W):
  """the same in int64 (for K too large for Python objects; |A| < 2^62 by the contract's count)"""
  D = np.rint((act - m[None]).astype(F64) * 2.0**20).astype(np.int64)
  A = (W[:, None, :, None] * D).sum(0)
  S = W.sum(0)
  with np.errstate(invalid='ignore', divide='ignore'):
    new = clip(m + (A.astype(F64) / (S.astype(F64)[None, :, None] * 2.0**20)).astype(F32))
  return np.where((S != 0)[None, :, None], new, m)


def branch_returns(side, sc, act):
  res, b = tb.run_ok(side, sc, act, 0x00, null=('success_last', 'first_success', 'last_obs'))
  b.check('the oracle\'s branch rollout')
  return res['out.ret'].cpu().numpy()


def oracle(side, sc, mean, K, I, sigma, inv_t, nc, iteration0=0, fast=False, value=None):
  """-> the five outputs as host tensors under 'out.*', and 'iters': per iteration dict(act, m, ret, W, tail, ..) for the coverage conditions.  value (a
  tabletop_value_helpers.Value): the returns are its discounted sums of K existing rollouts plus the net on the last rows, not the branch launch's"""
  H, n = int(mean.shape[0]), sc.n
  cfg = sc.cfg()
  plan, ret0, iters = np.asarray(mean, F32), np.empty((I, n), F64), []
  for i in range(I):
    act, m, tail = candidates(cfg, K, H, iteration0 + i, sigma, nc, plan)
    more = dict(ret=branch_returns(side, sc, act)) if value is None else value.returns(side, sc, act)
    ret = more['ret']
    W, beta, bk = weights(ret, inv_t)
    plan = (update_fast if fast else update)(act, m, W)
    ret0[i] = ret[0]
    iters.append(dict(act=act, m=m, W=W, tail=tail, plan=plan, bk=bk, **more))
  out = {'out.plan': plan, 'out.ret': ret, 'out.ret0': ret0, 'out.best_ret': beta, 'out.best_k': bk}
  return {**{k: ta._t(v) for k, v in out.items()}, 'iters': iters}


# ---------------------------------------------------------------------------------------------------- one call
def params(K, H, I, sigma, inv_t, nc, iteration0=0):
  s = np.broadcast_to(np.asarray(sigma, F32), (3,))
  return _abi.PlanParams(K=K, H=H, iterations=I, iteration0=iteration0, sigma=(C.c_float * 3)(*[float(v) for v in s]), noise_counter=nc & 0xFFFFFFFF,
                         inv_temperature=float(inv_t))


def told(pp, tell):
  """pp with the fields of `tell` set: earl_plan_params as the call is TOLD them, the buffers keeping their sizes"""
  for k, v in (tell or {}).items():
    if k == 'sigma':
      pp.sigma = (C.c_float * 3)(*v)
    else:
      setattr(pp, k, v)
  return pp


def entry(side, sc, name, value, r):
  """-> (the entry point `name` of the scene's env -- its `_value` form when a value specification is given --, that form's extra argument as a tuple, what must
  stay alive until the call returns); the net's parameters go into r's banded buffer 'in.value'"""
  if value is None:
    return getattr(side.lib, ta._pfx(sc) + name), (), None
  pv, keep = value.block(r)
  return getattr(side.lib, ta._pfx(sc) + name + '_value'), (None if pv is None else C.byref(pv),), (pv, keep)


def run_plan(side, sc, mean, K, fill, I=1, sigma=0.3, inv_t=1.0, nc=7, iteration0=0, null=(), alias=False, n_call=None, cfg_over=None, mean_null=False,
             params_null=False, plan_ptr=None, tell=None, value=None):
  """one call -> (rc, results, Bands).  `alias`: plan is the mean's buffer (which then counts as the output 'plan').  tell: fields of earl_plan_params as the call
  is TOLD them, the buffers keeping their sizes; plan_ptr: the plan's address as a function of the mean's.  value: None = earl_tabletop[3]_plan_mppi; a
  tabletop_value_helpers.Value = earl_tabletop[3]_plan_mppi_value with its discount, net and the block as told"""
  n, H = sc.n, int(mean.shape[0])
  r = ta.Run(side, fill, null)
  st = r.state(sc)
  if alias:
    m = plan = r.put('out.plan', mean, n * 3)
  else:
    m = r.put('in.mean', mean, n * 3)
    plan = r.blank('out.plan', (H, n, 3), torch.float32, n * 3)
  r.blank('out.ret', (K, n), torch.float64, n)
  r.blank('out.ret0', (I, n), torch.float64, n)
  r.blank('out.best_ret', (n,), torch.float64, n)
  r.blank('out.best_k', (n,), torch.int32, n)
  pp = told(params(K, H, I, sigma, inv_t, nc, iteration0), tell)
  fn, pv, keep = entry(side, sc, 'plan_mppi', value, r)
  cfg = sc.cfg(**(cfg_over or {}))
  if n_call is not None:
    cfg.n = n_call
  pl = None if plan is None else plan.data_ptr()
  if plan_ptr is not None:
    pl = plan_ptr(m.data_ptr())
  rc = fn(C.byref(cfg), C.byref(st), None if params_null else C.byref(pp), *pv, None if mean_null else m.data_ptr(), pl, r.ptr('out.ret'), r.ptr('out.ret0'),
          r.ptr('out.best_ret'), r.ptr('out.best_k'), side.stream)
  side.sync()
  del keep
  return rc, {k: v[3].clone() for k, v in r.b.bufs.items() if k.startswith(('st.', 'out.'))}, r.b


def run_ok(side, sc, mean, K, fill, **kw):
  rc, res, b = run_plan(side, sc, mean, K, fill, **kw)
  _abi.check(rc, 'plan_mppi' if kw.get('value') is None else 'plan_mppi_value', side.lib)
  return res, b


def run_candidates(side, sc, mean, K, fill, j=0, sigma=0.3, nc=7, n_call=None, mean_null=False, out_null=False, params_null=False, cfg_null=False, tell=None):
  n, H = sc.n, int(mean.shape[0])
  r = ta.Run(side, fill)
  m = r.put('in.mean', mean, n * 3)
  a = r.blank('out.act', (K, H, n, 3), torch.float32, n * 3)
  pp = told(params(K, H, 1, sigma, 1.0, nc), tell)
  cfg = sc.cfg()
  if n_call is not None:
    cfg.n = n_call
  rc = side.lib.earl_tabletop_plan_candidates(None if cfg_null else C.byref(cfg), None if params_null else C.byref(pp), j, None if mean_null else m.data_ptr(),
                                              None if out_null else a.data_ptr(), side.stream)
  side.sync()
  return rc, {k: v[3].clone() for k, v in r.b.bufs.items() if k.startswith('out.')}, r.b


def compare(got, ref, what, names=OUTS):
  for k in names:
    ta.same(got['out.' + k].cpu(), ref['out.' + k].cpu(), f'{what}: {k}')


# ---------------------------------------------------------------------------------------------------- cases
class PlanCase:
  """scene, mean and parameters of one call, made once and never written.  The mean reaches beyond the action box (item 1 clips it) and close to its faces
  (item 2 clips candidates)"""

  def __init__(self, nobj=1, rt='sparse', n=70, K=5, H=9, I=2, general=False, sigma=(0.5, 0.5, 0.8), inv_t=None, nc=0x9E3779B9, iteration0=0, seed=2):
    self.nobj, self.rt, self.n, self.K, self.H, self.I, self.general = nobj, rt, n, K, H, I, general
    self.sc = tb.case(nobj, rt, n=n, K=1, H=1, general=general).sc
    self.mean = np.random.default_rng(seed).uniform(-1.15, 1.15, (H, n, 3)).astype(F32)
    # a small temperature under the dense reward: the weights of poor branches underflow to W_k = 0; under the sparse one returns are small integers
    self.kw = dict(I=I, sigma=sigma, inv_t=(1.0 if rt == 'sparse' else 40.0) if inv_t is None else inv_t, nc=nc, iteration0=iteration0)
    self.what = f'plan nobj={nobj} {rt} n={n} K={K} H={H} I={I}' + (' general' if general else '')


@functools.lru_cache(None)
def case(*args, **kw):
  return PlanCase(*args, **kw)


_REF = {}


def reference(cs, side, key=None, sc=None, mean=None, K=None, value=None, fast=False, **over):
  """the oracle of the case, made once per (case or key, value specification, side); the entry keeps the specification's net alive, so that its id stays its own"""
  key = (id(cs) if key is None else key, None if value is None else value.key, side.device)
  if key not in _REF:
    kw = {**cs.kw, **over}
    _REF[key] = (value, oracle(side, cs.sc if sc is None else sc, cs.mean if mean is None else mean, cs.K if K is None else K, kw['I'], kw['sigma'], kw['inv_t'], kw['nc'],
                               kw['iteration0'], fast=fast, value=value))
  return _REF[key][1]


def check_coverage(cs, ref):
  """the core case's conditions, on the oracle, before anything is compared"""
  its = ref['iters']
  ret, plan, m, act, W = (its[0][k] for k in ('ret', 'plan', 'm', 'act', 'W'))
  differ = ret.min(0) != ret.max(0)
  assert bool((differ & (plan != m).any((0, 2))).any()), 'no env whose returns differ across branches and whose plan changes'
  if cs.rt == 'sparse':                                    # (the dense reward is continuous in the positions: distinct candidates never score alike)
    eq = np.nonzero(~differ)[0]
    assert len(eq), 'no env whose returns are all equal'
    assert bool((W[:, eq] == 2**24).all()) and bool((plan[:, eq] != m[:, eq]).any()), 'equal returns: equal weights, the plan moves by the plain noise average'
  assert bool((np.abs(act[1:]) == 1).any()) and bool((np.abs(cs.mean) > 1).any()), 'no candidate component clipped at +-1'
  assert bool(any(it['tail'].any() for it in its)) and bool(any((~it['tail']).any() for it in its)), 'the quantile took one branch only'
  if cs.rt == 'dense':
    assert bool(any((it['W'] == 0).any() for it in its)), 'no W_k == 0 under the dense reward'
  assert not np.array_equal(its[-1]['plan'], its[0]['plan']), 'the second iteration changes nothing'


def state_untouched(res, sc, what):
  tb.state_untouched(res, sc, what)


def check_case(side, cs, key=None, sc=None, mean=None, K=None, alias=False, value=None, fast=False, nan_returns=False, **over):
  """both fills: bands intact, every output overwritten; the state untouched; every output equal to the oracle, bit for bit.  nan_returns: the case has NaN returns,
  whose sign and payload the contract leaves open (the oracle's are numpy's, the device's its own): ret and ret0 are NaN in the same places and equal elsewhere"""
  sc, mean, K = cs.sc if sc is None else sc, cs.mean if mean is None else mean, cs.K if K is None else K
  ref = reference(cs, side, key, sc, mean, K, value, fast, **over)
  what = cs.what if value is None else f'{cs.what} {value.what}'
  res = ta.both_fills(run_ok, side, sc, mean, K, what=what, alias=alias, value=value, **{**cs.kw, **over})
  state_untouched(res, sc, what)
  if nan_returns:
    compare(res, ref, what, ['plan', 'best_ret', 'best_k'])
    for k in ('ret', 'ret0'):
      ta.same(res['out.' + k].cpu(), ref['out.' + k].cpu(), f'{what}: {k}', atol=0.0)
  else:
    compare(res, ref, what)
  return res


def check_pointers(side, cs, full):
  """each optional pointer NULL in turn, the in-place call, ret NULL refused"""
  for name in OPTIONAL:
    res = ta.both_fills(run_ok, side, cs.sc, cs.mean, cs.K, what=f'{cs.what} without {name}', null=(name,), **cs.kw)
    assert 'out.' + name not in res
    state_untouched(res, cs.sc, cs.what)
    compare(res, full, f'{cs.what} without {name}', [k for k in OUTS if k != name])
  res = ta.both_fills(run_ok, side, cs.sc, cs.mean, cs.K, what=f'{cs.what} in place', alias=True, **cs.kw)
  state_untouched(res, cs.sc, cs.what)
  compare(res, full, f'{cs.what} in place')
  rc, res, b = run_plan(side, cs.sc, cs.mean, cs.K, 0xFF, null=('ret',), **cs.kw)
  assert rc == -1 and side.lib.earl_last_error()
  b.check('ret NULL')
  ta.assert_untouched(res, cs.sc, 'ret NULL')


def check_chaining(side, cs, I=3):
  """I iterations in one call == I calls of one, numbered on, each fed the previous plan (in place); 256 is the last iteration index"""
  kw = {**cs.kw, 'I': I}
  whole, b = run_ok(side, cs.sc, cs.mean, cs.K, 0x00, **kw)
  b.check('chaining, one call')
  plan, ret0 = cs.mean, []
  for j in range(I):
    one, b = run_ok(side, cs.sc, plan, cs.K, 0xFF, **{**kw, 'I': 1, 'iteration0': j})
    b.check(f'chaining, call {j}')
    plan = one['out.plan'].cpu().numpy()
    ret0.append(one['out.ret0'].cpu())
  compare(one, whole, 'chained calls vs one call', ['plan', 'ret', 'best_ret', 'best_k'])
  ta.same(torch.cat(ret0), whole['out.ret0'].cpu(), 'chained calls vs one call: ret0')
  compare(whole, oracle(side, cs.sc, cs.mean, cs.K, I, kw['sigma'], kw['inv_t'], kw['nc']), 'three iterations vs the oracle')
  top, b = run_ok(side, cs.sc, cs.mean, cs.K, 0x00, **{**kw, 'I': 2, 'iteration0': 254})
  b.check('iterations 254, 255')
  compare(top, oracle(side, cs.sc, cs.mean, cs.K, 2, kw['sigma'], kw['inv_t'], kw['nc'], iteration0=254), 'iterations 254, 255 vs the oracle')
  rc, res, b = run_plan(side, cs.sc, cs.mean, cs.K, 0xFF, **{**kw, 'I': 2, 'iteration0': 255})
  assert rc == -1
  ta.assert_untouched(res, cs.sc, 'iteration0 + iterations = 257')


def check_candidates(side, cs):
  """the entry point == the oracle's candidates; branch 0 == the clipped mean; sigma = 0: every branch the clipped mean, and plan == clip(mean)"""
  cfg, kw = cs.sc.cfg(), cs.kw
  for j in (0, 1, 255):
    want, m, _ = candidates(cfg, cs.K, cs.H, j, np.broadcast_to(np.asarray(kw['sigma'], F32), (3,)), kw['nc'], cs.mean)
    for fill in ta.FILLS:
      rc, res, b = run_candidates(side, cs.sc, cs.mean, cs.K, fill, j=j, sigma=kw['sigma'], nc=kw['nc'])
      assert rc == 0
      b.check(f'candidates j={j}')
      ta.same(res['out.act'].cpu(), ta._t(want), f'{cs.what}: candidates of iteration {j}')
    ta.same(res['out.act'][0].cpu(), ta._t(clip(cs.mean)), 'branch 0 is the clipped mean')
    assert j == 0 or not np.array_equal(want, first)
    first = want if j == 0 else first
  rc, res, b = run_candidates(side, cs.sc, cs.mean, cs.K, 0x00, sigma=0.0, nc=kw['nc'])
  assert rc == 0
  ta.same(res['out.act'].cpu(), ta._t(np.broadcast_to(clip(cs.mean), (cs.K,) + cs.mean.shape).copy()), 'sigma = 0: every branch is the clipped mean')
  got, b = run_ok(side, cs.sc, cs.mean, cs.K, 0x00, **{**kw, 'sigma': 0.0})
  ta.same(got['out.plan'].cpu(), ta._t(clip(cs.mean)), 'sigma = 0: plan == clip(mean)')
  ret = got['out.ret'].cpu().numpy()
  assert np.array_equal(ret, np.broadcast_to(ret[:1], ret.shape)) and bool((got['out.best_k'] == 0).all())


def check_edges(side, nobj, rt='sparse'):
  """K = 1; H = 1; n = 1, 64, 65; a different noise_counter changes the candidates, the same one repeats them"""
  base = case(nobj, rt)
  one = check_case(side, base, key=('K=1', nobj, rt), K=1)
  ta.same(one['out.plan'].cpu(), ta._t(clip(base.mean)), 'K = 1: plan == clip(mean)')
  assert bool((one['out.best_k'] == 0).all())
  check_case(side, case(nobj, rt, H=1))
  for n in (1, 64, 65):
    check_case(side, case(nobj, rt, n=n, K=3, H=2, I=1))
  a = check_case(side, base)
  b_ = check_case(side, base, key=('nc + 1', nobj, rt), nc=base.kw['nc'] + 1)
  assert not torch.equal(a['out.plan'], b_['out.plan']), 'another noise_counter, the same plan'


def check_shards(side, nobj, rt='sparse'):
  """two shards (0..40, 40..70, env_offset moving with them) == the batch: the draws follow the global env id"""
  cs = case(nobj, rt, general=True)
  full = check_case(side, cs)
  for lo, hi in ((0, 40), (40, 70)):
    part, b = run_ok(side, tb.shard(cs.sc, lo, hi), np.ascontiguousarray(cs.mean[:, lo:hi]), cs.K, 0x00, **cs.kw)
    b.check(f'shard {lo}..{hi}')
    for k in OUTS:
      whole = full['out.' + k]
      ta.same(part['out.' + k].cpu(), (whole[:, lo:hi] if whole.dim() > 1 else whole[lo:hi]).cpu().contiguous(), f'shard {lo}..{hi}: {k}')


def check_nonfinite(side, nobj=1):
  """item 7 as the header states it: a NaN / infinite mean is clipped to -1 / +-1 (the oracle's clip does the same: outputs equal, all finite); an env whose state
  holds a NaN has, under the dense reward, NaN returns throughout: no weights, plan = clip(mean), best_ret = -Inf, best_k = 0 -- and its neighbours are as ever"""
  cs = case(nobj, 'dense')
  mean = cs.mean.copy()
  mean[0, 3, 0], mean[1, 5, 1], mean[2, 7, 2], mean[3, 66, 0] = np.nan, np.inf, -np.inf, np.nan
  res = check_case(side, cs, key=('non-finite mean', nobj), mean=mean)
  assert bool(torch.isfinite(res['out.plan']).all()) and bool(torch.isfinite(res['out.ret']).all())
  sc = tb.with_cfg(cs.sc)
  sc.state = {k: v.copy() for k, v in cs.sc.state.items()}
  sc.state['qpos'][9, 2] = np.nan
  ref = reference(cs, side, key=('NaN state', nobj), sc=sc)
  assert bool(torch.isnan(ref['out.ret'][:, 9]).all()), 'the NaN of the state does not reach the returns'
  res = check_case(side, cs, key=('NaN state', nobj), sc=sc)
  assert bool((res['out.best_ret'][9] == -np.inf)) and int(res['out.best_k'][9]) == 0
  ta.same(res['out.plan'][:, 9].cpu(), ta._t(ref['iters'][-1]['m'][:, 9]), 'no weights: the plan is the clipped mean')


def check_device_vs_host(cs, dev, host):
  """sparse: every output of the case bit for bit.  dense: ONE iteration (after it the two plans, and with them the candidates, may differ), ret, ret0 and best_ret
  within 1e-6 * sum_t |r_t| -- the branch launch's bound, the sums from the twin's own rollouts of the candidates -- and the plan not compared"""
  kw = cs.kw if cs.rt == 'sparse' else {**cs.kw, 'I': 1}
  d, b = run_ok(dev, cs.sc, cs.mean, cs.K, 0x00, **kw)
  b.check(cs.what + ' device')
  h, b = run_ok(host, cs.sc, cs.mean, cs.K, 0x00, **kw)
  b.check(cs.what + ' host')
  if cs.rt == 'sparse':
    return compare(d, h, cs.what + ' device vs host')
  act = candidates(cs.sc.cfg(), cs.K, cs.H, kw['iteration0'], np.broadcast_to(np.asarray(kw['sigma'], F32), (3,)), kw['nc'], cs.mean)[0]
  bound = tb.DENSE_REL * tb.reference(cs, host, cs.sc, act, key=(id(cs), 'sum |r|'))['abs']
  for name, bnd in (('ret', bound), ('ret0', bound[:1]), ('best_ret', bound.max(0))):
    err = (d['out.' + name].cpu() - h['out.' + name].cpu()).abs().numpy()
    print(f'{cs.what}: {name}: max |d| = {err.max():.3e}, min bound = {bnd.min():.3e}, max ratio = {(err / bnd).max():.3e}')
    assert bool((err <= bnd).all()), f'{cs.what}: |d {name}| up to {err.max()} beyond 1e-6 * sum |r|'


# ---------------------------------------------------------------------------------------------------- refusals and empty work
def refusals(cs):
  nan, inf = float('nan'), float('inf')
  out = [('n < 0', dict(n_call=-1)), ('reward_type', dict(cfg_over=dict(reward_type=7))), ('qpos NULL', dict(null=('qpos',))), ('params NULL', dict(params_null=True)),
         ('mean NULL', dict(mean_null=True)), ('plan NULL', dict(null=('plan',))), ('ret NULL', dict(null=('ret',))), ('K = 0', dict(tell=dict(K=0))), ('K < 0', dict(tell=dict(K=-1))),
         ('K = 65537', dict(tell=dict(K=65537))), ('H = 0', dict(tell=dict(H=0))), ('H = 65537', dict(tell=dict(H=65537))), ('iterations = 0', dict(tell=dict(iterations=0))),
         ('iteration0 < 0', dict(tell=dict(iteration0=-1))), ('iteration0 + iterations = 257', dict(tell=dict(iteration0=250, iterations=7))),
         ('iterations overflow', dict(tell=dict(iteration0=2**31 - 1, iterations=2**31 - 1))), ('sigma < 0', dict(tell=dict(sigma=(0.1, -0.1, 0.1)))),
         ('sigma NaN', dict(tell=dict(sigma=(0.1, 0.1, nan)))), ('sigma Inf', dict(tell=dict(sigma=(inf, 0.1, 0.1)))), ('inv_temperature 0', dict(tell=dict(inv_temperature=0.0))),
         ('inv_temperature < 0', dict(tell=dict(inv_temperature=-1.0))), ('inv_temperature NaN', dict(tell=dict(inv_temperature=nan))), ('inv_temperature Inf', dict(tell=dict(inv_temperature=inf))),
         ('plan overlaps mean from above', dict(plan_ptr=lambda m: m + 12)), ('plan overlaps mean from below', dict(plan_ptr=lambda m: m - 12))]
  if cs.nobj == 1:
    out.append(('lifelong arrays NULL', dict(cfg_over=dict(goal_change_frequency=3), null=ta.LIFELONG_STATE)))
  else:
    out += [('3 objects: wide_init', dict(cfg_over=dict(wide_init=1))), ('3 objects: lifelong', dict(cfg_over=dict(goal_change_frequency=3)))]
  return out


def check_refusals(side, cs):
  for what, kw in refusals(cs):
    rc, res, b = run_plan(side, cs.sc, cs.mean, cs.K, 0xFF, **{**cs.kw, **kw})
    assert rc == -1, f'{cs.what} {what}: rc = {rc}'
    assert side.lib.earl_last_error(), what
    b.check(f'{cs.what} {what}')
    ta.assert_untouched(res, cs.sc, f'{cs.what} {what}')
  big = ta.Scene(2, nobj=cs.nobj)                             # grids: told n, nothing that large allocated
  for what, n_call, told in (('2^32 lanes in the score launch', 2**26, dict(K=64)), ('2^32 lanes in the update launch', 2**27, dict(H=32))):
    rc, res, b = run_plan(side, big, np.zeros((1, 2, 3), F32), 1, 0xFF, n_call=n_call, tell=told)
    assert rc == -1 and b'launch' in side.lib.earl_last_error(), what
    ta.assert_untouched(res, big, what)
  for fn in ('earl_tabletop_plan_mppi', 'earl_tabletop3_plan_mppi'):
    assert getattr(side.lib, fn)(None, None, None, None, None, None, None, None, None, side.stream) == -1
  for what, kw in (('cfg NULL', dict(cfg_null=True)), ('params NULL', dict(params_null=True)), ('mean NULL', dict(mean_null=True)), ('act_out NULL', dict(out_null=True)),
                   ('n < 0', dict(n_call=-1)), ('j < 0', dict(j=-1)), ('j = 256', dict(j=256)), ('K = 0', dict(tell=dict(K=0))), ('H = 65537', dict(tell=dict(H=65537))),
                   ('sigma NaN', dict(tell=dict(sigma=(float('nan'), 0.0, 0.0)))), ('grid', dict(n_call=2**26, tell=dict(K=64)))):
    rc, res, b = run_candidates(side, cs.sc, cs.mean, cs.K, 0xFF, **kw)
    assert rc == -1, f'candidates {what}: rc = {rc}'
    b.check('candidates ' + what)
    ta.assert_untouched(res, cs.sc, 'candidates ' + what)


def check_empty(side, cs):
  """n == 0: EARL_OK, nothing written"""
  for fill in ta.FILLS:
    rc, res, b = run_plan(side, cs.sc, cs.mean, cs.K, fill, n_call=0, **cs.kw)
    assert rc == 0
    b.check('plan n = 0')
    ta.assert_untouched(res, cs.sc, 'plan n = 0')
    rc, res, b = run_candidates(side, cs.sc, cs.mean, cs.K, fill, n_call=0)
    assert rc == 0
    b.check('candidates n = 0')
    ta.assert_untouched(res, cs.sc, 'candidates n = 0')


# ---------------------------------------------------------------------------------------------------- through Python
def check_python(env, K=4, H=9, I=2, seed=3):
  """plan_mppi leaves the env as found; the plan it returns, fed to rollout_branches as [1, H, N, 3], gives the ret0 a further iteration reports; plan_candidates[best_k]
  scores best_ret; the `out=` rules"""
  u = env.unwrapped
  n, dev = u.num_envs, u.device
  mean = torch.from_numpy(np.random.default_rng(seed).uniform(-1.1, 1.1, (H, n, 3)).astype(F32)).to(dev)
  before, steps = tb.snapshot(env), u.total_step_count
  got = env.plan_mppi(mean, K=K, iterations=I, sigma=(0.5, 0.5, 0.8), temperature=0.5)
  tb.assert_env_as_found(env, before, 'plan_mppi')
  assert u.total_step_count == steps
  assert {k: (tuple(v.shape), v.dtype) for k, v in got.items()} == {'plan': ((H, n, 3), torch.float32), 'ret': ((K, n), torch.float64), 'ret0': ((I, n), torch.float64),
                                                                    'best_ret': ((n,), torch.float64), 'best_k': ((n,), torch.int32)}
  nxt = env.plan_mppi(got['plan'], K=K, iterations=1, iteration0=I, sigma=(0.5, 0.5, 0.8), temperature=0.5)
  scored = env.rollout_branches(got['plan'][None], last_obs=False)['ret']
  ta.same(scored[0].cpu(), nxt['ret0'][0].cpu(), 'rollout_branches(plan) vs the ret0 of a further iteration')
  cand = env.plan_candidates(got['plan'], K, sigma=(0.5, 0.5, 0.8), iteration=I)
  ta.same(env.rollout_branches(cand, last_obs=False)['ret'].cpu(), nxt['ret'].cpu(), 'rollout_branches(plan_candidates) vs ret')
  pick = cand[nxt['best_k'].long(), :, torch.arange(n, device=dev)].permute(1, 0, 2).contiguous()
  ta.same(env.rollout_branches(pick[None], last_obs=False)['ret'][0].cpu(), nxt['best_ret'].cpu(), 'candidate best_k scores best_ret')
  tb.assert_env_as_found(env, before, 'plan_candidates / rollout_branches')
  # out=: in place on the mean; a missing key is not computed; a wrong one is refused
  buf = mean.clone()
  res = env.plan_mppi(buf, K=K, iterations=I, sigma=(0.5, 0.5, 0.8), temperature=0.5, out={'plan': buf, 'best_k': None})
  assert set(res) == {'plan', 'ret'} and res['plan'] is buf
  ta.same(buf.cpu(), got['plan'].cpu(), 'in place through Python')
  zeros = env.plan_mppi(horizon=H, K=K, sigma=0.0)
  assert bool((zeros['plan'] == 0).all())
  for bad in ({'plan': buf[:, :, :2]}, {'plan': buf, 'ret': torch.empty(K, n, device=dev)}, {'plan': buf, 'nope': buf}, {'ret0': torch.empty(I, n, dtype=torch.float64, device=dev)}):
    try:
      env.plan_mppi(mean, K=K, iterations=I, out=bad)
    except ValueError:
      continue
    raise AssertionError(f'out = {list(bad)} was accepted')
  return {k: v.cpu() for k, v in got.items()}

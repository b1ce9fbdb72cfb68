"""Drivers and the oracle of earl_tabletop[3]_plan_cem / earl_tabletop_cem_candidates / earl_tabletop[3]_mpc_rollout_cem (include/earl_tabletop.h, "CEM planning") for
tests/test_tabletop_cem*.py; a plain module on tests/tabletop_abi.py's banded buffers, tests/tabletop_branch_helpers.py's scenes and the arithmetic of
tests/tabletop_plan_helpers.py (numpy Philox, the policy-math host build's quantile, the exact fmaf), none of which it changes.

THE ORACLE uses none of the new code:
  candidates   the numpy Philox with word 0 = 0x43454D00 | j, normal_quantile_f32 of the policy-math host build, fmaf32 (exact), with the per-row clamped std
  returns      the SAME library's existing earl_tabletop[3]_branch_rollout fed with those candidates (on the device: the device's own); for the value variant the
               existing rollouts, earl_mlp_policy_forward_cpu and the discounted numpy sum of tests/tabletop_value_helpers.py
  elites       a Python sort of each env's branches on the key (is-NaN, -ret, k); the first E that are not NaN
  update       Python integers for D, A1, A2 and V; numpy float32 / float64 for the rest (a float32 np.sqrt is correctly rounded)
Every output is compared bit for bit, under both rewards.  Device against host twin: bit for bit under the sparse reward; under the dense one ret, ret0 and best_ret
within 1e-6 * sum_t |r_t| (one iteration) and the plans not compared -- the bound the header states for the MPPI twins.
THE MPC REFERENCE is the composition the header defines: per real step earl_tabletop[3]_plan_cem with std0 = NULL at counter c0 + s and noise_counter + s, the
library's one-step rollout on the plan's first row, the shift in numpy (tests/tabletop_mpc_helpers.py's).
"""
import ctypes as C
import functools

import numpy as np
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_mpc_helpers as mh
import tabletop_plan_helpers as h
from earl_benchmark_amd import _abi

F32, F64 = np.float32, np.float64
CEM_DRAW = 0x43454D00
OUTS = ('plan', 'std', 'ret', 'ret0', 'best_ret', 'best_k')
OPTIONAL = ('ret0', 'best_ret', 'best_k')


# ---------------------------------------------------------------------------------------------------- the oracle
def sclamp(x, lo, hi):
  """item 1: two compare-and-selects, NaN -> std_min"""
  x = np.asarray(x, F32)
  y = np.where(x > F32(lo), x, F32(lo))
  return np.where(y < F32(hi), y, F32(hi)).astype(F32)


def sigma3(sigma):
  return np.broadcast_to(np.asarray(sigma, F32), (3,)).copy()


def candidates(cfg, K, H, j, nc, mean, s):
  """items 1-2 with the clamped std s [H, n, 3] -> (act [K, H, n, 3], m [H, n, 3])"""
  n = int(cfg.n)
  m = h.clip(mean)
  k = np.arange(K, dtype=np.uint64)[:, None, None]
  t = np.arange(H, dtype=np.uint64)[None, :, None]
  g = ((np.arange(n, dtype=np.int64) + int(cfg.env_offset)) & 0xFFFFFFFF).astype(np.uint64)[None, None, :]
  shape = (K, H, n)
  ctr = (np.full(shape, CEM_DRAW | j, np.uint64), np.broadcast_to(g, shape), np.broadcast_to((k << np.uint64(16)) | t, shape), np.full(shape, nc & 0xFFFFFFFF, np.uint64))
  words = h.philox4x32_10(ctr, (int(cfg.seed) & 0xFFFFFFFF, int(cfg.seed) >> 32))
  eps = h.quantile(np.stack([(w >> np.uint64(8)).astype(np.uint32) for w in words[:3]], -1))
  act = h.clip(h.fmaf32(np.broadcast_to(s[None], eps.shape), eps, np.broadcast_to(m[None], eps.shape)))
  act[0] = m
  return act, m


def elites(ret, E):
  """item 4 on ret [K, n] -> per env the list of elite branches, best first"""
  out = []
  for i in range(ret.shape[1]):
    order = sorted(range(ret.shape[0]), key=lambda k: (bool(np.isnan(ret[k, i])), -float(ret[k, i]) if not np.isnan(ret[k, i]) else 0.0, k))
    out.append([k for k in order[:E] if not np.isnan(ret[k, i])])
  return out


def update(act, m, s, el, alpha, lo, hi):
  """item 5 in Python integers -> (mean' [H, n, 3], std' [H, n, 3], e_std [H, n, 3] (NaN where Ne == 0))"""
  D = np.rint((act - m[None]).astype(F64) * 2.0**20).astype(np.int64).astype(object)          # (act - m: one float32 subtraction)
  mean2, std2, es = m.copy(), s.copy(), np.full(m.shape, np.nan, F32)
  for i, ks in enumerate(el):
    Ne = len(ks)
    if Ne == 0:
      continue
    A1 = sum(D[k, :, i] for k in ks)
    A2 = sum(D[k, :, i] * D[k, :, i] for k in ks)
    V = Ne * A2 - A1 * A1
    assert all(0 <= int(v) < 2**63 for v in V.reshape(-1)) and all(int(v) < 2**52 for v in A2.reshape(-1))
    f = lambda a: np.array([float(int(v)) for v in a.reshape(-1)], F64).reshape(a.shape)      # (float(int): round to nearest)
    e_mean = m[:, i] + (f(A1) / (F64(Ne) * 2.0**20)).astype(F32)
    e_std = np.sqrt((f(V) / (F64(Ne) * F64(Ne) * 2.0**40)).astype(F32))
    a = np.full(e_mean.shape, alpha, F32)
    mean2[:, i] = h.clip(h.fmaf32(a, m[:, i] - e_mean, e_mean))
    std2[:, i] = sclamp(h.fmaf32(a, s[:, i] - e_std, e_std), lo, hi)
    es[:, i] = e_std
  return mean2, std2, es


def oracle(side, sc, mean, std0, K, I, E, sigma, alpha, lo, hi, nc, iteration0=0, value=None):
  """-> the six outputs as host tensors under 'out.*', and 'iters': per iteration dict(act, m, s, ret, el, e_std, plan, std) for the coverage conditions"""
  H, n = int(mean.shape[0]), sc.n
  cfg = sc.cfg()
  plan, ret0, iters = np.asarray(mean, F32), np.empty((I, n), F64), []
  std = np.broadcast_to(sigma3(sigma), (H, n, 3)) if std0 is None else np.asarray(std0, F32)
  for i in range(I):
    s = sclamp(std, lo, hi)
    act, m = candidates(cfg, K, H, iteration0 + i, nc, plan, s)
    ret = h.branch_returns(side, sc, act) if value is None else value.returns(side, sc, act)['ret']
    el = elites(ret, E)
    plan, std, es = update(act, m, s, el, alpha, lo, hi)
    ret0[i] = ret[0]
    iters.append(dict(act=act, m=m, s=s, ret=ret, el=el, e_std=es, plan=plan, std=std))
  _, beta, bk = h.weights(ret, 1.0)
  out = {'out.plan': plan, 'out.std': std, 'out.ret': ret, 'out.ret0': ret0, 'out.best_ret': beta, 'out.best_k': bk}
  return {**{k: ta._t(v) for k, v in out.items()}, 'iters': iters}


# ---------------------------------------------------------------------------------------------------- one call
def params(K, H, I, E, sigma, alpha, lo, hi, nc, iteration0=0):
  return _abi.CemParams(K=K, H=H, iterations=I, iteration0=iteration0, elites=E, sigma=(C.c_float * 3)(*[float(v) for v in sigma3(sigma)]), noise_counter=nc & 0xFFFFFFFF,
                        alpha=float(alpha), std_min=float(lo), std_max=float(hi))


def value_block(value, r):
  if value is None:
    return None, None
  pv, keep = value.block(r)
  return (None if pv is None else C.byref(pv)), (pv, keep)


def run_cem(side, sc, mean, std0, K, fill, I=1, E=2, sigma=0.3, alpha=0.0, lo=0.0, hi=2.0, nc=7, iteration0=0, null=(), alias=False, n_call=None, cfg_over=None,
            mean_null=False, params_null=False, ptrs=None, tell=None, value=None):
  """one call -> (rc, results, Bands).  std0 None: NULL.  alias: plan is the mean's buffer and std the std0's (which then count as the outputs).  tell: fields of
  earl_cem_params as the call is TOLD them; ptrs: dict(plan= / std= / std0=: the address as a function of the dict of the four real addresses)"""
  n, H = sc.n, int(mean.shape[0])
  r = ta.Run(side, fill, null)
  st = r.state(sc)
  if alias:
    m = plan = r.put('out.plan', mean, n * 3)
    s0 = std = r.put('out.std', std0, n * 3)
  else:
    m = r.put('in.mean', mean, n * 3)
    s0 = None if std0 is None else r.put('in.std0', std0, n * 3)
    plan = r.blank('out.plan', (H, n, 3), torch.float32, n * 3)
    std = r.blank('out.std', (H, n, 3), torch.float32, n * 3)
  r.blank('out.ret', (K, n), torch.float64, n)
  r.blank('out.ret0', (I, n), torch.float64, n)
  r.blank('out.best_ret', (n,), torch.float64, n)
  r.blank('out.best_k', (n,), torch.int32, n)
  cp = h.told(params(K, H, I, E, sigma, alpha, lo, hi, nc, iteration0), tell)
  pv, keep = value_block(value, r)
  cfg = sc.cfg(**(cfg_over or {}))
  if n_call is not None:
    cfg.n = n_call
  p = lambda t: None if t is None else t.data_ptr()
  addr = dict(mean=p(m), std0=p(s0), plan=p(plan), std=p(std))
  for k, f in (ptrs or {}).items():
    addr[k] = f(addr)
  fn = getattr(side.lib, ta._pfx(sc) + 'plan_cem')
  rc = fn(C.byref(cfg), C.byref(st), None if params_null else C.byref(cp), pv, None if mean_null else addr['mean'], addr['std0'], addr['plan'], addr['std'],
          r.ptr('out.ret'), r.ptr('out.ret0'), r.ptr('out.best_ret'), r.ptr('out.best_k'), side.stream)
  side.sync()
  del keep
  return rc, {k: v[3].clone() for k, v in r.b.bufs.items() if k.startswith(('st.', 'out.'))}, r.b


def run_ok(side, sc, mean, std0, K, fill, **kw):
  rc, res, b = run_cem(side, sc, mean, std0, K, fill, **kw)
  _abi.check(rc, 'plan_cem', side.lib)
  return res, b


def run_candidates(side, sc, mean, std, K, fill, j=0, sigma=0.3, lo=0.0, hi=2.0, nc=7, n_call=None, mean_null=False, out_null=False, params_null=False, cfg_null=False,
                   tell=None):
  n, H = sc.n, int(mean.shape[0])
  r = ta.Run(side, fill)
  m = r.put('in.mean', mean, n * 3)
  s = None if std is None else r.put('in.std', std, n * 3)
  a = r.blank('out.act', (K, H, n, 3), torch.float32, n * 3)
  cp = h.told(params(K, H, 1, 1, sigma, 0.0, lo, hi, nc), tell)
  cfg = sc.cfg()
  if n_call is not None:
    cfg.n = n_call
  rc = side.lib.earl_tabletop_cem_candidates(None if cfg_null else C.byref(cfg), None if params_null else C.byref(cp), j, None if mean_null else m.data_ptr(),
                                             None if s is None else s.data_ptr(), None if out_null else a.data_ptr(), side.stream)
  side.sync()
  return rc, {k: v[3].clone() for k, v in r.b.bufs.items() if k.startswith('out.')}, r.b


def compare(got, ref, what, names=OUTS):
  for k in names:
    ta.same(got['out.' + k].cpu(), ref['out.' + k].cpu(), f'{what}: {k}')


# ---------------------------------------------------------------------------------------------------- cases
class CemCase:
  """scene, mean, std0 and parameters of one call, made once and never written.  The mean reaches beyond the action box; std0 reaches below std_min and above
  std_max.  seed / nc: chosen on the host twin so that the ORACLE meets check_coverage (the conditions are the oracle's, not the code's)"""

  def __init__(self, nobj=1, rt='sparse', n=70, K=5, H=9, I=2, E=2, general=False, sigma=(0.5, 0.5, 0.8), alpha=0.25, lo=0.05, hi=0.6, nc=0x9E3779B9, iteration0=0, seed=2,
               std0=True):
    self.nobj, self.rt, self.n, self.K, self.H, self.I, self.E, self.general = nobj, rt, n, K, H, I, E, general
    self.sc = tb.case(nobj, rt, n=n, K=1, H=1, general=general).sc
    rng = np.random.default_rng(seed)
    self.mean = rng.uniform(-1.15, 1.15, (H, n, 3)).astype(F32)
    self.std0 = rng.uniform(0.0, 0.8, (H, n, 3)).astype(F32) if std0 else None
    self.kw = dict(I=I, E=E, sigma=sigma, alpha=alpha, lo=lo, hi=hi, nc=nc, iteration0=iteration0)
    self.what = f'cem nobj={nobj} {rt} n={n} K={K} H={H} I={I} E={E}' + (' general' if general else '') + ('' if std0 else ' std0=NULL')


@functools.lru_cache(None)
def case(*args, **kw):
  return CemCase(*args, **kw)


_REF = {}


def reference(cs, side, key=None, sc=None, mean=None, std0='case', K=None, value=None, **over):
  key = (id(cs) if key is None else key, None if value is None else value.key, side.device)
  if key not in _REF:
    kw = {**cs.kw, **over}
    _REF[key] = (value, oracle(side, cs.sc if sc is None else sc, cs.mean if mean is None else mean, cs.std0 if isinstance(std0, str) else std0, cs.K if K is None else K,
                               kw['I'], kw['E'], kw['sigma'], kw['alpha'], kw['lo'], kw['hi'], kw['nc'], kw['iteration0'], value=value))
  return _REF[key][1]


def check_coverage(cs, ref):
  """the core case's conditions, on the oracle's intermediates, before anything is compared"""
  its, E, kw = ref['iters'], cs.E, cs.kw
  lo, hi = F32(kw['lo']), F32(kw['hi'])
  tie = notie = with0 = without0 = False
  for it in its:
    ret = it['ret']
    for i, el in enumerate(it['el']):
      r = sorted((v for v in ret[:, i] if not np.isnan(v)), reverse=True)
      if len(r) > E:
        tie, notie = tie or r[E - 1] == r[E], notie or r[E - 1] != r[E]
      with0, without0 = with0 or 0 in el, without0 or (len(el) > 0 and 0 not in el)
  if cs.rt == 'sparse':                                    # (the dense reward is continuous in the positions: distinct candidates never score alike)
    assert tie, 'no env with a tie in ret straddling rank E - 1 / E'
  assert notie, 'no env without a tie at rank E - 1 / E'
  assert with0 and without0, f'elite sets with branch 0: {with0}, without: {without0}'
  assert bool(any((np.abs(it['act'][1:]) == 1).any() for it in its)) and bool((np.abs(cs.mean) > 1).any()), 'no candidate component clipped at +-1'
  s_all = np.concatenate([it['s'].reshape(-1) for it in its] + [it['std'].reshape(-1) for it in its])
  assert bool((s_all == lo).any()) and bool((s_all == hi).any()), 'sclamp never hits std_min / std_max'
  assert bool(any(((it['e_std'] > 0) & (it['std'] > lo) & (it['std'] < hi)).any() for it in its)), 'no e_std that is neither 0 nor clamped'
  assert not np.array_equal(its[-1]['plan'], its[0]['plan']), 'the second iteration changes nothing'


def check_case(side, cs, key=None, sc=None, mean=None, std0='case', K=None, alias=False, value=None, nan_returns=False, **over):
  """both fills: bands intact, every output overwritten; the state untouched; every output equal to the oracle, bit for bit.  nan_returns: as
  tabletop_plan_helpers.check_case (a NaN's sign and payload are open: ret and ret0 NaN in the same places, equal elsewhere)"""
  sc, mean, K = cs.sc if sc is None else sc, cs.mean if mean is None else mean, cs.K if K is None else K
  s0 = cs.std0 if isinstance(std0, str) else std0
  ref = reference(cs, side, key, sc, mean, s0, K, value, **over)
  what = cs.what + (f' [{key}]' if key is not None else '') + (f' {value.what}' if value is not None else '')
  res = ta.both_fills(run_ok, side, sc, mean, s0, K, what=what, alias=alias, value=value, **{**cs.kw, **over})
  tb.state_untouched(res, sc, what)
  if nan_returns:
    compare(res, ref, what, ['plan', 'std', 'best_ret', 'best_k'])
    for k in ('ret', 'ret0'):
      ta.same(res['out.' + k].cpu(), ref['out.' + k].cpu(), f'{what}: {k}', atol=0.0)
  else:
    compare(res, ref, what)
  return res


def check_pointers(side, cs, full):
  """the optional pointers NULL in every combination, the in-place forms (plan == mean and std == std0), std0 NULL == a std0 holding sigma; ret / std NULL refused"""
  for mask in range(1, 8):
    null = tuple(k for b, k in enumerate(OPTIONAL) if mask >> b & 1)
    res = ta.both_fills(run_ok, side, cs.sc, cs.mean, cs.std0, cs.K, what=f'{cs.what} without {null}', null=null, **cs.kw)
    assert not any('out.' + k in res for k in null)
    tb.state_untouched(res, cs.sc, cs.what)
    compare(res, full, f'{cs.what} without {null}', [k for k in OUTS if k not in null])
  res = ta.both_fills(run_ok, side, cs.sc, cs.mean, cs.std0, cs.K, what=f'{cs.what} in place', alias=True, **cs.kw)
  tb.state_untouched(res, cs.sc, cs.what)
  compare(res, full, f'{cs.what} in place')
  flat = np.broadcast_to(sigma3(cs.kw['sigma']), cs.mean.shape).copy()
  a, b = run_ok(side, cs.sc, cs.mean, None, cs.K, 0x00, **cs.kw)
  b.check('std0 NULL')
  z, b = run_ok(side, cs.sc, cs.mean, flat, cs.K, 0xFF, **cs.kw)
  compare(a, z, 'std0 NULL vs std0 = sigma in every row')
  for name in ('ret', 'std'):
    rc, res, b = run_cem(side, cs.sc, cs.mean, cs.std0, cs.K, 0xFF, null=(name,), **cs.kw)
    assert rc == -1 and side.lib.earl_last_error()
    b.check(name + ' NULL')
    ta.assert_untouched(res, cs.sc, name + ' NULL')


def check_value_identity(side, cs):
  """pv = {1.0, NULL} equals pv == NULL bit for bit"""
  import tabletop_value_helpers as vh
  free, b = run_ok(side, cs.sc, cs.mean, cs.std0, cs.K, 0x00, **cs.kw)
  got, b = run_ok(side, cs.sc, cs.mean, cs.std0, cs.K, 0xFF, value=vh.Value(None, 1.0), **cs.kw)
  b.check('pv = {1.0, NULL}')
  compare(got, free, cs.what + ' pv = {1.0, NULL} vs pv NULL')


def check_e_edges(side, nobj, rt):
  """E = 1: V = 0, std' = sclamp(alpha * s) -- std_min with alpha = 0; E = K: every branch that is not NaN; E = K with alpha = 0"""
  cs = case(nobj, rt)
  one = check_case(side, cs, key=('E=1', nobj, rt), E=1, alpha=0.0, I=1)
  assert bool((one['out.std'] == cs.kw['lo']).all()), 'E = 1, alpha = 0: std\' = std_min'
  check_case(side, cs, key=('E=1 smoothed', nobj, rt), E=1)
  check_case(side, cs, key=('E=K', nobj, rt), E=cs.K)
  check_case(side, cs, key=('E=K alpha=0', nobj, rt), E=cs.K, alpha=0.0)


def check_k_mapping(side, nobj, K, mpc_T=None):
  """n = 3, H = 2, E = min(8, K), sigma 2.0: |D| near 2^21, many candidates at +-1; the planner (and with mpc_T the fused loop) at this K"""
  cs = case(nobj, 'sparse', n=3, K=K, H=2, I=1, E=min(8, K), sigma=(2.0, 2.0, 2.0), lo=0.0, hi=2.0, std0=False)
  ref = reference(cs, side)
  if K > 8:
    act = ref['iters'][0]['act']
    assert bool((np.abs(act[1:]) == 1).mean() > 0.3) and int(np.abs(np.rint((act - ref['iters'][0]['m'][None]).astype(F64) * 2.0**20)).max()) > 2**20
  check_case(side, cs)
  if mpc_T:
    check_mpc_case(side, cs, mpc_T)


def check_chaining(side, cs, I=3):
  """I iterations in one call == I calls of one, numbered on, each fed the previous plan and std (in place)"""
  kw = {**cs.kw, 'I': I}
  whole, b = run_ok(side, cs.sc, cs.mean, cs.std0, cs.K, 0x00, **kw)
  b.check('chaining, one call')
  plan, std, ret0 = cs.mean, cs.std0, []
  for j in range(I):
    one, b = run_ok(side, cs.sc, plan, std, cs.K, 0xFF, alias=True, **{**kw, 'I': 1, 'iteration0': j})
    b.check(f'chaining, call {j}')
    plan, std = one['out.plan'].cpu().numpy(), one['out.std'].cpu().numpy()
    ret0.append(one['out.ret0'].cpu())
  compare(one, whole, 'chained calls vs one call', ['plan', 'std', 'ret', 'best_ret', 'best_k'])
  ta.same(torch.cat(ret0), whole['out.ret0'].cpu(), 'chained calls vs one call: ret0')
  compare(whole, reference(cs, side, key=('I', I, id(cs)), I=I), 'three iterations vs the oracle')


def check_shards(side, cs):
  """two shards (0..40, 40..70, env_offset moving with them) == the batch"""
  full = check_case(side, cs)
  for lo, hi in ((0, 40), (40, 70)):
    part, b = run_ok(side, tb.shard(cs.sc, lo, hi), np.ascontiguousarray(cs.mean[:, lo:hi]), np.ascontiguousarray(cs.std0[:, lo:hi]), cs.K, 0x00, **cs.kw)
    b.check(f'shard {lo}..{hi}')
    for k in OUTS:
      whole = full['out.' + k]
      ta.same(part['out.' + k].cpu(), (whole[:, lo:hi] if whole.dim() > 1 else whole[lo:hi]).cpu().contiguous(), f'shard {lo}..{hi}: {k}')


def check_noise_words(side, cs):
  """iteration0 and noise_counter enter the draws; word 0 is CEM's own: the MPPI candidates at the same counters differ"""
  base = check_case(side, cs)
  for what, over in (('iteration0 = 5', dict(iteration0=5)), ('noise_counter + 1', dict(nc=cs.kw['nc'] + 1))):
    other = check_case(side, cs, key=(what, id(cs)), **over)
    assert not torch.equal(base['out.plan'], other['out.plan']), what + ': the same plan'
  flat = np.broadcast_to(sigma3(cs.kw['sigma']), cs.mean.shape).copy()
  rc, cem, b = run_candidates(side, cs.sc, cs.mean, flat, cs.K, 0x00, sigma=cs.kw['sigma'], nc=cs.kw['nc'])
  assert rc == 0
  rc, mppi, b = h.run_candidates(side, cs.sc, cs.mean, cs.K, 0x00, sigma=cs.kw['sigma'], nc=cs.kw['nc'])
  assert rc == 0
  ta.same(cem['out.act'][0].cpu(), mppi['out.act'][0].cpu(), 'branch 0 of both planners is the clipped mean')
  assert not bool((cem['out.act'][1:] == mppi['out.act'][1:]).all(-1).any()), 'a CEM candidate equals the MPPI candidate at the same counters'


def nan_quadrant_net(D, x0, y0):
  """a ReLU value network D -> 16 -> 16 -> 1 whose output is Inf - Inf = NaN where the gripper ends right of x0 AND above y0, +Inf / -Inf where only one holds and 0
  elsewhere: h_j = relu(1e30 * (q_j - q0_j)), g_j = relu(1e38 * h_j) (0 or an overflow to Inf), V = g_0 - g_1"""
  import tabletop_value_helpers as vh
  W0, b0, W1, Wo = np.zeros((16, D), F32), np.zeros(16, F32), np.zeros((16, 16), F32), np.zeros((1, 16), F32)
  for j, q0 in enumerate((x0, y0)):
    W0[j, j], b0[j], W1[j, j] = 1e30, -1e30 * float(q0), 1e38
  Wo[0, 0], Wo[0, 1] = 1.0, -1.0
  return vh.Net(D, (16, 16), 'relu', 'none', layers=[(W0, b0), (W1, np.zeros(16, F32)), (Wo, np.zeros(1, F32))])


def check_nonfinite(side, nobj):
  """NaN and +-Inf in mean and std0: clipped / clamped, every output finite and equal to the oracle.  SOME returns of an env NaN (a value network that is NaN in one
  quadrant, E = K): Ne < E, the +-Inf returns take their places in the order.  A NaN in one env's state under the dense reward: ALL its returns are NaN, Ne = 0,
  plan' = m and std' = s.  The state is untouched throughout and nothing faults"""
  import tabletop_value_helpers as vh
  cs = case(nobj, 'dense')
  mean, std0 = cs.mean.copy(), cs.std0.copy()
  mean[0, 3, 0], mean[1, 5, 1], mean[2, 7, 2], mean[3, 66, 0] = np.nan, np.inf, -np.inf, np.nan
  std0[0, 4, 0], std0[1, 6, 1], std0[2, 8, 2], std0[3, 67, 0] = np.nan, np.inf, -np.inf, np.nan
  res = check_case(side, cs, key=('non-finite mean and std0', nobj), mean=mean, std0=std0)
  assert all(bool(torch.isfinite(res['out.' + k]).all()) for k in ('plan', 'std', 'ret'))
  last = vh.branch_rollouts(side, cs.sc, reference(cs, side)['iters'][0]['act'])[1]       # where the existing rollouts leave the gripper: env 9's branches straddle
  value = vh.Value(nan_quadrant_net(cs.sc.obs_dim, *last[0, 9, :2]), 0.9)                 # the point its branch 0 reaches
  ref = reference(cs, side, key=('some NaN', nobj), value=value, E=cs.K)
  nans = np.isnan(ref['iters'][0]['ret']).sum(0)
  assert bool(((nans > 0) & (nans < cs.K)).any()), 'no env with some, not all, returns NaN'
  assert bool(np.isinf(ref['iters'][0]['ret']).any())
  assert any(0 < len(el) < cs.K for el in ref['iters'][0]['el'])
  check_case(side, cs, key=('some NaN', nobj), value=value, E=cs.K, nan_returns=True)
  sc = tb.with_cfg(cs.sc)
  sc.state = {k: v.copy() for k, v in cs.sc.state.items()}
  sc.state['qpos'][9, 2] = np.nan
  ref = reference(cs, side, key=('NaN state', nobj), sc=sc)
  assert bool(torch.isnan(ref['out.ret'][:, 9]).all()) and ref['iters'][-1]['el'][9] == [], 'the NaN of the state does not reach every return'
  res = check_case(side, cs, key=('NaN state', nobj), sc=sc, nan_returns=True)
  assert float(res['out.best_ret'][9]) == -np.inf and int(res['out.best_k'][9]) == 0
  ta.same(res['out.plan'][:, 9].cpu(), ta._t(ref['iters'][0]['m'][:, 9]), 'Ne = 0: the plan is the clipped mean')
  ta.same(res['out.std'][:, 9].cpu(), ta._t(ref['iters'][0]['s'][:, 9]), 'Ne = 0: the std is the clamped std0')


def check_value(side, cs):
  """with pv: one tanh value net D -> 16 -> 1 and discount 0.9 against the oracle whose returns are the existing rollouts' discounted sums plus the host forward"""
  import tabletop_value_helpers as vh
  value = vh.Value(vh.net(cs.sc.obs_dim, (16,), 'tanh', 'none'), 0.9)
  ref, free = reference(cs, side, value=value), reference(cs, side)
  assert not np.array_equal(ref['iters'][0]['ret'], free['iters'][0]['ret'])
  check_case(side, cs, value=value)


def check_candidates(side, cs):
  """the entry point == the oracle's candidates; fed to the existing branch launch they reproduce plan_cem's ret; best_k indexes them; std NULL: sigma"""
  kw = cs.kw
  s = sclamp(cs.std0, kw['lo'], kw['hi'])
  for j in (0, 1, 255):
    want, m = candidates(cs.sc.cfg(), cs.K, cs.H, j, kw['nc'], cs.mean, s)
    for fill in ta.FILLS:
      rc, res, b = run_candidates(side, cs.sc, cs.mean, cs.std0, cs.K, fill, j=j, lo=kw['lo'], hi=kw['hi'], nc=kw['nc'])
      assert rc == 0
      b.check(f'cem candidates j={j}')
      ta.same(res['out.act'].cpu(), ta._t(want), f'{cs.what}: candidates of iteration {j}')
    ta.same(res['out.act'][0].cpu(), ta._t(h.clip(cs.mean)), 'branch 0 is the clipped mean')
  got, b = run_ok(side, cs.sc, cs.mean, cs.std0, cs.K, 0x00, **{**kw, 'I': 1, 'iteration0': 255})
  ret = h.branch_returns(side, cs.sc, res['out.act'].cpu().numpy())
  ta.same(got['out.ret'].cpu(), ta._t(ret), 'the branch launch on cem_candidates vs plan_cem\'s ret')
  bk = got['out.best_k'].cpu().numpy()
  ta.same(got['out.best_ret'].cpu(), ta._t(ret[bk, np.arange(cs.n)]), 'best_k indexes the candidates')
  flat = np.broadcast_to(sigma3(kw['sigma']), cs.mean.shape).copy()
  rc, a, b = run_candidates(side, cs.sc, cs.mean, None, cs.K, 0x00, sigma=kw['sigma'], nc=kw['nc'])
  rc2, z, b = run_candidates(side, cs.sc, cs.mean, flat, cs.K, 0xFF, sigma=(0.0, 0.0, 0.0), nc=kw['nc'])
  assert rc == 0 and rc2 == 0
  ta.same(a['out.act'].cpu(), z['out.act'].cpu(), 'std NULL: sigma in every row')


def check_device_vs_host(cs, dev, host):
  """sparse: every output bit for bit.  dense: ONE iteration, ret / ret0 / best_ret within 1e-6 * sum_t |r_t| (the sums from the twin's own rollouts of the
  candidates), plan and std not compared"""
  kw = cs.kw if cs.rt == 'sparse' else {**cs.kw, 'I': 1}
  d, b = run_ok(dev, cs.sc, cs.mean, cs.std0, cs.K, 0x00, **kw)
  b.check(cs.what + ' device')
  hh, b = run_ok(host, cs.sc, cs.mean, cs.std0, cs.K, 0x00, **kw)
  b.check(cs.what + ' host')
  if cs.rt == 'sparse':
    return compare(d, hh, cs.what + ' device vs host')
  act = candidates(cs.sc.cfg(), cs.K, cs.H, kw['iteration0'], kw['nc'], cs.mean, sclamp(cs.std0, kw['lo'], kw['hi']))[0]
  bound = tb.DENSE_REL * tb.reference(cs, host, cs.sc, act, key=(id(cs), 'cem sum |r|'))['abs']
  for name, bnd in (('ret', bound), ('ret0', bound[:1]), ('best_ret', bound.max(0))):
    err = (d['out.' + name].cpu() - hh['out.' + name].cpu()).abs().numpy()
    print(f'{cs.what}: {name}: max |d| = {err.max():.3e}, min bound = {bnd.min():.3e}, max ratio = {(err / bnd).max():.3e}')
    assert bool((err <= bnd).all()), f'{cs.what}: |d {name}| up to {err.max()} beyond 1e-6 * sum |r|'


# ---------------------------------------------------------------------------------------------------- refusals and empty work
def refusals(cs):
  nan, inf = float('nan'), float('inf')
  keep = ('n < 0', 'reward_type', 'qpos NULL', 'params NULL', 'mean NULL', 'plan NULL', 'ret NULL', 'K = 0', 'K < 0', 'K = 65537', 'H = 0', 'H = 65537', 'iterations = 0',
          'iteration0 < 0', 'iteration0 + iterations = 257', 'iterations overflow', 'sigma < 0', 'sigma NaN', 'sigma Inf', 'lifelong arrays NULL', '3 objects: wide_init',
          '3 objects: lifelong')
  out = [(what, kw) for what, kw in h.refusals(cs) if what in keep]                         # everything the MPPI counterpart refuses (but its temperature)
  out += [('K = 1025', dict(tell=dict(K=1025))), ('elites = 0', dict(tell=dict(elites=0))), ('elites < 0', dict(tell=dict(elites=-1))),
          ('elites = K + 1', dict(tell=dict(elites=cs.K + 1))), ('alpha < 0', dict(tell=dict(alpha=-0.1))), ('alpha = 1', dict(tell=dict(alpha=1.0))),
          ('alpha NaN', dict(tell=dict(alpha=nan))), ('alpha Inf', dict(tell=dict(alpha=inf))), ('std_min < 0', dict(tell=dict(std_min=-0.1))),
          ('std_min > std_max', dict(tell=dict(std_min=0.7))), ('std_min NaN', dict(tell=dict(std_min=nan))), ('std_max NaN', dict(tell=dict(std_max=nan))),
          ('std_max Inf', dict(tell=dict(std_max=inf))), ('std NULL', dict(null=('std',))),
          ('plan overlaps mean from above', dict(ptrs=dict(plan=lambda a: a['mean'] + 12))), ('plan overlaps mean from below', dict(ptrs=dict(plan=lambda a: a['mean'] - 12))),
          ('std overlaps std0', dict(ptrs=dict(std=lambda a: a['std0'] + 12))), ('std is mean', dict(ptrs=dict(std=lambda a: a['mean']))),
          ('std is plan', dict(ptrs=dict(std=lambda a: a['plan']))), ('std0 is mean', dict(ptrs=dict(std0=lambda a: a['mean']))),
          ('std0 is plan', dict(ptrs=dict(std0=lambda a: a['plan']))), ('plan is std0', dict(ptrs=dict(plan=lambda a: a['std0'])))]
  return out


def check_refusals(side, cs):
  import tabletop_value_helpers as vh
  for what, kw in refusals(cs):
    rc, res, b = run_cem(side, cs.sc, cs.mean, cs.std0, cs.K, 0xFF, **{**cs.kw, **kw})
    assert rc == -1, f'{cs.what} {what}: rc = {rc}'
    assert side.lib.earl_last_error(), what
    b.check(f'{cs.what} {what}')
    ta.assert_untouched(res, cs.sc, f'{cs.what} {what}')
  for what, vnet, kw in vh.value_refusals(cs.sc.obs_dim)[1:]:                               # (pv NULL is the value-free call here)
    rc, res, b = run_cem(side, cs.sc, cs.mean, cs.std0, cs.K, 0xFF, value=vh.Value(vnet, **kw), **cs.kw)
    assert rc == -1 and side.lib.earl_last_error(), f'{cs.what} {what}: rc = {rc}'
    ta.assert_untouched(res, cs.sc, f'{cs.what} {what}')
  big = ta.Scene(2, nobj=cs.nobj)                             # grids: told n, nothing that large allocated
  for what, n_call, told in (('2^32 lanes in the score launch', 2**26, dict(K=64, elites=1)), ('2^32 lanes in the update launch', 2**27, dict(H=32))):
    rc, res, b = run_cem(side, big, np.zeros((1, 2, 3), F32), None, 1, 0xFF, E=1, n_call=n_call, tell=told)
    assert rc == -1 and b'launch' in side.lib.earl_last_error(), what
    ta.assert_untouched(res, big, what)
  for fn in ('earl_tabletop_plan_cem', 'earl_tabletop3_plan_cem'):
    assert getattr(side.lib, fn)(*([None] * 12), side.stream) == -1
  for what, kw in (('cfg NULL', dict(cfg_null=True)), ('params NULL', dict(params_null=True)), ('mean NULL', dict(mean_null=True)), ('act_out NULL', dict(out_null=True)),
                   ('n < 0', dict(n_call=-1)), ('j < 0', dict(j=-1)), ('j = 256', dict(j=256)), ('K = 0', dict(tell=dict(K=0))), ('K = 1025', dict(tell=dict(K=1025))),
                   ('H = 65537', dict(tell=dict(H=65537))), ('sigma NaN', dict(tell=dict(sigma=(float('nan'), 0.0, 0.0)))), ('std_min > std_max', dict(tell=dict(std_min=3.0))),
                   ('grid', dict(n_call=2**26, tell=dict(K=64)))):
    rc, res, b = run_candidates(side, cs.sc, cs.mean, cs.std0, cs.K, 0xFF, **kw)
    assert rc == -1, f'cem candidates {what}: rc = {rc}'
    b.check('cem candidates ' + what)
    ta.assert_untouched(res, cs.sc, 'cem candidates ' + what)


def check_empty(side, cs):
  """n == 0: EARL_OK, nothing written"""
  for fill in ta.FILLS:
    rc, res, b = run_cem(side, cs.sc, cs.mean, cs.std0, cs.K, fill, n_call=0, **cs.kw)
    assert rc == 0
    b.check('plan_cem n = 0')
    ta.assert_untouched(res, cs.sc, 'plan_cem n = 0')
    rc, res, b = run_candidates(side, cs.sc, cs.mean, cs.std0, cs.K, fill, n_call=0)
    assert rc == 0
    b.check('cem candidates n = 0')
    ta.assert_untouched(res, cs.sc, 'cem candidates n = 0')


# ---------------------------------------------------------------------------------------------------- MPC
def run_mpc(side, sc, plan, K, T, fill, I=1, E=2, sigma=0.3, alpha=0.0, lo=0.0, hi=2.0, nc=7, iteration0=0, null=(), n_call=None, T_call=None, cfg_over=None, out_null=False,
            mpc_null=False, params_null=False, tell=None, value=None):
  """tabletop_mpc_helpers.run_mpc on earl_tabletop[3]_mpc_rollout_cem"""
  n, H, D = sc.n, int(plan.shape[0]), sc.obs_dim
  r = ta.Run(side, fill, null)
  st = r.state(sc)
  p = None if 'plan' in r.null else r.put('io.plan', plan, n * 3)
  out = r.out((T, n), D)
  r.blank('out.act', (T, n, 3), torch.float32, n * 3)
  r.blank('out.ret0', (T, I, n), torch.float64, n)
  r.blank('out.best_ret', (T, n), torch.float64, n)
  mpc = _abi.MpcOut(act=r.ptr('out.act'), plan=None if p is None else p.data_ptr(), ret0=r.ptr('out.ret0'), best_ret=r.ptr('out.best_ret'))
  cp = h.told(params(K, H, I, E, sigma, alpha, lo, hi, nc, iteration0), tell)
  pv, keep = value_block(value, r)
  cfg = sc.cfg(**(cfg_over or {}))
  if n_call is not None:
    cfg.n = n_call
  fn = getattr(side.lib, ta._pfx(sc) + 'mpc_rollout_cem')
  rc = fn(C.byref(cfg), C.byref(st), None if params_null else C.byref(cp), pv, T if T_call is None else T_call, None if out_null else C.byref(out),
          None if mpc_null else C.byref(mpc), side.stream)
  side.sync()
  del keep
  return rc, {k: v[3].clone() for k, v in r.b.bufs.items() if k.startswith(('st.', 'out.', 'io.'))}, r.b


def run_mpc_ok(side, sc, plan, K, T, fill, **kw):
  rc, res, b = run_mpc(side, sc, plan, K, T, fill, **kw)
  _abi.check(rc, 'mpc_rollout_cem', side.lib)
  return res, b


def composed(side, sc, plan, K, T, nc=7, **kw):
  """the header's definition, call by call (tabletop_mpc_helpers.composed with plan_cem, std0 = NULL, as the planner)"""
  cur, P = sc, np.asarray(plan, F32)
  rows = {k: [] for k in mh.OUTS}
  rets, plans = [], [P]
  for s in range(T):
    res, b = run_ok(side, cur, P, None, K, 0x00, nc=(nc + s) & 0xFFFFFFFF, **kw)
    b.check('the reference\'s plan_cem')
    tb.state_untouched(res, cur, 'the reference\'s plan_cem')
    Pp = res['out.plan'].cpu().numpy()
    out, b = ta.run_rollout(side, cur, np.ascontiguousarray(Pp[:1]), 0x00)
    b.check('the reference\'s rollout')
    for k in mh.OUT4:
      rows[k].append(out['out.' + k].cpu()[0])
    rows['act'].append(ta._t(Pp[0]))
    rows['ret0'].append(res['out.ret0'].cpu())
    rows['best_ret'].append(res['out.best_ret'].cpu())
    rets.append(res['out.ret'].cpu().numpy())
    P = mh.shift(Pp, out['out.done'].cpu().numpy()[0], bool(cur.cfg().auto_reset))
    plans.append(P)
    cur = mh.after(sc, out, sc.counter + s + 1)
  ref = {'out.' + k: torch.stack(v) for k, v in rows.items()}
  ref['io.plan'] = ta._t(P)
  ref.update({'st.' + k: ta._t(cur.state[k]) for k in ta.STATE})
  ref.update(rets=np.stack(rets), dones=ref['out.done'].numpy().astype(bool), plans=np.stack(plans))
  return ref


_MREF = {}


def mpc_reference(side, cs, T, key=None, sc=None, plan=None, **over):
  key = ((id(cs), T) if key is None else key, side.device)
  if key not in _MREF:
    _MREF[key] = composed(side, cs.sc if sc is None else sc, cs.mean if plan is None else plan, cs.K, T, **{**cs.kw, **over})
  return _MREF[key]


def check_mpc_case(side, cs, T, key=None, sc=None, plan=None, **over):
  """both fills; every output, the final plan and the final state equal to the composed reference, bit for bit"""
  sc, plan = cs.sc if sc is None else sc, cs.mean if plan is None else plan
  ref = mpc_reference(side, cs, T, key, sc, plan, **over)
  what = f'cem mpc T={T} {cs.what}' + (f' [{key}]' if key is not None else '')
  res = ta.both_fills(run_mpc_ok, side, sc, plan, cs.K, T, what=what, **{**cs.kw, **over})
  mh.compare(res, ref, what)
  return res


def check_mpc_coverage(cs, ref, general=False):
  act, plans, rets = ref['out.act'].numpy(), ref['plans'], ref['rets']
  assert bool((act[0] != h.clip(plans[0][0])).any()), 'every executed action is the clipped start plan: the planner moved nothing'
  if cs.rt == 'dense' or general:
    assert bool((rets.min(1) != rets.max(1)).any()), 'no env whose returns differ across branches at some real step'
  if general:
    dones = ref['dones']
    assert bool(dones.any()), 'no env resets inside the launch'
    hit = False
    for s, i in zip(*np.nonzero(dones[:-1])):
      assert not plans[s + 1][:, i].any(), 'the plan of a reset env was not zeroed'
      hit = hit or bool(act[s + 1:, i].any())
    assert hit, 'no env with a non-zero action after its plan was zeroed'


def check_mpc_pointers(side, cs, T, full):
  for name in mh.OUTS:
    what = f'cem mpc {cs.what} without {name}'
    res = ta.both_fills(run_mpc_ok, side, cs.sc, cs.mean, cs.K, T, what=what, null=(name,), **cs.kw)
    assert 'out.' + name not in res and set(res) == set(full) - {'out.' + name}
    mh.compare(res, full, what)


def check_mpc_chaining(side, cs, T1=2, T2=3):
  whole = check_mpc_case(side, cs, T1 + T2)
  a, b = run_mpc_ok(side, cs.sc, cs.mean, cs.K, T1, 0x00, **cs.kw)
  b.check('chaining, first call')
  nxt = mh.after(cs.sc, a, cs.sc.counter + T1)
  z, b = run_mpc_ok(side, nxt, a['io.plan'].cpu().numpy(), cs.K, T2, 0xFF, **{**cs.kw, 'nc': cs.kw['nc'] + T1})
  b.check('chaining, second call')
  for k in whole:
    if k.startswith('out.'):
      ta.same(torch.cat([a[k].cpu(), z[k].cpu()]), whole[k].cpu(), f'chained calls vs one call: {k}')
    else:
      ta.same(z[k].cpu(), whole[k].cpu(), f'chained calls vs one call: {k}')


def check_mpc_shards(side, cs, T):
  full = check_mpc_case(side, cs, T)
  for lo, hi in ((0, 40), (40, 70)):
    part, b = run_mpc_ok(side, tb.shard(cs.sc, lo, hi), np.ascontiguousarray(cs.mean[:, lo:hi]), cs.K, T, 0x00, **cs.kw)
    b.check(f'shard {lo}..{hi}')
    for k, v in part.items():
      whole = full[k].cpu()
      env_axis = 0 if k.startswith('st.') else (2 if k == 'out.ret0' else 1)
      ta.same(v.cpu(), whole.narrow(env_axis, lo, hi - lo).contiguous(), f'shard {lo}..{hi}: {k}')


def check_mpc_device_vs_host(cs, T, dev, host):
  assert cs.rt == 'sparse'
  d, b = run_mpc_ok(dev, cs.sc, cs.mean, cs.K, T, 0x00, **cs.kw)
  b.check(cs.what + ' device')
  hh, b = run_mpc_ok(host, cs.sc, cs.mean, cs.K, T, 0x00, **cs.kw)
  b.check(cs.what + ' host')
  mh.compare(d, hh, cs.what + ' device vs host')


def mpc_refusals(cs):
  drop = ('mean NULL', 'ret NULL', 'std NULL', 'plan overlaps mean from above', 'plan overlaps mean from below', 'std overlaps std0', 'std is mean', 'std is plan', 'std0 is mean',
          'std0 is plan', 'plan is std0')
  out = [(what, kw) for what, kw in refusals(cs) if what not in drop]
  out += [('out NULL', dict(out_null=True)), ('every pointer of out NULL', dict(null=mh.OUT4)), ('mpc NULL', dict(mpc_null=True)), ('T < 0', dict(T_call=-1)),
          ('H = 257', dict(tell=dict(H=257)))]
  return out


def check_mpc_refusals(side, cs, T=3):
  """every rule, the documented refusal of a value block included; n == 0 and T == 0 write nothing"""
  import tabletop_value_helpers as vh
  for what, kw in mpc_refusals(cs):
    rc, res, b = run_mpc(side, cs.sc, cs.mean, cs.K, T, 0xFF, **{**cs.kw, **kw})
    assert rc == -1, f'cem mpc {cs.what} {what}: rc = {rc}'
    assert side.lib.earl_last_error(), what
    b.check(f'cem mpc {cs.what} {what}')
    mh.assert_untouched(res, cs.sc, cs.mean, f'cem mpc {cs.what} {what}')
  for value in (vh.Value(vh.net(cs.sc.obs_dim, (16,), 'tanh', 'none'), 0.9), vh.Value(None, 1.0)):   # one tanh value net 12|20 -> 16 -> 1, discount 0.9: the documented refusal
    rc, res, b = run_mpc(side, cs.sc, cs.mean, cs.K, T, 0xFF, value=value, **cs.kw)
    assert rc == -1 and b'pv' in side.lib.earl_last_error(), value.what
    b.check('cem mpc with a value block')
    mh.assert_untouched(res, cs.sc, cs.mean, 'cem mpc with a value block')
  big = ta.Scene(2, nobj=cs.nobj)
  plan = np.zeros((1, 2, 3), F32)
  for what, n_call, told in (('2^32 lanes', 2**26, dict(K=64)), ('2^32 lanes of sixteen waves', 2**22, dict(K=1024))):
    rc, res, b = run_mpc(side, big, plan, 1, 1, 0xFF, E=1, n_call=n_call, tell=told)
    assert rc == -1 and b'launch' in side.lib.earl_last_error(), what
    mh.assert_untouched(res, big, plan, what)
  for fn in ('earl_tabletop_mpc_rollout_cem', 'earl_tabletop3_mpc_rollout_cem'):
    assert getattr(side.lib, fn)(None, None, None, None, 1, None, None, side.stream) == -1
  for what, kw in (('n = 0', dict(n_call=0)), ('T = 0', dict(T_call=0))):
    for fill in ta.FILLS:
      rc, res, b = run_mpc(side, cs.sc, cs.mean, cs.K, T, fill, **{**cs.kw, **kw})
      assert rc == 0, f'cem mpc {what}: rc = {rc}'
      b.check('cem mpc ' + what)
      mh.assert_untouched(res, cs.sc, cs.mean, 'cem mpc ' + what)


# ---------------------------------------------------------------------------------------------------- through Python
def check_python_plan(env, K=6, E=2, H=9, I=2, seed=3):
  """plan_cem leaves the env as found; cem_candidates fed to rollout_branches reproduces the ret of a further iteration and best_k indexes it; the `out=` rules"""
  u = env.unwrapped
  n, dev = u.num_envs, u.device
  rng = np.random.default_rng(seed)
  mean = torch.from_numpy(rng.uniform(-1.1, 1.1, (H, n, 3)).astype(F32)).to(dev)
  std = torch.from_numpy(rng.uniform(0.0, 0.8, (H, n, 3)).astype(F32)).to(dev)
  kw = dict(K=K, elites=E, sigma=(0.5, 0.5, 0.8), alpha=0.25, std_min=0.05, std_max=0.6)
  before, steps = tb.snapshot(env), u.total_step_count
  got = env.plan_cem(mean, iterations=I, std=std, **kw)
  tb.assert_env_as_found(env, before, 'plan_cem')
  assert u.total_step_count == steps
  assert {k: (tuple(v.shape), v.dtype) for k, v in got.items()} == {
      'plan': ((H, n, 3), torch.float32), 'std': ((H, n, 3), torch.float32), 'ret': ((K, n), torch.float64), 'ret0': ((I, n), torch.float64),
      'best_ret': ((n,), torch.float64), 'best_k': ((n,), torch.int32)}
  assert bool((got['std'] >= 0.05).all()) and bool((got['std'] <= 0.6).all())
  nxt = env.plan_cem(got['plan'], iterations=1, iteration0=I, std=got['std'], **{**kw, 'std_min': 0.0, 'std_max': 2.0})
  cand = env.cem_candidates(got['plan'], K, std=got['std'], iteration=I)
  ta.same(env.rollout_branches(cand, last_obs=False)['ret'].cpu(), nxt['ret'].cpu(), 'rollout_branches(cem_candidates) vs ret')
  pick = cand[nxt['best_k'].long(), :, torch.arange(n, device=dev)].permute(1, 0, 2).contiguous()
  ta.same(env.rollout_branches(pick[None], last_obs=False)['ret'][0].cpu(), nxt['best_ret'].cpu(), 'candidate best_k scores best_ret')
  tb.assert_env_as_found(env, before, 'cem_candidates / rollout_branches')
  pbuf, sbuf = mean.clone(), std.clone()
  res = env.plan_cem(pbuf, iterations=I, std=sbuf, out={'plan': pbuf, 'std': sbuf, 'best_k': None}, **kw)
  assert set(res) == {'plan', 'std', 'ret'} and res['plan'] is pbuf and res['std'] is sbuf
  ta.same(pbuf.cpu(), got['plan'].cpu(), 'in place through Python: plan')
  ta.same(sbuf.cpu(), got['std'].cpu(), 'in place through Python: std')
  for bad in ({'plan': pbuf[:, :, :2]}, {'plan': pbuf, 'std': torch.empty(H, n, 3, dtype=torch.float64, device=dev)}, {'plan': pbuf, 'nope': pbuf}, {'std': sbuf}):
    try:
      env.plan_cem(mean, iterations=I, out=bad, **kw)
    except ValueError:
      continue
    raise AssertionError(f'out = {list(bad)} was accepted')
  for bad in (dict(elites=0), dict(elites=K + 1), dict(K=1025), dict(alpha=1.0), dict(std_min=0.7), dict(discount=0.0)):
    try:
      env.plan_cem(mean, **{**kw, **bad})
    except ValueError:
      continue
    raise AssertionError(f'{bad} was accepted')
  return {k: v.cpu() for k, v in got.items()}


def python_loop(env, T, plan, **kw):
  """the loop rollout_mpc(method='cem') replaces, on the public methods"""
  rows = {k: [] for k in mh.KEYS if k != 'plan'}
  plan = plan.clone()
  for _ in range(T):
    got = env.plan_cem(plan, **kw)
    plan = got['plan']
    obs, rew, done, succ = env.rollout(plan[:1].contiguous())
    for k, v in zip(('obs', 'reward', 'done', 'success', 'actions', 'ret0', 'best_ret'), (obs[0], rew[0], done[0], succ[0], plan[0].clone(), got['ret0'], got['best_ret'])):
      rows[k].append(v)
    plan = torch.cat([plan[1:], plan[-1:]])
    if env.unwrapped._cfg.auto_reset:
      plan[:, done[0]] = 0
  out = {k: torch.stack(v) for k, v in rows.items()}
  out['plan'] = plan
  return out


def check_python_mpc(device, nobj, general=False, T=4, K=6, E=2, H=6, I=2, seed=3):
  """rollout_mpc(method='cem') == the hand-written loop on a second env built alike; rollout_mpc() with no new keyword == the existing composition of plan_mppi and
  rollout (tabletop_mpc_helpers.python_loop): the parent's path; the CEM keywords are refused under 'mppi'"""
  env, twin = tb.make_env(nobj, device, general=general), tb.make_env(nobj, device, general=general)
  u = env.unwrapped
  n, dev = u.num_envs, u.device
  plan = torch.from_numpy(np.random.default_rng(seed).uniform(-1.1, 1.1, (H, n, 3)).astype(F32)).to(dev)
  kw = dict(K=K, elites=E, iterations=I, sigma=(0.5, 0.5, 0.8), alpha=0.25, std_min=0.05, std_max=0.6)
  c0, steps = int(u._cfg.counter), u.total_step_count
  got = env.rollout_mpc(T, plan, method='cem', temperature=123.0, **kw)
  want = python_loop(twin, T, plan, **kw)
  assert int(u._cfg.counter) == c0 + T == int(twin.unwrapped._cfg.counter) and u.total_step_count == steps + T
  for k in mh.KEYS:
    ta.same(got[k].cpu(), want[k].cpu(), f"rollout_mpc(method='cem') vs the loop ({device}): {k}")
  a, b = tb.make_env(nobj, device, general=general), tb.make_env(nobj, device, general=general)
  mkw = dict(K=K, iterations=I, sigma=(0.5, 0.5, 0.8), temperature=0.5)
  old, ref = a.rollout_mpc(T, plan, **mkw), mh.python_loop(b, T, plan, **mkw)
  for k in mh.KEYS:
    ta.same(old[k].cpu(), ref[k].cpu(), f'rollout_mpc() without a new keyword vs the plan_mppi loop ({device}): {k}')
  same = tb.make_env(nobj, device, general=general).rollout_mpc(T, plan, method='mppi', **mkw)
  for k in mh.KEYS:
    ta.same(same[k].cpu(), old[k].cpu(), f"method='mppi' is the default: {k}")
  for bad in (dict(elites=4), dict(alpha=0.5), dict(std_min=0.1), dict(std_max=1.0), dict(method='cma')):
    try:
      env.rollout_mpc(2, plan, **{**mkw, **bad})
    except ValueError:
      continue
    raise AssertionError(f'{bad} was accepted under mppi')
  try:
    env.rollout_mpc(2, plan, method='cem', discount=0.9, **kw)
  except ValueError:
    pass
  else:
    raise AssertionError("method='cem' took a discount")
  return {k: v.cpu() for k, v in got.items()}

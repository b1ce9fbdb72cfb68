"""Drivers and the reference of earl_tabletop[3]_mpc_rollout (include/earl_tabletop.h, "receding-horizon MPPI control") for tests/test_tabletop_mpc.py
(libearl_host.so) and tests/test_tabletop_mpc_gpu.py (libearl_hip.so); a plain module on tests/tabletop_abi.py's banded buffers and tests/tabletop_plan_helpers.py's
scenes and drivers.

THE REFERENCE is the COMPOSED route through the same library's EXISTING entry points, as the header defines the call: per real step earl_tabletop[3]_plan_mppi
(tabletop_plan_helpers.run_ok; itself pinned to an oracle that shares none of its code) at counter c0 + s and noise_counter + s, earl_tabletop[3]_rollout with T = 1
(tabletop_abi.run_rollout) on the plan's first row, and the shift (zeros for an env that auto-reset) in numpy.  The fused call must equal it in every output, the
final plan and the final state, bit for bit, under both rewards, device against device and host against host.  Device against host twin: bit for bit under the
sparse reward, not compared under the dense one (the device's exp moves the plans apart after the first step).
"""
import copy
import ctypes as C

import numpy as np
import torch

import tabletop_abi as ta
import tabletop_branch_helpers as tb
import tabletop_plan_helpers as h
from earl_benchmark_amd import _abi

F32 = np.float32
OUT4 = ta.OUT4
EXTRA = ('act', 'ret0', 'best_ret')
OUTS = OUT4 + EXTRA                                       # every optional pointer; the plan ('io.plan') is required


# ---------------------------------------------------------------------------------------------------- one call
def run_mpc(side, sc, plan, K, T, fill, I=1, sigma=0.3, inv_t=1.0, nc=7, iteration0=0, null=(), n_call=None, T_call=None, cfg_over=None, out_null=False,
            mpc_null=False, params_null=False, tell=None, value=None):
  """one call -> (rc, results, Bands); results: clones of the state arrays ('st.*'), the optional outputs ('out.*', pre-filled with the pattern) and the plan
  ('io.plan').  Names in `null`: the seven optional outputs, 'plan', the state's arrays.  *_call / cfg_over / tell: what the call is TOLD, the buffers keeping
  their sizes.  value: None = earl_tabletop[3]_mpc_rollout; a tabletop_value_helpers.Value = earl_tabletop[3]_mpc_rollout_value"""
  n, H, D = sc.n, int(plan.shape[0]), sc.obs_dim
  r = ta.Run(side, fill, null)
  st = r.state(sc)
  p = None if 'plan' in r.null else r.put('io.plan', plan, n * 3)
  out = r.out((T, n), D)
  r.blank('out.act', (T, n, 3), torch.float32, n * 3)
  r.blank('out.ret0', (T, I, n), torch.float64, n)
  r.blank('out.best_ret', (T, n), torch.float64, n)
  mpc = _abi.MpcOut(act=r.ptr('out.act'), plan=None if p is None else p.data_ptr(), ret0=r.ptr('out.ret0'), best_ret=r.ptr('out.best_ret'))
  pp = h.told(h.params(K, H, I, sigma, inv_t, nc, iteration0), tell)
  fn, pv, keep = h.entry(side, sc, 'mpc_rollout', value, r)
  cfg = sc.cfg(**(cfg_over or {}))
  if n_call is not None:
    cfg.n = n_call
  rc = fn(C.byref(cfg), C.byref(st), None if params_null else C.byref(pp), *pv, T if T_call is None else T_call, None if out_null else C.byref(out),
          None if mpc_null else C.byref(mpc), side.stream)
  side.sync()
  del keep
  return rc, {k: v[3].clone() for k, v in r.b.bufs.items() if k.startswith(('st.', 'out.', 'io.'))}, r.b


def run_ok(side, sc, plan, K, T, fill, **kw):
  rc, res, b = run_mpc(side, sc, plan, K, T, fill, **kw)
  _abi.check(rc, 'mpc_rollout' if kw.get('value') is None else 'mpc_rollout_value', side.lib)
  return res, b


def assert_untouched(res, sc, plan, what):
  """every output still holds the pattern, the plan and the state are the inputs"""
  ta.assert_untouched({k: v for k, v in res.items() if not k.startswith('io.')}, sc, what)
  if 'io.plan' in res:
    ta.same(res['io.plan'].cpu(), ta._t(plan), f'{what}: the plan')


# ---------------------------------------------------------------------------------------------------- the reference
def after(sc, state, counter):
  """the scene holding `state` (results of a call, 'st.*') at `counter`"""
  new = copy.copy(sc)
  new.state = {k: (state['st.' + k].cpu().numpy().copy() if 'st.' + k in state else sc.state[k]) for k in ta.STATE}
  new.counter = counter
  return new


def shift(plan, done, auto_reset):
  nxt = np.concatenate([plan[1:], plan[-1:]]).astype(F32)
  if auto_reset:
    nxt[:, done.astype(bool)] = 0
  return nxt


def composed(side, sc, plan, K, T, I=1, sigma=0.3, inv_t=1.0, nc=7, iteration0=0, value=None):
  """the header's definition, call by call -> the fused call's results under the same keys, and what the coverage conditions read: 'rets' [T, K, n] (the last
  iteration's returns of each step), 'dones' [T, n], 'plans' [T + 1, H, n, 3] (P_0 .. P_T).  value: the planner of every step is earl_tabletop[3]_plan_mppi_value"""
  cur, P = sc, np.asarray(plan, F32)
  rows = {k: [] for k in OUTS}
  rets, plans = [], [P]
  for s in range(T):
    res, b = h.run_ok(side, cur, P, K, 0x00, I=I, sigma=sigma, inv_t=inv_t, nc=(nc + s) & 0xFFFFFFFF, iteration0=iteration0, value=value)
    b.check('the reference\'s plan_mppi')
    tb.state_untouched(res, cur, 'the reference\'s plan_mppi')
    Pp = res['out.plan'].cpu().numpy()
    out, b = ta.run_rollout(side, cur, np.ascontiguousarray(Pp[:1]), 0x00)
    b.check('the reference\'s rollout')
    for k in OUT4:
      rows[k].append(out['out.' + k].cpu()[0])
    rows['act'].append(ta._t(Pp[0]))
    rows['ret0'].append(res['out.ret0'].cpu())
    rows['best_ret'].append(res['out.best_ret'].cpu())
    rets.append(res['out.ret'].cpu().numpy())
    P = shift(Pp, out['out.done'].cpu().numpy()[0], bool(cur.cfg().auto_reset))
    plans.append(P)
    cur = after(sc, out, sc.counter + s + 1)
  ref = {'out.' + k: torch.stack(v) for k, v in rows.items()}
  ref['io.plan'] = ta._t(P)
  ref.update({'st.' + k: ta._t(cur.state[k]) for k in ta.STATE})
  ref.update(rets=np.stack(rets), dones=ref['out.done'].numpy().astype(bool), plans=np.stack(plans), scene=cur)
  return ref


_REF = {}


def reference(side, cs, T, key=None, sc=None, plan=None, K=None, value=None, **over):
  """the composed reference, made once per (case and T, or key; value specification; side); the entry keeps the specification's net alive (tabletop_plan_helpers.reference)"""
  key = ((id(cs), T) if key is None else key, None if value is None else value.key, side.device)
  if key not in _REF:
    _REF[key] = (value, composed(side, cs.sc if sc is None else sc, cs.mean if plan is None else plan, cs.K if K is None else K, T, value=value, **{**cs.kw, **over}))
  return _REF[key][1]


def compare(got, ref, what, skip=()):
  for k, v in got.items():
    if k not in skip:
      ta.same(v.cpu(), ref[k].cpu(), f'{what}: {k}')


def check_coverage(cs, ref, general=False):
  """on the composed reference, before anything is compared"""
  act, plans, rets = ref['out.act'].numpy(), ref['plans'], ref['rets']
  assert bool((act[0] != h.clip(plans[0][0])).any()), 'every executed action is the clipped start plan: the planner moved nothing'
  assert bool((rets.min(1) != rets.max(1)).any()), 'no env whose returns differ across branches at some real step'
  if general:
    dones = ref['dones']
    assert bool(dones.any(0).all()), 'not every env resets inside the launch'
    hit = False
    for s, i in zip(*np.nonzero(dones[:-1])):
      assert not plans[s + 1][:, i].any(), 'the plan of a reset env was not zeroed'
      hit = hit or bool(act[s + 1:, i].any())
    assert hit, 'no env with a non-zero action after its plan was zeroed'
  if cs.rt == 'dense':
    assert bool(any((h.weights(r, cs.kw['inv_t'])[0] == 0).any() for r in rets)), 'no W_k == 0 under the dense reward'


def check_case(side, cs, T, key=None, sc=None, plan=None, K=None, value=None, **over):
  """both fills: bands intact, every output overwritten, the two runs equal; every output, the final plan and the final state equal to the composed reference"""
  sc, plan, K = cs.sc if sc is None else sc, cs.mean if plan is None else plan, cs.K if K is None else K
  ref = reference(side, cs, T, key, sc, plan, K, value, **over)
  what = f'mpc T={T} {cs.what}' + (f' [{key}]' if key is not None else '') + (f' {value.what}' if value is not None else '')
  res = ta.both_fills(run_ok, side, sc, plan, K, T, what=what, value=value, **{**cs.kw, **over})
  compare(res, ref, what)
  return res


def check_pointers(side, cs, T, full):
  """each optional pointer NULL in turn: the others, the plan and the state as in the full call"""
  for name in OUTS:
    what = f'mpc {cs.what} without {name}'
    res = ta.both_fills(run_ok, side, cs.sc, cs.mean, cs.K, T, what=what, null=(name,), **cs.kw)
    assert 'out.' + name not in res and set(res) == set(full) - {'out.' + name}
    compare(res, full, what)


def check_chaining(side, cs, T1=4, T2=5, **over):
  """T1 steps, then T2 from the state and the plan they left, counter and noise_counter moved on by T1 == T1 + T2 steps in one call"""
  kw = {**cs.kw, **over}
  whole = check_case(side, cs, T1 + T2, key=('chain', id(cs), T1 + T2, tuple(sorted(over.items()))), **over)
  a, b = run_ok(side, cs.sc, cs.mean, cs.K, T1, 0x00, **kw)
  b.check('chaining, first call')
  nxt = after(cs.sc, a, cs.sc.counter + T1)
  z, b = run_ok(side, nxt, a['io.plan'].cpu().numpy(), cs.K, T2, 0xFF, **{**kw, 'nc': kw['nc'] + T1})
  b.check('chaining, second call')
  for k in whole:
    if k.startswith('out.'):
      ta.same(torch.cat([a[k].cpu(), z[k].cpu()]), whole[k].cpu(), f'chained calls vs one call: {k}')
    else:
      ta.same(z[k].cpu(), whole[k].cpu(), f'chained calls vs one call: {k}')


def check_shards(side, cs, T):
  """two shards (0..40, 40..70, env_offset moving with them) == the batch"""
  full = check_case(side, cs, T)
  for lo, hi in ((0, 40), (40, 70)):
    part, b = run_ok(side, tb.shard(cs.sc, lo, hi), np.ascontiguousarray(cs.mean[:, lo:hi]), cs.K, T, 0x00, **cs.kw)
    b.check(f'shard {lo}..{hi}')
    for k, v in part.items():
      whole = full[k].cpu()
      env_axis = 0 if k.startswith('st.') else (2 if k == 'out.ret0' else 1)
      ta.same(v.cpu(), whole.narrow(env_axis, lo, hi - lo).contiguous(), f'shard {lo}..{hi}: {k}')


def check_sigma_zero(side, cs, T):
  """no noise: the plan never moves, the actions are the clipped start plan shifted (its last row repeated)"""
  res = check_case(side, cs, T, key=('sigma 0', id(cs), T), sigma=0.0)
  m = h.clip(cs.mean)
  want = np.stack([m[min(s, cs.H - 1)] for s in range(T)])
  assert not reference(side, cs, T, key=('sigma 0', id(cs), T))['dones'].any()
  ta.same(res['out.act'].cpu(), ta._t(want), 'sigma = 0: the actions')


def check_nan_state(side, nobj, T=4, env=9):
  """a NaN in one env's state under the dense reward: every return of that env is NaN, no branch has a weight, the env executes its clipped start plan; and the
  other envs are as in the clean batch"""
  cs = h.case(nobj, 'dense')
  clean = check_case(side, cs, T)
  sc = tb.with_cfg(cs.sc)
  sc.state = {k: v.copy() for k, v in cs.sc.state.items()}
  sc.state['qpos'][env, 2] = np.nan
  ref = reference(side, cs, T, key=('NaN state', nobj, T), sc=sc)
  assert bool(np.isnan(ref['rets'][:, :, env]).all()), 'the NaN of the state does not reach the returns'
  res = check_case(side, cs, T, key=('NaN state', nobj, T), sc=sc)
  m = h.clip(cs.mean)
  ta.same(res['out.act'][:, env].cpu(), ta._t(np.stack([m[min(s, cs.H - 1), env] for s in range(T)])), 'the NaN env executes its clipped start plan')
  assert bool((res['out.best_ret'][:, env] == -np.inf).all())
  others = [i for i in range(cs.n) if i != env]
  for k, v in res.items():
    env_axis = 0 if k.startswith('st.') else (2 if k == 'out.ret0' else 1)
    ta.same(v.cpu().index_select(env_axis, torch.tensor(others)), clean[k].cpu().index_select(env_axis, torch.tensor(others)), f'the NaN env\'s neighbours: {k}')


def check_device_vs_host(cs, T, dev, host):
  assert cs.rt == 'sparse'
  d, b = run_ok(dev, cs.sc, cs.mean, cs.K, T, 0x00, **cs.kw)
  b.check(cs.what + ' device')
  hh, b = run_ok(host, cs.sc, cs.mean, cs.K, T, 0x00, **cs.kw)
  b.check(cs.what + ' host')
  compare(d, hh, cs.what + ' device vs host')


# ---------------------------------------------------------------------------------------------------- refusals and empty work
def refusals(cs):
  out = [(what, kw) for what, kw in h.refusals(cs) if what not in ('mean NULL', 'ret NULL', 'plan overlaps mean from above', 'plan overlaps mean from below')]
  out += [('out NULL', dict(out_null=True)), ('every pointer of out NULL', dict(null=OUT4)), ('mpc NULL', dict(mpc_null=True)), ('T < 0', dict(T_call=-1)),
          ('K = 1025', dict(tell=dict(K=1025))), ('H = 257', dict(tell=dict(H=257)))]
  return out


def check_refusals(side, cs, T=3):
  for what, kw in refusals(cs):
    rc, res, b = run_mpc(side, cs.sc, cs.mean, cs.K, T, 0xFF, **{**cs.kw, **kw})
    assert rc == -1, f'mpc {cs.what} {what}: rc = {rc}'
    assert side.lib.earl_last_error(), what
    b.check(f'mpc {cs.what} {what}')
    assert_untouched(res, cs.sc, cs.mean, f'mpc {cs.what} {what}')
  big = ta.Scene(2, nobj=cs.nobj)                             # grids: told n, nothing that large allocated
  plan = np.zeros((1, 2, 3), F32)
  for what, n_call, told in (('2^32 lanes', 2**26, dict(K=64)), ('2^32 lanes of sixteen waves', 2**22, dict(K=1024))):
    rc, res, b = run_mpc(side, big, plan, 1, 1, 0xFF, n_call=n_call, tell=told)
    assert rc == -1 and b'launch' in side.lib.earl_last_error(), what
    assert_untouched(res, big, plan, what)
  for fn in ('earl_tabletop_mpc_rollout', 'earl_tabletop3_mpc_rollout'):
    assert getattr(side.lib, fn)(None, None, None, 1, None, None, side.stream) == -1


def check_empty(side, cs, T=3):
  """n == 0, T == 0: EARL_OK, nothing written"""
  for what, kw in (('n = 0', dict(n_call=0)), ('T = 0', dict(T_call=0))):
    for fill in ta.FILLS:
      rc, res, b = run_mpc(side, cs.sc, cs.mean, cs.K, T, fill, **{**cs.kw, **kw})
      assert rc == 0, f'mpc {what}: rc = {rc}'
      b.check('mpc ' + what)
      assert_untouched(res, cs.sc, cs.mean, 'mpc ' + what)


# ---------------------------------------------------------------------------------------------------- through Python
KEYS = ('obs', 'reward', 'done', 'success', 'actions', 'plan', 'ret0', 'best_ret')


def python_loop(env, T, plan, **kw):
  """the loop the call replaces, on the public methods"""
  rows = {k: [] for k in KEYS if k != 'plan'}
  plan = plan.clone()
  for _ in range(T):
    got = env.plan_mppi(plan, **kw)
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


def check_python(device, nobj, general=False, T=5, K=4, H=6, I=2, seed=3):
  """rollout_mpc == the hand-written loop on a second env built alike (default noise_counter: the env's counter); counters and total_step_count advance by T; the
  `out=` rules"""
  env, twin = tb.make_env(nobj, device, general=general), tb.make_env(nobj, device, general=general)
  u = env.unwrapped
  n, dev = u.num_envs, u.device
  plan = torch.from_numpy(np.random.default_rng(seed).uniform(-1.1, 1.1, (H, n, 3)).astype(F32)).to(dev)
  kw = dict(K=K, iterations=I, sigma=(0.5, 0.5, 0.8), temperature=0.5)
  c0, steps = int(u._cfg.counter), u.total_step_count
  keep = plan.clone()
  got = env.rollout_mpc(T, plan, **kw)
  ta.same(plan, keep, 'rollout_mpc wrote the plan it was given without being asked to')
  want = python_loop(twin, T, plan, **kw)
  assert int(u._cfg.counter) == c0 + T == int(twin.unwrapped._cfg.counter) and u.total_step_count == steps + T
  assert {k: (tuple(v.shape), v.dtype) for k, v in got.items()} == {
      'obs': ((T, n, u.OBS_DIM), torch.float32), 'reward': ((T, n), torch.float32), 'done': ((T, n), torch.bool), 'success': ((T, n), torch.bool),
      'actions': ((T, n, 3), torch.float32), 'plan': ((H, n, 3), torch.float32), 'ret0': ((T, I, n), torch.float64), 'best_ret': ((T, n), torch.float64)}
  for k in KEYS:
    ta.same(got[k].cpu(), want[k].cpu(), f'rollout_mpc vs the loop ({device}): {k}')
  after_env, after_twin = tb.snapshot(env), tb.snapshot(twin)
  for k, v in after_env.items():
    if torch.is_tensor(v):
      ta.same(v, after_twin[k], f'rollout_mpc vs the loop ({device}): env {k}')
    else:
      assert v == after_twin[k], (k, v, after_twin[k])
  # out=: in place on the plan; a missing or None key is not computed; the next call carries on where the loop does
  res = env.rollout_mpc(2, got['plan'], out={'plan': got['plan'], 'reward': torch.empty(2, n, device=dev), 'ret0': None}, **kw)
  assert set(res) == {'plan', 'reward'} and res['plan'] is got['plan']
  more = python_loop(twin, 2, want['plan'], **kw)
  ta.same(res['reward'].cpu(), more['reward'].cpu(), 'the second call, in place on the plan: reward')
  ta.same(res['plan'].cpu(), more['plan'].cpu(), 'the second call, in place on the plan: plan')
  zeros = env.rollout_mpc(1, horizon=H, K=K, sigma=0.0)
  assert bool((zeros['actions'] == 0).all()) and bool((zeros['plan'] == 0).all())
  twin.rollout(torch.zeros(1, n, 3, device=dev))
  buf = got['plan']
  for bad in ({'plan': buf[:, :, :2]}, {'plan': buf, 'reward': torch.empty(2, n, dtype=torch.float64, device=dev)}, {'plan': buf, 'nope': buf}, {'plan': buf, 'actions': torch.empty(2, n, 3, device=dev)}):
    try:
      env.rollout_mpc(2, buf, out=bad, **kw)
    except ValueError:
      continue
    raise AssertionError(f'out = {list(bad)} was accepted')
  for bad in (dict(T=0), dict(K=1025), dict(plan=buf[:, :-1])):
    try:
      env.rollout_mpc(**{**dict(T=2, plan=buf), **kw, **bad})
    except ValueError:
      continue
    raise AssertionError(f'{bad} was accepted')
  return {k: v.cpu() for k, v in got.items()}

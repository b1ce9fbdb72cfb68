"""The Sawyer door / peg MPPI planner (include/earl_physics.h: earl_sawyer_plan_mppi, earl_sawyer_plan_candidates, earl_sawyer_plan_ws_bytes), what can be held without
a GPU:
  1. the candidates twin (earl_sawyer_plan_candidates_cpu: the candidates kernel's per-element function) equals the Python oracle of tests/sawyer_plan_helpers.py bit
     for bit, with the coverage conditions asserted on the oracle's own output;
  2. the update twin (earl_sawyer_plan_update_cpu: the update kernel's per-element functions) equals items 4 - 7 in Python integers on synthetic returns -- distinct,
     tied, NaN, all NaN, -Inf, all -Inf, a tiny and a huge temperature -- and, at K = 8192, the int64 oracle;
  3. three candidate / update rounds chained through the twins, in place, equal the oracle's and the rounds run one at a time;
  4. every refusal of the header's list returns EARL_ERR_ARG before the entry point touches the device (host stand-in pointers, as tests/test_sawyer_branches.py does);
     the workspace size query; the struct as gcc sees it; the Python front end's argument errors and its refusal on the envs without a planner;
  5. both kernels of csrc/sawyer_plan.hip compile for gfx950 without scratch and without AGPRs, and the unit holds nothing else.
The GPU side is tests/test_sawyer_plan_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_build
import sawyer_plan_helpers as sp
from conftest import REPO
from earl_benchmark_amd import _abi
from test_physics_abi import EARL_ERR_ARG, host_ptr, sawyer_args

F32, F64 = np.float32, np.float64
N, OFF, K, H, SEED, NC = 5, 3, 4, 6, 0x1234567890ABCDEF, 0x9E3779B9


def nasty_mean(seed=2, H=H, n=N):
  """entries beyond +-1, close to the faces, a NaN and both infinities"""
  mean = np.random.default_rng(seed).uniform(-1.15, 1.15, (H, n, 4)).astype(F32)
  mean[0, 1 % n, 0], mean[1 % H, 2 % n, 3], mean[2 % H, 3 % n, 1] = np.nan, np.inf, -np.inf
  return mean


# ---------------------------------------------------------------------------------------------------------------- 1. candidates
@pytest.mark.parametrize('j', [0, 255])
@pytest.mark.parametrize('sigma', [0.5, (0.5, 0.0, 0.8, 0.3)], ids=['scalar', 'vector'])
def test_candidates_twin_equals_the_oracle(j, sigma):
  host = _abi.load_host()
  mean = nasty_mean()
  want, m, tail = sp.candidates(SEED, OFF, N, K, H, j, sigma, NC, mean)
  # coverage, on the oracle
  assert bool(tail.any()) and bool((~tail).any()), 'the quantile took one branch only'
  inside = np.abs(m) < 1
  assert bool(((want[1:] == 1) & inside[None]).any()) and bool(((want[1:] == -1) & inside[None]).any()), 'no candidate component clipped at each bound'
  assert bool((np.abs(mean) > 1).any()) and np.isfinite(want).all()
  sp.same_bits(want[0], sp.clip(mean), 'row 0 is the clipped mean')
  assert m[0, 1, 0] == -1 and m[1, 2, 3] == 1 and m[2, 3, 1] == -1                      # NaN -> -1, +-Inf -> +-1
  if not np.isscalar(sigma):
    sp.same_bits(want[:, :, :, 1], np.broadcast_to(m[None, :, :, 1], (K, H, N)), 'sigma = 0 in one dimension: the clipped mean')
    assert bool((want[1:, :, :, 3] != m[None, :, :, 3]).any())                          # (the gripper word is drawn and clipped like the others)
  got = sp.host_candidates(host, sp.cfg_of(N, OFF, SEED), sp.params(K, H, sigma=sigma, nc=NC), j, mean)
  sp.same_bits(got, want, f'candidates of iteration {j}')


def test_candidates_depend_on_the_global_id_and_the_counters_only():
  host = _abi.load_host()
  mean = nasty_mean()
  full = sp.host_candidates(host, sp.cfg_of(N, OFF, SEED), sp.params(K, H, sigma=0.5, nc=NC), 1, mean)
  part = sp.host_candidates(host, sp.cfg_of(2, OFF + 3, SEED), sp.params(K, H, sigma=0.5, nc=NC), 1, mean[:, 3:])
  sp.same_bits(part, full[:, :, 3:], 'a shard of two envs')
  for other in (sp.host_candidates(host, sp.cfg_of(N, OFF, SEED), sp.params(K, H, sigma=0.5, nc=NC + 1), 1, mean),
                sp.host_candidates(host, sp.cfg_of(N, OFF, SEED), sp.params(K, H, sigma=0.5, nc=NC), 2, mean),
                sp.host_candidates(host, sp.cfg_of(N, OFF, SEED + 1), sp.params(K, H, sigma=0.5, nc=NC), 1, mean)):
    sp.same_bits(other[0], full[0], 'row 0')
    assert not np.array_equal(other[1:], full[1:])


# ---------------------------------------------------------------------------------------------------------------- 2. update
def synthetic_returns(K, rng):
  """[K, 7]: env 0 distinct, 1 ties for the maximum, 2 one NaN, 3 all NaN, 4 one -Inf, 5 all -Inf, 6 the NaN where the maximum would have been"""
  ret = rng.uniform(0.0, 3.0, (K, 7))
  ret[[1, K - 2], 1] = 5.0
  ret[2, 2] = np.nan
  ret[:, 3] = np.nan
  ret[1, 4] = -np.inf
  ret[:, 5] = -np.inf
  ret[0, 6] = np.nan
  return ret


@pytest.mark.parametrize('inv_t', [1.0, 1e9, 1e-9])
@pytest.mark.parametrize('in_place', [False, True])
def test_update_twin_equals_python_integers(inv_t, in_place):
  host = _abi.load_host()
  K, H, n = 6, 3, 7
  mean = nasty_mean(3, H, n)
  act, m, _ = sp.candidates(SEED, OFF, n, K, H, 4, (0.5, 0.5, 0.8, 0.4), NC, mean)
  ret = synthetic_returns(K, np.random.default_rng(5))
  want = sp.oracle_update(act, m, ret, inv_t)
  W = want['W']
  # the cases, on the oracle
  assert want['best_k'].tolist() == [int(np.argmax(ret[:, 0])), 1, int(np.nanargmax(ret[:, 2])), 0, int(np.argmax(ret[:, 4])), 0, int(np.nanargmax(ret[:, 6]))]
  assert W[2, 2] == 0 and (W[:, 3] == 0).all() and W[1, 4] == 0 and (W[:, 5] == 0).all() and W[0, 6] == 0
  assert want['best_ret'][3] == -np.inf and want['best_ret'][5] == -np.inf and want['best_ret'][1] == 5.0
  sp.same_bits(want['plan'][:, [3, 5]], m[:, [3, 5]], 'no weight: the update is skipped')
  if inv_t == 1e9:
    assert (W[:, 0] != 0).sum() == 1 and (W[:, 1] != 0).sum() == 2                       # one nonzero weight (two for the tie)
    # one weight: the plan is that candidate, up to the 2^-21 of the integer delta's rounding and two float32 roundings near 1
    assert np.abs(want['plan'][:, 0].astype(F64) - act[want['best_k'][0], :, 0]).max() <= 2.0**-21 + 2.0**-23
  elif inv_t == 1e-9:
    assert (W[:, 0] == 2**24).all() and (W[[0, 2, 3, 4, 5], 4] == 2**24).all()           # all weights 2^24
  else:
    assert len(np.unique(W[:, 0])) == K and bool((want['plan'][:, 0] != m[:, 0]).any())
  got = sp.host_update(host, sp.cfg_of(n, OFF, SEED), sp.params(K, H, inv_t=inv_t), 4, mean, act, ret, in_place=in_place)
  for k in ('plan', 'best_ret', 'best_k'):
    sp.same_bits(got[k], want[k], f'{k} (inv_temperature {inv_t})')
  assert np.array_equal(np.isnan(got['ret0']), np.isnan(want['ret0'])) and np.array_equal(got['ret0'][~np.isnan(got['ret0'])], want['ret0'][~np.isnan(want['ret0'])])


def test_update_twin_at_the_largest_K():
  host = _abi.load_host()
  K, H, n = _abi.SAWYER_PLAN_MAX_K, 2, 2
  assert K == 8192
  mean = nasty_mean(4, H, n)
  act, m, _ = sp.candidates(SEED, OFF, n, K, H, 0, 0.7, NC, mean)
  ret = np.random.default_rng(6).normal(0.0, 2.0, (K, n))
  ret[17, 1] = np.nan
  want = sp.oracle_update(act, m, ret, 0.5, fast=True)
  assert bool((want['plan'] != m).any()) and len(np.unique(want['W'])) > 1000
  got = sp.host_update(host, sp.cfg_of(n, OFF, SEED), sp.params(K, H, inv_t=0.5), 0, mean, act, ret)
  for k in ('plan', 'best_ret', 'best_k', 'ret0'):
    sp.same_bits(got[k], want[k], k + ' at K = 8192')


# ---------------------------------------------------------------------------------------------------------------- 3. chaining
def test_three_rounds_through_the_twins():
  """I = 3 rounds of candidates -> (synthetic returns) -> update through the twins, in place on one buffer, equal the oracle's three rounds; and each round run on its
  own from the plan that entered it (iteration0 = j, out of place) gives the same bits"""
  host = _abi.load_host()
  K, n, j0, sigma, inv_t = 5, N, 7, (0.4, 0.5, 0.6, 0.3), 2.0
  cfg = sp.cfg_of(n, OFF, SEED)
  rets = [np.random.default_rng(10 + i).uniform(0.0, 2.0, (K, n)) for i in range(3)]
  plan, entering = nasty_mean(5), []
  for i in range(3):                                                                     # the oracle
    entering.append(plan)
    act, m, _ = sp.candidates(SEED, OFF, n, K, H, j0 + i, sigma, NC, plan)
    plan = sp.oracle_update(act, m, rets[i], inv_t)['plan']
  assert not np.array_equal(entering[1], entering[2]) and not np.array_equal(entering[2], plan)
  buf = nasty_mean(5)
  for i in range(3):                                                                     # the twins, chained in place
    pp = sp.params(K, H, sigma=sigma, inv_t=inv_t, nc=NC)
    act = sp.host_candidates(host, cfg, pp, j0 + i, buf)
    buf = sp.host_update(host, cfg, pp, j0 + i, buf, act, rets[i], in_place=True)['plan']
    if i < 2:
      sp.same_bits(buf, entering[i + 1], f'the plan after round {i}')
  sp.same_bits(buf, plan, 'three chained rounds')
  for i in range(3):                                                                     # one at a time
    pp = sp.params(K, H, sigma=sigma, inv_t=inv_t, nc=NC, iteration0=j0 + i)
    act = sp.host_candidates(host, cfg, pp, j0 + i, entering[i])
    one = sp.host_update(host, cfg, pp, j0 + i, entering[i], act, rets[i])['plan']
    sp.same_bits(one, entering[i + 1] if i < 2 else plan, f'round {i} on its own')


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def ws_bytes(lib, nv, K, H, n):
  need = C.c_int64(-1)
  rc = lib.earl_sawyer_plan_ws_bytes(nv, K, H, n, C.byref(need))
  return rc, need.value


MEAN = host_ptr(1 << 16)


def call(lib, nv, cfg, st, tell=None, model='given', params='given', mean=MEAN, plan='other', ret='given', ws='given', ws_bytes_=1 << 40, ws_base=None):
  """earl_sawyer_plan_mppi on host stand-in pointers: only for calls that return before anything reads through them.  tell: fields of earl_sawyer_plan_params"""
  pp = sp.params(2, 3, I=1, sigma=0.3, inv_t=1.0)
  for k, v in (tell or {}).items():
    setattr(pp, k, (C.c_float * 4)(*v) if k == 'sigma' else v)
  w = None if ws is None else _abi.SawyerBranchWs(base=(host_ptr() if ws_base is None else ws_base) if ws == 'given' else None, bytes=ws_bytes_)
  pl = {'other': host_ptr(1 << 16), 'same': mean, None: None}.get(plan, plan)
  return lib.earl_sawyer_plan_mppi(host_ptr() if model == 'given' else None, None, nv, C.byref(cfg), C.byref(st), C.byref(pp) if params == 'given' else None, mean, pl,
                                   host_ptr() if ret == 'given' else None, host_ptr(), host_ptr(), host_ptr(), host_ptr(), None, None if w is None else C.byref(w), None)


@pytest.mark.parametrize('nv', [10, 15])
def test_every_refusal_fires_before_the_device(nv):
  """n = 4 and K = 2: an accepted call would launch, so every EARL_ERR_ARG below was decided on the host"""
  lib = _abi.load()
  nan, inf = float('nan'), float('inf')
  ok = lambda **kw: sawyer_args(n=4, nv=nv, **kw)[:2]
  cfg, st = ok()
  # what earl_sawyer_branch_rollout refuses in model / cfg / st / nv
  assert call(lib, nv, cfg, st, model=None) == EARL_ERR_ARG
  assert call(lib, 12, cfg, st) == EARL_ERR_ARG and call(lib, 23, cfg, st) == EARL_ERR_ARG
  for bad in (ok(gcf=3, with_sgc=False), ok(n_goal_rows=2), sawyer_args(n=-1, nv=nv)[:2]):
    assert call(lib, nv, *bad) == EARL_ERR_ARG
  c2, s2 = ok()
  s2.qpos = None
  assert call(lib, nv, c2, s2) == EARL_ERR_ARG
  if nv == 15:
    c2, s2 = ok(reward_type=1, att_grasp=4, att_lpad=5, att_rpad=6)
    s2.obj_init = None
    assert call(lib, nv, c2, s2) == EARL_ERR_ARG                                         # peg dense reward without obj_init
  assert lib.earl_sawyer_plan_mppi(host_ptr(), None, nv, None, C.byref(st), C.byref(sp.params(2, 3)), MEAN, host_ptr(), host_ptr(), None, None, None, None, None,
                                   C.byref(_abi.SawyerBranchWs(base=host_ptr(), bytes=1 << 40)), None) == EARL_ERR_ARG      # cfg NULL
  assert lib.earl_sawyer_plan_mppi(host_ptr(), None, nv, C.byref(cfg), None, C.byref(sp.params(2, 3)), MEAN, host_ptr(), host_ptr(), None, None, None, None, None,
                                   C.byref(_abi.SawyerBranchWs(base=host_ptr(), bytes=1 << 40)), None) == EARL_ERR_ARG      # st NULL
  # the planner's own
  for kw in (dict(params=None), dict(mean=None), dict(plan=None), dict(ret=None), dict(ws=None)):
    assert call(lib, nv, cfg, st, **kw) == EARL_ERR_ARG, kw
  for tell in (dict(K=0), dict(K=-1), dict(K=_abi.SAWYER_PLAN_MAX_K + 1), dict(H=0), dict(H=-1), dict(H=65537), dict(iterations=0), dict(iteration0=-1),
               dict(iteration0=250, iterations=7), dict(iteration0=2**31 - 1, iterations=2**31 - 1), dict(sigma=(0.1, -0.1, 0.1, 0.1)), dict(sigma=(0.1, 0.1, 0.1, -0.1)),
               dict(sigma=(0.1, 0.1, nan, 0.1)), dict(sigma=(inf, 0.1, 0.1, 0.1)), dict(inv_temperature=0.0), dict(inv_temperature=-1.0), dict(inv_temperature=nan),
               dict(inv_temperature=inf)):
    assert call(lib, nv, cfg, st, tell=tell) == EARL_ERR_ARG, tell
    assert lib.earl_last_error()
  assert call(lib, nv, cfg, st, plan=MEAN + 16) == EARL_ERR_ARG and call(lib, nv, cfg, st, plan=MEAN - 16) == EARL_ERR_ARG      # a partial overlap (H n 16 = 192 bytes)
  assert call(lib, nv, cfg, st, plan=MEAN + 3 * 4 * 16 - 4) == EARL_ERR_ARG
  big, bst = sawyer_args(n=1 << 19, nv=nv)[:2]
  assert call(lib, nv, big, bst, tell=dict(K=4096)) == EARL_ERR_ARG                      # K n = 2^31
  # the workspace block
  need = ws_bytes(lib, nv, 2, 3, 4)[1]
  assert need > 0 and call(lib, nv, cfg, st, ws_bytes_=need - 1) == EARL_ERR_ARG         # too small
  assert call(lib, nv, cfg, st, ws='null base') == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, ws_base=host_ptr(1 << 16) + 4) == EARL_ERR_ARG           # misaligned


@pytest.mark.parametrize('nv', [10, 15])
def test_the_empty_call_and_the_lane_switch(nv):
  lib = _abi.load()
  zero, zst, _ = sawyer_args(n=0, nv=nv)
  assert call(lib, nv, zero, zst) == _abi.EARL_OK
  assert call(lib, nv, zero, zst, ws='null base', ws_bytes_=0) == _abi.EARL_OK           # (no virtual env: no block needed)
  assert call(lib, nv, zero, zst, plan='same') == _abi.EARL_OK
  assert call(lib, nv, zero, zst, tell=dict(K=0)) == EARL_ERR_ARG                        # (the parameter rules hold for an empty batch too)
  cfg, st, _ = sawyer_args(n=4, nv=nv)
  assert lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
  try:
    assert call(lib, nv, cfg, st) == EARL_ERR_ARG
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK


def test_candidates_refusals_on_both_libraries():
  lib, host = _abi.load(), _abi.load_host()
  nan = float('nan')
  act = host_ptr(1 << 16)
  assert act % 16 == 0 or (act + 8) % 16 == 0
  act += act % 16

  def both(cfg, pp, j, mean, out):
    a = lib.earl_sawyer_plan_candidates(None if cfg is None else C.byref(cfg), None if pp is None else C.byref(pp), j, mean, out, None)
    b = host.earl_sawyer_plan_candidates_cpu(None if cfg is None else C.byref(cfg), None if pp is None else C.byref(pp), j, mean, out)
    assert a == b, (a, b)
    return a

  cfg, pp = sp.cfg_of(4), sp.params(2, 3)
  for args in ((None, pp, 0, MEAN, act), (cfg, None, 0, MEAN, act), (cfg, pp, 0, None, act), (cfg, pp, 0, MEAN, None), (cfg, pp, -1, MEAN, act), (cfg, pp, 256, MEAN, act),
               (sp.cfg_of(-1), pp, 0, MEAN, act), (cfg, sp.params(0, 3), 0, MEAN, act), (cfg, sp.params(_abi.SAWYER_PLAN_MAX_K + 1, 3), 0, MEAN, act),
               (cfg, sp.params(2, 0), 0, MEAN, act), (cfg, sp.params(2, 65537), 0, MEAN, act), (cfg, sp.params(2, 3, sigma=(0.1, 0.1, 0.1, nan)), 0, MEAN, act),
               (cfg, sp.params(2, 3, sigma=-0.5), 0, MEAN, act), (sp.cfg_of(1 << 19), sp.params(4096, 3), 0, MEAN, act)):
    assert both(*args) == EARL_ERR_ARG, args
  assert lib.earl_sawyer_plan_candidates(C.byref(cfg), C.byref(pp), 0, MEAN, act + 4, None) == EARL_ERR_ARG      # the device call stores 16 bytes per lane
  assert both(sp.cfg_of(0), pp, 0, MEAN, act) == _abi.EARL_OK                                                      # n == 0: nothing written
  # the update twin: the planner's rules for what it reads
  upd = lambda cfg, pp, j, mean, a, ret, plan: host.earl_sawyer_plan_update_cpu(None if cfg is None else C.byref(cfg), None if pp is None else C.byref(pp), j, mean, a, ret,
                                                                                plan, None, None, None)
  other, ret = host_ptr(1 << 16), host_ptr()
  for args in ((None, pp, 0, MEAN, act, ret, other), (cfg, None, 0, MEAN, act, ret, other), (cfg, pp, 0, None, act, ret, other), (cfg, pp, 0, MEAN, None, ret, other),
               (cfg, pp, 0, MEAN, act, None, other), (cfg, pp, 0, MEAN, act, ret, None), (cfg, pp, 256, MEAN, act, ret, other), (cfg, pp, 0, MEAN, act, ret, MEAN + 16),
               (cfg, sp.params(2, 3, inv_t=0.0), 0, MEAN, act, ret, other), (cfg, sp.params(2, 3, inv_t=nan), 0, MEAN, act, ret, other),
               (cfg, sp.params(_abi.SAWYER_PLAN_MAX_K + 1, 3), 0, MEAN, act, ret, other)):
    assert upd(*args) == EARL_ERR_ARG, args
  assert upd(sp.cfg_of(0), pp, 0, MEAN, act, ret, other) == _abi.EARL_OK


def test_workspace_size_holds_the_branch_block_and_the_candidates():
  lib = _abi.load()
  for nv in (10, 15):
    for K_, H_, n_ in ((0, 3, 7), (7, 3, 0), (0, 0, 0)):
      assert ws_bytes(lib, nv, K_, H_, n_) == (_abi.EARL_OK, 0)
    grid = [(K_, H_, n_) for K_ in (1, 2, 65, 8192) for H_ in (1, 2, 20) for n_ in (1, 5, 64)]
    sizes = {g: ws_bytes(lib, nv, *g) for g in grid}
    assert all(rc == _abi.EARL_OK and b > 0 for rc, b in sizes.values())
    for a, (_, b) in sizes.items():
      branch = C.c_int64(-1)
      assert lib.earl_sawyer_branch_ws_bytes(nv, a[0], a[2], C.byref(branch)) == _abi.EARL_OK
      assert b >= branch.value + a[0] * a[1] * a[2] * 16 and b % 8 == 0, (nv, a, b)
      for a2, (_, b2) in sizes.items():
        if all(x2 >= x for x2, x in zip(a2, a)) and a2 != a:
          assert b2 > b, (nv, a, a2)
    assert ws_bytes(lib, nv, 1 << 15, 1, 1 << 16)[0] == EARL_ERR_ARG and ws_bytes(lib, nv, -1, 1, 4)[0] == EARL_ERR_ARG
    assert ws_bytes(lib, nv, 1, -1, 4)[0] == EARL_ERR_ARG and ws_bytes(lib, nv, 1, 1, -4)[0] == EARL_ERR_ARG
    assert lib.earl_sawyer_plan_ws_bytes(nv, 1, 1, 1, None) == EARL_ERR_ARG
  assert ws_bytes(lib, 12, 3, 2, 5)[0] == EARL_ERR_ARG
  # the realistic call of the design note: (N, K, H) = (16, 256, 20) is 1.3 MB of candidates
  assert 16 * 256 * 20 * 16 == 1310720


def test_params_struct_matches_what_gcc_sees(tmp_path):
  fields = [f[0] for f in _abi.SawyerPlanParams._fields_]
  src = ('#include <stdio.h>\n#include <stddef.h>\n#include "earl_physics.h"\nint main(void) {\nprintf("%zu %d", sizeof(earl_sawyer_plan_params), EARL_SAWYER_PLAN_MAX_K);\n'
         + '\n'.join(f'printf(" %zu", offsetof(earl_sawyer_plan_params, {f}));' for f in fields) + '\nprintf("\\n");\nreturn 0; }\n')
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src)
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  tok = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
  assert tok[0] == C.sizeof(_abi.SawyerPlanParams) and tok[1] == _abi.SAWYER_PLAN_MAX_K and tok[2:] == [getattr(_abi.SawyerPlanParams, f).offset for f in fields]


def bare(cls, n=3):
  import torch
  env = object.__new__(cls)                                                # (no GPU here: the argument errors need no state)
  env.num_envs, env.device, env.total_step_count = n, torch.device('cpu'), 0
  return env


def test_python_argument_errors():
  import torch
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  for cls in (SawyerDoor, SawyerPeg):
    env = bare(cls)
    mean = torch.zeros(4, 3, 4)
    for kw in (dict(), dict(mean=torch.zeros(4, 3, 3)), dict(mean=torch.zeros(4, 2, 4)), dict(mean=mean, horizon=5), dict(mean=mean, sigma=(0.1, 0.2, 0.3)),
               dict(mean=mean, temperature=0.0), dict(mean=mean, K=0), dict(mean=mean, K=_abi.SAWYER_PLAN_MAX_K + 1), dict(mean=mean, iterations=0),
               dict(mean=mean, out={'nope': mean}), dict(mean=mean, out={'ret0': torch.zeros(1, 3, dtype=torch.float64)}), dict(mean=mean, out={'plan': torch.zeros(4, 3, 3)}),
               dict(mean=mean, K=4, out={'plan': mean, 'ret': torch.zeros(4, 3)}), dict(mean=mean, K=4, out={'plan': mean, 'fail': torch.zeros(4, 3, dtype=torch.int64)})):
      with pytest.raises(ValueError):
        env.plan_mppi(**kw)
    for args, kw in (((torch.zeros(4, 3, 3), 4), {}), ((mean, 0), {}), ((mean, 4), dict(sigma=(1.0, 2.0)))):
      with pytest.raises(ValueError):
        env.plan_candidates(*args, **kw)
    for kw in (dict(T=0, horizon=4), dict(T=2), dict(T=2, plan=torch.zeros(4, 3, 3)), dict(T=2, horizon=4, K=0), dict(T=2, horizon=4, temperature=-1.0)):
      with pytest.raises(ValueError):
        env.mpc_rollout(**kw)


def test_the_base_class_refuses_where_no_planner_is_built():
  from earl_benchmark_amd.envs.kitchen import Kitchen
  from earl_benchmark_amd.envs.minitaur import Minitaur
  from earl_benchmark_amd.envs.physics_env import PhysicsEnv
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  for name in ('plan_mppi', 'plan_candidates', 'mpc_rollout'):
    for cls in (Minitaur, Kitchen):
      assert getattr(cls, name) is getattr(PhysicsEnv, name)
      with pytest.raises(NotImplementedError, match=name + '.*' + cls.ENV):
        getattr(object.__new__(cls), name)(None)
    assert getattr(SawyerPeg, name) is getattr(SawyerDoor, name) is not getattr(PhysicsEnv, name)


# ---------------------------------------------------------------------------------------------------------------- 5. the build
def test_the_two_kernels_compile_without_scratch_and_the_unit_holds_nothing_else():
  unit = kernel_build.unit('sawyer_plan.hip')
  res = unit.resources
  print(res)
  assert sorted(res) == ['sawyer_plan_candidates_kernel', 'sawyer_plan_update_kernel'], sorted(res)
  for name, r in res.items():
    assert r['scratch'] == 0 and r['agpr'] == 0, (name, r)
  assert res['sawyer_plan_candidates_kernel']['lds'] == 0
  assert _abi.SAWYER_PLAN_MAX_K * 4 <= res['sawyer_plan_update_kernel']['lds'] <= 40 * 1024      # one env's int32 weights, and the waves' maxima
  # the object list gains exactly this unit, and the unit is no further inclusion of the stepper or of the rollout kernel's text
  mk = open(os.path.join(kernel_build.CSRC, 'Makefile')).read()
  src = re.search(r'^SRC\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
  assert src.count('sawyer_plan.hip') == 1 and len(src) == len(set(src))
  assert [u for u in src if 'plan' in u and u.startswith(('sawyer', 'physics'))] == ['sawyer_plan.hip']
  text = ''.join(open(os.path.join(kernel_build.CSRC, f)).read() for f in ('sawyer_plan.hip', 'sawyer_plan.h', 'sawyer_shoot.h'))
  assert not re.search(r'#include\s+"physics_', text), 'the planner reaches the branch launch through the public ABI only'
  rollout_text = [f for f in sorted(os.listdir(kernel_build.CSRC)) if f.endswith(('.h', '.hip'))
                  and '#include "physics_env_sawyer_rollout.inc"' in open(os.path.join(kernel_build.CSRC, f)).read()]
  assert rollout_text == ['physics_env_sawyer.h'], rollout_text                          # (three inclusions, all in that header: none was added)
  assert open(os.path.join(kernel_build.CSRC, 'physics_env_sawyer.h')).read().count('#include "physics_env_sawyer_rollout.inc"') == 3

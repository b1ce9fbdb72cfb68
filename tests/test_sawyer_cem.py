"""The Sawyer door / peg CEM planner (include/earl_physics.h, "CEM planning on the door and the peg": earl_sawyer_plan_cem, earl_sawyer_cem_candidates,
earl_sawyer_cem_update), what can be held without a GPU:
  1. the candidates twin (earl_sawyer_cem_candidates_cpu: the candidates kernel's per-element functions) equals the Python oracle of tests/sawyer_cem_helpers.py bit for
     bit, without a std (sigma in every row), with one, and with a NaN and entries outside [std_min, std_max] in it;
  2. the update twin (earl_sawyer_cem_update_cpu) equals items 4 - 7 as a Python sort and Python integers on the crafted returns of sawyer_cem_helpers.patterns --
     all equal, a tie across rank E - 1, all distinct, NaNs (Ne < E), all NaN, +-0, +-Inf, keys that differ in their lowest / highest byte only -- each pattern's own
     condition asserted on the oracle first, for K in {1, 2, 65, 513} and E in {1, a middle value, K}, and at K = 8192 with E = 1024;
  3. the in-place calls (plan is mean, std is std_in), and three rounds chained through the twins equal the oracle's three rounds;
  4. every refusal of the header's list returns EARL_ERR_ARG before the entry point touches the device, on both libraries where both have the call; the struct as gcc
     sees it; EARL_SAWYER_CEM_MAX_E; the Python front end's argument errors and its refusal on the envs without a planner;
  5. both kernels of csrc/sawyer_cem.hip compile for gfx950 without scratch and without AGPRs, the update kernel inside 64 KiB of LDS, and the unit holds nothing else.
The GPU side is tests/test_sawyer_cem_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_build
import sawyer_cem_helpers as sc
from conftest import REPO
from earl_benchmark_amd import _abi
from test_physics_abi import EARL_ERR_ARG, host_ptr, sawyer_args

F32, F64 = np.float32, np.float64
N, OFF, K, H, SEED, NC = 5, 3, 4, 6, 0x1234567890ABCDEF, 0x9E3779B9
LO, HI = 0.05, 0.6


def nasty_mean(seed=2, H=H, n=N):
  """entries beyond +-1, close to the faces, a NaN and both infinities"""
  mean = np.random.default_rng(seed).uniform(-1.15, 1.15, (H, n, 4)).astype(F32)
  mean[0, 1 % n, 0], mean[1 % H, 2 % n, 3], mean[2 % H, 3 % n, 1] = np.nan, np.inf, -np.inf
  return mean


def nasty_std(seed=3, H=H, n=N):
  """entries below std_min and above std_max, a NaN, an infinity and a negative number"""
  std = np.random.default_rng(seed).uniform(-0.1, 0.9, (H, n, 4)).astype(F32)
  std[0, 0, 1], std[1 % H, 1 % n, 2], std[2 % H, 2 % n, 3] = np.nan, np.inf, -1.0
  return std


# ---------------------------------------------------------------------------------------------------------------- 1. candidates
@pytest.mark.parametrize('j', [0, 255])
@pytest.mark.parametrize('with_std', [False, True], ids=['sigma', 'std0'])
def test_candidates_twin_equals_the_oracle(j, with_std):
  host = _abi.load_host()
  mean, sigma = nasty_mean(), (0.5, 0.01, 0.8, 0.3)
  std0 = nasty_std() if with_std else None
  s = sc.sclamp(sc.std_rows(std0, sigma, H, N), LO, HI)
  want, m = sc.candidates(SEED, OFF, N, K, H, j, NC, mean, s)
  # coverage, on the oracle
  assert bool((s >= F32(LO)).all()) and bool((s <= F32(HI)).all())
  if with_std:
    assert s[0, 0, 1] == F32(LO) and s[1, 1, 2] == F32(HI) and s[2, 2, 3] == F32(LO)             # NaN -> std_min, Inf -> std_max, negative -> std_min
    assert len(np.unique(s)) > 20 and bool((std0 > HI).any()) and bool((std0 < LO).any())
  else:
    assert s[0, 0].tolist() == [F32(0.5), F32(LO), F32(HI), F32(0.3)]                            # sigma clamped like a row
  inside = np.abs(m) < 1
  assert bool(((want[1:] == 1) & inside[None]).any()) and bool(((want[1:] == -1) & inside[None]).any()), 'no candidate component clipped at each bound'
  assert np.isfinite(want).all() and bool((want[1:, :, :, 3] != m[None, :, :, 3]).any())         # (the gripper word is drawn like the others)
  sc.same_bits(want[0], sc.clip(mean), 'row 0 is the clipped mean')
  got = sc.host_candidates(host, sc.cfg_of(N, OFF, SEED), sc.params(K, H, sigma=sigma, lo=LO, hi=HI, nc=NC), j, mean, std0)
  sc.same_bits(got, want, f'candidates of iteration {j}')


def test_the_cem_draw_is_its_own_and_a_shard_sees_the_same_noise():
  import sawyer_plan_helpers as sp
  host = _abi.load_host()
  mean = np.clip(nasty_mean(), -0.5, 0.5)
  mean[np.isnan(mean)] = 0.0
  cem = sc.host_candidates(host, sc.cfg_of(N, OFF, SEED), sc.params(K, H, sigma=0.5, nc=NC), 1, mean, None)
  mppi = sp.host_candidates(host, sp.cfg_of(N, OFF, SEED), sp.params(K, H, sigma=0.5, nc=NC), 1, mean)
  sc.same_bits(cem[0], mppi[0], 'row 0')
  assert float((cem[1:] == mppi[1:]).mean()) < 0.05, 'word 0 of the counter: CEM and MPPI draw different noise (equal only where both clip)'
  part = sc.host_candidates(host, sc.cfg_of(2, OFF + 3, SEED), sc.params(K, H, sigma=0.5, nc=NC), 1, mean[:, 3:], None)
  sc.same_bits(part, cem[:, :, 3:], 'a shard of two envs')


# ---------------------------------------------------------------------------------------------------------------- 2. update
def middle(K):
  return {1: 1, 2: 1, 65: 8, 513: 64, 8192: 300}[K]


def check_crafted(update, K, E, H, group, seed, what, std_given=True, in_place=False):
  """one crafted call (three envs, one pattern each): the patterns' conditions on the oracle, then `update` against the oracle; -> the oracle's dict"""
  names = sc.PATTERNS[group]
  mean, std_in, act, ret, holds = sc.crafted(names, K, E, H, seed)
  if not std_given:
    std_in = None
  sigma, alpha = (0.3, 0.02, 0.9, 0.4), 0.25
  s = sc.sclamp(sc.std_rows(std_in, sigma, H, len(names)), LO, HI)
  m = sc.clip(mean)
  want = sc.oracle_update(act, m, s, ret, E, alpha, LO, HI)
  for i, nm in enumerate(names):
    assert holds[i](want['el'][i], ret[:, i]), f'pattern {nm} at K = {K}, E = {E} does not exercise its path'
    if nm == 'all_nan' or (nm == 'nans' and E == 1):
      sc.same_bits(want['plan'][:, i], m[:, i], 'Ne = 0: the mean stays')
      sc.same_bits(want['std'][:, i], s[:, i], 'Ne = 0: the std stays')
      assert want['best_ret'][i] == -np.inf and want['best_k'][i] == 0
    elif K > 2:
      assert bool((want['plan'][:, i] != m[:, i]).any()) or E == 1
  got = update(sc.cfg_of(len(names), OFF, SEED), sc.params(K, H, E=E, sigma=sigma, alpha=alpha, lo=LO, hi=HI), 3, mean, std_in, act, ret, in_place=in_place)
  sc.compare_update(got, want, f'{what}: K = {K}, E = {E}, patterns {names}')
  return want


@pytest.mark.parametrize('K_', [1, 2, 65, 513])
def test_update_twin_equals_the_sort_and_python_integers(K_):
  host = _abi.load_host()
  for E in sorted({1, middle(K_), K_}):
    for group in range(3):
      check_crafted(lambda *a, **kw: sc.host_update(host, *a, **kw), K_, E, 2, group, 100 * K_ + 10 * E + group, 'the update twin', std_given=group != 1)


def test_update_twin_at_the_largest_K_and_the_largest_E():
  host = _abi.load_host()
  assert (sc.MAX_K, sc.MAX_E) == (_abi.SAWYER_PLAN_MAX_K, _abi.SAWYER_CEM_MAX_E) == (8192, 1024)
  for group in range(3):
    check_crafted(lambda *a, **kw: sc.host_update(host, *a, **kw), 8192, 1024, 2, group, 7 + group, 'the update twin')


# ---------------------------------------------------------------------------------------------------------------- 3. in place, chaining
def test_the_in_place_calls():
  host = _abi.load_host()
  for group in range(3):
    check_crafted(lambda *a, **kw: sc.host_update(host, *a, **kw), 65, 8, 9, group, 40 + group, 'plan is mean, std is std_in', in_place=True)
  check_crafted(lambda *a, **kw: sc.host_update(host, *a, **kw), 65, 8, 3, 0, 44, 'plan is mean, no std_in', std_given=False, in_place=True)


def test_three_rounds_through_the_twins():
  """I = 3 rounds of candidates -> (synthetic returns) -> update through the twins, in place on one pair of buffers, equal the oracle's three rounds"""
  host = _abi.load_host()
  K_, E, n, j0, sigma, alpha = 9, 3, N, 7, (0.4, 0.5, 0.6, 0.3), 0.1
  cfg = sc.cfg_of(n, OFF, SEED)
  rets = [np.random.default_rng(10 + i).uniform(0.0, 2.0, (K_, n)) for i in range(3)]
  plan, std, stds = nasty_mean(5), sc.std_rows(None, sigma, H, n), []
  for i in range(3):                                                                     # the oracle
    s = sc.sclamp(std, LO, HI)
    act, m = sc.candidates(SEED, OFF, n, K_, H, j0 + i, NC, plan, s)
    o = sc.oracle_update(act, m, s, rets[i], E, alpha, LO, HI)
    plan, std = o['plan'], o['std']
    stds.append(std)
  assert not np.array_equal(stds[0], stds[1]) and not np.array_equal(stds[1], stds[2]) and len(np.unique(stds[2])) > 20      # the std is refitted per (step, env, dim)
  buf, sbuf = nasty_mean(5), None
  for i in range(3):                                                                     # the twins, chained in place
    pp = sc.params(K_, H, E=E, sigma=sigma, alpha=alpha, lo=LO, hi=HI, nc=NC)
    act = sc.host_candidates(host, cfg, pp, j0 + i, buf, sbuf)
    got = sc.host_update(host, cfg, pp, j0 + i, buf, sbuf, act, rets[i], in_place=True)
    buf, sbuf = got['plan'], got['std']
    sc.same_bits(sbuf, stds[i], f'the std after round {i}')
  sc.same_bits(buf, plan, 'three chained rounds')


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def aligned_ptr(nbytes=4096):
  return (host_ptr(nbytes + 16) + 15) & ~15


MEAN, STD0 = aligned_ptr(), aligned_ptr()


def bad_params():
  nan, inf = float('nan'), float('inf')
  return (dict(K=0), dict(K=-1), dict(K=_abi.SAWYER_PLAN_MAX_K + 1), dict(H=0), dict(H=-1), dict(H=65537), dict(sigma=(0.1, -0.1, 0.1, 0.1)), dict(sigma=(0.1, 0.1, 0.1, nan)),
          dict(sigma=(inf, 0.1, 0.1, 0.1)), dict(std_min=-0.1), dict(std_min=nan), dict(std_max=inf), dict(std_min=0.5, std_max=0.4), dict(std_max=nan))


def bad_update_params():
  nan = float('nan')
  return (dict(elites=0), dict(elites=-1), dict(elites=3), dict(K=2000, elites=_abi.SAWYER_CEM_MAX_E + 1), dict(alpha=1.0), dict(alpha=-0.1), dict(alpha=nan),
          dict(alpha=float('inf')))


def told(tell, K_=2, H_=3):
  pp = sc.params(K_, H_, I=1, E=1)
  for k, v in (tell or {}).items():
    setattr(pp, k, (C.c_float * 4)(*v) if k == 'sigma' else v)
  return pp


def call(lib, nv, cfg, st, tell=None, model='given', params='given', mean=MEAN, std0=None, plan='other', std='other', ret='given', ws='given', ws_bytes_=1 << 40,
         ws_base=None):
  """earl_sawyer_plan_cem on host stand-in pointers: only for calls that return before anything reads through them.  tell: fields of earl_sawyer_cem_params"""
  pp = told(tell)
  w = None if ws is None else _abi.SawyerBranchWs(base=(host_ptr() if ws_base is None else ws_base) if ws == 'given' else None, bytes=ws_bytes_)
  pl = {'other': aligned_ptr(), 'same': mean, None: None}.get(plan, plan)
  sd = {'other': aligned_ptr(), 'same': std0, None: None}.get(std, std)
  return lib.earl_sawyer_plan_cem(host_ptr() if model == 'given' else None, None, nv, C.byref(cfg), C.byref(st), C.byref(pp) if params == 'given' else None, mean, std0, pl, sd,
                                  host_ptr() if ret == 'given' else None, host_ptr(), host_ptr(), host_ptr(), host_ptr(), host_ptr(), None,
                                  None if w is None else C.byref(w), None)


@pytest.mark.parametrize('nv', [10, 15])
def test_every_refusal_fires_before_the_device(nv):
  """n = 4 and K = 2: an accepted call would launch, so every EARL_ERR_ARG below was decided on the host"""
  lib = _abi.load()
  ok = lambda **kw: sawyer_args(n=4, nv=nv, **kw)[:2]
  cfg, st = ok()
  # what earl_sawyer_plan_mppi refuses through the branch launch in model / cfg / st / nv
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
  tail = (MEAN, None, aligned_ptr(), aligned_ptr(), host_ptr(), None, None, None, None, None, None, C.byref(_abi.SawyerBranchWs(base=host_ptr(), bytes=1 << 40)), None)
  assert lib.earl_sawyer_plan_cem(host_ptr(), None, nv, None, C.byref(st), C.byref(told(None)), *tail) == EARL_ERR_ARG      # cfg NULL
  assert lib.earl_sawyer_plan_cem(host_ptr(), None, nv, C.byref(cfg), None, C.byref(told(None)), *tail) == EARL_ERR_ARG     # st NULL
  # the planner's own
  for kw in (dict(params=None), dict(mean=None), dict(plan=None), dict(std=None), dict(ret=None), dict(ws=None)):
    assert call(lib, nv, cfg, st, **kw) == EARL_ERR_ARG, kw
  for tell in bad_params() + bad_update_params() + (dict(iterations=0), dict(iteration0=-1), dict(iteration0=250, iterations=7),
                                                    dict(iteration0=2**31 - 1, iterations=2**31 - 1)):
    assert call(lib, nv, cfg, st, tell=tell) == EARL_ERR_ARG, tell
    assert lib.earl_last_error()
  # the overlaps: H n 16 = 192 bytes per array; (mean, plan) and (std0, std) may coincide, nothing else may touch
  assert call(lib, nv, cfg, st, plan=MEAN + 16) == EARL_ERR_ARG and call(lib, nv, cfg, st, plan=MEAN - 16) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, std0=STD0, std=STD0 + 16) == EARL_ERR_ARG and call(lib, nv, cfg, st, std0=STD0, std=STD0 + 176) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, std=MEAN) == EARL_ERR_ARG and call(lib, nv, cfg, st, std0=MEAN) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, std0=STD0, plan=STD0) == EARL_ERR_ARG and call(lib, nv, cfg, st, plan='same', std=MEAN) == EARL_ERR_ARG
  other = aligned_ptr()
  assert call(lib, nv, cfg, st, plan=other, std=other + 96) == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, plan=aligned_ptr() + 4) == EARL_ERR_ARG and call(lib, nv, cfg, st, std=aligned_ptr() + 8) == EARL_ERR_ARG      # a row is one 16-byte store
  big, bst = sawyer_args(n=1 << 19, nv=nv)[:2]
  assert call(lib, nv, big, bst, tell=dict(K=4096)) == EARL_ERR_ARG                      # K n = 2^31
  # the workspace block: earl_sawyer_plan_ws_bytes' size
  need = C.c_int64(-1)
  assert lib.earl_sawyer_plan_ws_bytes(nv, 2, 3, 4, C.byref(need)) == _abi.EARL_OK and need.value > 0
  assert call(lib, nv, cfg, st, ws_bytes_=need.value - 1) == EARL_ERR_ARG                # too small
  assert call(lib, nv, cfg, st, ws='null base') == EARL_ERR_ARG
  assert call(lib, nv, cfg, st, ws_base=host_ptr(1 << 16) + 4) == EARL_ERR_ARG           # misaligned


@pytest.mark.parametrize('nv', [10, 15])
def test_the_empty_call_and_the_lane_switch(nv):
  lib = _abi.load()
  zero, zst, _ = sawyer_args(n=0, nv=nv)
  assert call(lib, nv, zero, zst) == _abi.EARL_OK
  assert call(lib, nv, zero, zst, ws='null base', ws_bytes_=0) == _abi.EARL_OK           # (no virtual env: no block needed)
  assert call(lib, nv, zero, zst, plan='same', std0=STD0, std='same') == _abi.EARL_OK    # both in-place pairs
  assert call(lib, nv, zero, zst, tell=dict(elites=0)) == EARL_ERR_ARG                   # (the parameter rules hold for an empty batch too)
  cfg, st, _ = sawyer_args(n=4, nv=nv)
  assert lib.earl_debug_set_physics_lanes(64) == _abi.EARL_OK
  try:
    assert call(lib, nv, cfg, st) == EARL_ERR_ARG
  finally:
    assert lib.earl_debug_set_physics_lanes(16) == _abi.EARL_OK


def test_candidates_and_update_refusals_on_both_libraries():
  lib, host = _abi.load(), _abi.load_host()
  act, other, sother, ret = aligned_ptr(), aligned_ptr(), aligned_ptr(), host_ptr()
  ref = lambda x: None if x is None else C.byref(x)

  def cand(cfg, pp, j, mean, std, out):
    a = lib.earl_sawyer_cem_candidates(ref(cfg), ref(pp), j, mean, std, out, None)
    b = host.earl_sawyer_cem_candidates_cpu(ref(cfg), ref(pp), j, mean, std, out)
    assert a == b, (a, b)
    return a

  def upd(cfg, pp, j, mean, std_in, a_, ret_, plan, std):
    a = lib.earl_sawyer_cem_update(ref(cfg), ref(pp), j, mean, std_in, a_, ret_, plan, std, None, None, None, None, None)
    b = host.earl_sawyer_cem_update_cpu(ref(cfg), ref(pp), j, mean, std_in, a_, ret_, plan, std, None, None, None, None)
    assert a == b, (a, b)
    return a

  cfg, pp = sc.cfg_of(4), told(None)
  for args in ((None, pp, 0, MEAN, None, act), (cfg, None, 0, MEAN, None, act), (cfg, pp, 0, None, None, act), (cfg, pp, 0, MEAN, None, None), (cfg, pp, -1, MEAN, None, act),
               (cfg, pp, 256, MEAN, None, act), (sc.cfg_of(-1), pp, 0, MEAN, None, act), (sc.cfg_of(1 << 19), told(None, 4096), 0, MEAN, None, act),
               (cfg, pp, 0, MEAN, MEAN + 16, act)) + tuple((cfg, told(t), 0, MEAN, None, act) for t in bad_params()):
    assert cand(*args) == EARL_ERR_ARG, args
  zero = sc.cfg_of(0)
  assert cand(zero, told(dict(elites=0, alpha=7.0)), 0, MEAN, None, act) == _abi.EARL_OK  # n == 0: nothing written; elites and alpha are not the candidates'
  assert cand(zero, pp, 0, MEAN, STD0, act) == _abi.EARL_OK
  assert lib.earl_sawyer_cem_candidates(C.byref(cfg), C.byref(pp), 0, MEAN, None, act + 4, None) == EARL_ERR_ARG      # the device call stores 16 bytes per lane
  # the update on given candidates and returns
  good = (cfg, pp, 0, MEAN, None, act, ret, other, sother)
  for pos, val in ((0, None), (1, None), (3, None), (5, None), (6, None), (7, None), (8, None), (2, 256), (2, -1), (7, MEAN + 16), (8, MEAN), (7, sother)):
    args = list(good)
    args[pos] = val
    assert upd(*args) == EARL_ERR_ARG, (pos, val)
  assert upd(cfg, pp, 0, MEAN, STD0, act, ret, other, STD0 + 32) == EARL_ERR_ARG and upd(cfg, pp, 0, MEAN, STD0, act, ret, STD0, sother) == EARL_ERR_ARG
  for t in bad_params() + bad_update_params():
    assert upd(cfg, told(t), 0, MEAN, None, act, ret, other, sother) == EARL_ERR_ARG, t
  assert upd(zero, pp, 0, MEAN, None, act, ret, other, sother) == _abi.EARL_OK
  assert upd(zero, pp, 0, MEAN, STD0, act, ret, MEAN, STD0) == _abi.EARL_OK               # both in-place pairs
  assert lib.earl_sawyer_cem_update(C.byref(cfg), C.byref(pp), 0, MEAN, None, act + 8, ret, other, sother, None, None, None, None, None) == EARL_ERR_ARG      # misaligned act
  assert lib.earl_sawyer_cem_update(C.byref(cfg), C.byref(pp), 0, MEAN, None, act, ret, other + 4, sother, None, None, None, None, None) == EARL_ERR_ARG


def test_params_struct_matches_what_gcc_sees(tmp_path):
  fields = [f[0] for f in _abi.SawyerCemParams._fields_]
  src = ('#include <stdio.h>\n#include <stddef.h>\n#include "earl_physics.h"\nint main(void) {\nprintf("%zu %d %d", sizeof(earl_sawyer_cem_params), EARL_SAWYER_CEM_MAX_E, '
         'EARL_SAWYER_PLAN_MAX_K);\n' + '\n'.join(f'printf(" %zu", offsetof(earl_sawyer_cem_params, {f}));' for f in fields) + '\nprintf("\\n");\nreturn 0; }\n')
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src)
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  tok = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
  assert tok[0] == C.sizeof(_abi.SawyerCemParams) and tok[3:] == [getattr(_abi.SawyerCemParams, f).offset for f in fields]
  assert tok[1] == _abi.SAWYER_CEM_MAX_E == 1024 and tok[2] == _abi.SAWYER_PLAN_MAX_K
  assert fields == ['K', 'H', 'iterations', 'iteration0', 'elites', 'sigma', 'noise_counter', 'alpha', 'std_min', 'std_max'] and _abi.SawyerCemParams.sigma.size == 16


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
               dict(mean=mean, K=0), dict(mean=mean, K=_abi.SAWYER_PLAN_MAX_K + 1), dict(mean=mean, iterations=0), dict(mean=mean, K=4, elites=5), dict(mean=mean, elites=0),
               dict(mean=mean, K=2000, elites=1025), dict(mean=mean, alpha=1.0), dict(mean=mean, alpha=-0.5), dict(mean=mean, std_min=-1.0), dict(mean=mean, std_min=1.0, std_max=0.5),
               dict(mean=mean, std_max=float('inf')), dict(mean=mean, std=torch.zeros(4, 3, 3)), dict(mean=mean, std=torch.zeros(5, 3, 4)),
               dict(mean=mean, out={'nope': mean}), dict(mean=mean, out={'ret0': torch.zeros(1, 3, dtype=torch.float64)}), dict(mean=mean, out={'plan': torch.zeros(4, 3, 3)}),
               dict(mean=mean, K=8, out={'plan': mean, 'std': torch.zeros(4, 3, 4, dtype=torch.float64)}),
               dict(mean=mean, K=8, out={'plan': mean, 'elite': torch.zeros(8, 3, dtype=torch.int32)})):
      with pytest.raises(ValueError):
        env.plan_cem(**kw)
    for args, kw in (((torch.zeros(4, 3, 3), 4), {}), ((mean, 0), {}), ((mean, 4), dict(sigma=(1.0, 2.0))), ((mean, 4), dict(std=torch.zeros(4, 3))),
                     ((mean, 4), dict(std_min=2.0, std_max=1.0))):
      with pytest.raises(ValueError):
        env.cem_candidates(*args, **kw)
    for kw in (dict(T=2, horizon=4, method='random'), dict(T=0, horizon=4, method='cem'), dict(T=2, method='cem'), dict(T=2, horizon=4, method='cem', K=4, elites=5),
               dict(T=2, horizon=4, method='cem', alpha=1.0), dict(T=2, horizon=4, method='cem', std_min=-1.0)):
      with pytest.raises(ValueError):
        env.mpc_rollout(**kw)


def test_the_base_class_refuses_where_no_planner_is_built():
  from earl_benchmark_amd.envs.kitchen import Kitchen
  from earl_benchmark_amd.envs.minitaur import Minitaur
  from earl_benchmark_amd.envs.physics_env import PhysicsEnv
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  for name in ('plan_cem', 'cem_candidates'):
    for cls in (Minitaur, Kitchen):
      assert getattr(cls, name) is getattr(PhysicsEnv, name)
      with pytest.raises(NotImplementedError, match=name + '.*CEM.*' + cls.ENV):
        getattr(object.__new__(cls), name)(None)
    assert getattr(SawyerPeg, name) is getattr(SawyerDoor, name) is not getattr(PhysicsEnv, name)
  for cls in (Minitaur, Kitchen):                                           # the existing messages stay as they are
    with pytest.raises(NotImplementedError, match='plan_mppi: the MPPI planner is not built for ' + cls.ENV):
      object.__new__(cls).plan_mppi(None)


# ---------------------------------------------------------------------------------------------------------------- 5. the build
def test_the_two_kernels_compile_without_scratch_and_the_unit_holds_nothing_else():
  unit = kernel_build.unit('sawyer_cem.hip')
  res = unit.resources
  print(res)
  assert sorted(res) == ['sawyer_cem_candidates_kernel', 'sawyer_cem_update_kernel'], sorted(res)
  for name, r in res.items():
    assert r['scratch'] == 0 and r['agpr'] == 0, (name, r)
  assert res['sawyer_cem_candidates_kernel']['lds'] == 0
  assert 0 < res['sawyer_cem_update_kernel']['lds'] <= 65536
  mk = open(os.path.join(kernel_build.CSRC, 'Makefile')).read()
  src = re.search(r'^SRC\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
  assert src.count('sawyer_cem.hip') == 1 and len(src) == len(set(src))
  assert re.search(r'^sawyer_cem\.o:.*\bsawyer_cem\.h\b.*\bcem_select\.h\b', mk, flags=re.M)
  text = ''.join(open(os.path.join(kernel_build.CSRC, f)).read() for f in ('sawyer_cem.hip', 'sawyer_cem.h', 'sawyer_shoot.h', 'cem_select.h'))
  assert not re.search(r'#include\s+"physics_', text), 'the planner reaches the branch launch through the public ABI only'
  select = open(os.path.join(kernel_build.CSRC, 'cem_select.h')).read()
  assert not re.search(r'sawyer|Sawyer|#include\s+"', select), 'the selection names no env and includes no project header: another update kernel can adopt it'

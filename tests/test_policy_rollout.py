"""earl_tabletop_policy_rollout (include/earl_tabletop.h): the closed-loop tabletop rollout with a float32 MLP policy evaluated between the env steps.
Without a GPU, through csrc/libearl_host.so (the kernel's own header, csrc/tabletop_policy.h, compiled for the host):
  1. closed = open, bit for bit: the launch equals the open-loop `_cpu` entry point fed with the actions it recorded;
  2. pinned to the reference: the oracle stepped with the recorded actions reproduces observations, sparse reward and flags exactly;
  3. the actions are the policy's: within the a-priori rounding bound of a float64 evaluation of the same float32 weights, every row; and on one small
     case exactly, against the fmaf chain evaluated in fractions.Fraction with one float32 rounding per step;
  4. tanh_f32 over every float32 in 2^-12 <= |x| <= 16 and a log-spaced sample outside: odd, monotone, bounded, special values, error in ulp;
  5. argument errors from both libraries, and MLPPolicy's limits;
  6. no scratch in any instantiation of the kernel (cross-compiled).
tests/test_policy_rollout_gpu.py holds the device to the host bit for bit."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import hip_harness as hx
import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from oracle import tabletop_oracle as orc

CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')
U = 2.0 ** -24
TANH_ULP_BOUND = 1.0          # asserted bound of tanh_f32 against double tanh, in float32 ulp: the next whole ulp above the sweep's measurement (0.49999999: correctly rounded over the whole sweep)


# ---------------------------------------------------------------------------------------------------------------- helpers (shared with the GPU tests)
class Policy:
  """random ASYMMETRIC weights (no symmetry hides a transposed lane map), packed as struct earl_mlp_policy wants them"""

  def __init__(self, hidden, hidden_act='relu', out_act='tanh', seed=0, gain=1.0, device='cpu'):
    rng = np.random.default_rng(seed)
    self.dims = [12] + list(hidden) + [3]
    self.hidden_act, self.out_act = hidden_act, out_act
    self.layers = []
    for l, (k, n) in enumerate(zip(self.dims[:-1], self.dims[1:])):
      s = gain * (2.5 if l == len(self.dims) - 2 else 1.0) / np.sqrt(k)                 # the last layer's gain: some actions saturate the env's clip, some do not
      self.layers.append(((rng.standard_normal((n, k)) * s).astype(np.float32), (rng.standard_normal(n) * 0.3).astype(np.float32)))
    flat = np.concatenate([a.reshape(-1) for wb in self.layers for a in wb])
    self.params = torch.tensor(flat, device=device)
    d = self.dims + [0] * (4 - len(self.dims))
    self.struct = _abi.MlpPolicy(n_layers=len(self.layers), dims=(C.c_int32 * 4)(*d), hidden_act=_abi.ACTIVATIONS[hidden_act],
                                 out_act=_abi.ACTIVATIONS[out_act], precision=0, params=self.params.data_ptr())


def policy_rollout(h, pol, E, T, reset_first, null=()):
  """earl_tabletop_policy_rollout through the harness `h` (either library) -> dict of numpy arrays; outputs named in `null` are passed as NULL"""
  lead = (E, T, h.n) if reset_first else (T, h.n)
  arrs, out = h._outs(lead)
  names = ('obs', 'reward', 'done', 'success')
  for k in null:
    if k in names:
      setattr(out, k, None)
  act = torch.full(lead + (3,), float('nan'), dtype=torch.float32, device=h.dev)
  st = h._state()
  rc = h.lib.earl_tabletop_policy_rollout(C.byref(h.cfg), C.byref(st), C.byref(pol.struct), E, T, int(reset_first), C.byref(out),
                                          None if 'act' in null else act.data_ptr(), h.stream)
  h._ok(rc, 'policy_rollout')
  h.cfg.counter += E * (T + 1) if reset_first else T
  res = {k: a.cpu().numpy() for k, a in zip(names, arrs)}
  res['act'] = act.cpu().numpy()
  return res


def snapshot(h):
  return {k: getattr(h, k).clone() for k in h.STATE}, int(h.cfg.counter)


def restore(h, snap):
  for k, v in snap[0].items():
    getattr(h, k).copy_(v)
  h.cfg.counter = snap[1]


def final_state(h):
  return {k: h.host(k).copy() for k in h.STATE}, int(h.cfg.counter)


def open_loop(h, act, reset_first):
  """the existing open-loop entry point fed with recorded actions"""
  names = ('obs', 'reward', 'done', 'success')
  if reset_first:
    return dict(zip(names, (a.cpu().numpy() for a in h.eval_episodes(np.ascontiguousarray(act)))))
  return dict(zip(names, h.rollout(np.ascontiguousarray(act))))


def assert_same_bits(got, want, keys=('obs', 'reward', 'done', 'success')):
  for k in keys:
    a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
    assert a.shape == b.shape and a.dtype == b.dtype, k
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=k)


def assert_same_state(a, b):
  for k in a[0]:
    np.testing.assert_array_equal(a[0][k].view(np.uint8), b[0][k].view(np.uint8), err_msg=k)
  assert a[1] == b[1]


def closed_equals_open(dev, pol, n, E, T, reset_first, **kw):
  h = hx.HipTabletop(n, device=dev, seed=5, env_offset=2, **kw)
  h.reset()
  if not reset_first:                         # a continuing rollout starts somewhere: a few scripted steps first
    rng = np.random.default_rng(1)
    h.rollout(rng.uniform(-1, 1, size=(9, n, 3)).astype(np.float32))
  snap = snapshot(h)
  got = policy_rollout(h, pol, E, T, reset_first)
  end = final_state(h)
  assert not np.isnan(got['act']).any()
  restore(h, snap)
  want = open_loop(h, got['act'], reset_first)
  assert_same_bits(got, want)
  assert_same_state(end, final_state(h))
  return got, snap


CPU = 'cpu'


# ---------------------------------------------------------------------------------------------------------------- 1. closed = open
@pytest.mark.parametrize('T', [200, 37])
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
@pytest.mark.parametrize('wide', [False, True])
def test_closed_equals_open_evaluation_form(T, rt, wide):
  pol = Policy((64,), seed=T)
  closed_equals_open(CPU, pol, 70, 3, T, True, reward_type=rt, wide_init=wide, horizon=T)


@pytest.mark.parametrize('kw', [dict(goal_change_frequency=50, horizon=10**6), dict(auto_reset=True, horizon=13), dict(goal_change_frequency=50, auto_reset=True, horizon=31, wide_init=True)],
                         ids=['lifelong', 'auto_reset', 'both'])
def test_closed_equals_open_continuing_form(kw):
  pol = Policy((48, 32), hidden_act='tanh', seed=3)
  got, _ = closed_equals_open(CPU, pol, 70, 1, 200, False, reward_type='dense', **kw)
  if kw.get('auto_reset'):
    assert got['done'].any()


# ---------------------------------------------------------------------------------------------------------------- 2. pinned to the reference
@pytest.mark.parametrize('wide', [False, True])
def test_oracle_stepped_with_the_recorded_actions_reproduces_the_closed_loop(wide):
  n, E, T = 50, 3, 40
  kw = dict(reward_type='sparse', wide_init=wide, horizon=T, seed=9, env_offset=1)
  pol = Policy((32,), seed=11)
  h, o = hx.HipTabletop(n, device=CPU, **kw), orc.OracleTabletop(n, **kw)
  got = policy_rollout(h, pol, E, T, True)
  for e in range(E):
    o.reset()
    obs, rew, done, succ = o.rollout(np.ascontiguousarray(got['act'][e]))
    np.testing.assert_array_equal(got['obs'][e].view(np.uint32), obs.view(np.uint32))
    np.testing.assert_array_equal(got['reward'][e], rew)
    np.testing.assert_array_equal(got['done'][e], done)
    np.testing.assert_array_equal(got['success'][e], succ)
  np.testing.assert_array_equal(h.host('qpos'), o.qpos)
  assert h.cfg.counter == o.cfg.counter


# ---------------------------------------------------------------------------------------------------------------- 3. the actions are the policy's
def consumed_observations(h_kw, n, E, T, got):
  """the float32 observation each step consumed: the reset's observation for t = 0 (from the oracle, which test 2 pins), row t - 1 otherwise"""
  o = orc.OracleTabletop(n, **h_kw)
  x = np.empty((E, T, n, 12), np.float32)
  for e in range(E):
    x[e, 0] = o.reset()
    o.rollout(np.ascontiguousarray(got['act'][e]))
    x[e, 1:] = got['obs'][e, :-1]
  return x


def f64_policy_with_bound(pol, x):
  """float64 evaluation of the float32 weights and the a-priori bound on what a float32 k-ascending fmaf chain can differ from it, layer by layer:
  e_out,j = gamma_K (|b_j| + sum_k |W_jk| |x_k|) + sum_k |W_jk| e_in,k, gamma_K = K u / (1 - K u), u = 2^-24; e = 0 at the input; ReLU and tanh are
  1-Lipschitz; where tanh_f32 is applied its own asserted bound (TANH_ULP_BOUND ulp of a value of magnitude <= |tanh| + e) is added"""
  v = x.astype(np.float64)
  e = np.zeros_like(v)
  for l, (w, b) in enumerate(pol.layers):
    w64, b64, K = w.astype(np.float64), b.astype(np.float64), w.shape[1]
    gam = K * U / (1 - K * U)
    e = gam * (np.abs(b64) + np.abs(v) @ np.abs(w64).T) + e @ np.abs(w64).T
    v = v @ w64.T + b64
    kind = pol.hidden_act if l + 1 < len(pol.layers) else pol.out_act
    if kind == 'relu':
      v = np.maximum(v, 0)
    elif kind == 'tanh':
      v = np.tanh(v)
      e = e + TANH_ULP_BOUND * 2.0 ** -23 * (np.abs(v) + e) + 2.0 ** -149
  return v, e


@pytest.mark.parametrize('hidden,hact,oact', [((64,), 'relu', 'tanh'), ((48, 32), 'tanh', 'none'), ((256, 256), 'relu', 'tanh')])
def test_actions_are_the_policy_within_the_a_priori_bound(hidden, hact, oact):
  n, E, T = 40, 2, 25
  kw = dict(reward_type='sparse', horizon=T, seed=4)
  pol = Policy(hidden, hact, oact, seed=2)
  h = hx.HipTabletop(n, device=CPU, **kw)
  got = policy_rollout(h, pol, E, T, True)
  x = consumed_observations(kw, n, E, T, got)
  want, bound = f64_policy_with_bound(pol, x)
  err = np.abs(got['act'].astype(np.float64) - want)
  print(f'{hidden} {hact}/{oact}: max |error| {err.max():.3e}, max error / bound {np.max(err / bound):.3f}, bound <= {bound.max():.3e}')
  assert (err <= bound).all()                      # every row
  assert bound.max() < 1e-2                        # ... and the bound says something (actions are O(1); worst-case growth through two 256-wide layers is 6e-3)


def round_f32(fr):
  """a Fraction rounded ONCE to the nearest float32 (ties to even), as a Fraction"""
  if fr == 0:
    return Fraction(0)
  a, e = abs(fr), 0
  while a >= 2:
    a /= 2; e += 1
  while a < 1:
    a *= 2; e -= 1
  e = max(e, -126)
  q = Fraction(2) ** (e - 23)
  return (1 if fr > 0 else -1) * round(abs(fr) / q) * q


def test_small_case_exactly_against_the_fmaf_chain_in_fractions():
  n, T = 4, 2
  kw = dict(reward_type='sparse', horizon=T, seed=1, wide_init=True)
  pol = Policy((16,), 'relu', 'none', seed=8)
  h = hx.HipTabletop(n, device=CPU, **kw)
  got = policy_rollout(h, pol, 1, T, True)
  x = consumed_observations(kw, n, 1, T, got)
  for t in range(T):
    for i in range(n):
      v = [Fraction(float(a)) for a in x[0, t, i]]
      for l, (w, b) in enumerate(pol.layers):
        nxt = []
        for j in range(w.shape[0]):
          acc = Fraction(float(b[j]))
          for k in range(w.shape[1]):
            acc = round_f32(v[k] * Fraction(float(w[j, k])) + acc)          # fmaf: one rounding
          nxt.append(max(acc, Fraction(0)) if l == 0 else acc)
        v = nxt
      want = np.array([float(a) for a in v], np.float32)
      np.testing.assert_array_equal(got['act'][0, t, i].view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 4. tanh_f32
SWEEP = r'''
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "tabletop_policy.h"
using earl::tanh_f32;
static float f(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }
static uint32_t u(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
static double ulp_err(float x) {                      // |tanh_f32(x) - tanh(x)| in units of the float32 spacing at tanh(x)
  const double ref = std::tanh((double)x);
  int e; std::frexp(ref, &e);                         // |ref| in [2^(e-1), 2^e)
  if (e - 1 < -126) e = -125;
  return std::fabs((double)tanh_f32(x) - ref) / std::ldexp(1.0, e - 1 - 23);
}
int main() {
  const uint32_t lo = u(0x1p-12f), hi = u(16.0f);
  double worst = 0; uint32_t worst_at = 0; long long not_odd = 0, not_monotone = 0, above_one = 0;
#pragma omp parallel
  {
    double w = 0; uint32_t at = 0; long long a = 0, b = 0, c = 0;
#pragma omp for schedule(static, 1 << 16) nowait
    for (long long k = lo; k <= (long long)hi; ++k) {
      const float x = f((uint32_t)k), y = tanh_f32(x);
      if (u(tanh_f32(-x)) != (u(y) ^ 0x80000000u)) ++a;
      if (k > lo && tanh_f32(f((uint32_t)k - 1)) > y) ++b;             // (negative arguments: oddness carries it over)
      if (!(std::fabs(y) <= 1.0f)) ++c;
      const double er = ulp_err(x);
      if (er > w) { w = er; at = (uint32_t)k; }
    }
#pragma omp critical
    { not_odd += a; not_monotone += b; above_one += c; if (w > worst) { worst = w; worst_at = at; } }
  }
  // log-spaced sample outside the swept range: the smallest subnormal .. 2^-12 and 16 .. FLT_MAX (bit patterns are log-spaced), both ends included
  double worst_out = 0; long long bad_out = 0;
  for (int part = 0; part < 2; ++part) {
    const uint32_t a = part ? hi : 1u, b = part ? 0x7f7fffffu : lo;
    for (int k = 0; k < 500000; ++k) {
      const uint32_t bits = a + (uint32_t)(((unsigned long long)(b - a) * (unsigned long long)k) / 499999ull);
      const float x = f(bits), y = tanh_f32(x);
      if (u(tanh_f32(-x)) != (u(y) ^ 0x80000000u) || !(std::fabs(y) <= 1.0f)) ++bad_out;
      const double er = ulp_err(x);
      if (er > worst_out) worst_out = er;
    }
  }
  printf("sweep %u %u\n", lo, hi);
  printf("worst_ulp %.9f at %a\n", worst, (double)f(worst_at));
  printf("not_odd %lld not_monotone %lld above_one %lld\n", not_odd, not_monotone, above_one);
  printf("outside worst_ulp %.9f bad %lld\n", worst_out, bad_out);
  printf("zeros %08x %08x\n", u(tanh_f32(0.0f)), u(tanh_f32(-0.0f)));
  printf("inf %08x %08x\n", u(tanh_f32(INFINITY)), u(tanh_f32(-INFINITY)));
  printf("nan %d %d\n", (int)std::isnan(tanh_f32(NAN)), (int)std::isnan(tanh_f32(-NAN)));
  printf("max %08x subnormal %08x\n", u(tanh_f32(FLT_MAX)), u(tanh_f32(f(1u))));
  return 0;
}
'''


def test_tanh_f32_over_every_float32_of_the_swept_range(tmp_path):
  src = tmp_path / 'tanh_sweep.cpp'
  src.write_text(SWEEP)
  exe = tmp_path / 'tanh_sweep'
  subprocess.run(['g++', '-O2', '-std=c++17', '-mavx2', '-mfma', '-ffp-contract=off', '-fno-fast-math', '-fopenmp', '-DEARL_HOST_BUILD', '-I', CSRC,
                  '-o', str(exe), str(src)], check=True)
  out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=900).stdout
  print(out)
  ln = dict(line.split(' ', 1) for line in out.strip().splitlines())
  lo, hi = (int(t) for t in ln['sweep'].split())
  assert lo == 0x39800000 and hi == 0x41800000 and hi - lo + 1 > 1.3e8                  # every float32 in [2^-12, 16], and (oddness) its negative
  assert ln['not_odd'] == '0 not_monotone 0 above_one 0'
  worst = float(ln['worst_ulp'].split()[0])
  assert worst <= TANH_ULP_BOUND                                                          # measured 0.49999999 (double tanh is itself within 1e-9 float32 ulp of tanh)
  t = ln['outside'].split()
  assert float(t[1]) <= TANH_ULP_BOUND and t[3] == '0'
  assert ln['zeros'] == '00000000 80000000'
  assert ln['inf'] == '3f800000 bf800000'
  assert ln['nan'] == '1 1'
  assert ln['max'] == '3f800000 subnormal 00000001'


# ---------------------------------------------------------------------------------------------------------------- 5. ABI edges
def _edge_calls(lib, host):
  h = hx.HipTabletop(8, device=CPU)
  st = h._state()
  arrs, out = h._outs((1, 4, 8))
  pol = Policy((16,))

  def call(cfg=h.cfg, state=st, p=pol.struct, E=1, T=4, rf=1, o=out):
    args = [C.byref(cfg) if cfg is not None else None, C.byref(state) if state is not None else None, C.byref(p) if p is not None else None, E, T, rf,
            C.byref(o) if o is not None else None, None]
    return lib.earl_tabletop_policy_rollout_cpu(*args) if host else lib.earl_tabletop_policy_rollout(*args, None)

  def variant(**kw):
    d = dict(n_layers=pol.struct.n_layers, dims=tuple(pol.struct.dims), hidden_act=pol.struct.hidden_act, out_act=pol.struct.out_act, precision=0,
             params=pol.struct.params)
    d.update(kw)
    d['dims'] = (C.c_int32 * 4)(*d['dims'])
    return _abi.MlpPolicy(**d)

  bad = [dict(cfg=None), dict(state=None), dict(p=None), dict(o=None), dict(p=variant(params=None)), dict(p=variant(precision=1)),
         dict(p=variant(n_layers=1)), dict(p=variant(n_layers=4)), dict(p=variant(dims=(13, 16, 3, 0))), dict(p=variant(dims=(12, 16, 4, 0))),
         dict(p=variant(dims=(12, 24, 3, 0))), dict(p=variant(dims=(12, 272, 3, 0))), dict(p=variant(dims=(12, 0, 3, 0))),
         dict(p=variant(n_layers=3, dims=(12, 16, 8, 3))), dict(p=variant(hidden_act=0)), dict(p=variant(hidden_act=3)), dict(p=variant(out_act=1)),
         dict(T=0), dict(T=-1), dict(E=0), dict(E=2, rf=0), dict(rf=2)]
  for kw in bad:
    assert call(**kw) == -1, kw
    assert (lib.earl_host_last_error if host else lib.earl_last_error)(), kw
  call.keep = (h, arrs, pol)                                # the buffers the structs point into
  return call


def test_argument_errors_from_the_host_library():
  lib = _abi.load_host()
  call = _edge_calls(lib._cdll, True)
  assert call() == 0                                       # the good call runs (host pointers)


def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  _edge_calls(lib, False)
  assert lib.earl_tabletop_policy_rollout(None, None, None, 1, 1, 1, None, None, None) == -1
  assert b'NULL' in lib.earl_last_error()


def test_mlp_policy_rejects_what_the_kernel_cannot_take():
  from earl_benchmark_amd.policy import MLPPolicy

  def net(*dims):
    return [(np.zeros((n, k), np.float32), np.zeros(n, np.float32)) for k, n in zip(dims[:-1], dims[1:])]

  MLPPolicy(net(12, 16, 3))
  MLPPolicy(net(12, 256, 256, 3))
  for dims, what in (((12, 24, 3), 'width 24'), ((12, 272, 3), 'width 272'), ((12, 16, 16, 16, 3), '3 hidden layers'), ((13, 16, 3), 'width 13'), ((12, 16, 4), 'width 4')):
    with pytest.raises(ValueError, match=what):
      MLPPolicy(net(*dims))
  with pytest.raises(ValueError):
    MLPPolicy(net(12, 16, 3), hidden_act='gelu')
  seq = torch.nn.Sequential(torch.nn.Linear(12, 32), torch.nn.Tanh(), torch.nn.Linear(32, 3), torch.nn.Tanh())
  pi = MLPPolicy(seq)
  assert pi.dims == [12, 32, 3] and pi.hidden_act == 'tanh' and pi.out_act == 'tanh' and pi.params.numel() == 12 * 32 + 32 + 32 * 3 + 3
  x = torch.randn(5, 12)
  torch.testing.assert_close(pi(x), seq(x))


def test_rollout_policy_on_the_host_through_the_loader_and_the_wrappers():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import MLPPolicy
  pol = Policy((64,), seed=6)
  pi = MLPPolicy(pol.layers, 'relu', 'tanh', device='cpu')
  np.testing.assert_array_equal(pi.params.numpy(), pol.params.numpy())
  train_env, eval_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=33, device='cpu', seed=3).get_envs()
  T = 20
  sd = eval_env.unwrapped.state_dict()
  obs, rew, done, succ, act = eval_env.rollout_policy(pi, T, episodes=2)
  assert tuple(obs.shape) == (2, T, 33, 12) and tuple(act.shape) == (2, T, 33, 3) and eval_env.total_steps == 2 * T
  assert int(eval_env.num_interventions.sum()) == 2 * 33
  end = eval_env.unwrapped.state_dict()
  eval_env.unwrapped.load_state_dict(sd)
  o2, r2, d2, s2 = eval_env.rollout_episodes(act)
  assert torch.equal(obs.view(torch.int32), o2.view(torch.int32)) and torch.equal(rew, r2) and torch.equal(done, d2) and torch.equal(succ, s2)
  assert eval_env.unwrapped.state_dict()['rng_counter'] == end['rng_counter']
  # the train env: lifelong wrapper, continuing form
  train_env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', setup_as_lifelong_learning=True, num_envs=33, device='cpu', seed=3).get_envs()
  train_env.unwrapped._cfg.goal_change_frequency = 7        # (the loader's 400 would not switch within T)
  train_env.reset()
  sd = train_env.unwrapped.state_dict()
  obs, rew, done, succ, act = train_env.rollout_policy(pi, T, reset_first=False)
  assert tuple(obs.shape) == (T, 33, 12)
  lret = train_env.lifelong_return.clone()
  train_env.unwrapped.load_state_dict(sd)
  o2, r2, d2, s2 = train_env.rollout(act)
  assert torch.equal(obs.view(torch.int32), o2.view(torch.int32)) and torch.equal(rew, r2)
  assert torch.equal(lret, train_env.lifelong_return)
  with pytest.raises(ValueError):
    train_env.rollout_policy(pi, T, episodes=2, reset_first=False)


# ---------------------------------------------------------------------------------------------------------------- 6. no scratch
def test_no_instantiation_of_the_policy_kernel_uses_scratch():
  figures = {k: fig for k, fig in kernel_build.unit('tabletop_policy.hip').figures.items() if 'policy_rollout_kernel' in k}
  assert len(figures) == 10, figures                                    # NT2 = 0..4 x GENERAL
  for name, fig in figures.items():
    assert fig[3] == 0, (name, fig[3])

"""earl_sawyer_policy_rollout (include/earl_physics.h): the Sawyer door / peg rollout with a float32 MLP policy 14 -> hidden (-> hidden) -> 4 evaluated inside
the rollout kernel.  What can be held without a GPU:
  1. earl_mlp_policy_forward_cpu (libearl_host.so), the host statement of the policy contract and the oracle of the device's actions, exactly against the
     k-ascending fmaf chain evaluated in fractions.Fraction with one float32 rounding per step;
  2. the entry points are declared, bound and exported where they belong;
  3. every argument error of the device entry point comes back before any HIP call;
  4. MLPPolicy / GaussianMLPPolicy with obs_dim=14, act_dim=4, and the tabletop paths refusing such a policy;
  5. compile time: no scratch inside the timestep loop of any new instantiation, and the occupancy of the plain instantiation it derives from.
tests/test_sawyer_policy_rollout_gpu.py holds the launch itself."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import kernel_build
from conftest import REPO
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, head, variant as variant_of

CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')


# ---------------------------------------------------------------------------------------------------------------- helpers (shared with the GPU tests)
def random_layers(dims, seed, gain=1.0, last_gain=1.0):
  """random ASYMMETRIC weights (no symmetry hides a transposed lane map)"""
  rng = np.random.default_rng(seed)
  layers = []
  for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
    s = gain * (last_gain if l == len(dims) - 2 else 1.0) / np.sqrt(k)
    layers.append(((rng.standard_normal((n, k)) * s).astype(np.float32), (rng.standard_normal(n) * 0.3 * gain).astype(np.float32)))
  return layers


def pack(layers, hidden_act, out_act):
  """struct earl_mlp_policy over host memory; returns (struct, the array it points into)"""
  dims = [layers[0][0].shape[1]] + [w.shape[0] for w, _ in layers]
  flat = np.ascontiguousarray(np.concatenate([a.reshape(-1) for wb in layers for a in wb]), np.float32)
  d = dims + [0] * (4 - len(dims))
  return _abi.MlpPolicy(n_layers=len(layers), dims=(C.c_int32 * 4)(*d), hidden_act=_abi.ACTIVATIONS[hidden_act], out_act=_abi.ACTIVATIONS[out_act], precision=0,
                        params=flat.ctypes.data), flat


def forward_cpu(layers, hidden_act, out_act, obs, head=None, eps=None):
  """earl_mlp_policy_forward_cpu on float32 rows obs [n, K] -> actions [n, A]; head: None or (mode, log_std_map, lo, hi)"""
  host = _abi.load_host()
  st, keep = pack(layers, hidden_act, out_act)
  obs = np.ascontiguousarray(obs, np.float32)
  n = obs.shape[0]
  A = layers[-1][0].shape[0] // (2 if head else 1)
  act = np.full((n, A), np.nan, np.float32)
  hs = None if head is None else _abi.GaussianHead(mode=head[0], log_std_map=head[1], log_std_min=head[2], log_std_max=head[3], eps_out=None)
  if eps is not None:
    eps = np.ascontiguousarray(eps, np.float32)
  rc = host.earl_mlp_policy_forward_cpu(C.byref(st), None if hs is None else C.byref(hs), n, obs.ctypes.data, None if eps is None else eps.ctypes.data,
                                        act.ctypes.data)
  assert rc == 0, host.earl_last_error()
  del keep
  return act


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


def chain_in_fractions(layers, hidden_act, x):
  """the pre-activations of the last layer for ONE float32 input row: acc = b_j; k ascending: acc = fmaf(x_k, W_jk, acc), one float32 rounding per step; ReLU is
  max(acc, 0); tanh is the library's tanh_f32 of the (exact) float32 pre-activation"""
  host = _abi.load_host()
  v = [Fraction(float(a)) for a in x]
  for l, (w, b) in enumerate(layers):
    nxt = []
    for j in range(w.shape[0]):
      acc = Fraction(float(b[j]))
      for k in range(w.shape[1]):
        acc = round_f32(v[k] * Fraction(float(w[j, k])) + acc)
      if l + 1 < len(layers):
        acc = max(acc, Fraction(0)) if hidden_act == 'relu' else Fraction(float(host.earl_tanh_f32(float(acc))))
      nxt.append(acc)
    v = nxt
  return v


def as_f32_bits(values):
  return np.array([float(a) for a in values], np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. the host statement of the contract
@pytest.mark.parametrize('hidden_act,out_act', [('relu', 'none'), ('tanh', 'tanh'), ('relu', 'tanh')])
def test_forward_cpu_exactly_against_the_fmaf_chain_in_fractions(hidden_act, out_act):
  host = _abi.load_host()
  layers = random_layers([14, 16, 4], seed=8, last_gain=2.5)
  x = np.random.default_rng(2).uniform(-1, 1, size=(5, 14)).astype(np.float32)
  got = forward_cpu(layers, hidden_act, out_act, x)
  for i in range(x.shape[0]):
    v = chain_in_fractions(layers, hidden_act, x[i])
    want = [Fraction(float(host.earl_tanh_f32(float(a)))) if out_act == 'tanh' else a for a in v]
    np.testing.assert_array_equal(got[i].view(np.uint32), as_f32_bits(want))


def test_forward_cpu_with_the_head_at_its_mean_and_sampled():
  host = _abi.load_host()
  layers = random_layers([14, 16, 16, 8], seed=5, last_gain=2.5)
  rng = np.random.default_rng(3)
  x = rng.uniform(-1, 1, size=(4, 14)).astype(np.float32)
  lo, hi = np.float32(-5.0), np.float32(2.0)
  # at the mean (mode MEAN, and mode SAMPLE without eps): rows 0..3 of the last layer, no activation (out_act none)
  for head, eps in (((_abi.HEAD_MEAN, _abi.LOGSTD_CLAMP, lo, hi), None), ((_abi.HEAD_SAMPLE, _abi.LOGSTD_CLAMP, lo, hi), None)):
    got = forward_cpu(layers, 'relu', 'none', x, head=head, eps=eps)
    assert got.shape == (4, 4)
    for i in range(4):
      np.testing.assert_array_equal(got[i].view(np.uint32), as_f32_bits(chain_in_fractions(layers, 'relu', x[i])[:4]))
  # sampled, clamp map: ls = min(max(raw, lo), hi) (exact), sigma = exp_f32(ls) through the library, u = fmaf(sigma, eps, mean) with one rounding; the draws
  # are normal_quantile_f32 of 24-bit words through the library
  k24 = rng.integers(0, 2 ** 24, size=(4, 4), dtype=np.uint32)
  eps = np.array([[host.earl_normal_quantile_f32(int(k)) for k in row] for row in k24], np.float32)
  got = forward_cpu(layers, 'relu', 'none', x, head=(_abi.HEAD_SAMPLE, _abi.LOGSTD_CLAMP, lo, hi), eps=eps)
  for i in range(4):
    v = chain_in_fractions(layers, 'relu', x[i])
    want = []
    for d in range(4):
      ls = min(max(np.float32(float(v[4 + d])), lo), hi)
      sigma = Fraction(float(host.earl_exp_f32(float(ls))))
      want.append(round_f32(sigma * Fraction(float(eps[i, d])) + v[d]))
    np.testing.assert_array_equal(got[i].view(np.uint32), as_f32_bits(want))
  # the quantile is odd in k <-> 2^24 - 1 - k, and exp_f32(0) is 1: the library functions are the contract's
  assert host.earl_normal_quantile_f32(5) == -host.earl_normal_quantile_f32(2 ** 24 - 1 - 5) and host.earl_exp_f32(0.0) == 1.0


def test_forward_cpu_takes_other_widths_and_refuses_bad_arguments():
  host = _abi.load_host()
  layers = random_layers([3, 5, 2], seed=1)                             # any input width 1..256, any action width
  x = np.random.default_rng(0).uniform(-1, 1, size=(2, 3)).astype(np.float32)
  got = forward_cpu(layers, 'relu', 'none', x)
  for i in range(2):
    np.testing.assert_array_equal(got[i].view(np.uint32), as_f32_bits(chain_in_fractions(layers, 'relu', x[i])))
  st, keep = pack(layers, 'relu', 'none')
  act = np.zeros((2, 2), np.float32)
  assert host.earl_mlp_policy_forward_cpu(None, None, 2, x.ctypes.data, None, act.ctypes.data) == -1
  assert host.earl_mlp_policy_forward_cpu(C.byref(st), None, 2, None, None, act.ctypes.data) == -1
  st.precision = 1
  assert host.earl_mlp_policy_forward_cpu(C.byref(st), None, 2, x.ctypes.data, None, act.ctypes.data) == -1
  assert host.earl_last_error()


# ---------------------------------------------------------------------------------------------------------------- 2. declared, bound, exported
def test_entry_points_are_declared_bound_and_exported():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'int\s+earl_sawyer_policy_rollout\s*\((.*?)\)\s*;', src, flags=re.S)
  assert m, 'earl_sawyer_policy_rollout is not declared'
  assert len(m.group(1).split(',')) == len(_abi.SIGNATURES['earl_sawyer_policy_rollout']) == 13
  m = re.search(r'int32_t\s+earl_mlp_policy_forward_cpu\s*\((.*?)\)\s*;', src, flags=re.S)
  assert m and len(m.group(1).split(',')) == len(_abi.HOST_EXTRA_SIGNATURES['earl_mlp_policy_forward_cpu'][0]) == 6
  lib, host = _abi.load(), C.CDLL(_abi.HOST_LIB_PATH)
  assert hasattr(lib, 'earl_sawyer_policy_rollout') and not hasattr(host, 'earl_sawyer_policy_rollout')
  assert hasattr(host, 'earl_mlp_policy_forward_cpu') and not hasattr(lib, 'earl_mlp_policy_forward_cpu')
  for name in ('earl_tanh_f32', 'earl_exp_f32', 'earl_normal_quantile_f32'):
    assert hasattr(host, name), name


# ---------------------------------------------------------------------------------------------------------------- 3. argument errors, no GPU
def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  layers = random_layers([14, 16, 4], seed=0)
  pol, keep = pack(layers, 'relu', 'tanh')
  aligned = aligned_params(pol, keep)
  cfg = _abi.SawyerCfg(n=8, frame_skip=5)
  buf = np.zeros(4096, np.float64)                                       # never read: every call below returns before any HIP call
  p = buf.ctypes.data
  st = _abi.SawyerState(qpos=p, qvel=p, mocap_pos=p, goal=p)
  out = _abi.SawyerOut(obs=p)

  def variant(base=pol, **kw):
    return variant_of(base, **kw)

  def call(model=p, nv=10, cfg=cfg, st=st, pol=pol, head=None, obs0=p, T=4, actions=p, out=out):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_sawyer_policy_rollout(model, None, nv, ref(cfg), ref(st), ref(pol), ref(head), obs0, T, None, actions, ref(out), None)

  pol8 = variant(dims=(14, 16, 8, 0))
  bad = [dict(pol=None), dict(obs0=None), dict(actions=None), dict(out=_abi.SawyerOut(obs=None)), dict(out=None), dict(model=None), dict(cfg=None), dict(st=None),
         dict(pol=variant(dims=(12, 16, 4, 0))), dict(pol=variant(dims=(15, 16, 4, 0))),                                  # dims[0] != 14
         dict(pol=variant(dims=(14, 16, 3, 0))), dict(pol=pol8), dict(pol=pol, head=head()), dict(pol=variant(dims=(14, 16, 6, 0)), head=head()),   # the last layer
         dict(pol=variant(dims=(14, 24, 4, 0))), dict(pol=variant(dims=(14, 272, 4, 0))), dict(pol=variant(dims=(14, 0, 4, 0))), dict(pol=variant(dims=(14, 8, 4, 0))),
         dict(pol=variant(n_layers=3, dims=(14, 16, 24, 4))),                                                            # hidden widths
         dict(pol=variant(n_layers=1)), dict(pol=variant(n_layers=4)), dict(pol=variant(dims=(14, 16, 4, 1))),
         dict(pol=variant(precision=1)), dict(pol=variant(params=None)), dict(pol=variant(params=pol.params + 4)),
         dict(pol=variant(hidden_act=0)), dict(pol=variant(hidden_act=3)), dict(pol=variant(out_act=1)),
         dict(T=0), dict(T=-1), dict(nv=23), dict(nv=12),
         dict(pol=pol8, head=head(mode=2)), dict(pol=pol8, head=head(m=2)), dict(pol=pol8, head=head(lo=-21.0)), dict(pol=pol8, head=head(hi=4.5)),
         dict(pol=pol8, head=head(lo=1.0, hi=0.0)), dict(pol=pol8, head=head(lo=float('nan')))]                          # the head errors of the tabletop entry point
  for kw in bad:
    assert call(**kw) == -1, kw
  cfg0 = _abi.SawyerCfg(n=0, frame_skip=5)
  assert call(cfg=cfg0) == 0 and call(cfg=cfg0, pol=pol8, head=head()) == 0     # n = 0: every check passed and nothing was launched (the arguments above are otherwise good)
  del aligned, buf


# ---------------------------------------------------------------------------------------------------------------- 4. the Python policy classes
def test_policy_classes_take_the_sawyer_widths_and_the_tabletop_refuses_them():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import AgentPair, GaussianMLPPolicy, MLPPolicy, PolicyPopulation
  layers = random_layers([14, 32, 4], seed=4)
  pi = MLPPolicy(layers, 'relu', 'tanh', obs_dim=14, act_dim=4)
  assert pi.dims == [14, 32, 4] and (pi.obs_dim, pi.act_dim) == (14, 4) and pi.params.numel() == 14 * 32 + 32 + 32 * 4 + 4
  assert list(pi.struct.dims) == [14, 32, 4, 0] and pi.macs == 14 * 32 + 32 * 4
  x = torch.as_tensor(np.random.default_rng(0).uniform(-1, 1, size=(6, 14)).astype(np.float32))
  np.testing.assert_allclose(pi(x).numpy(), forward_cpu(layers, 'relu', 'tanh', x.numpy()), rtol=0, atol=1e-5)      # (torch's summation order: close, not bit-identical)
  glayers = random_layers([14, 16, 16, 8], seed=6)
  g = GaussianMLPPolicy(glayers, 'tanh', squash=True, log_std_map='clamp', obs_dim=14, act_dim=4)
  assert g.dims == [14, 16, 16, 8] and tuple(g(x).shape) == (6, 4) and tuple(g.sample(x, torch.zeros(6, 4)).shape) == (6, 4)
  np.testing.assert_allclose(g(x).numpy(), forward_cpu(glayers, 'tanh', 'tanh', x.numpy(), head=(_abi.HEAD_MEAN, _abi.LOGSTD_CLAMP, -5.0, 2.0)), rtol=0, atol=1e-5)
  # the defaults are the tabletop's and read as they always did
  with pytest.raises(ValueError, match='the input is the 12-wide tabletop observation, got width 14'):
    MLPPolicy(layers, 'relu', 'tanh')
  with pytest.raises(ValueError, match='the output is the 4-wide action, got width 3'):
    MLPPolicy(random_layers([14, 32, 3], seed=4), obs_dim=14, act_dim=4)
  with pytest.raises(ValueError, match='the output is the 8-wide mean and raw log_std of the action, got width 4'):
    GaussianMLPPolicy(layers, obs_dim=14, act_dim=4)
  # the tabletop's paths take 12 / 3 only, and say which widths they were given
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    PolicyPopulation([pi, pi])
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    PolicyPopulation(pi, params=torch.zeros(2, pi.params.numel()))
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    AgentPair(pi, pi)
  _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=4, device='cpu', seed=3).get_envs()
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    env.rollout_policy(pi, 5)
  with pytest.raises(ValueError, match='observation width 14 and action width 4'):
    env.evaluate_policy(pi, 5)


# ---------------------------------------------------------------------------------------------------------------- 5. compile time
def test_new_instantiations_keep_the_timestep_loop_free_of_scratch_and_the_occupancy():
  """every sawyer_policy_rollout_kernel instantiation: zero scratch instructions inside its timestep loop (tools/scratch_in_loops.py's count) and the
  occupancy (and LDS) of the sawyer_rollout_kernel instantiation of the same template arguments in the same unit, from the resource-usage remarks"""
  tool = kernel_build.tool()
  assert 'sawyer_policy_rollout_kernel' in tool.KERNELS
  want = {'physics.hip': {'<10, 16, false>', '<15, 16, false>', '<15, 16, true>'}, 'physics_w8.hip': {'<10, 16, false>'}}
  for unit_name, insts in want.items():
    unit = kernel_build.unit(unit_name)
    lines = [ln for ln in unit.scratch_report() if 'sawyer_policy_rollout_kernel' in ln]
    assert {re.search(r'sawyer_policy_rollout_kernel(<[^>]*>)', ln).group(1) for ln in lines} == insts, lines
    kernel_build.check_scratch_lines(lines, otherwise=('no scratch at all',))
    res = {k: (v['occupancy'], v['lds']) for k, v in unit.resources.items() if 'rollout_kernel<' in k}
    for inst in insts:
      assert res['sawyer_policy_rollout_kernel' + inst] == res['sawyer_rollout_kernel' + inst], (unit_name, inst, res)

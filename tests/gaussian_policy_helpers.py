"""Shared by tests/test_policy_gaussian.py (no GPU) and tests/test_policy_gaussian_gpu.py: a packed Gaussian-head policy with asymmetric random weights, the
call of earl_tabletop_policy_rollout_gaussian through tests/hip_harness.py's HipTabletop (either library), and an independent numpy statement of the draw
layout of csrc/tabletop_policy.h (Philox4x32-10, the 24-bit uniform, the double-precision quantile)."""
import ctypes as C

import numpy as np
import torch

from earl_benchmark_amd import _abi
from test_policy_rollout import final_state, open_loop, restore, snapshot, assert_same_bits, assert_same_state

GAUSS_DRAW = 0x504F4C00
QUANTILE_ULP_BOUND = 5.0      # normal_quantile_f32 against the double-precision quantile, float32 ulp of the result: the next whole ulp above the exhaustive sweep's 4.934 (cap: 8)
EXP_ULP_BOUND = 1.0           # exp_f32 against double exp over every float32 of [-20, 4]: the next whole ulp above the sweep's 0.5000000


class Packed:
  """layers [(W, b), ...] packed as struct earl_mlp_policy wants them"""

  def __init__(self, layers, hidden_act, out_act, device='cpu'):
    self.layers = layers
    self.dims = [layers[0][0].shape[1]] + [w.shape[0] for w, _ in layers]
    self.hidden_act, self.out_act = hidden_act, out_act
    flat = np.concatenate([a.reshape(-1) for wb in layers for a in wb])
    self.params = torch.tensor(flat, device=device)
    d = self.dims + [0] * (4 - len(self.dims))
    self.struct = _abi.MlpPolicy(n_layers=len(layers), dims=(C.c_int32 * 4)(*d), hidden_act=_abi.ACTIVATIONS[hidden_act], out_act=_abi.ACTIVATIONS[out_act],
                                 precision=0, params=self.params.data_ptr())


class GaussPolicy(Packed):
  """random ASYMMETRIC weights, last layer 6 wide: rows 0..2 (mean) with the gain of test_policy_rollout.Policy (some actions saturate the env's clip, some do not),
  rows 3..5 (raw log_std) scaled so that raw spans about +-12: both ends of a clamp to (-5, 2) and its interior occur, and sigma eps moves actions across the clip"""

  def __init__(self, hidden, hidden_act='relu', out_act='tanh', seed=0, device='cpu', log_std_gain=6.0):
    rng = np.random.default_rng(seed)
    dims = [12] + list(hidden) + [6]
    layers = []
    for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
      w = rng.standard_normal((n, k)) / np.sqrt(k)
      b = rng.standard_normal(n) * 0.3
      if l == len(dims) - 2:
        w[:3] *= 2.5
        w[3:] *= log_std_gain
        b[3:] = np.array([-2.0, 0.0, 1.0])
      layers.append((w.astype(np.float32), b.astype(np.float32)))
    super().__init__(layers, hidden_act, out_act, device)

  def mean_twin(self, device='cpu'):
    """the 3-output policy made of rows 0..2 of the last layer"""
    w, b = self.layers[-1]
    return Packed(self.layers[:-1] + [(np.ascontiguousarray(w[:3]), np.ascontiguousarray(b[:3]))], self.hidden_act, self.out_act, device)


def head_struct(mode='sample', log_std_map='tanh', bounds=(-5.0, 2.0), eps_out=None):
  return _abi.GaussianHead(mode={'mean': 0, 'sample': 1}.get(mode, mode), log_std_map={'clamp': 0, 'tanh': 1}.get(log_std_map, log_std_map),
                           log_std_min=bounds[0], log_std_max=bounds[1], eps_out=eps_out)


def gaussian_rollout(h, pol, E, T, reset_first, mode='sample', log_std_map='tanh', bounds=(-5.0, 2.0), null=()):
  """earl_tabletop_policy_rollout_gaussian through the harness `h` (either library) -> dict of numpy arrays; outputs named in `null` are passed as NULL"""
  lead = (E, T, h.n) if reset_first else (T, h.n)
  arrs, out = h._outs(lead)
  names = ('obs', 'reward', 'done', 'success')
  for k in null:
    if k in names:
      setattr(out, k, None)
  act = torch.full(lead + (3,), float('nan'), dtype=torch.float32, device=h.dev)
  eps = torch.full(lead + (3,), float('nan'), dtype=torch.float32, device=h.dev)
  head = head_struct(mode, log_std_map, bounds, None if 'eps' in null else eps.data_ptr())
  st = h._state()
  rc = h.lib.earl_tabletop_policy_rollout_gaussian(C.byref(h.cfg), C.byref(st), C.byref(pol.struct), C.byref(head), E, T, int(reset_first), C.byref(out),
                                                   None if 'act' in null else act.data_ptr(), h.stream)
  h._ok(rc, 'policy_rollout_gaussian')
  h.cfg.counter += E * (T + 1) if reset_first else T
  res = {k: a.cpu().numpy() for k, a in zip(names, arrs)}
  res['act'], res['eps'] = act.cpu().numpy(), eps.cpu().numpy()
  return res


def gaussian_closed_equals_open(h, pol, E, T, reset_first, **head_kw):
  """the launch == the open-loop entry point of the same library fed with act_out: outputs, state left behind, counter"""
  snap = snapshot(h)
  got = gaussian_rollout(h, pol, E, T, reset_first, **head_kw)
  end = final_state(h)
  assert not np.isnan(got['act']).any() and not np.isnan(got['eps']).any()
  restore(h, snap)
  want = open_loop(h, got['act'], reset_first)
  assert_same_bits(got, want)
  assert_same_state(end, final_state(h))
  return got, snap


# ---------------------------------------------------------------------------------------------------------------- the draws, independently
def philox4x32_10(c0, c1, c2, c3, k0, k1):
  """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words"""
  M = np.uint64(0xFFFFFFFF)
  c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in (c0, c1, c2, c3))
  k0, k1 = np.uint64(k0), np.uint64(k1)
  for _ in range(10):
    p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
    k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
  return c0, c1, c2, c3


def ndtri64(u):
  return torch.special.ndtri(torch.as_tensor(u, dtype=torch.float64)).numpy()


def expected_uniform_index(seed, env_ids, counters):
  """k [len(counters), len(env_ids), 3]: the 24-bit uniform index of action dimension d of env `env_id` (global) at the env step with Philox counter `counter`"""
  ctr = np.asarray(counters, np.uint64)[:, None] + np.zeros((1, len(env_ids)), np.uint64)
  env = np.asarray(env_ids, np.uint64)[None, :] + np.zeros_like(ctr)
  x, y, z, _ = philox4x32_10(np.full_like(ctr, GAUSS_DRAW), env, ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
  return np.stack([x, y, z], axis=-1) >> np.uint64(8)


def expected_eps(seed, env_offset, n, E, T, reset_first=True, counter0=0):
  """[E, T, n, 3] float64: Phi^-1((k + 0.5) 2^-24) of the specified draws"""
  counters = np.array([counter0 + e * (T + 1) + int(reset_first) + t for e in range(E) for t in range(T)], np.uint64)
  k = expected_uniform_index(seed, np.arange(n) + env_offset, counters)
  return ndtri64((k.astype(np.float64) + 0.5) * 2.0 ** -24).reshape(E, T, n, 3)


def ulp32(ref):
  """the float32 spacing at |ref| (normal range)"""
  _, e = np.frexp(np.asarray(ref, np.float64))
  return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)

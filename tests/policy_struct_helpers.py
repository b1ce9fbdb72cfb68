"""The ctypes stand-ins that the no-GPU argument-error tests of the stepper envs' closed-loop entry points share (tests/test_sawyer_policy_rollout.py,
test_sawyer_population.py, test_sawyer_pair.py, test_minitaur_policy_rollout.py): a 16-byte aligned home for a policy's parameters, a copy of a policy struct with
some fields changed, and a Gaussian head."""
import ctypes as C

import numpy as np

from earl_benchmark_amd import _abi


def aligned_params(pol, keep, rows=1):
  """point pol.params at a 16-byte aligned copy of `keep` with room for `rows` rows (the stepper units read weight rows in 16-byte pieces) -> the array to keep alive"""
  aligned = np.zeros(rows * (keep.size + 8) + 8, np.float32)
  off = (-aligned.ctypes.data % 16) // 4
  aligned[off:off + keep.size] = keep
  pol.params = aligned.ctypes.data + 4 * off
  return aligned


def variant(base, **kw):
  """struct earl_mlp_policy like `base` with the given fields replaced (dims: a 4-tuple)"""
  d = dict(n_layers=base.n_layers, dims=tuple(base.dims), hidden_act=base.hidden_act, out_act=base.out_act, precision=base.precision, params=base.params)
  d.update(kw)
  d['dims'] = (C.c_int32 * 4)(*d['dims'])
  return _abi.MlpPolicy(**d)


def head(mode=_abi.HEAD_SAMPLE, m=_abi.LOGSTD_TANH, lo=-5.0, hi=2.0):
  return _abi.GaussianHead(mode=mode, log_std_map=m, log_std_min=lo, log_std_max=hi, eps_out=None)

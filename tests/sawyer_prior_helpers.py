"""The oracle of a policy-prior branch's action on the Sawyer door / peg (include/earl_physics.h, "policy-prior branches on the door and the peg") for
tests/test_sawyer_prior.py (no GPU) and tests/test_sawyer_prior_gpu.py; a plain module.

THE ORACLE uses none of the new code: u is earl_mlp_policy_forward_cpu (the policy contract's host statement, older than the feature) on the float32 rounding of the
row, eps comes from tests/tabletop_plan_helpers.py's numpy Philox with the counter words of planner item 2 -- (draw | j, global id, (k << 16) | t, noise_counter), key =
the seed -- and its host-built normal_quantile_f32; a = clip(fmaf(sigma, eps, u)) with that module's exact fmaf and clip."""
import numpy as np

from sawyer_plan_helpers import sigma4
from tabletop_cem_helpers import CEM_DRAW
from tabletop_plan_helpers import PLAN_DRAW, clip, fmaf32, philox4x32_10, quantile
from test_sawyer_policy_rollout import forward_cpu

F32, F64 = np.float32, np.float64


def noise(seed, env_offset, n, k, t, j, nc, cem=False):
  """eps [n, 4] of branch k at step t: the block noise branch k of the planner draws (words x, y, z, w for the four dimensions)"""
  g = ((np.arange(n, dtype=np.int64) + int(env_offset)) & 0xFFFFFFFF).astype(np.uint64)
  ctr = (np.full(n, (CEM_DRAW if cem else PLAN_DRAW) | j, np.uint64), g, np.full(n, (int(k) << 16) | int(t), np.uint64), np.full(n, nc & 0xFFFFFFFF, np.uint64))
  words = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
  return quantile(np.stack([(w >> np.uint64(8)).astype(np.uint32) for w in words], -1))


def step_actions(layers, hidden_act, out_act, obs, seed, env_offset, k, t, j, nc, sigma, cem=False):
  """obs [n, 14] float64, what branch k sees at step t -> its action rows [n, 4] float32"""
  obs = np.ascontiguousarray(obs, F64).reshape(-1, 14)
  n = obs.shape[0]
  u = forward_cpu(layers, hidden_act, out_act, obs.astype(F32))
  eps = noise(seed, env_offset, n, k, t, j, nc, cem)
  return clip(fmaf32(np.broadcast_to(sigma4(sigma)[None], eps.shape), eps, u)).astype(F32)


def rows_actions(layers, hidden_act, out_act, obs, seed, env_offset, k, j, nc, sigma, cem=False):
  """obs [H, n, 14] -> [H, n, 4]: step_actions for t = 0 .. H - 1"""
  return np.stack([step_actions(layers, hidden_act, out_act, obs[t], seed, env_offset, k, t, j, nc, sigma, cem) for t in range(obs.shape[0])])

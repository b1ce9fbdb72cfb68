"""Shared by tests/test_policy_population.py (no GPU) and tests/test_policy_population_gpu.py: a packed population of policies, the call of
earl_tabletop_population_rollout through tests/hip_harness.py's HipTabletop (either library), the per-policy procedure of the contract (cut the shard at the
multiples of G, call the EXISTING single-policy entry point on each piece) and the definitions of the three summary arrays in numpy."""
import ctypes as C

import numpy as np
import torch

import hip_harness as hx
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import GaussPolicy, gaussian_rollout, head_struct
from test_policy_rollout import Policy, policy_rollout

OUT = ('obs', 'reward', 'done', 'success')
SUMMARY = ('ret', 'success_last', 'first_success')
PAD = 5                                                   # floats between the members' rows beyond the parameter count: the stride is not the count


class Population:
  """P members (test_policy_rollout.Policy or gaussian_policy_helpers.GaussPolicy, seeds seed0 ..) stacked as [P, n_params + PAD]; the padding holds NaN, which
  any read past a member's own parameters would carry into the actions"""

  def __init__(self, hidden, P, G, gaussian=False, hidden_act='relu', out_act='tanh', seed0=0, device='cpu'):
    make = GaussPolicy if gaussian else Policy
    self.members = [make(hidden, hidden_act, out_act, seed=seed0 + p, device=device) for p in range(P)]
    self.gaussian, self.G, self.P = gaussian, G, P
    rows = torch.stack([m.params for m in self.members])
    self.n_params = rows.shape[1]
    self.params = torch.full((P, self.n_params + PAD), float('nan'), dtype=torch.float32, device=device)
    self.params[:, :self.n_params] = rows
    m = self.members[0].struct
    self.struct = _abi.MlpPolicy(n_layers=m.n_layers, dims=m.dims, hidden_act=m.hidden_act, out_act=m.out_act, precision=0, params=self.params.data_ptr())
    self.pop = _abi.PolicyPopulation(n_policies=P, envs_per_policy=G, param_stride=self.n_params + PAD)


def members_needed(env_offset, n, G):
  return (env_offset + n - 1) // G + 1


def population_rollout(h, struct, pop, E, T, reset_first, head=None, null=(), summary=True):
  """earl_tabletop_population_rollout through the harness `h` -> dict of numpy arrays.  head: None (deterministic) or the keyword arguments of head_struct;
  names in `null` ('obs', 'reward', 'done', 'success', 'act', 'eps') are passed as NULL; summary=False passes a NULL summary"""
  lead = (E, T, h.n) if reset_first else (T, h.n)
  arrs, out = h._outs(lead)
  for k in null:
    if k in OUT:
      setattr(out, k, None)
  act = torch.full(lead + (3,), float('nan'), dtype=torch.float32, device=h.dev)
  eps = torch.full(lead + (3,), float('nan'), dtype=torch.float32, device=h.dev)
  hd = None if head is None else head_struct(eps_out=None if 'eps' in null else eps.data_ptr(), **head)
  ret = torch.full((E, h.n), float('nan'), dtype=torch.float64, device=h.dev)
  last = torch.full((E, h.n), 7, dtype=torch.uint8, device=h.dev)
  first = torch.full((E, h.n), -7, dtype=torch.int32, device=h.dev)
  sm = _abi.EpisodeSummary(ret=ret.data_ptr(), success_last=last.data_ptr(), first_success=first.data_ptr())
  st = h._state()
  rc = h.lib.earl_tabletop_population_rollout(C.byref(h.cfg), C.byref(st), C.byref(struct), None if pop is None else C.byref(pop), None if hd is None else C.byref(hd),
                                              E, T, int(reset_first), C.byref(out), None if 'act' in null else act.data_ptr(), C.byref(sm) if summary else None, h.stream)
  h._ok(rc, 'population_rollout')
  h.cfg.counter += E * (T + 1) if reset_first else T
  res = {k: a.cpu().numpy() for k, a in zip(OUT, arrs)}
  res.update(act=act.cpu().numpy(), eps=eps.cpu().numpy(), ret=ret.cpu().numpy(), success_last=last.cpu().numpy(), first_success=first.cpu().numpy())
  return res


def pieces(env_offset, n, G):
  """[(first local index, length, member)] of the shard cut at the global ids that are multiples of G"""
  out, i = [], 0
  while i < n:
    g = env_offset + i
    m = min(n - i, (g // G + 1) * G - g)
    out.append((i, m, g // G))
    i += m
  return out


def per_policy_launches(h0, snap, popn, E, T, reset_first, head=None, **kw):
  """the contract's procedure with TODAY's entry points: one harness per piece (env_offset = the piece's first global id, its rows of the state `snap`), the
  member's own packed policy -> (outputs concatenated along the env axis, final state rows concatenated, counter)"""
  outs, states, counter = [], [], None
  for i0, m, member in pieces(h0.cfg.env_offset, h0.n, popn.G):
    h = hx.HipTabletop(m, device=str(h0.dev), env_offset=h0.cfg.env_offset + i0, **kw)
    for k, v in snap[0].items():
      getattr(h, k).copy_(v[i0:i0 + m])
    h.cfg.counter = snap[1]
    pol = popn.members[member]
    outs.append(gaussian_rollout(h, pol, E, T, reset_first, **head) if head is not None else policy_rollout(h, pol, E, T, reset_first))
    states.append({k: h.host(k).copy() for k in h.STATE})
    assert counter in (None, int(h.cfg.counter))
    counter = int(h.cfg.counter)
  axis = 2 if reset_first else 1
  keys = OUT + ('act',) + (('eps',) if head is not None else ())
  return ({k: np.concatenate([o[k] for o in outs], axis=axis) for k in keys}, {k: np.concatenate([s[k] for s in states], axis=0) for k in states[0]}, counter)


def summary_by_definition(reward, success):
  """the three arrays of earl_episode_summary from out->reward / out->success [E, T, n]: the float32 rewards summed in float64 with t ascending (numpy's own
  sum is pairwise: the loop is the definition), success of step T - 1, the smallest t with success or -1"""
  E, T, n = reward.shape
  ret = np.zeros((E, n), np.float64)
  for t in range(T):
    ret = ret + reward[:, t].astype(np.float64)
  s = success.astype(bool)
  first = np.where(s.any(axis=1), s.argmax(axis=1), -1).astype(np.int32)
  return {'ret': ret, 'success_last': success[:, -1].astype(np.uint8), 'first_success': first}


def assert_bits(got, want, keys):
  for k in keys:
    a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
    assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=k)

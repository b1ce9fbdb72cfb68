"""Shared by tests/test_policy_pair.py (no GPU) and tests/test_policy_pair_gpu.py: the two agents of a pair packed as [2, n_params + PAD], the call of
earl_tabletop_pair_rollout through tests/hip_harness.py's HipTabletop (either library), the handover rule of include/earl_tabletop.h restated in numpy, and the
procedures the contract is checked against, built only from entry points that existed before the pair (single-policy launches, step, a reset on scratch state for
the goal draw)."""
import ctypes as C

import numpy as np
import torch

import hip_harness as hx
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import GaussPolicy, Packed, gaussian_rollout, head_struct
from test_policy_rollout import Policy, policy_rollout

OUT = ('obs', 'reward', 'done', 'success')
PAD = 5                                                   # floats between the two rows beyond the parameter count: the stride is not the count
INITIAL = np.array([0.0, 0.0, 2.5, 0.0, -1.0, -1.0])      # the env's initial state as a goal row (backward_goal = 'initial')


class Pair:
  """two members (test_policy_rollout.Policy or gaussian_policy_helpers.GaussPolicy / Packed) stacked as [2, n_params + PAD]; the padding holds NaN, which any read
  past an agent's own parameters would carry into the actions"""

  def __init__(self, hidden=(64,), gaussian=False, hidden_act='relu', out_act='tanh', seed0=0, device='cpu', members=None):
    make = GaussPolicy if gaussian else Policy
    self.members = members or [make(hidden, hidden_act, out_act, seed=seed0 + p, device=device) for p in range(2)]
    self.gaussian = gaussian
    rows = torch.stack([m.params for m in self.members])
    self.n_params = rows.shape[1]
    self.params = torch.full((2, self.n_params + PAD), float('nan'), dtype=torch.float32, device=device)
    self.params[:, :self.n_params] = rows
    m = self.members[0].struct
    self.struct = _abi.MlpPolicy(n_layers=m.n_layers, dims=m.dims, hidden_act=m.hidden_act, out_act=m.out_act, precision=0, params=self.params.data_ptr())
    self.stride = self.n_params + PAD


def still_pair(gaussian=False, device='cpu', bias=0.0):
  """agents whose action is (nearly) zero whatever they see: zero last-layer weights, the bias `bias` on the mean rows -- the arm barely moves, and the handover
  causes are decided by where the env sits (the coverage recipe of the issue)"""
  rng = np.random.default_rng(3)
  nout = 6 if gaussian else 3
  members = []
  for p in range(2):
    w0, b0 = (rng.standard_normal((16, 12)) / 4).astype(np.float32), (rng.standard_normal(16) * 0.3).astype(np.float32)
    wo, bo = np.zeros((nout, 16), np.float32), np.zeros(nout, np.float32)
    bo[:3] = bias * (1 if p == 0 else -1)
    if gaussian:
      bo[3:] = -20.0                                      # raw log_std at the lower bound: sigma = e^-5
    members.append(Packed([(w0, b0), (wo, bo)], 'relu', 'tanh', device))
  return Pair(gaussian=gaussian, device=device, members=members)


class PairState:
  """the caller-owned phase state of n envs (copies of what it is given: the launch writes into it)"""

  def __init__(self, n, device='cpu', phase=None, sip=None):
    self.phase = torch.zeros(n, dtype=torch.int8, device=device) if phase is None else torch.tensor(np.asarray(phase), dtype=torch.int8, device=device)
    self.sip = torch.zeros(n, dtype=torch.int32, device=device) if sip is None else torch.tensor(np.asarray(sip), dtype=torch.int32, device=device)

  def clone(self):
    s = PairState(0)
    s.phase, s.sip = self.phase.clone(), self.sip.clone()
    return s

  def host(self):
    return self.phase.cpu().numpy().copy(), self.sip.cpu().numpy().copy()


def pair_struct(pair, ps, switch_every, switch_on_success, goal=None, agent=None, fs=None, bs=None):
  se = (switch_every, switch_every) if np.ndim(switch_every) == 0 else tuple(switch_every)
  return _abi.AgentPair(switch_every=(C.c_int32 * 2)(*se), switch_on_success=int(switch_on_success), pad_=0, param_stride=pair.stride,
                        backward_goal=None if goal is None else goal.data_ptr(), phase=ps.phase.data_ptr(), steps_in_phase=ps.sip.data_ptr(),
                        agent_out=None if agent is None else agent.data_ptr(), forward_success=None if fs is None else fs.data_ptr(),
                        backward_success=None if bs is None else bs.data_ptr())


def pair_rollout(h, pair, ps, E, T, reset_first, switch_every, switch_on_success, backward_goal=None, head=None, null=()):
  """earl_tabletop_pair_rollout through the harness `h` -> dict of numpy arrays.  head: None (deterministic) or the keyword arguments of head_struct; names in
  `null` ('obs', ..., 'act', 'eps', 'agent', 'fs', 'bs') are passed as NULL.  `ps` (PairState) is updated in place by the launch"""
  lead = (E, T, h.n) if reset_first else (T, h.n)
  arrs, out = h._outs(lead)
  for k in null:
    if k in OUT:
      setattr(out, k, None)
  act = torch.full(lead + (3,), float('nan'), dtype=torch.float32, device=h.dev)
  eps = torch.full(lead + (3,), float('nan'), dtype=torch.float32, device=h.dev)
  agent = torch.full(lead, 7, dtype=torch.int8, device=h.dev)
  fs = torch.full((E, h.n), -7, dtype=torch.int32, device=h.dev)
  bs = torch.full((E, h.n), -7, dtype=torch.int32, device=h.dev)
  goal = None if backward_goal is None else torch.tensor(np.asarray(backward_goal, np.float64), device=h.dev)
  hd = None if head is None else head_struct(eps_out=None if 'eps' in null else eps.data_ptr(), **head)
  pst = pair_struct(pair, ps, switch_every, switch_on_success, goal, None if 'agent' in null else agent, None if 'fs' in null else fs, None if 'bs' in null else bs)
  st = h._state()
  rc = h.lib.earl_tabletop_pair_rollout(C.byref(h.cfg), C.byref(st), C.byref(pair.struct), C.byref(pst), None if hd is None else C.byref(hd), E, T, int(reset_first),
                                        C.byref(out), None if 'act' in null else act.data_ptr(), h.stream)
  h._ok(rc, 'pair_rollout')
  h.cfg.counter += E * (T + 1) if reset_first else T
  res = {k: a.cpu().numpy() for k, a in zip(OUT, arrs)}
  res.update(act=act.cpu().numpy(), eps=eps.cpu().numpy(), agent=agent.cpu().numpy(), fs=fs.cpu().numpy(), bs=bs.cpu().numpy())
  return res


def single_rollout(h, pol, E, T, reset_first, head=None):
  """the existing single-policy entry point of the head"""
  return gaussian_rollout(h, pol, E, T, reset_first, **head) if head is not None else policy_rollout(h, pol, E, T, reset_first)


def goal_draw(h, counter):
  """sample_goal(cfg, counter, env, NULL) for every env of `h`, through an entry point that existed before the pair: a reset of scratch state with that counter"""
  s = hx.HipTabletop(h.n, device=str(h.dev), seed=int(h.cfg.seed), env_offset=int(h.cfg.env_offset))
  s.cfg.counter = counter
  s.reset()
  return s.host('goal_idx').copy()


def with_goal_row(h, row):
  """append one goal row to the harness's table (the way reset_goal(goal) installs a custom goal) -> its index"""
  gt = np.concatenate([h.goal_table.cpu().numpy(), np.asarray(row, np.float64)[None]], 0)
  h.goal_table = torch.tensor(gt, device=h.dev)
  h.cfg.n_goals = len(gt)
  return len(gt) - 1


def handover_rule(success, done, phase0, sip0, switch_every, switch_on_success, auto_reset, reset_first):
  """the contract's items 5 and 6 applied to a launch's own success / done [E, T, n] -> (agent [E, T, n], phase, sip, fs [E, n], bs [E, n], causes [4]): causes counts
  the handovers (forward by success, forward by clock, reset by success, reset by clock)"""
  E, T, n = success.shape
  phase, sip = phase0.astype(np.int64).copy(), sip0.astype(np.int64).copy()
  se = np.array((switch_every, switch_every) if np.ndim(switch_every) == 0 else switch_every)
  agent = np.zeros((E, T, n), np.int8)
  fs, bs = np.zeros((E, n), np.int32), np.zeros((E, n), np.int32)
  causes = np.zeros(4, np.int64)
  for e in range(E):
    if reset_first:
      phase[:], sip[:] = 0, 0
    for t in range(T):
      agent[e, t] = phase
      reset = done[e, t].astype(bool) & bool(auto_reset)
      s = success[e, t].astype(bool) & bool(switch_on_success)
      sip = np.where(reset, 0, sip + 1)
      over = ~reset & (s | (sip >= se[phase]))
      by_s = over & s
      fs[e] += by_s & (phase == 0)
      bs[e] += by_s & (phase == 1)
      for k, m in enumerate((by_s & (phase == 0), over & ~s & (phase == 0), by_s & (phase == 1), over & ~s & (phase == 1))):
        causes[k] += int(m.sum())
      phase = np.where(reset, 0, np.where(over, phase ^ 1, phase))
      sip = np.where(over, 0, sip)
  return agent, phase.astype(np.int8), sip.astype(np.int32), fs, bs, causes


def assert_bits(got, want, keys):
  for k in keys:
    a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
    assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=k)


def workgroup_shares(agent):
  """agent [..., T, n] -> the shares of (workgroup, step) pairs that are mixed / uniform-forward / uniform-reset, workgroups = 16 consecutive env indices"""
  a = agent.reshape(-1, agent.shape[-1])
  n = a.shape[1]
  mixed = fwd = rst = 0
  for i0 in range(0, n, 16):
    blk = a[:, i0:i0 + 16]
    any1, any0 = (blk == 1).any(axis=1), (blk == 0).any(axis=1)
    mixed += int((any1 & any0).sum())
    fwd += int((any0 & ~any1).sum())
    rst += int((any1 & ~any0).sum())
  tot = mixed + fwd + rst
  return mixed / tot, fwd / tot, rst / tot

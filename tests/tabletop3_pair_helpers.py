"""Shared by tests/test_tabletop3_pair.py (no GPU) and tests/test_tabletop3_pair_gpu.py: what tests/pair_helpers.py offers, at the three-object widths -- the two
agents of a pair packed as [2, n_params + PAD] (20-wide networks), the call of earl_tabletop3_pair_rollout through tests/hip_harness.py's HipTabletop(nobj=3) (either
library), the single-policy launch it is held to (earl_tabletop3_policy_rollout with one policy), the goal draw through a reset of scratch state, and a `still_pair`.
The goal side of the handover rule is restated here in numpy (goal_rule); the phase side (handover_rule), PairState, pair_struct, with_goal_row, assert_bits and
workgroup_shares are pair_helpers' own: they do not depend on the widths."""
import ctypes as C

import numpy as np
import torch

import tabletop3_policy_helpers as t3
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import Packed, head_struct
from pair_helpers import OUT, PAD, PairState, assert_bits, handover_rule, pair_struct, with_goal_row, workgroup_shares      # noqa: F401 (re-exported)

OBS, NG = 20, 10
INITIAL3 = np.array([0.0, 0.0, 2.5, 0.0, 2.5, -1.0, 2.5, 1.0, -1.0, -1.0])      # the env's initial state as a goal row (backward_goal = 'initial')
TASK3 = np.array([0.0, 0.0, 0.0, -2.0, 0.0, 2.0, -2.5, 1.0, -1.0, -1.0])        # the env's one task goal
TABLE3 = np.stack([TASK3, INITIAL3, np.array([1.0, 0.5, 2.0, -2.0, -1.0, 2.0, -2.5, 0.0, -1.0, -1.0])])      # a table the forward handover can draw from (n_sample_goals = 3)


class Pair3:
  """two 20-wide members (tabletop3_policy_helpers.net3, or given as Packed) stacked as [2, n_params + PAD]; the padding holds NaN, which any read past an agent's own
  parameters would carry into the actions"""

  def __init__(self, hidden=(64,), gaussian=False, hidden_act='relu', out_act='tanh', seed0=0, device='cpu', members=None):
    self.members = members or [t3.net3(hidden, hidden_act, out_act, seed=seed0 + p, gaussian=gaussian, device=device) for p in range(2)]
    self.gaussian = gaussian
    rows = torch.stack([m.params for m in self.members])
    self.n_params = rows.shape[1]
    self.params = torch.full((2, self.n_params + PAD), float('nan'), dtype=torch.float32, device=device)
    self.params[:, :self.n_params] = rows
    m = self.members[0].struct
    self.struct = _abi.MlpPolicy(n_layers=m.n_layers, dims=m.dims, hidden_act=m.hidden_act, out_act=m.out_act, precision=0, params=self.params.data_ptr())
    self.stride = self.n_params + PAD


def still_pair(gaussian=False, device='cpu', grip=0.5):
  """agents whose arm stays put whatever they see: zero last-layer weights and zero bias on the two motion rows (tanh(0) = 0 exactly), the bias +grip (forward agent:
  the gripper closes) resp. -grip (reset agent: it opens) on the third -- success is decided by where the goal rows are placed, a hold by where the gripper sits"""
  rng = np.random.default_rng(3)
  nout = 6 if gaussian else 3
  members = []
  for p in range(2):
    w0, b0 = (rng.standard_normal((16, OBS)) / 4).astype(np.float32), (rng.standard_normal(16) * 0.3).astype(np.float32)
    wo, bo = np.zeros((nout, 16), np.float32), np.zeros(nout, np.float32)
    bo[2] = grip * (1 if p == 0 else -1)
    if gaussian:
      bo[3:] = -20.0                                      # raw log_std at the lower bound: sigma = e^-5
    members.append(Packed([(w0, b0), (wo, bo)], 'relu', 'tanh', device))
  return Pair3(gaussian=gaussian, device=device, members=members)


def harness(device, n=t3.N, env_offset=t3.OFFSET, table=TABLE3, **kw):
  """HipTabletop(nobj=3) with a goal table of three rows the forward handover draws from"""
  return t3.harness(device, n=n, env_offset=env_offset, goal_table=table, n_sample_goals=len(table), **kw)


def prepared(device, reset_first, n=t3.N, **kw):
  """a harness in the state a launch starts from: a continuing rollout starts somewhere (a reset and a few scripted steps)"""
  h = harness(device, n=n, **kw)
  h.reset()
  if not reset_first:
    h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, n, 3)).astype(np.float32))
  return h


def pair_rollout3(h, pair, ps, E, T, reset_first, switch_every, switch_on_success, backward_goal=None, head=None, null=()):
  """earl_tabletop3_pair_rollout through the harness `h` -> dict of numpy arrays.  head: None (deterministic) or the keyword arguments of head_struct; names in `null`
  ('obs', ..., 'act', 'eps', 'agent', 'fs', 'bs') are passed as NULL.  `ps` (PairState) is updated in place by the launch"""
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
  assert goal is None or goal.numel() == NG
  hd = None if head is None else head_struct(eps_out=None if 'eps' in null else eps.data_ptr(), **head)
  pst = pair_struct(pair, ps, switch_every, switch_on_success, goal, None if 'agent' in null else agent, None if 'fs' in null else fs, None if 'bs' in null else bs)
  st = h._state()
  rc = h.lib.earl_tabletop3_pair_rollout(C.byref(h.cfg), C.byref(st), C.byref(pair.struct), C.byref(pst), None if hd is None else C.byref(hd), E, T, int(reset_first),
                                         C.byref(out), None if 'act' in null else act.data_ptr(), h.stream)
  h._ok(rc, 'tabletop3_pair_rollout')
  h.cfg.counter += E * (T + 1) if reset_first else T
  res = {k: a.cpu().numpy() for k, a in zip(OUT, arrs)}
  res.update(act=act.cpu().numpy(), eps=eps.cpu().numpy(), agent=agent.cpu().numpy(), fs=fs.cpu().numpy(), bs=bs.cpu().numpy())
  return res


def single_rollout3(h, pol, E, T, reset_first, head=None):
  """the single-policy entry point of the three-object env (one policy, no summaries)"""
  return t3.rollout3(h, pol.struct, E, T, reset_first, head=head, summary=False)


def goal_draw3(h, counter):
  """sample_goal(cfg, counter, env, NULL) for every env of `h`, through an entry point that existed before the pair: a reset of scratch state with that counter"""
  s = t3.harness(str(h.dev), n=h.n, env_offset=int(h.cfg.env_offset), seed=int(h.cfg.seed), goal_table=h.goal_table.cpu().numpy(), n_sample_goals=int(h.cfg.n_sample_goals))
  s.cfg.counter = counter
  s.reset()
  return s.host('goal_idx').copy()


def goal_rule(h, success, done, phase0, sip0, goal_idx0, counter0, switch_every, switch_on_success, auto_reset, backward_goal):
  """the contract's goal side of items 5 and 6 applied to a continuing launch's own success / done [T, n], independent of the env's code but for the draw itself
  (goal_draw3: a reset of scratch state): -> (goal_idx left behind [n], the goal slots 10..19 of every out->obs row [T, n, 10]).  Step t has the Philox counter
  counter0 + t.  An auto-reset redraws goal_idx at that counter and the row of that step stays the terminal one (the goal that was in force); a handover into the
  forward phase redraws goal_idx at that counter and the row carries that table row; a handover into the reset phase leaves goal_idx alone and the row carries the
  backward goal if there is one"""
  T, n = success.shape
  table = h.goal_table.cpu().numpy()
  se = np.array((switch_every, switch_every) if np.ndim(switch_every) == 0 else switch_every)
  phase, sip, gi = phase0.astype(np.int64).copy(), sip0.astype(np.int64).copy(), goal_idx0.astype(np.int64).copy()
  in_force = np.where(((phase == 1) & (backward_goal is not None))[:, None], table[0] if backward_goal is None else np.asarray(backward_goal)[None], table[gi])
  rows = np.zeros((T, n, NG), np.float32)
  for t in range(T):
    reset = done[t].astype(bool) & bool(auto_reset)
    s = success[t].astype(bool) & bool(switch_on_success)
    sip = np.where(reset, 0, sip + 1)
    over = ~reset & (s | (sip >= se[phase]))
    to_forward, to_reset = over & (phase == 1), over & (phase == 0)
    rows[t] = in_force.astype(np.float32)                    # (an auto-reset step's row: the terminal observation, the goal that was in force)
    if (reset | to_forward).any():
      gi = np.where(reset | to_forward, goal_draw3(h, counter0 + t), gi)
    in_force = np.where((reset | to_forward)[:, None], table[gi], in_force)
    if backward_goal is not None:
      in_force = np.where(to_reset[:, None], np.asarray(backward_goal)[None], in_force)
    rows[t] = np.where(over[:, None], in_force, rows[t]).astype(np.float32)
    phase = np.where(reset, 0, np.where(over, phase ^ 1, phase))
    sip = np.where(over, 0, sip)
  return gi.astype(np.int32), rows


def keys_of(head):
  return OUT + ('act',) + (('eps',) if head is not None else ())

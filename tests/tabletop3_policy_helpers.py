"""Shared by tests/test_tabletop3_policy.py (no GPU) and tests/test_tabletop3_policy_gpu.py: packed 20-wide policies with asymmetric random weights, the call of
earl_tabletop3_policy_rollout through tests/hip_harness.py's HipTabletop(nobj=3) (either library), the open loop it is held to (earl_tabletop3_reset +
earl_tabletop3_rollout fed with act_out), and the start states and policy of the coverage condition's run."""
import ctypes as C

import numpy as np
import torch

import hip_harness as hx
from earl_benchmark_amd import _abi
from gaussian_policy_helpers import Packed, head_struct
from policy_width_cases import N, OFFSET, T
from population_helpers import PAD
from test_policy_rollout import final_state, restore, snapshot

OBS = 20
OUT = ('obs', 'reward', 'done', 'success')
SUMMARY = ('ret', 'success_last', 'first_success')


def net3(hidden, hidden_act='relu', out_act='tanh', seed=0, gaussian=False, gain=1.0, log_std_gain=2.0, device='cpu'):
  """test_policy_rollout.Policy / gaussian_policy_helpers.GaussPolicy with a 20-wide input: the last layer's mean rows carry the gain 2.5 (some actions saturate the
  env's clip, some do not), a Gaussian head's raw log_std rows `log_std_gain` and the biases (-2, 0, 1)"""
  rng = np.random.default_rng(seed)
  dims = [OBS] + list(hidden) + [6 if gaussian else 3]
  layers = []
  for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
    w = rng.standard_normal((n, k)) * gain / np.sqrt(k)
    b = rng.standard_normal(n) * 0.3
    if l == len(dims) - 2:
      w[:3] *= 2.5
      if gaussian:
        w[3:] *= log_std_gain
        b[3:] = np.array([-2.0, 0.0, 1.0])
    layers.append((w.astype(np.float32), b.astype(np.float32)))
  return Packed(layers, hidden_act, out_act, device)


def mean_twin(pol, device='cpu'):
  """the 3-output policy made of rows 0..2 of a Gaussian policy's last layer"""
  w, b = pol.layers[-1]
  return Packed(pol.layers[:-1] + [(np.ascontiguousarray(w[:3]), np.ascontiguousarray(b[:3]))], pol.hidden_act, pol.out_act, device)


class Population3:
  """P members stacked as [P, n_params + PAD]; the padding holds NaN, which any read past a member's own parameters would carry into the actions"""

  def __init__(self, hidden, P, G, gaussian=False, hidden_act='relu', out_act='tanh', seed0=0, device='cpu'):
    self.members = [net3(hidden, hidden_act, out_act, seed=seed0 + p, gaussian=gaussian, device=device) for p in range(P)]
    self.G, self.P = G, P
    rows = torch.stack([m.params for m in self.members])
    self.n_params = rows.shape[1]
    self.params = torch.full((P, self.n_params + PAD), float('nan'), dtype=torch.float32, device=device)
    self.params[:, :self.n_params] = rows
    m = self.members[0].struct
    self.struct = _abi.MlpPolicy(n_layers=m.n_layers, dims=m.dims, hidden_act=m.hidden_act, out_act=m.out_act, precision=0, params=self.params.data_ptr())
    self.pop = _abi.PolicyPopulation(n_policies=P, envs_per_policy=G, param_stride=self.n_params + PAD)


def harness(device, n=N, env_offset=OFFSET, **kw):
  return hx.HipTabletop(n, device=device, nobj=3, env_offset=env_offset, **kw)


def rollout3(h, struct, E, T, reset_first, pop=None, head=None, null=(), summary=True):
  """earl_tabletop3_policy_rollout through the harness `h` -> dict of numpy arrays.  head: None (deterministic) or the keyword arguments of head_struct; names in
  `null` ('obs', 'reward', 'done', 'success', 'act', 'eps') are passed as NULL; summary=False passes a NULL summary"""
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
  rc = h.lib.earl_tabletop3_policy_rollout(C.byref(h.cfg), C.byref(st), C.byref(struct), None if pop is None else C.byref(pop), None if hd is None else C.byref(hd),
                                           E, T, int(reset_first), C.byref(out), None if 'act' in null else act.data_ptr(), C.byref(sm) if summary else None, h.stream)
  h._ok(rc, 'tabletop3_policy_rollout')
  h.cfg.counter += E * (T + 1) if reset_first else T
  res = {k: a.cpu().numpy() for k, a in zip(OUT, arrs)}
  res.update(act=act.cpu().numpy(), eps=eps.cpu().numpy(), ret=ret.cpu().numpy(), success_last=last.cpu().numpy(), first_success=first.cpu().numpy())
  return res


def open_loop3(h, act, reset_first):
  """the open-loop entry points fed with recorded actions: per episode earl_tabletop3_reset (all envs) + earl_tabletop3_rollout, or the rollout alone"""
  if not reset_first:
    return dict(zip(OUT, h.rollout(np.ascontiguousarray(act))))
  eps = []
  for e in range(act.shape[0]):
    h.reset()
    eps.append(h.rollout(np.ascontiguousarray(act[e])))
  return {k: np.stack([ep[j] for ep in eps]) for j, k in enumerate(OUT)}


def start_somewhere(h, steps=9):
  """a continuing rollout starts somewhere: a reset and a few scripted steps first"""
  h.reset()
  h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(steps, h.n, 3)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the coverage condition's run
COVERAGE_SEED, COVERAGE_T = 0, T


def coverage_harness(device):
  """N envs whose grippers lie near objects: env i's gripper sits 0.1 .. 0.35 from object i % 3 (the other two are farther than the grasp radius 0.4 from it in
  most envs), a third of the envs hold an object already; the continuing form, no auto-reset"""
  h = harness(device, reward_type='sparse', horizon=10**6, seed=31)
  h.reset()
  rng = np.random.default_rng(COVERAGE_SEED)
  q = h.host('qpos').copy()
  q[:, 0:2] = rng.uniform(-1.5, 1.5, size=(N, 2))
  q[:, 2:8] = rng.uniform(-2.5, 2.5, size=(N, 6))
  for i in range(N):
    k, r, th = i % 3, rng.uniform(0.1, 0.35), rng.uniform(0, 2 * np.pi)
    q[i, 2 + 2 * k:4 + 2 * k] = q[i, 0:2] + r * np.array([np.cos(th), np.sin(th)])
  att = np.where(np.arange(N) % 3 == 2, (np.arange(N) // 3) % 3, -1).astype(np.int8)
  h.qpos.copy_(torch.from_numpy(q))
  h.attached.copy_(torch.from_numpy(att))
  return h


def coverage_policy(device):
  return net3((48,), 'tanh', 'tanh', seed=COVERAGE_SEED, gain=0.5, device=device)


def coverage_of(att0, res):
  """(objects latched during the run, envs that released, action dimensions with a component strictly inside (-1, 1)) from the start flags, obs and act_out [T, n, ..]"""
  flag = res['obs'][..., 8]                                             # -1 free, 0 / 0.5 / 1 holding object 0 / 1 / 2
  held = np.concatenate([att0[None].astype(np.float32) * 0.5 * (att0[None] >= 0) - (att0[None] < 0), flag])
  latched = {int(round(2 * v)) for v in held[1:][(held[:-1] < 0) & (held[1:] >= 0)]}
  released = int(((held[:-1] >= 0) & (held[1:] < 0)).any(axis=0).sum())
  inside = [bool((np.abs(res['act'][..., d]) < 1).any()) for d in range(3)]
  return latched, released, inside


def closed_equals_open3(h, struct, E, T, reset_first, **kw):
  """the launch == the open-loop entry points of the same library fed with act_out: outputs, state left behind, counter -> (the launch's results, start snapshot)"""
  from test_policy_rollout import assert_same_bits, assert_same_state
  snap = snapshot(h)
  got = rollout3(h, struct, E, T, reset_first, **kw)
  end = final_state(h)
  assert not np.isnan(got['act']).any()
  restore(h, snap)
  want = open_loop3(h, got['act'], reset_first)
  assert_same_bits(got, want)
  assert_same_state(end, final_state(h))
  return got, snap

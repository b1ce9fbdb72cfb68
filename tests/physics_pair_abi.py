"""Driver of earl_minitaur_agents_rollout / earl_kitchen_agents_rollout (include/earl_physics.h) for tests/test_minitaur_pair_gpu.py and tests/test_kitchen_pair_gpu.py: a
plain module, no fixtures and no tests here.  It builds on tests/population_abi.py (banded launches from a `Snapshot`, the summary's definitions, the guard cap),
tests/physics_abi.py (`Snapshot`, `run`: the plain rollout entry points) and tests/pair_helpers.py::handover_rule.

- `Pairs`: P forward / reset pairs stacked as [P, 2, stride], the padding NaN (a read past an agent's own parameters would carry it into the actions).
- `launch`: one pair launch of rows [lo, hi) of a snapshot through the C ABI, every buffer inside guard bands, every optional pointer replaceable by NULL.
- `expected`: items 5 and 6 of the contract applied on the host to a launch's own success flags: phases, counters, the goal rows with the 0xFFFD / 0xFFFE draws
  recomputed in numpy.
- `stepwise`: the procedure that does not run the code under test: T launches of the plain `*_rollout_clocked` with the pair launch's actions, the handover rule and
  the goal rows applied by the test between them.
- the bodies of the assertions the two envs share."""
import contextlib
import copy
import ctypes as C

import numpy as np
import torch

import physics_abi as ab
import population_abi as pa
from earl_benchmark_amd import _abi
from pair_helpers import handover_rule
from physics_abi import A_DIM, OBS_DIM, OUTS, STATE_FIELDS, Bands, same, stream

G = pa.G
GOAL_W = {'minitaur': 2, 'kitchen': 23}                                  # doubles of a goal row
GOAL_AT = {'minitaur': 30, 'kitchen': 23}                                # where the goal block starts in an observation row
SE = (3, 2)                                                              # switch_every of the tests
PAIR_KEYS = ('pair.phase', 'pair.sip', 'pair.fs', 'pair.bs', 'goals.row')            # rows [n]
PAIR_T_KEYS = ('pair.agent', 'goals.row_out')                            # rows [T, n]
BACK_DRAW, FWD_DRAW = 0xFFFD, 0xFFFE


def counter0(snap):
  """the counter the draws of a launch's step 0 are keyed with (population_abi.launch sets the same)"""
  return snap.step_counter if snap.kind == 'minitaur' else 1000 + 7 * snap.n


class Pairs:
  """members: [((forward policy, its host layers), (reset policy, its host layers))] of one architecture, as the tests' `policy()` returns them"""

  def __init__(self, kind, members, pad=8):
    self.kind, self.first = kind, members[0][0][0]
    self.count = int(self.first.params.numel())
    self.pair_stride = (self.count + pad + 3) // 4 * 4
    rows = torch.full((len(members), 2, self.pair_stride), float('nan'), dtype=torch.float32)
    for p, pair in enumerate(members):
      for k in (0, 1):
        rows[p, k, :self.count] = pair[k][0].params.detach().cpu()
    assert not torch.equal(rows[0, 0, :self.count], rows[0, 1, :self.count])      # the two agents differ
    self.params = rows.cuda().contiguous()
    self.layers = [[pair[0][1], pair[1][1]] for pair in members]
    self.P, self.hidden_act = len(members), self.first.hidden_act

  def struct_at(self, p=0, k=0):
    s = self.first.struct
    return _abi.MlpPolicy(n_layers=s.n_layers, dims=s.dims, hidden_act=s.hidden_act, out_act=s.out_act, precision=0, params=self.params[p, k].data_ptr())

  @property
  def pop_struct(self):
    return _abi.PolicyPopulation(n_policies=self.P, envs_per_policy=G, param_stride=2 * self.pair_stride)

  def head(self, sample=True, eps_out=None):
    return self.first.head(sample=sample, eps_out=eps_out)

  def row(self, k):
    """agent k of every pair as a population of single policies (earl_*_population_rollout reads the same memory)"""
    return _Row(self, k)


class _Row:
  def __init__(self, pairs, k):
    self.struct, self.pop_struct, self.head, self._keep = pairs.struct_at(0, k), pairs.pop_struct, pairs.head, pairs


def make_pairs(kind, policy, n, off, hidden, head, hidden_act='relu'):
  members = [(policy(hidden, hidden_act, head=head, seed=100 + 2 * p), policy(hidden, hidden_act, head=head, seed=101 + 2 * p)) for p in range((off + n - 1) // G + 1)]
  return Pairs(kind, members)


def stagger(snap):
  """phase = g % 2, steps_in_phase = g % 3 by global id: every wave is mixed"""
  g = int(snap.env._cfg.env_offset) + np.arange(snap.n)
  return (g % 2).astype(np.int8), (g % 3).astype(np.int32)


def launch(snap, T, fill, pairs, head=None, phase=None, sip=None, se=SE, sos=1, goal=None, table=None, fwd=None, goal_table=None, pop=True, member=0, rows=None, null=(),
           summary=True, obs0=None, state=None, dt=0, row0=None):
  """one launch of earl_<kind>_agents_rollout over rows [lo, hi) of the snapshot (state: {field: full-batch tensor} instead of the snapshot's).
  phase / sip: full-batch arrays (default: all 0); goal: ONE backward row, or table [R, W]; fwd: the kitchen's forward table [R, 23]; goal_table: the minitaur's
  cfg.goal_table [R, 2] instead of the env's; pop=False: the pair `member` alone, pop = NULL; dt: added to the launch's step counter; row0: goals->row before.
  null: as population_abi.launch plus 'pair.agent', 'pair.fs', 'pair.bs', 'goals.row', 'goals.row_out'.
  -> (results incl. PAIR_KEYS / PAIR_T_KEYS without what was NULL or not asked for, Bands)"""
  kind, env = snap.kind, snap.env
  lo, hi = rows if rows is not None else (0, snap.n)
  m, A, W = hi - lo, A_DIM[kind], GOAL_W[kind]
  null = set(null)
  src = snap.state if state is None else state
  b = Bands(fill)
  dev = dict(device='cuda')
  for f, _ in STATE_FIELDS[kind]:
    b.like('st.' + f, src[f][lo:hi].contiguous())
  for name, dty, row in OUTS[kind]:
    b.new('out.' + name, (T, m, row) if row > 1 else (T, m), dty, m * row)
  b.new('actions', (T, m, A), torch.float32, m * A)
  b.new('eps', (T, m, A), torch.float32, m * A)
  b.new('sum.ret', (m,), torch.float64, m)
  b.new('sum.last', (m,), torch.uint8, m)
  b.new('sum.first', (m,), torch.int32, m)
  b.like('obs0', (src['last_obs'][lo:hi] if obs0 is None else obs0).contiguous())
  ph = np.zeros(snap.n, np.int8) if phase is None else np.asarray(phase, np.int8)
  sp = np.zeros(snap.n, np.int32) if sip is None else np.asarray(sip, np.int32)
  b.like('pair.phase', torch.as_tensor(ph[lo:hi].copy(), **dev))
  b.like('pair.sip', torch.as_tensor(sp[lo:hi].copy(), **dev))
  b.new('pair.agent', (T, m), torch.int8, m, interior=0x55)
  b.new('pair.fs', (m,), torch.int32, m, interior=0x55)
  b.new('pair.bs', (m,), torch.int32, m, interior=0x55)
  tensor64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), **dev)
  if goal is not None:
    b.like('goal', tensor64(goal).reshape(W))
  if table is not None:
    b.like('table', tensor64(table).reshape(-1, W))
    b.like('goals.row', torch.full((m,), -1, dtype=torch.int32, **dev) if row0 is None else torch.as_tensor(np.asarray(row0, np.int32)[lo:hi].copy(), **dev))
    b.new('goals.row_out', (T, m), torch.int32, m, interior=0x55)
  if fwd is not None:
    b.like('fwd', tensor64(fwd).reshape(-1, W))
  if goal_table is not None:
    b.like('goal_table', tensor64(goal_table).reshape(-1, 2))
  cfg = type(env._cfg).from_buffer_copy(env._cfg)
  cfg.n, cfg.env_offset = m, int(env._cfg.env_offset) + lo
  if kind == 'minitaur':
    cfg.goal_change_frequency, cfg.step_counter = snap.gcf, counter0(snap) + dt
    if goal_table is not None:
      cfg.goal_table, cfg.n_goals = b['goal_table'].data_ptr(), int(b['goal_table'].shape[0])
  else:
    cfg.counter = counter0(snap) + dt
  stp = {f: b.ptr('st.' + f, null) for f, _ in STATE_FIELDS[kind]}
  o = (_abi.KitchenOut if kind == 'kitchen' else _abi.MinitaurOut)(**{name: b.ptr('out.' + name, null) for name, _, _ in OUTS[kind]})
  st = (_abi.KitchenState if kind == 'kitchen' else _abi.MinitaurState)(**stp)
  hd = None if head is None else pairs.head(sample=head == 'sample', eps_out=None if 'eps' in null else b['eps'])
  ps = _abi.AgentPair(switch_every=(C.c_int32 * 2)(*se), switch_on_success=int(sos), pad_=0, param_stride=pairs.pair_stride, backward_goal=b.ptr('goal'),
                      phase=b['pair.phase'].data_ptr(), steps_in_phase=b['pair.sip'].data_ptr(), agent_out=b.ptr('pair.agent', null),
                      forward_success=b.ptr('pair.fs', null), backward_success=b.ptr('pair.bs', null))
  gl = None if table is None else _abi.BackwardGoals(table=b['table'].data_ptr(), n_rows=int(b['table'].shape[0]), pad_=0, row=b.ptr('goals.row', null),
                                                     row_out=b.ptr('goals.row_out', null))
  sm = _abi.EpisodeSummary(ret=b['sum.ret'].data_ptr(), success_last=b['sum.last'].data_ptr(), first_success=b['sum.first'].data_ptr()) if summary else None
  ref = lambda s: None if s is None else C.byref(s)
  pol = pairs.struct_at(0 if pop else member, 0)
  popst = pairs.pop_struct if pop else None
  lib, mod = env._lib, env.model
  pre = (mod.buf.data_ptr(), mod.col_ptr) + ((C.byref(env._params),) if kind == 'kitchen' else ()) + (C.byref(cfg), C.byref(st), C.byref(pol), C.byref(ps), ref(popst), ref(gl))
  mid = (b.ptr('fwd'), 0 if fwd is None else int(b['fwd'].shape[0])) if kind == 'kitchen' else ()
  post = (ref(hd), b['obs0'].data_ptr(), T, None, b.ptr('actions', null), C.byref(o), ref(sm), stream())
  rc = getattr(lib, f'earl_{kind}_agents_rollout')(*pre, *mid, *post)
  _abi.check(rc, f'{kind} agents rollout')
  torch.cuda.synchronize()
  b.check(f'{kind} pair rows {lo}:{hi} null={sorted(null)} fill {fill:#x}')
  skip = null | {'obs0', 'goal', 'table', 'fwd', 'goal_table'} | (set() if head is not None else {'eps'}) | (set() if summary else {'sum.ret', 'sum.last', 'sum.first'})
  return {k: v[3].clone() for k, v in b.bufs.items() if k not in skip}, b


def concat(parts):
  """the pieces' results side by side along the env axis"""
  env_first = lambda k: k.startswith(('st.', 'sum.')) or k in PAIR_KEYS
  return {k: torch.cat([p[k] for p in parts], dim=0 if env_first(k) else 1) for k in parts[0]}


def same_results(a, bb, what, keys=None):
  for k in (keys if keys is not None else sorted(set(a) & set(bb))):
    same(a[k], bb[k], f'{what}: {k}')


# ---------------------------------------------------------------------------------------------------------------- the contract on the host
def draw(index, seed, gids, ev, rows):
  """min(int(u01(b.x, b.y) rows), rows - 1) of the Philox block {index, global id, ev lo, ev hi} under key seed, per env"""
  from gaussian_policy_helpers import philox4x32_10
  gids = np.asarray(gids, np.uint64)
  evs = np.full(len(gids), ev, np.uint64)
  x, y, _, _ = philox4x32_10(np.full(len(gids), index, np.uint64), gids, evs & np.uint64(0xFFFFFFFF), evs >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
  u01 = (((y << np.uint64(32)) | x) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
  return np.minimum((u01 * float(rows)).astype(np.int64), rows - 1)


class Host:
  """items 5 and 6 step by step: phase, steps_in_phase, counters, the goal in force and the table rows, advanced with one step's success flags at a time"""

  def __init__(self, snap, phase, sip, goal_rows, se=SE, sos=1, goal=None, table=None, fwd=None, rows=None, dt=0, row0=None):
    lo, hi = rows if rows is not None else (0, snap.n)
    self.gids = int(snap.env._cfg.env_offset) + np.arange(lo, hi)
    self.seed, self.ev0 = int(snap.env._cfg.seed), counter0(snap) + dt
    self.phase, self.sip = np.asarray(phase)[lo:hi].astype(np.int64), np.asarray(sip)[lo:hi].astype(np.int64)
    self.goal = np.array(goal_rows[lo:hi], np.float64)
    self.se, self.sos = np.asarray(se), bool(sos)
    self.back = None if goal is None and table is None else np.asarray(goal if table is None else table, np.float64).reshape(-1, self.goal.shape[1])
    self.tabled = table is not None
    self.fwd = None if fwd is None else np.asarray(fwd, np.float64).reshape(-1, self.goal.shape[1])
    m = hi - lo
    self.fs, self.bs, self.causes = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(4, np.int64)
    self.row = np.full(m, -1, np.int32) if row0 is None else np.asarray(row0, np.int32)[lo:hi].copy()
    self.t = 0

  def step(self, success):
    """-> (agent of this step [m], row_out of this step [m], changed [m]: the envs whose goal row was rewritten); self.goal is the goal in force afterwards"""
    agent = self.phase.astype(np.int8)
    s = np.asarray(success).astype(bool) & self.sos
    self.sip = self.sip + 1
    over = s | (self.sip >= self.se[self.phase])
    for k, msk in enumerate((over & s & (self.phase == 0), over & ~s & (self.phase == 0), over & s & (self.phase == 1), over & ~s & (self.phase == 1))):
      self.causes[k] += int(msk.sum())
    self.fs += (over & s & (self.phase == 0)).astype(np.int32)
    self.bs += (over & s & (self.phase == 1)).astype(np.int32)
    to_reset, to_fwd = over & (self.phase == 0), over & (self.phase == 1)
    row_out = np.full(len(agent), -1, np.int32)
    changed = np.zeros(len(agent), bool)
    if self.back is not None:
      r = draw(BACK_DRAW, self.seed, self.gids, self.ev0 + self.t, len(self.back))
      self.goal[to_reset] = self.back[r][to_reset]
      changed |= to_reset
      if self.tabled:
        row_out[to_reset] = r[to_reset]
        self.row[to_reset] = r[to_reset]
    if self.fwd is not None:
      r = draw(FWD_DRAW, self.seed, self.gids, self.ev0 + self.t, len(self.fwd))
      self.goal[to_fwd] = self.fwd[r][to_fwd]
      changed |= to_fwd
    self.phase = np.where(over, self.phase ^ 1, self.phase)
    self.sip = np.where(over, 0, self.sip)
    self.t += 1
    return agent, row_out, changed


def forward_table(snap, fwd=None, goal_table=None):
  """what a forward entry draws from: the kitchen's forward_goals (None: the goal stays), the minitaur's cfg.goal_table"""
  if snap.kind == 'kitchen':
    return fwd
  return snap.env._goal_table.cpu().numpy() if goal_table is None else np.asarray(goal_table, np.float64)


def check_handover(snap, res, what, phase, sip, se=SE, sos=1, goal=None, table=None, fwd=None, goal_table=None, rows=None, dt=0, state=None):
  """1: agent, final phase / steps_in_phase, both counters, st->goal, the patched goal blocks and the table rows == items 5 and 6 applied to the launch's own success
  -> causes [4]: handovers (forward by success, forward by clock, reset by success, reset by clock)"""
  kind = snap.kind
  lo, hi = rows if rows is not None else (0, snap.n)
  at, W = GOAL_AT[kind], GOAL_W[kind]
  goal0 = (snap.state if state is None else state)['goal'].cpu().numpy()
  h = Host(snap, phase, sip, goal0, se, sos, goal, table, forward_table(snap, fwd, goal_table), rows, dt)
  suc = res['out.success'].cpu().numpy() != 0
  T = suc.shape[0]
  agent, row_out, goal_after = np.zeros((T, hi - lo), np.int8), np.zeros((T, hi - lo), np.int32), np.zeros((T, hi - lo, W))
  for t in range(T):
    agent[t], row_out[t], _ = h.step(suc[t])
    goal_after[t] = h.goal
  # tests/pair_helpers.py's statement of the same rule (no resets inside a launch)
  a2, p2, s2, f2, b2, c2 = handover_rule(suc[None], np.zeros_like(suc[None]), np.asarray(phase)[lo:hi], np.asarray(sip)[lo:hi], se, sos, False, False)
  assert np.array_equal(a2[0], agent) and np.array_equal(p2, h.phase) and np.array_equal(s2, h.sip) and np.array_equal(f2[0], h.fs) and np.array_equal(b2[0], h.bs)
  assert np.array_equal(c2, h.causes)
  t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda')
  same(res['pair.agent'], t64(agent), what + ': agent')
  same(res['pair.phase'], t64(h.phase.astype(np.int8)), what + ': phase')
  same(res['pair.sip'], t64(h.sip.astype(np.int32)), what + ': steps_in_phase')
  same(res['pair.fs'], t64(h.fs), what + ': forward_success')
  same(res['pair.bs'], t64(h.bs), what + ': backward_success')
  same(res['st.goal'], t64(h.goal), what + ': st->goal is the goal in force at launch exit')
  same(res['out.obs'][:, :, at:at + W].contiguous(), t64(goal_after), what + ': the goal block of every emitted row is the goal in force after its step')
  same(res['st.last_obs'], res['out.obs'][-1], what + ': last_obs is the last emitted row')
  if table is not None:
    same(res['goals.row_out'], t64(row_out), what + ': row_out is the recomputed 0xFFFD draw, -1 elsewhere')
    same(res['goals.row'], t64(h.row), what + ': goals->row is the last drawn row')
  print(f'{what}: handovers (forward by success, forward by clock, reset by success, reset by clock) = {h.causes.tolist()}')
  return h.causes


def check_actions(snap, res, pairs, head, what, obs0=None, member_of=None):
  """2: actions[t] == earl_mlp_policy_forward_cpu of float32(the row emitted at t - 1, goal patch included; obs0 at t = 0) with the parameters of agent[t]'s row of the
  env's member, and eps as returned"""
  from test_sawyer_policy_rollout import forward_cpu
  kind = snap.kind
  T, n = res['out.obs'].shape[:2]
  first = (snap.state['last_obs'] if obs0 is None else obs0).cpu().numpy()
  x = np.concatenate([first[None], res['out.obs'].cpu().numpy()[:-1]]).astype(np.float32).reshape(T * n, OBS_DIM[kind])
  agent = res['pair.agent'].cpu().numpy().reshape(T * n)
  member = np.tile(np.zeros(n, np.int64) if member_of is None else np.asarray(member_of), T)
  eps = res['eps'].cpu().numpy().reshape(T * n, A_DIM[kind]) if head == 'sample' else None
  hd = None if head is None else ({'mean': 0, 'sample': 1}[head], _abi.LOGSTD_MAPS['clamp'], -5.0, 2.0)
  want = np.full((T * n, A_DIM[kind]), np.nan, np.float32)
  for p in np.unique(member):
    for k in (0, 1):
      sel = (member == p) & (agent == k)
      if sel.any():
        want[sel] = forward_cpu(pairs.layers[p][k], pairs.hidden_act, 'tanh', x[sel], head=hd, eps=None if eps is None else eps[sel])
  got = res['actions'].cpu().numpy().reshape(T * n, A_DIM[kind])
  np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what + ': actions per phase')
  assert (agent == 0).any() and (agent == 1).any()


@contextlib.contextmanager
def _counter_of(snap, value):
  """physics_abi.run keys the kitchen's draws with the env's own cfg.counter and the minitaur's with snap.step_counter: set for the block, restored afterwards"""
  if snap.kind == 'kitchen':
    prev, snap.env._cfg.counter = int(snap.env._cfg.counter), value
  else:
    prev, snap.step_counter = snap.step_counter, value
  try:
    yield
  finally:
    if snap.kind == 'kitchen':
      snap.env._cfg.counter = prev
    else:
      snap.step_counter = prev


def stepwise(snap, actions, phase, sip, se=SE, sos=1, goal=None, table=None, fwd=None):
  """3: T launches of the plain earl_<kind>_rollout_clocked with actions[t:t+1]; after each the handover rule on the host, the goal rows written and the goal block of
  last_obs (and of the returned row) patched by the test.  Full batch, the env's own goal table.  -> results in launch()'s keys"""
  kind, at, W = snap.kind, GOAL_AT[snap.kind], GOAL_W[snap.kind]
  s2 = copy.copy(snap)
  s2.state = {k: v.clone() for k, v in snap.state.items()}
  h = Host(snap, phase, sip, snap.state['goal'].cpu().numpy(), se, sos, goal, table, forward_table(snap, fwd))
  T = actions.shape[0]
  outs, agents, row_outs = [], [], []
  for t in range(T):
    with _counter_of(s2, counter0(snap) + t):
      res, _ = ab.run(s2, actions[t:t + 1].contiguous(), 0x00)
    s2.state = {f: res['st.' + f] for f, _ in STATE_FIELDS[kind]}
    agent, row_out, changed = h.step(res['out.success'][0].cpu().numpy() != 0)
    msk = torch.as_tensor(changed, device='cuda')
    new = torch.as_tensor(h.goal, device='cuda')
    s2.state['goal'][msk] = new[msk]
    s2.state['last_obs'][:, at:at + W][msk] = new[msk]
    res['out.obs'][0, :, at:at + W][msk] = new[msk]
    outs.append({k: v for k, v in res.items() if k.startswith('out.')})
    agents.append(agent)
    row_outs.append(row_out)
  t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda')
  want = {k: torch.cat([o[k] for o in outs]) for k in outs[0]}
  want.update({'st.' + f: s2.state[f] for f, _ in STATE_FIELDS[kind]})
  want.update({'pair.agent': t64(np.stack(agents)), 'pair.phase': t64(h.phase.astype(np.int8)), 'pair.sip': t64(h.sip.astype(np.int32)), 'pair.fs': t64(h.fs),
               'pair.bs': t64(h.bs)})
  if table is not None:
    want.update({'goals.row_out': t64(np.stack(row_outs)), 'goals.row': t64(h.row)})
  return want


def check_summary(res, what):
  pa.check_summary(res, what)


def all_four_events(causes, what):
  assert all(int(c) >= 1 for c in causes), f'{what}: every handover cause must occur (forward / reset by success / clock): {list(causes)}'

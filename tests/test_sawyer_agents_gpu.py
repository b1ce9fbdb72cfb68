"""earl_sawyer_agents_rollout on the device (include/earl_physics.h; env.rollout_agents with a table of backward goals or a PairPopulation, env.evaluate_agents).
Every comparison is bit for bit.  The oracles are entry points that existed before (earl_sawyer_pair_rollout, rollout) and numpy:
  1. a table of ONE row, and a table of five equal rows, == earl_sawyer_pair_rollout with that row;
  2. the draw: at every entry into the reset phase the goal block, 'backward_row' and env.backward_row are the row of the Philox draw 0xFFFD recomputed on the host;
     forward entries still follow the 0xFFFE draw; all fifteen rows of the peg's table occur at n = 4160;
  3. one launch == the step-by-step procedure of rollout(actions[t:t+1]) launches with the goal rows written by the test;
  4. T launches of one == one launch of T; two ragged shards == the batch;
  5. a PairPopulation == its pieces, with and without a table, rows padded with NaN;
  6. evaluate_agents == the definitions applied to rollout_agents' arrays from the same state, the same end state, no [T, N] allocation;
  7. every optional pointer NULL in turn leaves the rest what it was; the Python surface, the tabletop's refusals included.
Shapes and seeds are tests/test_sawyer_pair_gpu.py's: T = 23, switch_every = (5, 3), door 64 (one-wave build) and 4160 (eight-wave build), peg 64 and 4160 (time-sliced
schedule, slices of 10 steps), phase state staggered by global index.  Every test prints the share of rows in the failure guard and holds it to MAX_GUARD_SHARE."""
import ctypes as C

import numpy as np
import pytest

from pair_helpers import assert_bits
from test_physics_step_graph_gpu import STATE, make, same
from test_sawyer_pair_gpu import OUT_KEYS, SE, SHAPES, T, goal_draw, guard_share_host, host, make_env, make_pair, reset_row, same_state, stagger, state_of
from test_sawyer_policy_rollout_gpu import MAX_GUARD_SHARE, guard_share
from test_sawyer_population_gpu import by_definition, rows_of, same_np

pytestmark = pytest.mark.gpu

BACK_DRAW = 0xFFFD


def back_draw(u, step, rows):
  """the backward table's draw of env step `step` for every env -> row indices [n]: Philox block {0xFFFD, global id, ev}, u01 = (y:x >> 11) 2^-53,
  index = min(int(u01 rows), rows - 1) -- the counter words, u01 and clamp of goal_draw"""
  from gaussian_policy_helpers import philox4x32_10
  n, seed = u.num_envs, int(u._cfg.seed)
  gid = np.uint64(int(u._cfg.env_offset)) + np.arange(n, dtype=np.uint64)
  ev = np.full(n, step, np.uint64)
  x, y, _, _ = philox4x32_10(np.full(n, BACK_DRAW, np.uint64), gid, ev & np.uint64(0xFFFFFFFF), ev >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
  u01 = (((y << np.uint64(32)) | x) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
  return np.minimum((u01 * float(rows)).astype(np.int64), rows - 1)


def door_table(u):
  """five backward goals around the door's reset row, distinct in the object entries"""
  row = reset_row(u).cpu().numpy()
  table = np.repeat(row[None], 5, 0)
  table[:, 4:7] += 0.01 * np.arange(1, 6)[:, None] * np.array([1.0, -0.5, 0.25])
  return table


def table_of(kind, u):
  """-> (what AgentPair takes as backward_goal, the rows on the host)"""
  if kind == 'peg':
    return 'initial_states', np.asarray(u.initial_states, dtype=np.float64)
  table = door_table(u)
  return table, table


def share(out, what):
  g = guard_share_host(out) if isinstance(out['status'], np.ndarray) else guard_share(out)
  print(f'{what}: guard share {g:.5f}')
  assert g <= MAX_GUARD_SHARE
  return g


def raw(u, pair, entry, head=False, goal=None, table=None, pop=None, summary=False, null=(), rubbish=77):
  """one direct call of earl_sawyer_pair_rollout ('pair') or earl_sawyer_agents_rollout ('agents') on the env's own structs from its current state, every output given
  but those named in `null`; counters, summary and row_out start as rubbish, `row` (caller-owned) as -1.  The env's bookkeeping is left alone: the caller restores."""
  import torch
  from earl_benchmark_amd import _abi
  n, kw = u.num_envs, dict(device='cuda')
  keep = u._new_out((T,), info=u.nv >= 15)
  keep['actions'], keep['agent'] = torch.empty(T, n, 4, dtype=torch.float32, **kw), torch.empty(T, n, dtype=torch.int8, **kw)
  keep['fs'], keep['bs'] = torch.full((n,), rubbish, dtype=torch.int32, **kw), torch.full((n,), -rubbish, dtype=torch.int32, **kw)
  if head:
    keep['eps'] = torch.empty(T, n, 4, dtype=torch.float32, **kw)
  if table is not None:
    keep['row'], keep['row_out'] = torch.full((n,), -1, dtype=torch.int32, **kw), torch.full((T, n), rubbish, dtype=torch.int32, **kw)
  if summary:
    keep['ret'], keep['last'] = torch.full((n,), 1e300, dtype=torch.float64, **kw), torch.ones(n, dtype=torch.bool, **kw)
    keep['first'] = torch.full((n,), 12345, dtype=torch.int32, **kw)
  ptr = lambda k: keep[k].data_ptr() if k in keep and k not in null else None
  ref = lambda s: None if s is None else C.byref(s)
  o = _abi.SawyerOut(obs=ptr('obs'), reward=ptr('reward'), done=ptr('done'), success=ptr('success'), status=ptr('status'), info=ptr('info'))
  ps = _abi.AgentPair(switch_every=(C.c_int32 * 2)(*pair.switch_every), switch_on_success=int(pair.switch_on_success), pad_=0, param_stride=pair.pair_stride,
                      backward_goal=None if goal is None else goal.data_ptr(), phase=u.agent_phase.data_ptr(), steps_in_phase=u.steps_in_phase.data_ptr(),
                      agent_out=ptr('agent'), forward_success=ptr('fs'), backward_success=ptr('bs'))
  hd = pair.head(sample=True, eps_out=None if 'eps' in null else keep['eps']) if head else None
  assert not u._last_obs_stale
  u._cfg.step_counter = u.total_step_count
  if u._uses_queue(T):
    u.sched.zero_()
  common = (u.model.buf.data_ptr(), u.model.col_ptr, u.nv, u._cfg_ref, u._st_ref, C.byref(pair.struct), C.byref(ps))
  tail = (ref(hd), u.last_obs.data_ptr(), T, None, ptr('actions'), C.byref(o))
  if entry == 'pair':
    assert table is None and pop is None and not summary
    _abi.check(u._lib.earl_sawyer_pair_rollout(*common, *tail, u._stream()), 'earl_sawyer_pair_rollout')
  else:
    goals = None if table is None else _abi.BackwardGoals(table=table.data_ptr(), n_rows=int(table.shape[0]), pad_=0, row=ptr('row'), row_out=ptr('row_out'))
    sm = _abi.EpisodeSummary(ret=ptr('ret'), success_last=ptr('last'), first_success=ptr('first')) if summary else None
    _abi.check(u._lib.earl_sawyer_agents_rollout(*common, ref(pop), ref(goals), *tail, ref(sm), u._stream()), 'earl_sawyer_agents_rollout')
  torch.cuda.synchronize()
  keep['phase'], keep['sip'] = u.agent_phase.clone(), u.steps_in_phase.clone()
  keep.update({'state:' + k: v for k, v in state_of(u).items()})
  return {k: v for k, v in keep.items() if k not in null}


def same_dicts(a, b, what, skip=()):
  assert set(a) - set(skip) == set(b) - set(skip), (what, sorted(set(a) ^ set(b)))
  for k in a:
    if k not in skip:
      same(a[k], b[k], f'{what}: {k}')


# ---------------------------------------------------------------------------------------------------------------- 1. a table of one row == the fixed row
@pytest.mark.parametrize('kind,n', SHAPES)
@pytest.mark.parametrize('head', [None, 'sample'])
def test_a_table_of_one_row_and_of_equal_rows_equals_the_pair_entry_point(kind, n, head):
  """outputs, actions, eps, agent, state, fail_count, phase words and counters; the five-row table draws (row_out holds indices 0..4) and installs the same row"""
  import torch
  env = make_env(kind, n)
  u = env.unwrapped
  row = reset_row(u).contiguous()
  pair, _ = make_pair(head=head, seed=n, sos=True)
  sd = u.state_dict()
  runs = []
  for entry, kw in (('pair', dict(goal=row)), ('agents', dict(table=row[None].contiguous())), ('agents', dict(table=row[None].repeat(5, 1).contiguous()))):
    u.load_state_dict(sd)
    stagger(u)
    runs.append(raw(u, pair, entry, head=bool(head), **kw))
  want, one, five = runs
  share({'status': want['status']}, f'{kind} n={n} head={head}')
  same_dicts(want, one, 'one row', skip=('row', 'row_out'))
  same_dicts(want, five, 'five equal rows', skip=('row', 'row_out'))
  after = torch.cat([want['agent'][1:], want['phase'][None]])
  entered = (want['agent'] == 0) & (after == 1)
  assert int(entered.sum()) > n
  assert bool((one['row_out'][entered] == 0).all()) and bool((one['row_out'][~entered] == -1).all())
  drawn = five['row_out'][entered]
  assert bool((five['row_out'][~entered] == -1).all()) and int(drawn.min()) == 0 and int(drawn.max()) == 4
  assert bool((one['row'][entered.any(0)] == 0).all()) and bool((one['row'][~entered.any(0)] == -1).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the draw
@pytest.mark.parametrize('kind,n', SHAPES)
def test_the_reset_goal_is_the_row_of_the_recomputed_draw(kind, n):
  env = make_env(kind, n)
  u = env.unwrapped
  given, table = table_of(kind, u)
  pair, _ = make_pair(seed=n, sos=True, goal=given)
  env.rollout_agents(pair, 2)                                             # (the launch under test starts at a step counter that is not 0)
  assert u.backward_row is not None
  u.backward_row.fill_(-1)                                                # (what the two steps may have drawn is put aside)
  ph0, _ = stagger(u)
  step0 = u.total_step_count
  out = host(env.rollout_agents(pair, T))
  share(out, f'{kind} n={n}')
  assert out['backward_row'].shape == (T, n) and out['backward_row'].dtype == np.int32
  agent = out['agent'].astype(np.int64)
  np.testing.assert_array_equal(agent[0], ph0)
  after = np.concatenate([agent[1:], u.agent_phase.cpu().numpy().astype(np.int64)[None]])
  entered, left = (agent == 0) & (after == 1), (agent == 1) & (after == 0)
  assert entered.sum() > n and left.sum() > n
  r = np.stack([back_draw(u, step0 + t, len(table)) for t in range(T)])
  np.testing.assert_array_equal(out['backward_row'], np.where(entered, r, -1).astype(np.int32))
  assert_bits({'goal block': out['obs'][..., 7:][entered]}, {'goal block': table[r[entered]]}, ('goal block',))
  fwd = np.stack([goal_draw(u, step0 + t)[0] for t in range(T)])
  assert_bits({'goal block': out['obs'][..., 7:][left]}, {'goal block': fwd[left]}, ('goal block',))
  # env.backward_row: the last row drawn, -1 for an env that never entered (the envs staggered into phase 1 among them, until they come round)
  last = np.full(n, -1, np.int64)
  for t in range(T):
    last = np.where(entered[t], r[t], last)
  np.testing.assert_array_equal(u.backward_row.cpu().numpy(), last.astype(np.int32))
  assert (last == -1).sum() == (~entered.any(0)).sum()
  # goal_t is that row while the env is in the reset phase
  now = (after[-1] == 1) & entered.any(0)
  assert now.sum() > 0
  assert_bits({'goal_t': u.goal_t.cpu().numpy()[now]}, {'goal_t': table[last[now]]}, ('goal_t',))
  if n == 4160:
    assert set(np.unique(r[entered]).tolist()) == set(range(len(table))), 'not every row of the table was drawn'
  assert len(np.unique(r[entered])) > 1


# ---------------------------------------------------------------------------------------------------------------- 3. the launch == the step-by-step procedure
@pytest.mark.parametrize('kind,n', SHAPES)
@pytest.mark.parametrize('head', [None, 'sample'])
def test_table_launch_equals_the_step_by_step_procedure(kind, n, head):
  """tests/test_sawyer_pair_gpu.py's procedure with the drawn row: T launches of rollout(actions[t:t+1]); after step t the test hands over by the rule and writes goal_t
  and last_obs[:, 7:] of the envs that changed goal -- the backward table's row of the 0xFFFD draw, or the goal table's row of the 0xFFFE draw, both recomputed here"""
  import torch
  env = make_env(kind, n, seed=8)
  u = env.unwrapped
  given, table = table_of(kind, u)
  pair, _ = make_pair(head=head, seed=3, sos=True, goal=given)
  env.rollout(torch.zeros(2, n, 4, device='cuda'))                       # (step counter not 0)
  sd = u.state_dict()
  ph, sip = stagger(u)
  step0 = u.total_step_count
  got = host(env.rollout_agents(pair, T))
  share(got, f'{kind} n={n} head={head}')
  end, end_phase, end_sip, end_row = state_of(u), u.agent_phase.cpu().numpy(), u.steps_in_phase.cpu().numpy(), u.backward_row.cpu().numpy()
  fs_got, bs_got = (c.cpu().numpy() for c in u.pair_counts)
  u.load_state_dict(sd)
  actions = torch.as_tensor(got['actions'], device='cuda')
  ph, sip = ph.astype(np.int64), sip.astype(np.int64)
  fs, bs, last = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
  for t in range(T):
    np.testing.assert_array_equal(got['agent'][t], ph)
    r = host(env.rollout(actions[t:t + 1]))
    s = r['success'][0].astype(bool)
    sip += 1
    over = s | (sip >= np.array(SE)[ph])
    fs += over & s & (ph == 0)
    bs += over & s & (ph == 1)
    ph = np.where(over, ph ^ 1, ph)
    sip = np.where(over, 0, sip)
    fwd, _ = goal_draw(u, step0 + t)
    idx = back_draw(u, step0 + t, len(table))
    new = np.where((ph == 1)[:, None], table[idx], fwd)
    drew = over & (ph == 1)
    last = np.where(drew, idx, last).astype(np.int32)
    np.testing.assert_array_equal(got['backward_row'][t], np.where(drew, idx, -1).astype(np.int32))
    m = torch.as_tensor(over, device='cuda')
    rows = torch.as_tensor(new, device='cuda')
    u.goal_t[m] = rows[m]
    u.last_obs[m, 7:] = rows[m]
    u._last_obs_stale = False
    r['obs'][0][over, 7:] = new[over]
    for k in OUT_KEYS:
      if k in got:
        assert_bits({k: got[k][t]}, {k: r[k][0]}, (k,))
  same_state(end, state_of(u))
  np.testing.assert_array_equal(end_phase, ph)
  np.testing.assert_array_equal(end_sip, sip)
  np.testing.assert_array_equal(end_row, last)
  np.testing.assert_array_equal(fs_got, fs)
  np.testing.assert_array_equal(bs_got, bs)


# ---------------------------------------------------------------------------------------------------------------- 4. launches of one; shards
@pytest.mark.parametrize('kind', ['door', 'peg'])
@pytest.mark.parametrize('head', [None, 'sample'])
def test_one_table_launch_of_T_equals_T_launches_of_one(kind, head):
  import torch
  n = 40
  ea, eb = make_env(kind, n, seed=9), make_env(kind, n, seed=9)
  given, _ = table_of(kind, ea.unwrapped)
  pair, _ = make_pair(head=head, seed=2, sos=True, goal=given)
  kw = {'return_noise': True} if head else {}
  stagger(ea.unwrapped)
  stagger(eb.unwrapped)
  one = ea.rollout_agents(pair, T, **kw)
  share(one, f'{kind} head={head}')
  rows, fs, bs = [], 0, 0
  for _ in range(T):
    rows.append({k: v.clone() for k, v in eb.rollout_agents(pair, 1, **kw).items()})
    fs, bs = fs + eb.unwrapped.pair_counts[0], bs + eb.unwrapped.pair_counts[1]
  assert 'backward_row' in one and int((one['backward_row'] >= 0).sum()) > n
  for k in one:
    same(one[k], torch.cat([r[k] for r in rows]), k)
  ua, ub = ea.unwrapped, eb.unwrapped
  same_state(state_of(ua), state_of(ub))
  for k in ('agent_phase', 'steps_in_phase', 'backward_row'):
    same(getattr(ua, k), getattr(ub, k), k)
  same(ua.pair_counts[0], fs, 'forward_success')
  same(ua.pair_counts[1], bs, 'backward_success')


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_two_ragged_table_shards_equal_the_batch(kind):
  """env_offset 3 and a cut at 26: no shard starts or ends at a multiple of 4 or 16 -- the draw depends on seed, global id and step only"""
  import torch
  n, off, cut = 64, 3, 26
  whole = make_env(kind, n, seed=4, env_offset=off)
  parts = [make_env(kind, cut, seed=4, env_offset=off), make_env(kind, n - cut, seed=4, env_offset=off + cut)]
  sd = whole.unwrapped.state_dict()
  for p, (a, b) in zip(parts, ((0, cut), (cut, n))):
    p.unwrapped.load_state_dict(rows_of(sd, a, b))
  given, _ = table_of(kind, whole.unwrapped)
  pair, _ = make_pair(head='sample', seed=6, sos=True, goal=given)
  stagger(whole.unwrapped, off)
  out = whole.rollout_agents(pair, T, return_noise=True)
  share(out, kind)
  outs = []
  for p, o in zip(parts, (off, off + cut)):
    stagger(p.unwrapped, o)
    outs.append(p.rollout_agents(pair, T, return_noise=True))
  assert int((out['backward_row'] >= 0).sum()) > n and len(torch.unique(out['backward_row'])) > 2
  for k in out:
    same(out[k], torch.cat([o[k] for o in outs], 1), k)
  for k in STATE[kind] + ('agent_phase', 'steps_in_phase', 'backward_row'):
    same(getattr(whole.unwrapped, k), torch.cat([getattr(p.unwrapped, k) for p in parts]), k)
  for c in range(2):
    same(whole.unwrapped.pair_counts[c], torch.cat([p.unwrapped.pair_counts[c] for p in parts]), 'counts')


# ---------------------------------------------------------------------------------------------------------------- 5. a population of pairs == its pieces
def pair_population(P, G, given, head=None, seed=0, pad=8):
  """P pairs of different weights; the rows widened by `pad` floats of NaN past the parameter count, so a read past a member's row shows"""
  import torch
  from earl_benchmark_amd.policy import PairPopulation
  pairs = [make_pair(head=head, seed=seed + 2 * p, sos=True, goal=given)[0] for p in range(P)]
  pop = PairPopulation(pairs, envs_per_policy=G, device='cuda')
  wide = torch.full((P, 2, pop.pair_stride + pad), float('nan'), dtype=torch.float32)
  wide[:, :, :pop.n_params] = pop.params[:, :, :pop.n_params].cpu()
  pop.params = wide
  pop.to('cuda')
  assert pop.pair_stride % 4 == 0 and pop.stride == 2 * pop.pair_stride and bool(pop.params[:, :, pop.n_params:].isnan().all())
  return pop


POP_SETTINGS = [('door', 64, 0), ('door', 64, 8), ('peg', 64, 0), ('door', 4160, 0)]


@pytest.mark.parametrize('kind,n,off', POP_SETTINGS, ids=[f'{s[0]}-{s[1]}-off{s[2]}' for s in POP_SETTINGS])
@pytest.mark.parametrize('tabled', [False, True], ids=['row', 'table'])
def test_pair_population_equals_its_pieces(kind, n, off, tabled):
  """G = 16: four members at 64 envs (five at env_offset 8, the first and the last partial: a shard whose env_offset is no multiple of G), 260 at 4160 (the eight-wave
  build against one-wave pieces).  The pieces are launches of ONE pair -- member g // G's -- on an env of the piece's rows, offset and length."""
  import torch
  G = 16
  big = make_env(kind, n, env_offset=off)
  u = big.unwrapped
  given, _ = table_of(kind, u) if tabled else (reset_row(u), None)
  P = (off + n - 1) // G + 1
  pop = pair_population(P, G, given, head='sample', seed=n + off)
  sd = u.state_dict()
  stagger(u, off)
  got = {k: v.clone() for k, v in big.rollout_agents(pop, T, return_noise=True).items()}
  share(got, f'{kind} n={n} off={off} tabled={tabled}')
  assert ('backward_row' in got) == tabled and not bool(got['actions'].isnan().any())
  cuts = [off] + [g for g in range((off // G + 1) * G, off + n, G)] + [off + n]
  assert len(cuts) - 1 == P == (260 if n == 4160 else 4 + (off > 0))
  pieces = {}                                                              # one env per piece length, moved from piece to piece
  want, ends, extra = [], [], []
  for a, b in zip(cuts[:-1], cuts[1:]):
    if b - a not in pieces:
      pieces[b - a] = make(kind, b - a, seed=5, **(dict(reset_at_goal=True) if kind == 'peg' else {}))
    pu = pieces[b - a].unwrapped
    pu.load_state_dict(rows_of(sd, a - off, b - off))
    pu._cfg.env_offset = a
    pu.backward_row = None
    stagger(pu, a)
    want.append({k: v.clone() for k, v in pu.rollout_agents(pop.pair(a // G), T, return_noise=True).items()})
    ends.append(state_of(pu))
    extra.append([pu.agent_phase.clone(), pu.steps_in_phase.clone(), pu.pair_counts[0].clone(), pu.pair_counts[1].clone()] + ([pu.backward_row.clone()] if tabled else []))
  for k in got:
    same(got[k], torch.cat([w[k] for w in want], 1), k)
  for k, v in state_of(u).items():
    same(v, torch.cat([e[k] for e in ends]), k)
  mine = [u.agent_phase, u.steps_in_phase, u.pair_counts[0], u.pair_counts[1]] + ([u.backward_row] if tabled else [])
  for j, v in enumerate(mine):
    same(v, torch.cat([e[j] for e in extra]), f'per-env word {j}')
  # (members with different weights: equal pieces could not come from every env reading member 0)
  assert not torch.equal(pop.params[0, :, :pop.n_params], pop.params[P - 1, :, :pop.n_params])
  if tabled:
    assert int((got['backward_row'] >= 0).sum()) > n


# ---------------------------------------------------------------------------------------------------------------- 6. evaluate_agents
EVAL_SETTINGS = [('door', 64, 'pair'), ('peg', 4160, 'pair'), ('door', 4160, 'population')]


@pytest.mark.parametrize('kind,n,form', EVAL_SETTINGS, ids=[f'{s[0]}-{s[1]}-{s[2]}' for s in EVAL_SETTINGS])
def test_evaluate_agents_is_the_definitions_applied_to_rollout_agents(kind, n, form):
  import torch
  env = make_env(kind, n)
  u = env.unwrapped
  given, _ = table_of(kind, u)
  if form == 'population':
    pair = pair_population(n // 16, 16, given, head='sample', seed=n)
  else:
    pair, _ = make_pair(head='sample', seed=n, sos=True, goal=given)
  env.rollout_agents(pair, 2)
  sd = u.state_dict()
  ph0, sip0 = stagger(u)
  full = {k: v.clone() for k, v in env.rollout_agents(pair, T).items()}
  share(full, f'{kind} n={n} {form}')
  end = state_of(u)
  words = {k: getattr(u, k).clone() for k in ('agent_phase', 'steps_in_phase', 'backward_row', '_last_success')}
  fs, bs = (c.clone() for c in u.pair_counts)
  guard = (u.fail_count - sd['fail_count']).clone()
  total = u.total_step_count
  u.load_state_dict(sd)
  stagger(u)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  s = env.evaluate_agents(pair, T)
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - base
  assert set(s) == {'ret', 'success', 'first_success', 'guard_steps', 'forward_success', 'backward_success'}
  ret, last, first = by_definition(full['reward'], full['success'])
  same_np(s['ret'], ret, 'ret')
  same_np(s['success'], last, 'success')
  same_np(s['first_success'], first, 'first_success')
  same(s['guard_steps'], guard, 'guard_steps')
  same(s['forward_success'], fs, 'forward_success')
  same(s['backward_success'], bs, 'backward_success')
  same_state(end, state_of(u))
  for k, v in words.items():
    same(getattr(u, k), v, k)
  assert u.total_step_count == total and not u._last_obs_stale
  # the six [N] results and the copy of fail_count are 29 bytes per env, each tensor rounded up to the allocator's 512-byte block: 64 bytes per env and ten blocks
  # bound them, and lie below the smallest float [T, N] array (4 T = 92 bytes per env), let alone the observations (112 T)
  print(f'{kind} n={n} {form}: peak {peak} bytes above the resident state, {peak / n:.1f} per env')
  assert peak <= 64 * n + 10 * 512


# ---------------------------------------------------------------------------------------------------------------- 7. NULL pointers; the Python surface
@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_every_optional_pointer_null_in_turn_leaves_the_rest(kind):
  import torch
  n = 64
  env = make_env(kind, n, seed=10)
  u = env.unwrapped
  given, table = table_of(kind, u)
  table = torch.as_tensor(table, device='cuda').contiguous()
  pop = pair_population(4, 16, given, head='sample', seed=5)
  sd = u.state_dict()

  def launch(null=()):
    u.load_state_dict(sd)
    stagger(u)
    return raw(u, pop, 'agents', head=True, table=table, pop=pop.pop_struct, summary=True, null=null)
  full = launch()
  share({'status': full['status']}, kind)
  ret, last, first = by_definition(full['reward'], full['success'])
  same_np(full['ret'], ret, 'ret')
  same_np(full['last'], last, 'success_last')
  same_np(full['first'], first, 'first_success')
  assert 0 <= int(full['fs'].min()) and int(full['fs'].max()) <= T and 0 <= int(full['bs'].min()) and int(full['bs'].max()) <= T      # (the rubbish is gone)
  assert int((full['row_out'] >= 0).sum()) > n and int(full['row_out'].max()) < len(table) and int(full['row_out'].min()) == -1
  optional = ['actions', 'eps', 'obs', 'reward', 'done', 'success', 'status', 'agent', 'fs', 'bs', 'row', 'row_out', 'ret', 'last', 'first'] + (['info'] if kind == 'peg' else [])
  for k in optional:
    same_dicts(full, launch(null=(k,)), f'without {k}', skip=(k,))
  same_dicts(full, launch(null=tuple(optional)), 'without any', skip=tuple(optional))


@pytest.mark.parametrize('kind', ['door', 'peg'])
def test_python_surface(kind):
  import torch
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import AgentPair, PairPopulation
  from earl_benchmark_amd.wrappers import LifelongWrapper
  n = 64
  env = make_env(kind, n, seed=2)
  u = env.unwrapped
  given, table = table_of(kind, u)
  pair, _ = make_pair(seed=1, sos=True, goal=given)
  fixed, _ = make_pair(seed=1, sos=True, goal=reset_row(u))
  assert u.backward_row is None and 'backward_row' not in u.state_dict()
  out = env.rollout_agents(fixed, T)
  assert 'backward_row' not in out and u.backward_row is None             # (ONE row: as ever)
  out = env.rollout_agents(pair, T)
  share(out, kind)
  assert tuple(out['backward_row'].shape) == (T, n) and out['backward_row'].dtype == torch.int32
  assert tuple(u.backward_row.shape) == (n,) and u.backward_row.dtype == torch.int32 and bool((u.backward_row >= 0).any()) and int(u.backward_row.max()) < len(table)
  assert ('info' in out) == (kind == 'peg') and u.total_step_count == 2 * T
  # the state dict carries the row once it exists; a restored env repeats the launch
  sd = u.state_dict()
  same(sd['backward_row'], u.backward_row, 'backward_row')
  nxt = {k: v.clone() for k, v in env.rollout_agents(pair, 4).items()}
  row = u.backward_row.clone()
  u.load_state_dict(sd)
  same(u.backward_row, sd['backward_row'], 'restored')
  again = env.rollout_agents(pair, 4)
  for k in nxt:
    same(again[k], nxt[k], k)
  same(u.backward_row, row, 'after the repeated launch')
  # reset(mask) puts the masked envs' row back to -1
  u.backward_row.fill_(3)
  mask = torch.arange(n, device='cuda') % 3 == 0
  env.reset(mask)
  assert bool((u.backward_row[mask] == -1).all()) and bool((u.backward_row[~mask] == 3).all())
  env.reset()
  assert bool((u.backward_row == -1).all())
  # a population through rollout_agents and evaluate_agents; the member range
  pop = PairPopulation([make_pair(seed=p, sos=True, goal=given)[0] for p in range(4)], envs_per_policy=16, device='cuda')
  got = env.rollout_agents(pop, 3)
  assert tuple(got['agent'].shape) == (3, n) and 'backward_row' in got
  s = env.evaluate_agents(pop, 3)
  assert all(tuple(v.shape) == (n,) for v in s.values()) and s['ret'].dtype == torch.float64 and s['success'].dtype == torch.bool
  same(s['forward_success'], u.pair_counts[0], 'pair_counts')
  with pytest.raises(ValueError, match='need members up to 3 of 2'):
    env.rollout_agents(PairPopulation([pair, pair], envs_per_policy=16, device='cuda'), 2)
  # 'initial' keeps its rules; the refusals
  pf, pb = pair.agent(0), pair.agent(1)
  if kind == 'peg':
    with pytest.raises(ValueError, match=r'env\.initial_states'):
      env.rollout_agents(AgentPair(pf, pb, switch_every=SE, obs_dim=14, act_dim=4), T)
  else:
    states = env.rollout_agents(AgentPair(pf, pb, switch_every=SE, backward_goal='initial_states', obs_dim=14, act_dim=4), T)
    assert 'backward_row' not in states                                   # (the door's single row behaves as 'initial')
  with pytest.raises(ValueError, match='agent pair IS the lifelong mechanism'):
    LifelongWrapper(make_env(kind, 4), 5).unwrapped.evaluate_agents(pair, 2)
  with pytest.raises(ValueError, match='AgentPair goes to rollout_agents'):
    env.rollout_policy(pop, 2)
  with pytest.raises(ValueError, match='sample=False needs Gaussian agents'):
    env.evaluate_agents(pair, 2, sample=False)
  with pytest.raises(ValueError, match='T = 0 < 1'):
    env.evaluate_agents(pair, 0)
  # the tabletop refuses both by name, on the device too
  _, tt = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=4, device='cuda', seed=3).get_envs()
  with pytest.raises(ValueError, match='a table of backward goals runs on the Sawyer door and peg only'):
    tt.rollout_agents(pair, 5)
  with pytest.raises(ValueError, match='a PairPopulation runs on the Sawyer door and peg only'):
    tt.rollout_agents(pop, 5)

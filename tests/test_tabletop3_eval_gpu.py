"""earl_tabletop3_eval_episodes on the device: the fused role-split launch (csrc/tabletop3_rollout_ws.h) against the host twin and against the device's own
sequence of earl_tabletop3_reset + earl_tabletop3_rollout, bit for bit -- the four outputs and every state array; the dense reward bit for bit against the
device's sequence (the storers call the same reward_success<3>) and within the header's 1e-6 against the twin (the host's exp is another libm's).  Every buffer
sits between guard bands of 0x00 and of 0xFF and every output starts as a pattern that must be gone (tests/tabletop_abi.py).  Inputs: the two sets of
tests/tabletop3_eval_helpers.py, whose coverage tests/test_tabletop3_eval.py asserts."""
import numpy as np
import pytest
import torch

import tabletop3_eval_helpers as h
import tabletop_abi as ta
from test_tabletop_gpu import DENSE_ATOL, DENSE_RTOL

pytestmark = pytest.mark.gpu
K = h.K
DENSE = (DENSE_RTOL, DENSE_ATOL)


@pytest.fixture(scope='module')
def dev():
  return ta.Side('cuda')


@pytest.fixture(scope='module')
def host():
  return ta.Side('cpu')


def held_to_both(dev, host, sc, act, episodes, what, null=(), **over):
  """the device's call (both fills) == the device's sequence == the twin -> the device's results"""
  got = ta.both_fills(h.run_eval3, dev, sc, act, what=what, episodes=episodes, null=null, **over)
  seq, b = h.run_sequence3(dev, sc, act, 0x00, episodes=episodes, null=null, **over)
  b.check(what + ' sequence')
  ta.agree(got, seq, what + ': device vs its own sequence', null=null)
  twin, _ = h.run_eval3(host, sc, act, 0x00, episodes=episodes, null=null, **over)
  dense = DENSE if sc.kw['reward_type'] == 'dense' else None
  ta.agree(got, twin, what + ': device vs twin', null=null, dense=dense)
  return got


@pytest.mark.parametrize('E', [1, 2, 5])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_small_shapes(dev, host, n, E):
  """sparse / dense x own / shared actions, T = 3 K (own) and 2 K (shared).  At most four workgroups per episode: on a chip of 8 CUs or more every episode
  of these cases is a group of its own (E groups of one episode); groups of several episodes are test_groups_of_several_episodes' cases"""
  for rt in ('sparse', 'dense'):
    for shared in (False, True):
      at_goal = (rt == 'dense') != shared
      T = 2 * K if shared else 3 * K
      sc = h.scene(n, T, rt, at_goal, env_offset=3 if n == 65 else 0)
      act, episodes = h.inputs('b' if at_goal else 'a', n, T, E, shared)
      got = held_to_both(dev, host, sc, act, episodes, f'n={n} E={E} {rt} shared={shared}')
      assert int(got['st.steps_since_reset'].min()) == T


def test_launch_forms_agree(dev):
  n, E, T = 200, 5, 2 * K
  for rt, which in (('sparse', 'a'), ('dense', 'b')):
    sc = h.scene(n, T, rt, which == 'b')
    act, _ = h.inputs(which, n, T, E)
    res = {}
    for form in (0, 1, 2):
      with h.form3(form):
        res[form] = ta.both_fills(h.run_eval3, dev, sc, act, what=f'form {form}')
    ta.agree(res[0], res[1], f'{rt}: automatic vs the sequence of existing kernels')
    ta.agree(res[2], res[1], f'{rt}: no episodes in flight vs the sequence of existing kernels')


@pytest.mark.parametrize('trigger', ['T=2K+4', 'obs NULL', 'auto_reset'])
def test_fallback_triggers(dev, host, trigger):
  n, E = 200, 3
  T = 2 * K + 4 if trigger == 'T=2K+4' else 2 * K
  null = ('obs',) if trigger == 'obs NULL' else ()
  over = dict(auto_reset=1) if trigger == 'auto_reset' else {}
  for rt, which in (('sparse', 'a'), ('dense', 'b')):
    sc = h.scene(n, T, rt, which == 'b')
    act, _ = h.inputs(which, n, T, E)
    held_to_both(dev, host, sc, act, None, f'{trigger} {rt}', null=null, **over)


def part(sc, lo, hi):
  """rows [lo, hi) of a scene as a shard of their own: (scene, the cfg fields that change)"""
  sub = ta.Scene.__new__(ta.Scene)
  sub.__dict__.update(sc.__dict__)
  sub.n = hi - lo
  sub.state = {k: v[lo:hi].copy() for k, v in sc.state.items()}
  return sub, dict(n=hi - lo, env_offset=int(sc._cfg.env_offset) + lo)


def test_shards_equal_the_batch(dev):
  n, E, T = 200, 5, 2 * K
  sc = h.scene(n, T, 'sparse', True, env_offset=3)
  act, _ = h.inputs('b', n, T, E)
  whole = ta.both_fills(h.run_eval3, dev, sc, act, what='batch')
  for lo, hi in ((0, 70), (70, 200)):
    sub, over = part(sc, lo, hi)
    got = ta.both_fills(h.run_eval3, dev, sub, np.ascontiguousarray(act[:, :, lo:hi]), what=f'shard [{lo}, {hi})', **over)
    for k, v in got.items():                                                # outputs are [E, T, n, ..], state arrays [n, ..]
      ta.same(v, whole[k][:, :, lo:hi] if k.startswith('out.') else whole[k][lo:hi], f'shard [{lo}, {hi}) {k}')


def test_two_launches_equal_one(dev):
  n, T = 200, 3 * K
  sc = h.scene(n, T, 'dense', False)
  act, _ = h.inputs('a', n, T, 5)
  one = ta.both_fills(h.run_eval3, dev, sc, act, what='E=5')
  first = ta.both_fills(h.run_eval3, dev, sc, np.ascontiguousarray(act[:2]), what='E=2')
  nxt = ta.Scene.__new__(ta.Scene)
  nxt.__dict__.update(sc.__dict__)
  nxt.state = {k: first['st.' + k].cpu().numpy() for k in sc.state}
  nxt.counter = sc.counter + 2 * (T + 1)
  second = ta.both_fills(h.run_eval3, dev, nxt, np.ascontiguousarray(act[2:]), what='E=3')
  for k in ta.OUT4:
    ta.same(torch.cat([first['out.' + k], second['out.' + k]]), one['out.' + k], f'E=2 then E=3 vs E=5: {k}')
  for k in sc.state:
    ta.same(second['st.' + k], one['st.' + k], f'E=2 then E=3 vs E=5: state {k}')


def geometry(n, E, c):
  """(ep_groups, ep_per_group) of the fused launch: the rule of csrc/tabletop3_eval.hip (= csrc/tabletop.hip: do_rollout), restated"""
  grid = (n + 63) // 64
  if E > 1 and grid * 2 <= c:
    P = min(c // grid, E)
    per = -(-E // P)
    return -(-E // per), per
  return 1, E


@pytest.mark.parametrize('case', ['32C x 5', '16C x 9', '4C-24 x 37', '16C x 28'])
def test_groups_of_several_episodes(dev, host, case):
  """several episode groups that each walk MORE than one episode (ep0 = grp * ep_per_group, the group's own rows, action rows and counters from its second
  episode on), with a shorter last group where E does not divide: 2 slots x 5 episodes = groups of 3 and 2; 4 slots x 9 = 3, 3, 3; 16 slots x 37 = twelve
  groups of 3 and one of 1, ragged last workgroup; 4 slots x 28 = the measured 4 x 7.  Own actions; against form 1, the device's sequence and the twin."""
  c = ta.cus()
  n, E, rt, which = {'32C x 5': (32 * c, 5, 'sparse', 'a'), '16C x 9': (16 * c, 9, 'dense', 'b'), '4C-24 x 37': (4 * c - 24, 37, 'sparse', 'b'),
                     '16C x 28': (16 * c, 28, 'dense', 'a')}[case]
  groups, per = geometry(n, E, c)
  want_geometry = {'32C x 5': (2, 3), '16C x 9': (3, 3), '4C-24 x 37': (13, 3), '16C x 28': (4, 7)}[case]
  assert (groups, per) == want_geometry and groups > 1 and per > 1, (groups, per)           # (any chip whose CU count is a multiple of 16)
  T = 2 * K
  sc = h.scene(n, T, rt, which == 'b', env_offset=3)
  act, _ = h.inputs(which, n, T, E)
  got = held_to_both(dev, host, sc, act, None, case)
  with h.form3(1):
    want, b = h.run_eval3(dev, sc, act, 0x00)
    b.check(case + ' form 1')
  ta.agree(got, want, case + ': fused vs the sequence of existing kernels')
  np.testing.assert_array_equal(got['st.num_interventions'].cpu().numpy(), sc.state['num_interventions'] + E)


@pytest.mark.parametrize('which', ['32C', '32C+64', '64C+65'])
def test_large_grids(dev, which):
  """the last grid that runs episodes in flight, the first that does not, and more workgroups than CUs with a ragged last one: against form 1"""
  c = ta.cus()
  n = {'32C': 32 * c, '32C+64': 32 * c + 64, '64C+65': 64 * c + 65}[which]
  E, T = 2, 2 * K
  sc = h.scene(n, T, 'sparse', False)
  act, _ = h.inputs('a', n, T, E)
  got = ta.both_fills(h.run_eval3, dev, sc, act, what=f'n={n}')
  with h.form3(1):
    want, b = h.run_eval3(dev, sc, act, 0x00)
    b.check(f'n={n} form 1')
  ta.agree(got, want, f'n={n}: fused vs the sequence of existing kernels')


def test_empty_work(dev):
  sc = h.scene(5, 2 * K)
  act, _ = h.inputs('a', 5, 2 * K, 2)
  for fill in ta.FILLS:
    for what, kw in (('n=0', dict(n_call=0)), ('episodes=0', dict(E_call=0))):
      res, b = h.run_eval3(dev, sc, act, fill, **kw)
      b.check(what)
      ta.assert_untouched(res, sc, what)
    res, b = h.run_eval3(dev, sc, act, fill, T_call=0)                      # T = 0: the resets only, as the sequence would
    b.check('T=0')
    ta.assert_untouched({k: v for k, v in res.items() if k.startswith('out.')}, sc, 'T=0')
    o = sc.oracle()
    o.reset()
    o.reset()
    ta.agree({k: v for k, v in res.items() if k.startswith('st.')}, ta._pack(o), 'T=0: the state after two resets')


def test_rollout_episodes_on_the_device_equals_the_host():
  from test_tabletop3_eval import python_path
  got, want = python_path('cuda'), python_path('cpu')
  for k in range(4):
    ta.same(got[k].cpu(), want[k], f'rollout_episodes cuda vs cpu: output {k}')

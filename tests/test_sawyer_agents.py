"""earl_sawyer_agents_rollout (include/earl_physics.h): the Sawyer agent pair in its general form -- a table of backward goals, a population of pairs, episode
summaries.  What can be held without a GPU:
  1. the entry point is declared, bound in _abi.SIGNATURES and exported; earl_sawyer_pair_rollout keeps its 14 arguments; earl_backward_goals is what gcc sees;
  2. every new argument error comes back before any HIP call (the malformed structs as a table, like tests/test_policy_contract.py), and the well-formed
     combinations are accepted with n = 0;
  3. AgentPair tables and 'initial_states', PairPopulation: packing, indexing, the refusals by member and field, the member range against the env's global ids, the
     tabletop's refusals by name;
  4. the table's fields live in SawyerPolicyArgs only and are read through the kernel-argument segment; the new rules stand in csrc/policy_check.h.
tests/test_sawyer_agents_gpu.py holds the launches."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from earl_benchmark_amd import _abi
from policy_struct_helpers import aligned_params, head as head_of, variant as variant_of
from test_sawyer_policy_rollout import pack, random_layers

CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')
NAME = 'earl_sawyer_agents_rollout'


# ---------------------------------------------------------------------------------------------------------------- 1. declared, bound, exported; the struct
def declared(name):
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'int\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
  assert m, f'{name} is not declared'
  return [a.strip() for a in m.group(1).split(',')]


def test_entry_point_is_declared_bound_and_exported():
  args = declared(NAME)
  assert len(args) == len(_abi.SIGNATURES[NAME]) == 17
  assert [a.split()[-1].lstrip('*') for a in args] == ['model', 'col', 'nv', 'cfg', 'st', 'policy', 'pair', 'pop', 'goals', 'head', 'obs0', 'T', 'clock', 'actions', 'out',
                                                      'summary', 'stream']
  for arg, text in ((6, 'const earl_agent_pair* pair'), (7, 'const earl_policy_population* pop'), (8, 'const earl_backward_goals* goals'),
                    (15, 'const earl_episode_summary* summary')):
    assert args[arg] == text
  sig = _abi.SIGNATURES[NAME]
  assert sig[6]._type_ is _abi.AgentPair and sig[7]._type_ is _abi.PolicyPopulation and sig[8]._type_ is _abi.BackwardGoals and sig[15]._type_ is _abi.EpisodeSummary
  assert hasattr(_abi.load(), NAME) and not hasattr(C.CDLL(_abi.HOST_LIB_PATH), NAME)


def test_the_pair_entry_point_keeps_its_fourteen_arguments():
  assert len(declared('earl_sawyer_pair_rollout')) == len(_abi.SIGNATURES['earl_sawyer_pair_rollout']) == 14
  assert C.sizeof(_abi.AgentPair) == 72


def test_backward_goals_matches_what_gcc_sees(tmp_path):
  cname, cls = 'earl_backward_goals', _abi.BackwardGoals
  src = '#include <stdio.h>\n#include <stddef.h>\n#include "earl_physics.h"\nint main(void) {\n'
  src += f'printf("%zu ", sizeof({cname}));\n' + ''.join(f'printf("%zu ", offsetof({cname}, {f[0]}));\n' for f in cls._fields_)
  want = [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
  c, exe = tmp_path / 'probe.c', tmp_path / 'probe'
  c.write_text(src + 'return 0; }\n')
  subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(REPO, 'include'), '-o', str(exe), str(c)], check=True)
  assert [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == want
  assert want == [32, 0, 8, 12, 16, 24] and [f[0] for f in cls._fields_] == ['table', 'n_rows', 'pad_', 'row', 'row_out']


def test_the_header_names_the_draw_indices():
  txt = open(os.path.join(REPO, 'include', 'earl_physics.h')).read()
  at = txt.index('typedef struct earl_backward_goals')
  doc = txt[txt.rindex('/* ----', 0, at):at]
  for word in ('0xFFFD', '0xFFFE', '0xFFF0 .. 0xFFF2', '0xFFFF', '0x504F4C00', '0 .. 31'):
    assert word in doc, word


# ---------------------------------------------------------------------------------------------------------------- 2. argument errors
def test_new_argument_errors_need_no_gpu():
  """every refusal comes back before any HIP call (the pointers are host stand-ins that are never read: n = 0 where the call is accepted), malformed structs as a table"""
  lib = _abi.load()
  pol, keep = pack(random_layers([14, 16, 4], seed=0), 'relu', 'tanh')
  count = keep.size
  assert count == 308
  aligned = aligned_params(pol, keep, rows=8)
  buf = np.zeros(4096, np.float64)
  p = buf.ctypes.data
  st = _abi.SawyerState(qpos=p, qvel=p, mocap_pos=p, goal=p, last_obs=p, steps_since_goal_change=p)
  out, out_none = _abi.SawyerOut(obs=p), _abi.SawyerOut()

  def cfg(n=0, rows=1, gcf=0, off=0):
    return _abi.SawyerCfg(n=n, env_offset=off, frame_skip=5, n_goal_rows=rows, goal_table=p if rows else None, goal_change_frequency=gcf)

  def pair(se=(5, 3), sos=1, stride=count, goal=None, phase=p):
    return _abi.AgentPair(switch_every=(C.c_int32 * 2)(*se), switch_on_success=sos, pad_=0, param_stride=stride, backward_goal=goal, phase=phase, steps_in_phase=p,
                          agent_out=p, forward_success=p, backward_success=p)

  def pop(P=4, G=16, stride=2 * count):
    return _abi.PolicyPopulation(n_policies=P, envs_per_policy=G, param_stride=stride)

  def goals(table=p, rows=5, row=p, row_out=p):
    return _abi.BackwardGoals(table=table, n_rows=rows, pad_=0, row=row, row_out=row_out)

  summary = _abi.EpisodeSummary(ret=p, success_last=p, first_success=p)

  def call(cfg=cfg(), st=st, pol=pol, pair=pair(), pop=None, goals=None, head=None, T=4, actions=p, out=out, summary=None, nv=10):
    ref = lambda s: None if s is None else C.byref(s)
    return lib.earl_sawyer_agents_rollout(p, None, nv, ref(cfg), ref(st), ref(pol), ref(pair), ref(pop), ref(goals), ref(head), p, T, None, actions, ref(out),
                                          ref(summary), None)

  good = [dict(), dict(nv=15), dict(pop=pop()), dict(goals=goals()), dict(summary=summary), dict(pop=pop(), goals=goals(), summary=summary),
          dict(goals=goals(rows=1)), dict(goals=goals(row=None, row_out=None)), dict(goals=goals(), cfg=cfg(rows=15)),
          dict(pop=pop(stride=2 * count + 4)), dict(pop=pop(G=32)), dict(pop=pop(), pair=pair(stride=count)),
          dict(pop=pop(), goals=goals(), summary=summary, actions=None, out=out_none),                      # every [T] pointer NULL
          dict(pair=pair(goal=p)),                                                                           # the ONE fixed row, as ever
          dict(pol=variant_of(pol, dims=(14, 16, 8, 0)), head=head_of(), pair=pair(stride=376), pop=pop(stride=752), goals=goals())]
  for kw in good:
    assert call(**kw) == _abi.EARL_OK, kw
  bad = [
      # goals
      dict(goals=goals(table=None)), dict(goals=goals(rows=0)), dict(goals=goals(rows=-3)),                  # NULL table, n_rows < 1
      dict(goals=goals(), pair=pair(goal=p)),                                                                # a table AND the fixed row
      dict(goals=goals(), cfg=cfg(rows=0)), dict(goals=goals(rows=1), cfg=cfg(rows=0)),                      # the forward goal could not be restored
      # pop: check_population's rules and the stride rule
      dict(pop=pop(P=0)), dict(pop=pop(G=0)), dict(pop=pop(G=8)), dict(pop=pop(G=24)),
      dict(pop=pop(stride=2 * count - 4)), dict(pop=pop(stride=count)), dict(pop=pop(stride=0)),             # < 2 x pair stride (count: one policy fits, a pair does not)
      dict(pop=pop(stride=2 * count + 1)), dict(pop=pop(stride=2 * count + 2)),                              # a multiple of 4
      dict(pop=pop(stride=2 * count + 4), pair=pair(stride=count + 4)),                                      # 2 x (count + 4) > 2 count + 4
      dict(pop=pop(P=4), cfg=cfg(n=1, off=64)), dict(pop=pop(P=4), cfg=cfg(n=65, off=0)), dict(pop=pop(), cfg=cfg(n=4, off=-1)),      # the member range, env_offset < 0
      # everything earl_sawyer_pair_rollout refuses
      dict(pair=None), dict(pair=pair(phase=None)), dict(pair=pair(se=(0, 3))), dict(pair=pair(sos=2)), dict(pair=pair(stride=count - 4)), dict(pair=pair(stride=count + 2)),
      dict(cfg=cfg(gcf=5)), dict(cfg=cfg(rows=0), pair=pair(goal=p)), dict(out=out_none, st=_abi.SawyerState(qpos=p, qvel=p, mocap_pos=p, goal=p)),
      dict(out=None), dict(pol=None), dict(cfg=None), dict(st=None), dict(T=0), dict(nv=23), dict(pol=variant_of(pol, dims=(12, 16, 4, 0))), dict(head=head_of()),
      dict(pol=variant_of(pol, params=pol.params + 4)),
  ]
  for kw in bad:
    for extra in (dict(), dict(summary=summary)):
      assert call(**{**extra, **kw}) == -1, kw
  del aligned, buf


def test_the_new_rules_stand_next_to_check_pair():
  src = open(os.path.join(CSRC, 'policy_check.h')).read()
  at = src.index('inline int check_pair(')
  assert src.index('inline int check_pair_population(') > at and src.index('inline int check_backward_goals(') > at
  # the entry points apply them through the ONE closed-loop contract, which stands after them in the same header
  whole = src[src.index('inline int check_closed_loop('):]
  assert 'check_pair_population(' in whole and 'check_backward_goals(' in whole and src.index('inline int check_closed_loop(') > src.index('inline int check_backward_goals(')
  host = open(os.path.join(CSRC, 'physics.hip')).read()
  assert 'check_closed_loop(' in host and 'never both' not in host


# ---------------------------------------------------------------------------------------------------------------- 3. the Python surface
def agents(dims=(14, 16, 4), head=False, seed=0):
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  layers = [random_layers(list(dims), seed=seed + k, last_gain=1.5) for k in range(2)]
  if head:
    return [GaussianMLPPolicy(l, 'tanh', squash=True, log_std_map='clamp', obs_dim=14, act_dim=4) for l in layers]
  return [MLPPolicy(l, 'relu', 'tanh', obs_dim=14, act_dim=4) for l in layers]


def pair_of(seed=0, dims=(14, 16, 4), head=False, **kw):
  from earl_benchmark_amd.policy import AgentPair
  f, b = agents(dims, head, seed)
  kw.setdefault('backward_goal', None)
  return AgentPair(f, b, obs_dim=14, act_dim=4, **kw)


class Rows:
  def __init__(self, rows):
    self.initial_states = rows


def test_agent_pair_tables_and_initial_states():
  from earl_benchmark_amd.envs import sawyer_door, sawyer_peg
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy
  table = np.arange(35, dtype=np.float64).reshape(5, 7) / 8
  for given in (table, torch.as_tensor(table), table.tolist(), table.astype(np.float32)):
    pair = pair_of(backward_goal=given)
    assert pair.backward_goal is None and pair.backward_goals.dtype == torch.float64 and tuple(pair.backward_goals.shape) == (5, 7)
    np.testing.assert_array_equal(pair.backward_goals.numpy(), table)
    np.testing.assert_array_equal(pair.goal_table(None).numpy(), table)
    assert pair.goal_row(None) is None
  # everything else goes through today's rule with today's messages: ONE row as [7] or [1, 7]; a wrong width; the tabletop
  one = pair_of(backward_goal=table[:1])
  assert one.backward_goals is None and one.goal_table(None) is None
  np.testing.assert_array_equal(one.goal_row(None).numpy(), table[0])
  with pytest.raises(ValueError, match='ONE goal row of 7 values, got 6'):
    pair_of(backward_goal=np.zeros(6))
  with pytest.raises(ValueError, match='ONE goal row of 7 values, got 12'):
    pair_of(backward_goal=np.zeros((2, 6)))
  with pytest.raises(ValueError, match='ONE goal row of 7 values, got 42'):
    pair_of(backward_goal=np.zeros((2, 3, 7)))
  pi12 = MLPPolicy(random_layers([12, 16, 3], seed=0))
  with pytest.raises(ValueError, match='ONE goal row of 6 values, got 12'):
    AgentPair(pi12, pi12, backward_goal=np.zeros((2, 6)))
  with pytest.raises(ValueError, match='ONE goal row of 6 values, got 14'):
    AgentPair(pi12, pi12, backward_goal=np.zeros((2, 7)))
  with pytest.raises(ValueError):
    AgentPair(pi12, pi12, backward_goal='initial_states')               # (Sawyer widths only)
  assert pair_of().backward_goals is None and pair_of().goal_table(Rows(sawyer_peg.initial_states)) is None
  # 'initial_states': the peg's fifteen rows; the door's single row behaves as 'initial'
  init = pair_of(backward_goal='initial_states')
  assert init.backward_goal == 'initial_states' and init.backward_goals is None
  rows = init.goal_table(Rows(sawyer_peg.initial_states))
  assert tuple(rows.shape) == (15, 7) and rows.dtype == torch.float64
  np.testing.assert_array_equal(rows.numpy(), sawyer_peg.initial_states)
  assert init.goal_table(Rows(sawyer_peg.initial_states)) is rows        # one upload, not one per launch
  assert init.goal_table(Rows(sawyer_door.initial_states)) is None
  np.testing.assert_array_equal(init.goal_row(Rows(sawyer_door.initial_states)).numpy(), sawyer_door.initial_states[0])
  # 'initial' on the peg stays a ValueError naming env.initial_states
  with pytest.raises(ValueError, match=r'env\.initial_states has 15 rows'):
    pair_of(backward_goal='initial').goal_row(Rows(sawyer_peg.initial_states))
  assert pair_of(backward_goal='initial').goal_table(Rows(sawyer_peg.initial_states)) is None


@pytest.mark.parametrize('head', [False, True])
def test_pair_population_packs_and_indexes(head):
  from earl_benchmark_amd.policy import PairPopulation
  dims = (14, 32, 16, 8 if head else 4)
  table = np.arange(21, dtype=np.float64).reshape(3, 7)
  pairs = [pair_of(seed=10 * p, dims=dims, head=head, switch_every=(5, 3), switch_on_success=False, backward_goal=table) for p in range(5)]
  pop = PairPopulation(pairs, envs_per_policy=32)
  n_params = sum(n * (k + 1) for k, n in zip(dims[:-1], dims[1:]))
  assert (pop.n_policies, pop.envs_per_policy, pop.n_params, pop.gaussian, pop.switch_every, pop.switch_on_success) == (5, 32, n_params, head, (5, 3), False)
  assert tuple(pop.params.shape) == (5, 2, pop.pair_stride) and pop.params.dtype == torch.float32 and pop.params.is_contiguous()
  assert pop.pair_stride >= n_params and pop.pair_stride % 4 == 0 and pop.stride == 2 * pop.pair_stride
  assert (pop.pop_struct.n_policies, pop.pop_struct.envs_per_policy, pop.pop_struct.param_stride) == (5, 32, pop.stride)
  assert list(pop.struct.dims) == list(dims) and pop.struct.params == pop.params.data_ptr()
  np.testing.assert_array_equal(pop.goal_table(None).numpy(), table)
  for p, m in enumerate(pairs):
    np.testing.assert_array_equal(pop.params[p].numpy(), m.params.numpy())
    q = pop.pair(p)
    assert type(q.template) is type(m.template) and (q.switch_every, q.switch_on_success, q.dims) == (m.switch_every, m.switch_on_success, m.dims)
    np.testing.assert_array_equal(q.params.numpy(), m.params.numpy())
    np.testing.assert_array_equal(q.backward_goals.numpy(), table)
  # written in place: what the kernel reads is .params itself
  ptr = pop.params.data_ptr()
  pop.params.add_(1.0)
  assert pop.params.data_ptr() == ptr == pop.struct.params
  np.testing.assert_array_equal(pop.pair(2).params.numpy(), pairs[2].params.numpy() + 1.0)
  np.testing.assert_array_equal(pop.policy_index(torch.tensor([0, 31, 32, 159])).numpy(), [0, 0, 1, 4])
  if head:
    assert pop.head(sample=True).mode == _abi.HEAD_SAMPLE and pop.head(sample=False).log_std_map == _abi.LOGSTD_CLAMP


def test_pair_population_rejects_by_member_and_field():
  from earl_benchmark_amd.policy import AgentPair, MLPPolicy, PairPopulation, require_widths
  base = dict(switch_every=(5, 3), switch_on_success=True)
  a = pair_of(seed=0, **base)
  for G in (0, 8, 24):
    with pytest.raises(ValueError, match='envs_per_policy'):
      PairPopulation([a], envs_per_policy=G)
  with pytest.raises(ValueError, match='non-empty list of AgentPair'):
    PairPopulation([])
  with pytest.raises(ValueError, match='non-empty list of AgentPair'):
    PairPopulation([a, agents()[0]])
  pi12 = MLPPolicy(random_layers([12, 16, 3], seed=0))
  with pytest.raises(ValueError, match='observation width 12 and action width 3; 14 and 4 were declared'):
    PairPopulation([AgentPair(pi12, pi12)])
  table = np.ones((2, 7))
  cases = [('dims', pair_of(seed=1, dims=(14, 32, 4), **base)), ('gaussian', pair_of(seed=1, dims=(14, 16, 8), head=True, **base)),
           ('switch_every', pair_of(seed=1, switch_every=(5, 4), switch_on_success=True)), ('switch_on_success', pair_of(seed=1, switch_every=(5, 3), switch_on_success=False)),
           ('backward_goal', pair_of(seed=1, **base, backward_goal=np.zeros(7))), ('backward_goal', pair_of(seed=1, **base, backward_goal=table)),
           ('backward_goal', pair_of(seed=1, **base, backward_goal='initial_states'))]
  for field, other in cases:
    with pytest.raises(ValueError, match=f'member 2 has {field} = '):
      PairPopulation([a, pair_of(seed=3, **base), other])
  ga = pair_of(seed=0, dims=(14, 16, 8), head=True, **base)
  f, b = agents((14, 16, 8), True, 5)
  f.log_std_bounds = b.log_std_bounds = (-4.0, 1.0)
  with pytest.raises(ValueError, match='member 1 has log_std_bounds = '):
    PairPopulation([ga, AgentPair(f, b, obs_dim=14, act_dim=4, backward_goal=None, **base)])
  same_table = [pair_of(seed=p, **base, backward_goal=table.copy()) for p in range(2)]
  assert PairPopulation(same_table).n_policies == 2                       # (equal tables are one backward goal)

  # the member range against the env's global ids
  class Env:
    device = torch.device('cpu')

    def __init__(self, n, off):
      self.num_envs, self._cfg = n, _abi.SawyerCfg(n=n, env_offset=off)
  pop = PairPopulation([pair_of(seed=p, **base) for p in range(4)], envs_per_policy=16)
  assert require_widths(pop, 'rollout_agents', 14, 4, env=Env(64, 0), pair=True, pairs=True) is False
  assert require_widths(pop, 'rollout_agents', 14, 4, env=Env(13, 51), pair=True, pairs=True) is False
  for n, off in ((65, 0), (1, 64), (4, -1)):
    with pytest.raises(ValueError, match='rollout_agents: global env ids .* need members up to'):
      require_widths(pop, 'rollout_agents', 14, 4, env=Env(n, off), pair=True, pairs=True)
  with pytest.raises(ValueError, match='an AgentPair goes to rollout_agents'):
    require_widths(pop, 'rollout_policy', 14, 4, env=Env(64, 0))


def test_the_tabletop_refuses_a_table_and_a_pair_population_by_name():
  import earl_benchmark_amd as eb
  from earl_benchmark_amd.policy import PairPopulation
  _, env = eb.EARLEnvs('tabletop_manipulation', reward_type='sparse', num_envs=4, device='cpu', seed=3).get_envs()
  with pytest.raises(ValueError, match='a table of backward goals runs on the Sawyer door and peg only'):
    env.rollout_agents(pair_of(backward_goal=np.zeros((3, 7))), 5)
  with pytest.raises(ValueError, match='a table of backward goals runs on the Sawyer door and peg only'):
    env.rollout_agents(pair_of(backward_goal='initial_states'), 5)
  with pytest.raises(ValueError, match='a PairPopulation runs on the Sawyer door and peg only'):
    env.rollout_agents(PairPopulation([pair_of()]), 5)
  with pytest.raises(ValueError, match='observation width 14 and action width 4; the tabletop takes 12 and 3'):
    env.rollout_agents(pair_of(), 5)                                      # (ONE pair of the wrong widths: the message it always had)
  assert not hasattr(env.unwrapped, 'evaluate_agents')


def test_the_sawyer_envs_offer_the_surface():
  from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
  from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
  import inspect
  assert SawyerPeg.rollout_agents is SawyerDoor.rollout_agents and SawyerPeg.evaluate_agents is SawyerDoor.evaluate_agents
  assert list(inspect.signature(SawyerDoor.evaluate_agents).parameters) == ['self', 'pair', 'T', 'sample']
  assert inspect.signature(SawyerDoor.evaluate_agents).parameters['sample'].default is True


# ---------------------------------------------------------------------------------------------------------------- 4. where the table's fields live
def test_the_table_fields_live_in_the_policy_arguments_only():
  hdr = open(os.path.join(CSRC, 'physics_env_sawyer.h')).read()
  from population_no_gpu import policy_fields
  plain, policy, _ = policy_fields('physics_env_sawyer.h', 'SawyerPolicyArgs', 'SawyerArgs')
  for field in ('pair_goal', 'pair_goal_rows', 'pair_row', 'pair_row_out'):
    assert re.search(r'\b%s;' % field, policy) and field not in plain, field
  body = open(os.path.join(CSRC, 'physics_env_sawyer_rollout.inc')).read()
  for field in ('pair_goal', 'pair_goal_rows', 'pair_row', 'pair_row_out'):
    assert f'ka->{field}' in body and f'a.{field}' not in body, field      # read through the kernel-argument segment, at the point of use
  assert body.count('philox4x32_10(') == 1 and '0xFFFDu : 0xFFFEu' in body   # ONE draw, generalised: not a copy
  assert len(re.findall(r'void (\w+)\(const SawyerPolicyArgs a\)', hdr)) == 1      # no sibling kernel

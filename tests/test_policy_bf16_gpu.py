"""bf16 policy parameters inside the closed-loop rollouts of the door, the peg, the minitaur and the kitchen on the device (earl_mlp_policy.precision ==
EARL_PRECISION_BF16; the kernels of csrc/physics_bf16.hip, physics_w8_bf16.hip, physics_mt_bf16.hip and physics_kitchen_policy_bf16.hip).

The oracle everywhere is the float32 launch of `pi.widened()`: bf16 is a storage format, a stored value widens exactly and enters the same fmaf chain, so
everything a launch returns or leaves behind is compared BIT FOR BIT -- obs, reward, done, success, status, info, actions, eps, summaries, agent, backward_row, the
state tensors, fail_count, the pair's state and counters.  No tolerance anywhere.
  1. one policy, per env in every launch form (the door's two builds, the peg's two schedules, the minitaur's four forms, the kitchen's five): N = 40 (several
     workgroups, a ragged last wave; the peg's time-sliced schedule needs more 16-env workgroups than CUs), T = 6; networks (16,) and (48, 80) (rows clamped past the
     last output group; at 32 lanes per env a half-full last k-tile), deterministic and sampled, relu and tanh; the (48, 80) tanh network carries the special bf16
     values of tests/policy_bf16_cases.py in its first layer's first and last rows; (256, 256) once per env at N = 16, T = 2;
  2. T launches of one step == one launch of T, in bf16;
  3. a population: P = 3, G = 16, env_offset = 5, N = 40 (a wave holds envs of two members, the last member is partly used), a stride with padding beyond the rounded
     count; the rollout and the summary-only evaluation;
  4. the agent pair and the population of pairs: switch_every = (2, 3), T = 8 (both networks are read inside one launch), with and without switch_on_success, tables
     of backward goals of more than one row on the door, the peg and the kitchen, P = 2 pairs;
  5. make_step_graph(T, policy=pi_bf16) replays what the graph of pi.widened() replays (torch only: `.layers` hold the widened values).
The condition on the inputs: small-gain networks with a bounded output, so that no row of the float32 launch sits in the failure guard (asserted: status.sum() == 0,
guard_steps == 0): no env is excluded from any comparison."""
import contextlib

import numpy as np
import pytest

import policy_bf16_cases as B
from test_physics_step_graph_gpu import make, same
from test_sawyer_policy_rollout import random_layers

pytestmark = pytest.mark.gpu

N, T6 = 40, 6
GAIN, LAST_GAIN = 1.0, 0.5


def build(kind, hidden, hact='relu', head=False, seed=0, specials=False, lmap='tanh'):
  """-> the bf16 policy on the GPU (its oracle is .widened()): small random weights, tanh output; with a head the raw log-std biases at -2"""
  import torch
  from earl_benchmark_amd.policy import GaussianMLPPolicy, MLPPolicy
  O, A = B.WIDTHS[kind]
  layers = random_layers([O] + list(hidden) + [2 * A if head else A], seed=seed, gain=GAIN, last_gain=LAST_GAIN)
  if specials:
    assert hact == 'tanh'                                  # (the hidden layer bounds the rows that carry bf16's largest value)
    B.plant_specials(layers)
  if head:
    layers[-1][1][A:] = np.float32(-2.0)
    pi = GaussianMLPPolicy(layers, hact, squash=True, log_std_bounds=(-5.0, 2.0), log_std_map=lmap, device='cuda', obs_dim=O, act_dim=A, param_dtype=torch.bfloat16)
  else:
    pi = MLPPolicy(layers, hact, 'tanh', device='cuda', obs_dim=O, act_dim=A, param_dtype=torch.bfloat16)
  assert pi.params.dtype == torch.bfloat16 and pi.params.is_cuda and pi.struct.precision == 16 and pi.widened().struct.precision == 0
  if specials:
    np.testing.assert_array_equal(B.bits16(pi.params)[:len(B.SPECIAL)], B.special_bf16_bits())
  return pi


def same_dict(got, want, what):
  import torch
  assert set(got) == set(want), (what, sorted(got), sorted(want))
  for k in sorted(want):
    if torch.is_tensor(want[k]):
      same(got[k], want[k], f'{what}: {k}')
    elif isinstance(want[k], (tuple, list)):
      for i, (a, b) in enumerate(zip(got[k], want[k])):
        same(a, b, f'{what}: {k}[{i}]')
    else:
      assert got[k] == want[k], (what, k, got[k], want[k])


def same_state(ea, eb, what):
  ua, ub = ea.unwrapped, eb.unwrapped
  same_dict(ua.state_dict(), ub.state_dict(), what + ' state')
  same(ua._last_success, ub._last_success, what + ' _last_success')
  assert ua.total_step_count == ub.total_step_count
  if ub.pair_counts is not None:
    for i in (0, 1):
      same(ua.pair_counts[i], ub.pair_counts[i], f'{what} pair_counts[{i}]')


def clone(out):
  return {k: v.clone() for k, v in out.items()}


def no_guard(out, what):
  assert int((out['status'] != 0).sum()) == 0, what + ': a row of the float32 launch sits in the failure guard'


# ---------------------------------------------------------------------------------------------------------------- the launch forms, forced as the envs' own tests do
@contextlib.contextmanager
def door_variant(v):
  from earl_benchmark_amd import _abi
  lib = _abi.load()
  assert lib.earl_debug_set_door_variant(v) == 0
  try:
    yield
  finally:
    lib.earl_debug_set_door_variant(0)


@contextlib.contextmanager
def peg_schedule(k):
  from earl_benchmark_amd import _abi
  lib = _abi.load()
  lib.earl_debug_set_peg_schedule(k)
  try:
    yield
  finally:
    lib.earl_debug_set_peg_schedule(1)


def cu_count():
  import torch
  return torch.cuda.get_device_properties(0).multi_processor_count


def form_of(kind, form):
  """-> (context manager, n): the launch form for the block and the batch it runs at"""
  from test_kitchen_policy_rollout_gpu import launch_form as kitchen_form
  from test_minitaur_policy_rollout_gpu import FORMS as MT_FORMS, launch_form as minitaur_form
  if kind == 'door':
    return door_variant({'one_wave': 1, 'eight_wave': 2}[form]), N
  if kind == 'peg':
    # the time-sliced schedule runs when there are more 16-env workgroups than CUs: the smallest such batch, in slices of 2 env steps (three slices per env)
    return (peg_schedule(0), N) if form == 'static' else (peg_schedule(2), 16 * cu_count() + 24)
  if kind == 'minitaur':
    return minitaur_form(**MT_FORMS[form]), N
  return kitchen_form(int(form)), N


FORMS = ([('door', 'one_wave'), ('door', 'eight_wave'), ('peg', 'static'), ('peg', 'sliced')] +
         [('minitaur', f) for f in ('one_wave_packed', 'one_wave_env_per_wave', 'one_wave_env_per_workgroup', 'two_wave')] + [('kitchen', str(s)) for s in range(5)])
# (hidden, hidden activation, Gaussian head sampled, the special bf16 values planted)
NETS = [((16,), 'relu', False, False), ((16,), 'tanh', True, False), ((48, 80), 'tanh', False, True), ((48, 80), 'relu', True, False)]


# ---------------------------------------------------------------------------------------------------------------- 1. one policy, every launch form
@pytest.mark.parametrize('kind,form', FORMS, ids=[f'{k}-{f}' for k, f in FORMS])
def test_one_policy_in_every_launch_form(kind, form):
  ctx, n = form_of(kind, form)
  with ctx:
    ea, eb = make(kind, n, seed=5, env_offset=3), make(kind, n, seed=5, env_offset=3)
    if (kind, form) == ('peg', 'sliced'):
      assert ea.unwrapped._uses_queue(T6) and (n + 15) // 16 > cu_count()
    for s, (hidden, hact, head, specials) in enumerate(NETS):           # (the two envs walk through the four launches in step)
      pi = build(kind, hidden, hact, head, seed=10 * s + len(kind), specials=specials, lmap=('tanh', 'clamp')[s % 2])
      kw = {'return_noise': True} if head else {}
      want = clone(eb.rollout_policy(pi.widened(), T6, **kw))
      got = clone(ea.rollout_policy(pi, T6, **kw))
      what = f'{kind} {form} {hidden} {hact} head={head}'
      no_guard(want, what)
      assert tuple(want['actions'].shape) == (T6, n, B.WIDTHS[kind][1]) and float(want['actions'].abs().max()) <= 1.0 and bool((want['actions'] != 0).any())
      same_dict(got, want, what)
      same_state(ea, eb, what)


@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur', 'kitchen'])
def test_the_widest_network(kind):
  n, T = 16, 2
  ea, eb = make(kind, n, seed=6), make(kind, n, seed=6)
  pi = build(kind, (256, 256), 'relu', True, seed=21)
  want = clone(eb.rollout_policy(pi.widened(), T, return_noise=True))
  got = clone(ea.rollout_policy(pi, T, return_noise=True))
  no_guard(want, kind)
  same_dict(got, want, kind + ' 256 x 256')
  same_state(ea, eb, kind + ' 256 x 256')
  # the rounding is in the values: the float32 policy of the UNROUNDED parameters acts otherwise
  import torch
  from earl_benchmark_amd.policy import GaussianMLPPolicy
  O, A = B.WIDTHS[kind]
  layers = random_layers([O, 256, 256, 2 * A], seed=21, gain=GAIN, last_gain=LAST_GAIN)
  layers[-1][1][A:] = np.float32(-2.0)
  exact = GaussianMLPPolicy(layers, 'relu', squash=True, log_std_bounds=(-5.0, 2.0), log_std_map='tanh', device='cuda', obs_dim=O, act_dim=A)
  ec = make(kind, n, seed=6)
  assert not torch.equal(ec.rollout_policy(exact, T)['actions'], want['actions'])


# ---------------------------------------------------------------------------------------------------------------- 2. T launches of one == one launch of T
@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur', 'kitchen'])
def test_launches_of_one_step_equal_one_launch(kind):
  import torch
  n, T = 16, 4
  ea, eb = make(kind, n, seed=7, env_offset=2), make(kind, n, seed=7, env_offset=2)
  pi = build(kind, (48, 80), 'tanh', True, seed=4, specials=True)
  one = clone(ea.rollout_policy(pi, T, return_noise=True))
  rows = [clone(eb.rollout_policy(pi, 1, return_noise=True)) for _ in range(T)]
  no_guard(one, kind)
  same_dict({k: torch.cat([r[k] for r in rows]) for k in rows[0]}, one, kind)
  same_state(eb, ea, kind)


# ---------------------------------------------------------------------------------------------------------------- 3. a population
def population(kind, P, hact='relu', head=False, pad=16):
  """P bf16 members behind a stride with `pad` elements of padding beyond the rounded count (the template form)"""
  import torch
  from earl_benchmark_amd.policy import PolicyPopulation
  O, A = B.WIDTHS[kind]
  members = [build(kind, (48, 80), hact, head, seed=30 + p, specials=(hact == 'tanh' and p == 1)) for p in range(P)]
  tight = PolicyPopulation(members, envs_per_policy=16, obs_dim=O, act_dim=A)
  wide = torch.full((P, tight.stride + pad), 7.0, dtype=torch.bfloat16)      # (the padding is never read: rubbish there changes nothing)
  wide[:, :tight.n_params] = tight.params[:, :tight.n_params].cpu()
  pop = PolicyPopulation(members[0], envs_per_policy=16, params=wide, device='cuda', obs_dim=O, act_dim=A)
  assert pop.stride == tight.stride + pad and pop.stride % 8 == 0 and pop.stride > (pop.n_params + 7) // 8 * 8 and pop.struct.precision == 16
  return pop


@pytest.mark.parametrize('head', [False, True], ids=['deterministic', 'sampled'])
@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur', 'kitchen'])
def test_population_rollout_and_evaluation(kind, head):
  P, off = 3, 5
  ea, eb = make(kind, N, seed=8, env_offset=off), make(kind, N, seed=8, env_offset=off)
  pop = population(kind, P, 'tanh' if head else 'relu', head)
  wpop = pop.widened()
  assert (off + N - 1) // 16 == P - 1 and (off + N) % 16 != 0 and wpop.struct.precision == 0      # every member runs, the last one partly
  sawyer = kind in ('door', 'peg')
  kw = {'return_noise': True} if head else {}
  roll = lambda env, p: clone((env.rollout_policy if sawyer else env.rollout_population)(p, T6, **kw))
  want, got = roll(eb, wpop), roll(ea, pop)
  no_guard(want, kind)
  same_dict(got, want, kind + ' population')
  same_state(ea, eb, kind + ' population')
  ev = lambda env, p: (env.evaluate_policy if sawyer else env.evaluate_population)(p, T6, episodes=1, sample=head)
  want, got = ev(eb, wpop), ev(ea, pop)
  assert set(want) == {'ret', 'success', 'first_success', 'guard_steps'} and int(want['guard_steps'].sum()) == 0
  same_dict(got, want, kind + ' population summaries')
  same_state(ea, eb, kind + ' population summaries')


# ---------------------------------------------------------------------------------------------------------------- 4. the agent pair, the population of pairs
def backward_goal_of(kind, env):
  """a backward goal with a table of more than one row where the env takes one (door: five rows around its reset row; peg, kitchen: their initial states)"""
  if kind == 'door':
    from test_sawyer_agents_gpu import door_table
    return door_table(env.unwrapped)
  return 'initial' if kind == 'minitaur' else 'initial_states'


def pair_of(kind, env, seed, head, sos, hact='relu'):
  from earl_benchmark_amd.policy import AgentPair
  O, A = B.WIDTHS[kind]
  f, b = build(kind, (48, 80), hact, head, seed=seed), build(kind, (48, 80), hact, head, seed=seed + 1, specials=hact == 'tanh')
  return AgentPair(f, b, switch_every=(2, 3), switch_on_success=sos, backward_goal=backward_goal_of(kind, env), obs_dim=O, act_dim=A)


def pair_calls(kind):
  sawyer = kind in ('door', 'peg')
  return (lambda env, p, T, **kw: (env.rollout_agents if sawyer else env.rollout_pair)(p, T, **kw),
          lambda env, p, T: (env.evaluate_agents if sawyer else env.evaluate_pair)(p, T))


@pytest.mark.parametrize('sos', [False, True], ids=['by_the_clock', 'switch_on_success'])
@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur', 'kitchen'])
def test_agent_pair(kind, sos):
  T = 8
  ea, eb = make(kind, N, seed=9, env_offset=3), make(kind, N, seed=9, env_offset=3)
  head = bool(sos)
  pair = pair_of(kind, ea, 40, head, sos, 'tanh' if sos else 'relu')
  wpair = pair.widened()
  assert pair.params.dtype != wpair.params.dtype and pair.struct.precision == 16 and wpair.struct.precision == 0 and pair.stride % 8 == 0
  rollout, evaluate = pair_calls(kind)
  kw = {'return_noise': True} if head else {}
  want, got = clone(rollout(eb, wpair, T, **kw)), clone(rollout(ea, pair, T, **kw))
  no_guard(want, kind)
  assert set(want['agent'].unique().tolist()) == {0, 1}                  # both networks were read inside the launch
  if kind != 'minitaur':
    assert 'backward_row' in want and int(want['backward_row'].max()) >= 1      # ... and a table of more than one row was drawn from
  same_dict(got, want, kind + ' pair')
  same_state(ea, eb, kind + ' pair')
  want, got = evaluate(eb, wpair, T), evaluate(ea, pair, T)               # (continues from the phases the rollout left)
  assert int(want['guard_steps'].sum()) == 0
  same_dict(got, want, kind + ' pair summaries')
  same_state(ea, eb, kind + ' pair summaries')


@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur', 'kitchen'])
def test_population_of_pairs(kind):
  from earl_benchmark_amd.policy import PairPopulation
  n, off, T = 24, 5, 8
  ea, eb = make(kind, n, seed=10, env_offset=off), make(kind, n, seed=10, env_offset=off)
  pairs = PairPopulation([pair_of(kind, ea, 50 + 2 * p, True, True, 'tanh') for p in range(2)], envs_per_policy=16, device='cuda')
  wpairs = pairs.widened()
  assert pairs.struct.precision == 16 and wpairs.struct.precision == 0 and pairs.pair_stride % 8 == 0 and (off + n - 1) // 16 == 1
  rollout, evaluate = pair_calls(kind)
  want, got = clone(rollout(eb, wpairs, T, return_noise=True)), clone(rollout(ea, pairs, T, return_noise=True))
  no_guard(want, kind)
  assert set(want['agent'].unique().tolist()) == {0, 1}
  same_dict(got, want, kind + ' pairs')
  same_state(ea, eb, kind + ' pairs')
  want, got = evaluate(eb, wpairs, T), evaluate(ea, pairs, T)
  assert int(want['guard_steps'].sum()) == 0
  same_dict(got, want, kind + ' pairs summaries')
  same_state(ea, eb, kind + ' pairs summaries')


# ---------------------------------------------------------------------------------------------------------------- 5. the step graph (torch only)
@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur', 'kitchen'])
def test_step_graph_with_a_bf16_policy_replays_the_widened_policy(kind):
  import torch
  n, T = 8, 3
  ea, eb = make(kind, n, seed=11), make(kind, n, seed=11)
  pi = build(kind, (48, 80), 'tanh', False, seed=12, specials=True)
  ga, gb = ea.make_step_graph(T, policy=pi), eb.make_step_graph(T, policy=pi.widened())
  for rep in range(2):
    oa, ra, da, ia = ga.replay()
    ob, rb, db, ib = gb.replay()
    same(oa, ob, 'obs'), same(ra, rb, 'reward'), same(da, db, 'done'), same(ga.actions, gb.actions, 'actions')
    for k in ib:
      if torch.is_tensor(ib[k]):
        same(ia[k], ib[k], 'info ' + k)
    assert bool((gb.actions != 0).any())
  same_state(ea, eb, kind + ' step graph')

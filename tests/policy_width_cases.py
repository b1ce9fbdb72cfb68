"""The case tables of the width and instantiation matrix of the in-kernel policies, shared by tests/test_policy_math.py (no GPU: the tables reach every
instantiation and every width, and the host twin alone meets the sensitivity condition on every case) and tests/test_policy_widths_gpu.py /
tests/test_sawyer_policy_widths_gpu.py (the device against the host twin on these cases).

The launchers' dispatch rule, restated (csrc/tabletop_policy.hip, tabletop_policy_gaussian.hip, tabletop_policy_population.hip, tabletop_pair_kernel.h):
  NT2     = ceil(dims[2] / 64) with two hidden layers, 0 with one              (the pair: 0 .. 2, EARL_PAIR_MAX_H2 = 128)
  GENERAL = goal_change_frequency > 0 or auto_reset                           (the pair: always)
  GAUSS   = a head is given
  POP     = the population entry point"""
import numpy as np

import hip_harness as hx
from gaussian_policy_helpers import GaussPolicy, gaussian_rollout
from pair_helpers import Pair, PairState, pair_rollout
from population_helpers import Population, members_needed, population_rollout
from test_policy_rollout import Policy, final_state, policy_rollout

WIDTHS = tuple(range(16, 257, 16))
ONE_HIDDEN = [(h,) for h in WIDTHS]
ANTI_DIAGONAL = [(272 - h2, h2) for h2 in WIDTHS]                        # both layers see every width; H1 != H2 (136 is no width)
CLASS_EDGES = [(h, h) for h in (64, 80, 128, 144, 192, 208, 256)]
SHAPES = ONE_HIDDEN + ANTI_DIAGONAL + CLASS_EDGES
PAIR_MAX_H2 = 128

# the smallest launch that still has a full workgroup, a middle one and a ragged one (16 envs per workgroup)
N, OFFSET, T = 40, 3, 12
FORMS = ('evaluation', 'continuing')
HEADS = ('deterministic', 'sample')
GAIN = 1.0                                                              # of Policy: the helper's own (some actions saturate the env's clip, some do not)
LOG_STD_GAIN = 2.0                                                      # of GaussPolicy's raw log_std rows: raw spans about +-4, so sigma stays small enough that a tanh output does not saturate on every row


def nt2_of(hidden):
  return (hidden[1] + 63) // 64 if len(hidden) == 2 else 0


def instantiation(entry, hidden, cfg_kw, head):
  """the kernel instantiation a launch dispatches to, as the launchers decide it: ('single' | 'population' | 'pair', NT2, GENERAL, GAUSS)"""
  general = cfg_kw.get('goal_change_frequency', 0) > 0 or bool(cfg_kw.get('auto_reset', False))
  if entry == 'pair':
    assert nt2_of(hidden) <= 2
    general = True
  return (entry, nt2_of(hidden), general, head != 'deterministic')


def name_of(inst):
  entry, nt2, general, gauss = inst
  kernel = {'single': 'policy_rollout_kernel', 'population': 'policy_population_kernel', 'pair': 'pair_kernel'}[entry]
  if entry == 'pair':                                                   # (no GENERAL parameter: the pair's step is always the general one)
    return f'{kernel}<NOBJ = 1, NT2 = {nt2}, GAUSS = {str(gauss).lower()}>'
  return f'{kernel}<NT2 = {nt2}, GENERAL = {str(general).lower()}, GAUSS = {str(gauss).lower()}>'


class Case:
  """one row of the table: shape x head x form, with the alternating settings fixed by the shape's position `s` in SHAPES"""

  def __init__(self, s, hidden, head, form):
    self.s, self.hidden, self.head, self.form = s, hidden, head, form
    self.hact = ('relu', 'tanh')[s % 2]
    self.oact = ('tanh', 'none')[(s // 2) % 2]
    self.log_std_map = ('tanh', 'clamp')[(s % 3) % 2]
    self.reset_first = form == 'evaluation'
    self.E = 2 if self.reset_first else 1
    if self.reset_first:
      self.cfg_kw = dict(horizon=T)
    else:                                                               # a goal switch or an auto reset falls inside the launch
      self.cfg_kw = (dict(goal_change_frequency=5, horizon=10**6), dict(auto_reset=True, horizon=7))[(s // 4 + s) % 2]
    self.inst = instantiation('single', hidden, self.cfg_kw, head)
    self.seed = 1000 + 10 * s + (head == 'sample')
    self.id = f'{"x".join(map(str, hidden))}-{head}-{form}'

  def harness_kw(self):
    return dict(reward_type='sparse', wide_init=True, seed=self.seed, env_offset=OFFSET, **self.cfg_kw)

  def policy(self, device):
    if self.head == 'sample':
      return GaussPolicy(self.hidden, self.hact, self.oact, seed=self.seed, device=device, log_std_gain=LOG_STD_GAIN)
    return Policy(self.hidden, self.hact, self.oact, seed=self.seed, gain=GAIN, device=device)

  def harness(self, device):
    h = hx.HipTabletop(N, device=device, **self.harness_kw())
    h.reset()
    if not self.reset_first:                                            # a continuing rollout starts somewhere: a few scripted steps first
      h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, N, 3)).astype(np.float32))
    return h

  def run(self, h, pol):
    if self.head == 'sample':
      return gaussian_rollout(h, pol, self.E, T, self.reset_first, mode='sample', log_std_map=self.log_std_map)
    return policy_rollout(h, pol, self.E, T, self.reset_first)

  def keys(self):
    return ('act',) + (('eps',) if self.head == 'sample' else ()) + ('obs', 'reward', 'done', 'success')


CASES = [Case(s, hidden, head, form) for s, hidden in enumerate(SHAPES) for head in HEADS for form in FORMS]

# the population: one shape per NT2 class (ragged widths: waves with unequal numbers of tiles), both forms, both heads -- its 20 instantiations
POPULATION_SHAPES = [(208,), (144, 48), (80, 112), (112, 176), (48, 240)]
POPULATION_G = 16                                                        # global ids 3 .. 42: members 0, 1, 2, one per workgroup
POPULATION_FORMS = {'evaluation': dict(horizon=T), 'continuing': dict(goal_change_frequency=5, horizon=10**6)}
POPULATION_CASES = [(hidden, head, form) for hidden in POPULATION_SHAPES for head in HEADS for form in FORMS]

HEAD_KW = {'deterministic': None, 'sample': dict(mode='sample', log_std_map='tanh')}


def zero_last_tile(params, hidden, layer):
  """the last 16 rows (the last N-tile) of hidden layer `layer`'s weights and biases set to zero, in place; params: the packed parameters [n_params], or one
  row per member [P, stride]"""
  dims = [12] + list(hidden)
  off = sum(dims[l + 1] * (dims[l] + 1) for l in range(layer))
  k, n = dims[layer], dims[layer + 1]
  params[..., off + (n - 16) * k:off + n * k] = 0
  params[..., off + n * k + n - 16:off + n * k + n] = 0


def population_run(device, hidden, head, form, mutate=None):
  """one launch of the population entry point -> (outputs, final state); mutate(params [P, stride]) edits the members' parameters before the launch"""
  reset_first = form == 'evaluation'
  P = members_needed(OFFSET, N, POPULATION_G)
  popn = Population(hidden, P, POPULATION_G, gaussian=head == 'sample', hidden_act='tanh' if len(hidden) == 2 and hidden[1] % 32 else 'relu', seed0=11, device=device)
  if mutate:
    mutate(popn.params)
  h = hx.HipTabletop(N, device=device, reward_type='sparse', wide_init=True, seed=77, env_offset=OFFSET, **POPULATION_FORMS[form])
  h.reset()
  if not reset_first:
    h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, N, 3)).astype(np.float32))
  res = population_rollout(h, popn.struct, popn.pop, 2 if reset_first else 1, T, reset_first, head=HEAD_KW[head])
  return res, final_state(h)


# the pair: every width with one hidden layer, the anti-diagonal up to EARL_PAIR_MAX_H2, and the largest square
PAIR_SHAPES = ONE_HIDDEN + [sh for sh in ANTI_DIAGONAL if sh[1] <= PAIR_MAX_H2] + [(128, 128)]
PAIR_CASES = [(hidden, head) for hidden in PAIR_SHAPES for head in HEADS]
PAIR_SWITCH_EVERY, PAIR_SWITCH_ON_SUCCESS = (7, 5), 1



def pair_run(device, hidden, head, mutate=None):
  """one continuing launch of the pair entry point from mixed phases -> (outputs, final state, (phase, steps_in_phase)); both clocks run out inside the launch"""
  s = PAIR_SHAPES.index(hidden)
  pr = Pair(hidden, gaussian=head == 'sample', hidden_act=('relu', 'tanh')[s % 2], out_act=('tanh', 'none')[(s // 2) % 2], seed0=4 + s, device=device)
  if mutate:
    mutate(pr.params)
  h = hx.HipTabletop(N, device=device, reward_type='sparse', reset_at_goal=True, wide_init=True, seed=9, env_offset=OFFSET, horizon=10**6)
  h.reset()
  h.rollout(np.random.default_rng(1).uniform(-1, 1, size=(9, N, 3)).astype(np.float32))
  rng = np.random.default_rng(0)                                          # every workgroup mixed from the first step on
  ps = PairState(N, device=device, phase=rng.integers(0, 2, N).astype(np.int8), sip=rng.integers(0, 4, N).astype(np.int32))
  res = pair_rollout(h, pr, ps, 1, T, False, PAIR_SWITCH_EVERY, PAIR_SWITCH_ON_SUCCESS, head=HEAD_KW[head])
  return res, final_state(h), ps.host()


# exact lane maps (weights in {-1, 0, 1}): the wide shapes of the issue and one ragged shape per NT2 class
EXACT_SHAPES = [(256,), (128, 192), (192, 128), (256, 256), (208,), (240, 48), (144, 80), (80, 176), (112, 208)]

# the Sawyer rollout: pol_layer works in groups of 64 output rows
SAWYER_SHAPES = ONE_HIDDEN + ANTI_DIAGONAL + [(80, 80), (144, 208)]
SAWYER_PEG_WIDTHS = (48, 64, 80, 128, 144, 240, 256)                      # the group edges
SAWYER_N, SAWYER_OFFSET, SAWYER_T = 32, 3, 6
SAWYER_HEADS = (None, 'mean', 'sample')


def sawyer_cases():
  """[(kind, hidden, hidden_act, out_act, head, log_std_map)]: every shape on the door, the group-edge widths on the peg as well; head, activations and map alternate"""
  rows = [('door', sh) for sh in SAWYER_SHAPES] + [('peg', sh) for sh in SAWYER_SHAPES if (sh[-1] in SAWYER_PEG_WIDTHS and (len(sh) == 1 or sh in ANTI_DIAGONAL))]
  out = []
  for s, (kind, sh) in enumerate(rows):
    out.append((kind, sh, ('relu', 'tanh')[s % 2], ('tanh', 'none')[(s // 2) % 2], SAWYER_HEADS[s % 3], ('clamp', 'tanh')[(s // 3) % 2]))
  return out


def sawyer_groups(width):
  """(full groups of 64 output rows, rows of the partial group after them)"""
  return width // 64, width % 64

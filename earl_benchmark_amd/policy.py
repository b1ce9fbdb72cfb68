"""A float32 MLP policy 12 -> hidden (-> hidden) -> 3 (tabletop; obs_dim=14, act_dim=4: the Sawyer door and peg) in the form the fused closed-loop rollout takes (include/earl_tabletop.h: struct
earl_mlp_policy, earl_tabletop_policy_rollout): the parameters packed once, layer by layer (W_l row-major like torch.nn.Linear.weight, then b_l).

  pi = MLPPolicy([(w0, b0), (w1, b1)], hidden_act='relu', out_act='tanh', device='cuda')      # or MLPPolicy(torch.nn.Sequential(...))
  obs, reward, done, success, actions = env.rollout_policy(pi, T=200, episodes=4)               # ONE launch: reset + T closed-loop steps, x 4
  g = env.make_step_graph(T, policy=pi)                                                         # the same network as torch ops between captured steps

`pi(obs)` evaluates the same network with torch (matmul order is torch's: close to, not bit-identical with, the fused kernel, whose arithmetic is the
k-ascending fmaf chain that csrc/tabletop_policy.h states).

The Sawyer door and peg take the same two classes with obs_dim=14, act_dim=4 (include/earl_physics.h: earl_sawyer_policy_rollout):

  pi = MLPPolicy(layers, 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4)
  out = door.rollout_policy(pi, T=300)                                                          # rollout()'s dict plus 'actions' [T, N, 4], ONE launch

The three-object tabletop takes the same classes with obs_dim=20, act_dim=3 (include/earl_tabletop.h: earl_tabletop3_policy_rollout), packed as the tabletop's
(float32, rows as they are), a `PolicyPopulation` of them included; what it returns is the single-object env's with obs [.., 20]:

  pi = MLPPolicy(layers, 'relu', 'tanh', device='cuda', obs_dim=20, act_dim=3)                  # or GaussianMLPPolicy(..., obs_dim=20, act_dim=3)
  obs, reward, done, success, actions = env3.rollout_policy(pi, T=200, episodes=4)              # ONE launch
  s = env3.evaluate_policy(PolicyPopulation([...], obs_dim=20, act_dim=3), T=200)               # summaries only

The minitaur takes them with obs_dim=32, act_dim=8 and a bounded output (include/earl_physics.h: earl_minitaur_policy_rollout):

  pi = MLPPolicy(layers, 'relu', 'tanh', device='cuda', obs_dim=32, act_dim=8)                  # or GaussianMLPPolicy(..., squash=True, obs_dim=32, act_dim=8)
  out = minitaur.rollout_policy(pi, T=250)                                                      # rollout()'s dict plus 'actions' [T, N, 8], ONE launch

The kitchen takes them with obs_dim=46, act_dim=9, bounded or not -- the env clips the action as the reference does (include/earl_physics.h: earl_kitchen_policy_rollout):

  pi = MLPPolicy(layers, 'relu', 'tanh', device='cuda', obs_dim=46, act_dim=9)                  # or GaussianMLPPolicy(..., obs_dim=46, act_dim=9)
  out = kitchen.rollout_policy(pi, T=400)                                                       # rollout()'s dict plus 'actions' [T, N, 9], ONE launch

On those four envs (door, peg, minitaur, kitchen) the parameters may be STORED as bf16 (include/earl_tabletop.h: EARL_PRECISION_BF16), which halves what the kernel loads per
env step -- worth it for wide networks (256 x 256), not for narrow ones.  The arithmetic stays float32 on the exactly widened values:

  pi = MLPPolicy(layers, 'relu', 'tanh', device='cuda', obs_dim=14, act_dim=4, param_dtype=torch.bfloat16)      # each parameter rounded once; pi.params is the bf16 tensor the kernel reads
  out = door.rollout_policy(pi, T=300)                                                          # bit-identical to door.rollout_policy(pi.widened(), T=300)
  pi32 = pi.widened()                                                                           # the float32 policy of exactly those values (what the tabletop takes)

`GaussianMLPPolicy` is the SAC-style actor with a tanh-Gaussian head, 12 -> hidden (-> hidden) -> 6 (rows 0..2 mean, rows 3..5 raw log_std), for
earl_tabletop_policy_rollout_gaussian: the actions are SAMPLED inside the kernel from the env's counter-based RNG.

  pi = GaussianMLPPolicy(actor_trunk, squash=True, log_std_bounds=(-5.0, 2.0), log_std_map='tanh', device='cuda')
  obs, reward, done, success, actions = env.rollout_policy(pi, T=200, episodes=4)                     # exploration: tanh(mean + exp(log_std) eps)
  obs, reward, done, success, actions, eps = env.rollout_policy(pi, T=200, return_noise=True)         # ... and the standard-normal draws as used
  obs, reward, done, success, actions = env.rollout_policy(pi, T=200, episodes=4, sample=False)       # evaluation at the mean, same packed network

`PolicyPopulation` is P networks of ONE architecture (checkpoints, seeds, the perturbed copies of an evolution strategy) for earl_tabletop_population_rollout: the env
with global id g runs member g // envs_per_policy, all in one launch, and `evaluate_policy` returns one return / success per episode instead of [T] arrays.

  pop = PolicyPopulation([pi_0, ..., pi_255], envs_per_policy=16, device='cuda')                      # or PolicyPopulation(pi, params=theta)  with theta [P, n_params]
  s = env.evaluate_policy(pop, T=200, episodes=4)                                                     # {'ret': [4, N] float64, 'success': [4, N] bool, 'first_success': [4, N] int32}
  fitness = sharding.population_fitness(s, env_offset, pop.envs_per_policy, pop.n_policies)           # [P, 3]: return sum, success count, rows -- additive over shards
  pop.params.add_(sigma * noise)                                                                      # [P, stride], read by the next launch as it is

The Sawyer door and peg take populations of 14 / 4 members (include/earl_physics.h: earl_sawyer_population_rollout), one episode per launch:

  pop = PolicyPopulation([pi_0, ..., pi_511], envs_per_policy=16, device='cuda', obs_dim=14, act_dim=4)
  out = door.rollout_policy(pop, T=300)                                                               # what it returns for one policy
  s = door.evaluate_policy(pop, T=300, episodes=4)                                                    # the tabletop's dict plus 'guard_steps' [4, N] int32; no [T] tensor

`AgentPair` is the forward / reset agent pair of autonomous RL for earl_tabletop_pair_rollout: two networks of ONE architecture that hand every env to each other
after a fixed number of steps or as soon as the acting agent has succeeded, inside one launch.

  pair = AgentPair(forward_pi, backward_pi, switch_every=(200, 200), switch_on_success=True, backward_goal='initial', device='cuda')
  obs, reward, done, success, actions, agent = env.rollout_agents(pair, T=1000)                       # the training stream: continuing, agent [T, N] int8 = who acted
  env.agent_phase, env.steps_in_phase, env.pair_counts                                                # the state the next launch continues from; successes of the last one

The Sawyer door and peg take pairs of 14 / 4 agents in the general form (include/earl_physics.h: earl_sawyer_agents_rollout): a TABLE of backward goals the reset
agent's goal is drawn from at every handover, a `PairPopulation` of P pairs in one launch, and summaries instead of [T] arrays.

  pair = AgentPair(f, b, switch_every=(200, 200), backward_goal='initial_states', obs_dim=14, act_dim=4)       # or backward_goal=rows [R, 7]
  out = peg.rollout_agents(pair, T=1000)                                                              # ... plus 'backward_row' [T, N] int32: the row drawn, -1 elsewhere
  pairs = PairPopulation([pair_0, ..., pair_511], envs_per_policy=16, device='cuda')                  # .params [P, 2, stride], written in place
  s = peg.evaluate_agents(pairs, T=1000)                                                              # {'ret', 'success', 'first_success', 'guard_steps', 'forward_success', 'backward_success'}: [N]"""
import operator

import numpy as np
import torch

from . import _abi

OBS_DIM, ACT_DIM = 12, 3
TABLETOP_WIDTHS = ((OBS_DIM, ACT_DIM), (20, ACT_DIM))      # the single-object and the three-object tabletop: weights in registers, float32 only, rows taken as they are
MIN_WIDTH, MAX_WIDTH = 16, 256
PARAM_DTYPES = {torch.float32: 0, torch.bfloat16: _abi.PRECISION_BF16}      # param_dtype -> earl_mlp_policy.precision


def _param_dtype(who, dtype):
  if dtype not in PARAM_DTYPES:
    raise ValueError(f'{who}: param_dtype must be torch.float32 or torch.bfloat16, got {dtype!r}')
  return dtype


def _piece(dtype, tabletop=False):
  """elements of `dtype` in a 16-byte piece: what the stepper kernels read the rows of a container in, so what its stride is padded to (the tabletop's float32
  rows are taken as they are)"""
  return 8 if dtype == torch.bfloat16 else (1 if tabletop else 4)


def _padded(host, piece):
  """rows [..., n] -> rows of whole `piece`s, zero-filled"""
  return torch.nn.functional.pad(host, (0, -host.shape[-1] % piece)) if host.shape[-1] % piece else host


def _unpack(rows, dims):
  """packed rows [..., stride] (W0, b0, W1, b1, ...) -> [(W [..., n, k], b [..., n])] as views of them"""
  layers, at = [], 0
  for k, n in zip(dims[:-1], dims[1:]):
    layers.append((rows[..., at:at + n * k].reshape(*rows.shape[:-1], n, k), rows[..., at + n * k:at + n * k + n]))
    at += n * k + n
  return layers


def _forward(obs, layers, hidden_act, act_dim):
  """the network as torch ops: obs [..., obs_dim] -> (the first act_dim outputs, every output) before the output activation"""
  x = obs.to(torch.float32)
  for l, (w, b) in enumerate(layers):
    x = torch.addmm(b, x.reshape(-1, x.shape[-1]), w.t()).reshape(*x.shape[:-1], w.shape[0])
    if l + 1 < len(layers):
      x = torch.relu(x) if hidden_act == 'relu' else torch.tanh(x)
  return x[..., :act_dim], x


def _require_shared(who, members, attrs, clause):
  """every member's `attrs` ('a', or 'template.a': shown as 'a') equal member 0's"""
  for p, m in enumerate(members):
    for what in attrs:
      get = operator.attrgetter(what)
      if get(m) != get(members[0]):
        raise ValueError(f'{who}: member {p} has {what.rpartition(".")[2].strip("_")} = {get(m)!r}, member 0 has {get(members[0])!r} ({clause})')


class _PackedMLP:
  """What the four containers share: the architecture's scalars, `.params` on a device and struct earl_mlp_policy over it."""
  SHARED = ('__class__', 'dims', 'hidden_act', 'out_act', 'param_dtype')      # what the members of a container have in common, and for a Gaussian head:
  SHARED_HEAD = ('squash', 'log_std_bounds', 'log_std_map')

  def _describe(self, dims, hidden_act, out_act, gaussian, param_dtype):
    self.dims, self.hidden_act, self.out_act, self.gaussian, self.param_dtype = list(dims), hidden_act, out_act, gaussian, param_dtype
    self.macs = sum(k * n for k, n in zip(dims[:-1], dims[1:]))          # multiply-adds per env step
    self.n_params = sum(n * (k + 1) for k, n in zip(dims[:-1], dims[1:]))

  def _describe_like(self, t):
    self._describe(t.dims, t.hidden_act, t.out_act, t.gaussian, t.param_dtype)

  def to(self, device):
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    self.device = dev
    self._place()
    dims = self.dims + [0] * (4 - len(self.dims))
    self.struct = _abi.MlpPolicy(n_layers=len(self.dims) - 1, dims=(_abi.C.c_int32 * 4)(*dims), hidden_act=_abi.ACTIVATIONS[self.hidden_act],
                                 out_act=_abi.ACTIVATIONS[self.out_act], precision=PARAM_DTYPES[self.param_dtype], params=self.params.data_ptr())
    return self

  def _place(self):
    """(to's hook) `.params` onto `.device`, and what a container keeps next to it"""
    self.params = self.params.to(self.device).contiguous()

  def _population(self):
    return _abi.PolicyPopulation(n_policies=self.n_policies, envs_per_policy=self.envs_per_policy, param_stride=self.stride)


def _like(t, row, device, param_dtype, obs_dim, act_dim):
  """a policy of `t`'s class, architecture and head over a copy of the packed `row`"""
  layers = [(w.clone(), b.clone()) for w, b in _unpack(row.detach().to('cpu', torch.float32), t.dims)]
  if isinstance(t, GaussianMLPPolicy):
    return GaussianMLPPolicy(layers, t.hidden_act, squash=t.squash, log_std_bounds=t.log_std_bounds, log_std_map=t.log_std_map, device=device, obs_dim=obs_dim,
                             act_dim=act_dim, param_dtype=param_dtype)
  return MLPPolicy(layers, t.hidden_act, t.out_act, device=device, obs_dim=obs_dim, act_dim=act_dim, param_dtype=param_dtype)


def _layers_of_sequential(seq):
  layers, acts = [], []
  for m in seq:
    if isinstance(m, torch.nn.Linear):
      if m.bias is None:
        raise ValueError('MLPPolicy: every Linear needs a bias (pass zeros)')
      layers.append((m.weight.detach(), m.bias.detach()))
      acts.append('none')
    elif isinstance(m, (torch.nn.ReLU, torch.nn.Tanh)):
      if not layers or acts[-1] != 'none':
        raise ValueError('MLPPolicy: an activation must follow a Linear')
      acts[-1] = 'relu' if isinstance(m, torch.nn.ReLU) else 'tanh'
    else:
      raise ValueError(f'MLPPolicy: unsupported module {type(m).__name__} (Linear / ReLU / Tanh only)')
  if len(layers) < 2:
    raise ValueError('MLPPolicy: need at least one hidden layer')
  hidden = set(acts[:-1])
  if len(hidden) != 1 or hidden == {'none'}:
    raise ValueError(f'MLPPolicy: the hidden layers must share one activation (relu or tanh), got {acts[:-1]}')
  return layers, hidden.pop(), acts[-1]


class MLPPolicy(_PackedMLP):
  OUT_DIM, OUT_WHAT = ACT_DIM, 'action'

  def __init__(self, layers, hidden_act='relu', out_act='tanh', device='cpu', obs_dim=OBS_DIM, act_dim=ACT_DIM, param_dtype=torch.float32):
    """obs_dim / act_dim: the env's observation and action widths -- the tabletop's 12 / 3 by default, 20 / 3 for the three-object tabletop, 14 / 4 for the Sawyer door and peg, 32 / 8 for the minitaur, 46 / 9 for the kitchen (`env.rollout_policy`).
    param_dtype: the format the parameters are STORED in.  torch.bfloat16 (the door, the peg, the minitaur and the kitchen; earl_mlp_policy.precision =
    EARL_PRECISION_BF16) rounds every parameter ONCE, with torch's round-to-nearest-even; `.params` is then the bf16 tensor the kernel reads (writable in place), and
    `.layers` hold the widened float32 values, so pi(obs), pi.sample and make_step_graph(T, policy=pi) evaluate the network the kernel evaluates: bf16 is a storage
    format, the arithmetic is float32 on the widened values, and a launch returns the bits of the float32 launch of pi.widened()."""
    name = type(self).__name__                                        # (MLPPolicy's own messages read as they always did)
    param_dtype = _param_dtype(name, param_dtype)
    self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
    if self.obs_dim < 1 or self.act_dim < 1:
      raise ValueError(f'{name}: obs_dim = {obs_dim}, act_dim = {act_dim}: both >= 1')
    out_dim = self.act_dim * (self.OUT_DIM // ACT_DIM)                  # (the Gaussian head: twice the action width)
    what = 'tabletop observation' if self.obs_dim == OBS_DIM else 'observation'
    if isinstance(layers, torch.nn.Sequential):
      layers, hidden_act, out_act = _layers_of_sequential(layers)
    layers = [(torch.as_tensor(np.asarray(w) if not torch.is_tensor(w) else w).detach().to('cpu', torch.float32),
               torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).detach().to('cpu', torch.float32)) for w, b in layers]
    if len(layers) not in (2, 3):
      raise ValueError(f'{name}: {len(layers) - 1} hidden layers; the fused kernel takes one or two')
    if hidden_act not in ('relu', 'tanh'):
      raise ValueError(f"{name}: hidden_act must be 'relu' or 'tanh', got {hidden_act!r}")
    if out_act not in ('none', 'tanh', None):
      raise ValueError(f"{name}: out_act must be 'none' or 'tanh', got {out_act!r}")
    dims = [int(layers[0][0].shape[1])]
    for l, (w, b) in enumerate(layers):
      if w.dim() != 2 or b.dim() != 1 or w.shape[1] != dims[-1] or b.shape[0] != w.shape[0]:
        raise ValueError(f'{name}: layer {l} has weight {tuple(w.shape)} and bias {tuple(b.shape)} after width {dims[-1]}')
      dims.append(int(w.shape[0]))
    if dims[0] != self.obs_dim:
      raise ValueError(f'{name}: the input is the {self.obs_dim}-wide {what}, got width {dims[0]}')
    if dims[-1] != out_dim:
      raise ValueError(f'{name}: the output is the {out_dim}-wide {self.OUT_WHAT}, got width {dims[-1]}')
    for h in dims[1:-1]:
      if h < MIN_WIDTH or h > MAX_WIDTH or h % 16:
        raise ValueError(f'{name}: hidden width {h}: a multiple of 16 in {MIN_WIDTH}..{MAX_WIDTH}')
    self._describe(dims, hidden_act, out_act or 'none', isinstance(self, GaussianMLPPolicy), param_dtype)
    if param_dtype != torch.float32:                                  # rounded once; from here on the float32 values ARE the stored ones, widened
      layers = [(w.to(param_dtype).to(torch.float32), b.to(param_dtype).to(torch.float32)) for w, b in layers]
    self._host_layers = layers
    self.to(device)

  def _place(self):
    self.layers = [(w.to(self.device).contiguous(), b.to(self.device).contiguous()) for w, b in self._host_layers]
    self.params = torch.cat([t.reshape(-1) for wb in self.layers for t in wb]).to(self.param_dtype).contiguous()      # W0, b0, W1, b1, ...  (bf16: exact, the values are widened bf16)

  def with_param_dtype(self, dtype):
    """the policy of the values that stand in `.params` now, stored as `dtype` (torch.float32 | torch.bfloat16: rounded once), on the same device"""
    return _like(self, self.params, self.device, _param_dtype(type(self).__name__, dtype), self.obs_dim, self.act_dim)

  def widened(self):
    """the float32 policy with exactly the stored values: the network a launch with this policy evaluates, bit for bit (and what the tabletop takes)"""
    return self.with_param_dtype(torch.float32)

  def __call__(self, obs):
    x, _ = _forward(obs, self.layers, self.hidden_act, self.act_dim)
    return torch.tanh(x) if self.out_act == 'tanh' else x


class GaussianMLPPolicy(MLPPolicy):
  """The tanh-Gaussian actor: `layers` (or a torch.nn.Sequential ending in Linear(H, 6) without activation) packed like MLPPolicy's.  squash=True applies
  tanh to u = mean + exp(log_std) eps (SAC); squash=False leaves the clip to the env.  log_std_map: 'tanh' -> lo + 0.5 (hi - lo) (tanh(raw) + 1) (the
  pytorch_sac / DrQ actor), 'clamp' -> min(max(raw, lo), hi), with (lo, hi) = log_std_bounds inside [-20, 4].
  pi(obs) is the MEAN action (what evaluation uses, and what make_step_graph(T, policy=pi) captures); pi.sample(obs, eps) the sampled action for given
  standard-normal eps -- torch's statement of csrc/tabletop_policy.h's contract, close to but not bit-identical with the kernel."""
  OUT_DIM, OUT_WHAT = 2 * ACT_DIM, 'mean and raw log_std of the action'

  def __init__(self, layers, hidden_act='relu', squash=True, log_std_bounds=(-5.0, 2.0), log_std_map='tanh', device='cpu', obs_dim=OBS_DIM, act_dim=ACT_DIM,
               param_dtype=torch.float32):
    if isinstance(layers, torch.nn.Sequential):
      layers, hidden_act, last = _layers_of_sequential(layers)
      if last != 'none':
        raise ValueError('GaussianMLPPolicy: no activation after the last Linear (squash=True is the tanh of the sampled action)')
    if log_std_map not in _abi.LOGSTD_MAPS:
      raise ValueError(f"GaussianMLPPolicy: log_std_map must be 'tanh' or 'clamp', got {log_std_map!r}")
    lo, hi = (float(np.float32(v)) for v in log_std_bounds)
    if not (-20.0 <= lo <= hi <= 4.0):                       # (NaN fails the chain)
      raise ValueError(f'GaussianMLPPolicy: log_std_bounds {tuple(log_std_bounds)}: finite, min <= max, inside [-20, 4]')
    self.squash, self.log_std_bounds, self.log_std_map = bool(squash), (lo, hi), log_std_map
    super().__init__(layers, hidden_act, 'tanh' if squash else 'none', device, obs_dim=obs_dim, act_dim=act_dim, param_dtype=param_dtype)

  def head(self, sample=True, eps_out=None):
    """struct earl_gaussian_head for one launch; eps_out: a float32 tensor [E, T, N, act_dim] on the policy's device, or None"""
    return _abi.GaussianHead(mode=_abi.HEAD_SAMPLE if sample else _abi.HEAD_MEAN, log_std_map=_abi.LOGSTD_MAPS[self.log_std_map],
                             log_std_min=self.log_std_bounds[0], log_std_max=self.log_std_bounds[1],
                             eps_out=None if eps_out is None else eps_out.data_ptr())

  def _mean_and_log_std(self, obs):
    mean, x = _forward(obs, self.layers, self.hidden_act, self.act_dim)
    raw = x[..., self.act_dim:]
    lo, hi = self.log_std_bounds
    log_std = lo + 0.5 * (hi - lo) * (torch.tanh(raw) + 1.0) if self.log_std_map == 'tanh' else torch.clamp(raw, lo, hi)
    return mean, log_std

  def __call__(self, obs):
    mean, _ = self._mean_and_log_std(obs)
    return torch.tanh(mean) if self.squash else mean

  def sample(self, obs, eps):
    mean, log_std = self._mean_and_log_std(obs)
    u = mean + torch.exp(log_std) * torch.as_tensor(eps, dtype=torch.float32, device=mean.device)
    return torch.tanh(u) if self.squash else u


GOAL_DIMS = {(OBS_DIM, ACT_DIM): 6, (20, ACT_DIM): 10, (14, 4): 7, (32, 8): 2, (46, 9): 23}      # width of an AgentPair's backward goal by the agents' widths
PAIR_POPULATION_WIDTHS = ((14, 4), (32, 8), (46, 9))                          # the envs whose pair launch takes a population of pairs


def require_widths(policy, who, obs_dim, act_dim, env=None, pair=False, bounded=None, pairs=False):
  """The one check of a policy against the widths it is to have -> is it Gaussian.  env=None: a container of declared widths (the tabletop's 12 -> .. -> 3 unless
  said otherwise) takes networks of those widths only.  env given (its `device`, `num_envs`, `_cfg.env_offset`): a launch of `who` on that env -- the type (an
  MLPPolicy, a GaussianMLPPolicy or a PolicyPopulation of them; pair=True: an AgentPair, with pairs=True also a PairPopulation), the env's widths, the env's device,
  and a population's members against the env's global ids.  bounded: None, or the bound outside which the env's reference raises on an action (the minitaur): an unbounded output is refused."""
  if env is not None and pair and isinstance(policy, PairPopulation) and not pairs:
    raise ValueError(f'{who}: a PairPopulation runs on the Sawyer door and peg only (earl_sawyer_agents_rollout); this env takes ONE AgentPair')
  if env is not None and not isinstance(policy, (AgentPair, PairPopulation) if pair else (MLPPolicy, PolicyPopulation)):
    raise ValueError(f'{who}: ' + (('pair is an AgentPair' + (' or a PairPopulation' if pairs else '')) if pair else
                                   'an MLPPolicy, a GaussianMLPPolicy or a PolicyPopulation of them (an AgentPair goes to rollout_agents)'))
  what, ctor = ('an AgentPair', 'AgentPair') if pair else ('a policy', 'MLPPolicy')
  od, ad = getattr(policy, 'obs_dim', OBS_DIM), getattr(policy, 'act_dim', ACT_DIM)
  if (od, ad) != (obs_dim, act_dim):
    takes = (f'the tabletop takes {OBS_DIM} and {ACT_DIM}' if (obs_dim, act_dim) == (OBS_DIM, ACT_DIM) else
             f'{obs_dim} and {act_dim} were declared' if env is None else f'this env takes {obs_dim} and {act_dim} ({ctor}(..., obs_dim={obs_dim}, act_dim={act_dim}))')
    raise ValueError(f'{who}: {what} of observation width {od} and action width {ad}; {takes}')
  gaussian = policy.gaussian if isinstance(policy, (PolicyPopulation, AgentPair, PairPopulation)) else isinstance(policy, GaussianMLPPolicy)
  if env is None:
    return gaussian
  if (obs_dim, act_dim) in TABLETOP_WIDTHS and getattr(policy, 'param_dtype', torch.float32) != torch.float32:
    raise ValueError(f'{who}: the parameters are stored as {policy.param_dtype}; the tabletop holds its weights in registers for the whole launch and takes float32 '
                     'only: pass .widened(), the float32 policy of exactly these values')
  if policy.device != env.device:
    noun = 'pair' if pair else 'policy'
    raise ValueError(f'{who}: the {noun} is on {policy.device}, the env on {env.device} ({noun}.to(device))')
  if isinstance(policy, (PolicyPopulation, PairPopulation)):
    lo, hi = int(env._cfg.env_offset), int(env._cfg.env_offset) + env.num_envs - 1
    if lo < 0 or hi // policy.envs_per_policy >= policy.n_policies:
      raise ValueError(f'{who}: global env ids {lo} .. {hi} need members up to {hi // policy.envs_per_policy} of {policy.n_policies}')
  if bounded is not None and policy.out_act != 'tanh':
    given = 'GaussianMLPPolicy(..., squash=False)' if gaussian else f'MLPPolicy(..., out_act={policy.out_act!r})'
    raise ValueError(f'{who}: {given} is unbounded; the reference env raises on an action outside +-{bounded} and a kernel cannot, so this env takes bounded '
                     "policies only: MLPPolicy(..., out_act='tanh') or GaussianMLPPolicy(..., squash=True)")
  return gaussian


class PolicyPopulation(_PackedMLP):
  """P members of one architecture behind struct earl_policy_population: `policies` is a list of MLPPolicy or of GaussianMLPPolicy (same dims, activations and,
  for the Gaussian head, squash / bounds / map -- only the parameters differ), or ONE template policy with `params` [P, n_params] (n_params <= the row length:
  a wider row is the stride).  The env with GLOBAL id g runs member g // envs_per_policy (a multiple of 16: a member owns whole 16-env workgroups of the kernel).
  `.params` [P, stride] float32 (bf16 if the members store bf16: `param_dtype` is theirs, and a mixed list is refused) holds every member in MLPPolicy's packing order (W0, b0, W1, b1, ...) and is what the kernel reads: write into it in place.
  obs_dim / act_dim: the members' widths -- the tabletop's 12 / 3 by default, as MLPPolicy's; 14 / 4 for the Sawyer door and peg (earl_sawyer_population_rollout,
  whose rows are then padded to a stride of whole 16-byte pieces: 4 float32 or 8 bf16 elements -- the stride counts elements of the stored type)."""

  def __init__(self, policies, envs_per_policy=16, device=None, params=None, obs_dim=OBS_DIM, act_dim=ACT_DIM):
    self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
    G = int(envs_per_policy)
    if G < 16 or G % 16:
      raise ValueError(f'PolicyPopulation: envs_per_policy = {envs_per_policy}: a multiple of 16, >= 16')
    if isinstance(policies, MLPPolicy):
      if params is None:
        raise ValueError('PolicyPopulation: a template policy needs params [P, n_params]')
      template, members = policies, None
      require_widths(template, 'PolicyPopulation', self.obs_dim, self.act_dim)
    else:
      members = list(policies)
      if not members or not all(isinstance(m, MLPPolicy) for m in members):
        raise ValueError('PolicyPopulation: a non-empty list of MLPPolicy / GaussianMLPPolicy, or one template policy with params=')
      if params is not None:
        raise ValueError('PolicyPopulation: params= goes with ONE template policy, not with a list')
      template = members[0]
      for m in members:
        require_widths(m, 'PolicyPopulation', self.obs_dim, self.act_dim)
      _require_shared('PolicyPopulation', members, self.SHARED + (self.SHARED_HEAD if template.gaussian else ()), 'the members of a population share one architecture')
    self.template, self.envs_per_policy = template, G
    self._describe_like(template)
    if members is not None:
      host = torch.stack([m.params.detach().to('cpu', self.param_dtype) for m in members])
    else:
      given = params.dtype if torch.is_tensor(params) else None
      if torch.bfloat16 in (given, self.param_dtype) and given != self.param_dtype:
        raise ValueError(f'PolicyPopulation: params is {given or type(params).__name__}, the template policy stores {self.param_dtype} '
                         '(template.with_param_dtype(...), or params.to(...): the rows are read as they are)')
      host = torch.as_tensor(params).detach().to('cpu', self.param_dtype)
      if host.dim() != 2 or host.shape[0] < 1 or host.shape[1] < self.n_params:
        raise ValueError(f'PolicyPopulation: params {tuple(host.shape)}: [P, >= {self.n_params}] (one row per member, packed like MLPPolicy.params)')
    self.n_policies = int(host.shape[0])
    piece = _piece(self.param_dtype, (self.obs_dim, self.act_dim) in TABLETOP_WIDTHS)      # (the stepper kernels read every member's rows in 16-byte pieces)
    self.params = _padded(host, piece).clone().contiguous()
    self.to(template.device if device is None else device)

  @property
  def stride(self):
    return int(self.params.shape[1])

  def _place(self):
    super()._place()
    self.pop_struct = self._population()

  def widened(self):
    """the float32 population of exactly the stored values (MLPPolicy.widened)"""
    return PolicyPopulation(self.template.widened(), self.envs_per_policy, device=self.device, params=self.params.detach().to('cpu', torch.float32),
                            obs_dim=self.obs_dim, act_dim=self.act_dim)

  def head(self, sample=True, eps_out=None):
    return self.template.head(sample=sample, eps_out=eps_out)

  def member(self, p):
    """member p as a policy of its own (a copy of its row of .params, stored in the population's param_dtype)"""
    return _like(self.template, self.params[int(p)], self.device, self.param_dtype, self.obs_dim, self.act_dim)

  def policy_index(self, global_ids):
    """the member each GLOBAL env id runs"""
    g = torch.as_tensor(global_ids)
    return torch.div(g, self.envs_per_policy, rounding_mode='floor')

  def __call__(self, obs, env_offset=0):
    """obs [..., N, obs_dim] of the envs with global ids env_offset .. env_offset + N - 1 -> actions [..., N, act_dim] (a Gaussian population: at the mean), every env
    through its own member: one batched matmul per layer over the members present (torch's summation order: close to the kernel, not bit-identical)"""
    x = obs.to(torch.float32)
    lead, N, G = x.shape[:-2], int(x.shape[-2]), self.envs_per_policy
    m0, m1 = int(env_offset) // G, (int(env_offset) + N - 1) // G
    if env_offset < 0 or m1 >= self.n_policies:
      raise ValueError(f'PolicyPopulation: global env ids {env_offset} .. {env_offset + N - 1} need members {m0} .. {m1} of {self.n_policies}')
    M = m1 - m0 + 1
    slot = torch.arange(N, device=x.device) + (int(env_offset) - m0 * G)            # where the env sits in the members' [M, G] grid
    x = x.reshape(-1, N, x.shape[-1])
    L = x.shape[0]
    grid = x.new_zeros(L, M * G, x.shape[-1])
    grid[:, slot] = x
    h = grid.reshape(L, M, G, -1).permute(1, 0, 2, 3).reshape(M, L * G, -1)
    layers = _unpack(self.params[m0:m1 + 1].to(x.device, torch.float32), self.dims)     # (bf16 rows: widened first)
    for l, (w, b) in enumerate(layers):
      h = torch.baddbmm(b[:, None, :], h, w.transpose(1, 2))
      if l + 1 < len(layers):
        h = torch.relu(h) if self.hidden_act == 'relu' else torch.tanh(h)
    A = self.act_dim
    h = h[..., :A]
    if self.out_act == 'tanh':
      h = torch.tanh(h)
    out = h.reshape(M, L, G, A).permute(1, 0, 2, 3).reshape(L, M * G, A)[:, slot]
    return out.reshape(*lead, N, A)


class AgentPair(_PackedMLP):
  """The forward and the reset (backward) agent behind struct earl_agent_pair: both `MLPPolicy`, or both `GaussianMLPPolicy`, of one architecture (dims, activations
  and, for the Gaussian head, squash / bounds / map -- only the parameters differ).  `.params` [2, stride] float32 holds row 0 = forward, row 1 = reset in MLPPolicy's
  packing order and is what the kernel reads: write into it in place.  switch_every: steps after which the acting agent hands over, one int for both or (forward,
  reset); switch_on_success: also hand over after a step whose success flag is set; backward_goal: the goal row the reset agent is conditioned on -- 'initial' (the
  env's initial state, resolved by the env at launch), None (the reset agent keeps seeing the task goal) or a 6-vector in goal-table format.
  A second hidden layer may be at most 128 wide (EARL_PAIR_MAX_H2: two weight sets share one wave's registers); one hidden layer may have every width.
  obs_dim / act_dim: the agents' widths -- the tabletop's 12 / 3 by default; 20 / 3 for the three-object tabletop (earl_tabletop3_pair_rollout: the same rules with a
  goal row of 10 values, 'initial' = [0, 0, 2.5, 0, 2.5, -1, 2.5, 1, -1, -1]); 14 / 4 for the Sawyer door and peg (earl_sawyer_pair_rollout), where the backward goal is
  a row of 7 values in the Sawyer goal format, the rows are padded to a stride of whole 16-byte pieces as PolicyPopulation's, and no width limit applies (the weights
  are read from memory at every step).  There backward_goal may also be a TABLE [R, 7], R >= 2 (kept as `.backward_goals`; `.backward_goal` is then None), or
  'initial_states' (the env's `initial_states`, resolved at launch: the peg's fifteen rows, the door's one, which behaves as 'initial'): at every entry into the
  reset phase the env's goal is a row of the table drawn from the env's counter-based RNG (earl_sawyer_agents_rollout; `env.backward_row`).
  32 / 8 is the minitaur and 46 / 9 the kitchen (earl_minitaur_agents_rollout, earl_kitchen_agents_rollout; `env.rollout_pair`): the same rules with a goal row of 2
  values (x, y; 'initial' is the reset pose's) and of 23 (a qpos; 'initial_states' is the table of `get_init_states()`, 'initial' its one row where there is one)."""

  def __init__(self, forward, backward, switch_every=200, switch_on_success=True, backward_goal='initial', device=None, obs_dim=OBS_DIM, act_dim=ACT_DIM):
    self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
    tabletop = (self.obs_dim, self.act_dim) in TABLETOP_WIDTHS        # (12 / 3, and the three-object env's 20 / 3: earl_tabletop3_pair_rollout)
    self.goal_dim = GOAL_DIMS.get((self.obs_dim, self.act_dim), 7)      # the env's goal row: 6 tabletop (three objects: 10), 7 Sawyer door / peg, 2 minitaur (x, y), 23 kitchen (a qpos)
    members = [forward, backward]
    if not all(isinstance(m, MLPPolicy) for m in members):
      raise ValueError('AgentPair: forward and backward are MLPPolicy / GaussianMLPPolicy')
    for m in members:
      require_widths(m, 'AgentPair', self.obs_dim, self.act_dim)
    template = forward
    _require_shared('AgentPair', members, self.SHARED + (self.SHARED_HEAD if template.gaussian else ()), 'the two agents of a pair share one architecture')
    if tabletop and len(template.dims) == 4 and template.dims[2] > _abi.PAIR_MAX_H2:
      raise ValueError(f'AgentPair: second hidden width {template.dims[2]} > {_abi.PAIR_MAX_H2} (EARL_PAIR_MAX_H2: two weight sets share one wave\'s registers)')
    se = (switch_every, switch_every) if np.ndim(switch_every) == 0 else tuple(switch_every)
    if len(se) != 2 or any(int(v) != v or int(v) < 1 for v in se):
      raise ValueError(f'AgentPair: switch_every = {switch_every!r}: one int >= 1, or (forward, reset)')
    self.switch_every, self.switch_on_success = (int(se[0]), int(se[1])), bool(switch_on_success)
    self.backward_goals = None                           # Sawyer widths: a TABLE of goal rows [R, 7], R >= 2 (the reset agent's goal is drawn from it at every handover)
    table = None
    if not tabletop and not isinstance(backward_goal, str) and backward_goal is not None:
      table = backward_goal.detach().cpu().numpy() if torch.is_tensor(backward_goal) else np.asarray(backward_goal)
      table = table if table.ndim == 2 and table.shape[0] >= 2 and table.shape[1] == self.goal_dim else None
    if backward_goal is None or (isinstance(backward_goal, str) and (backward_goal == 'initial' or (backward_goal == 'initial_states' and not tabletop))):
      self.backward_goal = backward_goal
    elif table is not None:
      self.backward_goal = None
      self.backward_goals = torch.as_tensor(np.ascontiguousarray(table, dtype=np.float64)).clone()
    else:
      g = torch.as_tensor(np.asarray(backward_goal, dtype=np.float64) if not torch.is_tensor(backward_goal) else backward_goal).detach().to('cpu', torch.float64).reshape(-1)
      if g.numel() != self.goal_dim:
        raise ValueError(f"AgentPair: backward_goal is 'initial', None or ONE goal row of {self.goal_dim} values, got {g.numel()}")
      self.backward_goal = g.clone()
    self.template = template
    self._describe_like(template)
    host = torch.stack([m.params.detach().to('cpu', self.param_dtype) for m in members])
    self.params = _padded(host, _piece(self.param_dtype, tabletop)).contiguous()      # (the stepper kernels read both agents' rows in 16-byte pieces)
    self.to(template.device if device is None else device)

  @property
  def stride(self):
    return int(self.params.shape[1])

  pair_stride = stride                                               # (floats between the two agents' rows: PairPopulation's name for it)

  def _place(self):
    super()._place()
    dev = self.device
    self._goal_dev = None if not torch.is_tensor(self.backward_goal) else self.backward_goal.to(dev).contiguous()
    self._initial_dev = None                                         # ('initial' as numpy, its row on `dev`), filled by goal_row
    self._goals_dev = None if self.backward_goals is None else self.backward_goals.to(dev).contiguous()
    self._initial_states_dev = None                                  # ('initial_states' as numpy, its rows on `dev`), filled by goal_table

  def with_param_dtype(self, dtype):
    """the pair of the values that stand in `.params` now, its agents stored as `dtype` (MLPPolicy.with_param_dtype)"""
    goal = self.backward_goals if self.backward_goals is not None else self.backward_goal
    return AgentPair(self.agent(0).with_param_dtype(dtype), self.agent(1).with_param_dtype(dtype), switch_every=self.switch_every,
                     switch_on_success=self.switch_on_success, backward_goal=goal, device=self.device, obs_dim=self.obs_dim, act_dim=self.act_dim)

  def widened(self):
    """the float32 pair of exactly the stored values (MLPPolicy.widened)"""
    return self.with_param_dtype(torch.float32)

  def head(self, sample=True, eps_out=None):
    return self.template.head(sample=sample, eps_out=eps_out)

  def goal_table(self, env):
    """the reset agent's TABLE of goal rows as a float64 tensor [R, 7], R >= 2, on the pair's device, or None (then goal_row is the rule): a table given as
    backward_goal, or 'initial_states' on an env whose `initial_states` has more than one row (the peg's fifteen; the door's single row behaves as 'initial')"""
    if self._goals_dev is not None:
      return self._goals_dev
    if not (isinstance(self.backward_goal, str) and self.backward_goal == 'initial_states'):
      return None
    rows = np.asarray(env.initial_states, dtype=np.float64).reshape(-1, self.goal_dim)
    if len(rows) < 2:
      return None
    if self._initial_states_dev is None or not np.array_equal(self._initial_states_dev[0], rows):      # one upload per (pair, device, table), not one per launch
      self._initial_states_dev = (rows.copy(), torch.as_tensor(rows, device=self.device).contiguous())
    return self._initial_states_dev[1]

  def goal_row(self, env):
    """the reset agent's goal row as a float64 tensor [6] (three-object tabletop: [10]; Sawyer widths: [7]) on the pair's device, or None; 'initial' is `env.initial_state` (the Sawyer door: the one
    row of `env.initial_states`; the peg has fifteen, so the caller picks one -- or asks for 'initial_states', the whole table: goal_table)"""
    if self.backward_goal is None:
      return None
    if self._goal_dev is not None:
      return self._goal_dev
    if (self.obs_dim, self.act_dim) not in TABLETOP_WIDTHS:
      rows = np.asarray(env.initial_states, dtype=np.float64).reshape(-1, self.goal_dim)
      if len(rows) != 1:
        raise ValueError(f"AgentPair: backward_goal='initial' needs ONE initial state and env.initial_states has {len(rows)} rows: pass the row to condition the "
                         'reset agent on (backward_goal=env.initial_states[k])')
      init = rows[0]
    else:
      init = np.asarray(env.initial_state, dtype=np.float64).reshape(-1)
    if self._initial_dev is None or not np.array_equal(self._initial_dev[0], init):      # one upload per (pair, device, initial state), not one per launch
      self._initial_dev = (init.copy(), torch.as_tensor(init, device=self.device).contiguous())
    return self._initial_dev[1]

  def agent(self, k):
    """agent k (0 forward, 1 reset) as a policy of its own (a copy of its row of .params, stored in the pair's param_dtype)"""
    return _like(self.template, self.params[int(k)], self.device, self.param_dtype, self.obs_dim, self.act_dim)

  def __call__(self, obs, phase):
    """obs [..., N, obs_dim], phase [N] or [..., N] (0 forward, 1 reset) -> actions [..., N, act_dim] (Gaussian agents: at the mean): torch's statement -- close to the kernel,
    not bit-identical"""
    ph = torch.as_tensor(phase, device=obs.device).bool()
    acts = []
    for row in self.params.detach().to(obs.device, torch.float32):   # the layers are views of .params: no copy, and in-place updates are seen (bf16 rows: widened first)
      x, _ = _forward(obs.to(torch.float32).reshape(-1, obs.shape[-1]), _unpack(row, self.dims), self.hidden_act, self.act_dim)      # (Gaussian agents: the mean)
      acts.append((torch.tanh(x) if self.out_act == 'tanh' else x).reshape(*obs.shape[:-1], self.act_dim))
    return torch.where(ph[..., None], acts[1], acts[0])


class PairPopulation(_PackedMLP):
  """P forward / reset pairs of ONE architecture, head, switch rule and backward goal behind struct earl_policy_population next to struct earl_agent_pair
  (earl_sawyer_agents_rollout, earl_minitaur_agents_rollout, earl_kitchen_agents_rollout): `pairs` is a list of `AgentPair` of one env's widths (obs_dim=14,
  act_dim=4 on the Sawyer door and peg; 32 / 8 on the minitaur; 46 / 9 on the kitchen) -- only the parameters differ.  The env with GLOBAL id g runs pair
  g // envs_per_policy (a multiple of 16).  `.params` [P, 2, stride] float32 holds every pair's rows (0 forward, 1 reset) in MLPPolicy's packing order and is what the
  kernel reads: write into it in place."""
  SHARED = ('gaussian', 'dims', 'hidden_act', 'out_act', 'param_dtype', 'switch_every', 'switch_on_success')

  def __init__(self, pairs, envs_per_policy=16, device=None):
    G = int(envs_per_policy)
    if G < 16 or G % 16:
      raise ValueError(f'PairPopulation: envs_per_policy = {envs_per_policy}: a multiple of 16, >= 16')
    members = list(pairs)
    if not members or not all(isinstance(m, AgentPair) for m in members):
      raise ValueError('PairPopulation: a non-empty list of AgentPair')
    t = members[0]
    self.obs_dim, self.act_dim = t.obs_dim, t.act_dim
    widths = (t.obs_dim, t.act_dim) if (t.obs_dim, t.act_dim) in PAIR_POPULATION_WIDTHS else (14, 4)
    for m in members:
      require_widths(m, 'PairPopulation', *widths)
    clause = 'the pairs of a population share one architecture, head, switch rule and backward goal'
    _require_shared('PairPopulation', members, self.SHARED + (tuple('template.' + a for a in self.SHARED_HEAD) if t.gaussian else ()), clause)
    for p, m in enumerate(members):
      if not self._same_goal(m, t):
        shown = lambda a: a.backward_goals if a.backward_goals is not None else a.backward_goal
        raise ValueError(f'PairPopulation: member {p} has backward_goal = {shown(m)!r}, member 0 has {shown(t)!r} ({clause})')
    self.envs_per_policy, self.n_policies = G, len(members)
    self._describe_like(t)
    self.switch_every, self.switch_on_success = t.switch_every, t.switch_on_success
    self.backward_goal, self.backward_goals = t.backward_goal, t.backward_goals
    self._head_of = t.template                                        # (a policy of the members' head: only its head settings are used)
    self.params = torch.stack([m.params.detach().to('cpu', self.param_dtype) for m in members]).contiguous()      # [P, 2, stride]
    self.to(t.device if device is None else device)

  @staticmethod
  def _same_goal(a, b):
    ga, gb = (a.backward_goals, a.backward_goal), (b.backward_goals, b.backward_goal)
    for x, y in zip(ga, gb):
      if torch.is_tensor(x) or torch.is_tensor(y):
        if not (torch.is_tensor(x) and torch.is_tensor(y) and x.shape == y.shape and bool((x == y).all())):
          return False
      elif x != y:
        return False
    return True

  @property
  def pair_stride(self):
    """floats between the two agents' rows of one pair"""
    return int(self.params.shape[2])

  @property
  def stride(self):
    """floats between two pairs"""
    return 2 * self.pair_stride

  def _place(self):
    super()._place()
    self.pop_struct = self._population()
    self._goals = self.pair(0)                                         # resolves and caches the backward goal on the device (goal_row / goal_table)

  def head(self, sample=True, eps_out=None):
    return self._head_of.head(sample=sample, eps_out=eps_out)

  def goal_row(self, env):
    return self._goals.goal_row(env)

  def goal_table(self, env):
    return self._goals.goal_table(env)

  def pair(self, p):
    """pair p as an AgentPair of its own (a copy of its rows of .params)"""
    agents = [_like(self._head_of, row, 'cpu', self.param_dtype, self.obs_dim, self.act_dim) for row in self.params[int(p)]]
    goal = self.backward_goals if self.backward_goals is not None else self.backward_goal
    return AgentPair(agents[0], agents[1], switch_every=self.switch_every, switch_on_success=self.switch_on_success, backward_goal=goal, device=self.device,
                     obs_dim=self.obs_dim, act_dim=self.act_dim)

  def widened(self):
    """the float32 pairs of exactly the stored values (MLPPolicy.widened)"""
    return PairPopulation([self.pair(p).widened() for p in range(self.n_policies)], self.envs_per_policy, device=self.device)

  def policy_index(self, global_ids):
    """the pair each GLOBAL env id runs"""
    return torch.div(torch.as_tensor(global_ids), self.envs_per_policy, rounding_mode='floor')

"""A float32 MLP policy 12 -> hidden (-> hidden) -> 3 in the form the fused closed-loop rollout takes (include/earl_tabletop.h: struct
earl_mlp_policy, earl_tabletop_policy_rollout): the parameters packed once, layer by layer (W_l row-major like torch.nn.Linear.weight, then b_l).

  pi = MLPPolicy([(w0, b0), (w1, b1)], hidden_act='relu', out_act='tanh', device='cuda')      # or MLPPolicy(torch.nn.Sequential(...))
  obs, reward, done, success, actions = env.rollout_policy(pi, T=200, episodes=4)               # ONE launch: reset + T closed-loop steps, x 4
  g = env.make_step_graph(T, policy=pi)                                                         # the same network as torch ops between captured steps

`pi(obs)` evaluates the same network with torch (matmul order is torch's: close to, not bit-identical with, the fused kernel, whose arithmetic is the
k-ascending fmaf chain that csrc/tabletop_policy.h states).

`GaussianMLPPolicy` is the SAC-style actor with a tanh-Gaussian head, 12 -> hidden (-> hidden) -> 6 (rows 0..2 mean, rows 3..5 raw log_std), for
earl_tabletop_policy_rollout_gaussian: the actions are SAMPLED inside the kernel from the env's counter-based RNG.

  pi = GaussianMLPPolicy(actor_trunk, squash=True, log_std_bounds=(-5.0, 2.0), log_std_map='tanh', device='cuda')
  obs, reward, done, success, actions = env.rollout_policy(pi, T=200, episodes=4)                     # exploration: tanh(mean + exp(log_std) eps)
  obs, reward, done, success, actions, eps = env.rollout_policy(pi, T=200, return_noise=True)         # ... and the standard-normal draws as used
  obs, reward, done, success, actions = env.rollout_policy(pi, T=200, episodes=4, sample=False)       # evaluation at the mean, same packed network"""
import numpy as np
import torch

from . import _abi

OBS_DIM, ACT_DIM = 12, 3
MIN_WIDTH, MAX_WIDTH = 16, 256


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


class MLPPolicy:
  OUT_DIM, OUT_WHAT = ACT_DIM, 'action'

  def __init__(self, layers, hidden_act='relu', out_act='tanh', device='cpu'):
    name = type(self).__name__                                        # (MLPPolicy's own messages read as they always did)
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
    if dims[0] != OBS_DIM:
      raise ValueError(f'{name}: the input is the {OBS_DIM}-wide tabletop observation, got width {dims[0]}')
    if dims[-1] != self.OUT_DIM:
      raise ValueError(f'{name}: the output is the {self.OUT_DIM}-wide {self.OUT_WHAT}, got width {dims[-1]}')
    for h in dims[1:-1]:
      if h < MIN_WIDTH or h > MAX_WIDTH or h % 16:
        raise ValueError(f'{name}: hidden width {h}: a multiple of 16 in {MIN_WIDTH}..{MAX_WIDTH}')
    self.dims, self.hidden_act, self.out_act = dims, hidden_act, out_act or 'none'
    self._host_layers = layers
    self.macs = sum(a * b for a, b in zip(dims[:-1], dims[1:]))       # multiply-adds per env step
    self.to(device)

  def to(self, device):
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    self.device = dev
    self.layers = [(w.to(dev).contiguous(), b.to(dev).contiguous()) for w, b in self._host_layers]
    self.params = torch.cat([t.reshape(-1) for wb in self.layers for t in wb]).contiguous()      # W0, b0, W1, b1, ...
    dims = self.dims + [0] * (4 - len(self.dims))
    self.struct = _abi.MlpPolicy(n_layers=len(self.layers), dims=(_abi.C.c_int32 * 4)(*dims), hidden_act=_abi.ACTIVATIONS[self.hidden_act],
                                 out_act=_abi.ACTIVATIONS[self.out_act], precision=0, params=self.params.data_ptr())
    return self

  def __call__(self, obs):
    x = obs.to(torch.float32)
    for l, (w, b) in enumerate(self.layers):
      x = torch.addmm(b, x, w.t())
      kind = self.hidden_act if l + 1 < len(self.layers) else self.out_act
      x = torch.relu(x) if kind == 'relu' else torch.tanh(x) if kind == 'tanh' else x
    return x


class GaussianMLPPolicy(MLPPolicy):
  """The tanh-Gaussian actor: `layers` (or a torch.nn.Sequential ending in Linear(H, 6) without activation) packed like MLPPolicy's.  squash=True applies
  tanh to u = mean + exp(log_std) eps (SAC); squash=False leaves the clip to the env.  log_std_map: 'tanh' -> lo + 0.5 (hi - lo) (tanh(raw) + 1) (the
  pytorch_sac / DrQ actor), 'clamp' -> min(max(raw, lo), hi), with (lo, hi) = log_std_bounds inside [-20, 4].
  pi(obs) is the MEAN action (what evaluation uses, and what make_step_graph(T, policy=pi) captures); pi.sample(obs, eps) the sampled action for given
  standard-normal eps -- torch's statement of csrc/tabletop_policy.h's contract, close to but not bit-identical with the kernel."""
  OUT_DIM, OUT_WHAT = 2 * ACT_DIM, 'mean and raw log_std of the action'

  def __init__(self, layers, hidden_act='relu', squash=True, log_std_bounds=(-5.0, 2.0), log_std_map='tanh', device='cpu'):
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
    super().__init__(layers, hidden_act, 'tanh' if squash else 'none', device)

  def head(self, sample=True, eps_out=None):
    """struct earl_gaussian_head for one launch; eps_out: a float32 tensor [E, T, N, 3] on the policy's device, or None"""
    return _abi.GaussianHead(mode=_abi.HEAD_SAMPLE if sample else _abi.HEAD_MEAN, log_std_map=_abi.LOGSTD_MAPS[self.log_std_map],
                             log_std_min=self.log_std_bounds[0], log_std_max=self.log_std_bounds[1],
                             eps_out=None if eps_out is None else eps_out.data_ptr())

  def _mean_and_log_std(self, obs):
    x = obs.to(torch.float32)
    for l, (w, b) in enumerate(self.layers):
      x = torch.addmm(b, x.reshape(-1, x.shape[-1]), w.t()).reshape(*x.shape[:-1], w.shape[0])
      if l + 1 < len(self.layers):
        x = torch.relu(x) if self.hidden_act == 'relu' else torch.tanh(x)
    mean, raw = x[..., :ACT_DIM], x[..., ACT_DIM:]
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

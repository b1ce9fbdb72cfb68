"""A float32 MLP policy 12 -> hidden (-> hidden) -> 3 in the form the fused closed-loop rollout takes (include/earl_tabletop.h: struct
earl_mlp_policy, earl_tabletop_policy_rollout): the parameters packed once, layer by layer (W_l row-major like torch.nn.Linear.weight, then b_l).

  pi = MLPPolicy([(w0, b0), (w1, b1)], hidden_act='relu', out_act='tanh', device='cuda')      # or MLPPolicy(torch.nn.Sequential(...))
  obs, reward, done, success, actions = env.rollout_policy(pi, T=200, episodes=4)               # ONE launch: reset + T closed-loop steps, x 4
  g = env.make_step_graph(T, policy=pi)                                                         # the same network as torch ops between captured steps

`pi(obs)` evaluates the same network with torch (matmul order is torch's: close to, not bit-identical with, the fused kernel, whose arithmetic is the
k-ascending fmaf chain that csrc/tabletop_policy.h states)."""
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
  def __init__(self, layers, hidden_act='relu', out_act='tanh', device='cpu'):
    if isinstance(layers, torch.nn.Sequential):
      layers, hidden_act, out_act = _layers_of_sequential(layers)
    layers = [(torch.as_tensor(np.asarray(w) if not torch.is_tensor(w) else w).detach().to('cpu', torch.float32),
               torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).detach().to('cpu', torch.float32)) for w, b in layers]
    if len(layers) not in (2, 3):
      raise ValueError(f'MLPPolicy: {len(layers) - 1} hidden layers; the fused kernel takes one or two')
    if hidden_act not in ('relu', 'tanh'):
      raise ValueError(f"MLPPolicy: hidden_act must be 'relu' or 'tanh', got {hidden_act!r}")
    if out_act not in ('none', 'tanh', None):
      raise ValueError(f"MLPPolicy: out_act must be 'none' or 'tanh', got {out_act!r}")
    dims = [int(layers[0][0].shape[1])]
    for l, (w, b) in enumerate(layers):
      if w.dim() != 2 or b.dim() != 1 or w.shape[1] != dims[-1] or b.shape[0] != w.shape[0]:
        raise ValueError(f'MLPPolicy: layer {l} has weight {tuple(w.shape)} and bias {tuple(b.shape)} after width {dims[-1]}')
      dims.append(int(w.shape[0]))
    if dims[0] != OBS_DIM:
      raise ValueError(f'MLPPolicy: the input is the {OBS_DIM}-wide tabletop observation, got width {dims[0]}')
    if dims[-1] != ACT_DIM:
      raise ValueError(f'MLPPolicy: the output is the {ACT_DIM}-wide action, got width {dims[-1]}')
    for h in dims[1:-1]:
      if h < MIN_WIDTH or h > MAX_WIDTH or h % 16:
        raise ValueError(f'MLPPolicy: hidden width {h}: a multiple of 16 in {MIN_WIDTH}..{MAX_WIDTH}')
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

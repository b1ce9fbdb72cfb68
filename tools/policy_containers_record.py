#!/usr/bin/env python3
"""What the four containers of earl_benchmark_amd/policy.py (MLPPolicy / GaussianMLPPolicy, PolicyPopulation, AgentPair, PairPopulation) ARE for a grid of
architectures, heads, widths and storage formats -- the bytes of `.params`, every struct field but the pointer, the scalars, what member() / agent() / pair() /
widened() / with_param_dtype() return -- and the full text of every refusal in the module, as one JSON file: tests/golden/policy_containers_parent.json, which
tests/test_policy_containers.py holds the module to.  Nothing needs a GPU; the weights come from integer arithmetic, so the bytes do not depend on the machine.
  python tools/policy_containers_record.py --policy /path/to/the/recorded/policy.py [--out tests/golden/policy_containers_parent.json]
--policy: the policy.py to record (the commit before a refactor), loaded in place of the package's own; it also asserts that every `raise` of that file was
reached by exactly one of the bad constructions below."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys
import traceback
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN = ((16,), (48, 80), (256, 256))
ACTS = ('relu', 'tanh')
HEADS = (None, (True, 'tanh'), (True, 'clamp'), (False, 'tanh'), (False, 'clamp'))      # None: MLPPolicy; else GaussianMLPPolicy (squash, log_std_map)
WIDTHS = ((12, 3), (14, 4), (32, 8), (46, 9))
DTYPES = ('float32', 'bfloat16')


def weights(torch, dims, seed):
  """[(W, b)] with packed element i = ((37 (i + 131 seed) + 11) % 997 - 498) / 1024: exact in float32, rounded by bfloat16"""
  n = sum(n * (k + 1) for k, n in zip(dims[:-1], dims[1:]))
  flat = ((37 * (torch.arange(n, dtype=torch.int64) + 131 * seed) + 11) % 997 - 498).to(torch.float32) / 1024
  layers, at = [], 0
  for k, n in zip(dims[:-1], dims[1:]):
    layers.append((flat[at:at + n * k].reshape(n, k).clone(), flat[at + n * k:at + n * k + n].clone()))
    at += n * k + n
  return layers


def make_policy(P, torch, hidden, act, head, widths, dtype, seed):
  O, A = widths
  dt = getattr(torch, dtype)
  if head is None:
    return P.MLPPolicy(weights(torch, [O, *hidden, A], seed), act, 'tanh', obs_dim=O, act_dim=A, param_dtype=dt)
  return P.GaussianMLPPolicy(weights(torch, [O, *hidden, 2 * A], seed), act, squash=head[0], log_std_bounds=(-4.0, 1.5), log_std_map=head[1], obs_dim=O, act_dim=A,
                             param_dtype=dt)


def make_goal(widths):
  """one backward-goal row of the widths' goal format (12 / 3: 'initial')"""
  dim = {(14, 4): 7, (32, 8): 2, (46, 9): 23}.get(widths)
  return 'initial' if dim is None else [0.125 * j - 0.5 for j in range(dim)]


def make_containers(P, torch, hidden, act, head, widths, dtype):
  """{name: a callable that builds the container}; a build may refuse (a tabletop pair with a wide second layer, a pair population of tabletop widths)"""
  O, A = widths
  mk = lambda seed: make_policy(P, torch, hidden, act, head, widths, dtype, seed)
  pair = lambda s: P.AgentPair(mk(s), mk(s + 1), switch_every=(5, 3), switch_on_success=True, backward_goal=make_goal(widths), obs_dim=O, act_dim=A)

  def rows():
    t = mk(0)
    theta = torch.stack([torch.nn.functional.pad(mk(s).params, (0, 3)) for s in (5, 6)])      # [2, n_params + 3]: a wider row is the stride
    return P.PolicyPopulation(t, envs_per_policy=32, params=theta, obs_dim=O, act_dim=A)
  return {'policy': lambda: mk(0), 'population': lambda: P.PolicyPopulation([mk(0), mk(1), mk(2)], envs_per_policy=16, obs_dim=O, act_dim=A), 'population_rows': rows,
          'pair': lambda: pair(3), 'pair_population': lambda: P.PairPopulation([pair(3), pair(7)], envs_per_policy=16)}


def sha(t):
  """the first 128 bits of the sha256 of a tensor's bytes"""
  return hashlib.sha256(t.detach().contiguous().view(__import__('torch').uint8).numpy().tobytes()).hexdigest()[:32]


def fields(s):
  """a struct's fields but the pointer, in their order"""
  return [(list(getattr(s, name)) if hasattr(getattr(s, name), '__len__') else getattr(s, name)) for name, _ in s._fields_ if name != 'params']


def describe(torch, c):
  """what the container is (of a policy's scalars the one it always had: macs)"""
  d = {'params': sha(c.params), 'shape': list(c.params.shape), 'dtype': str(c.params.dtype), 'struct': fields(c.struct)}
  for name in ('macs',) if hasattr(c, 'layers') else ('macs', 'n_params', 'gaussian', 'goal_dim', 'stride', 'pair_stride'):
    if hasattr(c, name):
      d[name] = getattr(c, name)
  if hasattr(c, 'pop_struct'):
    d['pop_struct'] = fields(c.pop_struct)
  if hasattr(c, 'layers'):
    d['layers'] = sha(torch.cat([t.reshape(-1) for wb in c.layers for t in wb]))
  other = torch.bfloat16 if c.param_dtype == torch.float32 else torch.float32
  for name, get in (('member', lambda: c.member(1)), ('agent', lambda: c.agent(1)), ('pair', lambda: c.pair(1)), ('widened', lambda: c.widened()),
                    ('with_param_dtype', lambda: c.with_param_dtype(other))):      # what the container hands out, as the hashes of their params
    if hasattr(c, name):
      got = get()
      d[name] = f'{type(got).__name__} {got.params.dtype} {list(got.params.shape)} {sha(got.params)}'
  return json.loads(json.dumps(d))


CONTAINERS = ('policy', 'population', 'population_rows', 'pair', 'pair_population')


def digests(cases):
  """grid() as the fixture holds it: {'hidden act head': {'widths dtype': the five containers' digests}}, a digest = 64 bits of the sha256 of a description"""
  out = {}
  for case, containers in cases.items():
    group, widths, dtype = case.rsplit(' ', 2)
    out.setdefault(group, {})[f'{widths} {dtype}'] = ' '.join(hashlib.sha256(json.dumps(containers[name], sort_keys=True).encode()).hexdigest()[:16] for name in CONTAINERS)
  return out


def grid(P, torch, hiddens=HIDDEN):
  """{case: {container: description, or the refusal's text}}"""
  out, threads = {}, torch.get_num_threads()
  torch.set_num_threads(1)                                             # (copies of 80k elements: starting a thread pool for each costs 30 x what they take)
  for hidden in hiddens:
    for act in ACTS:
      for head in HEADS:
        for widths in WIDTHS:
          for dtype in DTYPES:
            case = f'{"x".join(map(str, hidden))} {act} {"mlp" if head is None else f"gaussian squash={head[0]} {head[1]}"} {widths[0]}/{widths[1]} {dtype}'
            out[case] = {}
            for name, build in make_containers(P, torch, hidden, act, head, widths, dtype).items():
              try:
                out[case][name] = describe(torch, build())
              except ValueError as e:
                out[case][name] = f'ValueError: {e}'
  torch.set_num_threads(threads)
  return out


def refusals(P, torch):
  """[(what, a callable that is refused)]: one bad construction or call per `raise` of the module"""
  L, S = torch.nn.Linear, torch.nn.Sequential
  w = lambda dims, seed=0: weights(torch, dims, seed)
  mlp = lambda hidden=(16,), O=12, A=3, seed=0, **kw: P.MLPPolicy(w([O, *hidden, A], seed), 'relu', kw.pop('out_act', 'tanh'), obs_dim=O, act_dim=A, **kw)
  gau = lambda seed=0, O=12, A=3, **kw: P.GaussianMLPPolicy(w([O, 16, 2 * A], seed), 'relu', obs_dim=O, act_dim=A, **kw)
  env = lambda **kw: types.SimpleNamespace(**{**dict(device=torch.device('cpu'), num_envs=32, _cfg=types.SimpleNamespace(env_offset=0)), **kw})
  pair = lambda a=3, b=4, O=14, A=4, make=mlp, **kw: P.AgentPair(make(seed=a, O=O, A=A), make(seed=b, O=O, A=A), obs_dim=O, act_dim=A,
                                                                 **{**dict(backward_goal=make_goal((O, A))), **kw})
  pairs = lambda: P.PairPopulation([pair(), pair(5, 6)])
  return [
      ('param_dtype float16', lambda: mlp(param_dtype=torch.float16)),
      ('Sequential: Linear without bias', lambda: P.MLPPolicy(S(L(12, 16, bias=False), torch.nn.ReLU(), L(16, 3)))),
      ('Sequential: activation first', lambda: P.MLPPolicy(S(torch.nn.ReLU(), L(12, 16), L(16, 3)))),
      ('Sequential: Sigmoid', lambda: P.MLPPolicy(S(L(12, 16), torch.nn.Sigmoid(), L(16, 3)))),
      ('Sequential: one Linear', lambda: P.MLPPolicy(S(L(12, 3)))),
      ('Sequential: relu then tanh', lambda: P.MLPPolicy(S(L(12, 16), torch.nn.ReLU(), L(16, 16), torch.nn.Tanh(), L(16, 3)))),
      ('obs_dim 0', lambda: P.MLPPolicy(w([12, 16, 3]), obs_dim=0)),
      ('three hidden layers', lambda: P.MLPPolicy(w([12, 16, 16, 16, 3]))),
      ('hidden_act sigmoid', lambda: P.MLPPolicy(w([12, 16, 3]), hidden_act='sigmoid')),
      ('out_act relu', lambda: P.MLPPolicy(w([12, 16, 3]), out_act='relu')),
      ('layer shapes disagree', lambda: P.MLPPolicy([w([12, 16, 3])[0], w([12, 32, 3])[1]])),
      ('input width 13', lambda: P.MLPPolicy(w([13, 16, 3]))),
      ('output width 4', lambda: P.MLPPolicy(w([12, 16, 4]))),
      ('hidden width 24', lambda: P.MLPPolicy(w([12, 24, 3]))),
      ('Gaussian Sequential ending in Tanh', lambda: P.GaussianMLPPolicy(S(L(12, 16), torch.nn.ReLU(), L(16, 6), torch.nn.Tanh()))),
      ('log_std_map exp', lambda: gau(log_std_map='exp')),
      ('log_std_bounds reversed', lambda: gau(log_std_bounds=(1.0, -1.0))),
      ('require_widths: a PairPopulation where one pair goes', lambda: P.require_widths(pairs(), 'launch', 14, 4, env=env(), pair=True)),
      ('require_widths: not a policy', lambda: P.require_widths(object(), 'launch', 12, 3, env=env())),
      ('require_widths: widths', lambda: P.require_widths(mlp(O=14, A=4), 'launch', 12, 3, env=env())),
      ('require_widths: bf16 on the tabletop', lambda: P.require_widths(mlp(param_dtype=torch.bfloat16), 'launch', 12, 3, env=env())),
      ('require_widths: device', lambda: P.require_widths(mlp(), 'launch', 12, 3, env=env(device=torch.device('cuda', 0)))),
      ('require_widths: members', lambda: P.require_widths(P.PolicyPopulation([mlp()]), 'launch', 12, 3, env=env())),
      ('require_widths: unbounded', lambda: P.require_widths(mlp(O=32, A=8, out_act='none'), 'launch', 32, 8, env=env(), bounded=1.0)),
      ('population: envs_per_policy 8', lambda: P.PolicyPopulation([mlp()], envs_per_policy=8)),
      ('population: template without params', lambda: P.PolicyPopulation(mlp())),
      ('population: empty list', lambda: P.PolicyPopulation([])),
      ('population: list with params', lambda: P.PolicyPopulation([mlp()], params=torch.zeros(1, 255))),
      ('population: members differ', lambda: P.PolicyPopulation([mlp(), mlp((32,))])),
      ('population: bf16 params for a float32 template', lambda: P.PolicyPopulation(mlp(), params=torch.zeros(1, 255, dtype=torch.bfloat16))),
      ('population: params too short', lambda: P.PolicyPopulation(mlp(), params=torch.zeros(2, 100))),
      ('population call: ids past the members', lambda: P.PolicyPopulation([mlp()])(torch.zeros(32, 12))),
      ('pair: not policies', lambda: P.AgentPair(mlp(), object())),
      ('pair: agents differ', lambda: P.AgentPair(mlp(), mlp(out_act='none'))),
      ('pair: second hidden width 144', lambda: P.AgentPair(mlp((16, 144)), mlp((16, 144)))),
      ('pair: switch_every 0', lambda: P.AgentPair(mlp(), mlp(), switch_every=0)),
      ('pair: backward_goal of 5 values', lambda: P.AgentPair(mlp(), mlp(), backward_goal=[0.0] * 5)),
      ("pair: 'initial' on an env with two initial states", lambda: pair(backward_goal='initial').goal_row(types.SimpleNamespace(initial_states=[[0.0] * 7] * 2))),
      ('pairs: envs_per_policy 24', lambda: P.PairPopulation([pair()], envs_per_policy=24)),
      ('pairs: not pairs', lambda: P.PairPopulation([mlp()])),
      ('pairs: switch rule differs', lambda: P.PairPopulation([pair(), pair(switch_every=7)])),
      ('pairs: head differs', lambda: P.PairPopulation([pair(make=gau), pair(make=lambda **kw: gau(log_std_map='clamp', **kw))])),
      ('pairs: backward goal differs', lambda: P.PairPopulation([pair(), pair(backward_goal=[1.0] * 7)])),
  ]


def refused(P, torch):
  """-> ({what: 'Type: message'}, {what: the line of P's file that raised})"""
  texts, lines = {}, {}
  for what, call in refusals(P, torch):
    try:
      call()
    except (ValueError, NotImplementedError) as e:
      texts[what] = f'{type(e).__name__}: {e}'
      lines[what] = [f.lineno for f in traceback.extract_tb(e.__traceback__) if f.filename == P.__file__][-1]
    else:
      raise AssertionError(f'{what}: not refused')
  return texts, lines


def raise_lines(P):
  with open(P.__file__) as f:
    return {i for i, line in enumerate(f, 1) if line.lstrip().startswith('raise ')}


def load(path):
  """`path` as earl_benchmark_amd.policy (its relative imports are the package's)"""
  import earl_benchmark_amd
  spec = importlib.util.spec_from_file_location('earl_benchmark_amd.policy', path)
  P = importlib.util.module_from_spec(spec)
  sys.modules['earl_benchmark_amd.policy'] = earl_benchmark_amd.policy = P
  spec.loader.exec_module(P)
  return P


def main():
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument('--policy', required=True)
  ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'policy_containers_parent.json'))
  a = ap.parse_args()
  import torch
  P = load(os.path.abspath(a.policy))
  texts, lines = refused(P, torch)
  reached = sorted(lines.values())
  assert reached == sorted(raise_lines(P)), f'raise lines {sorted(raise_lines(P))}, reached {reached}'      # every raise, each by one construction
  with open(a.out, 'w') as f:
    rows = lambda d: ',\n'.join(f'{json.dumps(k)}:{json.dumps(v, sort_keys=True, separators=(",", ":"))}' for k, v in d.items())      # one entry per line
    f.write('{"grid":{\n' + rows(digests(grid(P, torch))) + '\n},\n"refusals":{\n' + rows(texts) + '\n}}\n')
  print(f'{a.out}: {len(texts)} refusals, {os.path.getsize(a.out)} bytes')


if __name__ == '__main__':
  main()

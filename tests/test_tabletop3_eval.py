"""earl_tabletop3_eval_episodes (include/earl_tabletop.h) without a GPU: the host twin, the Python path on device='cpu', the argument errors of both
libraries (they come before any HIP call), the cross-compiled kernels' resources, and what the two input sets shared with tests/test_tabletop3_eval_gpu.py
exercise.  Inputs and drivers: tests/tabletop3_eval_helpers.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_build
import tabletop3_eval_helpers as h
import tabletop_abi as ta
from earl_benchmark_amd import _abi
from test_tabletop_gpu import DENSE_ATOL, DENSE_RTOL

CPU = 'cpu'
N, T = 200, 24
LDS_BYTES = 108032      # row images 2 x 8 x 5,120 + actions 2 x 8 x 3 x 64 x 8 + loader staging 2 x 768


@pytest.fixture(scope='module')
def side():
  return ta.Side(CPU)


@pytest.mark.parametrize('env_offset', [0, 3])
@pytest.mark.parametrize('shared', [False, True], ids=['own', 'shared'])
@pytest.mark.parametrize('at_goal', [False, True], ids=['fixed', 'at_goal'])
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
def test_the_twin_is_the_sequence_of_reset_and_rollout(side, rt, at_goal, shared, env_offset):
  E = 3
  sc = h.scene(N, T, rt, at_goal, env_offset)
  act, episodes = h.inputs('b' if at_goal else 'a', N, T, E, shared)
  got = ta.both_fills(h.run_eval3, side, sc, act, what='eval3 twin', episodes=episodes)
  want = ta.both_fills(h.run_sequence3, side, sc, act, what='reset3 + rollout3 twin', episodes=episodes)
  ta.agree(got, want, 'twin vs sequence')                                   # outputs and every state array, bit for bit
  assert int(got['st.steps_since_reset'].min()) == T == int(got['st.steps_since_reset'].max())
  np.testing.assert_array_equal(got['st.num_interventions'].numpy(), sc.state['num_interventions'] + E)
  assert bool(got['out.done'][:, -1].all()) and not bool(got['out.done'][:, :-1].any())
  # counter use: episode e draws with counter + e (T + 1) -- the same call one episode later equals episodes 1.. of this one
  if not shared:
    later = ta.Scene.__new__(ta.Scene)
    later.__dict__.update(sc.__dict__)
    later.counter = sc.counter + (T + 1)
    tail, _ = h.run_eval3(side, later, np.ascontiguousarray(act[1:]), 0x00)
    for k in ta.OUT4:
      ta.same(tail['out.' + k], got['out.' + k][1:], f'counter use {k}')


@pytest.mark.parametrize('at_goal', [False, True], ids=['fixed', 'at_goal'])
@pytest.mark.parametrize('rt', ['sparse', 'dense'])
def test_one_episode_of_the_twin_is_the_oracle(side, rt, at_goal):
  sc = h.scene(N, T, rt, at_goal, 3)
  act, _ = h.inputs('b' if at_goal else 'a', N, T, 1)
  got, _ = h.run_eval3(side, sc, act, 0x00)
  ta.agree(got, ta.ref_eval(sc, act), 'twin vs oracle', dense=(DENSE_RTOL, DENSE_ATOL) if rt == 'dense' else None)


def env3(device=CPU, n=40, **kw):
  from earl_benchmark_amd.envs.tabletop_3obj import TabletopManipulation
  return TabletopManipulation(reward_type='sparse', num_envs=n, device=device, seed=5, env_offset=3, **kw)


def python_path(device):
  """rollout_episodes on the three-object env against per-episode rollout(a[e], reset_first=True): both argument forms, out=, the bookkeeping, a wrapper"""
  from earl_benchmark_amd.wrappers import PersistentStateWrapper
  n, E, T = 40, 3, 2 * h.K
  a = torch.from_numpy(h.scripted(n, T, E).copy()).to(device)
  ref_env = env3(device, n)
  PersistentStateWrapper(ref_env, T)
  want = [ref_env.rollout(a[e], reset_first=True) for e in range(E)]
  env = env3(device, n)
  wrapped = PersistentStateWrapper(env, T)
  c0 = env._cfg.counter
  got = wrapped.rollout_episodes(a)                                         # [E, T, N, 3] through the wrapper's pass-through
  assert tuple(got[0].shape) == (E, T, n, 20) and got[0].dtype == torch.float32 and got[2].dtype == torch.bool
  for k in range(4):
    ta.same(got[k], torch.stack([w[k] for w in want]), f'rollout_episodes output {k}')
  assert env._cfg.counter == c0 + E * (T + 1) == ref_env._cfg.counter and env.total_step_count == E * T == ref_env.total_step_count
  for name in ('qpos', 'attached', 'goal_idx', 'steps_since_reset', 'interventions'):
    ta.same(getattr(env, name), getattr(ref_env, name), f'state {name}')
  assert wrapped.num_interventions.tolist() == [E] * n
  # [T, N, 3] with episodes=, into caller-owned tensors
  env2 = env3(device, n)
  PersistentStateWrapper(env2, T)
  outs = tuple(torch.empty_like(g) for g in got)
  back = env2.rollout_episodes(a[0], episodes=E, out=outs)
  assert all(b is o for b, o in zip(back, outs))
  ref2 = env3(device, n)
  PersistentStateWrapper(ref2, T)
  for e in range(E):
    w = ref2.rollout(a[0], reset_first=True)
    for k in range(4):
      ta.same(outs[k][e], w[k], f'shared actions: episode {e} output {k}')
  with pytest.raises(ValueError):
    env2.rollout_episodes(a[0])
  with pytest.raises(ValueError):
    env2.rollout_episodes(a, episodes=E + 1)
  return got


def test_rollout_episodes_on_the_host():
  python_path(CPU)


def _edge_calls(fn, stream):
  """every argument error of the entry point -> EARL_ERR_ARG; `stream`: the HIP library's trailing argument"""
  n, E, Tq = 5, 2, 16
  sc = h.scene(n, Tq)
  r = ta.Run(ta.Side(CPU), 0x00)                                            # host buffers: no call below gets as far as touching them
  st = r.state(sc)
  act = r.put('in.act', np.array(h.scripted(n, Tq, E)))
  out = r.out((E, Tq, n), 20)
  tail = (None,) if stream else ()
  call = lambda cfg, stp, e, t, a, stride, o: fn(cfg, stp, e, t, a, stride, o, *tail)
  good = (C.byref(sc.cfg()), C.byref(st), E, Tq, act.data_ptr(), Tq * n * 3, C.byref(out))
  bad = {
      'episodes < 0': good[:2] + (-1,) + good[3:],
      'T < 0': good[:3] + (-1,) + good[4:],
      'negative stride': good[:5] + (-1,) + good[6:],
      'act NULL': good[:4] + (None,) + good[5:],
      'out NULL': good[:6] + (None,),
      'cfg NULL': (None,) + good[1:],
      'state NULL': good[:1] + (None,) + good[2:],
      'wide_init': (C.byref(sc.cfg(wide_init=1)),) + good[1:],
      'goal_change_frequency': (C.byref(sc.cfg(goal_change_frequency=3)),) + good[1:],
      'n < 0': (C.byref(sc.cfg(n=-1)),) + good[1:],
      'reward_type': (C.byref(sc.cfg(reward_type=7)),) + good[1:],
  }
  for what, args in bad.items():
    assert call(*args) == -1, what
  # the empty calls are no errors, and they need no device either
  assert call(*(good[:2] + (0,) + good[3:])) == 0
  assert call(*((C.byref(sc.cfg(n=0)),) + good[1:])) == 0
  ta.assert_untouched({k: v[3] for k, v in r.b.bufs.items() if k.startswith(('st.', 'out.'))}, sc, 'argument errors')
  return good


def test_argument_errors_from_the_host_library():
  lib = _abi.load_host()
  good = _edge_calls(lib.earl_tabletop3_eval_episodes_cpu, False)
  assert lib.earl_tabletop3_eval_episodes_cpu(*good) == 0                   # (and the well-formed call is taken)
  assert b'' != lib.earl_last_error()


def test_argument_errors_from_the_hip_library_need_no_gpu():
  lib = _abi.load()
  _edge_calls(lib.earl_tabletop3_eval_episodes, True)
  prev = lib.earl_debug_set_rollout3_form(2)
  try:
    assert lib.earl_debug_set_rollout3_form(7) == 2 and lib.earl_debug_set_rollout3_form(1) == 2      # an unknown form is not taken
    assert lib.earl_debug_set_rollout3_form(0) == 1
  finally:
    lib.earl_debug_set_rollout3_form(prev)


def test_the_eval_unit_cross_compiles_without_scratch():
  res = kernel_build.unit('tabletop3_eval.hip').resources
  kernels = {k: v for k, v in res.items() if 'rollout3_ws_kernel' in k}
  assert len(kernels) == 2 and len(res) == 2, sorted(res)                   # the sparse and the dense instantiation, nothing else
  for name, r in res.items():
    print(name, r)
    assert r['scratch'] == 0, name
    assert r['lds'] == LDS_BYTES, name
    assert r['vgpr'] + r['agpr'] <= 256, name                              # seven waves per workgroup: two per SIMD
  recorded = kernel_build.recorded_figures()                                # profiles/policy_kernel_resources.txt holds the two lines as compiled
  figures = kernel_build.unit('tabletop3_eval.hip').figures
  assert len(figures) == 2
  for name, fig in figures.items():
    assert recorded.get(name) == [fig], (name, fig, recorded.get(name))
  src = open(kernel_build.CSRC + '/tabletop3_rollout_ws.h').read()
  assert f'constexpr int kWs3K = {h.K};' in src                             # the chunk length the tests (and the header's macro) work with


def test_what_the_input_sets_exercise(side):
  """floors about half of what the twin gives (n = 200, T = 24, env seed 3; measured: holding 13.7 / 8.9 / 11.2 %, releases 2.1 %, clipped 25.5 %, second grasp
  on another object 25 %; set (b): success rows 11.1 %, envs with both outcomes 19 %): a comparison on these inputs cannot pass on rows that never grasp"""
  E = 2
  a, _ = h.run_eval3(side, h.scene(N, T, 'sparse', False), h.scripted(N, T, E), 0x00)
  ca = h.coverage(a)
  print('set (a):', ca)
  assert all(f >= 0.04 for f in ca['holding']), ca
  assert ca['release'] >= 0.01 and ca['clipped'] >= 0.10 and ca['regrasp_other'] >= 0.10, ca
  b, _ = h.run_eval3(side, h.scene(N, T, 'sparse', True), h.jitter(N, T, E), 0x00)
  cb = h.coverage(b)
  print('set (b):', cb)
  assert 0.03 <= cb['success'] <= 0.97 and cb['both'] >= 0.10, cb

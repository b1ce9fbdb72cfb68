"""The width matrix of the Sawyer door / peg policy rollout on the MI355X (csrc/physics_env_sawyer.h: pol_layer works in groups of 64 output rows and clamps the
rows past a layer's end): every hidden width 16 .. 256 in every layer position on the door -- the partial group after a full one among them (widths 80 .. 112,
144 .. 176, 208 .. 240) --, the group-edge widths on the peg as well, and one door launch above 4096 envs so that the eight-wave build (csrc/physics_w8.hip) runs a
partial group too.  Structured as tests/test_sawyer_policy_rollout_gpu.py's test_actions_are_the_contract_bit_for_bit: every action of the launch equals
earl_mlp_policy_forward_cpu (libearl_host.so) on the float32 observation the step consumed, rolled-back rows included, and with a head the returned eps equal
normal_quantile_f32 of the Philox words recomputed on the host.  tests/policy_width_cases.py holds the table (tests/test_policy_math.py checks what it covers)."""
import numpy as np
import pytest

import policy_width_cases as W
from test_physics_step_graph_gpu import make
from test_sawyer_policy_rollout import forward_cpu
from test_sawyer_policy_rollout_gpu import HEADS, expected_eps, policy

pytestmark = pytest.mark.gpu


def actions_are_the_contract(kind, n, hidden, hact, oact, head, lmap):
  from earl_benchmark_amd import _abi
  T, off, seed = W.SAWYER_T, W.SAWYER_OFFSET, 11
  env = make(kind, n, seed=seed, env_offset=off)
  u = env.unwrapped
  pi, layers = policy(hidden, hact, oact, head=head, log_std_map=lmap, seed=len(hidden) * 7 + hidden[0])
  env.rollout_policy(pi, 2)                                             # (the launch under test starts at a step counter that is not 0)
  step0 = u.total_step_count
  obs0 = u.last_obs.clone()                                             # what the env last returned: the launch's obs0
  kw = {} if head is None else {'sample': head == 'sample', 'return_noise': True}
  out = env.rollout_policy(pi, T, **kw)
  x = np.concatenate([obs0.cpu().numpy()[None], out['obs'].cpu().numpy()[:-1]]).astype(np.float32).reshape(T * n, 14)
  hd, eps = None, None
  what = f'{kind} n={n} {hidden} {hact}/{oact} head={head} map={lmap} (output-row groups of 64 per layer: {[W.sawyer_groups(w) for w in hidden]})'
  if head is not None:
    hd = (HEADS[head], _abi.LOGSTD_MAPS[lmap], -5.0, 2.0)
    eps = out['eps'].cpu().numpy()
    np.testing.assert_array_equal(eps.view(np.uint32), expected_eps(seed, off, n, step0, T).view(np.uint32), err_msg=what)        # written in both modes
  want = forward_cpu(layers, hact, oact, x, head=hd, eps=None if eps is None else eps.reshape(T * n, 4)).reshape(T, n, 4)
  got = out['actions'].cpu().numpy()
  if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    t, i, j = bad[0]
    raise AssertionError(f'{what}: {len(bad)} of {want.size} actions differ; first at step {t} env {i} action {j}: device {got[t, i, j]!r} host {want[t, i, j]!r}')
  assert np.isfinite(got).all() and len(np.unique(got[:, :, 0])) > T * n // 2, what
  if head == 'sample':
    mean = forward_cpu(layers, hact, oact, x, head=(0,) + hd[1:]).reshape(T, n, 4)
    assert (got != mean).mean() > 0.9                                   # ... and the noise is in the actions
  print(f'{what}: guard share {float((out["status"] != 0).float().mean()):.5f}')


CASES = W.sawyer_cases()


@pytest.mark.parametrize('kind,hidden,hact,oact,head,lmap', CASES, ids=[f'{c[0]}-{"x".join(map(str, c[1]))}-{c[2]}-{c[3]}-{c[4]}-{c[5]}' for c in CASES])
def test_actions_are_the_contract_at_every_width(kind, hidden, hact, oact, head, lmap):
  """n = 32, env_offset = 3, T = 6: 34 door and 14 peg cases.  Observed (one MI355X): no difference on any of the 48; share of rows with status != 0: 0 in every case;
  at most 0.09 s a case after the first (0.47 s, which loads the library)"""
  actions_are_the_contract(kind, W.SAWYER_N, hidden, hact, oact, head, lmap)


def test_the_eight_wave_build_runs_a_partial_group_too():
  """4160 door envs (> 4096: the launcher takes physics_w8.hip's instantiation), hidden (80, 144): a partial group after a full one in both layers.
  Observed (one MI355X): no difference, guard share 0, 0.19 s"""
  actions_are_the_contract('door', 4160, (80, 144), 'relu', 'tanh', 'sample', 'tanh')

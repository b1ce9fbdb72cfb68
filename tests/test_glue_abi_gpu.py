"""The glue C ABI at its edges (include/earl_glue.h), called directly with the banded buffers of tests/tabletop_abi.py: bands of 0x00 and of 0xFF that must stay
intact and must not change a bit of the results, output interiors pre-filled with a pattern that must be gone, each optional output NULL in turn, and the result
equal to the reference bit for bit -- oracle/glue_oracle for the eight numpy restatements, a plain numpy Philox4x32-10 written here for earl_philox_uniform,
which has no other direct test.

  kernel of csrc/glue.hip          entry point                    n                 optional outputs           reference
  sawyer_sparse_kernel<double>     earl_sawyer_sparse_f64         1 255 256 257     reward, success            glue_oracle.sawyer_sparse
  sawyer_sparse_kernel<float>      earl_sawyer_sparse_f32         1 255 256 257     reward, success            glue_oracle.sawyer_sparse
  leg_to_motor_kernel              earl_minitaur_leg_to_motor     1 255 256 257                                glue_oracle.leg_to_motor
  motor_kernel                     earl_minitaur_motor_torque     1 255 256 257     actual, observed torque    glue_oracle.motor_torque
  minitaur_reward_kernel           earl_minitaur_reward           1 255 256 257     reward, success            glue_oracle.minitaur_reward
  kitchen_reward_kernel            earl_kitchen_reward            1 255 256 257     reward, success            glue_oracle.kitchen_reward
  kitchen_action_kernel            earl_kitchen_action            1 255 256 257                                glue_oracle.kitchen_action
  kitchen_obs_kernel               earl_kitchen_obs               1 255 256 257     noise (an input)           glue_oracle.kitchen_obs
  uniform_kernel                   earl_philox_uniform            1 7 257 x k 1 2 3 46                         numpy Philox4x32-10 (below)
"""
import ctypes as C

import numpy as np
import pytest

import tabletop_abi as ta
from conftest import load_golden

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257)          # one lane, a block less one, a whole block (256 lanes), one lane into the second block


@pytest.fixture(scope='module')
def side():
  return ta.Side('cuda')


def check(side, call, want, what, optional=()):
  """call(run) -> rc on a fresh ta.Run per fill; all outputs present, then each optional one NULL in turn: what remains equals `want`"""
  import torch
  for null in [()] + [(k,) for k in optional]:
    def fn(s, fill):
      r = ta.Run(s, fill, null)
      return r.finish(call(r), what)
    res = ta.both_fills(fn, side, what=f'{what} without {null}')
    ta.agree(res, {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in want.items()}, what, null=null)


def p(t):
  return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------- the eight numpy restatements
@pytest.mark.parametrize('n', NS)
def test_sawyer_sparse_both_precisions(side, n):
  import torch
  from oracle import glue_oracle as go
  rng = np.random.default_rng(n)
  obs = rng.uniform(-1, 1, size=(n, 14))
  near = np.arange(n) % 2 == 0                             # rows around the radius: both outcomes
  obs[near, 4:7] = obs[near, 11:14] + rng.uniform(-0.02, 0.02, size=(int(near.sum()), 3))
  for name, o in (('f64', obs), ('f32', obs.astype(np.float32))):
    for radius in (0.02, 0.05):
      rew, suc = go.sawyer_sparse(o, radius)

      def call(r):
        x = r.put('in.obs', o)
        return getattr(side.lib, 'earl_sawyer_sparse_' + name)(n, p(x), radius, p(r.blank('out.reward', (n,), torch.float32, n)),
                                                               p(r.blank('out.success', (n,), torch.uint8, n)), side.stream)
      check(side, call, {'out.reward': rew, 'out.success': suc}, f'sawyer_sparse_{name} n={n} r={radius}', optional=('reward', 'success'))
  assert n == 1 or 0 < int(go.sawyer_sparse(obs, 0.02)[1].sum()) < n


@pytest.mark.parametrize('n', NS)
def test_minitaur_leg_model_motor_model_and_reward(side, n):
  import torch
  from earl_benchmark_amd import _abi
  from oracle import glue_oracle as go
  rng = np.random.default_rng(n)
  act = rng.uniform(-1, 1, size=(n, 8))

  def leg(r):
    return side.lib.earl_minitaur_leg_to_motor(n, p(r.put('in.action', act)), p(r.blank('out.motor_angle', (n, 8), torch.float64, n * 8)), side.stream)
  check(side, leg, {'out.motor_angle': go.leg_to_motor(act)}, f'leg_to_motor n={n}')

  cmd, ang, vel = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-700, 700, n)
  for kp, kd, tc in ((1.2, 0.0, False), (1.2, 0.02, False), (1.2, 0.0, True)):
    a0, o0 = go.motor_torque(cmd, ang, vel, kp=kp, kd=kd, torque_control=tc)
    mp = _abi.MotorParams(kp=kp, kd=kd, voltage=16.0, viscous_damping=0.0, torque_control=int(tc))

    def motor(r):
      return side.lib.earl_minitaur_motor_torque(n, C.byref(mp), p(r.put('in.command', cmd)), p(r.put('in.angle', ang)), p(r.put('in.velocity', vel)),
                                                 p(r.blank('out.actual_torque', (n,), torch.float64, n)),
                                                 p(r.blank('out.observed_torque', (n,), torch.float64, n)), side.stream)
    check(side, motor, {'out.actual_torque': a0, 'out.observed_torque': o0}, f'motor_torque n={n} kd={kd} tc={tc}', optional=('actual_torque', 'observed_torque'))

  obs = rng.uniform(-1, 1, size=(n, 32))
  close = np.arange(n) % 2 == 0
  obs[close, 28:30] = obs[close, 30:32] + rng.uniform(-0.1, 0.1, size=(int(close.sum()), 2))
  rew, suc = go.minitaur_reward(obs, 2.0, 0.005, 0.01)

  def reward(r):
    return side.lib.earl_minitaur_reward(n, p(r.put('in.obs', obs)), 2.0, 0.005, 0.01, p(r.blank('out.reward', (n,), torch.float64, n)),
                                         p(r.blank('out.success', (n,), torch.uint8, n)), side.stream)
  check(side, reward, {'out.reward': rew, 'out.success': suc}, f'minitaur_reward n={n}', optional=('reward', 'success'))


@pytest.mark.parametrize('n', NS)
def test_kitchen_reward_action_and_observation(side, n):
  import torch
  from earl_benchmark_amd import _abi
  from oracle import glue_oracle as go
  rng = np.random.default_rng(n)
  z = load_golden('kitchen_step')
  po = go.kitchen_params(z['kitchen_pos_bound'], z['kitchen_vel_bound'], z['kitchen_pos_noise_amp'])     # the oracle's table: the reference's own config
  pd = _abi.KitchenParams()
  assert side.lib.earl_kitchen_default_params(C.byref(pd)) == 0

  obs = rng.uniform(-1, 1, size=(n, 46))
  solved = rng.integers(0, 9, size=n)                      # rows with their first `solved` components at the goal: every choice of the first unsolved one
  start = [9, 11, 13, 15, 17, 19, 20, 22, 23]
  for i in range(n):
    obs[i, 9:start[solved[i]]] = obs[i, 32:23 + start[solved[i]]]
  obs[::3, 9:23] = obs[::3, 32:46] + rng.uniform(-0.08, 0.08, size=obs[::3, 9:23].shape)      # around the success radius 0.3
  mocap, sites = rng.uniform(-1, 1, size=(n, 3)), rng.uniform(-1, 1, size=(n, 8, 3))
  rew, suc = go.kitchen_reward(obs, mocap, sites)

  def reward(r):
    return side.lib.earl_kitchen_reward(n, p(r.put('in.obs', obs)), p(r.put('in.mocap', mocap)), p(r.put('in.sites', sites)),
                                        p(r.blank('out.reward', (n,), torch.float64, n)), p(r.blank('out.success', (n,), torch.uint8, n)), side.stream)
  check(side, reward, {'out.reward': rew, 'out.success': suc.astype(np.uint8)}, f'kitchen_reward n={n}', optional=('reward', 'success'))

  act = rng.uniform(-1.5, 1.5, size=(n, 9))
  mp0 = rng.uniform([-0.7, -0.1, 1.8], [0.4, 0.5, 2.6], size=(n, 3))
  mp0[::4] = [0.4, -0.1, 2.6]                              # on the clip box
  lq = rng.uniform(-1, 1, size=(n, 9))
  mp1, ctrl = go.kitchen_action(po, act, mp0, lq)

  def action(r):
    return side.lib.earl_kitchen_action(n, C.byref(pd), p(r.put('in.action', act)), p(r.put('st.mocap', mp0)), p(r.put('in.last_qpos', lq)),
                                        p(r.blank('out.ctrl', (n, 9), torch.float64, n * 9)), side.stream)
  check(side, action, {'st.mocap': mp1, 'out.ctrl': ctrl}, f'kitchen_action n={n}')

  qpos, goal, noise = rng.uniform(-1, 1, size=(n, 23)), rng.uniform(-1, 1, size=(n, 23)), rng.uniform(-1, 1, size=(n, 46))
  for u in (noise, None):                                  # NULL noise: env.initializing

    def observe(r):
      return side.lib.earl_kitchen_obs(n, C.byref(pd), p(r.put('in.qpos', qpos)), p(r.put('in.goal', goal)), p(r.put('in.noise', u)),
                                       p(r.blank('out.obs', (n, 46), torch.float64, n * 46)), side.stream)
    check(side, observe, {'out.obs': go.kitchen_obs(po, qpos, goal, u)}, f'kitchen_obs n={n} noise={u is not None}')


# ---------------------------------------------------------------------------------------------------- earl_philox_uniform
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
  """Philox4x32-10 (Salmon et al., SC'11): ctr = four uint64 arrays holding 32-bit words, key = two words -> four arrays of words"""
  c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in ctr)
  k0, k1 = np.uint64(key[0]), np.uint64(key[1])
  for _ in range(10):
    p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
  return c0, c1, c2, c3


def test_the_numpy_philox_reproduces_the_known_answers():
  """the Random123 known-answer vectors of tests/test_oracle.py::test_philox_known_answers"""
  kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
  for ctr, key, want in kat:
    assert tuple(int(x) for x in philox4x32_10([np.array(c) for c in ctr], key)) == want


def uniform_reference(n, k, seed, counter, env_offset, stream_id, lo, hi):
  """out[env, j] = lo + (hi - lo) u, u from words (2 (j % 2), 2 (j % 2) + 1) of the block with counter {stream_id + j // 2, env_offset + env, counter lo,
  counter hi} under the key (seed lo, seed hi); u = ((hi_word << 32 | lo_word) >> 11) 2^-53"""
  j = np.arange(k, dtype=np.uint64)[None, :] + np.zeros((n, 1), np.uint64)
  env = np.arange(n, dtype=np.uint64)[:, None] + np.zeros((1, k), np.uint64)
  w = philox4x32_10(((np.uint64(stream_id) + j // np.uint64(2)) & M32, (np.uint64(env_offset) + env) & M32, np.full_like(j, counter & 0xFFFFFFFF),
                     np.full_like(j, counter >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
  odd = (j % np.uint64(2)) == 1
  lo_w, hi_w = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
  u = (((hi_w << np.uint64(32)) | lo_w) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
  return lo + (hi - lo) * u


STREAM_NOISE, STREAM_RESET = 0x4B00, 0x4B80      # the kitchen env's stream ids (earl_benchmark_amd/envs/kitchen.py)


@pytest.mark.parametrize('counter', [12345, (7 << 32) + 99], ids=['counter_below_2^32', 'counter_above_2^32'])
@pytest.mark.parametrize('k', [1, 2, 3, 46])
def test_philox_uniform_against_numpy(side, k, counter):
  """k odd: the kernel's last block of a row has one draw only (`if (2 * j + 1 < k)`); the element behind it is the next row's first, or the band when n = 1"""
  import torch
  seed = (0xDEADBEEF << 32) | 0x12345678
  for n in (1, 7, 257):
    for env_offset in (0, 1000):
      for stream_id, lo, hi in ((STREAM_NOISE, -1.0, 1.0), (STREAM_RESET, 0.0, 1.0)):       # the kitchen env's two uses: sensor noise and the reset's row pick
        def draw(nn, off):
          def call(r):
            return side.lib.earl_philox_uniform(nn, k, seed, counter, off, stream_id, lo, hi, p(r.blank('out.u', (nn, k), torch.float64, nn * k)), side.stream)
          return call
        want = uniform_reference(n, k, seed, counter, env_offset, stream_id, lo, hi)
        assert want.shape == (n, k) and (want >= lo).all() and (want < hi).all()
        what = f'philox_uniform n={n} k={k} env_offset={env_offset} stream={stream_id:#x}'
        check(side, draw(n, env_offset), {'out.u': want}, what)
        if n > 1:                                          # a batch equals its two shards
          a = n // 3 + 1
          check(side, draw(a, env_offset), {'out.u': want[:a]}, what + ' first shard')
          check(side, draw(n - a, env_offset + a), {'out.u': want[a:]}, what + ' second shard')
  # the high words matter: another counter high word / seed high word gives other draws
  assert not np.array_equal(uniform_reference(4, k, seed, counter, 0, STREAM_NOISE, 0.0, 1.0), uniform_reference(4, k, seed, counter + (1 << 32), 0, STREAM_NOISE, 0.0, 1.0))
  assert not np.array_equal(uniform_reference(4, k, seed, counter, 0, STREAM_NOISE, 0.0, 1.0), uniform_reference(4, k, seed + (1 << 32), counter, 0, STREAM_NOISE, 0.0, 1.0))

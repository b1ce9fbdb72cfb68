"""The Sawyer kernels' collision phases (csrc/physics_stepper.h: C0 bounding tests, C1 - C2 pair tests and compaction into contact slots) on the synthetic tables of
tests/collision_cases.py, through earl_physics_forward / earl_physics_step only: the closed-form response of one contact on the peg's free body, and the device against
the C restatement on tables chosen for the lane mapping (the chunk loop of blocks beyond 16 pairs, capsule runs, caps and max_con, four envs of a wave with four near
sets).  tests/test_collision_geometry.py holds the restatement to exact geometry on the same tables, without a GPU.

Every case runs with 16 lanes per env (four envs per wavefront) and under earl_debug_set_physics_lanes(64) (one env per wavefront), to the same tolerance."""
import numpy as np
import pytest

import collision_cases as cc

pytestmark = pytest.mark.gpu
RTOL = {10: 1e-8, 15: 1e-7}                      # tests/test_physics_gpu.py test_forward_matches_reference / test_peg_forward_matches_reference


@pytest.fixture(scope='module')
def gpu():
  import torch
  from earl_benchmark_amd import physics
  from oracle import physics_c, physics_oracle
  return torch, physics, physics_c, physics_oracle


def both_lanes(dm, fn):
  """fn(lanes) with 16 lanes per env, then under earl_debug_set_physics_lanes(64); the default is put back whatever happens"""
  fn(16)
  assert dm.lib.earl_debug_set_physics_lanes(64) == 0
  try:
    fn(64)
  finally:
    assert dm.lib.earl_debug_set_physics_lanes(16) == 0


def forward(torch, dm, state, sl):
  t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sl])).cuda()
  qacc, efc, _ = dm.forward(*(t(a) for a in state))
  return qacc.cpu().numpy(), efc.cpu().numpy()


def device_equals_restatement(gpu, d, state, want_ncon):
  """DeviceModel.forward against physics_c.CModel.run on n = 64 envs and on the slices [3, 3 + n) for n = 1, 4, 5 (a single env, one wave, a wave and a quarter), both lane
  mappings; the restatement's contact count per env must be want_ncon (what the case is about)"""
  torch, physics, physics_c, _ = gpu
  dm, cm = physics.DeviceModel(d), physics_c.CModel(d)
  ref = cm.run(*state, integrate=False)
  np.testing.assert_array_equal(ref['ncon'], want_ncon)
  rtol = RTOL[dm.nv]
  nrow = 6 + 2 * dm.nv

  def run(lanes):
    for sl in (slice(0, 64), slice(3, 4), slice(3, 7), slice(3, 8)):
      qacc, efc = forward(torch, dm, state, sl)
      for k, i in enumerate(range(*sl.indices(64))):
        np.testing.assert_allclose(qacc[k], ref['qacc'][i], rtol=rtol, atol=1e-8 * np.abs(ref['qacc'][i]).max(), err_msg=f'qacc: lanes {lanes}, envs {sl}, env {i}')
        np.testing.assert_allclose(efc[k], ref['efc'][i][:nrow], rtol=rtol, atol=1e-8 * (1 + np.abs(ref['efc'][i]).max()), err_msg=f'efc: lanes {lanes}, envs {sl}, env {i}')
  both_lanes(dm, run)
  return ref


# env i of 64: the hand's sets (listed first) are near in envs 1 and 3 of every wave, the free body's / the door's (listed last) in envs 2 and 3 -- env 0 of a wave has no near
# block at all, so the wave's first near block is never near there; env 3 has every block
HAND = np.arange(64) % 4 % 2 == 1
LAST = np.arange(64) % 4 >= 2
NEAR3 = np.arange(64) % 4 != 0                   # tables with one group of sets: near in envs 1 - 3 of every wave


# ------------------------------------------------------------------------------------------------------------------------------ closed form (peg)
def test_closed_form_on_the_device(gpu):
  """cc.peg_alpha and the exact normal against the peg kernel, free body's inertia 1e-4 kg m^2 (a misplaced line of action shows as angular acceleration).  Each bound is
  the larger of 1e-8 (the device-vs-restatement forward tolerance) and 16 x the figure the C restatement shows against the same closed form, per group of states
  (cc.closed_form_figures); the states just outside the margin give the contact-free qacc bit for bit.  Figures: COLL-FIG lines, DESIGN.md.  Where 16 x the
  restatement's figure is the larger -- alpha at the edge of the margin, 1.7e-7 -- the bound rests on that margin and not on the 1e-8 floor."""
  torch, physics, physics_c, po = gpu
  d = cc.peg_closed_form_table(free_inertia=1e-4)
  lm = po.LinkModel(d)
  states = cc.peg_closed_form_states(d)
  n = len(states)
  assert 300 <= n <= 400 and sum(s['hit'] for s in states) > 250
  state = (np.array([s['qpos'] for s in states]), np.zeros((n, 15)), np.tile([0.0, 0.6, 0.2], (n, 1)), np.tile([1.0, 0, 1, 0], (n, 1)), np.zeros((n, 2)))
  ref = physics_c.CModel(d).run(*state, integrate=False)
  exact = cc.closed_form_exact(d, lm, states)
  fig_ref = cc.closed_form_figures(d, lm, states, ref['qacc'], exact)
  cc.print_figures('restatement', fig_ref)
  dm, dm0 = physics.DeviceModel(d), physics.DeviceModel(d, contacts=False)
  miss = np.array([not s['hit'] for s in states])

  def run(lanes):
    qacc, free = np.zeros((n, 15)), np.zeros((n, 15))
    for a in range(0, n, 64):
      qacc[a:a + 64] = forward(torch, dm, state, slice(a, a + 64))[0]
      free[a:a + 64] = forward(torch, dm0, state, slice(a, a + 64))[0]
    fig = cc.closed_form_figures(d, lm, states, qacc, exact)
    cc.print_figures(f'device ({lanes} lanes)', fig)
    for g in fig:
      for k in ('alpha', 'angle', 'angular'):
        bound = max(1e-8, 16 * fig_ref[g][k])
        assert fig[g][k] <= bound, (lanes, g, k, fig[g][k], bound)
    assert miss.sum() == 78 and np.array_equal(qacc[miss], free[miss])            # bit for bit
    assert (np.abs(qacc[~miss, 9:12]).max(1) > 0).all()
  both_lanes(dm, run)


# ------------------------------------------------------------------------------------------------------------------------------ lane mapping (peg)
@pytest.mark.parametrize('name', list(cc.ROW_CONFIGS))
def test_peg_blocks_chunks_caps_and_max_con(gpu, name):
  """blocks of 1, 15, 16, 17 and 33 pairs with the active pairs in the last chunk / the last lane of a partial chunk; the cap binding in the first chunk, at the chunk
  boundary and in later chunks; max_con binding inside a block; a later block without a slot; four envs of a wave with the near sets none / first block / last blocks / all"""
  d, hits = cc.peg_rows_table(*cc.ROW_CONFIGS[name])
  nhand = sum(r[0] for r in cc.ROW_CONFIGS[name][2])
  hand, body = (HAND, LAST) if nhand else (NEAR3, NEAR3)
  state = cc.peg_rows_states(d, 64, 11, body_on_floor=body, hand_near=hand)
  want = [len(cc.expected_pairs(d, [p for p in hits if (hand[i] if p < nhand else body[i])])) for i in range(64)]
  assert want[0] == 0 and want[3] == len(cc.expected_pairs(d, hits)) > 0
  device_equals_restatement(gpu, d, state, want)


def test_peg_box_on_a_link(gpu):
  """the box rides on the free body, a world-fixed sphere and a world-fixed point in every region of it (tests/test_collision_geometry.py holds the restatement to the exact
  geometry on these states): the contact acts on the box's link, with the opposite sign"""
  d = cc.peg_moving_box_table()
  states = cc.peg_moving_box_states(d)[::2][:64]
  n = len(states)
  assert n == 64 and 20 < sum(s['hit'] for s in states) < 60
  state = (np.array([s['qpos'] for s in states]), np.zeros((n, 15)), np.tile([0.0, 0.6, 0.2], (n, 1)), np.tile([1.0, 0, 1, 0], (n, 1)), np.zeros((n, 2)))
  device_equals_restatement(gpu, d, state, [int(s['hit']) for s in states])


def test_peg_off_centre_sphere_with_friction(gpu):
  """spheres away from the centre of mass, sliding and spinning: the cone's sliding zone, torque from the contact point.  The restatement is the only reference here."""
  d, hits = cc.peg_rows_table([(3, [0, 2], 4), (17, [16], 4)], 12)
  state = list(cc.peg_rows_states(d, 64, 12, body_on_floor=np.arange(64) % 4 != 1))
  rng = np.random.default_rng(13)
  state[1][:, 9:11] = rng.normal(size=(64, 2)) * 0.2          # tangential velocity
  state[1][:, 11] = rng.normal(size=64) * 0.01
  state[1][:, 12:15] = rng.normal(size=(64, 3)) * 0.5
  ref = device_equals_restatement(gpu, d, tuple(state), [0 if i % 4 == 1 else 3 for i in range(64)])
  assert np.abs(ref['qacc'][::4, 12:15]).max() > 1.0 and np.abs(ref['qacc'][::4, 9:11]).max() > 0.1      # torque and friction were there to get wrong


def test_peg_step_in_which_a_sphere_crosses_the_margin(gpu):
  """one earl_physics_step of three timesteps: no contact in the first, the falling body's spheres inside the margin from the second on -- the contact count changes within
  the call, under the warm start of the active-set iteration"""
  torch, physics, physics_c, _ = gpu
  d, hits = cc.peg_rows_table([(17, [0, 16], 4), (3, [1], 4)], 12)
  n = 20
  qpos, qvel, mp, mq, ctrl = cc.peg_rows_states(d, n, 14)
  margin = float(d['col_cls_margin'][0])
  qpos[:, 11] = cc.FLOOR_TOP + cc.SPH_R + margin + 0.0006      # 0.6 mm clear of the margin (the 2 mrad tilt takes 0.07 mm); 1.25 mm per timestep at 0.5 m/s
  qvel[:, 11] = -0.5
  qpos[::5, 11] += 0.5                                          # (and envs that stay clear, among them env 0 of waves 0 and 1 ... every fifth)
  cm = physics_c.CModel(d)
  assert not cm.run(qpos, qvel, mp, mq, ctrl, integrate=False)['ncon'].any()
  ref = cm.run(qpos, qvel, mp, mq, ctrl, nsub=3)
  after = cm.run(ref['qpos'], ref['qvel'], mp, mq, ctrl, integrate=False)['ncon']
  np.testing.assert_array_equal(after, [0 if i % 5 == 0 else 3 for i in range(n)])
  one = cm.run(qpos, qvel, mp, mq, ctrl, nsub=1)
  assert (cm.run(one['qpos'], one['qvel'], mp, mq, ctrl, integrate=False)['ncon'] == after).all()      # in contact from the second timestep on
  dm = physics.DeviceModel(d)

  def run(lanes):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dq, dv = t(qpos), t(qvel)
    dm.step(dq, dv, t(mp), t(mq), t(ctrl), nsub=3)
    np.testing.assert_allclose(dq.cpu().numpy(), ref['qpos'], rtol=1e-8, atol=1e-8, err_msg=f'lanes {lanes}')
    np.testing.assert_allclose(dv.cpu().numpy(), ref['qvel'], rtol=1e-8, atol=1e-7, err_msg=f'lanes {lanes}')
  both_lanes(dm, run)
  assert np.abs(ref['qvel'][1::5, 11] + 0.5).min() > 0.05      # the contacts stopped the fall: they acted


# ------------------------------------------------------------------------------------------------------------------------------ lane mapping (door)
@pytest.mark.parametrize('name', list(cc.DOOR_CONFIGS))
def test_door_capsule_runs(gpu, name):
  """runs of capsule blocks packed onto the 16 lanes (5 + 5 + 5 and a fourth that does not fit), capsule blocks of 16 and of 17 pairs, capsule / box / capsule in near
  order, a capsule block near without a hit, max_con inside a run; sphere rows on the door listed last (blocks beyond 16 pairs in the nv = 10 kernel)"""
  _, _, _, po = gpu
  scenes, max_con, door_rows, want_all = cc.DOOR_CONFIGS[name]
  d = cc.door_scene_table(scenes, max_con, door_rows)
  nhand = sum(len(sc[1]) for sc in scenes)
  hand = HAND if door_rows else NEAR3
  state = cc.door_states(d, 64, 15, hand_near=hand, door_near=LAST)
  want = [len([p for p in want_all if (hand[i] if p < nhand else LAST[i])]) for i in range(64)]
  if door_rows:
    assert want[0] == 0 and 0 < want[1] < want[3] and 0 < want[2] < want[3]
  assert want[0] == 0 and want[3] == len(want_all)
  device_equals_restatement(gpu, d, state, want)


def test_door_every_segment_kind(gpu):
  """the closest-point kinds of tests/test_collision_geometry.py (interior, endpoint projections, endpoint pairs, near-parallel on both sides of den = 1e-12, an edge that
  meets the capsule's axis) on the device"""
  cases = cc.door_segment_cases()
  for k in range(0, len(cases), 8):
    part = cases[k:k + 8]
    d = cc.door_scene_table([('capsule', [(c, e)], 1, 1) for _, c, e in part])
    state = cc.door_states(d, 64, 16 + k, hand_near=NEAR3)
    nhit = sum(label != 'meeting' for label, _, _ in part)
    device_equals_restatement(gpu, d, state, [nhit if NEAR3[i] else 0 for i in range(64)])

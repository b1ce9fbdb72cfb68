"""numpy/ctypes front-end of oracle/physics_oracle.c (TEST INFRASTRUCTURE, NOT PRODUCT): the C restatement of the
articulated-body stepper and of the Sawyer door env loop, on host arrays.  PARITY WITH MUJOCO UNPINNED.
The model structs are the public ones of include/earl_physics.h, filled by earl_benchmark_amd.physics from the .npz tables."""
import ctypes as C

import numpy as np

from oracle.tabletop_oracle import lib, _p


class CModel:
  def __init__(self, name='sawyer_door', contacts=True):
    """name: a shipped model, or a tables dict with the keys of its *_links.npz (earl_benchmark_amd.physics.load_link_model takes both)"""
    from earl_benchmark_amd import _abi, physics
    self._abi = _abi
    self.struct, self.tables = physics.load_link_model(name)
    self.col = physics.load_collision_model(self.tables) if contacts else None
    if not contacts:
      for j in range(physics.MAXV):
        self.struct.drag_G[j] = 0.0
    self.nv, self.n_att, self.n_act = self.struct.nv, self.struct.n_att, self.struct.n_act
    self.att_names = [str(x) for x in self.tables['att_names']]

  def _col(self):
    return C.byref(self.col) if self.col is not None else None

  def run(self, qpos, qvel, mocap_pos, mocap_quat, ctrl, nsub=1, integrate=True):
    """-> dict(qpos, qvel, qacc, efc, att, ncon); qpos / qvel are copies advanced by nsub timesteps when integrate"""
    q, v = np.array(qpos, np.float64, ndmin=2), np.array(qvel, np.float64, ndmin=2)
    n = len(q)
    mp, mq, ct = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), (n, k))) for x, k in ((mocap_pos, 3), (mocap_quat, 4), (ctrl, self.n_act)))
    qacc, efc = np.zeros((n, self.nv)), np.zeros((n, 6 + 2 * self.nv))
    att, ncon = np.zeros((n, self.n_att, 3)), np.zeros(n, np.int32)
    fn = lib().oracle_physics24 if self.nv > 16 else lib().oracle_physics      # the kitchen's 24-dof table form / the Sawyer envs' 16-dof one
    fn(C.byref(self.struct), self._col(), C.c_int32(n), C.c_int32(nsub), C.c_int32(int(integrate)), _p(q), _p(v), _p(mp),
       _p(mq), _p(ct), _p(qacc), _p(efc), _p(att), _p(ncon))
    return dict(qpos=q, qvel=v, qacc=qacc, efc=efc, att=att, ncon=ncon)

  def sawyer_rollout(self, cfg_kwargs, qpos, qvel, mocap_pos, goal, steps_since_reset, actions, steps_since_goal_change=None, goal_table=None,
                     last_obs=None, fail_count=None, status=None):
    """the env loop of oracle/sawyer_oracle.py for a batch; arrays are updated in place; -> obs, reward, done, success
    (status [T, n] uint8, last_obs [n, 14], fail_count [n] int32: the failure guard's outputs / state, filled in place when given)"""
    a = self._abi
    T, n = actions.shape[:2]
    cfg = a.SawyerCfg(n=n, **{k: v for k, v in cfg_kwargs.items() if not isinstance(v, (tuple, list, np.ndarray))})
    for k, v in cfg_kwargs.items():
      if isinstance(v, (tuple, list, np.ndarray)):
        getattr(cfg, k)[:] = [float(x) for x in v]
    st = a.SawyerState(qpos=qpos.ctypes.data, qvel=qvel.ctypes.data, mocap_pos=mocap_pos.ctypes.data, goal=goal.ctypes.data,
                       steps_since_reset=steps_since_reset.ctypes.data,
                       steps_since_goal_change=None if steps_since_goal_change is None else steps_since_goal_change.ctypes.data,
                       last_obs=None if last_obs is None else last_obs.ctypes.data, fail_count=None if fail_count is None else fail_count.ctypes.data)
    if goal_table is not None:
      self._gt = np.ascontiguousarray(goal_table, np.float64)
      cfg.goal_table, cfg.n_goal_rows = self._gt.ctypes.data, len(self._gt)
    obs, rew = np.zeros((T, n, 14)), np.zeros((T, n), np.float32)
    done, suc = np.zeros((T, n), np.uint8), np.zeros((T, n), np.uint8)
    out = a.SawyerOut(obs=obs.ctypes.data, reward=rew.ctypes.data, done=done.ctypes.data, success=suc.ctypes.data,
                      status=None if status is None else status.ctypes.data)
    acts = np.ascontiguousarray(actions, np.float32)
    lib().oracle_sawyer_rollout(C.byref(self.struct), self._col(), C.byref(cfg), C.byref(st), _p(acts), C.c_int32(T), C.byref(out))
    return obs, rew, done.astype(bool), suc.astype(bool)


class CMinitaur:
  """host-array batch of minitaur envs on the C restatement (oracle_minitaur_reset / oracle_minitaur_rollout): the same call sequence and state
  layout as earl_benchmark_amd.envs.minitaur.Minitaur drives through the HIP library"""

  def __init__(self, n, seed=0, env_offset=0, randomize=True, horizon=0, contacts=True, goal_change_frequency=0, model='minitaur'):
    from earl_benchmark_amd.envs import minitaur as mt
    self.cm = CModel(model, contacts=contacts)
    self.n = n
    self.goal_table = np.ascontiguousarray(mt.GOAL_LOCATIONS, np.float64)
    self.reset_qpos = np.ascontiguousarray(self.cm.tables['qpos0'], np.float64)
    self.cfg = mt.make_cfg(self.cm.tables, n=n, env_offset=env_offset, horizon=horizon, randomize=randomize, seed=seed,
                           goal_table_ptr=self.goal_table.ctypes.data, reset_qpos_ptr=self.reset_qpos.ctypes.data)
    self.cfg.goal_change_frequency = goal_change_frequency
    self.qpos, self.qvel = np.zeros((n, 23)), np.zeros((n, 22))
    self.goal, self.motor_param = np.zeros((n, 2)), np.tile([16.0, 0.0, 1.0, 1.0, 1.0, -1.0], (n, 1))
    self.observed_torque, self.overheat, self.motor_enabled = np.zeros((n, 8)), np.zeros((n, 8), np.int32), np.ones((n, 8), np.uint8)
    self.steps_since_reset, self.steps_since_goal_change, self.fail_count = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    self.last_obs = np.zeros((n, 32))
    self.counter, self.total_steps = 0, 0

  def _state(self):
    a = self.cm._abi
    return a.MinitaurState(**{k: getattr(self, k).ctypes.data for k in ('qpos', 'qvel', 'goal', 'motor_param', 'observed_torque', 'overheat', 'motor_enabled',
                                                                        'steps_since_reset', 'steps_since_goal_change', 'fail_count', 'last_obs')})

  def reset(self, mask=None):
    obs = self.last_obs.copy()
    st = self._state()
    self.cfg.counter = self.counter
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    lib().oracle_minitaur_reset(C.byref(self.cm.struct), self.cm._col(), C.byref(self.cfg), C.byref(st), _p(m), _p(obs))
    self.counter += 1
    return obs

  def rollout(self, actions):
    acts = np.ascontiguousarray(actions, np.float32)
    T = acts.shape[0]
    assert acts.shape == (T, self.n, 8)
    obs, rew = np.zeros((T, self.n, 32)), np.zeros((T, self.n))
    done, suc, status = np.zeros((T, self.n), np.uint8), np.zeros((T, self.n), np.uint8), np.zeros((T, self.n), np.uint8)
    out = self.cm._abi.MinitaurOut(obs=obs.ctypes.data, reward=rew.ctypes.data, done=done.ctypes.data, success=suc.ctypes.data, status=status.ctypes.data)
    st = self._state()
    self.cfg.step_counter = self.total_steps
    lib().oracle_minitaur_rollout(C.byref(self.cm.struct), self.cm._col(), C.byref(self.cfg), C.byref(st), _p(acts), C.c_int32(T), C.byref(out))
    self.total_steps += T
    return dict(obs=obs, reward=rew, done=done.astype(bool), success=suc.astype(bool), status=status)


def set_threads(n):
  return int(lib().oracle_set_physics_threads(C.c_int(int(n))))


def door_cfg(reward_type='sparse', reset_at_goal=False, horizon=0, att_names=None):
  names = att_names
  hand_init = np.array([0.29, 0.74, 0.1] if reset_at_goal else [0, 0.4, 0.2], np.float32).astype(np.float64)
  return dict(env_offset=0, reward_type=0 if reward_type == 'sparse' else 1, horizon=horizon, frame_skip=5, att_hand=names.index('hand'),
              att_right=names.index('rightEndEffector'), att_left=names.index('leftEndEffector'), att_obj=names.index('handle'), obj_dof=9,
              action_scale=1.0 / 100, mocap_low=(-0.5, 0.40, 0.05), mocap_high=(0.5, 1.0, 0.5), mocap_quat=(1.0, 0.0, 1.0, 0.0),
              success_radius=0.02, hand_init_pos=hand_init, obj_init_pos=np.array([0.1, 0.95, 0.1], np.float32).astype(np.float64),
              obj_init_angle=0.0, angle_noise=(0.0, 0.0), seed=0, counter=0)


def peg_cfg(horizon=0, att_names=None):
  """earl_sawyer_cfg fields of the sawyer_peg task (sparse reward, reset ranges of the default reset_model)"""
  names = att_names
  return dict(env_offset=0, reward_type=0, horizon=horizon, frame_skip=5, att_hand=names.index('hand'), att_right=names.index('rightEndEffector'),
              att_left=names.index('leftEndEffector'), att_obj=names.index('pegHead'), obj_dof=9, obj_kind=1, n_goal_rows=0,
              action_scale=1.0 / 100, mocap_low=(-0.5, 0.40, 0.05), mocap_high=(0.5, 1.0, 0.5), mocap_quat=(1.0, 0.0, 1.0, 0.0),
              success_radius=0.05, hand_init_pos=(0.0, 0.6, 0.2), obj_init_pos=(0.0, 0.6, 0.02), obj_low=(0.0, 0.5, 0.02),
              obj_high=(0.2, 0.7, 0.02), obj_reject_xy=(-0.3, 0.6), obj_reject_radius=0.1, seed=0, counter=0)

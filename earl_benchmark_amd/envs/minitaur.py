"""Batched, GPU-resident counterpart of the reference's minitaur env (BASELINE configs[4]).

Mirrors `GoalConditionedMinitaurBulletEnv` (reference: earl_benchmark/envs/minitaur_gym_env.py:466-546 on MinitaurBulletEnv :56-464 and
envs/minitaur.py: Minitaur): `reset`, `step`, `reset_goal`, `get_next_goal`, `compute_reward`, `is_successful`, `_get_obs`, the observation layout
(motor angles 8, velocities 8, torques 8, base orientation 4 (x, y, z, w), base xy 2, goal 2), dense reward, `done` never set by the env -- for
`num_envs` independent instances, one env step = ONE kernel launch (earl_minitaur_rollout with T = 1; `rollout` fuses T steps).

The numpy the reference wraps around Bullet is followed line by line in the kernel (leg model, velocity-limited commands, DC-motor model with
overheat protection, reward, success; the first three are pinned bit-exact by tests/test_glue*.py against goldens recorded from the reference's own
functions).  **THE RIGID-BODY PART IS UNPINNED AND MODEL-LESS**: the reference simulates pybullet_data's minitaur.urdf in PyBullet 3.2.0, neither of
which is in its tree; the robot model here (tools/minitaur_model.py: 22 dofs, four loop closures, spheres against the ground and the wall tiles) is
this build's own authoring on this build's own stepper (MuJoCo-style soft constraints, not Bullet's sequential-impulse solver).  The env randomizer
[UPSTREAM pybullet_envs.bullet.minitaur_env_randomizer, restated from memory] is built in the reset kernel: battery voltage, motor damping, base /
leg-link / motor masses, foot friction, through the semantics of the reference's own setters (envs/minitaur.py:468-508).  DESIGN.md section 14.
"""
import ctypes as C

import numpy as np
import torch

from .. import _abi, physics
from ..spaces import Box
from . import physics_policy_rollout as closed_loop
from .physics_env import PhysicsEnv

INT32_MAX = 2**31 - 1
NUM_SUBSTEPS, SETTLE_STEPS = 5, 100                       # minitaur_gym_env.py:25, 161-164; :265-269
MOTOR_KP, MOTOR_KD, MOTOR_VELOCITY_LIMIT = 1.0, 0.02, 150.0   # :85-86, :472
DISTANCE_WEIGHT, ENERGY_WEIGHT = 2.0, 0.005               # :473, :71
OVERHEAT_SHUTDOWN_TORQUE, OVERHEAT_SHUTDOWN_TIME = 2.45, 1.0   # minitaur.py:14-15
ACTION_BOUND, ACTION_EPS = 1.0, 0.01                      # minitaur_gym_env.py:144, 30
GOAL_LOCATIONS = np.array([[0.4, 0.2], [0.2, 0.2], [-0.2, 0.2], [-0.4, 0.2], [0.4, 0.0], [0.2, 0.0], [-0.2, 0.0], [-0.4, 0.0],
                           [0.4, 0.4], [0.2, 0.4], [-0.2, 0.4], [-0.4, 0.4]])   # :467-469
OBS_DIM, ACT_DIM = 32, 8
BASE_MASS_ERR, LEG_MASS_ERR, FOOT_FRICTION = (-0.2, 0.2), (-0.2, 0.2), (0.8, 1.5)   # [UPSTREAM] the randomizer's ranges
N_PARAM = 6                                              # earl_minitaur_state.motor_param row: voltage, damping, three mass factors, foot friction


def make_cfg(tables, n=0, env_offset=0, horizon=0, randomize=True, seed=0, goal_table_ptr=None, reset_qpos_ptr=None):
  """struct earl_minitaur_cfg from the model tables (shared with the oracle's front end, which passes host pointers)"""
  dt = float(tables['timestep'])
  cfg = _abi.MinitaurCfg(n=n, env_offset=env_offset, horizon=horizon, num_substeps=NUM_SUBSTEPS, settle_steps=SETTLE_STEPS, randomize=(7 if randomize is True else (int(randomize) if randomize else 0)),
                         n_goals=len(GOAL_LOCATIONS), goal_change_frequency=0, overheat_steps=int(OVERHEAT_SHUTDOWN_TIME / dt),
                         motor_kp=MOTOR_KP, motor_kd=MOTOR_KD, motor_velocity_limit=MOTOR_VELOCITY_LIMIT, overheat_torque=OVERHEAT_SHUTDOWN_TORQUE,
                         distance_weight=DISTANCE_WEIGHT, energy_weight=ENERGY_WEIGHT, success_radius=0.1, goal_table=goal_table_ptr,
                         reset_qpos=reset_qpos_ptr, seed=int(seed) & (2**64 - 1), counter=0, step_counter=0)
  cfg.motor_dof[:] = [int(x) for x in tables['motor_dof']]
  cfg.base_mass_err[:], cfg.leg_mass_err[:], cfg.foot_friction[:] = BASE_MASS_ERR, LEG_MASS_ERR, FOOT_FRICTION
  cfg.leg_mass, cfg.motor_mass = float(tables['rand_leg_mass']), float(tables['rand_motor_mass'])
  cfg.motor_dir[:] = [float(x) for x in tables['motor_direction']]
  return cfg


class _Cfg(_abi.MinitaurCfg):
  pass


class Minitaur(PhysicsEnv):
  OBS_DIM, ACT_DIM, NV, NQ = OBS_DIM, ACT_DIM, 22, 23
  ENV, _OUT_STRUCT = 'the minitaur', _abi.MinitaurOut
  _BOUNDED = ACTION_BOUND + ACTION_EPS                     # minitaur_gym_env.py:276-281: the reference raises outside it, so a policy's output is bounded
  _PAIR_LIFELONG = 'a LifelongWrapper (goal_change_frequency > 0)'
  _graph_bounds = (-ACTION_BOUND - ACTION_EPS, ACTION_BOUND + ACTION_EPS)      # (flagged per step, see _actions)
  _STATE = ('qpos', 'qvel', 'goal_t', 'motor_param', 'observed_torque', 'overheat', 'motor_enabled', 'steps_since_reset', 'steps_since_goal_change',
            'interventions', 'fail_count', 'lifelong_return_t', 'last_obs')

  def __init__(self, num_envs=1, device='cuda', seed=0, env_offset=0, scalar_api=None, env_randomizer=True, contacts=True, reset_at_goal=False,
               auto_reset=False, reward_type='dense', model='minitaur'):
    """model: the shipped tables' name, or a tables dict with the keys of minitaur_links.npz (tests: synthetic collision tables), passed to physics.DeviceModel"""
    if auto_reset or reset_at_goal:
      raise NotImplementedError('minitaur: auto_reset / reset_at_goal do not exist in the reference env')
    del reward_type                                          # (the reference's env has one reward: the loader's reward_type is not passed to it)
    self._lib = _abi.load()
    dev = torch.device(device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
      raise _abi.EarlHipError(f'device={device!r}: the minitaur env runs on MI355X only (no CPU fallback)')
    if dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    self.device, self.num_envs = dev, int(num_envs)
    n = self.num_envs
    self.scalar_api = (n == 1) if scalar_api is None else bool(scalar_api)
    if self.scalar_api and n != 1:
      raise ValueError('scalar_api needs num_envs == 1')
    with torch.cuda.device(dev):
      self.model = physics.DeviceModel(model, device=dev, contacts=contacts)
    assert self.model.nv == self.NV and self.model.nq == self.NQ
    kw = dict(dtype=torch.float64, device=dev)
    self.qpos, self.qvel = torch.zeros(n, self.NQ, **kw), torch.zeros(n, self.NV, **kw)
    self.goal_t = torch.tensor(GOAL_LOCATIONS[0], **kw).repeat(n, 1).contiguous()
    self.motor_param = torch.tensor([16.0, 0.0, 1.0, 1.0, 1.0, -1.0], **kw).repeat(n, 1).contiguous()   # [n, N_PARAM], written by the reset kernel
    self.observed_torque = torch.zeros(n, 8, **kw)
    self.overheat = torch.zeros(n, 8, dtype=torch.int32, device=dev)
    self.motor_enabled = torch.ones(n, 8, dtype=torch.uint8, device=dev)
    self.steps_since_reset = torch.zeros(n, dtype=torch.int32, device=dev)
    self.steps_since_goal_change = torch.zeros(n, dtype=torch.int32, device=dev)
    self.interventions = torch.zeros(n, dtype=torch.int32, device=dev)
    self.fail_count = torch.zeros(n, dtype=torch.int32, device=dev)
    self.lifelong_return_t = torch.zeros(n, **kw)
    self.last_obs = torch.zeros(n, self.OBS_DIM, **kw)
    self.total_step_count = 0
    self._goal_table = torch.tensor(GOAL_LOCATIONS, **kw).contiguous()
    self._reset_qpos = torch.tensor(self.model.tables['qpos0'], **kw).contiguous()
    base = make_cfg(self.model.tables, n=n, env_offset=int(env_offset), horizon=INT32_MAX, randomize=env_randomizer, seed=seed,
                    goal_table_ptr=self._goal_table.data_ptr(), reset_qpos_ptr=self._reset_qpos.data_ptr())
    self._cfg = _Cfg.from_buffer_copy(base)
    self._st = _abi.MinitaurState(qpos=self.qpos.data_ptr(), qvel=self.qvel.data_ptr(), goal=self.goal_t.data_ptr(), motor_param=self.motor_param.data_ptr(),
                                  observed_torque=self.observed_torque.data_ptr(), overheat=self.overheat.data_ptr(), motor_enabled=self.motor_enabled.data_ptr(),
                                  steps_since_reset=self.steps_since_reset.data_ptr(), steps_since_goal_change=self.steps_since_goal_change.data_ptr(),
                                  fail_count=self.fail_count.data_ptr(), last_obs=self.last_obs.data_ptr())
    self.action_space = Box(-ACTION_BOUND, ACTION_BOUND, (ACT_DIM,), np.float32)     # minitaur_gym_env.py:175-178
    self.observation_space = Box(-np.inf, np.inf, (self.OBS_DIM,), np.float32)        # :179, :481-488
    self._counter = 0
    self._last_success = torch.zeros(n, dtype=torch.bool, device=dev)
    self.reset()
    self.interventions.zero_()

  # ------------------------------------------------------------------ gym-style API
  def reset(self, mask=None):
    """GoalConditionedMinitaurBulletEnv.reset (:476-479) of the (masked) envs -> obs [N, 32] (numpy [32] with scalar_api)"""
    n = self.num_envs
    with torch.cuda.device(self.device):
      m = None if mask is None else torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
      obs = self.last_obs.clone()
      self._cfg.counter = self._counter
      _abi.check(self._lib.earl_minitaur_reset(self.model.buf.data_ptr(), self.model.col_ptr, C.byref(self._cfg), C.byref(self._st),
                                               None if m is None else m.data_ptr(), obs.data_ptr(), self._stream()), 'earl_minitaur_reset')
      self.interventions += 1 if m is None else m.to(torch.int32)
      closed_loop.reset_pair_state(self, m)                # (a reset env starts with the forward agent)
    if m is None:
      self._last_obs_stale = False
    self._counter += 1
    return obs[0].cpu().numpy() if self.scalar_api else obs

  def _actions(self, a, lead):
    a = torch.as_tensor(np.asarray(a, dtype=np.float32) if not torch.is_tensor(a) else a, device=self.device).to(torch.float32)
    a = a.reshape(*lead, self.num_envs, ACT_DIM).contiguous()
    # minitaur_gym_env.py:276-281: `if not (-bound - eps <= a_i <= bound + eps): raise` -- the NEGATED in-range test, so a NaN raises too (the
    # mirrored out-of-range test let NaN through; the motor model then carried it into the state and the env sat in its failure guard)
    out_of_bounds = ~((a >= -ACTION_BOUND - ACTION_EPS) & (a <= ACTION_BOUND + ACTION_EPS))
    if bool(out_of_bounds.any()):
      bad = int(torch.nonzero(out_of_bounds.reshape(-1, ACT_DIM).any(0))[0])
      raise ValueError('{}th action out of bounds.'.format(bad))
    return a

  def rollout(self, actions, out=None):
    """T env steps in ONE launch: actions [T, N, 8] -> dict(obs [T,N,32], reward [T,N], done, success, status); bit-identical to T step() calls"""
    with torch.cuda.device(self.device):
      T = int(torch.as_tensor(actions).shape[0])
      a = self._actions(actions, (T,))
      res = out if out is not None else self._new_out((T,))
      self._cfg.step_counter = self.total_step_count
      if T > 0:
        _abi.check(self._lib.earl_minitaur_rollout(self.model.buf.data_ptr(), self.model.col_ptr, C.byref(self._cfg), C.byref(self._st), a.data_ptr(), T,
                                                   C.byref(self._out_struct(res)), self._stream()), 'earl_minitaur_rollout')
        closed_loop.finish(self, T, res['reward'], res['success'][-1])
    return res

  # ------------------------------------------------------------------ K action plans per env from the current state, and MPPI around them
  # (names of their own: rollout_branches / plan_mppi / plan_candidates / mpc_rollout / plan_cem / cem_candidates stay PhysicsEnv's refusals on this env, as
  # rollout_pair / evaluate_population stand beside rollout_agents / evaluate_policy)
  _WS_BYTES = {'branch': 'earl_minitaur_branch_ws_bytes', 'plan': 'earl_minitaur_plan_ws_bytes'}

  def _ws(self, kind, K, H=0):
    """the workspace (include/earl_physics.h: earl_minitaur_branch_ws) of a branch launch of K branches ('branch') or of a planner call ('plan': that block and the
    [K, H, N, 8] candidates behind it): one device block per kind, allocated at the first use, cached per (K, H) and grown when a larger one is asked for"""
    cache = self.__dict__.setdefault('_ws_cache', {})
    if (kind, K, H) not in cache:
      name, need = self._WS_BYTES[kind], C.c_int64(0)
      _abi.check(getattr(self._lib, name)(K, *(() if kind == 'branch' else (H,)), self.num_envs, C.byref(need)), name)
      block = cache.get(kind)
      if block is None or block.numel() * 8 < need.value:
        if block is not None:
          cache.setdefault('kept', []).append(block)         # (a captured graph may still hold the smaller block's address: it stays alive)
        block = cache[kind] = torch.empty(max(need.value, 8) // 8 + 1, dtype=torch.float64, device=self.device)
      cache[(kind, K, H)] = need.value
    block = cache[kind]
    return _abi.MinitaurBranchWs(base=block.data_ptr(), bytes=block.numel() * 8)

  def _branch_actions(self, a):
    """rollout's action check (it reads a flag back, so it raises on the host) -- but inside a captured region, where nothing can be read back: the kernel clips to the
    reference's bound there, as a captured step does"""
    if a.is_cuda and torch.cuda.is_current_stream_capturing():
      return a.to(torch.float32).contiguous()
    return self._actions(a, tuple(a.shape[:-2]))

  def branch_rollout(self, actions, K=None, clock=None):
    """K candidate action sequences of H steps scored per env FROM THE CURRENT STATE in one launch of the rollout kernel over K N virtual envs (include/earl_physics.h:
    earl_minitaur_branch_rollout): actions [K, H, N, 8] float32 -- or [H, N, 8] with K= for K replays of one block --
    -> {'ret' [K, N] float64, 'success' [K, N] bool (the success of step H - 1), 'first_success' [K, N] int32 (-1: none), 'last_obs' [K, N, 32] float64,
        'fail' [K, N] int32 (steps the failure guard rolled back)}.
    Row k is what rollout(actions[k]) would return next, reduced (ret = the float64 sum of its rewards, a rolled-back step adding 0), lifelong goal draws included:
    every branch of an env sees the env's own draws.  An action outside the reference's bound raises its '{}th action out of bounds.' as rollout does (not while the
    stream is being captured into a graph, where no flag can be read back: the kernel clips to that bound).  The env is left
    exactly as found -- state, motors, goals, counters, last_obs, fail_count: nothing happened to it.  clock: None, or the device address of the two uint64 words of
    earl_minitaur_rollout_clocked (a captured launch)."""
    a = torch.as_tensor(actions, device=self.device)
    n = self.num_envs
    if K is None:
      if a.dim() != 4 or a.shape[2] != n or a.shape[3] != ACT_DIM:
        raise ValueError(f'branch_rollout: actions must be [K, H, N, 8] = [K, H, {n}, 8], got {list(a.shape)} (one block for K branches: [H, {n}, 8] with K=)')
      K, H, stride = int(a.shape[0]), int(a.shape[1]), int(a.shape[1]) * n * ACT_DIM
      act = self._branch_actions(a)
    else:
      if a.dim() != 3 or a.shape[1] != n or a.shape[2] != ACT_DIM:
        raise ValueError(f'branch_rollout: with K= actions must be [H, N, 8] = [H, {n}, 8], got {list(a.shape)}')
      K, H, stride = int(K), int(a.shape[0]), 0
      act = self._branch_actions(a)
    if K < 1 or H < 1:                                                 # (the entry point writes nothing then: no branch, or no step to reduce)
      raise ValueError(f'branch_rollout: K = {K}, H = {H}: at least one branch of at least one step')
    if K * n > INT32_MAX:
      raise ValueError(f'branch_rollout: K N = {K * n} virtual envs do not fit one launch (at most {INT32_MAX})')
    kw = dict(device=self.device)
    res = {'ret': torch.empty(K, n, dtype=torch.float64, **kw), 'success': torch.empty(K, n, dtype=torch.bool, **kw),
           'first_success': torch.empty(K, n, dtype=torch.int32, **kw), 'last_obs': torch.empty(K, n, OBS_DIM, dtype=torch.float64, **kw),
           'fail': torch.empty(K, n, dtype=torch.int32, **kw)}
    summary = _abi.EpisodeSummary(ret=res['ret'].data_ptr(), success_last=res['success'].data_ptr(), first_success=res['first_success'].data_ptr())
    self._cfg.step_counter = self.total_step_count
    with torch.cuda.device(self.device):
      ws = self._ws('branch', K)
      _abi.check(self._lib.earl_minitaur_branch_rollout(self.model.buf.data_ptr(), self.model.col_ptr, C.byref(self._cfg), C.byref(self._st), K, H, act.data_ptr(), stride,
                                                        clock, C.byref(ws), C.byref(summary), res['last_obs'].data_ptr(), res['fail'].data_ptr(), self._stream()),
                 'earl_minitaur_branch_rollout')
    return res                                                         # (no counter, no interventions, no stale flag: the env has not moved)

  def _plan_mean(self, who, mean, horizon):
    n = self.num_envs
    if mean is None:
      if horizon is None:
        raise ValueError(f'{who}: give mean [H, N, 8] or horizon')
      return torch.zeros(int(horizon), n, ACT_DIM, dtype=torch.float32, device=self.device)
    m = torch.as_tensor(mean, device=self.device)
    if m.dim() != 3 or m.shape[1] != n or m.shape[2] != ACT_DIM or (horizon is not None and m.shape[0] != horizon):
      raise ValueError(f'{who}: mean must be [H, N, 8] = [{"H" if horizon is None else horizon}, {n}, 8], got {list(m.shape)}')
    return m.to(torch.float32).contiguous()                            # (the planner clips every word to +-1: a mean is not an action and raises nothing)

  def _plan_params(self, who, K, H, iterations, iteration0, sigma, temperature, noise_counter):
    s = torch.as_tensor(sigma, dtype=torch.float32).reshape(-1).tolist()
    if len(s) not in (1, ACT_DIM):
      raise ValueError(f'{who}: sigma is a number or eight, one per action dimension')
    if not float(temperature) > 0.0:
      raise ValueError(f'{who}: temperature = {temperature}: > 0')
    if not 1 <= int(K) <= _abi.MINITAUR_PLAN_MAX_K:
      raise ValueError(f'{who}: K = {K}: 1 .. {_abi.MINITAUR_PLAN_MAX_K} candidates per env (branch 0, the plan itself, included)')
    if int(H) < 1 or int(iterations) < 1:
      raise ValueError(f'{who}: H = {H}, iterations = {iterations}: at least one of each')
    nc = self.total_step_count if noise_counter is None else int(noise_counter)   # (None: the low word of the env's step count -- fresh noise per control step)
    return _abi.MinitaurPlanParams(K=int(K), H=int(H), iterations=int(iterations), iteration0=int(iteration0), sigma=(C.c_float * 8)(*(s * 8 if len(s) == 1 else s)),
                                   noise_counter=nc & 0xFFFFFFFF, inv_temperature=1.0 / float(temperature))

  def mppi_plan(self, mean=None, horizon=None, K=64, iterations=1, sigma=0.3, temperature=1.0, iteration0=0, noise_counter=None, clock=None, out=None):
    """`iterations` MPPI iterations on the device from the CURRENT state (include/earl_physics.h: earl_minitaur_plan_mppi): K candidates per env -- the mean plan itself
    and K - 1 copies with clipped Gaussian noise of scale `sigma` (a number or eight) -- scored by the branch launch exactly as branch_rollout scores them, the mean
    moved to their average under the weights exp((ret - max ret) / temperature), in integer sums.  Per iteration three launches (candidates, the branch launch,
    update); no allocation and no host synchronisation in the call once its workspace exists.  mean [H, N, 8] (None: zeros of [horizon, N, 8]; every word is clipped
    to +-1) ->
    {'plan' [H, N, 8] float32, 'ret' [K, N] float64 (the last iteration's returns), 'ret0' [iterations, N] float64 (the return of the plan entering each iteration),
     'best_ret' [N] float64, 'best_k' [N] int32 (mppi_candidates(...)[best_k] is that candidate), 'fail' [K, N] int32 (steps of the last iteration the failure guard
     rolled back: they count with reward 0, which on this env's negative reward is ABOVE an honest step)}.
    `noise_counter=None` takes the low 32 bits of env.total_step_count, so successive control steps draw fresh noise (a captured call replays the noise it was captured
    with); `iteration0` numbers the first iteration (iterations in one call == as many calls of one, numbered on).  `out`: an optional dict of preallocated tensors under
    the same keys; a key that is missing or None is not computed, except 'ret' (the branch launch writes it), which is then allocated; out['plan'] may be the `mean`
    tensor.  clock: as branch_rollout.  The env is left exactly as found."""
    who = 'mppi_plan'
    m = self._plan_mean(who, mean, horizon)
    n, H, K, I = self.num_envs, int(m.shape[0]), int(K), int(iterations)
    pp = self._plan_params(who, K, H, I, iteration0, sigma, temperature, noise_counter)
    if K * n > INT32_MAX:
      raise ValueError(f'{who}: K N = {K * n} virtual envs do not fit one launch (at most {INT32_MAX})')
    kw = dict(device=self.device)
    want = {'plan': ((H, n, ACT_DIM), torch.float32), 'ret': ((K, n), torch.float64), 'ret0': ((I, n), torch.float64), 'best_ret': ((n,), torch.float64),
            'best_k': ((n,), torch.int32), 'fail': ((K, n), torch.int32)}
    if out is None:
      res = {k: torch.empty(*shape, dtype=dt, **kw) for k, (shape, dt) in want.items()}
    else:
      if set(out) - set(want):
        raise ValueError(f'{who}: out holds {sorted(set(out) - set(want))}; the keys are {list(want)}')
      res = {k: t for k, t in out.items() if t is not None}
      for k, t in res.items():
        shape, dt = want[k]
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
          raise ValueError(f'out[{k!r}] must be contiguous {dt} {shape} on {self.device}')
      if 'plan' not in res:
        raise ValueError(f"{who}: out['plan'] is what the call computes")
      if 'ret' not in res:
        res['ret'] = torch.empty(*want['ret'][0], dtype=want['ret'][1], **kw)
    ptr = lambda k: None if res.get(k) is None else res[k].data_ptr()
    self._cfg.step_counter = self.total_step_count
    with torch.cuda.device(self.device):
      _abi.check(self._lib.earl_minitaur_plan_mppi(self.model.buf.data_ptr(), self.model.col_ptr, C.byref(self._cfg), C.byref(self._st), C.byref(pp), m.data_ptr(),
                                                   res['plan'].data_ptr(), res['ret'].data_ptr(), ptr('ret0'), ptr('best_ret'), ptr('best_k'), ptr('fail'), clock,
                                                   C.byref(self._ws('plan', K, H)), self._stream()), 'earl_minitaur_plan_mppi')
    return res                                                         # (no counter, no interventions, no stale flag: the env has not moved)

  def mppi_candidates(self, mean, K, sigma=0.3, iteration=0, noise_counter=None):
    """the K candidates of mppi_plan's iteration `iteration` around `mean` [H, N, 8], written out: [K, H, N, 8] float32, row 0 the clipped mean -- what branch_rollout
    takes (earl_minitaur_plan_candidates; mppi_plan runs the same kernel).  With mppi_plan's `noise_counter` (None: the env's step count, unchanged by mppi_plan) they
    are the candidates that call scored."""
    m = self._plan_mean('mppi_candidates', mean, None)
    H = int(m.shape[0])
    pp = self._plan_params('mppi_candidates', K, H, 1, 0, sigma, 1.0, noise_counter)
    act = torch.empty(int(K), H, self.num_envs, ACT_DIM, dtype=torch.float32, device=self.device)
    with torch.cuda.device(self.device):
      _abi.check(self._lib.earl_minitaur_plan_candidates(C.byref(self._cfg), C.byref(pp), int(iteration), m.data_ptr(), act.data_ptr(), self._stream()),
                 'earl_minitaur_plan_candidates')
    return act

  def mppi_control(self, T, plan=None, horizon=None, K=64, iterations=1, sigma=0.3, temperature=1.0, noise_counter=None):
    """T steps of receding-horizon MPPI control, DEFINED as this composition of public methods (one call each per control step; there is no fused launch):
        P = plan.clone()  (None: zeros of [horizon, N, 8]);  nc0 = noise_counter  (None: the low 32 bits of env.total_step_count at entry)
        for s in range(T):
          mppi_plan(P, K=, iterations=, sigma=, temperature=, noise_counter=(nc0 + s) mod 2^32, out={'plan': P, 'ret': <scratch>, 'ret0': ret0[s], 'best_ret': best_ret[s]})
          row s of the result = rollout(P[:1], out=<views of row s>);  actions[s] = P[0]
          P[t] <- P[t + 1] for t < H - 1  (the last row stays)
    -> rollout()'s dict with a leading [T] ('obs' [T, N, 32], 'reward', 'done', 'success', 'status' [T, N]) plus 'actions' [T, N, 8] float32, 'plan' [H, N, 8] (the
       shifted plan after the last step: what the next call continues from), 'ret0' [T, iterations, N] and 'best_ret' [T, N] float64.
    The loop adds no host synchronisation of its own (rollout's bounds check on the clipped plan row is the one each step has).  The env advances by T steps exactly
    as T calls of rollout advance it."""
    T = int(T)
    if T < 1:
      raise ValueError(f'mppi_control: T = {T}: at least one control step')
    P = self._plan_mean('mppi_control', plan, horizon).clone()
    n, H, K, I = self.num_envs, int(P.shape[0]), int(K), int(iterations)
    self._plan_params('mppi_control', K, H, I, 0, sigma, temperature, noise_counter)      # (the argument errors, before anything moves)
    nc0 = self.total_step_count if noise_counter is None else int(noise_counter)
    kw = dict(device=self.device)
    res = self._new_out((T,))
    rows = list(res)
    res.update(actions=torch.empty(T, n, ACT_DIM, dtype=torch.float32, **kw), ret0=torch.empty(T, I, n, dtype=torch.float64, **kw),
               best_ret=torch.empty(T, n, dtype=torch.float64, **kw))
    ret = torch.empty(K, n, dtype=torch.float64, **kw)
    for s in range(T):
      self.mppi_plan(P, K=K, iterations=I, sigma=sigma, temperature=temperature, noise_counter=(nc0 + s) & 0xFFFFFFFF,
                     out={'plan': P, 'ret': ret, 'ret0': res['ret0'][s], 'best_ret': res['best_ret'][s]})
      self.rollout(P[:1], out={k: res[k][s:s + 1] for k in rows})
      res['actions'][s].copy_(P[0])
      if H > 1:
        P[:-1] = P[1:].clone()
    res['plan'] = P
    return res

  @property
  def initial_states(self):
    """[1, 2]: where the reset pose stands (x, y), the goal row an AgentPair's backward_goal='initial' resolves to"""
    return self._reset_qpos[:2].cpu().numpy().reshape(1, 2)

  def _launch_policy(self, policy, head, obs0, T, out, summary=None, pair=None):
    """hook of physics_policy_rollout: earl_minitaur_population_rollout (a single policy: pop = NULL, which is earl_minitaur_policy_rollout bit for bit); `out` may
    lack any key, 'obs' included (the env's row of last_obs then carries the observation); summary: None or an _abi.EpisodeSummary; pair: None, or what
    physics_policy_rollout.pair_structs returns (earl_minitaur_agents_rollout)"""
    self._cfg.step_counter = self.total_step_count
    ptr = lambda k: None if out.get(k) is None else out[k].data_ptr()
    ref = lambda s: None if s is None else C.byref(s)
    o = self._out_struct(out)
    pop = getattr(policy, 'pop_struct', None)              # a PolicyPopulation: the env with global id g runs member g // envs_per_policy
    if pair is not None:
      with torch.cuda.device(self.device):
        _abi.check(self._lib.earl_minitaur_agents_rollout(self.model.buf.data_ptr(), self.model.col_ptr, C.byref(self._cfg), C.byref(self._st), C.byref(policy.struct),
                                                          C.byref(pair[0]), ref(pair[1]), ref(pair[2]), ref(head), obs0.data_ptr(), T, None, ptr('actions'), C.byref(o),
                                                          ref(summary), self._stream()), 'earl_minitaur_agents_rollout')
      return
    with torch.cuda.device(self.device):
      _abi.check(self._lib.earl_minitaur_population_rollout(self.model.buf.data_ptr(), self.model.col_ptr, C.byref(self._cfg), C.byref(self._st), C.byref(policy.struct),
                                                            ref(pop), ref(head), obs0.data_ptr(), T, None, ptr('actions'), C.byref(o), ref(summary), self._stream()),
                 'earl_minitaur_population_rollout')

  def step(self, action):
    """-> (obs [N,32], reward [N], done [N], info{success, status}); gym 4-tuple of numpy / python scalars with scalar_api"""
    res = self.rollout(torch.as_tensor(np.asarray(action, dtype=np.float32) if not torch.is_tensor(action) else action).reshape(1, self.num_envs, ACT_DIM))
    obs, rew, done, suc = res['obs'][0], res['reward'][0], res['done'][0], res['success'][0]
    if self.scalar_api:
      return obs[0].cpu().numpy(), float(rew[0]), bool(done[0]), {'success': float(suc[0])}
    return obs, rew, done, {'success': suc, 'status': res['status'][0]}

  # hook of PhysicsStepGraph: one captured step = the clocked T = 1 launch into the graph's output rows; an out-of-bounds action cannot raise inside the graph:
  # g.check_actions() raises the reference's ValueError after a replay
  def _graph_step(self, t, action, out, clock):
    self._cfg.step_counter = t                             # the goal-switch draws of the captured step t: clock[1] + t
    with torch.cuda.device(self.device):
      _abi.check(self._lib.earl_minitaur_rollout_clocked(self.model.buf.data_ptr(), self.model.col_ptr, C.byref(self._cfg), C.byref(self._st), action.data_ptr(), 1,
                                                         clock, C.byref(self._out_struct(out)), self._stream()), 'earl_minitaur_rollout_clocked')
      if int(self._cfg.goal_change_frequency) > 0:
        self.lifelong_return_t += out['reward'].reshape(1, -1).sum(0)

  def _graph_info(self, out):
    return {'success': out['success'], 'status': out['status']}

  def _get_obs_t(self):
    """_get_obs() as the [N, 32] tensor, whatever scalar_api says"""
    md, dr = torch.tensor([int(x) for x in self.model.tables['motor_dof']], device=self.device), torch.tensor(self.model.tables['motor_direction'], device=self.device)
    ang = self.qpos[:, md + 1] * dr
    vel = self.qvel[:, md] * dr
    q = self.qpos[:, 3:7]
    return torch.cat([ang, vel, self.observed_torque, q[:, 1:4], q[:, 0:1], self.qpos[:, 0:2], self.goal_t], 1)

  def _get_obs(self):
    """GetObservation + goal of the CURRENT state (:541-546): no simulation, the newest observed torques"""
    obs = self._get_obs_t()
    return obs[0].cpu().numpy() if self.scalar_api else obs

  get_obs = _get_obs

  def compute_reward(self, obs):
    """GoalConditionedMinitaurBulletEnv.compute_reward (:529-535)"""
    o = torch.as_tensor(obs, dtype=torch.float64, device=self.device).reshape(-1, self.OBS_DIM)
    dist = -(o[:, 28] - o[:, 30]).abs() - (o[:, 29] - o[:, 31]).abs()
    energy = (o[:, 8:16] * o[:, 16:24]).sum(1).abs() * float(self.model.tables['timestep'])
    r = DISTANCE_WEIGHT * dist - ENERGY_WEIGHT * energy
    return float(r[0]) if self.scalar_api else r

  def is_successful(self, obs=None):
    o = self._get_obs() if obs is None else obs
    o = torch.as_tensor(o, dtype=torch.float64, device=self.device).reshape(-1, self.OBS_DIM)
    s = ((o[:, 28:30] - o[:, 30:32]) ** 2).sum(1).sqrt() < 0.1                    # :495-503
    return float(s[0]) if self.scalar_api else s

  # ------------------------------------------------------------------ goals (:481-493)
  def get_next_goal(self):
    return GOAL_LOCATIONS[np.random.randint(len(GOAL_LOCATIONS))].copy()

  def reset_goal(self, goal=None, mask=None):
    g = self.get_next_goal() if goal is None else np.asarray(goal, np.float64)
    super().reset_goal(g[-2:] if g.shape[-1] == 30 else g, mask)                    # :484-487

"""Drivers of the physics envs' C entry points for tests/test_physics_abi_gpu.py (a plain module, imported by that file; no fixtures here).

- Banded buffers: every device buffer handed to an entry point is a view into a larger uint8 tensor with a guard band on each side, at least
  max(4 KiB, one [n, row] slice) and a multiple of 256 B, so the view keeps the alignment the kernels assume (float4 action loads).  A stray store lands
  in a band of the same allocation, where `Bands.check()` finds it.  Each case runs twice, with bands of 0x00 and of 0xFF bytes (NaN as doubles, 255 as
  flags): equal results show that nothing outside the given extents is read.
- Struct builders: the state of an env object copied into banded tensors, any optional pointer replaceable by NULL (`null=`), and direct calls of the
  plain and `_clocked` entry points.
- `form()`: one launch form set through the library's debug switches, the defaults restored in `finally`.
"""
import contextlib
import ctypes as C

import torch

from earl_benchmark_amd import _abi

ALIGN = 256
MIN_BAND = 4096
FILLS = (0x00, 0xFF)


def _up(x):
  return (x + ALIGN - 1) // ALIGN * ALIGN


class Bands:
  """the banded buffers of one run; `fill` is the byte every band holds"""

  def __init__(self, fill, device='cuda'):
    self.fill, self.device, self.bufs = fill, device, {}

  def new(self, name, shape, dtype, slice_elems, src=None, interior=0):
    """a [shape] view of `dtype` inside bands of max(4 KiB, slice_elems elements); filled from `src` or with the byte `interior`"""
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = item
    for s in shape:
      nbytes *= int(s)
    band = _up(max(MIN_BAND, int(slice_elems) * item))
    whole = torch.full((band + _up(nbytes) + band + ALIGN,), self.fill, dtype=torch.uint8, device=self.device)
    skip = (-whole.data_ptr()) % ALIGN                    # (the caching allocator's blocks are aligned already; a host tensor need not be)
    raw = whole[skip:skip + band + _up(nbytes) + band]
    raw[band:band + nbytes].fill_(interior)
    view = raw[band:band + nbytes].view(dtype).view(*shape)
    assert view.data_ptr() % ALIGN == 0
    if src is not None:
      view.copy_(src.reshape(shape))
    self.bufs[name] = (raw, band, nbytes, view)
    return view

  def like(self, name, src, slice_elems=None):
    """a banded copy of the tensor `src`; the default slice is the whole tensor (state rows [n, ...])"""
    return self.new(name, tuple(src.shape), src.dtype, src.numel() if slice_elems is None else slice_elems, src=src)

  def __getitem__(self, name):
    return self.bufs[name][3]

  def ptr(self, name, null=()):
    return None if name in null or name not in self.bufs else self.bufs[name][3].data_ptr()

  def check(self, what=''):
    """every band byte as it was filled (the slack that rounds a buffer up to 256 B counts as band)"""
    if torch.device(self.device).type == 'cuda':          # (bands in host memory: tests/tabletop_abi.py against libearl_host.so)
      torch.cuda.synchronize()
    for name, (raw, band, nbytes, _) in self.bufs.items():
      bad = torch.cat([raw[:band], raw[band + nbytes:]]) != self.fill
      assert not bool(bad.any()), f'{what}: {int(bad.sum())} band bytes of {name!r} changed (fill {self.fill:#x})'


def bits(x):
  if x.dtype == torch.float64:
    return x.contiguous().view(torch.int64)
  if x.dtype == torch.float32:
    return x.contiguous().view(torch.int32)
  return x


def same(a, b, what, atol=None):
  """bit for bit (NaNs included), or within atol with NaNs in the same places"""
  assert a.shape == b.shape and a.dtype == b.dtype, what
  if atol is None or not a.is_floating_point():
    eq = bits(a) == bits(b)
    if not bool(eq.all()):
      idx = torch.nonzero(~eq)[:3].tolist()
      raise AssertionError(f'{what}: {int((~eq).sum())} entries differ, first at {idx}')
    return
  na, nb = torch.isnan(a), torch.isnan(b)
  assert torch.equal(na, nb), f'{what}: NaNs differ'
  err = float((torch.nan_to_num(a) - torch.nan_to_num(b)).abs().max()) if a.numel() else 0.0
  assert err <= atol, f'{what}: {err} > {atol}'


def same_dicts(a, b, what, atol=None, skip=()):
  assert set(a) == set(b), (what, set(a) ^ set(b))
  for k in a:
    if k not in skip:
      same(a[k], b[k], f'{what} {k}', atol)


def stream():
  return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------- launch forms
_DEFAULTS = {'earl_debug_set_door_variant': 0, 'earl_debug_set_physics_lanes': 16, 'earl_debug_set_peg_schedule': 1, 'earl_debug_set_solo': -1,
             'earl_debug_set_solo_mt': -1, 'earl_debug_set_minitaur_duo': -1, 'earl_debug_set_minitaur_stepper': 1}


@contextlib.contextmanager
def form(**switches):
  """set the named debug switches (earl_debug_set_<name>=value) for the block; every switch back at its default afterwards"""
  lib = _abi.load()
  try:
    for k, v in switches.items():
      fn = 'earl_debug_set_' + k
      assert fn in _DEFAULTS, fn
      rc = getattr(lib, fn)(int(v))
      assert fn in ('earl_debug_set_solo', 'earl_debug_set_solo_mt', 'earl_debug_set_minitaur_duo') or rc == _abi.EARL_OK, (fn, v)
    yield
  finally:
    for fn, v in _DEFAULTS.items():
      getattr(lib, fn)(v)


# Forms per env: name -> (switches, envs per workgroup of that kernel: the first env of the last workgroup is (n - 1) // E * E).  None for E: decided by n
# (the automatic pick).
FORMS = {
    'door': {'auto': ({}, None), 'one_wave': ({'door_variant': 1}, 4), 'eight_wave': ({'door_variant': 2}, 32), 'sliced': ({'door_variant': 3}, 4),
             'lanes64': ({'physics_lanes': 64}, 1)},
    'peg': {'auto': ({}, None), 'static': ({'peg_schedule': 0}, 16), 'sliced3': ({'peg_schedule': 3}, 4), 'lanes64': ({'physics_lanes': 64}, 4)},
    'kitchen': {'auto': ({}, None), 'mode0': ({'solo': 0}, 8), 'mode1': ({'solo': 1}, 4), 'mode2': ({'solo': 2}, 1), 'mode3': ({'solo': 3}, 1),
                'mode4': ({'solo': 4}, 2)},
    'minitaur': {'auto': ({}, None), 'one_wave': ({'solo_mt': 0, 'minitaur_duo': 0}, 8), 'two_wave': ({'solo_mt': 0, 'minitaur_duo': 1}, 16),
                 'solo1': ({'solo_mt': 1}, 4), 'solo2': ({'solo_mt': 2}, 1), 'generic': ({'minitaur_stepper': 0}, None)},
}


def auto_envs_per_wg(kind, n, cus):
  """envs per workgroup of the kernel the launcher picks for a batch of n (physics.hip, physics_kitchen.hip, physics_mt.hip)"""
  if kind == 'door':
    return 32 if n > 4096 else 4
  if kind == 'peg':
    return 4 if (n + 15) // 16 > cus else 16          # (time-sliced: groups of four envs)
  if kind == 'kitchen':
    return 1 if n <= cus else (2 if n <= 2 * cus else (4 if n <= 4 * cus else 8))
  if n <= cus:
    return 1
  if n <= 4 * cus:
    return 4
  r1, r2 = (n + 8 * cus - 1) // (8 * cus), (n + 16 * cus - 1) // (16 * cus)
  return 16 if 16 * r2 < 10 * r1 else 8


def probe_envs(kind, n, cus, form_name='auto'):
  e = FORMS[kind][form_name][1] or auto_envs_per_wg(kind, n, cus)
  return sorted({0, n - 1, (n - 1) // e * e})


# ---------------------------------------------------------------------------------------------------- env objects
def make_env(kind, n, seed=3):
  if kind == 'door':
    from earl_benchmark_amd.envs.sawyer_door import SawyerDoor
    return SawyerDoor(num_envs=n, seed=seed, scalar_api=False)
  if kind == 'peg':
    from earl_benchmark_amd.envs.sawyer_peg import SawyerPeg
    return SawyerPeg(num_envs=n, seed=seed, scalar_api=False, reset_at_goal=True)      # 15 goal rows: a goal switch shows in the observation
  if kind == 'kitchen':
    from earl_benchmark_amd.envs.kitchen import Kitchen
    return Kitchen(num_envs=n, seed=seed, scalar_api=False, sensor_noise=False)
  from earl_benchmark_amd.envs.minitaur import Minitaur
  return Minitaur(num_envs=n, seed=seed, scalar_api=False)


A_DIM = {'door': 4, 'peg': 4, 'kitchen': 9, 'minitaur': 8}
OBS_DIM = {'door': 14, 'peg': 14, 'kitchen': 46, 'minitaur': 32}
SAWYER_STATE = (('qpos', 'qpos'), ('qvel', 'qvel'), ('mocap_pos', 'mocap_pos'), ('goal', 'goal_t'), ('steps_since_reset', 'steps_since_reset'),
                ('steps_since_goal_change', 'steps_since_goal_change'), ('obj_init', 'obj_init'), ('last_obs', 'last_obs'), ('fail_count', 'fail_count'))
KITCHEN_STATE = (('qpos', 'qpos'), ('qvel', 'qvel'), ('mocap_pos', 'mocap_pos'), ('goal', 'goal_t'), ('last_qp_robot', 'last_qp_robot'), ('att_xpos', 'att'),
                 ('steps_since_reset', 'steps_since_reset'), ('fail_count', 'fail_count'), ('last_obs', 'last_obs'))
KITCHEN_SCRATCH = ('action64', 'ctrl9', 'noise', 'qpos_bak', 'qvel_bak', 'sites', 'bad', 'mocap_bak', 'att_bak')
MINITAUR_STATE = (('qpos', 'qpos'), ('qvel', 'qvel'), ('goal', 'goal_t'), ('motor_param', 'motor_param'), ('observed_torque', 'observed_torque'),
                  ('overheat', 'overheat'), ('motor_enabled', 'motor_enabled'), ('steps_since_reset', 'steps_since_reset'),
                  ('steps_since_goal_change', 'steps_since_goal_change'), ('fail_count', 'fail_count'), ('last_obs', 'last_obs'))
OUTS = {'door': (('obs', torch.float64, 14), ('reward', torch.float32, 1), ('done', torch.uint8, 1), ('success', torch.uint8, 1), ('status', torch.uint8, 1),
                 ('info', torch.float64, _abi.SAWYER_INFO)),
        'kitchen': (('obs', torch.float64, 46), ('reward', torch.float64, 1), ('done', torch.uint8, 1), ('success', torch.uint8, 1), ('status', torch.uint8, 1)),
        'minitaur': (('obs', torch.float64, 32), ('reward', torch.float64, 1), ('done', torch.uint8, 1), ('success', torch.uint8, 1), ('status', torch.uint8, 1))}
OUTS['peg'] = OUTS['door']
STATE_FIELDS = {'door': SAWYER_STATE, 'peg': SAWYER_STATE, 'kitchen': KITCHEN_STATE, 'minitaur': MINITAUR_STATE}


class Snapshot:
  """the state of an env object (and anything a test writes into it), copied once; every run starts from these tensors"""

  def __init__(self, kind, env, gcf=0, sgc_pattern=True):
    self.kind, self.env, self.n = kind, env, env.num_envs
    self.state = {f: getattr(env, attr).clone() for f, attr in STATE_FIELDS[kind]}
    if kind in ('door', 'peg', 'minitaur'):
      self.gcf = gcf
      if sgc_pattern:                                    # envs at different distances from their next goal switch
        self.state['steps_since_goal_change'] = (torch.arange(self.n, device='cuda', dtype=torch.int32) % max(gcf, 1)).contiguous()
    self.step_counter = 1000 + 7 * self.n                 # (the goal-switch draws: some step other than 0)

  def poison(self, env_id):
    """a NaN in the env's velocity row: its first step diverges (arithmetic only, as in the failure-guard tests)"""
    self.state['qvel'][env_id, 1] = float('nan')


def _cfg_copy(kind, env):
  cls = type(env._cfg)
  return cls.from_buffer_copy(env._cfg)


def run(snap, acts, fill, null=(), clocked=None, with_scratch=False, info_fill=None):
  """one rollout of the snapshot's state through the env's C entry point, every buffer banded with `fill`.  null: state / out fields passed as NULL.
  clocked: None = the plain entry point, else (c0, c1) device clock words (the cfg counters lowered by them: same draws).  -> (results dict, Bands)"""
  kind, env, n = snap.kind, snap.env, snap.n
  T = int(acts.shape[0])
  b = Bands(fill)
  lib = env._lib
  for f, _ in STATE_FIELDS[kind]:
    src = snap.state[f]
    b.like('st.' + f, src)
  if kind in ('door', 'peg'):
    b.new('st.sched', (2 * ((n + 3) // 4),), torch.int32, 2 * ((n + 3) // 4))
  if kind == 'kitchen' and with_scratch:
    for k, v in env._scr.items():
      b.like('st.' + k, torch.zeros_like(v))
  b.like('act', acts, slice_elems=n * A_DIM[kind])
  for name, dt, row in OUTS[kind]:
    b.new('out.' + name, (T, n, row) if row > 1 else (T, n), dt, n * row)
  if info_fill is not None:
    info_fill(b['out.info'])
  clock = None
  cfg = _cfg_copy(kind, env)
  if kind != 'kitchen':
    cfg.goal_change_frequency = snap.gcf
    cfg.step_counter = snap.step_counter
  if clocked is not None:
    cw = b.new('clock', (2,), torch.int64, 2, src=torch.tensor(list(clocked), dtype=torch.int64, device='cuda'))
    clock = cw.data_ptr()
    cfg.counter = int(cfg.counter) - int(clocked[0])
    if kind != 'kitchen':
      cfg.step_counter = int(cfg.step_counter) - int(clocked[1])
  nullset = set(null)
  stp = {f: b.ptr('st.' + f, {'st.' + k for k in nullset}) for f, _ in STATE_FIELDS[kind]}
  outp = {name: b.ptr('out.' + name, {'out.' + k for k in nullset}) for name, _, _ in OUTS[kind]}
  m = env.model
  if kind in ('door', 'peg'):
    st = _abi.SawyerState(**stp, sched=b.ptr('st.sched', {'st.sched'} if 'sched' in nullset else ()))
    out = _abi.SawyerOut(**outp)
    args = (m.buf.data_ptr(), m.col_ptr, env.nv, C.byref(cfg), C.byref(st), b['act'].data_ptr(), T)
    rc = lib.earl_sawyer_rollout(*args, C.byref(out), stream()) if clock is None else lib.earl_sawyer_rollout_clocked(*args, clock, C.byref(out), stream())
  elif kind == 'kitchen':
    scr = {k: b.ptr('st.' + k) for k in KITCHEN_SCRATCH} if with_scratch else {}
    st = _abi.KitchenState(**stp, **scr)
    out = _abi.KitchenOut(**outp)
    args = (m.buf.data_ptr(), m.col_ptr, C.byref(env._params), C.byref(cfg), C.byref(st), b['act'].data_ptr(), T)
    rc = lib.earl_kitchen_rollout(*args, C.byref(out), stream()) if clock is None else lib.earl_kitchen_rollout_clocked(*args, clock, C.byref(out), stream())
  else:
    st = _abi.MinitaurState(**stp)
    out = _abi.MinitaurOut(**outp)
    args = (m.buf.data_ptr(), m.col_ptr, C.byref(cfg), C.byref(st), b['act'].data_ptr(), T)
    rc = lib.earl_minitaur_rollout(*args, C.byref(out), stream()) if clock is None else lib.earl_minitaur_rollout_clocked(*args, clock, C.byref(out), stream())
  _abi.check(rc, f'{kind} rollout')
  torch.cuda.synchronize()
  res = {k: v[3].clone() for k, v in b.bufs.items() if (k.startswith(('st.', 'out.')) and k != 'st.sched' and k[k.index('.') + 1:] not in nullset
                                                        and not (k.startswith('st.') and k[3:] in KITCHEN_SCRATCH))}
  return res, b


def run_both_fills(snap, acts, what, **kw):
  """the run with 0x00 and with 0xFF bands: bands intact in both, results equal bit for bit -> the results"""
  first = None
  for fill in FILLS:
    res, b = run(snap, acts, fill, **kw)
    b.check(f'{what} fill {fill:#x}')
    if first is None:
      first = res
    else:
      same_dicts(first, res, f'{what}: 0x00 bands vs 0xFF bands')
    del b
  return first


def actions(kind, T, n, seed):
  g = torch.Generator(device='cuda').manual_seed(seed)
  a = (torch.rand(T, n, A_DIM[kind], generator=g, device='cuda') * 2 - 1).to(torch.float32)
  return a.contiguous()


# ---------------------------------------------------------------------------------------------------- resets
def sawyer_reset(env, fill, mask=None, null=(), obs=True):
  """earl_sawyer_reset of the env's current state (copied into bands) -> (state dict, obs or None, Bands)"""
  n = env.num_envs
  b = Bands(fill)
  for f, attr in SAWYER_STATE:
    b.like('st.' + f, getattr(env, attr))
  if mask is not None:
    b.like('mask', mask)
  if obs:
    b.new('obs', (n, 14), torch.float64, n * 14)
  cfg = _cfg_copy('door', env)
  st = _abi.SawyerState(**{f: b.ptr('st.' + f, {'st.' + k for k in null}) for f, _ in SAWYER_STATE})
  q, v = env._reset_state
  rc = env._lib.earl_sawyer_reset(env.model.buf.data_ptr(), env.nv, C.byref(cfg), C.byref(st), q.data_ptr(), v.data_ptr(), b.ptr('mask'), b.ptr('obs'),
                                  stream())
  _abi.check(rc, 'sawyer reset')
  torch.cuda.synchronize()
  res = {k: v[3].clone() for k, v in b.bufs.items() if k.startswith('st.') and k[3:] not in null}
  return res, (b['obs'].clone() if obs else None), b


def minitaur_reset(env, fill, mask=None, null=(), obs=True):
  n = env.num_envs
  b = Bands(fill)
  for f, attr in MINITAUR_STATE:
    b.like('st.' + f, getattr(env, attr))
  if mask is not None:
    b.like('mask', mask)
  if obs:
    b.new('obs', (n, 32), torch.float64, n * 32)
  cfg = _cfg_copy('minitaur', env)
  cfg.counter = 5
  st = _abi.MinitaurState(**{f: b.ptr('st.' + f, {'st.' + k for k in null}) for f, _ in MINITAUR_STATE})
  rc = env._lib.earl_minitaur_reset(env.model.buf.data_ptr(), env.model.col_ptr, C.byref(cfg), C.byref(st), b.ptr('mask'), b.ptr('obs'), stream())
  _abi.check(rc, 'minitaur reset')
  torch.cuda.synchronize()
  res = {k: v[3].clone() for k, v in b.bufs.items() if k.startswith('st.') and k[3:] not in null}
  return res, (b['obs'].clone() if obs else None), b


def door_info(env, obs, status, info, gcf):
  """earl_sawyer_door_info over the [T, n] rows of a door rollout, in place on `info`"""
  cfg = _cfg_copy('door', env)
  cfg.goal_change_frequency = gcf
  rows = obs.shape[0] * obs.shape[1]
  rc = env._lib.earl_sawyer_door_info(C.byref(cfg), rows, obs.data_ptr(), None if status is None else status.data_ptr(), info.data_ptr(), stream())
  _abi.check(rc, 'door info')
  torch.cuda.synchronize()

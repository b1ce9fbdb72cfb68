"""The physics envs' C ABI at its edges (include/earl_physics.h), driven directly through tests/physics_abi.py: every buffer inside guard bands that must
stay untouched, and every run repeated with bands of 0x00 and 0xFF bytes that must not change a bit of the results.

- Launch forms at the launchers' own thresholds (physics.hip: door eight-wave for n > 4096, peg time-sliced for ceil(n / 16) > CUs; physics_kitchen.hip and
  physics_mt.hip: solo_mode at CUs and 4 x CUs, the kitchen's two-envs-per-workgroup form up to 2 x CUs, the minitaur's two-wave form by rounds of 8 / 16 x CUs):
  each size under every form the env offers equals the automatic pick bit for bit (the generic minitaur stepper: to 1e-8, as in tests/test_minitaur_gpu.py),
  and envs 0, n - 1 and the first env of the last workgroup match the C statement for one step from the same state.
- The failure guard on the clamped tail env of a ragged launch: a duplicate lane that stored would count a rolled-back step twice.
- Optional pointers set to NULL one at a time and all at once (the guard each relies on is named in the test), with one env diverging.
- Stale goal-switch markers in the door's info buffer.
"""
import ctypes as C

import numpy as np
import pytest

import physics_abi as pa

pytestmark = pytest.mark.gpu

GCF = 2              # goal switching on (Sawyer, minitaur): every second step, from envs at different distances to their next switch
T_OF = {'door': 4, 'peg': 4, 'kitchen': 3, 'minitaur': 4}


def cus():
  import torch
  return torch.cuda.get_device_properties(0).multi_processor_count


def sizes(kind, c):
  return {'door': [1, 3, 5, 4096, 4097],
          'peg': [1, 16 * c, 16 * c + 1],
          'kitchen': [1, c, c + 1, 2 * c, 2 * c + 1, 4 * c, 4 * c + 1],
          'minitaur': [1, 4 * c, 4 * c + 1, 8 * c, 8 * c + 1, 16 * c + 1, 24 * c + 1, 16 * (6 * c // 16 + 1) + 1]}[kind]


def env_actions(kind, T, n):
  """actions that depend on (step, env, component) only, not on the batch size: env e sees the same actions at every size"""
  import torch
  t = torch.arange(T, device='cuda', dtype=torch.float64)[:, None, None]
  e = torch.arange(n, device='cuda', dtype=torch.float64)[None, :, None]
  k = torch.arange(pa.A_DIM[kind], device='cuda', dtype=torch.float64)[None, None, :]
  x = torch.sin(12.9898 * (e + 1) + 78.233 * (k + 1) + 37.719 * (t + 1)) * 43758.5453
  return ((x - torch.floor(x)) * 2 - 1).to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------------- the C statement, one step
_ORACLE = {}


def oracle_step(kind, snap, acts, i):
  """one env step of env i from the snapshot's state on the C / numpy statement -> dict(obs, reward, done, success) of that row"""
  import torch
  st = {k: v[i:i + 1].cpu().numpy().copy() for k, v in snap.state.items()}
  a = acts[0:1, i:i + 1].cpu().numpy()
  env = snap.env
  if kind in ('door', 'peg'):
    from oracle import physics_c
    name = 'sawyer_door' if kind == 'door' else 'sawyer_peg'
    if name not in _ORACLE:
      _ORACLE[name] = physics_c.CModel(name)
    cm = _ORACLE[name]
    cfg = env._cfg
    kw = {}
    for f, _ in type(cfg)._fields_:
      if f in ('n', 'goal_table', 'wide_table', 'box_corners', 'pad2_', 'n_goal_rows'):
        continue
      v = getattr(cfg, f)
      kw[f] = tuple(v) if isinstance(v, C.Array) else v
    kw.update(env_offset=int(cfg.env_offset) + i, goal_change_frequency=snap.gcf, step_counter=snap.step_counter)
    ob, rew, done, suc = cm.sawyer_rollout(kw, st['qpos'], st['qvel'], st['mocap_pos'], st['goal'], st['steps_since_reset'], a,
                                           steps_since_goal_change=st['steps_since_goal_change'], goal_table=env._goal_table.cpu().numpy())
    return dict(obs=ob[0, 0], reward=float(rew[0, 0]), done=bool(done[0, 0]), success=bool(suc[0, 0]))
  if kind == 'kitchen':
    from conftest import load_golden
    from oracle import glue_oracle as go
    from oracle.kitchen_oracle import KitchenOracle
    key = ('kitchen', i) + tuple(np.concatenate([st[k].ravel() for k in ('qpos', 'qvel', 'mocap_pos', 'goal', 'last_qp_robot')]).tolist()) + tuple(a.ravel().tolist())
    if key not in _ORACLE:                                 # (env i starts from the same state with the same action at every size: one numpy step each)
      if 'kitchen!' not in _ORACLE:
        g = load_golden('kitchen_step')
        _ORACLE['kitchen!'] = KitchenOracle(go.kitchen_params(g['kitchen_pos_bound'], g['kitchen_vel_bound'], g['kitchen_pos_noise_amp']))
      ref = _ORACLE['kitchen!']
      ref.set(st['qpos'][0], st['qvel'][0], st['mocap_pos'][0], st['goal'][0], st['last_qp_robot'][0])
      o, r, s, _ = ref.step(a[0, 0])
      _ORACLE[key] = dict(obs=o, reward=r, done=False, success=s)
    return _ORACLE[key]
  from oracle import physics_c
  c = physics_c.CMinitaur(1, seed=int(env._cfg.seed), env_offset=int(env._cfg.env_offset) + i, goal_change_frequency=snap.gcf)
  c.cfg.horizon = int(env._cfg.horizon)
  for f, _ in pa.MINITAUR_STATE:
    getattr(c, f)[...] = st[f].reshape(getattr(c, f).shape)
  c.total_steps = snap.step_counter
  r = c.rollout(a)
  return dict(obs=r['obs'][0, 0], reward=float(r['reward'][0, 0]), done=bool(r['done'][0, 0]), success=bool(r['success'][0, 0]))


OBS_TOL = {'door': 2e-6, 'peg': 2e-6, 'kitchen': 1e-6, 'minitaur': 1e-6}


def check_against_oracle(kind, snap, acts, res, envs, what):
  worst = 0.0
  for i in envs:
    want = oracle_step(kind, snap, acts, i)
    got = res['out.obs'][0, i].cpu().numpy()
    err = float(np.abs(got - want['obs']).max())
    assert err < OBS_TOL[kind], f'{what} env {i}: obs off the C statement by {err}'
    worst = max(worst, err)
    r = float(res['out.reward'][0, i])
    if kind in ('door', 'peg'):
      assert r == want['reward'], (what, i, r, want['reward'])
    else:
      assert abs(r - want['reward']) < 1e-6 * max(1.0, abs(want['reward'])), (what, i, r, want['reward'])
    assert bool(res['out.success'][0, i]) == want['success'], (what, i)
    assert bool(res['out.done'][0, i]) == want['done'], (what, i)
  return worst


def snapshot(kind, n, seed=3, gcf=GCF):
  env = pa.make_env(kind, n, seed=seed)
  return pa.Snapshot(kind, env, gcf=0 if kind == 'kitchen' else gcf)


# ---------------------------------------------------------------------------------------------------- launch forms at the thresholds
@pytest.mark.parametrize('kind', ['door', 'peg', 'kitchen', 'minitaur'])
def test_every_launch_form_at_the_launcher_thresholds(kind):
  """per size: the automatic pick through the plain entry point; every forced form through the clocked one (clock words {3, 5}, the cfg counters lowered by
  as much: the same draws).  Bit-identical results, bands intact under both fills, three envs against the C statement."""
  import torch
  c = cus()
  T = T_OF[kind]
  for n in sizes(kind, c):
    snap = snapshot(kind, n)
    acts = env_actions(kind, T, n)
    with pa.form():
      ref = pa.run_both_fills(snap, acts, f'{kind} n={n} auto')
    probes = pa.probe_envs(kind, n, c)
    err = check_against_oracle(kind, snap, acts, ref, probes, f'{kind} n={n} auto')
    for name, (switches, _) in pa.FORMS[kind].items():
      if name == 'auto':
        continue
      what = f'{kind} n={n} {name}'
      with pa.form(**switches):
        res = pa.run_both_fills(snap, acts, what, clocked=(3, 5))
      pa.same_dicts(ref, res, what + ' vs auto', atol=1e-8 if name == 'generic' else None)
    print(f'{kind}: {c} CUs, n = {n}, T = {T}: forms {list(pa.FORMS[kind])} equal; envs {probes} off the C statement by {err:.2e}; '
          f'{int(ref["out.status"].sum())} rolled-back steps')
    if kind == 'peg' and n > 1:
      assert bool((ref['out.obs'][1:, :, 7:] != ref['out.obs'][:-1, :, 7:]).any())      # (a goal switch drew a new row: the draws are compared too)
    del snap, ref
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- the failure guard on the tail env
def ragged_size(kind, c):
  return {'door': 5, 'peg': 16 * c + 1, 'kitchen': 9, 'minitaur': 17}[kind]


@pytest.mark.parametrize('kind', ['door', 'peg', 'kitchen', 'minitaur'])
def test_failure_guard_on_the_clamped_tail_env(kind):
  """env n - 1 of a ragged launch (the env the idle lanes of its workgroup shadow) poisoned with a NaN velocity: every one of its T steps is rolled back and
  counted ONCE in fail_count; every other env's outputs and state equal the unpoisoned run bit for bit.  Under every form."""
  c = cus()
  n, T = ragged_size(kind, c), T_OF[kind]
  acts = env_actions(kind, T, n)
  clean, bad = snapshot(kind, n, gcf=0), snapshot(kind, n, gcf=0)      # (no goal switch: every rolled-back row is the last stable observation as it was)
  bad.poison(n - 1)
  f0 = int(bad.state['fail_count'][n - 1])
  for name, (switches, _) in pa.FORMS[kind].items():
    what = f'{kind} n={n} {name} poisoned tail'
    with pa.form(**switches):
      want = pa.run_both_fills(clean, acts, what + ' (clean)')
      got = pa.run_both_fills(bad, acts, what)
    st = got['out.status'][:, n - 1]
    assert st.tolist() == [1] * T, (what, st.tolist())
    assert int(got['st.fail_count'][n - 1]) == f0 + T, (what, int(got['st.fail_count'][n - 1]), f0 + T)
    last = bad.state['last_obs'][n - 1]
    for t in range(T):
      pa.same(got['out.obs'][t, n - 1], last, f'{what} row {t}: the last stable observation')
      assert float(got['out.reward'][t, n - 1]) == 0.0 and int(got['out.success'][t, n - 1]) == 0, what
    for k in got:
      other = (lambda x: x[:, :n - 1]) if k.startswith('out.') else (lambda x: x[:n - 1])
      pa.same(other(got[k]), other(want[k]), f'{what}: {k} of the other envs')
    # the rolled-back steps still count for the horizon
    pa.same(got['st.steps_since_reset'], want['st.steps_since_reset'], what + ' steps_since_reset')
    pa.same(got['out.done'], want['out.done'], what + ' done')


# ---------------------------------------------------------------------------------------------------- optional pointers
OPTIONAL = {
    # Sawyer (physics_env_sawyer.h): steps_since_goal_change -- gcf = st.steps_since_goal_change ? ... : 0 (:249), and gcf > 0 guards :266, :371;
    # obj_init -- `a.st.obj_init ? ... : nullptr` (:300), peg_terms needs obj_init != nullptr (sawyer_emit :178; the peg's out.info then goes NULL with
    # it: the launcher refuses the pair); last_obs -- `a.st.last_obs ? ... : nullptr` then NaN (:324-325), `a.st.last_obs &&` (:369); fail_count --
    # `if (a.st.fail_count)` (:329); sched -- the launcher takes the time-sliced kernels only with `st->sched` (physics.hip); out.status -- `&& a.out.status`
    # (:303); out.info -- `(NV >= 15 && a.out.info) ?` (:301), `a.out.info &&` (:331, :340, :354)
    'door': ('steps_since_goal_change', 'obj_init', 'last_obs', 'fail_count', 'sched', 'status', 'info'),
    'peg': ('steps_since_goal_change', 'obj_init', 'last_obs', 'fail_count', 'sched', 'status', 'info'),
    # kitchen rollout (physics_env_kitchen.h): fail_count -- `if (a.st.fail_count)` (kitchen_rollout_kernel); out.status -- `if (a.out.status)`; the step's
    # scratch (action64 ... att_bak) -- not referenced by kitchen_rollout_kernel at all
    'kitchen': ('fail_count', 'status', 'scratch'),
    # minitaur (physics_env_minitaur.h): steps_since_goal_change -- gcf = ... ? : 0 (:172, :286), gcf > 0 guards (:173, :246, :307, :490);
    # fail_count -- `if (a.st.fail_count)` (:197, :330); last_obs -- `a.st.last_obs ? ... : NAN` (:192, :325), `a.st.last_obs &&` (:248, :492);
    # out.status -- `if (a.out.status)` (:229, :371)
    'minitaur': ('steps_since_goal_change', 'fail_count', 'last_obs', 'status'),
}
POISONED = 2
GOAL_COLS = {'door': 7, 'peg': 7, 'minitaur': 2}


def null_case(kind, snap, acts, null, gcf_run, what):
  kw = {}
  nulls = set(null)
  if 'scratch' in nulls:
    nulls.discard('scratch')
  elif kind == 'kitchen':
    kw['with_scratch'] = True                              # (the reference run passes every scratch buffer)
  if kind == 'peg' and 'obj_init' in nulls:
    nulls.add('info')
  snap.gcf = gcf_run
  return pa.run_both_fills(snap, acts, what, null=tuple(nulls), **kw), nulls


@pytest.mark.parametrize('kind', ['door', 'peg', 'kitchen', 'minitaur'])
def test_optional_pointers_may_be_null(kind):
  """every documented-optional pointer NULL, one at a time and all at once, against the run that passes them all, with env 2 diverging from its first step:
  every output that is given equals the reference bit for bit; with last_obs NULL the diverged env's rows are NaN (include/earl_physics.h)"""
  import torch
  c = cus()
  n = 16 * c + 1 if kind == 'peg' else 11               # (the peg: a batch over one round, so that sched selects the time-sliced kernel)
  T = T_OF[kind]
  acts = env_actions(kind, T, n)
  snap = snapshot(kind, n)
  snap.poison(POISONED)
  opts = OPTIONAL[kind]
  for gcf in ((0, GCF) if kind != 'kitchen' else (0,)):
    ref, _ = null_case(kind, snap, acts, (), gcf, f'{kind} gcf={gcf} all given')
    assert int(ref['out.status'][:, POISONED].sum()) == T and int(ref['out.status'].sum()) == T
    cases = [(o,) for o in opts] + [opts]
    for null in cases:
      if gcf > 0 and 'steps_since_goal_change' in null:
        continue                                          # (refused: tests/test_physics_abi.py)
      what = f'{kind} gcf={gcf} NULL {",".join(null)}'
      res, nulls = null_case(kind, snap, acts, null, gcf, what)
      for k, v in res.items():
        w = ref[k]
        if k == 'out.obs' and 'last_obs' in nulls:
          body = pa.OBS_DIM[kind] - GOAL_COLS[kind]         # (a goal switch writes the new goal into the rolled-back row)
          assert bool(torch.isnan(v[:, POISONED, :body]).all()), what + ': the diverged env rows are NaN without last_obs'
          keep = [i for i in range(n) if i != POISONED]
          pa.same(v[:, keep], w[:, keep], what + ' obs')
        else:
          pa.same(v, w, f'{what} {k}')
      assert set(res) == {k for k in ref if k.split('.', 1)[1] not in nulls}, what


@pytest.mark.parametrize('kind', ['door', 'peg', 'minitaur'])
def test_reset_optional_pointers_and_mask(kind):
  """earl_sawyer_reset / earl_minitaur_reset: mask NULL equals an all-ones mask; obs NULL and each optional state pointer NULL leave every given output as the
  reference has it (guards: physics_env_sawyer.h :396 `!a.mask ||`, :463-464 `a.st.steps_since_* &&`, :469-478 obj_init / last_obs, :470 / :475 reset_obs;
  physics_env_minitaur.h :58 `!a.mask ||`, :157-158 `if (a.reset_obs)` / `if (a.st.last_obs)`, :167 `if (a.st.steps_since_goal_change)`).  A partial mask
  leaves the other envs' rows alone."""
  import torch
  n = 13
  env = pa.make_env(kind, n, seed=6)
  reset = pa.minitaur_reset if kind == 'minitaur' else pa.sawyer_reset
  opts = ('steps_since_goal_change', 'last_obs', 'fail_count') + (('obj_init',) if kind != 'minitaur' else ())
  ones = torch.ones(n, dtype=torch.uint8, device='cuda')
  for fill in pa.FILLS:
    ref, ref_obs, b = reset(env, fill, mask=ones)
    b.check(f'{kind} reset, mask of ones')
    for mask, null, obs in [(None, (), True), (ones, (), False)] + [(ones, (o,), True) for o in opts] + [(None, opts, False)]:
      what = f'{kind} reset fill {fill:#x} mask {"NULL" if mask is None else "ones"} NULL {null} obs {obs}'
      res, o, b = reset(env, fill, mask=mask, null=null, obs=obs)
      b.check(what)
      assert set(res) == {k for k in ref if k[3:] not in null}, what
      for k in res:
        pa.same(res[k], ref[k], f'{what} {k}')
      if obs:
        pa.same(o, ref_obs, what + ' obs')
    part = torch.zeros(n, dtype=torch.uint8, device='cuda')
    part[::3] = 1
    res, o, b = reset(env, fill, mask=part)
    b.check(f'{kind} reset, partial mask')
    sel, rest = part.bool(), ~part.bool()
    for k in res:
      pa.same(res[k][sel], ref[k][sel], f'{kind} partial mask {k} (reset envs)')
      pa.same(res[k][rest], getattr(env, dict(pa.MINITAUR_STATE if kind == 'minitaur' else pa.SAWYER_STATE)[k[3:]])[rest], f'{kind} partial mask {k} (others)')
    pa.same(o[sel], ref_obs[sel], f'{kind} partial mask obs')
    assert bool((o[rest] == 0).all())                              # (obs rows of envs outside the mask are not written: the buffer's zeros)


# ---------------------------------------------------------------------------------------------------- stale goal-switch markers
@pytest.mark.parametrize('name', list(pa.FORMS['door']))
def test_stale_info_markers_do_not_reach_door_info(name):
  """the door's info buffer pre-filled with 1.0 in slot 7 (the goal-switch marker) and garbage in slots 0-2: after the rollout and earl_sawyer_door_info the
  dict equals the one from a zeroed buffer -- with goal switching the rollout writes slot 7 of every row it emits (physics_env_sawyer.h :340, :359), without
  it earl_sawyer_door_info ignores the slot"""
  import torch
  n, T = 9, 4
  acts = env_actions('door', T, n)
  snap = snapshot('door', n)
  switches = pa.FORMS['door'][name][0]

  def stale(info):
    info.fill_(-7.5)
    info[..., 7] = 1.0
    info[..., 0:3] = 123.25

  for gcf in (0, GCF):
    snap.gcf = gcf
    outs = []
    for fill_fn in (None, stale):
      with pa.form(**switches):
        res, b = pa.run(snap, acts, 0xFF, info_fill=fill_fn)
      b.check(f'door {name} gcf={gcf}')
      info = res['out.info'].clone()
      if gcf > 0 and fill_fn is None:
        assert bool((info[..., 7] == 1.0).any()) and bool((info[..., 7] == 0.0).any())     # switch rows and plain rows both present
      pa.door_info(snap.env, res['out.obs'], res['out.status'], info, gcf)
      outs.append(info)
    pa.same(outs[0], outs[1], f'door {name} gcf={gcf}: info from a stale buffer')
    assert bool(torch.isfinite(outs[0]).all())

"""The minitaur's MPPI planner on the device (include/earl_physics.h: earl_minitaur_plan_mppi; Minitaur.mppi_plan / mppi_candidates / mppi_control), bit for bit
against its pieces:
  7. mppi_plan: ret and fail == branch_rollout(mppi_candidates(...)) (tests/test_minitaur_branches_gpu.py holds that launch against restored rollouts); plan, ret0,
     best_ret and best_k == the Python-integer update at K = 4 and the host twin at K = 65 on those returns; the candidates == the Python oracle; in place; three
     iterations in one call == three calls; two shards; the four launch forms; capture into a graph; the env untouched;
  8. mppi_control(T = 3) == its loop written out on public methods, on a twin env;
  9. one recorded observation, printed and not asserted: the mean ret0 over four iterations;
 10. the edges the Sawyer planner's suite holds, through the public ABI: a K wide enough for every strided loop of the update kernel and for the packed launch forms of
     the branch launch, sigma = 0, a poisoned env next to healthy ones, goal switches inside the look-ahead, the candidates at the top of the counter word, K = 1.
The update kernel on returns that no rollout produces is tests/test_plan_update_gpu.py."""
import numpy as np
import pytest

import minitaur_plan_helpers as mp
from physics_abi import form
from test_minitaur_branches_gpu import N, OFF, entered, lifelong, raw, unchanged
from test_minitaur_population_gpu import FORMS
from test_physics_step_graph_gpu import same
from test_sawyer_population_gpu import rows_of

pytestmark = pytest.mark.gpu

H, SIGMA, TEMP, NC = 4, (0.5, 0.0, 0.8, 0.3, 0.2, 0.6, 0.4, 0.7), 0.5, 0x9E3779B9
PLAN_KEYS = ('plan', 'ret', 'ret0', 'best_ret', 'best_k', 'fail')


def start_plan(n, seed=1, H=H):
  import torch
  g = torch.Generator(device='cuda').manual_seed(seed)
  m = (torch.rand(H, n, 8, generator=g, device='cuda') * 2.3 - 1.15).to(torch.float32)      # entries beyond +-1: the planner clips
  m[0, 1, 0] = float('nan')
  return m


def t2n(t):
  return t.detach().cpu().numpy()


@pytest.mark.parametrize('K', [4, 65])
def test_plan_against_its_pieces(K):
  import torch
  from earl_benchmark_amd import _abi
  u = entered(N, env_offset=OFF)
  mean = start_plan(N)
  before = raw(u)
  got = u.mppi_plan(mean, K=K, sigma=SIGMA, temperature=TEMP, noise_counter=NC, iteration0=2)
  assert [tuple(got[k].shape) for k in PLAN_KEYS] == [(H, N, 8), (K, N), (1, N), (N,), (N,), (K, N)]
  unchanged(u, before)
  cand = u.mppi_candidates(mean, K, sigma=SIGMA, iteration=2, noise_counter=NC)
  want_c, m = mp.candidates(int(u._cfg.seed), OFF, N, K, H, 2, SIGMA, NC, t2n(mean))
  mp.same_bits(t2n(cand), want_c, 'the candidates kernel against the Python oracle')
  scored = u.branch_rollout(cand)
  same(got['ret'], scored['ret'], 'ret')
  same(got['fail'], scored['fail'], 'fail')
  ret = t2n(scored['ret'])
  assert len(np.unique(ret)) > N
  if K == 4:
    want = mp.oracle_update(want_c, m, ret, 1.0 / TEMP)
  else:
    want = mp.host_update(_abi.load_host(), mp.cfg_of(N, OFF, int(u._cfg.seed)), mp.params(K, H, inv_t=1.0 / TEMP), 2, t2n(mean), t2n(cand), ret)
  mp.same_bits(t2n(got['plan']), want['plan'], 'plan')
  mp.same(t2n(got['ret0'])[0], want['ret0'], 'ret0')
  mp.same(t2n(got['best_ret']), want['best_ret'], 'best_ret')
  mp.same_bits(t2n(got['best_k']), want['best_k'].astype(np.int32), 'best_k')
  assert bool((got['plan'] != torch.from_numpy(m).cuda()).any()), 'the update moved nothing'
  # in place: out['plan'] is the mean tensor
  buf = mean.clone()
  res = u.mppi_plan(buf, K=K, sigma=SIGMA, temperature=TEMP, noise_counter=NC, iteration0=2, out={'plan': buf})
  assert res['plan'] is buf and set(res) == {'plan', 'ret'}
  same(buf, got['plan'], 'the in-place plan')
  unchanged(u, before)


def test_three_iterations_in_one_call_equal_three_calls():
  u = lifelong(N, env_offset=OFF)
  mean = start_plan(N, seed=2)
  before = raw(u)
  one = u.mppi_plan(mean, K=6, iterations=3, sigma=0.4, temperature=TEMP, noise_counter=NC, iteration0=5)
  plan, ret0 = mean, []
  for i in range(3):
    step = u.mppi_plan(plan, K=6, iterations=1, sigma=0.4, temperature=TEMP, noise_counter=NC, iteration0=5 + i)
    plan = step['plan']
    ret0.append(step['ret0'][0])
  for k in ('plan', 'ret', 'best_ret', 'best_k', 'fail'):
    same(one[k], step[k], k + ' after three iterations')
  import torch
  same(one['ret0'], torch.stack(ret0), 'ret0 of the three iterations')
  unchanged(u, before)


def test_two_shards_equal_the_batch():
  u = lifelong(N, seed=12)
  mean = start_plan(N, seed=3)
  kw = dict(K=5, iterations=2, sigma=SIGMA, temperature=TEMP, noise_counter=NC)
  full = u.mppi_plan(mean, **kw)
  for a, b in ((0, 2), (2, 5)):
    piece = lifelong(b - a, seed=12, env_offset=a)
    piece.load_state_dict(rows_of(u.state_dict(), a, b))
    got = piece.mppi_plan(mean[:, a:b].contiguous(), **kw)
    same(got['plan'], full['plan'][:, a:b].contiguous(), f'plan of rows {a}..{b}')
    for k in ('ret', 'ret0', 'fail'):
      same(got[k], full[k][:, a:b].contiguous(), f'{k} of rows {a}..{b}')
    for k in ('best_ret', 'best_k'):
      same(got[k], full[k][a:b].contiguous(), f'{k} of rows {a}..{b}')


def test_the_four_launch_forms_and_a_captured_graph_return_the_same_bits():
  import torch
  u = lifelong(N, seed=10, env_offset=OFF)
  mean = start_plan(N, seed=4)
  kw = dict(K=5, iterations=2, sigma=SIGMA, temperature=TEMP, noise_counter=NC)
  eager = u.mppi_plan(mean, **kw)
  for name, sw in FORMS.items():
    with form(**sw):
      res = u.mppi_plan(mean, **kw)
    for k in PLAN_KEYS:
      same(res[k], eager[k], f'{k} of {name}')
  before = raw(u)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    res = u.mppi_plan(mean, **kw)
  for rep in range(2):
    for v in res.values():
      v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in PLAN_KEYS:
      same(res[k], eager[k], f'{k} of replay {rep}')
  unchanged(u, before)


def test_control_loop_equals_its_composition_on_a_twin():
  import torch
  from earl_benchmark_amd.envs.minitaur import Minitaur
  T, Kc, I = 3, 5, 2
  ua, ub = lifelong(N, seed=7, env_offset=OFF), lifelong(N, seed=7, env_offset=OFF)
  plan0 = start_plan(N, seed=5)
  got = ua.mppi_control(T, plan=plan0, K=Kc, iterations=I, sigma=SIGMA, temperature=TEMP)
  assert [tuple(got[k].shape) for k in ('obs', 'reward', 'actions', 'plan', 'ret0', 'best_ret')] == [(T, N, 32), (T, N), (T, N, 8), (H, N, 8), (T, I, N), (T, N)]
  P, nc0, rows = plan0.clone(), ub.total_step_count, []
  for s in range(T):
    r = ub.mppi_plan(P, K=Kc, iterations=I, sigma=SIGMA, temperature=TEMP, noise_counter=(nc0 + s) & 0xFFFFFFFF)
    P = r['plan']
    out = ub.rollout(P[:1])
    rows.append((out, P[0].clone(), r['ret0'], r['best_ret']))
    P = torch.cat([P[1:], P[-1:]]).contiguous()
  for k in ('obs', 'reward', 'done', 'success', 'status'):
    same(got[k], torch.cat([r[0][k] for r in rows]), k)
  same(got['actions'], torch.stack([r[1] for r in rows]), 'actions')
  same(got['ret0'], torch.stack([r[2] for r in rows]), 'ret0')
  same(got['best_ret'], torch.stack([r[3] for r in rows]), 'best_ret')
  same(got['plan'], P, 'the shifted plan')
  for k in Minitaur._STATE:
    same(getattr(ua, k), getattr(ub, k), k + ' of the env after the loop')
  assert ua.total_step_count == ub.total_step_count == nc0 + T


def test_one_recorded_observation_is_printed():
  """mean ret0 over four iterations at K = 64, n = 8, H = 5: printed, not asserted (MPPI on a negative dense reward need not improve in four iterations)"""
  u = entered(8, seed=11)
  res = u.mppi_plan(horizon=5, K=64, iterations=4, sigma=0.3, temperature=0.05, noise_counter=1)
  print('mean ret0 per iteration:', [float(x) for x in res['ret0'].mean(1).cpu()], 'rolled-back steps:', int(res['fail'].sum()))


# ---------------------------------------------------------------------------------------------------------------- 10. the Sawyer suite's edges
def composition(u, mean, K, I, sigma, inv_t, nc, iteration0=0):
  """the planner as its pieces, chained over I iterations: the Python candidates -> the env's branch_rollout -> items 4 - 7 in Python integers; numpy arrays"""
  import torch
  n, Hc, plan, ret0 = u.num_envs, int(mean.shape[0]), t2n(mean), []
  for i in range(I):
    act, m = mp.candidates(int(u._cfg.seed), int(u._cfg.env_offset), n, K, Hc, iteration0 + i, sigma, nc, plan)
    br = u.branch_rollout(torch.from_numpy(act).cuda())
    ret = t2n(br['ret'])
    w = mp.oracle_update(act, m, ret, inv_t)
    plan = w['plan']
    ret0.append(ret[0])
  return dict(plan=plan, ret=ret, ret0=np.stack(ret0), best_ret=w['best_ret'], best_k=w['best_k'].astype(np.int32), fail=t2n(br['fail']))


def check_np(got, want, what, rows=None):
  """the six outputs of mppi_plan against numpy expectations, bit for bit (rows: the envs compared)"""
  pick = lambda a: a if rows is None else (a[rows] if a.ndim == 1 else a[:, rows])
  for k in PLAN_KEYS:
    mp.same(pick(t2n(got[k])), pick(np.asarray(want[k])), f'{k} {what}')


def test_a_wide_K_walks_every_strided_loop_and_leaves_the_small_batch_forms():
  """K = 1100: three passes of the workgroup's 512 lanes over the returns and the weights and eighteen of a wave's 64 lanes over the candidates, the last pass of each
  partial; H = 11: more plan steps than the workgroup has waves.  K n = 2200 virtual envs exceed 4 x the compute units, where the automatic rule of the branch launch
  (solo_mode: one env per workgroup up to CUs, one per wave up to 4 CUs) leaves the small-batch forms for the packed ones (minitaur_form)"""
  import torch
  from earl_benchmark_amd import _abi
  K, Hw, n, temperature = 1100, 11, 2, 0.05
  assert K * n > 4 * torch.cuda.get_device_properties(0).multi_processor_count
  u = entered(n, seed=12)
  mean = start_plan(n, seed=8, H=Hw)
  before = raw(u)
  got = u.mppi_plan(mean, K=K, sigma=SIGMA, temperature=temperature, noise_counter=23)
  cand = u.mppi_candidates(mean, K, sigma=SIGMA, noise_counter=23)
  scored = u.branch_rollout(cand)
  unchanged(u, before)
  same(got['ret'], scored['ret'], 'ret')
  same(got['fail'], scored['fail'], 'fail')
  want = mp.host_update(_abi.load_host(), mp.cfg_of(n, 0, int(u._cfg.seed)), mp.params(K, Hw, inv_t=1.0 / temperature), 0, t2n(mean), t2n(cand), t2n(scored['ret']))
  mp.same_bits(t2n(got['plan']), want['plan'], 'plan')
  mp.same(t2n(got['ret0'])[0], want['ret0'], 'ret0')
  mp.same(t2n(got['best_ret']), want['best_ret'], 'best_ret')
  mp.same_bits(t2n(got['best_k']), want['best_k'], 'best_k')
  assert int(got['best_k'].max()) > 0


def test_sigma_zero_every_candidate_is_the_clipped_mean():
  """K = 65, H = 9, n = 3: the 65 virtual envs of one env sit in different waves and workgroups of the branch launch and must return the same bits"""
  import torch
  K, Hs, n = 65, 9, 3
  u = entered(n, seed=13, env_offset=OFF)
  mean = start_plan(n, seed=9, H=Hs)
  m = mp.clip(t2n(mean))
  assert not (m == 0).any()                                                           # (no -0 + 0 in item 5)
  got = u.mppi_plan(mean, K=K, sigma=0.0, temperature=TEMP, noise_counter=NC)
  cand = u.mppi_candidates(mean, K, sigma=0.0, noise_counter=NC)
  mp.same_bits(t2n(cand), np.broadcast_to(m[None], (K, Hs, n, 8)).copy(), 'every candidate')
  for k in ('ret', 'fail'):
    same(got[k], got[k][:1].expand(K, n).contiguous(), f'all K rows of {k}')
  assert bool((got['best_k'] == 0).all())
  same(got['best_ret'], got['ret'][0].contiguous(), 'best_ret')
  same(got['ret0'][0].contiguous(), got['ret'][0].contiguous(), 'ret0')
  mp.same_bits(t2n(got['plan']), m, 'plan')
  assert bool(torch.isfinite(got['ret']).all())


def test_a_poisoned_env_next_to_healthy_ones():
  import torch
  K, Hp, n, bad, I = 3, 6, 7, 5, 2
  clean, env = entered(n, seed=9, env_offset=2), entered(n, seed=9, env_offset=2)
  env.qvel[bad, 1] = float('nan')
  mean = start_plan(n, seed=5, H=Hp)
  before = raw(env)
  kw = dict(K=K, iterations=I, sigma=SIGMA, temperature=TEMP, noise_counter=3)
  want, got = clean.mppi_plan(mean, **kw), env.mppi_plan(mean, **kw)
  unchanged(env, before)
  ok = [i for i in range(n) if i != bad]
  check_np(got, {k: t2n(v) for k, v in want.items()}, 'of the healthy envs', rows=ok)
  assert bool((got['fail'][:, bad] == Hp).all()) and bool((got['ret'][:, bad] == 0).all()) and int(got['best_k'][bad]) == 0      # every step rolled back: reward 0, equal weights
  assert bool(torch.isfinite(got['plan']).all()) and bool((got['plan'].abs() <= 1).all())
  assert bool(torch.isnan(env.qvel[bad, 1])) and int(env.fail_count[bad]) == 0
  check_np(got, composition(env, mean, K, I, SIGMA, 1.0 / TEMP, 3), 'of the poisoned batch against its pieces')
  assert not torch.equal(got['plan'][:, bad], torch.from_numpy(mp.clip(t2n(mean))).cuda()[:, bad]), 'equal weights: the plan moves by the plain noise average'


def test_goal_switches_inside_the_look_ahead():
  K, Hl, n, I = 3, 7, 6, 2
  u = lifelong(n, gcf=3, env_offset=OFF)
  assert 0 < int(u._cfg.goal_change_frequency) < Hl
  mean = start_plan(n, seed=4, H=Hl)
  before = raw(u)
  kw = dict(K=K, iterations=I, sigma=SIGMA, temperature=TEMP, noise_counter=11)
  got, again = u.mppi_plan(mean, **kw), u.mppi_plan(mean, **kw)
  unchanged(u, before)                                                                # goal_t and steps_since_goal_change among them
  for k in PLAN_KEYS:
    same(again[k], got[k], k + ' of the second call (the workspace carries nothing over)')
  check_np(got, composition(u, mean, K, I, SIGMA, 1.0 / TEMP, 11), 'with goal switches against its pieces')
  unchanged(u, before)


@pytest.mark.parametrize('K,Hc', [(8192, 2), (2, 65536)])
def test_candidates_at_the_top_of_the_counter_word(K, Hc):
  """word 2 of the counter is (k << 16) | t, the second block's has bit 31 set: at K = 8192 (k up to 2^13 - 1) and at H = 65536 (t up to 2^16 - 1) the fields meet
  neither each other nor that bit.  Through earl_minitaur_plan_candidates itself on a NaN-filled buffer: every word is written"""
  import ctypes as C
  import torch
  from earl_benchmark_amd import _abi
  assert (((K - 1) << 16) | (Hc - 1)) < 2**31
  u = entered(1, seed=14, env_offset=OFF)
  mean = (torch.rand(Hc, 1, 8, generator=torch.Generator(device='cuda').manual_seed(K), device='cuda') * 2.3 - 1.15).to(torch.float32)
  act = torch.full((K, Hc, 1, 8), float('nan'), dtype=torch.float32, device='cuda')
  pp = mp.params(K, Hc, sigma=0.5, nc=NC)
  _abi.check(u._lib.earl_minitaur_plan_candidates(C.byref(u._cfg), C.byref(pp), 255, mean.data_ptr(), act.data_ptr(), torch.cuda.current_stream().cuda_stream),
             'earl_minitaur_plan_candidates')
  torch.cuda.synchronize()
  got = t2n(act)
  assert not np.isnan(got).any(), 'a word was not written'
  want, m = mp.candidates(int(u._cfg.seed), OFF, 1, K, Hc, 255, 0.5, NC, t2n(mean))
  mp.same_bits(got, want, 'the candidates against the numpy Philox oracle')
  assert not np.array_equal(got[1:, ..., :4] - m[None, ..., :4], got[1:, ..., 4:] - m[None, ..., 4:]), 'the second block repeats the first'
  same(u.mppi_candidates(mean, K, sigma=0.5, iteration=255, noise_counter=NC), act, 'mppi_candidates')


def test_one_candidate_is_the_smallest_legal_call():
  """K = 1: the clipped mean alone -- plan == clip(mean), best_k == 0, ret0 == best_ret == ret[0]"""
  n = N
  u = entered(n, seed=15, env_offset=OFF)
  mean = start_plan(n, seed=6)
  before = raw(u)
  got = u.mppi_plan(mean, K=1, iterations=2, sigma=SIGMA, temperature=TEMP, noise_counter=NC)
  unchanged(u, before)
  assert [tuple(got[k].shape) for k in PLAN_KEYS] == [(H, n, 8), (1, n), (2, n), (n,), (n,), (1, n)]
  check_np(got, composition(u, mean, 1, 2, SIGMA, 1.0 / TEMP, NC), 'at K = 1 against its pieces')
  mp.same_bits(t2n(got['plan']), mp.clip(t2n(mean)), 'plan')
  assert bool((got['best_k'] == 0).all())
  same(got['best_ret'], got['ret'][0].contiguous(), 'best_ret')

// sawyer_cem.hip -- earl_sawyer_plan_cem / earl_sawyer_cem_candidates / earl_sawyer_cem_update (include/earl_physics.h, "CEM planning on the door and the peg"):
// I iterations of sample -> score -> refit around the EXISTING branch launch, the launches of earl_sawyer_plan_mppi with CEM's two kernels around it.  Per iteration on
// the caller's stream, ordered by the stream alone:
//   sawyer_cem_candidates_kernel    one lane per (k, t, env) in the order of the [K, H, n, 4] array: the row's clipped mean and clamped std, one Philox block, four
//                                   quantiles, one 16-byte store; row k = 0 is the clipped mean.  A grid-stride loop over a bounded grid.
//   earl_sawyer_branch_rollout      through the public ABI, not a line of it changed: the candidates in, ret [K, n] (and fail) out.
//   sawyer_cem_update_kernel        ONE workgroup of 512 lanes per env, three stages.  (1) Each lane loads the returns of its <= 16 branches (k = tid + 512 r) once, keeps
//                                   their order-preserving keys in registers, and the workgroup max-reduces beta / best_k as MPPI's update does.  (2) cem_select.h: a radix
//                                   select over the keys, eight passes of eight bits, finds the key of rank E - 1 and compacts the elites' indices into LDS -- O(K) per
//                                   env, where ranking every pair is O(K^2).  (3) Wave w takes the plan steps t = w, w + 8, ...: its 64 lanes split the compacted
//                                   list, read each elite's float4 from the candidates, keep int64 A1[4], A2[4], join them by shuffles; lane 0 writes the plan row and
//                                   the std row.  Row t of mean / std is read by the wave that writes it and by no other: plan == mean and std == std_in are safe.
// The per-element functions are sawyer_cem.h's and, where the MPPI planner computes the same, sawyer_shoot.h's (tabletop_cem.h's and tabletop_plan.h's for the
// dimension-free items), shared with the host twins of tabletop_host.cpp.  The workspace layout, the prologue of the call and the scoring call of an iteration are
// sawyer_shoot.h's too.
#include <hip/hip_runtime.h>

#include "sawyer_cem.h"
#include "cem_select.h"

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kUpdateThreads = 512, kUpdateWaves = kUpdateThreads / 64, kPerLane = EARL_SAWYER_PLAN_MAX_K / kUpdateThreads;
static_assert(kPerLane * kUpdateThreads == EARL_SAWYER_PLAN_MAX_K, "a lane's register keys cover K");
using SelectLds = CemSelectLds<kUpdateThreads, kPerLane, EARL_SAWYER_CEM_MAX_E>;

__global__ __launch_bounds__(kCandThreads) void sawyer_cem_candidates_kernel(const SawyerCemArgs p, float* __restrict__ act_out) {
  shoot_for_each_candidate(p.K, p.H, p.n, [&](unsigned long long e, int i, int k, int t) {
    float m[4], s[4], c[4];
    shoot_mean(p.mean, p.n, i, t, m);
    scem_std(p, i, t, s);
    shoot_candidate(p.word0, (uint32_t)(p.env_offset + i), (uint32_t)k, (uint32_t)t, p.noise_counter, p.seed, s, m, c);
    *reinterpret_cast<float4*>(act_out + e * 4) = float4{c[0], c[1], c[2], c[3]};
  });
}

__global__ __launch_bounds__(kUpdateThreads) void sawyer_cem_update_kernel(const SawyerCemArgs p) {
  __shared__ SelectLds sel;
  __shared__ double b_lds[kUpdateWaves];
  __shared__ int32_t k_lds[kUpdateWaves];
  const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = p.n, K = p.K;

  // item 4, first half: beta and best_k as the MPPI update finds them, and the keys of this lane's branches, each return read once
  uint64_t key[kPerLane];
  double beta = -__builtin_inf();
  int bk = 0;
#pragma unroll
  for (int r = 0; r < kPerLane; ++r) {
    const int k = tid + r * kUpdateThreads;
    key[r] = 0;
    if (k < K) {
      const double v = p.ret[(size_t)k * n + i];
      plan_best(v, k, beta, bk);
      key[r] = cem_key(v);
    }
  }
  block_best<kUpdateThreads>(beta, bk, b_lds, k_lds);

  // item 4, second half: the elites
  uint32_t mine;
  const int32_t Ne = cem_select<kUpdateThreads, kPerLane, EARL_SAWYER_CEM_MAX_E>(key, K, p.E, sel, mine);
  if (p.elite) {
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
      const int k = tid + r * kUpdateThreads;
      if (k < K) p.elite[(size_t)k * n + i] = (uint8_t)((mine >> r) & 1u);
    }
  }

  // item 5: a wave per plan step, its lanes over the elites
  for (int t = wave; t < p.H; t += kUpdateWaves) {
    float m[4], s[4];
    shoot_mean(p.mean, n, i, t, m);
    scem_std(p, i, t, s);
    int64_t A1[4] = {0, 0, 0, 0}, A2[4] = {0, 0, 0, 0};
    for (int e = lane; e < Ne; e += 64) {
      const int k = (int)sel.elite[e];
      if (k > 0) {                                                                  // (branch 0 is the mean: D = 0)
        const float4 v = *reinterpret_cast<const float4*>(p.act + shoot_act_index(p.H, n, i, k, t));
        const float c[4] = {v.x, v.y, v.z, v.w};
        scem_accumulate(c, m, A1, A2);
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      A1[d] = wave_sum(A1[d]);
      A2[d] = wave_sum(A2[d]);
    }
    if (lane == 0) {
      const size_t row = ((size_t)t * n + i) * 4;
      *reinterpret_cast<float4*>(p.plan + row) = float4{cem_new_mean(m[0], A1[0], Ne, p.alpha), cem_new_mean(m[1], A1[1], Ne, p.alpha),
                                                        cem_new_mean(m[2], A1[2], Ne, p.alpha), cem_new_mean(m[3], A1[3], Ne, p.alpha)};
      *reinterpret_cast<float4*>(p.std_out + row) =
          float4{cem_new_std(s[0], A1[0], A2[0], Ne, p.alpha, p.std_min, p.std_max), cem_new_std(s[1], A1[1], A2[1], Ne, p.alpha, p.std_min, p.std_max),
                 cem_new_std(s[2], A1[2], A2[2], Ne, p.alpha, p.std_min, p.std_max), cem_new_std(s[3], A1[3], A2[3], Ne, p.alpha, p.std_min, p.std_max)};
    }
  }
  if (tid == 0) {
    if (p.ret0) p.ret0[i] = p.ret[i];                                                // (branch 0: the plan entering the iteration)
    if (p.best_ret) p.best_ret[i] = beta;
    if (p.best_k) p.best_k[i] = bk;
  }
}

int launch_candidates(const SawyerCemArgs& p, float* act_out, hipStream_t stream) {
  sawyer_cem_candidates_kernel<<<shoot_candidates_grid(p.K, p.H, p.n), kCandThreads, 0, stream>>>(p, act_out);
  return launched("sawyer_cem_candidates_kernel");
}

int launch_update(const SawyerCemArgs& p, hipStream_t stream) {
  sawyer_cem_update_kernel<<<dim3((unsigned)p.n), kUpdateThreads, 0, stream>>>(p);
  return launched("sawyer_cem_update_kernel");
}

}  // namespace

extern "C" {

int earl_sawyer_cem_candidates(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out,
                               earl_stream_t stream) {
  if (int rc = check_sawyer_cem(SawyerCemCall::Candidates, cfg, params, j, mean, std, act_out, nullptr)) return rc;
  if (misaligned16(act_out)) return fail(EARL_ERR_ARG, "act_out is not 16-byte aligned");
  if (cfg->n == 0) return EARL_OK;
  SawyerCemArgs p = sawyer_cem_args(cfg, params, mean, std);
  p.word0 = kCemDraw | (uint32_t)j;
  return launch_candidates(p, act_out, (hipStream_t)stream);
}

int earl_sawyer_cem_update(const earl_sawyer_cfg* cfg, const earl_sawyer_cem_params* params, int32_t j, const float* mean, const float* std_in, const float* act,
                           const double* ret, float* plan, float* std, double* ret0_row, double* best_ret, int32_t* best_k, uint8_t* elite, earl_stream_t stream) {
  if (int rc = check_sawyer_cem(SawyerCemCall::Update, cfg, params, j, mean, std_in, plan, std)) return rc;
  if (!act || !ret) return fail(EARL_ERR_ARG, "act/ret is NULL");
  if (misaligned16(act)) return fail(EARL_ERR_ARG, "act is not 16-byte aligned");
  if (misaligned16(plan) || misaligned16(std)) return fail(EARL_ERR_ARG, "plan / std is not 16-byte aligned: a row is one 16-byte store");
  if (cfg->n == 0) return EARL_OK;
  SawyerCemArgs p = sawyer_cem_args(cfg, params, mean, std_in);
  p.plan = plan;
  p.std_out = std;
  p.act = act;
  p.ret = ret;
  p.ret0 = ret0_row;
  p.best_ret = best_ret;
  p.best_k = best_k;
  p.elite = elite;
  p.word0 = kCemDraw | (uint32_t)j;
  return launch_update(p, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// The body of the three entry points: pv and prior as in sawyer_plan.hip's plan_mppi, the draw word CEM's; the prologue and the scoring call are sawyer_shoot.h's
int plan_cem(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
             const earl_sawyer_cem_params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const float* mean, const float* std0, float* plan, float* std,
             double* ret, double* ret0, double* best_ret, int32_t* best_k, uint8_t* elite, int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
             earl_stream_t stream) {
  if (int rc = check_sawyer_cem(SawyerCemCall::Cem, cfg, params, 0, mean, std0, plan, std)) return rc;
  SawyerShoot s;
  if (int rc = sawyer_shoot_open(model, col, nv, cfg, st, params, pv, prior, {mean, plan, std0, std},
                                 misaligned16(plan) || misaligned16(std) ? "plan / std is not 16-byte aligned: a row is one 16-byte store" : nullptr, plan, ret, fail_count,
                                 clock, ws, stream, &s))
    return rc;
  const int n = cfg->n;
  if (n == 0) return EARL_OK;
  SawyerCemArgs p = sawyer_cem_args(cfg, params, mean, std0);
  p.plan = plan;
  p.std_out = std;
  p.act = s.act;
  p.ret = ret;
  for (int it = 0; it < params->iterations; ++it) {
    const bool last = it + 1 == params->iterations;
    p.word0 = kCemDraw | (uint32_t)(params->iteration0 + it);
    p.ret0 = ret0 ? ret0 + (size_t)it * n : nullptr;
    p.best_ret = last ? best_ret : nullptr;
    p.best_k = last ? best_k : nullptr;
    p.elite = last ? elite : nullptr;
    if (int rc = launch_candidates(p, s.act, (hipStream_t)stream)) return rc;
    if (int rc = sawyer_shoot_score(s, p.word0, it, last)) return rc;
    if (int rc = launch_update(p, (hipStream_t)stream)) return rc;
    p.mean = plan;                                                                   // (the next iteration starts from this one's results, in place)
    p.std_in = std;
  }
  return EARL_OK;
}

}  // namespace

extern "C" {

int earl_sawyer_plan_cem(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                         const earl_sawyer_cem_params* params, const float* mean, const float* std0, float* plan, float* std, double* ret, double* ret0,
                         double* best_ret, int32_t* best_k, uint8_t* elite, int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                         earl_stream_t stream) {
  return plan_cem(model, col, nv, cfg, st, params, nullptr, nullptr, mean, std0, plan, std, ret, ret0, best_ret, best_k, elite, fail_count, clock, ws, stream);
}

int earl_sawyer_plan_cem_value(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_sawyer_cem_params* params, const earl_plan_value* pv, const float* mean, const float* std0, float* plan, float* std, double* ret,
                               double* ret0, double* best_ret, int32_t* best_k, uint8_t* elite, int32_t* fail_count, const uint64_t* clock,
                               const earl_sawyer_branch_ws* ws, earl_stream_t stream) {
  return plan_cem(model, col, nv, cfg, st, params, sawyer_value_plain(pv) ? nullptr : pv, nullptr, mean, std0, plan, std, ret, ret0, best_ret, best_k, elite, fail_count, clock, ws,
                  stream);
}

int earl_sawyer_plan_cem_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                               const earl_sawyer_cem_params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const float* mean, const float* std0,
                               float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k, uint8_t* elite, int32_t* fail_count,
                               const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream) {
  if (!prior || !prior->policy) return fail(EARL_ERR_ARG, "prior / prior->policy is NULL");
  // branches == 0 (after the struct's own rules, checked inside): exactly the `_value` call, which is the plain call for pv NULL or {1.0, NULL}
  const bool none = prior->branches == 0;
  return plan_cem(model, col, nv, cfg, st, params, none && sawyer_value_plain(pv) ? nullptr : pv, prior, mean, std0, plan, std, ret, ret0, best_ret, best_k, elite, fail_count,
                  clock, ws, stream);
}

}  // extern "C"

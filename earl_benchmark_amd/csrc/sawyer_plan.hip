// sawyer_plan.hip -- earl_sawyer_plan_mppi / earl_sawyer_plan_candidates / earl_sawyer_plan_ws_bytes (include/earl_physics.h, "MPPI planning on the door and the peg"):
// I iterations of sample -> score -> reweight around the EXISTING branch launch.  Per iteration on the caller's stream, ordered by the stream alone:
//   sawyer_plan_candidates_kernel   one lane per (k, t, env) in the order of the [K, H, n, 4] array: one Philox block, four quantiles, one 16-byte store; row k = 0 is
//                                   the clipped mean.  A grid-stride loop over a bounded grid, one pass at every realistic size.
//   earl_sawyer_branch_rollout      through the public ABI (physics.hip, physics_branch.hip, physics_branch_w8.hip: not a line of them changes): the candidates in,
//                                   ret [K, n] (and fail) out.
//   sawyer_plan_update_kernel       ONE workgroup per env (n is small and K large where this planner is used): beta / best_k by a max-reduce of ret[:, env] over all
//                                   lanes (shuffles, then LDS across the waves), the integer weights W_k once per env into LDS (int32 [K], 32 KB at most), then wave w
//                                   takes the plan steps t = w, w + 8, ...: its 64 lanes split the K candidates of the step, each keeps int64 partial sums of W_k and
//                                   W_k * D_k for the four dimensions, joined across the lanes by shuffles.  Integer sums: any split gives the same bits.
// The per-element functions are sawyer_plan.h's and, where the CEM planner computes the same, sawyer_shoot.h's (tabletop_plan.h's for the dimension-free items), shared
// with the host twins of tabletop_host.cpp.  The workspace layout, the prologue of the call and the scoring call of an iteration are sawyer_shoot.h's too.
// The candidates go through memory on purpose: an env step costs tens of thousands of cycles and the whole array of a realistic call is about a megabyte, so there is
// no fourth inclusion of the rollout kernel's text with the noise inside.
#include <hip/hip_runtime.h>

#include "sawyer_plan.h"

static_assert(earl::kSawyerPriorDraw == earl::kPlanDraw, "earl_sawyer_branch_rollout_prior draws the noise of MPPI's branch k");

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kUpdateThreads = 512, kUpdateWaves = kUpdateThreads / 64;

__global__ __launch_bounds__(kCandThreads) void sawyer_plan_candidates_kernel(const SawyerPlanArgs p, float* __restrict__ act_out) {
  shoot_for_each_candidate(p.K, p.H, p.n, [&](unsigned long long e, int i, int k, int t) {
    float m[4], c[4];
    shoot_mean(p.mean, p.n, i, t, m);
    shoot_candidate(p.word0, (uint32_t)(p.env_offset + i), (uint32_t)k, (uint32_t)t, p.noise_counter, p.seed, p.sigma, m, c);
    *reinterpret_cast<float4*>(act_out + e * 4) = float4{c[0], c[1], c[2], c[3]};
  });
}

__global__ __launch_bounds__(kUpdateThreads) void sawyer_plan_update_kernel(const SawyerPlanArgs p) {
  __shared__ int32_t w_lds[EARL_SAWYER_PLAN_MAX_K];
  __shared__ double b_lds[kUpdateWaves];
  __shared__ int32_t k_lds[kUpdateWaves];
  const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = p.n, K = p.K;

  // item 4: beta and best_k -- a lane over its k ascending, then the workgroup's
  double beta = -__builtin_inf();
  int bk = 0;
  for (int k = tid; k < K; k += kUpdateThreads) plan_best(p.ret[(size_t)k * n + i], k, beta, bk);
  block_best<kUpdateThreads>(beta, bk, b_lds, k_lds);

  // the integer weights, once per (k, env)
  for (int k = tid; k < K; k += kUpdateThreads) w_lds[k] = plan_weight(p.ret[(size_t)k * n + i], beta, p.inv_temperature);
  __syncthreads();

  // item 5: a wave per plan step, its lanes over k.  Row t of the mean is read by this wave before it writes row t of the plan and by no other: plan == mean is safe.
  for (int t = wave; t < p.H; t += kUpdateWaves) {
    float m[4];
    shoot_mean(p.mean, n, i, t, m);
    int64_t A[4] = {0, 0, 0, 0}, S = 0;
    for (int k = lane; k < K; k += 64) {
      const int32_t W = w_lds[k];
      S += W;
      if (W != 0 && k > 0) {                                                        // (branch 0 is the mean: delta = 0)
        const float4 v = *reinterpret_cast<const float4*>(p.act + shoot_act_index(p.H, n, i, k, t));
        const float c[4] = {v.x, v.y, v.z, v.w};
        splan_accumulate(c, m, W, A);
      }
    }
    S = wave_sum(S);
#pragma unroll
    for (int d = 0; d < 4; ++d) A[d] = wave_sum(A[d]);
    if (lane == 0)
      *reinterpret_cast<float4*>(p.plan + ((size_t)t * n + i) * 4) =
          float4{plan_new_mean(m[0], A[0], S), plan_new_mean(m[1], A[1], S), plan_new_mean(m[2], A[2], S), plan_new_mean(m[3], A[3], S)};
  }
  if (tid == 0) {
    if (p.ret0) p.ret0[i] = p.ret[i];                                                // (branch 0: the plan entering the iteration)
    if (p.best_ret) p.best_ret[i] = beta;
    if (p.best_k) p.best_k[i] = bk;
  }
}

int launch_candidates(const SawyerPlanArgs& p, float* act_out, hipStream_t stream) {
  sawyer_plan_candidates_kernel<<<shoot_candidates_grid(p.K, p.H, p.n), kCandThreads, 0, stream>>>(p, act_out);
  return launched("sawyer_plan_candidates_kernel");
}

}  // namespace

extern "C" {

// the Plain block of sawyer_shoot.h's sawyer_ws_layout
int earl_sawyer_plan_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes) { return sawyer_ws_bytes(nv, K, H, n, SawyerWs::Plain, bytes); }

int earl_sawyer_plan_candidates(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, float* act_out, earl_stream_t stream) {
  if (int rc = check_sawyer_plan(SawyerPlanCall::Candidates, cfg, params, j, mean, act_out)) return rc;
  if (misaligned16(act_out)) return fail(EARL_ERR_ARG, "act_out is not 16-byte aligned");
  if (cfg->n == 0) return EARL_OK;
  SawyerPlanArgs p = sawyer_plan_args(cfg, params, mean);
  p.word0 = kPlanDraw | (uint32_t)j;
  return launch_candidates(p, act_out, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// The body of the three entry points; the prologue and the scoring call are sawyer_shoot.h's.  pv NULL (the value-free entry point, and the others with pv NULL or
// {1.0, NULL} where nothing else needs it): the plain sum and the Plain block; otherwise the discounted sum and / or the value network, the Value block.  prior given
// (earl_sawyer_plan_mppi_prior) with branches >= 1: the scoring call runs the last `branches` branches by the policy with this planner's draw word and OVERWRITES their
// blocks of the candidates the kernel above it wrote; the Prior block.  The update kernel reads the candidates back and does not know.
int plan_mppi(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
              const earl_sawyer_plan_params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0,
              double* best_ret, int32_t* best_k, int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream) {
  if (int rc = check_sawyer_plan(SawyerPlanCall::Mppi, cfg, params, 0, mean, plan)) return rc;
  SawyerShoot s;
  if (int rc = sawyer_shoot_open(model, col, nv, cfg, st, params, pv, prior, {mean, plan, nullptr, nullptr}, nullptr, plan, ret, fail_count, clock, ws, stream, &s)) return rc;
  const int n = cfg->n;
  if (n == 0) return EARL_OK;
  SawyerPlanArgs p = sawyer_plan_args(cfg, params, mean);
  p.plan = plan;
  p.act = s.act;
  p.ret = ret;
  for (int it = 0; it < params->iterations; ++it) {
    const bool last = it + 1 == params->iterations;
    p.word0 = kPlanDraw | (uint32_t)(params->iteration0 + it);
    p.ret0 = ret0 ? ret0 + (size_t)it * n : nullptr;
    p.best_ret = last ? best_ret : nullptr;
    p.best_k = last ? best_k : nullptr;
    if (int rc = launch_candidates(p, s.act, (hipStream_t)stream)) return rc;
    if (int rc = sawyer_shoot_score(s, p.word0, it, last)) return rc;
    sawyer_plan_update_kernel<<<dim3((unsigned)n), kUpdateThreads, 0, (hipStream_t)stream>>>(p);
    if (int rc = launched("sawyer_plan_update_kernel")) return rc;
    p.mean = plan;                                                                   // (the next iteration starts from this one's result, in place)
  }
  return EARL_OK;
}

}  // namespace

extern "C" {

int earl_sawyer_plan_mppi(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                          const earl_sawyer_plan_params* params, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                          int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream) {
  return plan_mppi(model, col, nv, cfg, st, params, nullptr, nullptr, mean, plan, ret, ret0, best_ret, best_k, fail_count, clock, ws, stream);
}

int earl_sawyer_plan_mppi_value(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                const earl_sawyer_plan_params* params, const earl_plan_value* pv, const float* mean, float* plan, double* ret, double* ret0,
                                double* best_ret, int32_t* best_k, int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream) {
  return plan_mppi(model, col, nv, cfg, st, params, sawyer_value_plain(pv) ? nullptr : pv, nullptr, mean, plan, ret, ret0, best_ret, best_k, fail_count, clock, ws, stream);
}

int earl_sawyer_plan_mppi_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                const earl_sawyer_plan_params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const float* mean, float* plan,
                                double* ret, double* ret0, double* best_ret, int32_t* best_k, int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                                earl_stream_t stream) {
  if (!prior || !prior->policy) return fail(EARL_ERR_ARG, "prior / prior->policy is NULL");
  // branches == 0 (after the struct's own rules, checked inside): exactly the `_value` call, which is the plain call for pv NULL or {1.0, NULL}
  const bool none = prior->branches == 0;
  return plan_mppi(model, col, nv, cfg, st, params, none && sawyer_value_plain(pv) ? nullptr : pv, prior, mean, plan, ret, ret0, best_ret, best_k, fail_count, clock, ws, stream);
}

}  // extern "C"

// minitaur_plan.hip -- earl_minitaur_plan_mppi / earl_minitaur_plan_candidates / earl_minitaur_plan_ws_bytes (include/earl_physics.h, "MPPI planning on the minitaur"):
// I iterations of sample -> score -> reweight around the branch launch.  Per iteration on the caller's stream, ordered by the stream alone:
//   minitaur_plan_candidates_kernel   one lane per (k, t, env) in the order of the [K, H, n, 8] array: two Philox blocks, eight quantiles, two 16-byte stores; row k = 0 is
//                                     the clipped mean.  A grid-stride loop over a bounded grid, one pass at every realistic size.
//   earl_minitaur_branch_rollout      through the public ABI (physics_mt.hip, physics_mt_branch.hip), untouched: the candidates in, ret [K, n] (and fail) out.
//   minitaur_plan_update_kernel       ONE workgroup per env: beta / best_k by a max-reduce of ret[:, env] over all lanes (shuffles, then LDS across the waves), the integer
//                                     weights W_k once per env into LDS (int32 [K], 32 KB at most), then wave w takes the plan steps t = w, w + 8, ...: its 64 lanes split
//                                     the K candidates of the step, each keeps int64 partial sums of W_k and W_k * D_k for the eight dimensions, joined across the lanes
//                                     by shuffles.  Integer sums: any split gives the same bits.
// The per-element functions are minitaur_plan.h's (tabletop_plan.h's and sawyer_shoot.h's for the dimension-free items), shared with the host twins of
// tabletop_host.cpp.  No stepper header: the planner reaches the stepper through the public ABI.  The candidates go through memory, as the Sawyer planner's do and
// for its reason: an env step costs tens of thousands of cycles.
#include <hip/hip_runtime.h>

#include "minitaur_plan.h"

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kUpdateThreads = 512, kUpdateWaves = kUpdateThreads / 64;

__global__ __launch_bounds__(kCandThreads) void minitaur_plan_candidates_kernel(const MinitaurPlanArgs p, float* __restrict__ act_out) {
  shoot_for_each_candidate(p.K, p.H, p.n, [&](unsigned long long e, int i, int k, int t) {
    float m[8], c[8];
    mtplan_mean(p.mean, p.n, i, t, m);
    mtplan_candidate(p.word0, (uint32_t)(p.env_offset + i), (uint32_t)k, (uint32_t)t, p.noise_counter, p.seed, p.sigma, m, c);
    float4* dst = reinterpret_cast<float4*>(act_out + e * 8);
    dst[0] = float4{c[0], c[1], c[2], c[3]};
    dst[1] = float4{c[4], c[5], c[6], c[7]};
  });
}

__global__ __launch_bounds__(kUpdateThreads) void minitaur_plan_update_kernel(const MinitaurPlanArgs p) {
  __shared__ int32_t w_lds[EARL_MINITAUR_PLAN_MAX_K];
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
    float m[8];
    mtplan_mean(p.mean, n, i, t, m);
    int64_t A[8] = {0, 0, 0, 0, 0, 0, 0, 0}, S = 0;
    for (int k = lane; k < K; k += 64) {
      const int32_t W = w_lds[k];
      S += W;
      if (W != 0 && k > 0) {                                                        // (branch 0 is the mean: delta = 0)
        const float4* src = reinterpret_cast<const float4*>(p.act + mtplan_act_index(p.H, n, i, k, t));
        const float4 v0 = src[0], v1 = src[1];
        const float c[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        mtplan_accumulate(c, m, W, A);
      }
    }
    S = wave_sum(S);
#pragma unroll
    for (int d = 0; d < 8; ++d) A[d] = wave_sum(A[d]);
    if (lane == 0) {
      float4* dst = reinterpret_cast<float4*>(p.plan + ((size_t)t * n + i) * 8);
      dst[0] = float4{plan_new_mean(m[0], A[0], S), plan_new_mean(m[1], A[1], S), plan_new_mean(m[2], A[2], S), plan_new_mean(m[3], A[3], S)};
      dst[1] = float4{plan_new_mean(m[4], A[4], S), plan_new_mean(m[5], A[5], S), plan_new_mean(m[6], A[6], S), plan_new_mean(m[7], A[7], S)};
    }
  }
  if (tid == 0) {
    if (p.ret0) p.ret0[i] = p.ret[i];                                                // (branch 0: the plan entering the iteration)
    if (p.best_ret) p.best_ret[i] = beta;
    if (p.best_k) p.best_k[i] = bk;
  }
}

int launch_candidates(const MinitaurPlanArgs& p, float* act_out, hipStream_t stream) {
  minitaur_plan_candidates_kernel<<<shoot_candidates_grid(p.K, p.H, p.n), kCandThreads, 0, stream>>>(p, act_out);
  return launched("minitaur_plan_candidates_kernel");
}

}  // namespace

extern "C" {

int earl_minitaur_plan_ws_bytes(int32_t K, int32_t H, int32_t n, int64_t* bytes) {
  MinitaurPlanLayout L;
  if (!bytes || minitaur_plan_layout(K, H, n, &L)) return EARL_ERR_ARG;
  *bytes = L.need;
  return EARL_OK;
}

int earl_minitaur_plan_candidates(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* params, int32_t j, const float* mean, float* act_out, earl_stream_t stream) {
  if (int rc = check_minitaur_plan(MinitaurPlanCall::Candidates, cfg, params, j, mean, act_out)) return rc;
  if (misaligned16(act_out)) return fail(EARL_ERR_ARG, "act_out is not 16-byte aligned");
  if (cfg->n == 0) return EARL_OK;
  MinitaurPlanArgs p = minitaur_plan_args(cfg, params, mean);
  p.word0 = kPlanDraw | (uint32_t)j;
  return launch_candidates(p, act_out, (hipStream_t)stream);
}

int earl_minitaur_plan_mppi(const void* model24, const earl_collision_model* col, const earl_minitaur_cfg* cfg, const earl_minitaur_state* st,
                            const earl_minitaur_plan_params* params, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                            int32_t* fail_count, const uint64_t* clock, const earl_minitaur_branch_ws* ws, earl_stream_t stream) {
  if (int rc = check_minitaur_plan(MinitaurPlanCall::Mppi, cfg, params, 0, mean, plan)) return rc;
  if (!ret) return fail(EARL_ERR_ARG, "ret is NULL: the branch launch writes it and the update reads it");
  if (!ws) return fail(EARL_ERR_ARG, "ws is NULL");
  const int n = cfg->n, K = params->K, H = params->H;
  MinitaurPlanLayout L;
  if (minitaur_plan_layout(K, H, n, &L)) return fail(EARL_ERR_ARG, "K = %d, H = %d, n = %d", K, H, n);
  if (n > 0 && (!ws->base || (reinterpret_cast<uintptr_t>(ws->base) & 7) != 0 || ws->bytes < L.need))
    return fail(EARL_ERR_ARG, "ws: base %p (8-byte aligned), %lld bytes of the %lld needed", ws->base, (long long)ws->bytes, (long long)L.need);
  float* const act = n > 0 ? minitaur_plan_candidates_at(ws->base, L) : plan;      // (`plan` stands in for the candidates where n == 0)
  const earl_minitaur_branch_ws bws{ws->base, L.branch};
  const earl_episode_summary sum{ret, nullptr, nullptr};
  // the model / col / cfg / st side and the stepper switch are the branch launch's to decide: with H = 0 it returns after its checks and before its first HIP call
  if (int rc = earl_minitaur_branch_rollout(model24, col, cfg, st, K, 0, act, 0, clock, &bws, &sum, nullptr, fail_count, stream)) return rc;      // (its own message stands)
  if (n == 0) return EARL_OK;
  MinitaurPlanArgs p = minitaur_plan_args(cfg, params, mean);
  p.plan = plan;
  p.act = act;
  p.ret = ret;
  for (int it = 0; it < params->iterations; ++it) {
    const bool last = it + 1 == params->iterations;
    p.word0 = kPlanDraw | (uint32_t)(params->iteration0 + it);
    p.ret0 = ret0 ? ret0 + (size_t)it * n : nullptr;
    p.best_ret = last ? best_ret : nullptr;
    p.best_k = last ? best_k : nullptr;
    if (int rc = launch_candidates(p, act, (hipStream_t)stream)) return rc;
    if (int rc = earl_minitaur_branch_rollout(model24, col, cfg, st, K, H, act, (int64_t)H * n * 8, clock, &bws, &sum, nullptr, last ? fail_count : nullptr, stream))
      return rc == EARL_ERR_ARG ? rc : fail(rc, "earl_minitaur_branch_rollout failed in iteration %d", params->iteration0 + it);
    minitaur_plan_update_kernel<<<dim3((unsigned)n), kUpdateThreads, 0, (hipStream_t)stream>>>(p);
    if (int rc = launched("minitaur_plan_update_kernel")) return rc;
    p.mean = plan;                                                                   // (the next iteration starts from this one's result, in place)
  }
  return EARL_OK;
}

}  // extern "C"

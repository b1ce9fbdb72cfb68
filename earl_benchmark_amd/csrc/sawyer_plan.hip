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
// The per-element functions are sawyer_plan.h's (tabletop_plan.h's for the dimension-free items), shared with the host twins of tabletop_host.cpp.
// The candidates go through memory on purpose: an env step costs tens of thousands of cycles and the whole array of a realistic call is about a megabyte, so there is
// no fourth inclusion of the rollout kernel's text with the noise inside.
#include <hip/hip_runtime.h>

#include "sawyer_plan.h"
#include "sawyer_value.h"   // the rules of earl_plan_value on these envs (earl_sawyer_plan_mppi_value)
#include "sawyer_prior.h"   // the rules of earl_sawyer_plan_prior and the `_prior` block (earl_sawyer_plan_mppi_prior)

static_assert(earl::kSawyerPriorDraw == earl::kPlanDraw, "earl_sawyer_branch_rollout_prior draws the noise of MPPI's branch k");

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kCandThreads = 256;
constexpr long long kCandMaxBlocks = 1 << 20;      // (the grid-stride loop takes what lies beyond: 2^28 candidates per pass)
constexpr int kUpdateThreads = 512, kUpdateWaves = kUpdateThreads / 64;

__global__ __launch_bounds__(kCandThreads) void sawyer_plan_candidates_kernel(const SawyerPlanArgs p, float* __restrict__ act_out) {
  const unsigned long long total = (unsigned long long)p.K * (unsigned long long)p.H * (unsigned long long)p.n;
  const unsigned long long stride = (unsigned long long)gridDim.x * kCandThreads;
  for (unsigned long long e = (unsigned long long)blockIdx.x * kCandThreads + threadIdx.x; e < total; e += stride) {
    const unsigned long long kt = e / (unsigned)p.n;
    const int i = (int)(e - kt * (unsigned)p.n), k = (int)(kt / (unsigned)p.H), t = (int)(kt - (unsigned long long)k * (unsigned)p.H);
    float m[4], c[4];
    splan_mean(p, i, t, m);
    splan_candidate(p, i, (uint32_t)k, (uint32_t)t, m, c);
    *reinterpret_cast<float4*>(act_out + e * 4) = float4{c[0], c[1], c[2], c[3]};      // (e IS splan_act_index(p, i, k, t) / 4)
  }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor((long long)v, s);
  return v;
}

__global__ __launch_bounds__(kUpdateThreads) void sawyer_plan_update_kernel(const SawyerPlanArgs p) {
  __shared__ int32_t w_lds[EARL_SAWYER_PLAN_MAX_K];
  __shared__ double b_lds[kUpdateWaves];
  __shared__ int32_t k_lds[kUpdateWaves];
  const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = p.n, K = p.K;

  // item 4: beta and best_k -- a lane over its k ascending, the lanes of a wave by shuffles, the waves through LDS (plan_best_merge is a total order: every lane ends alike)
  double beta = -__builtin_inf();
  int bk = 0;
  for (int k = tid; k < K; k += kUpdateThreads) plan_best(p.ret[(size_t)k * n + i], k, beta, bk);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double ob = __shfl_xor(beta, s);
    const int ok = __shfl_xor(bk, s);
    plan_best_merge(ob, ok, beta, bk);
  }
  if (lane == 0) {
    b_lds[wave] = beta;
    k_lds[wave] = bk;
  }
  __syncthreads();
  beta = b_lds[0];
  bk = k_lds[0];
#pragma unroll
  for (int v = 1; v < kUpdateWaves; ++v) plan_best_merge(b_lds[v], k_lds[v], beta, bk);

  // the integer weights, once per (k, env)
  for (int k = tid; k < K; k += kUpdateThreads) w_lds[k] = plan_weight(p.ret[(size_t)k * n + i], beta, p.inv_temperature);
  __syncthreads();

  // item 5: a wave per plan step, its lanes over k.  Row t of the mean is read by this wave before it writes row t of the plan and by no other: plan == mean is safe.
  for (int t = wave; t < p.H; t += kUpdateWaves) {
    float m[4];
    splan_mean(p, i, t, m);
    int64_t A[4] = {0, 0, 0, 0}, S = 0;
    for (int k = lane; k < K; k += 64) {
      const int32_t W = w_lds[k];
      S += W;
      if (W != 0 && k > 0) {                                                        // (branch 0 is the mean: delta = 0)
        const float4 v = *reinterpret_cast<const float4*>(p.act + splan_act_index(p, i, k, t));
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

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return EARL_OK;
}

int launch_candidates(const SawyerPlanArgs& p, float* act_out, hipStream_t stream) {
  const long long total = (long long)p.K * p.H * p.n, want = (total + kCandThreads - 1) / kCandThreads;
  sawyer_plan_candidates_kernel<<<dim3((unsigned)(want < kCandMaxBlocks ? want : kCandMaxBlocks)), kCandThreads, 0, stream>>>(p, act_out);
  return launched("sawyer_plan_candidates_kernel");
}

int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" {

// the block, carved in earl_sawyer_plan_mppi: the branch launch's workspace (rounded up to 8 bytes), then the candidates at the next 16-byte ADDRESS (base is only
// 8-byte aligned: 8 bytes of slack)
int earl_sawyer_plan_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes) {
  int64_t branch = 0;
  if (!bytes || H < 0) return EARL_ERR_ARG;
  if (int rc = earl_sawyer_branch_ws_bytes(nv, K, n, &branch)) return rc;
  *bytes = (int64_t)K * n == 0 ? 0 : round_up(branch, 8) + 8 + (int64_t)K * H * n * 16;
  return EARL_OK;
}

int earl_sawyer_plan_candidates(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, float* act_out, earl_stream_t stream) {
  if (int rc = check_sawyer_plan(SawyerPlanCall::Candidates, cfg, params, j, mean, act_out)) return rc;
  if ((reinterpret_cast<uintptr_t>(act_out) & 15) != 0) return fail(EARL_ERR_ARG, "act_out is not 16-byte aligned");
  if (cfg->n == 0) return EARL_OK;
  SawyerPlanArgs p = sawyer_plan_args(cfg, params, mean);
  p.word0 = kPlanDraw | (uint32_t)j;
  return launch_candidates(p, act_out, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// The body of earl_sawyer_plan_mppi and earl_sawyer_plan_mppi_value.  pv NULL (the value-free entry point, and `_value` with pv NULL or {1.0, NULL}): item 3 is
// earl_sawyer_branch_rollout, the block earl_sawyer_plan_ws_bytes'.  Otherwise item 3 is earl_sawyer_branch_rollout_value (sawyer_value.hip) and the block
// earl_sawyer_value_ws_bytes': that call's [K n] discounts sit between the branch launch's rows and the candidates.  Nothing else differs.
// prior NULL: as above.  Otherwise (earl_sawyer_plan_mppi_prior with branches >= 1; pv as the caller gave it, NULL included) item 3 is earl_sawyer_branch_rollout_prior's
// body with this planner's draw word, which OVERWRITES the last `branches` blocks of the candidates the kernel above it wrote; the block is earl_sawyer_prior_ws_bytes'.
// The update kernel reads the candidates back and does not know.
int plan_mppi(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
              const earl_sawyer_plan_params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0,
              double* best_ret, int32_t* best_k, int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream) {
  if (int rc = check_sawyer_plan(SawyerPlanCall::Mppi, cfg, params, 0, mean, plan)) return rc;
  if (int rc = check_sawyer_value(pv, g_err)) return rc;
  if (prior) {
    const uint64_t rows = (uint64_t)params->H * (uint64_t)cfg->n * 16u;
    const void* const in[4] = {mean, plan, nullptr, nullptr};
    const uint64_t in_bytes[4] = {rows, rows, 0, 0};
    if (int rc = check_sawyer_prior(prior, params->K, params->H, cfg->n, in, in_bytes, g_err)) return rc;
    if (prior->branches == 0) prior = nullptr;                                        // (the identity: from here on the `_value` call, launch for launch)
  }
  if (!ret) return fail(EARL_ERR_ARG, "ret is NULL: the branch launch writes it and the update reads it");
  if (!ws) return fail(EARL_ERR_ARG, "ws is NULL");
  const int n = cfg->n, K = params->K, H = params->H;
  int64_t branch = 0, need = 0;
  if (earl_sawyer_branch_ws_bytes(nv, K, n, &branch) ||
      (prior ? earl_sawyer_prior_ws_bytes(nv, K, H, n, &need) : (pv ? earl_sawyer_value_ws_bytes(nv, K, H, n, &need) : earl_sawyer_plan_ws_bytes(nv, K, H, n, &need))))
    return fail(EARL_ERR_ARG, "nv = %d: 10 (door) or 15 (peg)", nv);
  branch = round_up(branch, 8);
  // (what the scoring call takes of the block: earl_sawyer_prior_ws_bytes / earl_sawyer_value_ws_bytes with H = 0)
  const int64_t scored = prior ? sawyer_prior_scored_bytes(branch, (int64_t)K * n) : (pv ? branch + (int64_t)K * n * 8 : branch);
  if (n > 0 && (!ws->base || (reinterpret_cast<uintptr_t>(ws->base) & 7) != 0 || ws->bytes < need))
    return fail(EARL_ERR_ARG, "ws: base %p (8-byte aligned), %lld bytes of the %lld needed", ws->base, (long long)ws->bytes, (long long)need);
  const earl_sawyer_branch_ws bws{ws->base, branch};
  const earl_sawyer_branch_ws vws{ws->base, scored};
  float* const act = n > 0 ? reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws->base) + (uintptr_t)scored + 15) & ~(uintptr_t)15) : plan;
  const earl_episode_summary sum{ret, nullptr, nullptr};
  // everything the branch launch refuses in model / col / cfg / st / nv and the lane switch, decided by the branch launch itself: with H = 0 it returns after its
  // checks and before its first HIP call
  if (int rc = earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, 0, act, 0, clock, &bws, &sum, nullptr, fail_count, stream))
    return fail(rc, "earl_sawyer_branch_rollout refuses model / col / cfg / st / nv (or earl_debug_set_physics_lanes(64) is set)");
  if (n == 0) return EARL_OK;
  SawyerPlanArgs p = sawyer_plan_args(cfg, params, mean);
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
    if (prior) {
      if (int rc = earl_unit_sawyer_branch_scored_prior(model, col, nv, cfg, st, K, H, act, (int64_t)H * n * 4, clock, pv, prior, p.word0, p.noise_counter, &vws, &sum, nullptr,
                                                        last ? fail_count : nullptr, stream))
        return rc == EARL_ERR_ARG ? rc : fail(rc, "earl_sawyer_branch_rollout_prior failed in iteration %d", params->iteration0 + it);
    } else
    if (int rc = pv ? earl_sawyer_branch_rollout_value(model, col, nv, cfg, st, K, H, act, (int64_t)H * n * 4, clock, pv, &vws, &sum, nullptr, last ? fail_count : nullptr, stream)
                    : earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, H, act, (int64_t)H * n * 4, clock, &bws, &sum, nullptr, last ? fail_count : nullptr, stream))
      return fail(rc, "earl_sawyer_branch_rollout%s failed in iteration %d", pv ? "_value" : "", params->iteration0 + it);
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

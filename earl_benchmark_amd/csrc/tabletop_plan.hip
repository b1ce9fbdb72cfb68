// tabletop_plan.hip -- earl_tabletop_plan_mppi / earl_tabletop3_plan_mppi / earl_tabletop_plan_candidates (include/earl_tabletop.h, "MPPI planning"): I iterations of
// sample -> score -> reweight with the K candidate plans never in memory.  Per iteration two launches on the caller's stream, ordered by the stream alone (no
// cooperative launch, no grid-wide barrier, no flag between workgroups); the per-lane functions are tabletop_plan.h's plan_*, shared with the host twin.
//
// plan_score_kernel   (tabletop_plan_kernel.inc: one text with tabletop_plan_value.hip)
//                     the branch launch's shape: one lane per (branch, env), a wave = 64 consecutive envs of ONE branch (so `k == 0`, the plan itself, is
//                     wave-uniform), a workgroup = that wave, 1-D grid of K * ceil(n / 64).  Per env-step a lane loads 12 B of the mean, makes one Philox block
//                     and three quantiles, and stores nothing; at the end one float64 (and ret0 for k = 0).  No LDS.
// plan_update_kernel  one lane per (env, step): a workgroup is 64 consecutive envs x kPlanUpdateSteps steps, wave w = step t0 + w, so that what all steps of an
//                     env share -- beta, best_k and the integer weights W_k -- is computed ONCE per workgroup and handed round through LDS: every wave takes the
//                     max over its share of the K returns (merged through 6 KB), then per chunk of kPlanChunk branches the waves split the chunk's W_k
//                     (one exp_f32 each) into a [kPlanChunk][64] int32 tile (16 KB) and every lane walks the tile in ascending k: Philox block, three quantiles,
//                     three 64-bit multiply-adds in registers.  A lane reads its three words of the mean before the loop and writes its three words of the
//                     plan after it and nobody else touches them: plan == mean is safe.  Chosen over a [K, n] weight workspace (the ABI has none and the library
//                     allocates nothing) and over a weights-only first launch (a third launch per iteration for K * n exps); the price is that W_k is made
//                     ceil(H / kPlanUpdateSteps) times instead of once, one exp_f32 per kPlanUpdateSteps Philox blocks of the loop it feeds.
// plan_candidates_kernel  the score kernel's grid, the candidates stored instead of stepped.
#include <hip/hip_runtime.h>

#include "tabletop_hostside.h"
#include "tabletop_plan.h"

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kPlanChunk = 64;   // branches whose weights an update workgroup holds at a time

__global__ __launch_bounds__(kBranchBlock) void plan_candidates_kernel(const PlanArgs p, float* __restrict__ act_out, const unsigned tiles) {
  const unsigned k = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - k * tiles) * kBranchBlock + threadIdx.x;
  if (i < (unsigned)p.a.cfg.n) plan_candidates_body(p, (int)i, (int)k, act_out);
}

__global__ __launch_bounds__(kBranchBlock* kPlanUpdateSteps) void plan_update_kernel(const PlanArgs p, const unsigned tiles) {
  __shared__ int32_t w_lds[kPlanChunk][kBranchBlock];
  __shared__ double b_lds[kPlanUpdateSteps][kBranchBlock];
  __shared__ int32_t k_lds[kPlanUpdateSteps][kBranchBlock];
  const unsigned lane = threadIdx.x % kBranchBlock, w = threadIdx.x / kBranchBlock;
  const unsigned tg = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - tg * tiles) * kBranchBlock + lane, t = tg * kPlanUpdateSteps + w;
  const int n = p.a.cfg.n, K = p.K;
  const bool env = i < (unsigned)n, live = env && t < (unsigned)p.a.T;   // (dead lanes keep walking: the barriers below are the whole workgroup's)

  double beta = -__builtin_inf();
  int bk = 0;
  if (env)
    for (int k = (int)w; k < K; k += kPlanUpdateSteps) plan_best(p.ret[(size_t)k * n + i], k, beta, bk);
  b_lds[w][lane] = beta;
  k_lds[w][lane] = bk;
  __syncthreads();
  beta = b_lds[0][lane];
  bk = k_lds[0][lane];
#pragma unroll
  for (int v = 1; v < kPlanUpdateSteps; ++v) plan_best_merge(b_lds[v][lane], k_lds[v][lane], beta, bk);

  float m[3] = {0.0f, 0.0f, 0.0f};
  if (live) plan_mean(p, (int)i, (int)t, m);
  int64_t A[3] = {0, 0, 0}, S = 0;
  for (int k0 = 0; k0 < K; k0 += kPlanChunk) {
    if (k0) __syncthreads();   // every lane is done with the previous tile
    for (int kk = (int)w; kk < kPlanChunk; kk += kPlanUpdateSteps) {
      const int k = k0 + kk;
      w_lds[kk][lane] = env && k < K ? plan_weight(p.ret[(size_t)k * n + i], beta, p.inv_temperature) : 0;
    }
    __syncthreads();
    if (live) {
      const int kn = K - k0 < kPlanChunk ? K - k0 : kPlanChunk;
      for (int kk = 0; kk < kn; ++kk) {
        const int32_t W = w_lds[kk][lane];
        S += W;
        if (W != 0 && k0 + kk > 0) plan_accumulate(p, (int)i, (uint32_t)(k0 + kk), t, m, W, A);   // (branch 0 is the mean: delta = 0)
      }
    }
  }
  if (live) {
    float* dst = p.plan + ((size_t)t * n + i) * 3;
    dst[0] = plan_new_mean(m[0], A[0], S);
    dst[1] = plan_new_mean(m[1], A[1], S);
    dst[2] = plan_new_mean(m[2], A[2], S);
    if (t == 0) {
      if (p.best_ret) p.best_ret[i] = beta;
      if (p.best_k) p.best_k[i] = bk;
    }
  }
}

}  // namespace

// the update launch, for this unit's do_plan and for tabletop_plan_value.hip's (the update sees returns only: one kernel serves both)
namespace earl {
void plan_update_launch(const PlanArgs& p, unsigned tiles, unsigned ublocks, earl_stream_t stream) {
  plan_update_kernel<<<dim3(ublocks), kBranchBlock * kPlanUpdateSteps, 0, (hipStream_t)stream>>>(p, tiles);
}
}  // namespace earl

namespace {

#include "tabletop_plan_kernel.inc"   // plan_score_kernel and do_plan: one text with tabletop_plan_value.hip

}  // namespace

extern "C" {

int earl_tabletop_plan_mppi(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan, double* ret,
                            double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  return do_plan<1>(cfg, st, params, nullptr, mean, plan, ret, ret0, best_ret, best_k, stream);
}

int earl_tabletop3_plan_mppi(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const float* mean, float* plan, double* ret,
                             double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  return do_plan<3>(cfg, st, params, nullptr, mean, plan, ret, ret0, best_ret, best_k, stream);
}

int earl_tabletop_plan_candidates(const earl_tabletop_cfg* cfg, const earl_plan_params* params, int32_t j, const float* mean, float* act_out, earl_stream_t stream) {
  long long blocks, ublocks;
  if (int rc = check_plan(cfg, nullptr, 1, params, j, mean, act_out, nullptr, &blocks, &ublocks)) return rc;
  if (blocks == 0) return EARL_OK;
  PlanArgs p = plan_args(cfg, nullptr, params, mean, thresholds());
  p.word0 = kPlanDraw | (uint32_t)j;
  plan_candidates_kernel<<<dim3((unsigned)blocks), kBranchBlock, 0, (hipStream_t)stream>>>(p, act_out, (unsigned)(blocks / params->K));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "plan_candidates_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

}  // extern "C"

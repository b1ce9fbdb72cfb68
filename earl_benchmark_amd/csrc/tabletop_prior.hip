// tabletop_prior.hip -- earl_tabletop_plan_mppi_prior / earl_tabletop3_plan_mppi_prior (include/earl_tabletop.h, "MPPI with policy-prior branches"): the planner of
// tabletop_plan.hip / tabletop_plan_value.hip with P of its K candidates rolled out closed loop under a policy evaluated by the lane that owns the branch.  Per
// iteration THREE launches on the caller's stream, ordered by the stream alone; the per-lane functions are tabletop_plan.h's and tabletop_prior.h's, shared with the
// host twin.  A unit of its own: the six existing planner units compile to what they compiled to.
//
// prior_noise_kernel   plan_score_kernel's shape and body (plan_score_body) over the K - P branches that are NOT prior branches: workgroup index kk -> branch
//                      kk == 0 ? 0 : kk + P.  Same registers and occupancy as plan_score_kernel: the network is not in this kernel.
// prior_score_kernel   the same shape over the P prior branches, branch 1 + kk: prior_score_body.  A wave is 64 envs of ONE branch and every wave of this launch
//                      is a prior branch, so the policy's weights are wave-uniform scalar loads.  No LDS.
//                      The split was chosen over one kernel for all k (where the noise branches would inherit the network's register allocation and lose
//                      occupancy through the env step) and over scoring all K with the noise body first (P / K of that launch thrown away).  Its price is one
//                      more launch per iteration; the two score launches write disjoint rows of `ret` and could overlap, but run in stream order.
// prior_update_kernel  plan_update_kernel's text with the walk's candidate of k <= P loaded from prior->act (12 B per (k, env, step)) instead of made again.
#include <hip/hip_runtime.h>

#include "tabletop_hostside.h"
#include "tabletop_prior.h"

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kPlanChunk = 64;   // branches whose weights an update workgroup holds at a time (tabletop_plan.hip's)

template <int NOBJ, bool GENERAL, bool VALUE>
__global__ __launch_bounds__(kBranchBlock) void prior_noise_kernel(const PlanPriorArgs p, const unsigned tiles) {
  const unsigned kk = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - kk * tiles) * kBranchBlock + threadIdx.x;
  const unsigned k = kk ? kk + (unsigned)p.pr.P : 0u;
  if (i < (unsigned)p.a.cfg.n) plan_score_body<NOBJ, GENERAL, VALUE>(p, (int)i, (int)k, &p.v);
}

template <int NOBJ, bool GENERAL, bool VALUE>
__global__ __launch_bounds__(kBranchBlock) void prior_score_kernel(const PlanPriorArgs p, const unsigned tiles) {
  const unsigned kk = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - kk * tiles) * kBranchBlock + threadIdx.x;
  if (i < (unsigned)p.a.cfg.n) prior_score_body<NOBJ, GENERAL, VALUE>(p, (int)i, (int)(kk + 1));
}

__global__ __launch_bounds__(kBranchBlock* kPlanUpdateSteps) void prior_update_kernel(const PlanPriorArgs p, const unsigned tiles) {
  __shared__ int32_t w_lds[kPlanChunk][kBranchBlock];
  __shared__ double b_lds[kPlanUpdateSteps][kBranchBlock];
  __shared__ int32_t k_lds[kPlanUpdateSteps][kBranchBlock];
  const unsigned lane = threadIdx.x % kBranchBlock, w = threadIdx.x / kBranchBlock;
  const unsigned tg = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - tg * tiles) * kBranchBlock + lane, t = tg * kPlanUpdateSteps + w;
  const int n = p.a.cfg.n, K = p.K, P = p.pr.P;
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
        const int k = k0 + kk;
        S += W;
        if (W != 0 && k > 0) {                          // (branch 0 is the mean: delta = 0)
          if (k <= P) prior_accumulate(p, (int)i, (uint32_t)k, t, m, W, A);
          else plan_accumulate(p, (int)i, (uint32_t)k, t, m, W, A);
        }
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

template <int NOBJ, bool GENERAL, bool VALUE>
void launch_iteration(const PlanPriorArgs& p, unsigned tiles, unsigned ublocks, hipStream_t s) {
  const unsigned P = (unsigned)p.pr.P;
  prior_noise_kernel<NOBJ, GENERAL, VALUE><<<dim3(((unsigned)p.K - P) * tiles), kBranchBlock, 0, s>>>(p, tiles);
  if (P) prior_score_kernel<NOBJ, GENERAL, VALUE><<<dim3(P * tiles), kBranchBlock, 0, s>>>(p, tiles);
  prior_update_kernel<<<dim3(ublocks), kBranchBlock * kPlanUpdateSteps, 0, s>>>(p, tiles);
}

template <int NOBJ>
int do_plan_prior(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, const earl_plan_value* pv, const earl_plan_prior* prior,
                  const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  long long blocks, ublocks;
  if (int rc = check_plan(cfg, st, NOBJ, pp, 0, mean, plan, ret, &blocks, &ublocks)) return rc;
  if (pv)
    if (int rc = check_plan_value(pv, Dims<NOBJ>::NOBS)) return rc;
  if (int rc = check_plan_prior(cfg, pp, prior, Dims<NOBJ>::NOBS, mean, plan, ret)) return rc;
  if (blocks == 0) return EARL_OK;
  PlanPriorArgs p{};
  static_cast<PlanArgs&>(p) = plan_args(cfg, st, pp, mean, thresholds());
  if (pv) p.v = value_args(pv);
  p.pr = prior_args(prior);
  p.plan = plan;
  p.ret = ret;
  const unsigned tiles = (unsigned)(blocks / pp->K);
  const bool general = is_general(cfg), value = pv != nullptr;
  const hipStream_t s = (hipStream_t)stream;
  for (int it = 0; it < pp->iterations; ++it) {
    const bool last = it + 1 == pp->iterations;
    p.mean = it ? plan : mean;
    p.word0 = kPlanDraw | (uint32_t)(pp->iteration0 + it);
    p.ret0 = ret0 ? ret0 + (size_t)it * cfg->n : nullptr;
    p.best_ret = last ? best_ret : nullptr;
    p.best_k = last ? best_k : nullptr;
    if (general) value ? launch_iteration<NOBJ, true, true>(p, tiles, (unsigned)ublocks, s) : launch_iteration<NOBJ, true, false>(p, tiles, (unsigned)ublocks, s);
    else value ? launch_iteration<NOBJ, false, true>(p, tiles, (unsigned)ublocks, s) : launch_iteration<NOBJ, false, false>(p, tiles, (unsigned)ublocks, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "plan prior kernels: %s", hipGetErrorString(e));
  }
  return EARL_OK;
}

}  // namespace

extern "C" {

int earl_tabletop_plan_mppi_prior(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                  const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                                  earl_stream_t stream) {
  return do_plan_prior<1>(cfg, st, params, pv, prior, mean, plan, ret, ret0, best_ret, best_k, stream);
}

int earl_tabletop3_plan_mppi_prior(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                   const earl_plan_prior* prior, const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k,
                                   earl_stream_t stream) {
  return do_plan_prior<3>(cfg, st, params, pv, prior, mean, plan, ret, ret0, best_ret, best_k, stream);
}

}  // extern "C"

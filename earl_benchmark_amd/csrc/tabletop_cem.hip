// tabletop_cem.hip -- earl_tabletop_plan_cem / earl_tabletop3_plan_cem / earl_tabletop_cem_candidates (include/earl_tabletop.h, "CEM planning"): I iterations of
// sample -> score -> select -> refit with the K candidate plans never in memory.  Per iteration two launches on the caller's stream, ordered by the stream alone (no
// cooperative launch, no grid-wide barrier, no flag between workgroups); the per-lane functions are tabletop_cem.h's, shared with the host twin.
//
// cem_score_kernel    plan_score_kernel's shape: one lane per (branch, env), a wave = 64 consecutive envs of ONE branch, a workgroup = that wave, 1-D grid of
//                     K * ceil(n / 64).  Per env-step a lane loads 12 B of the mean and 12 B of the std (eight steps in flight), makes one Philox block and three
//                     quantiles, and stores nothing; at the end one float64 (and ret0 for k = 0).  No LDS.  VALUE: the discounted sum and the value network of
//                     tabletop_value.h on the lane's own last row, as plan_score_kernel of tabletop_plan_value.hip.
// cem_update_kernel   plan_update_kernel's shape: a workgroup is 64 consecutive envs x kPlanUpdateSteps steps, wave w = step t0 + w.  What all steps of an env share
//                     -- the elite set, beta and best_k -- is computed ONCE per workgroup: the waves split k in tiles of kCemRankTile, a lane counts the ranks of its
//                     tile's (k, env) against all K returns of its env in one pass (loads coalesced over the env lanes, each compared kCemRankTile times as the
//                     integer keys of cem_key) and an elite sets bit k of its env's mask in LDS: ceil(K / 32) words per env lane, 8 KB at K = 1024.
//                     After one barrier every (env, step) lane walks the set bits only: per elite one Philox block, three quantiles, six int64 multiply-adds in
//                     registers; Ne is the number of bits it met.  A lane reads its three words of mean and std before the loop and writes its three words of plan
//                     and std after it and nobody else touches them: plan == mean and std == std0 are safe.
// cem_candidates_kernel  the score kernel's grid, the candidates stored instead of stepped.
#include <hip/hip_runtime.h>

#include "tabletop_cem.h"

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kCemMaskWords = (kCemMaxK + 31) / 32;
constexpr int kCemRankTile = 8;   // branches a lane ranks per pass over its env's returns

__global__ __launch_bounds__(kBranchBlock) void cem_candidates_kernel(const CemArgs c, float* __restrict__ act_out, const unsigned tiles) {
  const unsigned k = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - k * tiles) * kBranchBlock + threadIdx.x;
  if (i < (unsigned)c.p.a.cfg.n) cem_candidates_body(c, (int)i, (int)k, act_out);
}

template <int NOBJ, bool GENERAL, bool VALUE>
__global__ __launch_bounds__(kBranchBlock) void cem_score_kernel(const CemArgs c, const unsigned tiles) {
  const unsigned k = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - k * tiles) * kBranchBlock + threadIdx.x;
  if (i < (unsigned)c.p.a.cfg.n) cem_score_body<NOBJ, GENERAL, VALUE>(c, (int)i, (int)k);
}

__global__ __launch_bounds__(kBranchBlock* kPlanUpdateSteps) void cem_update_kernel(const CemArgs c, const unsigned tiles) {
  __shared__ uint32_t e_lds[kCemMaskWords][kBranchBlock];
  __shared__ double b_lds[kPlanUpdateSteps][kBranchBlock];
  __shared__ int32_t k_lds[kPlanUpdateSteps][kBranchBlock];
  const PlanArgs& p = c.p;
  const unsigned lane = threadIdx.x % kBranchBlock, w = threadIdx.x / kBranchBlock;
  const unsigned tg = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - tg * tiles) * kBranchBlock + lane, t = tg * kPlanUpdateSteps + w;
  const int n = p.a.cfg.n, K = p.K, words = (K + 31) / 32;
  const bool env = i < (unsigned)n, live = env && t < (unsigned)p.a.T;

  for (int v = (int)w; v < words; v += kPlanUpdateSteps) e_lds[v][lane] = 0u;
  __syncthreads();
  double beta = -__builtin_inf();
  int bk = 0;
  if (env) {   // a wave takes tiles of kCemRankTile consecutive k: one pass over the K returns ranks the tile's branches, each load compared kCemRankTile times
    const double* col = p.ret + i;
    for (int k0 = (int)w * kCemRankTile; k0 < K; k0 += kPlanUpdateSteps * kCemRankTile) {
      uint64_t key[kCemRankTile];
      int rank[kCemRankTile];
#pragma unroll
      for (int j = 0; j < kCemRankTile; ++j) {
        const int k = k0 + j < K ? k0 + j : K - 1;
        const double r = col[(size_t)k * n];
        if (k0 + j < K) plan_best(r, k, beta, bk);
        key[j] = cem_key(r);
        rank[j] = 0;
      }
      for (int k2 = 0; k2 < K; ++k2) {
        const uint64_t u = cem_key(col[(size_t)k2 * n]);
#pragma unroll
        for (int j = 0; j < kCemRankTile; ++j) rank[j] += (u > key[j] || (u == key[j] && k2 < k0 + j)) ? 1 : 0;
      }
#pragma unroll
      for (int j = 0; j < kCemRankTile; ++j)
        if (k0 + j < K && rank[j] < c.E && key[j] != 0ull) atomicOr(&e_lds[(k0 + j) >> 5][lane], 1u << ((k0 + j) & 31));   // (key 0: a NaN)
    }
  }
  b_lds[w][lane] = beta;
  k_lds[w][lane] = bk;
  __syncthreads();
  if (!live) return;   // (no barrier below)
  beta = b_lds[0][lane];
  bk = k_lds[0][lane];
#pragma unroll
  for (int v = 1; v < kPlanUpdateSteps; ++v) plan_best_merge(b_lds[v][lane], k_lds[v][lane], beta, bk);

  float m[3], s[3];
  plan_mean(p, (int)i, (int)t, m);
  cem_std(c, (int)i, (int)t, s);
  int64_t A1[3] = {0, 0, 0}, A2[3] = {0, 0, 0};
  int32_t Ne = 0;
  for (int v = 0; v < words; ++v) {
    uint32_t bits = e_lds[v][lane];
    Ne += __builtin_popcount(bits);
    if (v == 0) bits &= ~1u;   // (branch 0 is the mean: D = 0)
    while (bits) {
      const int b = __builtin_ctz(bits);
      bits &= bits - 1;
      cem_accumulate(p, (int)i, (uint32_t)(v * 32 + b), t, m, s, A1, A2);
    }
  }
  const size_t row = ((size_t)t * n + i) * 3;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    p.plan[row + d] = cem_new_mean(m[d], A1[d], Ne, c.alpha);
    c.std_out[row + d] = cem_new_std(s[d], A1[d], A2[d], Ne, c.alpha, c.std_min, c.std_max);
  }
  if (t == 0) {
    if (p.best_ret) p.best_ret[i] = beta;
    if (p.best_k) p.best_k[i] = bk;
  }
}

template <int NOBJ, bool VALUE>
void score_launch(const CemArgs& c, bool general, unsigned blocks, unsigned tiles, hipStream_t s) {
  if (general) cem_score_kernel<NOBJ, true, VALUE><<<dim3(blocks), kBranchBlock, 0, s>>>(c, tiles);
  else cem_score_kernel<NOBJ, false, VALUE><<<dim3(blocks), kBranchBlock, 0, s>>>(c, tiles);
}

template <int NOBJ>
int do_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* cp, const earl_plan_value* pv, const float* mean, const float* std0,
           float* plan, float* std_out, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  long long blocks, ublocks;
  if (int rc = check_cem(cfg, st, NOBJ, Dims<NOBJ>::NOBS, cp, pv, 0, mean, std0, plan, std_out, ret, &blocks, &ublocks)) return rc;
  if (blocks == 0) return EARL_OK;
  CemArgs c = cem_args(cfg, st, cp, pv, mean, std0, thresholds());
  c.p.plan = plan;
  c.p.ret = ret;
  c.std_out = std_out;
  const unsigned tiles = (unsigned)(blocks / cp->K);
  const bool general = is_general(cfg);
  const hipStream_t s = (hipStream_t)stream;
  for (int it = 0; it < cp->iterations; ++it) {
    const bool last = it + 1 == cp->iterations;
    c.p.mean = it ? plan : mean;
    c.std_in = it ? std_out : std0;
    c.p.word0 = kCemDraw | (uint32_t)(cp->iteration0 + it);
    c.p.ret0 = ret0 ? ret0 + (size_t)it * cfg->n : nullptr;
    c.p.best_ret = last ? best_ret : nullptr;
    c.p.best_k = last ? best_k : nullptr;
    if (pv) score_launch<NOBJ, true>(c, general, (unsigned)blocks, tiles, s);
    else score_launch<NOBJ, false>(c, general, (unsigned)blocks, tiles, s);
    cem_update_kernel<<<dim3((unsigned)ublocks), kBranchBlock * kPlanUpdateSteps, 0, s>>>(c, tiles);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "cem kernels: %s", hipGetErrorString(e));
  }
  return EARL_OK;
}

}  // namespace

extern "C" {

int earl_tabletop_plan_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                           const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  return do_cem<1>(cfg, st, params, pv, mean, std0, plan, std, ret, ret0, best_ret, best_k, stream);
}

int earl_tabletop3_plan_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, const float* mean,
                            const float* std0, float* plan, float* std, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  return do_cem<3>(cfg, st, params, pv, mean, std0, plan, std, ret, ret0, best_ret, best_k, stream);
}

int earl_tabletop_cem_candidates(const earl_tabletop_cfg* cfg, const earl_cem_params* params, int32_t j, const float* mean, const float* std, float* act_out,
                                 earl_stream_t stream) {
  long long blocks, ublocks;
  if (int rc = check_cem(cfg, nullptr, 1, 0, params, nullptr, j, mean, std, act_out, nullptr, nullptr, &blocks, &ublocks)) return rc;
  if (blocks == 0) return EARL_OK;
  CemArgs c = cem_args(cfg, nullptr, params, nullptr, mean, std, thresholds());
  c.p.word0 = kCemDraw | (uint32_t)j;
  cem_candidates_kernel<<<dim3((unsigned)blocks), kBranchBlock, 0, (hipStream_t)stream>>>(c, act_out, (unsigned)(blocks / params->K));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "cem_candidates_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

}  // extern "C"

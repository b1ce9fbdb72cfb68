// sawyer_shoot.h -- what the two shooting planners of the Sawyer door / peg (sawyer_plan.hip: MPPI, sawyer_cem.hip: CEM) share, stated once:
//   per element   the clipped row of the plan, where a candidate lives in [K, H, n, 4], the candidate itself (one Philox block, four quantiles around the row, scaled by
//                 MPPI's sigma, CEM's std or a prior's sigma) and the fixed-point delta of the integer sums -- for the kernels and, under -DEARL_HOST_BUILD, for the host
//                 twins of tabletop_host.cpp;
//   device        the int64 wave sum, the workgroup's beta / best_k reduction and the candidates kernels' walk over (k, t, env);
//   host          the ONE statement of the workspace block (sawyer_ws_layout: the three public `*_ws_bytes` functions, the scoring call and the planner drivers read it
//                 and nothing else), the ONE scoring call of an iteration (earl_unit_sawyer_branch_scored, sawyer_value.hip) and everything a planner driver does between
//                 its own argument check and its iteration loop (sawyer_shoot_open).
// No stepper header: the planners reach the stepper through the public ABI and the hidden earl_unit_* calls.
#pragma once
#include "sawyer_prior.h"
#include "sawyer_value.h"
#include "tabletop_hostside.h"   // fail: the thread-local message behind earl_last_error
#include "tabletop_plan.h"       // plan_clip, plan_best_merge, the Philox block and the quantile
#include "../../include/earl_physics.h"

namespace earl {

// item 1: row t of env i of the plan entering, all four words clipped
__device__ __forceinline__ void shoot_mean(const float* mean, int n, int i, int t, float (&m)[4]) {
  const float* mp = mean + ((size_t)t * n + i) * 4;
#pragma unroll
  for (int d = 0; d < 4; ++d) m[d] = plan_clip(mp[d]);
}

// where candidate k of (step t, env i) lives in a [K, H, n, 4] array
__device__ __forceinline__ size_t shoot_act_index(int H, int n, int i, int k, int t) { return (((size_t)k * H + t) * n + i) * 4; }

// item 2: candidate k of (step t, the env with global id gid) around the clipped row m -- the row itself for k == 0, else one Philox block and four quantiles, each
// times its scale
__device__ __forceinline__ void shoot_candidate(uint32_t word0, uint32_t gid, uint32_t k, uint32_t t, uint32_t noise_counter, uint64_t seed, const float (&scale)[4],
                                                const float (&m)[4], float (&c)[4]) {
  if (k == 0) {
#pragma unroll
    for (int d = 0; d < 4; ++d) c[d] = m[d];
    return;
  }
  const U4 b = philox4x32_10(U4{word0, gid, (k << 16) | t, noise_counter}, (uint32_t)seed, (uint32_t)(seed >> 32));
  c[0] = plan_clip(fmaf(scale[0], normal_quantile_f32(b.x >> 8), m[0]));
  c[1] = plan_clip(fmaf(scale[1], normal_quantile_f32(b.y >> 8), m[1]));
  c[2] = plan_clip(fmaf(scale[2], normal_quantile_f32(b.z >> 8), m[2]));
  c[3] = plan_clip(fmaf(scale[3], normal_quantile_f32(b.w >> 8), m[3]));
}

// item 5: a candidate's word c, READ back from the candidates, against the clipped row's word m in units of 2^-20: |D| <= 2^21
__device__ __forceinline__ int64_t shoot_delta(float c, float m) { return (int64_t)(int32_t)__builtin_rint((double)(c - m) * 1048576.0); }

#ifndef EARL_HOST_BUILD
// ---------------------------------------------------------------------------------------------------------------- device
constexpr int kCandThreads = 256;
constexpr long long kCandMaxBlocks = 1 << 20;      // (the grid-stride loop takes what lies beyond: 2^28 candidates per pass)

// the candidates kernels' grid and their walk: one lane per (k, t, env) in the order of the [K, H, n, 4] array, f(e, i, k, t) with e = shoot_act_index(H, n, i, k, t) / 4
inline dim3 shoot_candidates_grid(int K, int H, int n) {
  const long long total = (long long)K * H * n, want = (total + kCandThreads - 1) / kCandThreads;
  return dim3((unsigned)(want < kCandMaxBlocks ? want : kCandMaxBlocks));
}
template <class F>
__device__ __forceinline__ void shoot_for_each_candidate(int K, int H, int n, F f) {
  const unsigned long long total = (unsigned long long)K * (unsigned long long)H * (unsigned long long)n;
  const unsigned long long stride = (unsigned long long)gridDim.x * kCandThreads;
  for (unsigned long long e = (unsigned long long)blockIdx.x * kCandThreads + threadIdx.x; e < total; e += stride) {
    const unsigned long long kt = e / (unsigned)n;
    const int i = (int)(e - kt * (unsigned)n), k = (int)(kt / (unsigned)H), t = (int)(kt - (unsigned long long)k * (unsigned)H);
    f(e, i, k, t);
  }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor((long long)v, s);
  return v;
}

// item 4: a lane's (beta, bk) over its own k ascending -> the workgroup's: the lanes of a wave by shuffles, the waves through LDS (plan_best_merge is a total order:
// every lane ends alike)
template <int kThreads>
__device__ __forceinline__ void block_best(double& beta, int& bk, double (&b_lds)[kThreads / 64], int32_t (&k_lds)[kThreads / 64]) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
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
  for (int v = 1; v < kThreads / 64; ++v) plan_best_merge(b_lds[v], k_lds[v], beta, bk);
}

// ---------------------------------------------------------------------------------------------------------------- host
inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hostside::fail(EARL_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return EARL_OK;
}
inline int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline bool misaligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; }

// The block of a scoring call or a planner call, from its 8-byte aligned base: the branch launch's workspace rounded up to 8 bytes (`branch`); Value and Prior: the [K n]
// discounts d_t (the prior kernels are built with the discounted sum and always carry them); Prior: at `queue` the work queue of a prior launch of its own, sized for any
// P < K, 2 ceil(K n / 4) int32 rounded up to 8 bytes -- `scored` bytes, all a scoring call takes; then a planner's [K, H, n, 4] candidates at the next 16-byte ADDRESS
// (8 bytes of slack), for Plain whatever H, otherwise for H > 0 (H = 0 sizes a scoring call).  need: 0 without a virtual env
enum class SawyerWs { Plain, Value, Prior };      // earl_sawyer_plan_ws_bytes, earl_sawyer_value_ws_bytes, earl_sawyer_prior_ws_bytes
struct SawyerWsLayout {
  int64_t branch, queue, scored, need;
};
inline int sawyer_ws_layout(int32_t nv, int32_t K, int32_t H, int32_t n, SawyerWs kind, SawyerWsLayout* L) {
  int64_t branch = 0;
  if (H < 0) return EARL_ERR_ARG;
  if (int rc = earl_sawyer_branch_ws_bytes(nv, K, n, &branch)) return rc;
  const int64_t V = (int64_t)K * n;
  L->branch = round_up(branch, 8);
  L->queue = L->branch + (kind == SawyerWs::Plain ? 0 : V * 8);
  L->scored = L->queue + (kind == SawyerWs::Prior ? round_up(2 * ((V + 3) / 4) * (int64_t)sizeof(int32_t), 8) : 0);
  L->need = V == 0 ? 0 : L->scored + (kind == SawyerWs::Plain || H > 0 ? 8 + V * H * 16 : 0);
  return EARL_OK;
}
// the body of the three public size functions
inline int sawyer_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, SawyerWs kind, int64_t* bytes) {
  SawyerWsLayout L;
  if (!bytes) return EARL_ERR_ARG;
  if (int rc = sawyer_ws_layout(nv, K, H, n, kind, &L)) return rc;
  *bytes = L.need;
  return EARL_OK;
}
// `ws` against what the layout needs: the refusal of the scoring call and of the planners (`whose`: "" or the size function to name)
inline int check_sawyer_ws(const earl_sawyer_branch_ws* ws, int64_t need, const char* whose) {
  if (!ws->base || (reinterpret_cast<uintptr_t>(ws->base) & 7) != 0 || ws->bytes < need)
    return hostside::fail(EARL_ERR_ARG, "ws: base %p (8-byte aligned), %lld bytes of the %lld needed%s", ws->base, (long long)ws->bytes, (long long)need, whose);
  return EARL_OK;
}

}  // namespace earl

// The scoring call of an iteration, and the body of earl_sawyer_branch_rollout_value and earl_sawyer_branch_rollout_prior behind their own checks (sawyer_value.hip).
// prior NULL and pv NULL or {1.0, NULL}: earl_sawyer_branch_rollout with the same arguments, nothing else touched.  prior NULL otherwise: the discounted launch and / or the
// value kernel, `ws` a Value block.  prior given (checked: check_sawyer_prior; branches >= 1): its last branches run by the policy with the noise of word0 = the calling
// planner's draw word | the iteration, pv as given (NULL included), `ws` a Prior block, `act` WRITTEN for those branches
extern "C" __attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_scored(const earl_link_model* model, const earl_collision_model* col, int32_t nv,
                                                                                    const earl_sawyer_cfg* cfg, const earl_sawyer_state* st, int32_t K, int32_t H, float* act,
                                                                                    int64_t act_branch_stride, const uint64_t* clock, const earl_plan_value* pv,
                                                                                    const earl_sawyer_plan_prior* prior, uint32_t word0, uint32_t noise_counter,
                                                                                    const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary, double* last_obs,
                                                                                    int32_t* fail_count, earl_stream_t stream);

namespace earl {

// what a planner call keeps from its prologue for its iterations
struct SawyerShoot {
  const earl_link_model* model;
  const earl_collision_model* col;
  const earl_sawyer_cfg* cfg;
  const earl_sawyer_state* st;
  const earl_plan_value* pv;              // NULL: the plain sum
  const earl_sawyer_plan_prior* prior;    // NULL, or branches >= 1
  const uint64_t* clock;
  int32_t* fail_count;
  float* act;                             // [K, H, n, 4]: the candidates, inside the block
  earl_sawyer_branch_ws ws;               // the scoring call's part of the block
  earl_episode_summary sum;               // {ret, NULL, NULL}
  earl_stream_t stream;
  int32_t nv, K, H, iteration0;
  uint32_t noise_counter;
};

// Everything between a planner's own argument check (check_sawyer_plan / check_sawyer_cem: cfg and params are not NULL) and its iteration loop, refusals in the header's
// order.  pv: NULL where the call reduces to the value-free one.  in: the arrays of H n 16 bytes (or NULL) that prior->act must not overlap.  rows_refusal: NULL, or the
// planner's own refusal of its output rows, due after `ws`.  `plan` stands in for the candidates where n == 0.  The model / col / cfg / st / nv side and the lane switch
// are decided by the branch launch itself: with H = 0 it returns after its checks and before its first HIP call.  n == 0: nothing to launch, *s unset beyond this point
template <class Params>
inline int sawyer_shoot_open(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                             const Params* params, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, const void* const (&in)[4], const char* rows_refusal,
                             float* plan, double* ret, int32_t* fail_count, const uint64_t* clock, const earl_sawyer_branch_ws* ws, earl_stream_t stream, SawyerShoot* s) {
  using hostside::fail;
  const int n = cfg->n, K = params->K, H = params->H;
  if (int rc = check_sawyer_value(pv, hostside::g_err)) return rc;
  if (prior) {
    const uint64_t rows = (uint64_t)H * (uint64_t)n * 16u;
    const uint64_t in_bytes[4] = {rows, rows, rows, rows};
    if (int rc = check_sawyer_prior(prior, K, H, n, in, in_bytes, hostside::g_err)) return rc;
    if (prior->branches == 0) prior = nullptr;                                        // (the identity: from here on the `_value` call, launch for launch)
  }
  if (!ret) return fail(EARL_ERR_ARG, "ret is NULL: the branch launch writes it and the update reads it");
  if (!ws) return fail(EARL_ERR_ARG, "ws is NULL");
  if (rows_refusal) return fail(EARL_ERR_ARG, "%s", rows_refusal);
  SawyerWsLayout L;
  if (sawyer_ws_layout(nv, K, H, n, prior ? SawyerWs::Prior : pv ? SawyerWs::Value : SawyerWs::Plain, &L)) return fail(EARL_ERR_ARG, "nv = %d: 10 (door) or 15 (peg)", nv);
  if (n > 0)
    if (int rc = check_sawyer_ws(ws, L.need, "")) return rc;
  float* const act = n > 0 ? reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws->base) + (uintptr_t)L.scored + 15) & ~(uintptr_t)15) : plan;
  *s = SawyerShoot{model, col, cfg, st, pv, prior, clock, fail_count, act, {ws->base, L.scored}, {ret, nullptr, nullptr}, stream, nv, K, H, params->iteration0,
                   params->noise_counter};
  const earl_sawyer_branch_ws bws{ws->base, L.branch};
  if (int rc = earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, 0, act, 0, clock, &bws, &s->sum, nullptr, fail_count, stream))
    return fail(rc, "earl_sawyer_branch_rollout refuses model / col / cfg / st / nv (or earl_debug_set_physics_lanes(64) is set)");
  return EARL_OK;
}

// item 3 of iteration `it` (word0 = the planner's draw word | iteration0 + it): the candidates in, ret [K, n] (and, on the last iteration, fail) out
inline int sawyer_shoot_score(const SawyerShoot& s, uint32_t word0, int it, bool last) {
  const int rc = earl_unit_sawyer_branch_scored(s.model, s.col, s.nv, s.cfg, s.st, s.K, s.H, s.act, (int64_t)s.H * s.cfg->n * 4, s.clock, s.pv, s.prior, word0, s.noise_counter,
                                                &s.ws, &s.sum, nullptr, last ? s.fail_count : nullptr, s.stream);
  if (rc == EARL_OK || (s.prior && rc == EARL_ERR_ARG)) return rc;                    // (a prior's refusal keeps its own message)
  return hostside::fail(rc, "earl_sawyer_branch_rollout%s failed in iteration %d", s.prior ? "_prior" : s.pv ? "_value" : "", s.iteration0 + it);
}
#endif  // EARL_HOST_BUILD

}  // namespace earl

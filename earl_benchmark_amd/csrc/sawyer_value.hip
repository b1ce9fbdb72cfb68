// sawyer_value.hip -- earl_sawyer_branch_rollout_value / earl_sawyer_value_ws_bytes (include/earl_physics.h, "discount and a terminal value on the door and the peg"):
// the branch launch with ret = sum_t gamma^t r_t + gamma^H V(o_H).  On the caller's stream, ordered by the stream alone:
//   the branch launch       discount == 1: earl_sawyer_branch_rollout through the public ABI, untouched.  discount != 1: the same launch with the rollout kernel built
//                           under EARL_BRANCH_DISCOUNT (physics_branch_value.hip, physics_branch_value_w8.hip; reached through physics.hip, which owns the checks and the
//                           launch forms), d_t in [K n] words of the workspace behind the branch launch's block.
//   sawyer_value_kernel     with a value network: the 16 lanes of a group own one virtual env's last observation row -- the caller's last_obs, or the workspace's carried
//                           rows, which already are those rows -- round it to float32 (element `sub` on lane `sub`), evaluate V with pol_layer<16, ..> of
//                           policy_lane_group.h exactly as the closed loop's policy phase does (first layer K = 14: the element-wise path; then 16-byte pieces), and lane 0
//                           does ret[v] += d_H * (double)V (sawyer_value.h, shared with the host twin).  One launch of K n evaluations per planner iteration, not per step.
// No stepper header here: the unit compiles in seconds and reaches the stepper through two hidden calls into physics.hip.
#include <hip/hip_runtime.h>

#include "sawyer_prior.h"
#include "sawyer_value.h"
#include "tabletop_hostside.h"   // fail: the thread-local message behind earl_last_error
#include "../../include/earl_physics.h"

using namespace earl;
using namespace earl::hostside;

// physics.hip: the branch launch with the discounted sum, and where the carried observation rows of a branch workspace start
extern "C" __attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_discounted(const earl_link_model* model, const earl_collision_model* col, int32_t nv,
                                                                                        const earl_sawyer_cfg* cfg, const earl_sawyer_state* st, int32_t K, int32_t H,
                                                                                        const float* act, int64_t act_branch_stride, const uint64_t* clock,
                                                                                        const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary, double* last_obs,
                                                                                        int32_t* fail, double gamma, double* disc, earl_stream_t stream);
extern "C" __attribute__((visibility("hidden"))) double* earl_unit_sawyer_branch_rows(int32_t nv, int64_t V, void* base);
// ... and with the last branches run by a policy (sawyer_prior.h: SawyerPriorLaunch)
extern "C" __attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv,
                                                                                   const earl_sawyer_cfg* cfg, const earl_sawyer_state* st, int32_t K, int32_t H, float* act,
                                                                                   int64_t act_branch_stride, const uint64_t* clock, const earl_sawyer_branch_ws* ws,
                                                                                   const earl_episode_summary* summary, double* last_obs, int32_t* fail, double gamma,
                                                                                   double* disc, const earl::SawyerPriorLaunch* pr, earl_stream_t stream);

namespace {
#include "policy_lane_group.h"

constexpr int kValueThreads = 256, kValueEnvs = kValueThreads / 16;      // 16 virtual envs per workgroup, four per wave

// The virtual envs past V in the last wave neither read nor write: their lanes compute on zeros (the loops of pol_layer are wave-uniform, and a group's shuffles
// stay inside the group).
__global__ __launch_bounds__(kValueThreads) void sawyer_value_kernel(const SawyerValueArgs a) {
#pragma clang fp contract(off)
  const int sub = (int)threadIdx.x & 15;
  const long long v_ = (long long)blockIdx.x * kValueEnvs + ((int)threadIdx.x >> 4);
  const bool live = v_ < a.V;
  const size_t v = live ? (size_t)v_ : 0;
  const int n_layers = a.net.n_layers, d0 = a.net.dims[0], d1 = a.net.dims[1], d2 = a.net.dims[2];
  const double x = (sub < 14 && live) ? a.rows[v * 14 + sub] : 0.0;
  // does the row hold a NaN?  One ballot per wave; a group reads its own 16 bits
  const unsigned long long nan_lanes = __ballot(x != x);
  const bool nan_row = ((nan_lanes >> (((int)threadIdx.x & 63) & ~15)) & 0xFFFFull) != 0;
  float h[kPolicyMaxWidth / 16];
  h[0] = svalue_row(x);
#pragma unroll
  for (int i = 1; i < kPolicyMaxWidth / 16; ++i) h[i] = 0.f;
  const float* w = a.net.params;
  pol_layer<16, false>(w, w + (size_t)d1 * d0, d0, d1, a.net.hidden_act, sub, h);
  w += (size_t)d1 * (d0 + 1);
  int KL = d1;
  if (n_layers == 3) {
    pol_layer<16, true>(w, w + (size_t)d2 * d1, d1, d2, a.net.hidden_act, sub, h);
    w += (size_t)d2 * (d1 + 1);
    KL = d2;
  }
  pol_layer<16, true>(w, w + (size_t)KL, KL, 1, EARL_ACT_NONE, sub, h);       // (one output: every lane's clamped row is row 0, lane 0 keeps it)
  if (sub == 0 && live) a.ret[v] = svalue_terminal(a.ret[v], a.d_H, policy_act(h[0], a.net.out_act), nan_row);
}

int64_t round_up(int64_t v, int64_t al) { return (v + al - 1) / al * al; }

// the value kernel behind a branch launch over V virtual envs: rows = the caller's last_obs or the workspace's carried rows
int launch_value(const earl_plan_value* pv, int32_t nv, int64_t V, int32_t H, double* last_obs, void* ws_base, double* ret, earl_stream_t stream) {
  SawyerValueArgs a{};
  a.net = *pv->value;
  a.rows = last_obs ? last_obs : earl_unit_sawyer_branch_rows(nv, V, ws_base);
  a.ret = ret;
  a.d_H = svalue_discount(pv->discount, H);
  a.V = (int32_t)V;
  sawyer_value_kernel<<<dim3((unsigned)((V + kValueEnvs - 1) / kValueEnvs)), kValueThreads, 0, (hipStream_t)stream>>>(a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "sawyer_value_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

}  // namespace

extern "C" {

// the block: the branch launch's workspace (rounded up to 8 bytes), then the [K n] discounts of a discounted launch, then -- H > 0, a planner's block -- the candidates
// at the next 16-byte ADDRESS (8 bytes of slack), as earl_sawyer_plan_ws_bytes lays them out
int earl_sawyer_value_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes) {
  int64_t branch = 0;
  if (!bytes || H < 0) return EARL_ERR_ARG;
  if (int rc = earl_sawyer_branch_ws_bytes(nv, K, n, &branch)) return rc;
  const int64_t V = (int64_t)K * n;
  *bytes = V == 0 ? 0 : round_up(branch, 8) + V * 8 + (H > 0 ? 8 + V * H * 16 : 0);
  return EARL_OK;
}

int earl_sawyer_branch_rollout_value(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                     int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_plan_value* pv,
                                     const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary, double* last_obs, int32_t* fail_count, earl_stream_t stream) {
  if (sawyer_value_plain(pv)) return earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, ws, summary, last_obs, fail_count, stream);
  if (int rc = check_sawyer_value(pv, g_err)) return rc;
  if (pv->value && !(summary && summary->ret)) return fail(EARL_ERR_ARG, "a value network without summary->ret: the terminal term has nothing to be added to");
  if (!cfg || !ws) return fail(EARL_ERR_ARG, "cfg/ws is NULL");
  int64_t branch = 0, need = 0;
  if (K < 0 || cfg->n < 0 || earl_sawyer_branch_ws_bytes(nv, K, cfg->n, &branch) || earl_sawyer_value_ws_bytes(nv, K, 0, cfg->n, &need))
    return fail(EARL_ERR_ARG, "nv = %d: 10 (door) or 15 (peg); K = %d, n = %d: not negative, K n at most 2^31 - 1", nv, K, cfg->n);
  const int64_t V = (int64_t)K * cfg->n;
  if (V > 0 && (!ws->base || (reinterpret_cast<uintptr_t>(ws->base) & 7) != 0 || ws->bytes < need))
    return fail(EARL_ERR_ARG, "ws: base %p (8-byte aligned), %lld bytes of the %lld needed (earl_sawyer_value_ws_bytes)", ws->base, (long long)ws->bytes, (long long)need);
  branch = round_up(branch, 8);
  const earl_sawyer_branch_ws bws{ws->base, branch};
  // everything else the branch launch refuses is the branch launch's to refuse; V == 0 or H == 0: it returns EARL_OK after its checks and nothing is launched
  int rc;
  if (pv->discount == 1.0) {
    rc = earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, stream);
  } else {
    double* const disc = V > 0 ? reinterpret_cast<double*>(static_cast<char*>(ws->base) + branch) : nullptr;
    rc = V > 0 ? earl_unit_sawyer_branch_discounted(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, pv->discount, disc, stream)
               : earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, stream);
  }
  if (rc || V == 0 || H == 0 || !pv->value) return rc;
  return launch_value(pv, nv, V, H, last_obs, ws->base, summary->ret, stream);
}

int earl_sawyer_prior_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes) {
  int64_t value = 0;
  if (!bytes) return EARL_ERR_ARG;
  if (int rc = earl_sawyer_value_ws_bytes(nv, K, H, n, &value)) return rc;
  const int64_t V = (int64_t)K * n;
  *bytes = V == 0 ? 0 : value + sawyer_prior_queue_bytes(V);
  return EARL_OK;
}

// The scoring call of the `_prior` entry points, `prior` checked by the caller (check_sawyer_prior) and prior->branches >= 1; word0 = the calling planner's draw word | the
// iteration.  The branch launch with the last P branches run by the policy (physics.hip: one launch of the prior kernel over all K n virtual envs, or two), then -- a
// network -- the value kernel over all K n rows.  Hidden: sawyer_plan.hip and sawyer_cem.hip call it once per iteration
__attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_scored_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg,
                                                                               const earl_sawyer_state* st, int32_t K, int32_t H, float* act, int64_t act_branch_stride,
                                                                               const uint64_t* clock, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior,
                                                                               uint32_t word0, uint32_t noise_counter, const earl_sawyer_branch_ws* ws,
                                                                               const earl_episode_summary* summary, double* last_obs, int32_t* fail_count, earl_stream_t stream) {
  if (int rc = check_sawyer_value(pv, g_err)) return rc;
  if (pv && pv->value && !(summary && summary->ret)) return fail(EARL_ERR_ARG, "a value network without summary->ret: the terminal term has nothing to be added to");
  if (!cfg || !ws || !prior || prior->branches < 1) return fail(EARL_ERR_ARG, "cfg/ws/prior is NULL");
  if ((act_branch_stride == 0 && (int64_t)H * cfg->n > 0) || (act_branch_stride & 3) != 0 || (reinterpret_cast<uintptr_t>(act) & 15) != 0)      // (no row, no block: the empty call)
    return fail(EARL_ERR_ARG, "act_branch_stride = %lld, act %p: with prior branches the call WRITES their blocks, one 16-byte store per row -- a stride that is a multiple of 4 "
                "and not 0, act 16-byte aligned", (long long)act_branch_stride, (const void*)act);
  int64_t branch = 0, need = 0;
  if (K < 0 || cfg->n < 0 || earl_sawyer_branch_ws_bytes(nv, K, cfg->n, &branch) || earl_sawyer_prior_ws_bytes(nv, K, 0, cfg->n, &need))
    return fail(EARL_ERR_ARG, "nv = %d: 10 (door) or 15 (peg); K = %d, n = %d: not negative, K n at most 2^31 - 1", nv, K, cfg->n);
  const int64_t V = (int64_t)K * cfg->n;
  if (V > 0 && (!ws->base || (reinterpret_cast<uintptr_t>(ws->base) & 7) != 0 || ws->bytes < need))
    return fail(EARL_ERR_ARG, "ws: base %p (8-byte aligned), %lld bytes of the %lld needed (earl_sawyer_prior_ws_bytes)", ws->base, (long long)ws->bytes, (long long)need);
  branch = round_up(branch, 8);
  const earl_sawyer_branch_ws bws{ws->base, branch};
  int rc;
  if (V == 0) {      // (nothing is launched; the branch launch's own refusals still apply)
    rc = earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, stream);
  } else {
    char* const b = static_cast<char*>(ws->base);
    const SawyerPriorLaunch pl{prior, word0, noise_counter, reinterpret_cast<int32_t*>(b + branch + V * 8)};
    rc = earl_unit_sawyer_branch_prior(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, pv ? pv->discount : 1.0,
                                       reinterpret_cast<double*>(b + branch), &pl, stream);
  }
  if (rc || V == 0 || H == 0 || !pv || !pv->value) return rc;
  return launch_value(pv, nv, V, H, last_obs, ws->base, summary->ret, stream);
}

int earl_sawyer_branch_rollout_prior(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                     int32_t K, int32_t H, float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_plan_value* pv,
                                     const earl_sawyer_plan_prior* prior, int32_t j, uint32_t noise_counter, const earl_sawyer_branch_ws* ws,
                                     const earl_episode_summary* summary, double* last_obs, int32_t* fail_count, earl_stream_t stream) {
  if (!cfg) return fail(EARL_ERR_ARG, "cfg is NULL");
  if (K < 0 || H < 0 || cfg->n < 0) return fail(EARL_ERR_ARG, "K = %d, H = %d, n = %d: not negative", K, H, cfg->n);
  const uint64_t cand = act_branch_stride > 0 ? (uint64_t)K * (uint64_t)act_branch_stride * 4u : (uint64_t)H * (uint64_t)cfg->n * 16u;
  const void* const in[4] = {act, nullptr, nullptr, nullptr};
  const uint64_t in_bytes[4] = {cand, 0, 0, 0};
  if (int rc = check_sawyer_prior(prior, K, H, cfg->n, in, in_bytes, g_err)) return rc;
  if (prior->branches == 0)
    return earl_sawyer_branch_rollout_value(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, pv, ws, summary, last_obs, fail_count, stream);
  if (j < 0 || j > 255) return fail(EARL_ERR_ARG, "iteration %d: 0 .. 255", j);
  return earl_unit_sawyer_branch_scored_prior(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, pv, prior, kSawyerPriorDraw | (uint32_t)j, noise_counter, ws, summary,
                                              last_obs, fail_count, stream);
}

}  // extern "C"

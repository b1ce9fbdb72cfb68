// sawyer_value.hip -- earl_sawyer_branch_rollout_value / earl_sawyer_value_ws_bytes (include/earl_physics.h, "discount and a terminal value on the door and the peg"):
// the branch launch with ret = sum_t gamma^t r_t + gamma^H V(o_H).  On the caller's stream, ordered by the stream alone:
//   the branch launch       discount == 1: earl_sawyer_branch_rollout through the public ABI, untouched.  discount != 1: the same launch with the rollout kernel built
//                           under EARL_BRANCH_DISCOUNT (physics_branch_value.hip, physics_branch_value_w8.hip; reached through physics.hip, which owns the checks and the
//                           launch forms), d_t in [K n] words of the workspace behind the branch launch's block.
//   sawyer_value_kernel     with a value network: the 16 lanes of a group own one virtual env's last observation row -- the caller's last_obs, or the workspace's carried
//                           rows, which already are those rows -- round it to float32 (element `sub` on lane `sub`), evaluate V with pol_layer<16, ..> of
//                           policy_lane_group.h exactly as the closed loop's policy phase does (first layer K = 14: the element-wise path; then 16-byte pieces), and lane 0
//                           does ret[v] += d_H * (double)V (sawyer_value.h, shared with the host twin).  One launch of K n evaluations per planner iteration, not per step.
// Also earl_sawyer_branch_rollout_prior / earl_sawyer_prior_ws_bytes, and the ONE scoring call behind all of them and behind both planners' iterations
// (earl_unit_sawyer_branch_scored: sawyer_shoot.h states it and the workspace layout it reads).
// No stepper header here: the unit compiles in seconds and reaches the stepper through three hidden calls into physics.hip.
#include <hip/hip_runtime.h>

#include "sawyer_shoot.h"   // the workspace layout and the declaration of the scoring call below

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

// the value kernel behind a branch launch over V virtual envs: rows = the caller's last_obs or the workspace's carried rows
int launch_value(const earl_plan_value* pv, int32_t nv, int64_t V, int32_t H, double* last_obs, void* ws_base, double* ret, earl_stream_t stream) {
  SawyerValueArgs a{};
  a.net = *pv->value;
  a.rows = last_obs ? last_obs : earl_unit_sawyer_branch_rows(nv, V, ws_base);
  a.ret = ret;
  a.d_H = svalue_discount(pv->discount, H);
  a.V = (int32_t)V;
  sawyer_value_kernel<<<dim3((unsigned)((V + kValueEnvs - 1) / kValueEnvs)), kValueThreads, 0, (hipStream_t)stream>>>(a);
  return launched("sawyer_value_kernel");
}

}  // namespace

extern "C" {

// the Value and the Prior block of sawyer_shoot.h's sawyer_ws_layout
int earl_sawyer_value_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes) { return sawyer_ws_bytes(nv, K, H, n, SawyerWs::Value, bytes); }
int earl_sawyer_prior_ws_bytes(int32_t nv, int32_t K, int32_t H, int32_t n, int64_t* bytes) { return sawyer_ws_bytes(nv, K, H, n, SawyerWs::Prior, bytes); }

// sawyer_shoot.h states the call.  The branch launch -- plain, discounted (physics.hip: the kernels built with EARL_BRANCH_DISCOUNT, d_t in the block's [K n] words) or
// with the last prior->branches branches run by the policy (one launch of the prior kernel over all K n virtual envs, or two) -- then, with a network, the value kernel over
// all K n rows.  Hidden: sawyer_plan.hip and sawyer_cem.hip call it once per iteration
__attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_scored(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg,
                                                                         const earl_sawyer_state* st, int32_t K, int32_t H, float* act, int64_t act_branch_stride,
                                                                         const uint64_t* clock, const earl_plan_value* pv, const earl_sawyer_plan_prior* prior, uint32_t word0,
                                                                         uint32_t noise_counter, const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary,
                                                                         double* last_obs, int32_t* fail_count, earl_stream_t stream) {
  if (!prior && sawyer_value_plain(pv)) return earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, ws, summary, last_obs, fail_count, stream);
  if (int rc = check_sawyer_value(pv, g_err)) return rc;
  if (pv && pv->value && !(summary && summary->ret)) return fail(EARL_ERR_ARG, "a value network without summary->ret: the terminal term has nothing to be added to");
  if (!cfg || !ws || (prior && prior->branches < 1)) return fail(EARL_ERR_ARG, prior ? "cfg/ws/prior is NULL" : "cfg/ws is NULL");
  if (prior && ((act_branch_stride == 0 && (int64_t)H * cfg->n > 0) || (act_branch_stride & 3) != 0 || misaligned16(act)))      // (no row, no block: the empty call)
    return fail(EARL_ERR_ARG, "act_branch_stride = %lld, act %p: with prior branches the call WRITES their blocks, one 16-byte store per row -- a stride that is a multiple of 4 "
                "and not 0, act 16-byte aligned", (long long)act_branch_stride, (const void*)act);
  SawyerWsLayout L;
  if (K < 0 || cfg->n < 0 || sawyer_ws_layout(nv, K, 0, cfg->n, prior ? SawyerWs::Prior : SawyerWs::Value, &L))
    return fail(EARL_ERR_ARG, "nv = %d: 10 (door) or 15 (peg); K = %d, n = %d: not negative, K n at most 2^31 - 1", nv, K, cfg->n);
  const int64_t V = (int64_t)K * cfg->n;
  if (V > 0)
    if (int rc = check_sawyer_ws(ws, L.need, prior ? " (earl_sawyer_prior_ws_bytes)" : " (earl_sawyer_value_ws_bytes)")) return rc;
  const earl_sawyer_branch_ws bws{ws->base, L.branch};
  const double gamma = pv ? pv->discount : 1.0;
  char* const b = static_cast<char*>(ws->base);
  // everything else the branch launch refuses is the branch launch's to refuse; V == 0 or H == 0: it returns EARL_OK after its checks and nothing is launched
  int rc;
  if (V == 0 || (!prior && gamma == 1.0)) {
    rc = earl_sawyer_branch_rollout(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, stream);
  } else if (!prior) {
    rc = earl_unit_sawyer_branch_discounted(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, gamma,
                                            reinterpret_cast<double*>(b + L.branch), stream);
  } else {
    const SawyerPriorLaunch pl{prior, word0, noise_counter, reinterpret_cast<int32_t*>(b + L.queue)};
    rc = earl_unit_sawyer_branch_prior(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, &bws, summary, last_obs, fail_count, gamma,
                                       reinterpret_cast<double*>(b + L.branch), &pl, stream);
  }
  if (rc || V == 0 || H == 0 || !pv || !pv->value) return rc;
  return launch_value(pv, nv, V, H, last_obs, ws->base, summary->ret, stream);
}

int earl_sawyer_branch_rollout_value(const earl_link_model* model, const earl_collision_model* col, int32_t nv, const earl_sawyer_cfg* cfg, const earl_sawyer_state* st,
                                     int32_t K, int32_t H, const float* act, int64_t act_branch_stride, const uint64_t* clock, const earl_plan_value* pv,
                                     const earl_sawyer_branch_ws* ws, const earl_episode_summary* summary, double* last_obs, int32_t* fail_count, earl_stream_t stream) {
  // (no prior: `act` is read only)
  return earl_unit_sawyer_branch_scored(model, col, nv, cfg, st, K, H, const_cast<float*>(act), act_branch_stride, clock, pv, nullptr, 0, 0, ws, summary, last_obs, fail_count,
                                        stream);
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
  return earl_unit_sawyer_branch_scored(model, col, nv, cfg, st, K, H, act, act_branch_stride, clock, pv, prior, kSawyerPriorDraw | (uint32_t)j, noise_counter, ws, summary, last_obs,
                                        fail_count, stream);
}

}  // extern "C"

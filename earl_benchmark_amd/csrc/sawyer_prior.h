// sawyer_prior.h -- the host side of the policy-prior branches of the Sawyer door / peg planners (include/earl_physics.h, "policy-prior branches on the door and the
// peg"): the argument rules of struct earl_sawyer_plan_prior and what physics.hip's branch launch takes for the prior branches (the workspace layout of the `_prior`
// calls is sawyer_shoot.h's sawyer_ws_layout).  Host only.  The kernel is physics_env_sawyer.h's sawyer_prior_action (physics_branch_prior.hip,
// physics_branch_prior_w8.hip); the host twin of its per-row arithmetic is tabletop_host.cpp's earl_sawyer_prior_actions_cpu.  Included by physics.hip and sawyer_shoot.h.
#pragma once
#include <cmath>
#include <cstdint>

#include "policy_check.h"
#include "policy_math.h"
#include "../../include/earl_physics.h"

namespace earl {

// word 0 of a prior branch's noise counter in earl_sawyer_branch_rollout_prior, | the iteration: MPPI's (tabletop_plan.h: kPlanDraw; sawyer_plan.hip asserts the equality)
constexpr uint32_t kSawyerPriorDraw = 0x504C4E00u;

// what the branch launch (physics.hip: sawyer_branch_launch) takes beside its own arguments when the last `prior->branches` branches of the call are the policy's
struct SawyerPriorLaunch {
  const earl_sawyer_plan_prior* prior;   // checked (check_sawyer_prior), branches >= 1
  uint32_t word0;                        // the planner's draw word | the iteration: kPlanDraw | j, kCemDraw | j
  uint32_t noise_counter;
  int32_t* sched;                        // the work queue of a prior launch of its OWN (the two-launch shape), 2 ceil(P n / 4) words (its replicate launch clears them where the time-sliced form runs)
};

inline bool sawyer_prior_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

// The rules of struct earl_sawyer_plan_prior for a call of K branches, H steps and n envs.  `in` / `in_bytes`: up to four arrays the call reads ([K, H, n, 4] candidates,
// mean, std0, ...) that prior->act must not overlap (NULL entries are skipped); obs0 and the parameters are inputs too.  `err`: NULL or contract::kErrLen bytes
inline int check_sawyer_prior(const earl_sawyer_plan_prior* prior, int32_t K, int32_t H, int32_t n, const void* const (&in)[4], const uint64_t (&in_bytes)[4], char* err) {
  using contract::refuse;
  if (!prior) return refuse(err, "prior is NULL");
  if (!prior->policy) return refuse(err, "prior->policy is NULL");
  if (prior->branches < 0 || prior->branches > K - 1)
    return refuse(err, "prior->branches = %d: 0 .. K - 1 = %d (branch 0 stays the plan itself)", prior->branches, K - 1);
  // 14 -> hidden (-> hidden) -> 4 under the closed-loop Sawyer launch's rules, float32 only (no kBf16Params), no head
  if (int rc = contract::check_policy(*prior->policy, 14, 4, nullptr, contract::kParamsAligned16, err)) return rc;
  for (int d = 0; d < 4; ++d)
    if (!std::isfinite(prior->sigma[d]) || !(prior->sigma[d] >= 0)) return refuse(err, "prior->sigma[%d] = %g: finite and >= 0", d, (double)prior->sigma[d]);
  if (prior->branches == 0) return EARL_OK;
  if (!prior->obs0) return refuse(err, "prior->obs0 is NULL: what the policy sees at step 0");
  if (K > EARL_SAWYER_PLAN_MAX_K || H > 65536) return refuse(err, "K = %d, H = %d: the noise words of a prior branch are keyed by (k << 16) | t: K <= %d, H <= 65536", K, H, EARL_SAWYER_PLAN_MAX_K);
  if (prior->act) {
    if ((uintptr_t)prior->act & 15) return refuse(err, "prior->act is not 16-byte aligned: a row is one 16-byte store");
    const uint64_t bytes = (uint64_t)prior->branches * (uint64_t)H * (uint64_t)n * 16u;
    for (int x = 0; x < 4; ++x)
      if (sawyer_prior_overlap(prior->act, bytes, in[x], in_bytes[x])) return refuse(err, "prior->act overlaps an input of the call");
    if (sawyer_prior_overlap(prior->act, bytes, prior->obs0, (uint64_t)n * 14u * 8u) ||
        sawyer_prior_overlap(prior->act, bytes, prior->policy->params, (uint64_t)contract::mlp_param_count(*prior->policy) * 4u))
      return refuse(err, "prior->act overlaps prior->obs0 or the policy's parameters");
  }
  return EARL_OK;
}

}  // namespace earl

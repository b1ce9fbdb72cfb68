// tabletop_policy_gaussian.hip -- earl_tabletop_policy_rollout_gaussian (include/earl_tabletop.h): the closed-loop tabletop rollout with a Gaussian-head MLP whose
// actions are sampled inside the kernel.  The kernel is tabletop_policy.h's policy_rollout_kernel with GAUSS = true (the sampling contract is stated there, once,
// for this unit and the host twin); its ten instantiations live here, the deterministic ten in tabletop_policy.hip.
#include <hip/hip_runtime.h>

#include "tabletop_policy.h"

using namespace earl;
using namespace earl::hostside;

namespace {

template <int NT2>
void launch_gaussian(const GaussianPolicyArgs& a, bool general, dim3 grid, hipStream_t s) {
  if (general) policy_rollout_kernel<NT2, true, true><<<grid, 256, 0, s>>>(a);
  else policy_rollout_kernel<NT2, false, true><<<grid, 256, 0, s>>>(a);
}

}  // namespace

extern "C" int earl_tabletop_policy_rollout_gaussian(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                                     const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                                     const earl_tabletop_out* out, float* act_out, earl_stream_t stream) {
  if (int rc = check_policy_gaussian(cfg, st, policy, head, episodes, T, reset_first, out)) return rc;      // (before any HIP call: testable without a GPU)
  if (cfg->n == 0) return EARL_OK;
  GaussianPolicyArgs a;
  static_cast<PolicyArgs&>(a) = PolicyArgs{KArgs{*cfg, *st, *out, nullptr, nullptr, nullptr, nullptr, T, thresholds()}, *policy, act_out, episodes, reset_first};
  a.head = *head;
  const bool general = is_general(cfg);
  const dim3 grid((unsigned)((cfg->n + kPolicyEnvsPerWg - 1) / kPolicyEnvsPerWg));
  const hipStream_t s = (hipStream_t)stream;
  switch (policy->n_layers == 3 ? (policy->dims[2] + 63) / 64 : 0) {      // as earl_tabletop_policy_rollout: N-tiles per wave of the hidden -> hidden layer
    case 0: launch_gaussian<0>(a, general, grid, s); break;
    case 1: launch_gaussian<1>(a, general, grid, s); break;
    case 2: launch_gaussian<2>(a, general, grid, s); break;
    case 3: launch_gaussian<3>(a, general, grid, s); break;
    default: launch_gaussian<4>(a, general, grid, s); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "policy_rollout_kernel (gaussian): %s", hipGetErrorString(e));
  return EARL_OK;
}

#ifdef EARL_POLICY_STAMPS
/* diagnostic build only: the six per-phase cycle sums of the last Gaussian launch (wave 0 of workgroup 0; [5] = the head); blocks until the copy is done */
extern "C" int earl_debug_read_policy_gaussian_profile(uint64_t* out) {
  if (!out) return fail(EARL_ERR_ARG, "bad profile buffer");
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(earl::g_policy_prof), 6 * 8) != hipSuccess) return fail(EARL_ERR_LAUNCH, "hipMemcpyFromSymbol failed");
  return EARL_OK;
}
#endif

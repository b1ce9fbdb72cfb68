// tabletop_policy.hip -- earl_tabletop_policy_rollout (include/earl_tabletop.h): the closed-loop tabletop rollout with a float32 MLP policy evaluated inside
// the kernel on v_mfma_f32_16x16x4_f32.  The kernel, its lane maps and the arithmetic contract are in tabletop_policy.h (shared with the host twin).
#include <hip/hip_runtime.h>

#include "tabletop_policy.h"

using namespace earl;
using namespace earl::hostside;

namespace {

template <int NT2>
void launch_policy(const PolicyArgs& a, bool general, dim3 grid, hipStream_t s) {
  if (general) policy_rollout_kernel<NT2, true><<<grid, 256, 0, s>>>(a);
  else policy_rollout_kernel<NT2, false><<<grid, 256, 0, s>>>(a);
}

}  // namespace

extern "C" int earl_tabletop_policy_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, int32_t episodes,
                                            int32_t T, int32_t reset_first, const earl_tabletop_out* out, float* act_out, earl_stream_t stream) {
  if (int rc = check_policy(cfg, st, policy, nullptr, episodes, T, reset_first, out)) return rc;      // (before any HIP call: testable without a GPU)
  if (cfg->n == 0) return EARL_OK;
  const PolicyArgs a{KArgs{*cfg, *st, *out, nullptr, nullptr, nullptr, nullptr, T, thresholds()}, *policy, act_out, episodes, reset_first};
  const bool general = is_general(cfg);
  const dim3 grid((unsigned)((cfg->n + kPolicyEnvsPerWg - 1) / kPolicyEnvsPerWg));
  const hipStream_t s = (hipStream_t)stream;
  // one instantiation per number of N-tiles a wave owns in the hidden -> hidden layer (its weights are that many x 64 registers per lane)
  switch (policy->n_layers == 3 ? (policy->dims[2] + 63) / 64 : 0) {
    case 0: launch_policy<0>(a, general, grid, s); break;
    case 1: launch_policy<1>(a, general, grid, s); break;
    case 2: launch_policy<2>(a, general, grid, s); break;
    case 3: launch_policy<3>(a, general, grid, s); break;
    default: launch_policy<4>(a, general, grid, s); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "policy_rollout_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

#ifdef EARL_POLICY_STAMPS
/* diagnostic build only: the five per-phase cycle sums of the last launch (wave 0 of workgroup 0); blocks until the copy is done */
extern "C" int earl_debug_read_policy_profile(uint64_t* out) {
  if (!out) return fail(EARL_ERR_ARG, "bad profile buffer");
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(earl::g_policy_prof), 5 * 8) != hipSuccess) return fail(EARL_ERR_LAUNCH, "hipMemcpyFromSymbol failed");
  return EARL_OK;
}
#endif

// tabletop_policy_pair.hip -- earl_tabletop_pair_rollout (include/earl_tabletop.h): the closed-loop tabletop rollout with the forward / reset agent pair of
// autonomous RL alternating inside ONE launch.  The kernel and the host front are tabletop_pair_kernel.h's at NOBJ = 1 (its header has the description and the
// register / LDS table); this unit instantiates the six kernels pair_kernel<1, NT2, GAUSS> and, in the diagnostic build, reads their cycle stamps.
#include "tabletop_pair_kernel.h"

using namespace earl;
using namespace earl::hostside;

extern "C" int earl_tabletop_pair_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                          const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out,
                                          float* act_out, earl_stream_t stream) {
  return launch_pair_rollout<1>(cfg, st, policy, pair, head, episodes, T, reset_first, out, act_out, stream, "pair_kernel<1>");
}

#ifdef EARL_POLICY_STAMPS
/* diagnostic build only: the six per-phase cycle sums of the last pair launch (wave 0 of workgroup 0); blocks until the copy is done */
extern "C" int earl_debug_read_policy_pair_profile(uint64_t* out) {
  if (!out) return fail(EARL_ERR_ARG, "bad profile buffer");
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(earl::g_policy_prof), 6 * 8) != hipSuccess) return fail(EARL_ERR_LAUNCH, "hipMemcpyFromSymbol failed");
  return EARL_OK;
}
#endif

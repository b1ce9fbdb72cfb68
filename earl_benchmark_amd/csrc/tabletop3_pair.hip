// tabletop3_pair.hip -- earl_tabletop3_pair_rollout (include/earl_tabletop.h): the closed-loop rollout of the THREE-object tabletop with the forward / reset agent
// pair alternating inside ONE launch.  The kernel and the host front are tabletop_pair_kernel.h's at NOBJ = 3 (its header has the description and the register / LDS
// table); this unit instantiates the six kernels pair_kernel<3, NT2, GAUSS>.
#include "tabletop_pair_kernel.h"

using namespace earl;
using namespace earl::hostside;

extern "C" int earl_tabletop3_pair_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy, const earl_agent_pair* pair,
                                           const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out,
                                           float* act_out, earl_stream_t stream) {
  return launch_pair_rollout<3>(cfg, st, policy, pair, head, episodes, T, reset_first, out, act_out, stream, "pair_kernel<3>");
}

// tabletop_mpc_value.hip -- earl_tabletop_mpc_rollout_value / earl_tabletop3_mpc_rollout_value (include/earl_tabletop.h, "discounted MPPI with a terminal value"):
// the receding-horizon loop of tabletop_mpc.hip with every planning step scored by  ret = sum_t gamma^t r_t + gamma^H V(o_H),  the value network evaluated inside
// the one launch.
//
// The SAME kernel text as tabletop_mpc.hip's mpc_kernel (tabletop_mpc_kernel.inc), compiled with EARL_PLAN_VALUE: the argument block is MpcValueArgs and SCORE runs
// mpc_score<.., true> (tabletop_mpc.h; the discounted sum and the network are tabletop_value.h's, shared with the host twin).  A translation unit of its own, the
// project's idiom for a second build: tabletop_mpc.hip compiles to what it compiled to before, and the namespace `value` tells these kernels from the value-free ones
// of the same name in a kernel trace.  Four kernels under __launch_bounds__(1024): no scratch, at most 128 VGPRs, the LDS of the value-free kernels.
#include <hip/hip_runtime.h>

#include "tabletop_mpc.h"

using namespace earl;
using namespace earl::hostside;

#define EARL_PLAN_VALUE 1
namespace {
namespace value {
#include "tabletop_mpc_kernel.inc"
}  // namespace value
}  // namespace

extern "C" {

int earl_tabletop_mpc_rollout_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                    const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream) {
  return value::do_mpc<1>(cfg, st, params, pv, T, out, mpc, stream);
}

int earl_tabletop3_mpc_rollout_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv, int32_t T,
                                     const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream) {
  return value::do_mpc<3>(cfg, st, params, pv, T, out, mpc, stream);
}

}  // extern "C"

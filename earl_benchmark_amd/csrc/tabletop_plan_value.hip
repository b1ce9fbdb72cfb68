// tabletop_plan_value.hip -- earl_tabletop_plan_mppi_value / earl_tabletop3_plan_mppi_value (include/earl_tabletop.h, "discounted MPPI with a terminal value"): the
// planner of tabletop_plan.hip with the score  ret = sum_t gamma^t r_t + gamma^H V(o_H),  the value network evaluated inside the score kernel.
//
// The SAME kernel text as tabletop_plan.hip's plan_score_kernel (tabletop_plan_kernel.inc), compiled with EARL_PLAN_VALUE: the argument block is PlanValueArgs and the
// per-lane body is plan_score_body<.., true> (tabletop_plan.h; the discounted sum and the network are tabletop_value.h's, shared with the host twin).  A translation
// unit of its own, the project's idiom for a second build: tabletop_plan.hip compiles to what it compiled to before, and the namespace `value` tells these kernels
// from the value-free ones of the same name in a kernel trace.  The update launch is tabletop_plan.hip's (it sees returns only).
#include <hip/hip_runtime.h>

#include "tabletop_hostside.h"
#include "tabletop_plan.h"

using namespace earl;
using namespace earl::hostside;

#define EARL_PLAN_VALUE 1
namespace {
namespace value {
#include "tabletop_plan_kernel.inc"
}  // namespace value
}  // namespace

extern "C" {

int earl_tabletop_plan_mppi_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                  const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  return value::do_plan<1>(cfg, st, params, pv, mean, plan, ret, ret0, best_ret, best_k, stream);
}

int earl_tabletop3_plan_mppi_value(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, const earl_plan_value* pv,
                                   const float* mean, float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (!st) return fail(EARL_ERR_ARG, "cfg/state is NULL");
  return value::do_plan<3>(cfg, st, params, pv, mean, plan, ret, ret0, best_ret, best_k, stream);
}

}  // extern "C"

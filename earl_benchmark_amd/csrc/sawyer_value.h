// sawyer_value.h -- the terminal value of the Sawyer door / peg planners (include/earl_physics.h, "discount and a terminal value on the door and the peg"): what the
// value kernel of sawyer_value.hip and its host twin earl_sawyer_value_terminal_cpu (tabletop_host.cpp, under -DEARL_HOST_BUILD) compute per virtual env, and the
// argument rules the `_value` entry points share.  The discounted SUM is the rollout kernel's (physics_env_sawyer.h: sawyer_branch_summary<true>); there is no host
// stepper, so it has no twin.
//
// svalue_discount   d_H by the recurrence d_0 = 1, d_{t+1} = d_t * gamma: H float64 roundings, on the host in both builds (d_H depends on gamma and H alone, so the
//                   launch carries it as a kernel argument; the rollout kernel's d_t in the workspace walks through the same products).
// svalue_row        one double of the observation row rounded to float32, as the closed-loop policy reads its rows.
// svalue_terminal   ret + d_H * (double)V: two float64 roundings, contraction off.  A row that holds a NaN gives a NaN whatever the network says: relu_f32 maps a NaN
//                   pre-activation to 0 and would hide it, and a branch without an observation must never win.
// The network itself is the policy contract's (policy_math.h): on the device by the 16 lanes of the virtual env through pol_layer<16, ..> (policy_lane_group.h), on
// the host by earl_mlp_policy_forward_cpu's loops -- the same chains, acc = b_j; k ascending: acc = fmaf(x_k, W_jk, acc).
#pragma once
#include "policy_check.h"
#include "policy_math.h"

namespace earl {

// what the value kernel carries.  rows: [V, 14] float64 (the caller's last_obs or the workspace's carried rows); ret: [V]
struct SawyerValueArgs {
  earl_mlp_policy net;
  const double* rows;
  double* ret;
  double d_H;
  int32_t V;
};

inline double svalue_discount(double gamma, int32_t H) {
  double d = 1.0;
  for (int32_t t = 0; t < H && d != 0.0; ++t) d = d * gamma;      // (0 stays 0: a horizon of millions ends here)
  return d;
}

__host__ __device__ __forceinline__ float svalue_row(double x) { return (float)x; }

__host__ __device__ __forceinline__ double svalue_terminal(double ret, double d_H, float V, bool nan_row) {
#pragma clang fp contract(off)
  const double v = nan_row ? (double)__builtin_nanf("") : (double)V;
  const double term = d_H * v;
  return ret + term;
}

// The rules of earl_plan_value on these envs (earl_tabletop_plan_mppi_value's domain of the discount; the network 14 -> hidden (-> hidden) -> 1 under the closed
// loop's rules: float32 only, no head, hidden widths multiples of 16 up to kPolicyMaxWidth, params 16-byte aligned because the rows are read in 16-byte pieces).
// pv NULL is the value-free call and passes.  `err`: NULL or contract::kErrLen bytes for the message; rules: the device's alignment rule (the host twin asks none)
inline int check_sawyer_value(const earl_plan_value* pv, char* err, unsigned rules = contract::kParamsAligned16) {
  if (!pv) return EARL_OK;
  if (!(pv->discount > 0.0 && pv->discount <= 1.0)) return contract::refuse(err, "discount = %g: 0 < discount <= 1", pv->discount);   // (NaN fails both comparisons)
  if (!pv->value) return EARL_OK;
  return contract::check_policy(*pv->value, 14, 1, nullptr, rules, err);
}
// does the call reduce to the value-free one?
inline bool sawyer_value_plain(const earl_plan_value* pv) { return !pv || (pv->discount == 1.0 && !pv->value); }

}  // namespace earl

// tabletop_mpc.hip -- earl_tabletop_mpc_rollout / earl_tabletop3_mpc_rollout (include/earl_tabletop.h, "receding-horizon MPPI control"): T real steps of
// plan -> act -> shift in ONE launch, equal bit for bit to the composition of earl_tabletop[3]_plan_mppi and the one-step rollout.  No cooperative launch, no flag
// between workgroups; the per-lane functions are tabletop_step.h's and tabletop_plan.h's (through tabletop_mpc.h), shared with the host twin.
//
// mpc_kernel  (tabletop_mpc_kernel.inc: one text with tabletop_mpc_value.hip)
//             a workgroup owns ONE env for the whole launch; its lanes are the K branches, 64 * ceil(K / 64) of them, lane k >= K idle in the score pass.
//   state     the real env (registers of ONE lane elsewhere: Lane<NOBJ> and its goal row) sits in LDS, loaded once and stored once by lane 0.  SCORE copies it into
//             every lane's registers; ACT lets every lane step such a copy with the same action (so `done` needs no broadcast) and lane 0 puts its copy back
//             and stores the output row.  Kept out of the registers between the two so that 1024 lanes (128 VGPRs each) hold the three-object env without scratch.
//   plan      [H][3] float32 in LDS, a ring: row t of the plan is slot (base + t) mod H, so the shift is `base += 1` and one row copy.
//   SCORE     lane k runs mpc_score on a copy of the registers: per look-ahead step one broadcast LDS read of the clipped row, one Philox block, three quantiles,
//             one wrapped step.  The K returns never leave the registers: beta / best_k by an xor butterfly of plan_best_merge (order-free) and across waves
//             through 16 LDS slots; lane k then makes its own W_k (one exp_f32) into w_lds[k] and adds it to S (64-bit LDS atomic: integer, order-free).
//   UPDATE    the REGENERATING form: item (t, g) -- step t, branch group g of G = max(1, lanes / H) -- makes the candidates (k, t) of its k = 1 + g, 1 + g + G, ..
//             again from the same counters, sums W_k * D_k in registers (int64) and adds the three sums to A_lds[t] (64-bit LDS atomics).  After a barrier the
//             lane that owns row t writes plan_new_mean and clears the sums.  Chosen over caching D_k in LDS during SCORE (12 B per (k, t): 24 KB at K = 64,
//             H = 32 -- six one-wave workgroups per CU where this form runs sixteen -- and beyond LDS altogether at EARL_MPC_MAX_K x EARL_MPC_MAX_H, so this form
//             has to exist either way).  Both forms give the same bits (items 4-5 of the planner's contract are integer sums).
//   LDS       dynamic, 36 * H + 4 * K + 200 bytes + the env (Lane<NOBJ> and its goal row): A [H][3] int64, 16 (float64, int32) partial maxima, S, the plan, K weights.
//             1.7 KB at K = 64, H = 32.
#include <hip/hip_runtime.h>

#include "tabletop_mpc.h"

using namespace earl;
using namespace earl::hostside;

namespace {

#include "tabletop_mpc_kernel.inc"   // mpc_kernel and do_mpc: one text with tabletop_mpc_value.hip

}  // namespace

extern "C" {

int earl_tabletop_mpc_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                              const earl_mpc_out* mpc, earl_stream_t stream) {
  return do_mpc<1>(cfg, st, params, nullptr, T, out, mpc, stream);
}

int earl_tabletop3_mpc_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                               const earl_mpc_out* mpc, earl_stream_t stream) {
  return do_mpc<3>(cfg, st, params, nullptr, T, out, mpc, stream);
}

}  // extern "C"

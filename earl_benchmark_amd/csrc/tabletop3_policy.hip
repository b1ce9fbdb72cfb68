// tabletop3_policy.hip -- earl_tabletop3_policy_rollout (include/earl_tabletop.h): the closed-loop rollout of the THREE-object tabletop, a float32 MLP policy
// 20 -> hidden (-> hidden) -> 3 (6 with a Gaussian head) evaluated between the env steps of one launch, for one policy or a population, with per-episode summaries.
// The kernel is tabletop_policy.h's body (tabletop_policy_kernel.inc) with NOBJ = 3: Lane<3> in the registers of the env lanes, the observation image [16][20]
// in LDS, five chained v_mfma_f32_16x16x4_f32 per N-tile of layer 0 (K = 20 is a multiple of 4: no padding); everything behind layer 0 is the single-object kernel's.
// One family of twenty instantiations (NT2 0..4 x GENERAL x GAUSS): the population form is always compiled in, pop.envs_per_policy == 0 means one policy.
#include <hip/hip_runtime.h>

#include "tabletop_policy.h"

using namespace earl;
using namespace earl::hostside;

namespace earl {

template <int NT2, bool GENERAL, bool GAUSS>
__global__ __launch_bounds__(256) void tabletop3_policy_kernel(const PopulationArgs a) {
  constexpr bool POP = true;
  constexpr int NOBJ = 3;
#include "tabletop_policy_kernel.inc"
}

}  // namespace earl

namespace {

template <int NT2, bool GAUSS>
void launch3(const PopulationArgs& a, bool general, dim3 grid, hipStream_t s) {
  if (general) tabletop3_policy_kernel<NT2, true, GAUSS><<<grid, 256, 0, s>>>(a);
  else tabletop3_policy_kernel<NT2, false, GAUSS><<<grid, 256, 0, s>>>(a);
}

template <bool GAUSS>
void launch3(const PopulationArgs& a, bool general, dim3 grid, hipStream_t s) {
  switch (a.p.n_layers == 3 ? (a.p.dims[2] + 63) / 64 : 0) {      // as earl_tabletop_policy_rollout: N-tiles per wave of the hidden -> hidden layer
    case 0: launch3<0, GAUSS>(a, general, grid, s); break;
    case 1: launch3<1, GAUSS>(a, general, grid, s); break;
    case 2: launch3<2, GAUSS>(a, general, grid, s); break;
    case 3: launch3<3, GAUSS>(a, general, grid, s); break;
    default: launch3<4, GAUSS>(a, general, grid, s); break;
  }
}

}  // namespace

extern "C" int earl_tabletop3_policy_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                             const earl_policy_population* pop, const earl_gaussian_head* head, int32_t episodes, int32_t T, int32_t reset_first,
                                             const earl_tabletop_out* out, float* act_out, const earl_episode_summary* summary, earl_stream_t stream) {
  if (int rc = check_population(cfg, st, policy, pop, head, episodes, T, reset_first, out, 3)) return rc;      // (before any HIP call: testable without a GPU)
  if (cfg->n == 0) return EARL_OK;
  const PopulationArgs a = population_args(cfg, st, policy, pop, head, episodes, T, reset_first, out, act_out, summary, thresholds());
  const bool general = cfg->auto_reset != 0;                         // (the three-object env has no lifelong switch: check_common)
  // workgroups aligned to global env ids, with or without a population: the first one starts (env_offset mod 16) ids before the shard
  const int64_t lead = cfg->env_offset & (kPolicyEnvsPerWg - 1);
  const dim3 grid((unsigned)((lead + cfg->n + kPolicyEnvsPerWg - 1) / kPolicyEnvsPerWg));
  const hipStream_t s = (hipStream_t)stream;
  if (head) launch3<true>(a, general, grid, s);
  else launch3<false>(a, general, grid, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "tabletop3_policy_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

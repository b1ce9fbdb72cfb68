// tabletop_policy_population.hip -- earl_tabletop_population_rollout (include/earl_tabletop.h): the closed-loop tabletop rollout for a POPULATION of policies
// (every 16-env workgroup loads the parameters of its own member) with per-episode summaries kept on the env lanes.  The kernel is tabletop_policy.h's
// policy_rollout_body with POP = true (workgroups aligned to global env ids; the addressing is stated there); its twenty instantiations live here, the
// single-policy twenty stay in tabletop_policy.hip and tabletop_policy_gaussian.hip, untouched.
#include <hip/hip_runtime.h>

#include "tabletop_policy.h"

using namespace earl;
using namespace earl::hostside;

namespace {

template <int NT2, bool GAUSS>
void launch_population(const PopulationArgs& a, bool general, dim3 grid, hipStream_t s) {
  if (general) policy_population_kernel<NT2, true, GAUSS><<<grid, 256, 0, s>>>(a);
  else policy_population_kernel<NT2, false, GAUSS><<<grid, 256, 0, s>>>(a);
}

template <bool GAUSS>
void launch_population(const PopulationArgs& a, bool general, dim3 grid, hipStream_t s) {
  switch (a.p.n_layers == 3 ? (a.p.dims[2] + 63) / 64 : 0) {      // as earl_tabletop_policy_rollout: N-tiles per wave of the hidden -> hidden layer
    case 0: launch_population<0, GAUSS>(a, general, grid, s); break;
    case 1: launch_population<1, GAUSS>(a, general, grid, s); break;
    case 2: launch_population<2, GAUSS>(a, general, grid, s); break;
    case 3: launch_population<3, GAUSS>(a, general, grid, s); break;
    default: launch_population<4, GAUSS>(a, general, grid, s); break;
  }
}

}  // namespace

extern "C" int earl_tabletop_population_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* policy,
                                                const earl_policy_population* pop, const earl_gaussian_head* head, int32_t episodes, int32_t T,
                                                int32_t reset_first, const earl_tabletop_out* out, float* act_out, const earl_episode_summary* summary,
                                                earl_stream_t stream) {
  if (int rc = check_population(cfg, st, policy, pop, head, episodes, T, reset_first, out)) return rc;      // (before any HIP call: testable without a GPU)
  if (cfg->n == 0) return EARL_OK;
  const PopulationArgs a = population_args(cfg, st, policy, pop, head, episodes, T, reset_first, out, act_out, summary, thresholds());
  const bool general = is_general(cfg);
  // workgroups aligned to global env ids: the first one starts (env_offset mod 16) ids before the shard
  const int64_t lead = cfg->env_offset & (kPolicyEnvsPerWg - 1);
  const dim3 grid((unsigned)((lead + cfg->n + kPolicyEnvsPerWg - 1) / kPolicyEnvsPerWg));
  const hipStream_t s = (hipStream_t)stream;
  if (head) launch_population<true>(a, general, grid, s);
  else launch_population<false>(a, general, grid, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "policy_population_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

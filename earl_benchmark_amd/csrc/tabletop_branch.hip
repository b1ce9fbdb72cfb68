// tabletop_branch.hip -- earl_tabletop_branch_rollout / earl_tabletop3_branch_rollout (include/earl_tabletop.h): K candidate action sequences of H steps scored
// per env FROM THE CURRENT STATE in one launch, the state left as it was -- what a shooting planner (random shooting, CEM, MPPI) asks of a simulator.
//
// One lane per (branch, env): branch_body (tabletop_plan.h) is rollout_body's loop with the per-step stores replaced by three reducers in registers.  A wave is
// 64 consecutive envs of ONE branch, so the three dword action loads of a step cover 768 contiguous bytes; a workgroup is that one wave (no LDS, no barrier, no
// atomics: nothing ties waves together, and a batch of 70 envs costs two waves per branch, not four).  The grid is 1-D, K * ceil(n / 64) workgroups, the branch
// taken from blockIdx.x: K is the large dimension of a planner and grid.y ends at 65,535.  Per env-step a lane reads 12 B and stores nothing.
#include <hip/hip_runtime.h>

#include "tabletop_hostside.h"
#include "tabletop_plan.h"

using namespace earl;
using namespace earl::hostside;

namespace {

template <int NOBJ, bool GENERAL>
__global__ __launch_bounds__(kBranchBlock) void branch_kernel(const BranchArgs b, const unsigned tiles) {
  const unsigned k = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - k * tiles) * kBranchBlock + threadIdx.x;   // (unsigned: the last tile of n close to 2^31 runs past INT32_MAX)
  if (i < (unsigned)b.a.cfg.n) branch_body<NOBJ, GENERAL>(b, (int)i, (int)k);
}

template <int NOBJ>
int do_branch(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t stride,
              const earl_episode_summary* summary, float* last_obs, earl_stream_t stream) {
  long long blocks;
  if (int rc = check_branch(cfg, st, NOBJ, K, H, act, stride, summary, last_obs, &blocks)) return rc;
  if (blocks == 0) return EARL_OK;
  const BranchArgs b{KArgs{*cfg, *st, earl_tabletop_out{nullptr, nullptr, nullptr, nullptr, nullptr}, act, nullptr, nullptr, nullptr, H, thresholds()},
                     (long long)stride, summary ? *summary : earl_episode_summary{nullptr, nullptr, nullptr}, last_obs};
  const unsigned tiles = (unsigned)(blocks / K);
  const dim3 grid((unsigned)blocks);
  if (is_general(cfg)) branch_kernel<NOBJ, true><<<grid, kBranchBlock, 0, (hipStream_t)stream>>>(b, tiles);
  else branch_kernel<NOBJ, false><<<grid, kBranchBlock, 0, (hipStream_t)stream>>>(b, tiles);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "branch_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

}  // namespace

extern "C" {

int earl_tabletop_branch_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                 const earl_episode_summary* summary, float* last_obs, earl_stream_t stream) {
  return do_branch<1>(cfg, st, K, H, act, act_branch_stride, summary, last_obs, stream);
}

int earl_tabletop3_branch_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t K, int32_t H, const float* act, int64_t act_branch_stride,
                                  const earl_episode_summary* summary, float* last_obs, earl_stream_t stream) {
  return do_branch<3>(cfg, st, K, H, act, act_branch_stride, summary, last_obs, stream);
}

}  // extern "C"

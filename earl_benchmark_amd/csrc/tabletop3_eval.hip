// tabletop3_eval.hip -- earl_tabletop3_eval_episodes (include/earl_tabletop.h): `episodes` evaluation episodes of the THREE-object tabletop, each
// earl_tabletop3_reset + earl_tabletop3_rollout, in ONE role-split launch (tabletop3_rollout_ws.h) when that kernel applies, otherwise as that sequence of the
// existing entry points -- which this unit reaches through the public ABI, so that tabletop.hip and its kernels stay as they are.
#include <hip/hip_runtime.h>

#include "tabletop3_rollout_ws.h"
#include "tabletop_hostside.h"

using namespace earl;
using namespace earl::hostside;

namespace {

int g_rollout3_form = 0;  // 0 = automatic, 1 = always the sequence of existing kernels, 2 = fused with all episodes on one group of workgroups

// compute units of the current device (MI355X: 256), asked once per device (tabletop.hip: cu_count)
int cu_count3() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int v = 0;
    cus[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return cus[dev];
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int earl_tabletop3_eval_episodes(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, int32_t episodes, int32_t T, const float* act,
                                 int64_t act_episode_stride, const earl_tabletop_out* out, earl_stream_t stream) {
  if (episodes < 0) return fail(EARL_ERR_ARG, "episodes = %d < 0", episodes);
  if (act_episode_stride < 0) return fail(EARL_ERR_ARG, "negative action stride");
  if (int rc = check_common(cfg, st, 3)) return rc;
  if (!act || !out) return fail(EARL_ERR_ARG, "act/out is NULL");
  if (T < 0) return fail(EARL_ERR_ARG, "T = %d < 0", T);
  if (episodes == 0 || cfg->n == 0) return EARL_OK;
  // the fused launch: no auto-reset, all four outputs (at the alignment its 16-byte row stores and dword flag stores take: any allocation's), whole chunks, at
  // least two per episode (one per slot of the row-image ring), and a launch-wide step count the kernel's int chunk counters hold
  const bool fused = g_rollout3_form != 1 && !cfg->auto_reset && out->obs && out->reward && out->done && out->success && T % kWs3K == 0 && T >= 2 * kWs3K &&
                     (long long)episodes * T < (1 << 24) && aligned_to(out->obs, 16) && aligned_to(out->reward, 4) && aligned_to(out->done, 4) &&
                     aligned_to(out->success, 4);
  if (!fused) {                                   // the sequence itself, through the existing kernels
    for (int32_t e = 0; e < episodes; ++e) {
      earl_tabletop_cfg c = *cfg;
      c.counter += (uint64_t)e * (uint64_t)(T + 1);
      if (int rc = earl_tabletop3_reset(&c, st, nullptr, nullptr, stream)) return rc;
      c.counter += 1;
      const size_t rows = (size_t)e * (size_t)T * (size_t)cfg->n;
      const earl_tabletop_out o{out->obs ? out->obs + rows * 20 : nullptr, out->reward ? out->reward + rows : nullptr, out->done ? out->done + rows : nullptr,
                                out->success ? out->success + rows : nullptr, nullptr};
      if (int rc = earl_tabletop3_rollout(&c, st, T, act + (size_t)e * (size_t)act_episode_stride, &o, stream)) return rc;
    }
    return EARL_OK;
  }
  Ws3Args w{cfg->n, T, episodes, cfg->horizon, act, (long long)act_episode_stride, st->qpos, st->attached, st->goal_idx, st->goal_table,
            st->steps_since_reset, st->num_interventions, out->obs, out->reward, out->done, out->success, thresholds(), *cfg, 0, 1, episodes};
  dim3 grid((unsigned)((cfg->n + 63) / 64));
  w.wgs = (int)grid.x;
  // episodes are independent of one another (each starts with the reset): a batch that fills at most half the CUs runs groups of them side by side, each on
  // its own workgroups (the single-object launch's rule, tabletop.hip: do_rollout)
  const unsigned cus = (unsigned)cu_count3();
  if (episodes > 1 && g_rollout3_form != 2 && grid.x * 2 <= cus) {
    const int slots = (int)(cus / grid.x);
    const int P = slots < episodes ? slots : episodes;
    w.ep_per_group = (episodes + P - 1) / P;
    w.ep_groups = (episodes + w.ep_per_group - 1) / w.ep_per_group;
    grid.x *= (unsigned)w.ep_groups;
  }
  if (cfg->reward_type == EARL_REWARD_SPARSE) rollout3_ws_kernel<EARL_REWARD_SPARSE><<<grid, kWs3Threads, 0, (hipStream_t)stream>>>(w);
  else rollout3_ws_kernel<EARL_REWARD_DENSE><<<grid, kWs3Threads, 0, (hipStream_t)stream>>>(w);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "rollout3_ws_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

/* test / bench hook: the launch form of earl_tabletop3_eval_episodes (0 automatic, 1 the sequence of existing kernels, 2 fused without episodes in flight);
 * returns the previous value */
int earl_debug_set_rollout3_form(int form) {
  const int prev = g_rollout3_form;
  if (form >= 0 && form <= 2) g_rollout3_form = form;
  return prev;
}

}  // extern "C"

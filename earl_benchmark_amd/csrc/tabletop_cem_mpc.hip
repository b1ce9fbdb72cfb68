// tabletop_cem_mpc.hip -- earl_tabletop_mpc_rollout_cem / earl_tabletop3_mpc_rollout_cem (include/earl_tabletop.h, "CEM planning"): T real steps of
// plan -> act -> shift in ONE launch, equal bit for bit to the composition of earl_tabletop[3]_plan_cem (std0 = NULL) and the one-step rollout.  No cooperative
// launch, no flag between workgroups; the per-lane functions are tabletop_step.h's, tabletop_plan.h's and tabletop_cem.h's, shared with the host twin.
//
// cem_mpc_kernel  mpc_kernel's frame (tabletop_mpc.hip): a workgroup owns ONE env for the whole launch, its lanes are the K branches; the real env, its goal row and
//                 the plan ring [H][3] sit in LDS; ACT and SHIFT are that kernel's.
//   std       std_lds[H][3] beside the plan, slot for slot; set to sclamp(sigma) at the top of every real step (the search starts from sigma each time).
//   SCORE     lane k runs cem_mpc_score on a copy of the env and puts its return into ret_lds[k] (float64); beta / best_k by the xor butterfly of plan_best_merge.
//   RANK      lane k counts the branches before it against ret_lds -- every lane reads the same address at a time, a broadcast -- and an elite writes
//             e_lds[rank] = k: the elites' ranks are 0 .. Ne - 1, since every return that is not NaN stands before every NaN.
//   UPDATE    item (t, g) -- step t, elite group g of G = max(1, lanes / H) -- makes the candidates (k, t) of the elites e_lds[g], e_lds[g + G], .. again from
//             their counters, sums D and D^2 in registers (int64) and adds the six sums to A1_lds[t], A2_lds[t] (64-bit LDS atomics: integer, order-free).  After
//             a barrier the lane that owns slot e writes cem_new_mean and cem_new_std and clears the sums: the same thread reads, writes and clears each slot.
//   value     none: with the value network inside, the three-object auto-reset kernel needs 12 bytes of scratch per lane at 128 VGPRs under 1024-lane launch bounds,
//             so the entry points refuse pv != NULL (the header says so) and no such kernel is built.
//   LDS       dynamic, 72 * H + 8 * K + 4 * E + 216 bytes + the env: A1, A2 [H][3] int64, 16 (float64, int32) partial maxima, Ne, the plan and std rings, K returns,
//             E elites.  3.0 KB at K = 64, E = 8, H = 32.
#include <hip/hip_runtime.h>

#include "tabletop_cem.h"

using namespace earl;
using namespace earl::hostside;

namespace {

constexpr int kMpcWaves = kMpcMaxK / kBranchBlock;   // 16

template <int NOBJ>
inline size_t cem_mpc_lds_bytes(int H, int K, int E) {
  return (size_t)H * 3 * 8 * 2 + (size_t)K * 8 + kMpcWaves * 8 + 8 + sizeof(Lane<NOBJ>) + Dims<NOBJ>::NG * 4 + (size_t)H * 3 * 4 * 2 + (size_t)E * 4 + kMpcWaves * 4;
}

template <int NOBJ, bool GENERAL>
__global__ __launch_bounds__(kMpcMaxK) void cem_mpc_kernel(const CemMpcArgs c) {
  extern __shared__ unsigned long long lds_raw[];
  const MpcArgs& x = c.x;
  const int H = x.p.a.T, K = x.p.K, n = x.p.a.cfg.n, E = c.E;
  unsigned long long* const A1_lds = lds_raw;                                  // [H][3]
  unsigned long long* const A2_lds = A1_lds + (size_t)H * 3;                   // [H][3]
  double* const ret_lds = reinterpret_cast<double*>(A2_lds + (size_t)H * 3);   // [K]
  double* const b_lds = ret_lds + K;                                           // [kMpcWaves]
  int32_t* const ne_lds = reinterpret_cast<int32_t*>(b_lds + kMpcWaves);       // one word (and four bytes of padding)
  static_assert(sizeof(Lane<NOBJ>) % 8 == 0, "the words after the env stay aligned");
  Lane<NOBJ>& L_lds = *reinterpret_cast<Lane<NOBJ>*>(ne_lds + 2);              // the real env
  float (&g_lds)[Dims<NOBJ>::NG] = *reinterpret_cast<float (*)[Dims<NOBJ>::NG]>(&L_lds + 1);
  float* const plan_lds = &g_lds[0] + Dims<NOBJ>::NG;                          // [H][3], a ring
  float* const std_lds = plan_lds + (size_t)H * 3;                             // [H][3], slot for slot
  int32_t* const e_lds = reinterpret_cast<int32_t*>(std_lds + (size_t)H * 3);  // [E]
  int32_t* const k_lds = e_lds + E;                                            // [kMpcWaves]

  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, wave = tid / kBranchBlock, waves = nthr / kBranchBlock;
  const int i = (int)blockIdx.x;   // (the grid is n workgroups)
  const int k = tid;
  const bool live = k < K;
  const KArgs& a = x.p.a;
  const float s0[3] = {cem_sclamp(x.p.sigma[0], c.std_min, c.std_max), cem_sclamp(x.p.sigma[1], c.std_min, c.std_max), cem_sclamp(x.p.sigma[2], c.std_min, c.std_max)};

  for (int e = tid; e < H * 3; e += nthr) {
    plan_lds[e] = x.m.plan[((size_t)(e / 3) * n + i) * 3 + e % 3];
    A1_lds[e] = 0ull;
    A2_lds[e] = 0ull;
  }
  if (tid == 0) {
    *ne_lds = 0;
    Lane<NOBJ> L;
    load_lane<NOBJ>(a, i, L);
    float g[Dims<NOBJ>::NG];
    load_goal<NOBJ>(a.st.goal_table, L.goal_idx, g);
    copy_lane<NOBJ>(L_lds, L);
#pragma unroll
    for (int j = 0; j < Dims<NOBJ>::NG; ++j) g_lds[j] = g[j];
  }
  PlanArgs q = x.p;
  int base = 0;
  const int G = nthr / H > 1 ? nthr / H : 1, items = H * G;

  for (int s = 0; s < x.T; ++s) {
    const uint64_t counter = a.cfg.counter + (uint64_t)s;
    q.noise_counter = x.p.noise_counter + (uint32_t)s;
    for (int e = tid; e < H * 3; e += nthr) std_lds[e] = s0[e % 3];
    __syncthreads();
    auto row = [&](int t, float (&m)[3], float (&sd)[3]) {
      int r = base + t;
      r = r >= H ? r - H : r;
      m[0] = plan_clip(plan_lds[r * 3]);
      m[1] = plan_clip(plan_lds[r * 3 + 1]);
      m[2] = plan_clip(plan_lds[r * 3 + 2]);
      sd[0] = std_lds[r * 3];   // (already clamped: sclamp(sigma) or a std' of item 5)
      sd[1] = std_lds[r * 3 + 1];
      sd[2] = std_lds[r * 3 + 2];
    };
    for (int it = 0; it < x.iterations; ++it) {
      q.word0 = kCemDraw | (uint32_t)(x.iteration0 + it);
      // SCORE
      double ret = 0.0, beta = -__builtin_inf();
      int bk = 0;
      if (live) {
        ret = cem_mpc_score<NOBJ, GENERAL>(q, i, k, counter, L_lds, g_lds, row);
        ret_lds[k] = ret;
        plan_best(ret, k, beta, bk);
      }
      if (tid == 0 && x.m.ret0) x.m.ret0[((size_t)s * x.iterations + it) * n + i] = ret;
#pragma unroll
      for (int off = kBranchBlock / 2; off > 0; off >>= 1) {
        const double rb = __shfl_xor(beta, off, kBranchBlock);
        const int rk = __shfl_xor(bk, off, kBranchBlock);
        plan_best_merge(rb, rk, beta, bk);
      }
      if (waves > 1 && tid % kBranchBlock == 0) {
        b_lds[wave] = beta;
        k_lds[wave] = bk;
      }
      __syncthreads();
      if (waves > 1) {
        beta = b_lds[0];
        bk = k_lds[0];
        for (int v = 1; v < waves; ++v) plan_best_merge(b_lds[v], k_lds[v], beta, bk);
      }
      // RANK
      if (live) {
        int rank = 0;
        for (int k2 = 0; k2 < K; ++k2) rank += cem_before(ret_lds[k2], k2, ret, k) ? 1 : 0;
        if (cem_elite(ret, rank, E)) {
          e_lds[rank] = k;
          atomicAdd(ne_lds, 1);
        }
      }
      __syncthreads();
      const int32_t Ne = *ne_lds;
      // UPDATE, regenerating the elites
      for (int item = tid; item < items; item += nthr) {
        const int t = item % H, grp = item / H;
        float m[3], sd[3];
        row(t, m, sd);
        int64_t A1[3] = {0, 0, 0}, A2[3] = {0, 0, 0};
        for (int ee = grp; ee < Ne; ee += G) {
          const int kk = e_lds[ee];
          if (kk > 0) cem_accumulate(q, i, (uint32_t)kk, (uint32_t)t, m, sd, A1, A2);   // (branch 0 is the mean: D = 0)
        }
        int r = base + t;
        r = r >= H ? r - H : r;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if (A1[d] != 0) atomicAdd(&A1_lds[r * 3 + d], (unsigned long long)A1[d]);
          if (A2[d] != 0) atomicAdd(&A2_lds[r * 3 + d], (unsigned long long)A2[d]);
        }
      }
      __syncthreads();
      for (int e = tid; e < H * 3; e += nthr) {   // (slot e of the rings: the same words read, written and cleared by one lane)
        const int64_t A1 = (int64_t)A1_lds[e], A2 = (int64_t)A2_lds[e];
        plan_lds[e] = cem_new_mean(plan_clip(plan_lds[e]), A1, Ne, c.alpha);
        std_lds[e] = cem_new_std(std_lds[e], A1, A2, Ne, c.alpha, c.std_min, c.std_max);
        A1_lds[e] = 0ull;
        A2_lds[e] = 0ull;
      }
      if (tid == 0 && it + 1 == x.iterations && x.m.best_ret) x.m.best_ret[(size_t)s * n + i] = beta;
      __syncthreads();
      if (tid == 0) *ne_lds = 0;   // (next added to after the next iteration's barriers)
    }
    // ACT: every lane steps a copy of the env with the plan's first row (`done` needs no broadcast); lane 0 puts its copy back
    const float act[3] = {plan_lds[base * 3], plan_lds[base * 3 + 1], plan_lds[base * 3 + 2]};
    Lane<NOBJ> L;
    copy_lane<NOBJ>(L, L_lds);
    float g[Dims<NOBJ>::NG];
#pragma unroll
    for (int j = 0; j < Dims<NOBJ>::NG; ++j) g[j] = g_lds[j];
    const bool done = mpc_act<NOBJ, GENERAL>(x, i, s, counter, L, g, act, tid == 0);
    __syncthreads();   // (everyone has read the env, and row 0 before its slot becomes row H - 1)
    if (tid == 0) {
      copy_lane<NOBJ>(L_lds, L);
#pragma unroll
      for (int j = 0; j < Dims<NOBJ>::NG; ++j) g_lds[j] = g[j];
    }
    // SHIFT
    if (GENERAL && done && a.cfg.auto_reset) {
      for (int e = tid; e < H * 3; e += nthr) plan_lds[e] = 0.0f;
    } else if (H > 1) {
      const int last = base == 0 ? H - 1 : base - 1;   // slot of row H - 1 before the shift = row H - 2 after it
      if (tid < 3) plan_lds[base * 3 + tid] = plan_lds[last * 3 + tid];
      base = base + 1 == H ? 0 : base + 1;
    }
    __syncthreads();
  }

  for (int e = tid; e < H * 3; e += nthr) {
    int r = base + e / 3;
    r = r >= H ? r - H : r;
    x.m.plan[((size_t)(e / 3) * n + i) * 3 + e % 3] = plan_lds[r * 3 + e % 3];
  }
  if (tid == 0) store_lane<NOBJ>(a, i, L_lds);
}

template <int NOBJ>
int do_cem_mpc(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* cp, const earl_plan_value* pv, int32_t T, const earl_tabletop_out* out,
               const earl_mpc_out* mpc, earl_stream_t stream) {
  int lanes;
  if (int rc = check_cem_mpc(cfg, st, NOBJ, cp, pv, T, out, mpc, &lanes)) return rc;
  if (lanes == 0) return EARL_OK;
  const CemMpcArgs c = cem_mpc_args(cfg, st, cp, T, out, mpc);
  const size_t lds = cem_mpc_lds_bytes<NOBJ>(cp->H, cp->K, cp->elites);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cfg->n), block((unsigned)lanes);
  if (is_general(cfg)) cem_mpc_kernel<NOBJ, true><<<grid, block, lds, s>>>(c);
  else cem_mpc_kernel<NOBJ, false><<<grid, block, lds, s>>>(c);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "cem_mpc_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

}  // namespace

extern "C" {

int earl_tabletop_mpc_rollout_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                  const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream) {
  return do_cem_mpc<1>(cfg, st, params, pv, T, out, mpc, stream);
}

int earl_tabletop3_mpc_rollout_cem(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_cem_params* params, const earl_plan_value* pv, int32_t T,
                                   const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream) {
  return do_cem_mpc<3>(cfg, st, params, pv, T, out, mpc, stream);
}

}  // extern "C"

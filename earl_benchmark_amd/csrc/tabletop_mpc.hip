// tabletop_mpc.hip -- earl_tabletop_mpc_rollout / earl_tabletop3_mpc_rollout (include/earl_tabletop.h, "receding-horizon MPPI control"): T real steps of
// plan -> act -> shift in ONE launch, equal bit for bit to the composition of earl_tabletop[3]_plan_mppi and the one-step rollout.  No cooperative launch, no flag
// between workgroups; the per-lane functions are tabletop_step.h's (through tabletop_mpc.h), shared with the host twin.
//
// mpc_kernel  a workgroup owns ONE env for the whole launch; its lanes are the K branches, 64 * ceil(K / 64) of them, lane k >= K idle in the score pass.
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

constexpr int kMpcWaves = kMpcMaxK / kBranchBlock;   // 16

template <int NOBJ>
inline size_t mpc_lds_bytes(int H, int K) {
  return (size_t)H * 3 * 8 + kMpcWaves * 8 + 8 + sizeof(Lane<NOBJ>) + Dims<NOBJ>::NG * 4 + (size_t)H * 3 * 4 + (size_t)K * 4 + kMpcWaves * 4;
}

template <int NOBJ, bool GENERAL>
__global__ __launch_bounds__(kMpcMaxK) void mpc_kernel(const MpcArgs x) {
  extern __shared__ unsigned long long lds_raw[];
  const int H = x.p.a.T, K = x.p.K, n = x.p.a.cfg.n;
  unsigned long long* const A_lds = lds_raw;                                   // [H][3]
  double* const b_lds = reinterpret_cast<double*>(A_lds + (size_t)H * 3);      // [kMpcWaves]
  unsigned long long* const S_lds = reinterpret_cast<unsigned long long*>(b_lds + kMpcWaves);
  static_assert(sizeof(Lane<NOBJ>) % 8 == 0, "the words after the env stay aligned");
  Lane<NOBJ>& L_lds = *reinterpret_cast<Lane<NOBJ>*>(S_lds + 1);               // the real env
  float (&g_lds)[Dims<NOBJ>::NG] = *reinterpret_cast<float (*)[Dims<NOBJ>::NG]>(&L_lds + 1);
  float* const plan_lds = &g_lds[0] + Dims<NOBJ>::NG;                          // [H][3], a ring
  int32_t* const w_lds = reinterpret_cast<int32_t*>(plan_lds + (size_t)H * 3); // [K]
  int32_t* const k_lds = w_lds + K;                                            // [kMpcWaves]

  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, wave = tid / kBranchBlock, waves = nthr / kBranchBlock;
  const int i = (int)blockIdx.x;   // (the grid is n workgroups)
  const int k = tid;
  const bool live = k < K;
  const KArgs& a = x.p.a;

  for (int e = tid; e < H * 3; e += nthr) {
    plan_lds[e] = x.m.plan[((size_t)(e / 3) * n + i) * 3 + e % 3];
    A_lds[e] = 0ull;
  }
  if (tid == 0) {
    *S_lds = 0ull;
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
  __syncthreads();

  for (int s = 0; s < x.T; ++s) {
    const uint64_t counter = a.cfg.counter + (uint64_t)s;
    q.noise_counter = x.p.noise_counter + (uint32_t)s;
    auto row = [&](int t, float (&m)[3]) {
      int r = base + t;
      r = r >= H ? r - H : r;
      m[0] = plan_clip(plan_lds[r * 3]);
      m[1] = plan_clip(plan_lds[r * 3 + 1]);
      m[2] = plan_clip(plan_lds[r * 3 + 2]);
    };
    for (int it = 0; it < x.iterations; ++it) {
      q.word0 = kPlanDraw | (uint32_t)(x.iteration0 + it);
      // SCORE
      double ret = 0.0, beta = -__builtin_inf();
      int bk = 0;
      if (live) {
        ret = mpc_score<NOBJ, GENERAL>(q, i, k, counter, L_lds, g_lds, row);
        plan_best(ret, k, beta, bk);
      }
      if (tid == 0 && x.m.ret0) x.m.ret0[((size_t)s * x.iterations + it) * n + i] = ret;
#pragma unroll
      for (int off = kBranchBlock / 2; off > 0; off >>= 1) {
        const double rb = __shfl_xor(beta, off, kBranchBlock);
        const int rk = __shfl_xor(bk, off, kBranchBlock);
        plan_best_merge(rb, rk, beta, bk);
      }
      if (waves > 1) {
        if (tid % kBranchBlock == 0) {
          b_lds[wave] = beta;
          k_lds[wave] = bk;
        }
        __syncthreads();
        beta = b_lds[0];
        bk = k_lds[0];
        for (int v = 1; v < waves; ++v) plan_best_merge(b_lds[v], k_lds[v], beta, bk);
      }
      if (live) {
        const int32_t W = plan_weight(ret, beta, q.inv_temperature);
        w_lds[k] = W;
        if (W != 0) atomicAdd(S_lds, (unsigned long long)W);
      }
      __syncthreads();
      // UPDATE, regenerating
      for (int item = tid; item < items; item += nthr) {
        const int t = item % H, grp = item / H;
        float m[3];
        row(t, m);
        int64_t A[3] = {0, 0, 0};
        for (int kk = 1 + grp; kk < K; kk += G) {   // (branch 0 is the mean: delta = 0)
          const int32_t W = w_lds[kk];
          if (W != 0) plan_accumulate(q, i, (uint32_t)kk, (uint32_t)t, m, W, A);
        }
        int r = base + t;
        r = r >= H ? r - H : r;
#pragma unroll
        for (int d = 0; d < 3; ++d)
          if (A[d] != 0) atomicAdd(&A_lds[r * 3 + d], (unsigned long long)A[d]);
      }
      __syncthreads();
      const int64_t S = (int64_t)*S_lds;
      for (int e = tid; e < H * 3; e += nthr) {   // (slot e of the ring: the same word read, written and cleared by one lane)
        plan_lds[e] = plan_new_mean(plan_clip(plan_lds[e]), (int64_t)A_lds[e], S);
        A_lds[e] = 0ull;
      }
      if (tid == 0 && it + 1 == x.iterations && x.m.best_ret) x.m.best_ret[(size_t)s * n + i] = beta;
      __syncthreads();
      if (tid == 0) *S_lds = 0ull;   // (next added to after the next iteration's barriers)
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
int do_mpc(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, int32_t T, const earl_tabletop_out* out, const earl_mpc_out* mpc,
           earl_stream_t stream) {
  int lanes;
  if (int rc = check_mpc(cfg, st, NOBJ, pp, T, out, mpc, &lanes)) return rc;
  if (lanes == 0) return EARL_OK;
  const MpcArgs x = mpc_args(cfg, st, pp, T, out, mpc);
  const size_t lds = mpc_lds_bytes<NOBJ>(pp->H, pp->K);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cfg->n), block((unsigned)lanes);
  if (cfg->goal_change_frequency > 0 || cfg->auto_reset) mpc_kernel<NOBJ, true><<<grid, block, lds, s>>>(x);
  else mpc_kernel<NOBJ, false><<<grid, block, lds, s>>>(x);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "mpc_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

}  // namespace

extern "C" {

int earl_tabletop_mpc_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                              const earl_mpc_out* mpc, earl_stream_t stream) {
  return do_mpc<1>(cfg, st, params, T, out, mpc, stream);
}

int earl_tabletop3_mpc_rollout(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* params, int32_t T, const earl_tabletop_out* out,
                               const earl_mpc_out* mpc, earl_stream_t stream) {
  return do_mpc<3>(cfg, st, params, T, out, mpc, stream);
}

}  // extern "C"

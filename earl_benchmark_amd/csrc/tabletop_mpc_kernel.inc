// tabletop_mpc_kernel.inc -- the receding-horizon kernel and its launcher: ONE text for the two units that instantiate it, included inside their anonymous namespaces
// (the project's idiom for a second build, as physics_bf16.hip: no new template parameter in a kernel's name, the first unit compiles to what it always compiled to).
//   tabletop_mpc.hip        as it stands: MpcArgs, the undiscounted sum.  The kernel's description is at the head of that file.
//   tabletop_mpc_value.hip  with EARL_PLAN_VALUE defined, inside namespace value: MpcValueArgs, mpc_score<.., true> -- the discounted sum and, after the look-ahead,
//                           the value network on the lane's own last observation row (tabletop_value.h: scalar weight loads, no LDS).  The env copy is dead by then;
//                           the row and one hidden layer of at most EARL_PLAN_VALUE_MAX_H1 registers are what is live.  UPDATE, ACT and SHIFT see returns only.
constexpr int kMpcWaves = kMpcMaxK / kBranchBlock;   // 16

template <int NOBJ>
inline size_t mpc_lds_bytes(int H, int K) {
  return (size_t)H * 3 * 8 + kMpcWaves * 8 + 8 + sizeof(Lane<NOBJ>) + Dims<NOBJ>::NG * 4 + (size_t)H * 3 * 4 + (size_t)K * 4 + kMpcWaves * 4;
}

#ifdef EARL_PLAN_VALUE
typedef MpcValueArgs LoopArgs;
#else
typedef MpcArgs LoopArgs;
#endif

template <int NOBJ, bool GENERAL>
__global__ __launch_bounds__(kMpcMaxK) void mpc_kernel(const LoopArgs x) {
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
#ifdef EARL_PLAN_VALUE
        ret = mpc_score<NOBJ, GENERAL, true>(q, i, k, counter, L_lds, g_lds, row, &x.v);
#else
        ret = mpc_score<NOBJ, GENERAL>(q, i, k, counter, L_lds, g_lds, row);
#endif
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

// pv: the `_value` entry points' block (checked here), NULL in tabletop_mpc.hip
template <int NOBJ>
int do_mpc(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, [[maybe_unused]] const earl_plan_value* pv, int32_t T,
           const earl_tabletop_out* out, const earl_mpc_out* mpc, earl_stream_t stream) {
  int lanes;
  if (int rc = check_mpc(cfg, st, NOBJ, pp, T, out, mpc, &lanes)) return rc;
#ifdef EARL_PLAN_VALUE
  if (int rc = check_plan_value(pv, Dims<NOBJ>::NOBS)) return rc;
#endif
  if (lanes == 0) return EARL_OK;
  LoopArgs x{};
  static_cast<MpcArgs&>(x) = mpc_args(cfg, st, pp, T, out, mpc);
#ifdef EARL_PLAN_VALUE
  x.v = value_args(pv);
#endif
  const size_t lds = mpc_lds_bytes<NOBJ>(pp->H, pp->K);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cfg->n), block((unsigned)lanes);
  if (is_general(cfg)) mpc_kernel<NOBJ, true><<<grid, block, lds, s>>>(x);
  else mpc_kernel<NOBJ, false><<<grid, block, lds, s>>>(x);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "mpc_kernel: %s", hipGetErrorString(e));
  return EARL_OK;
}

// tabletop_plan_kernel.inc -- the planner's score kernel and the loop of launches around it: ONE text for the two units that instantiate it, included inside their
// anonymous namespaces (the project's idiom for a second build, as physics_bf16.hip: no new template parameter in a kernel's name, the first unit compiles to what
// it always compiled to).
//   tabletop_plan.hip        as it stands: PlanArgs, the undiscounted sum
//   tabletop_plan_value.hip  with EARL_PLAN_VALUE defined, inside namespace value: PlanValueArgs, plan_score_body<.., true> -- the discounted sum and, after the loop,
//                            the value network on the lane's own observation row (tabletop_value.h: weights through scalar loads, no LDS)
// plan_score_kernel   the branch launch's shape: one lane per (branch, env), a wave = 64 consecutive envs of ONE branch (so `k == 0`, the plan itself, is
//                     wave-uniform), a workgroup = that wave, 1-D grid of K * ceil(n / 64).
#ifdef EARL_PLAN_VALUE
typedef PlanValueArgs ScoreArgs;
#else
typedef PlanArgs ScoreArgs;
#endif

template <int NOBJ, bool GENERAL>
__global__ __launch_bounds__(kBranchBlock) void plan_score_kernel(const ScoreArgs p, const unsigned tiles) {
  const unsigned k = blockIdx.x / tiles;
  const unsigned i = (blockIdx.x - k * tiles) * kBranchBlock + threadIdx.x;
#ifdef EARL_PLAN_VALUE
  if (i < (unsigned)p.a.cfg.n) plan_score_body<NOBJ, GENERAL, true>(p, (int)i, (int)k, &p.v);
#else
  if (i < (unsigned)p.a.cfg.n) plan_score_body<NOBJ, GENERAL>(p, (int)i, (int)k);
#endif
}

// pv: the `_value` entry points' block (checked here), NULL in tabletop_plan.hip
template <int NOBJ>
int do_plan(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_plan_params* pp, [[maybe_unused]] const earl_plan_value* pv, const float* mean,
            float* plan, double* ret, double* ret0, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  long long blocks, ublocks;
  if (int rc = check_plan(cfg, st, NOBJ, pp, 0, mean, plan, ret, &blocks, &ublocks)) return rc;
#ifdef EARL_PLAN_VALUE
  if (int rc = check_plan_value(pv, Dims<NOBJ>::NOBS)) return rc;
#endif
  if (blocks == 0) return EARL_OK;
  ScoreArgs p{};
  static_cast<PlanArgs&>(p) = plan_args(cfg, st, pp, mean, thresholds());
#ifdef EARL_PLAN_VALUE
  p.v = value_args(pv);
#endif
  p.plan = plan;
  p.ret = ret;
  const unsigned tiles = (unsigned)(blocks / pp->K);
  const bool general = is_general(cfg);
  const hipStream_t s = (hipStream_t)stream;
  for (int it = 0; it < pp->iterations; ++it) {
    const bool last = it + 1 == pp->iterations;
    p.mean = it ? plan : mean;
    p.word0 = kPlanDraw | (uint32_t)(pp->iteration0 + it);
    p.ret0 = ret0 ? ret0 + (size_t)it * cfg->n : nullptr;
    p.best_ret = last ? best_ret : nullptr;
    p.best_k = last ? best_k : nullptr;
    if (general) plan_score_kernel<NOBJ, true><<<dim3((unsigned)blocks), kBranchBlock, 0, s>>>(p, tiles);
    else plan_score_kernel<NOBJ, false><<<dim3((unsigned)blocks), kBranchBlock, 0, s>>>(p, tiles);
    plan_update_launch(p, tiles, (unsigned)ublocks, stream);   // (the update sees returns only: one kernel, in tabletop_plan.hip, for both units)
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EARL_ERR_LAUNCH, "plan kernels: %s", hipGetErrorString(e));
  }
  return EARL_OK;
}

// plan_update_probe.hip -- TEST INFRASTRUCTURE ONLY (tests/plan_update_cases.py builds it on demand; nothing here is part of libearl_hip.so).
//
// A door to the update kernel of a shooting planner on GIVEN returns: the product reaches sawyer_plan_update_kernel and minitaur_plan_update_kernel only through
// earl_*_plan_mppi, behind real rollouts, whose returns are finite, distinct and close together.  This unit INCLUDES the product unit itself, so that the kernel it
// launches is the product's text and not a copy, and adds one launcher whose arguments are the host twin's (earl_*_plan_update_cpu, include/earl_physics.h) plus a
// stream: the twin's argument check, the unit's own *_plan_args, <<<n, kUpdateThreads>>> as the driver launches it.
//
// Built twice with exactly the product's HIPFLAGS (csrc/Makefile): -DEARL_PROBE_SAWYER=1 includes csrc/sawyer_plan.hip, without it csrc/minitaur_plan.hip (the two
// units cannot share a translation unit: both define kUpdateThreads and launch_candidates in an anonymous namespace).  The public symbols the included unit calls
// (earl_sawyer_branch_rollout, earl_sawyer_branch_ws_bytes, earl_minitaur_branch_rollout, ...) stay undefined here: the loader resolves them from libearl_hip.so, which
// tests/plan_update_cases.py loads RTLD_GLOBAL first.  The launcher reaches none of them.
#ifdef EARL_PROBE_SAWYER
#include "../earl_benchmark_amd/csrc/sawyer_plan.hip"

// sawyer_shoot.h declares the planners' scoring call with hidden visibility (its definition is sawyer_value.hip's): a shared object cannot leave it undefined.  A
// test-only definition that refuses; the launcher below never reaches it.
extern "C" __attribute__((visibility("hidden"))) int earl_unit_sawyer_branch_scored(const earl_link_model*, const earl_collision_model*, int32_t, const earl_sawyer_cfg*,
                                                                                    const earl_sawyer_state*, int32_t, int32_t, float*, int64_t, const uint64_t*,
                                                                                    const earl_plan_value*, const earl_sawyer_plan_prior*, uint32_t, uint32_t,
                                                                                    const earl_sawyer_branch_ws*, const earl_episode_summary*, double*, int32_t*, earl_stream_t) {
  return EARL_ERR_LAUNCH;
}

extern "C" int probe_sawyer_plan_update(const earl_sawyer_cfg* cfg, const earl_sawyer_plan_params* params, int32_t j, const float* mean, const float* act, const double* ret,
                                        float* plan, double* ret0_row, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (int rc = check_sawyer_plan(SawyerPlanCall::Update, cfg, params, j, mean, plan)) return rc;
  if (!act || !ret) return fail(EARL_ERR_ARG, "act/ret is NULL");
  if (cfg->n == 0) return EARL_OK;
  SawyerPlanArgs p = sawyer_plan_args(cfg, params, mean);
  p.plan = plan;
  p.act = const_cast<float*>(act);                                                    // (the update kernel reads the candidates and never writes them)
  p.ret = ret;
  p.ret0 = ret0_row;
  p.best_ret = best_ret;
  p.best_k = best_k;
  p.word0 = kPlanDraw | (uint32_t)j;
  sawyer_plan_update_kernel<<<dim3((unsigned)cfg->n), kUpdateThreads, 0, (hipStream_t)stream>>>(p);
  return launched("sawyer_plan_update_kernel");
}
extern "C" int probe_plan_update_threads() { return kUpdateThreads; }
#else
#include "../earl_benchmark_amd/csrc/minitaur_plan.hip"

extern "C" int probe_minitaur_plan_update(const earl_minitaur_cfg* cfg, const earl_minitaur_plan_params* params, int32_t j, const float* mean, const float* act,
                                          const double* ret, float* plan, double* ret0_row, double* best_ret, int32_t* best_k, earl_stream_t stream) {
  if (int rc = check_minitaur_plan(MinitaurPlanCall::Update, cfg, params, j, mean, plan)) return rc;
  if (!act || !ret) return fail(EARL_ERR_ARG, "act/ret is NULL");
  if (cfg->n == 0) return EARL_OK;
  MinitaurPlanArgs p = minitaur_plan_args(cfg, params, mean);
  p.plan = plan;
  p.act = const_cast<float*>(act);                                                    // (the update kernel reads the candidates and never writes them)
  p.ret = ret;
  p.ret0 = ret0_row;
  p.best_ret = best_ret;
  p.best_k = best_k;
  p.word0 = kPlanDraw | (uint32_t)j;
  minitaur_plan_update_kernel<<<dim3((unsigned)cfg->n), kUpdateThreads, 0, (hipStream_t)stream>>>(p);
  return launched("minitaur_plan_update_kernel");
}
extern "C" int probe_plan_update_threads() { return kUpdateThreads; }
#endif

// physics_env_sawyer_prior.inc -- the pieces of the Sawyer door / peg rollout that only the prior-branch units hold (physics_branch_prior.hip, physics_branch_prior_w8.hip:
// EARL_BRANCH_PRIOR): the policy phase of a prior branch and sawyer_prior_rollout_kernel, the fourth inclusion of physics_env_sawyer_rollout.inc.  Included by
// physics_env_sawyer.h under that define, after the branch pieces and EARL_WAVES_PER_EU and in front of the other rollout kernels (whose bodies name sawyer_prior_step_action).
// The action of env step t of a PRIOR branch (sawyer_prior_rollout_kernel), on all 16 lanes of the virtual env's group: the policy phase of sawyer_policy_action on the
// row the branch carries (element `sub` on lane `sub`, each double rounded to float32; step 0: the env's row of obs0), then a[d] = plan_clip(fmaf(sigma[d], eps_d, u[d]))
// with eps from the ONE Philox block noise branch k of the planner would have drawn for (iteration, env, k, t, noise_counter) (sawyer_plan.h: splan_candidate; words
// x, y, z, w serve dimensions 0 .. 3).  Lane 0 of a live env stores the row -- one 16-byte store -- into the branch's block of the candidates the call scores, and into
// prior_act when given: replaying that array through the plain branch launch loads exactly these words.  Everything is read through the kernel-argument segment here
// (see sawyer_policy_action on why); a group that is not live computes on zeros and writes nothing.
__device__ __noinline__ float4 sawyer_prior_action(const uint64_t ka_bits, const double* __restrict__ seen, const int t, const int v, const int sub, const bool live) {
#pragma clang fp contract(off)
  const EARL_KARG SawyerBranchPriorArgs* ka = cl_kernarg<SawyerBranchPriorArgs>(ka_bits);
  const int n_layers = ka->pol.n_layers, d0 = ka->pol.dims[0], d1 = ka->pol.dims[1], d2 = ka->pol.dims[2], d3 = ka->pol.dims[3];
  const int hidden_act = ka->pol.hidden_act, out_act = ka->pol.out_act;
  const int n = ka->n_env, k = v / n, i = v - k * n;
  if (!seen) seen = ka->obs0 + (size_t)i * 14;         // step 0
  float h[16];
  h[0] = (sub < 14 && live) ? (float)seen[sub] : 0.f;
#pragma unroll
  for (int j = 1; j < 16; ++j) h[j] = 0.f;
  const float* w = ka->pol.params;
  pol_layer<16, false>(w, w + (size_t)d1 * d0, d0, d1, hidden_act, sub, h);
  w += (size_t)d1 * (d0 + 1);
  if (n_layers == 3) {
    pol_layer<16, true>(w, w + (size_t)d2 * d1, d1, d2, hidden_act, sub, h);
    w += (size_t)d2 * (d1 + 1);
  }
  const int KL = n_layers == 3 ? d2 : d1, NL = n_layers == 3 ? d3 : d2;
  pol_layer<16, true>(w, w + (size_t)NL * KL, KL, NL, EARL_ACT_NONE, sub, h);       // lane j < 4 holds output j
  const float u = earl::policy_act(h[0], out_act);
  const uint64_t seed = ka->cfg.seed;
  const earl::U4 b = earl::philox4x32_10(earl::U4{ka->word0, (uint32_t)(ka->cfg.env_offset + i), ((uint32_t)(ka->kbase + k) << 16) | (uint32_t)t, ka->noise_counter},
                                         (uint32_t)seed, (uint32_t)(seed >> 32));
  const int d = sub & 3;
  const float eps = earl::normal_quantile_f32((d == 0 ? b.x : (d == 1 ? b.y : (d == 2 ? b.z : b.w))) >> 8);
  const float s = d == 0 ? ka->sigma[0] : (d == 1 ? ka->sigma[1] : (d == 2 ? ka->sigma[2] : ka->sigma[3]));
  const float c = __builtin_fmaf(s, eps, u);
  const float lo = c > -1.0f ? c : -1.0f;              // plan_clip of tabletop_plan.h: two compare-and-selects, NaN -> -1
  const float a = lo < 1.0f ? lo : 1.0f;
  const float4 act{__shfl(a, 0, 16), __shfl(a, 1, 16), __shfl(a, 2, 16), __shfl(a, 3, 16)};
  if (sub == 0 && live) {
    const size_t row = ((size_t)t * n + i) * 4;
    *reinterpret_cast<float4*>(const_cast<float*>(ka->action) + (size_t)k * (size_t)ka->act_stride + row) = act;
    float* const pa = ka->prior_act;
    if (pa) *reinterpret_cast<float4*>(pa + (size_t)(k - ka->k0) * ((size_t)ka->T * n * 4) + row) = act;
  }
  return act;
}
// ... called from the rollout body: the row virtual env v emitted last (the workspace's or the caller's last_obs row: a rolled-back step's repeated row, the goal block a
// goal switch patched), lane `sub` reading what lane `sub` wrote; the first step of a time slice reads a row another wave wrote, under sched_release / sched_claim
// A virtual env in front of the launch's first prior branch loads its action like a plain branch; a wave that holds none of the policy's (wave-uniform: the prior
// branches are the tail, so in the one-launch shape that is all but the last P n / 4 waves) never enters the policy phase
__device__ __forceinline__ float4 sawyer_prior_step_action(const int t, const int v, const int sub, const bool live) {
  const EARL_KARG SawyerBranchPriorArgs* ka = cl_kernarg<SawyerBranchPriorArgs>();
  const bool mine = v >= ka->k0 * ka->n_env;
  if (!__any(mine && live)) return sawyer_branch_action(t, v);
  const double* seen = t > 0 ? ka->obs_row + (size_t)v * 14 : nullptr;
  const float4 act = sawyer_prior_action((uint64_t)ka, seen, t, v, sub, live && mine);
  return mine ? act : sawyer_branch_action(t, v);
}

// The branch rollout whose actions are the policy's (earl_sawyer_branch_rollout_prior: the last P branches of a call; instantiated in physics_branch_prior.hip and
// physics_branch_prior_w8.hip only): the branch inclusion with sawyer_prior_step_action in the place of the action load.  `a` must stay the kernel's ONLY argument
static_assert(std::is_trivially_copyable<SawyerBranchPriorArgs>::value, "the prior's policy phase reads SawyerBranchPriorArgs as laid out in the kernel-argument segment");
template <int NV, int LPE, bool SLICED = false>
__global__ __launch_bounds__(64 * Lim<NV>::WPB, EARL_WAVES_PER_EU) void sawyer_prior_rollout_kernel(const SawyerBranchPriorArgs a) {
  static_assert(LPE == 16, "the policy phase is laid out over 16 lanes per env");
  constexpr bool POLICY = false;
  constexpr bool BRANCH = true;
#include "physics_env_sawyer_rollout.inc"
}

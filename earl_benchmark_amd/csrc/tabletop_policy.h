// tabletop_policy.h -- the closed-loop tabletop rollout: a float32 MLP policy 12 -> hidden (-> hidden) -> 3 evaluated between the env steps of ONE
// launch (include/earl_tabletop.h: earl_tabletop_policy_rollout).  Shared by the gfx950 kernel (tabletop_policy.hip) and its host twin
// (tabletop_host.cpp, -DEARL_HOST_BUILD); the per-env step is tabletop_step.h's wrapped_step<1, GENERAL>, not restated here.  The same kernel with a
// Gaussian head (12 -> hidden (-> hidden) -> 6, actions sampled inside the launch: earl_tabletop_policy_rollout_gaussian) is instantiated in
// tabletop_policy_gaussian.hip; its sampling contract follows the deterministic one below.
//
// The policy arithmetic is a contract, stated here once for both builds:
//   pre-activation   acc = b_j;  for k = 0 .. K-1 ascending:  acc = fmaf(x_k, W_jk, acc)     (float32, one rounding per fused multiply-add)
//   ReLU             acc > 0 ? acc : +0                                                     (= fmaxf(acc, 0) with -0 -> +0 and NaN -> 0 pinned)
//   tanh             tanh_f32 below
// On gfx950 the chain is v_mfma_f32_16x16x4_f32: per output element bit for bit a k-ordered fmaf chain, C input = the bias.  The host states the loops.
#pragma once
#include "tabletop_hostside.h"
#include "tabletop_step.h"

namespace earl {

constexpr int kPolicyMaxWidth = 256;   // hidden widths: multiples of 16 in 16 .. 256
constexpr int kPolicyEnvsPerWg = 16;   // the M of 16x16x4

// ------------------------------------------------------------------------------------------------
// tanh_f32: float32 in, float32 out, evaluated in fp64 out of fma, +, *, the correctly rounded / and integer operations only (no libm / ocml call), and
// rounded to float32 ONCE -- host and device agree bit for bit, and the single rounding of a 1e-15-accurate value is what makes it odd, monotone over
// every float32 and within 0.5 ulp (+ 1e-8) of tanh (tests/test_policy_rollout.py sweeps every float32 in 2^-12 <= |x| <= 16).
//   |x| <  2^-6 : x + x z (-1/3 + z (2/15 + z (-17/315 + z 62/2835))), z = x^2                 (next term 1382/155925 z^5 < 1e-20 relative)
//   |x| <  10   : t = exp(-2|x|) = 2^k e^r, k = round(-2|x| log2 e), r in two Cody-Waite steps, e^r by its Taylor series to r^12 / 12!
//                 (|r| <= 0.35: remainder 3e-16); tanh = (1 - t) / (1 + t)
//   |x| >= 10   : 1 (1 - tanh(10) = 4e-9 < 2^-25), +-Inf included;  NaN -> NaN;  the sign is copied from x, so +-0 -> +-0
// ------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ float tanh_f32(float x) {
  const uint32_t ux = __builtin_bit_cast(uint32_t, x), ax = ux & 0x7fffffffu;
  if (ax > 0x7f800000u) return x + x;
  float r = 1.0f;
  if (ax < 0x41200000u) {
    const double a = (double)__builtin_bit_cast(float, ax);
    double v;
    if (ax < 0x3c800000u) {
      const double z = a * a;
      double p = 62.0 / 2835.0;
      p = fma(z, p, -17.0 / 315.0);
      p = fma(z, p, 2.0 / 15.0);
      p = fma(z, p, -1.0 / 3.0);
      v = fma(a, z * p, a);
    } else {
      const double y = -2.0 * a;
      const int k = (int)(y * 1.4426950408889634 - 0.5);
      const double kd = (double)k;
      double s = fma(kd, -6.93147180369123816490e-01, y);   // ln 2 split: the high part has 32 significant bits, k * hi is exact
      s = fma(kd, -1.90821492927058770002e-10, s);
      double p = 1.0 / 479001600.0;
      p = fma(s, p, 1.0 / 39916800.0);
      p = fma(s, p, 1.0 / 3628800.0);
      p = fma(s, p, 1.0 / 362880.0);
      p = fma(s, p, 1.0 / 40320.0);
      p = fma(s, p, 1.0 / 5040.0);
      p = fma(s, p, 1.0 / 720.0);
      p = fma(s, p, 1.0 / 120.0);
      p = fma(s, p, 1.0 / 24.0);
      p = fma(s, p, 1.0 / 6.0);
      p = fma(s, p, 0.5);
      p = fma(s, p, 1.0);
      p = fma(s, p, 1.0);
      const double t = p * __builtin_bit_cast(double, (uint64_t)(1023 + k) << 52);
      v = (1.0 - t) / (1.0 + t);
    }
    r = (float)v;
  }
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, r) | (ux & 0x80000000u));
}

__host__ __device__ __forceinline__ float relu_f32(float x) { return x > 0.0f ? x : 0.0f; }

__host__ __device__ __forceinline__ float policy_act(float x, int kind) {
  return kind == EARL_ACT_RELU ? relu_f32(x) : (kind == EARL_ACT_TANH ? tanh_f32(x) : x);
}

// ------------------------------------------------------------------------------------------------
// The Gaussian head (include/earl_tabletop.h: earl_tabletop_policy_rollout_gaussian).  The sampling contract, stated here once for the kernel and the host twin:
//   network     the same MLP with a 6-wide last layer and NO activation on it: rows 0..2 = mean, rows 3..5 = raw log_std
//   draws       ONE Philox4x32-10 block per (env, step): draw_block(cfg, counter, env, kGaussDraw) -- key = cfg.seed, counter words = {kGaussDraw, global env id,
//               counter lo, counter hi}, `counter` = the counter of that env step (the value policy_env_step passes to wrapped_step).  The env's own draws use
//               draw indices 0 .. 2048 (tabletop_device.h): the streams are disjoint, and the noise takes no counter values of its own.  Words x, y, z serve
//               action dimensions 0, 1, 2; w is unused.
//   uniform     the word's HIGH 24 bits: k = w >> 8, u = (k + 0.5) 2^-24; q = u - 0.5 and the tail probability 0.5 - |q| are exact in float32
//   eps         normal_quantile_f32(k) below = Phi^-1(u) within 5 float32 ulp, |eps| <= 5.4199834, exactly odd in k <-> 2^24 - 1 - k
//   log_std     CLAMP: t = raw > lo ? raw : lo; ls = t < hi ? t : hi   (= min(max(raw, lo), hi); NaN -> lo)
//               TANH : ls = lo + (0.5f * (hi - lo)) * (tanh_f32(raw) + 1.0f), every operation rounded to float32 once
//   action      MEAN: u = mean.  SAMPLE: u = fmaf(exp_f32(ls), eps, mean).  act = policy_act(u, out_act) (NONE or tanh_f32)
// exp_f32 and normal_quantile_f32 are, like tanh_f32, made of fma / fmaf, +, *, the correctly rounded / and float32 sqrt and integer operations only (no
// libm / ocml call): host and device agree bit for bit (tests/test_policy_gaussian.py sweeps all 2^24 quantile inputs and every float32 of [-20, 4]).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kGaussDraw = 0x504F4C00u;

// exp_f32: float32 in, float32 out; tanh_f32's exp (k = round(x log2 e), two Cody-Waite steps, Taylor series to r^12 / 12!, |r| <= 0.35) in fp64, rounded to
// float32 ONCE: within 0.5 ulp (+ 1e-8).  NaN -> NaN, x >= 89 -> +Inf, x <= -104 -> +0; the log_std bounds keep the argument inside [-20, 4].
__host__ __device__ __forceinline__ float exp_f32(float x) {
  if (!(x == x)) return x + x;
  if (x >= 89.0f) return __builtin_inff();
  if (x <= -104.0f) return 0.0f;
  const double y = (double)x;
  const int k = (int)(y * 1.4426950408889634 + (x < 0.0f ? -0.5 : 0.5));
  const double kd = (double)k;
  double s = fma(kd, -6.93147180369123816490e-01, y);
  s = fma(kd, -1.90821492927058770002e-10, s);
  double p = 1.0 / 479001600.0;
  p = fma(s, p, 1.0 / 39916800.0);
  p = fma(s, p, 1.0 / 3628800.0);
  p = fma(s, p, 1.0 / 362880.0);
  p = fma(s, p, 1.0 / 40320.0);
  p = fma(s, p, 1.0 / 5040.0);
  p = fma(s, p, 1.0 / 720.0);
  p = fma(s, p, 1.0 / 120.0);
  p = fma(s, p, 1.0 / 24.0);
  p = fma(s, p, 1.0 / 6.0);
  p = fma(s, p, 0.5);
  p = fma(s, p, 1.0);
  p = fma(s, p, 1.0);
  return (float)(p * __builtin_bit_cast(double, (uint64_t)(1023 + k) << 52));
}

// normal_quantile_f32: eps = Phi^-1((k + 0.5) 2^-24) for the 24-bit k, in float32.  Wichura's AS 241 PPND7 rationals: with m = 2 k + 1 - 2^24 (odd, |m| < 2^24:
// exact in float32) and |q| = |m| 2^-25,
//   |q| <= 0.425 : |q| R1(0.180625 - q^2)                                     (the form q R(q^2): relative accuracy holds down to the smallest |q| = 2^-25)
//   otherwise    : R2(sqrt(-ln p) - 1.6), p = 0.5 - |q| = (2^24 - |m|) 2^-25  (exact; AS 241's third branch, sqrt(-ln p) > 5, is unreachable: p >= 2^-25 gives 4.163)
// -ln p: p = mm 2^e with mm in [sqrt(1/2), sqrt 2), ln mm = 2 z + z^3 (2/3 + 2/5 z^2 + 2/7 z^4 + 2/9 z^6), z = (mm - 1) / (mm + 1), ln 2 split in two so that e ln2_hi
// is exact.  The sign is copied from m, so eps(k) == -eps(2^24 - 1 - k) as bit patterns.  Not monotone to the last bit (68 adjacent pairs out of order).
__host__ __device__ __forceinline__ float normal_quantile_f32(uint32_t k) {
  const int32_t m = (int32_t)(2u * k + 1u) - (1 << 24);
  const uint32_t am = (uint32_t)(m < 0 ? -m : m);
  const float aq = (float)am * 0x1p-25f;
  float v;
  if (am <= 14260633u) {                                   // aq <= 0.425
    const float r = fmaf(-aq, aq, 0.180625f);
    float num = fmaf(5.9109374720e+01f, r, 1.5929113202e+02f);
    num = fmaf(num, r, 5.0434271938e+01f);
    num = fmaf(num, r, 3.3871327179e+00f);
    float den = fmaf(6.7187563600e+01f, r, 7.8757757664e+01f);
    den = fmaf(den, r, 1.7895169469e+01f);
    den = fmaf(den, r, 1.0f);
    v = (aq * num) / den;
  } else {
    const float p = (float)((1u << 24) - am) * 0x1p-25f;
    const uint32_t b = __builtin_bit_cast(uint32_t, p), mb = b & 0x007fffffu;
    const bool up = mb > 0x003504f3u;
    const float ef = (float)((int32_t)(b >> 23) - 127 + (up ? 1 : 0));
    const float mm = __builtin_bit_cast(float, (mb | 0x3f800000u) - (up ? 0x00800000u : 0u));
    const float z = (mm - 1.0f) / (mm + 1.0f), w = z * z;
    float s = 2.0f / 9.0f;
    s = fmaf(w, s, 2.0f / 7.0f);
    s = fmaf(w, s, 2.0f / 5.0f);
    s = fmaf(w, s, 2.0f / 3.0f);
    const float lm = fmaf(z * w, s, 2.0f * z);
    const float nl = fmaf(-ef, 6.9313812256e-01f, -fmaf(ef, 9.0580006145e-06f, lm));
    const float r = __builtin_sqrtf(nl) - 1.6f;
    float num = fmaf(1.7023821103e-01f, r, 1.3067284816e+00f);
    num = fmaf(num, r, 2.7568153900e+00f);
    num = fmaf(num, r, 1.4234372777e+00f);
    float den = fmaf(1.2021132975e-01f, r, 7.3700164250e-01f);
    den = fmaf(den, r, 1.0f);
    v = num / den;
  }
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) | (m < 0 ? 0x80000000u : 0u));
}

// one (env, dimension) of the head: the action from the network's two outputs and the draw eps = normal_quantile_f32(word >> 8)
__host__ __device__ __forceinline__ float gaussian_head_action(const earl_gaussian_head& h, int out_act, float mean, float raw, float eps) {
  float u = mean;
  if (h.mode == EARL_HEAD_SAMPLE) {
    const float lo = h.log_std_min, hi = h.log_std_max;
    float ls;
    if (h.log_std_map == EARL_LOGSTD_TANH) {
      ls = lo + (0.5f * (hi - lo)) * (tanh_f32(raw) + 1.0f);
    } else {
      const float t = raw > lo ? raw : lo;
      ls = t < hi ? t : hi;
    }
    u = fmaf(exp_f32(ls), eps, mean);
  }
  return policy_act(u, out_act);
}

// ------------------------------------------------------------------------------------------------
// arguments
// ------------------------------------------------------------------------------------------------
struct PolicyArgs {
  KArgs k;              // cfg / state / outputs / thresholds; k.T = steps per episode; k.act unused
  earl_mlp_policy p;
  float* act_out;
  int32_t episodes;
  int32_t reset_first;
};
struct GaussianPolicyArgs : PolicyArgs {   // the deterministic kernels keep PolicyArgs as their kernel argument
  earl_gaussian_head head;
};
template <bool GAUSS>
struct PolicyArgsOf { using type = PolicyArgs; };
template <>
struct PolicyArgsOf<true> { using type = GaussianPolicyArgs; };

namespace hostside {

inline int check_policy(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, int32_t episodes, int32_t T,
                        int32_t reset_first, const earl_tabletop_out* out, int out_dim = EARL_TABLETOP_ACT_DIM) {
  if (int rc = check_common(cfg, st, 1)) return rc;
  if (!p || !out) return fail(EARL_ERR_ARG, "policy/out is NULL");
  if (!p->params) return fail(EARL_ERR_ARG, "policy params is NULL");
  if (p->precision != 0) return fail(EARL_ERR_ARG, "policy precision = %d: only 0 (fp32) exists", p->precision);
  if (p->n_layers != 2 && p->n_layers != 3) return fail(EARL_ERR_ARG, "policy n_layers = %d: 2 (one hidden layer) or 3 (two)", p->n_layers);
  if (p->dims[0] != EARL_TABLETOP_OBS_DIM || p->dims[p->n_layers] != out_dim)
    return fail(EARL_ERR_ARG, "policy dims: input %d, output %d (want 12 and %d)", p->dims[0], p->dims[p->n_layers], out_dim);
  for (int l = 1; l < p->n_layers; ++l)
    if (p->dims[l] < 16 || p->dims[l] > kPolicyMaxWidth || p->dims[l] % 16) return fail(EARL_ERR_ARG, "policy hidden width %d: a multiple of 16 in 16..256", p->dims[l]);
  if (p->n_layers == 2 && p->dims[3] != 0) return fail(EARL_ERR_ARG, "policy dims[3] = %d is unused and must be 0", p->dims[3]);
  if (p->hidden_act != EARL_ACT_RELU && p->hidden_act != EARL_ACT_TANH) return fail(EARL_ERR_ARG, "policy hidden_act = %d", p->hidden_act);
  if (p->out_act != EARL_ACT_NONE && p->out_act != EARL_ACT_TANH) return fail(EARL_ERR_ARG, "policy out_act = %d", p->out_act);
  if (T < 1) return fail(EARL_ERR_ARG, "T = %d < 1", T);
  if (episodes < 1) return fail(EARL_ERR_ARG, "episodes = %d < 1", episodes);
  if (reset_first != 0 && reset_first != 1) return fail(EARL_ERR_ARG, "reset_first = %d", reset_first);
  if (!reset_first && episodes != 1) return fail(EARL_ERR_ARG, "episodes = %d without reset_first: a continuing rollout is one episode", episodes);
  return EARL_OK;
}

// the Gaussian-head entry points: the policy's checks with a 6-wide last layer (mean, raw log_std), then the head's
inline int check_policy_gaussian(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, const earl_gaussian_head* h,
                                 int32_t episodes, int32_t T, int32_t reset_first, const earl_tabletop_out* out) {
  if (int rc = check_policy(cfg, st, p, episodes, T, reset_first, out, 2 * EARL_TABLETOP_ACT_DIM)) return rc;
  if (!h) return fail(EARL_ERR_ARG, "head is NULL");
  if (h->mode != EARL_HEAD_MEAN && h->mode != EARL_HEAD_SAMPLE) return fail(EARL_ERR_ARG, "head mode = %d", h->mode);
  if (h->log_std_map != EARL_LOGSTD_CLAMP && h->log_std_map != EARL_LOGSTD_TANH) return fail(EARL_ERR_ARG, "head log_std_map = %d", h->log_std_map);
  if (!(h->log_std_min >= -20.0f && h->log_std_max <= 4.0f && h->log_std_min <= h->log_std_max))       // (NaN fails every comparison)
    return fail(EARL_ERR_ARG, "head log_std bounds [%g, %g]: finite, min <= max, inside [-20, 4]", (double)h->log_std_min, (double)h->log_std_max);
  return EARL_OK;
}

}  // namespace hostside

// the env's side of one closed-loop launch, shared by the kernel's env lanes and the host loop: what happens to ONE env before episode e's first step
// (reset_body's reset on register state, or nothing) and the observation the first action is computed from
template <bool GENERAL>
__device__ __forceinline__ void policy_episode_begin(const PolicyArgs& a, int i, int e, Lane<1>& L, float (&g)[6], float (&o)[12]) {
  if (a.reset_first) {                              // reset_body: Philox counter of episode e's reset = cfg.counter + e (T + 1)
    L.goal_idx = reset_env<1>(L.e, a.k.cfg, a.k.cfg.counter + (uint64_t)e * (uint64_t)(a.k.T + 1), i, a.k.st.goal_table, nullptr, a.k.th);
    L.steps = 0;
    L.sgc = 0;
    L.resets += 1;
    load_goal<1>(a.k.st.goal_table, L.goal_idx, g);
  }
  make_obs<1>(L.e, g, o);
}

// the Philox counter of step t of episode e: what wrapped_step gets, and what keys the Gaussian head's draw of that step
__device__ __forceinline__ uint64_t policy_step_counter(const PolicyArgs& a, int e, int t) {
  return a.k.cfg.counter + (uint64_t)e * (uint64_t)(a.k.T + 1) + (uint64_t)(a.reset_first ? 1 : 0) + (uint64_t)t;
}

// one closed-loop step of one env given the policy's action (a0, a1, a2): act_out, wrapped_step, outputs
template <bool GENERAL>
__device__ __forceinline__ void policy_env_step(const PolicyArgs& a, int i, int e, int t, Lane<1>& L, float (&g)[6], float a0, float a1, float a2, float (&o)[12]) {
  const size_t row = ((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)i;
  if (a.act_out) {
    float* ap = a.act_out + row * 3;
    ap[0] = a0; ap[1] = a1; ap[2] = a2;
  }
  const uint64_t counter = policy_step_counter(a, e, t);
  float reward;
  bool done, succ;
  wrapped_step<1, GENERAL>(a.k, i, counter, L, g, a0, a1, a2, o, reward, done, succ);
  if (a.k.out.obs) store_obs<1>(a.k.out.obs + row * 12, o);
  if (a.k.out.reward) a.k.out.reward[row] = reward;
  if (a.k.out.done) a.k.out.done[row] = done;
  if (a.k.out.success) a.k.out.success[row] = succ;
}

#ifdef EARL_HOST_BUILD
// ------------------------------------------------------------------------------------------------
// host twin: the MLP as the plain loops of the contract, one env at a time
// ------------------------------------------------------------------------------------------------
inline void mlp_layers(const earl_mlp_policy& p, const float (&x)[12], float* act, int last_act) {
  float h[2][kPolicyMaxWidth];
  const float* in = x;
  const float* w = p.params;
  for (int l = 0; l < p.n_layers; ++l) {
    const int K = p.dims[l], N = p.dims[l + 1];
    const float* b = w + (size_t)N * K;
    const int kind = l + 1 < p.n_layers ? p.hidden_act : last_act;
    float* dst = l + 1 < p.n_layers ? h[l & 1] : act;
    for (int j = 0; j < N; ++j) {
      float acc = b[j];
      for (int k = 0; k < K; ++k) acc = fmaf(in[k], w[(size_t)j * K + k], acc);
      dst[j] = policy_act(acc, kind);
    }
    in = dst;
    w = b + N;
  }
}
inline void mlp_forward(const earl_mlp_policy& p, const float (&x)[12], float (&act)[3]) { mlp_layers(p, x, act, p.out_act); }

template <bool GENERAL>
inline void policy_rollout_env(const PolicyArgs& a, int i) {
  Lane<1> L;
  load_lane<1>(a.k, i, L);
  float g[6], o[12];
  load_goal<1>(a.k.st.goal_table, L.goal_idx, g);
  for (int e = 0; e < a.episodes; ++e) {
    policy_episode_begin<GENERAL>(a, i, e, L, g, o);
    for (int t = 0; t < a.k.T; ++t) {
      float act[3];
      mlp_forward(a.p, o, act);
      policy_env_step<GENERAL>(a, i, e, t, L, g, act[0], act[1], act[2], o);
    }
  }
  store_lane<1>(a.k, i, L);
}

// the Gaussian head: the 6-wide last layer without activation, then the contract's head per dimension
template <bool GENERAL>
inline void gaussian_rollout_env(const GaussianPolicyArgs& a, int i) {
  Lane<1> L;
  load_lane<1>(a.k, i, L);
  float g[6], o[12];
  load_goal<1>(a.k.st.goal_table, L.goal_idx, g);
  for (int e = 0; e < a.episodes; ++e) {
    policy_episode_begin<GENERAL>(a, i, e, L, g, o);
    for (int t = 0; t < a.k.T; ++t) {
      float y[6], act[3];
      mlp_layers(a.p, o, y, EARL_ACT_NONE);
      const U4 b = draw_block(a.k.cfg, policy_step_counter(a, e, t), i, kGaussDraw);
      const uint32_t word[3] = {b.x, b.y, b.z};
      const size_t row = ((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)i;
      for (int d = 0; d < 3; ++d) {
        const float eps = normal_quantile_f32(word[d] >> 8);
        act[d] = gaussian_head_action(a.head, a.p.out_act, y[d], y[3 + d], eps);
        if (a.head.eps_out) a.head.eps_out[row * 3 + d] = eps;
      }
      policy_env_step<GENERAL>(a, i, e, t, L, g, act[0], act[1], act[2], o);
    }
  }
  store_lane<1>(a.k, i, L);
}

#else
// ------------------------------------------------------------------------------------------------
// gfx950 kernel.  One workgroup = 16 envs (the M of v_mfma_f32_16x16x4_f32) x four waves.
//   env step        lanes 0..15 of wave 0, one lane per env, state in registers for the whole launch (as rollout_body)
//   layer 0         12 -> H1:  A = the 16 observation rows (LDS), B = W0 tiles in registers; N-tile `tl` belongs to wave tl & 3
//   hidden layer    H1 -> H2 (NT2 > 0 only): A = the 16 x H1 activations (LDS), B = the wave's NT2 tiles of W1 in registers, H1 / 4 k-steps per tile, the
//                   tiles of a wave interleaved so that consecutive MFMAs do not depend on one another
//   output layer    Hlast -> 3 (padded to one 16-wide tile) on wave 0: ONE accumulator, Hlast / 4 dependent MFMAs -- the serial part
// Weights are loaded ONCE, in the B-operand lane map (lane l of k-step s holds B[k = 4 s + (l >> 4)][j = l & 15] = W[n0 + j][k]); every register
// array is indexed by unrolled constants only.  The A operand of k-step s is A[i = l & 15][k = 4 s + (l >> 4)]: activations are kept in LDS as
// [row][k & 3][k >> 2] so that a lane's operands of four consecutive k-steps are one 16-byte read.  C/D: column l & 15, rows 4 (l >> 4) + r.
// K is never padded (12 and the hidden widths are multiples of 4); only the output's N = 3 is (zero columns, results dropped).
// ------------------------------------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kPolX = 0;                                             // LDS floats: observation rows [16][12]
constexpr int kPolH1 = 16 * 12;                                      // hidden activations [16][H1]
constexpr int kPolH2 = kPolH1 + 16 * kPolicyMaxWidth;                // [16][H2]
constexpr int kPolAct = kPolH2 + 16 * kPolicyMaxWidth;               // actions [16][4]
constexpr int kPolWo = kPolAct + 16 * 4;                              // output-layer weights [3][4][HL / 4] (the NT2 = 4 instantiation only)
constexpr int kPolLds = kPolWo + 3 * kPolicyMaxWidth;
// with a Gaussian head (GAUSS): the output tile has 6 live columns, the action rows are [16][8] (0..2 mean -> action, 3..5 raw log_std) and the
// output-layer weights, where they live in LDS, are [6][4][HL / 4]
constexpr int kPolWoG = kPolAct + 16 * 8;
constexpr int kPolEpsG = kPolWoG + 6 * kPolicyMaxWidth;            // the step's draws [16][4]
constexpr int kPolLdsG = kPolEpsG + 16 * 4;

// EARL_POLICY_STAMPS = diagnostic build only (tools/build_policy_stamped.sh, tools/prof_policy.py; never in libearl_hip.so): s_memtime stamps of wave 0 of
// workgroup 0 at the end of each phase of a step, summed over the launch: [0] observation -> LDS + barrier, [1] layer 0 + barrier, [2] hidden layer +
// barrier, [3] output layer + barrier (GAUSS: wave 1 makes the step's draws meanwhile), [4] env step (action read, tanh, wrapped_step, stores), [5] GAUSS only:
// the head on lanes 0..47 of wave 0 + the wavefront fence.  Each unit that instantiates the kernel has its own copy of the sums and its own reader
// (earl_debug_read_policy_profile: 5 words; earl_debug_read_policy_gaussian_profile: 6).
#ifdef EARL_POLICY_STAMPS
static __device__ unsigned long long g_policy_prof[8];
__device__ __forceinline__ unsigned long long pol_clock() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define POL_STAMP(k) do { const unsigned long long now_ = pol_clock(); prof[k] += now_ - last_; last_ = now_; } while (0)
#else
#define POL_STAMP(k)
#endif

// where element (row, k) of a [16][K] activation image lives
__device__ __forceinline__ int pol_idx(int row, int k, int K) { return row * K + (k & 3) * (K >> 2) + (k >> 2); }

// GAUSS (tabletop_policy_gaussian.hip only): the head runs one lane per (env, dimension), lane 16 d + env of a wave's lanes 0..47.
//   draws   wave 1, WHILE wave 0 runs the output layer (the draw depends on the step's counter only, not on the network): the Philox block of the step,
//           eps = normal_quantile_f32, eps -> LDS and eps_out.  The output layer's barrier publishes it.
//   head    wave 0, after that barrier: log_std map, sigma, u, out_act; the action is written over the mean in the action row, and the env lanes, same
//           wave, read the row after a wavefront fence.  No workgroup barrier is added, and the three serial tanh_f32 leave the env lane.
template <int NT2, bool GENERAL, bool GAUSS = false>
__global__ __launch_bounds__(256) void policy_rollout_kernel(const typename PolicyArgsOf<GAUSS>::type a) {
  constexpr int NOUT = GAUSS ? 6 : 3, ACTW = GAUSS ? 8 : 4, WO_OFF = GAUSS ? kPolWoG : kPolWo;
  __shared__ __attribute__((aligned(16))) float lds[GAUSS ? kPolLdsG : kPolLds];
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int H1 = a.p.dims[1], HL = a.p.dims[a.p.n_layers - 1], H2 = NT2 > 0 ? a.p.dims[2] : 0;
  const float* __restrict__ W0 = a.p.params;
  const float* __restrict__ B0 = W0 + H1 * 12;
  const float* __restrict__ W1 = B0 + H1;
  const float* __restrict__ B1 = W1 + H2 * H1;
  const float* __restrict__ WO = NT2 > 0 ? B1 + H2 : W1;
  const float* __restrict__ BO = WO + NOUT * HL;

  // ---- prologue: weights into registers, once
  const int nt0 = (H1 / 16 - wave + 3) >> 2;                          // this wave's N-tiles of layer 0: tl = wave + 4 j, j < nt0
  float w0[4][3], b0[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = (wave + 4 * j) * 16 + c;
    const bool ok = j < nt0;
#pragma unroll
    for (int s = 0; s < 3; ++s) w0[j][s] = ok ? W0[n * 12 + 4 * s + q] : 0.0f;
    b0[j] = ok ? B0[n] : 0.0f;
  }
  constexpr int NT2A = NT2 > 0 ? NT2 : 1;
  const int nt1 = NT2 > 0 ? (H2 / 16 - wave + 3) >> 2 : 0;
  float w1[NT2A][64], b1[NT2A];
  if constexpr (NT2 > 0) {
#pragma unroll
    for (int j = 0; j < NT2; ++j) {
      const int n = (wave + 4 * j) * 16 + c;
      const bool ok = j < nt1;
#pragma unroll
      for (int s = 0; s < 64; ++s) w1[j][s] = (ok && 4 * s < H1) ? W1[n * H1 + 4 * s + q] : 0.0f;
      b1[j] = ok ? B1[n] : 0.0f;
    }
  }
  // the output layer's B operand: registers too, except beside a 256-wide second hidden layer (NT2 = 4), whose 256 weight registers per lane leave no
  // room for 64 more -- there it stays in LDS in the order a lane reads it (3 KB, one 16-byte read per four k-steps, independent of the MFMA chain)
  constexpr bool WO_LDS = GAUSS ? NT2 >= 3 : NT2 == 4;                  // (the Gaussian head's own registers: from NT2 = 3 on)
  float wo[WO_LDS ? 1 : 64], bo;
  if constexpr (WO_LDS) {
    for (int k = (int)threadIdx.x; k < NOUT * HL; k += 256) {
      const int j = k / HL, kk = k - j * HL;
      lds[WO_OFF + (j * 4 + (kk & 3)) * (HL >> 2) + (kk >> 2)] = WO[k];
    }
    wo[0] = 0.0f;
  } else {
#pragma unroll
    for (int s = 0; s < 64; ++s) wo[s] = (wave == 0 && c < NOUT && 4 * s < HL) ? WO[c * HL + 4 * s + q] : 0.0f;
  }
  bo = c < NOUT ? BO[c] : 0.0f;

  // ---- env lanes
  const int i = blockIdx.x * kPolicyEnvsPerWg + (int)threadIdx.x;
  const bool env_lane = threadIdx.x < kPolicyEnvsPerWg && i < a.k.cfg.n;
  Lane<1> L;
  float g[6], o[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = 0.0f;
  if (env_lane) {
    load_lane<1>(a.k, i, L);
    load_goal<1>(a.k.st.goal_table, L.goal_idx, g);
  }
  float* const X = lds + kPolX;
  float* const A1 = lds + kPolH1;
  float* const A2 = lds + kPolH2;
  float* const AL = NT2 > 0 ? A2 : A1;
  float* const ACT = lds + kPolAct;

#ifdef EARL_POLICY_STAMPS
  unsigned long long prof[6] = {0, 0, 0, 0, 0, 0}, last_ = 0;
#endif
  for (int e = 0; e < a.episodes; ++e) {
    if (env_lane) policy_episode_begin<GENERAL>(a, i, e, L, g, o);
#ifdef EARL_POLICY_STAMPS
    last_ = pol_clock();
#endif
    for (int t = 0; t < a.k.T; ++t) {
      if (threadIdx.x < kPolicyEnvsPerWg) {                           // (rows of a ragged last workgroup: zeros, results never read)
#pragma unroll
        for (int k = 0; k < 12; ++k) X[pol_idx((int)threadIdx.x, k, 12)] = o[k];
      }
      __syncthreads();
      POL_STAMP(0);
      // ---- layer 0: 12 -> H1
      {
        float xa[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) xa[s] = X[c * 12 + q * 3 + s];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < nt0) {
            f32x4 acc = {b0[j], b0[j], b0[j], b0[j]};
#pragma unroll
            for (int s = 0; s < 3; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], w0[j][s], acc, 0, 0, 0);
            const int n = (wave + 4 * j) * 16 + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) A1[pol_idx(q * 4 + r, n, H1)] = policy_act(acc[r], a.p.hidden_act);
          }
        }
      }
      __syncthreads();
      POL_STAMP(1);
      // ---- hidden layer: H1 -> H2
      if constexpr (NT2 > 0) {
        f32x4 acc[NT2];
#pragma unroll
        for (int j = 0; j < NT2; ++j) acc[j] = f32x4{b1[j], b1[j], b1[j], b1[j]};
        if (nt1 > 0) {
          const float* arow = A1 + c * H1 + q * (H1 >> 2);
#pragma unroll
          for (int s4 = 0; s4 < 16; ++s4) {
            if (s4 * 16 < H1) {
              const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * s4);
#pragma unroll
              for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int j = 0; j < NT2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], w1[j][4 * s4 + s], acc[j], 0, 0, 0);
              }
            }
          }
#pragma unroll
          for (int j = 0; j < NT2; ++j) {
            if (j < nt1) {
              const int n = (wave + 4 * j) * 16 + c;
#pragma unroll
              for (int r = 0; r < 4; ++r) A2[pol_idx(q * 4 + r, n, H2)] = policy_act(acc[j][r], a.p.hidden_act);
            }
          }
        }
        __syncthreads();
      }
      POL_STAMP(2);
      if constexpr (GAUSS) {
        // ---- the step's draws on wave 1, beside the output layer: lane = (env, dimension)
        if (wave == 1 && lane < 3 * kPolicyEnvsPerWg) {
          const int is = blockIdx.x * kPolicyEnvsPerWg + c;             // (q = the dimension)
          const U4 b = draw_block(a.k.cfg, policy_step_counter(a, e, t), is, kGaussDraw);
          const float eps = normal_quantile_f32((q == 0 ? b.x : (q == 1 ? b.y : b.z)) >> 8);
          lds[kPolEpsG + c * 4 + q] = eps;
          if (a.head.eps_out && is < a.k.cfg.n) a.head.eps_out[(((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)is) * 3 + q] = eps;
        }
      }
      // ---- output layer on wave 0: one accumulator, HL / 4 dependent MFMAs
      if (wave == 0) {
        f32x4 acc = {bo, bo, bo, bo};
        const float* arow = AL + c * HL + q * (HL >> 2);
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) {
          if (s4 * 16 < HL) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * s4);
            if constexpr (WO_LDS) {
              f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
              if (c < NOUT) bv = *reinterpret_cast<const f32x4*>(lds + WO_OFF + (c * 4 + q) * (HL >> 2) + 4 * s4);
#pragma unroll
              for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
            } else {
#pragma unroll
              for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], wo[4 * s4 + s], acc, 0, 0, 0);
            }
          }
        }
        if (c < NOUT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) ACT[(q * 4 + r) * ACTW + c] = acc[r];
        }
      }
      __syncthreads();
      POL_STAMP(3);
      if constexpr (GAUSS) {
        // ---- the head, one lane per (env, dimension): lanes 0..47 of wave 0
        if (threadIdx.x < 3 * kPolicyEnvsPerWg) {
          const float act = gaussian_head_action(a.head, a.p.out_act, ACT[c * ACTW + q], ACT[c * ACTW + 3 + q], lds[kPolEpsG + c * 4 + q]);
          ACT[c * ACTW + q] = act;
        }
        if (wave == 0) {                                                // the env lanes are lanes of this wave: a wavefront fence, no workgroup barrier
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
        POL_STAMP(5);
      }
      // ---- env step, one lane per env
      if (env_lane) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ACT + (int)threadIdx.x * ACTW);
        float a0 = av[0], a1 = av[1], a2 = av[2];
        if constexpr (!GAUSS) {
          a0 = policy_act(a0, a.p.out_act); a1 = policy_act(a1, a.p.out_act); a2 = policy_act(a2, a.p.out_act);
        }
        policy_env_step<GENERAL>(a, i, e, t, L, g, a0, a1, a2, o);
      }
      POL_STAMP(4);
    }
  }
#ifdef EARL_POLICY_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) g_policy_prof[k] = prof[k];
  }
#endif
  if (env_lane) store_lane<1>(a.k, i, L);
}
#endif  // EARL_HOST_BUILD

}  // namespace earl

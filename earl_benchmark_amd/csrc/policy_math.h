// policy_math.h -- the arithmetic of the in-kernel policies, stated once for every unit that evaluates one: the activations (relu_f32, tanh_f32), the Gaussian
// head (exp_f32, normal_quantile_f32, the log-std maps, gaussian_head_action) and the draw index of its Philox stream.  Included by tabletop_policy.h (the tabletop
// kernels and their host twin), by physics_env_sawyer.h (the Sawyer door / peg rollout with a policy) and by physics_env_minitaur.h (the minitaur's): it needs the ABI structs and nothing of any env.
// Every function body states `fp contract(off)` itself: the tabletop units are compiled with -ffp-contract=off anyway, the stepper units run under
// `fp contract(fast)` (physics_stepper.h), and these functions are a bit-exact contract in both.
#pragma once
#include "earl_rt.h"

#include <cstdint>

#include "../../include/earl_tabletop.h"

namespace earl {

constexpr int kPolicyMaxWidth = 256;   // hidden widths: multiples of 16 in 16 .. 256

// ------------------------------------------------------------------------------------------------
// tanh_f32: float32 in, float32 out, evaluated in fp64 out of fma, +, *, the correctly rounded / and integer operations only (no libm / ocml call), and
// rounded to float32 ONCE -- host and device agree bit for bit, and the single rounding of a 1e-15-accurate value is what makes it odd, monotone over
// every float32 and within 0.5 ulp (+ 1e-8) of tanh (tests/test_policy_rollout.py sweeps every float32 in 2^-12 <= |x| <= 16 on the host;
// tests/test_policy_math_gpu.py sweeps the same range on the device, in the tabletop units' context and under the stepper's contract(fast): device == host).
//   |x| <  2^-6 : x + x z (-1/3 + z (2/15 + z (-17/315 + z 62/2835))), z = x^2                 (next term 1382/155925 z^5 < 1e-20 relative)
//   |x| <  10   : t = exp(-2|x|) = 2^k e^r, k = round(-2|x| log2 e), r in two Cody-Waite steps, e^r by its Taylor series to r^12 / 12!
//                 (|r| <= 0.35: remainder 3e-16); tanh = (1 - t) / (1 + t)
//   |x| >= 10   : 1 (1 - tanh(10) = 4e-9 < 2^-25), +-Inf included;  NaN -> NaN;  the sign is copied from x, so +-0 -> +-0
// ------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ float tanh_f32(float x) {
#pragma clang fp contract(off)
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
#pragma clang fp contract(off)
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
// libm / ocml call): host and device agree bit for bit (tests/test_policy_gaussian.py sweeps all 2^24 quantile inputs and every float32 of [-20, 4] on the
// host against double; tests/test_policy_math_gpu.py runs the same sweeps and 2^20 rows of gaussian_head_action per mode / map / bounds on the device in both
// compile contexts and holds them to the host's bits).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kGaussDraw = 0x504F4C00u;

// exp_f32: float32 in, float32 out; tanh_f32's exp (k = round(x log2 e), two Cody-Waite steps, Taylor series to r^12 / 12!, |r| <= 0.35) in fp64, rounded to
// float32 ONCE: within 0.5 ulp (+ 1e-8).  NaN -> NaN, x >= 89 -> +Inf, x <= -104 -> +0; the log_std bounds keep the argument inside [-20, 4].
__host__ __device__ __forceinline__ float exp_f32(float x) {
#pragma clang fp contract(off)
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
#pragma clang fp contract(off)
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
#pragma clang fp contract(off)
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

}  // namespace earl

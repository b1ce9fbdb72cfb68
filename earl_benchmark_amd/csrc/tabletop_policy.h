// tabletop_policy.h -- the closed-loop tabletop rollout: a float32 MLP policy 12 -> hidden (-> hidden) -> 3 evaluated between the env steps of ONE
// launch (include/earl_tabletop.h: earl_tabletop_policy_rollout).  Shared by the gfx950 kernel (tabletop_policy.hip) and its host twin
// (tabletop_host.cpp, -DEARL_HOST_BUILD); the per-env step is tabletop_step.h's wrapped_step<1, GENERAL>, not restated here.
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
// arguments
// ------------------------------------------------------------------------------------------------
struct PolicyArgs {
  KArgs k;              // cfg / state / outputs / thresholds; k.T = steps per episode; k.act unused
  earl_mlp_policy p;
  float* act_out;
  int32_t episodes;
  int32_t reset_first;
};

namespace hostside {

inline int check_policy(const earl_tabletop_cfg* cfg, const earl_tabletop_state* st, const earl_mlp_policy* p, int32_t episodes, int32_t T,
                        int32_t reset_first, const earl_tabletop_out* out) {
  if (int rc = check_common(cfg, st, 1)) return rc;
  if (!p || !out) return fail(EARL_ERR_ARG, "policy/out is NULL");
  if (!p->params) return fail(EARL_ERR_ARG, "policy params is NULL");
  if (p->precision != 0) return fail(EARL_ERR_ARG, "policy precision = %d: only 0 (fp32) exists", p->precision);
  if (p->n_layers != 2 && p->n_layers != 3) return fail(EARL_ERR_ARG, "policy n_layers = %d: 2 (one hidden layer) or 3 (two)", p->n_layers);
  if (p->dims[0] != EARL_TABLETOP_OBS_DIM || p->dims[p->n_layers] != EARL_TABLETOP_ACT_DIM)
    return fail(EARL_ERR_ARG, "policy dims: input %d, output %d (want 12 and 3)", p->dims[0], p->dims[p->n_layers]);
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

// one closed-loop step of one env given the policy's action (a0, a1, a2): act_out, wrapped_step, outputs
template <bool GENERAL>
__device__ __forceinline__ void policy_env_step(const PolicyArgs& a, int i, int e, int t, Lane<1>& L, float (&g)[6], float a0, float a1, float a2, float (&o)[12]) {
  const size_t row = ((size_t)e * (size_t)a.k.T + (size_t)t) * (size_t)a.k.cfg.n + (size_t)i;
  if (a.act_out) {
    float* ap = a.act_out + row * 3;
    ap[0] = a0; ap[1] = a1; ap[2] = a2;
  }
  const uint64_t counter = a.k.cfg.counter + (uint64_t)e * (uint64_t)(a.k.T + 1) + (uint64_t)(a.reset_first ? 1 : 0) + (uint64_t)t;
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
inline void mlp_forward(const earl_mlp_policy& p, const float (&x)[12], float (&act)[3]) {
  float h[2][kPolicyMaxWidth];
  const float* in = x;
  const float* w = p.params;
  for (int l = 0; l < p.n_layers; ++l) {
    const int K = p.dims[l], N = p.dims[l + 1];
    const float* b = w + (size_t)N * K;
    const int kind = l + 1 < p.n_layers ? p.hidden_act : p.out_act;
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

// EARL_POLICY_STAMPS = diagnostic build only (tools/build_policy_stamped.sh, tools/prof_policy.py; never in libearl_hip.so): s_memtime stamps of wave 0 of
// workgroup 0 at the end of each phase of a step, summed over the launch: [0] observation -> LDS + barrier, [1] layer 0 + barrier, [2] hidden layer +
// barrier, [3] output layer + barrier, [4] env step (action read, tanh, wrapped_step, stores)
#ifdef EARL_POLICY_STAMPS
__device__ unsigned long long g_policy_prof[8];
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

template <int NT2, bool GENERAL>
__global__ __launch_bounds__(256) void policy_rollout_kernel(const PolicyArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kPolLds];
  const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int H1 = a.p.dims[1], HL = a.p.dims[a.p.n_layers - 1], H2 = NT2 > 0 ? a.p.dims[2] : 0;
  const float* __restrict__ W0 = a.p.params;
  const float* __restrict__ B0 = W0 + H1 * 12;
  const float* __restrict__ W1 = B0 + H1;
  const float* __restrict__ B1 = W1 + H2 * H1;
  const float* __restrict__ WO = NT2 > 0 ? B1 + H2 : W1;
  const float* __restrict__ BO = WO + 3 * HL;

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
  constexpr bool WO_LDS = NT2 == 4;
  float wo[WO_LDS ? 1 : 64], bo;
  if constexpr (WO_LDS) {
    for (int k = (int)threadIdx.x; k < 3 * HL; k += 256) {
      const int j = k / HL, kk = k - j * HL;
      lds[kPolWo + (j * 4 + (kk & 3)) * (HL >> 2) + (kk >> 2)] = WO[k];
    }
    wo[0] = 0.0f;
  } else {
#pragma unroll
    for (int s = 0; s < 64; ++s) wo[s] = (wave == 0 && c < 3 && 4 * s < HL) ? WO[c * HL + 4 * s + q] : 0.0f;
  }
  bo = c < 3 ? BO[c] : 0.0f;

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
  unsigned long long prof[5] = {0, 0, 0, 0, 0}, last_ = 0;
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
              if (c < 3) bv = *reinterpret_cast<const f32x4*>(lds + kPolWo + (c * 4 + q) * (HL >> 2) + 4 * s4);
#pragma unroll
              for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
            } else {
#pragma unroll
              for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], wo[4 * s4 + s], acc, 0, 0, 0);
            }
          }
        }
        if (c < 3) {
#pragma unroll
          for (int r = 0; r < 4; ++r) ACT[(q * 4 + r) * 4 + c] = acc[r];
        }
      }
      __syncthreads();
      POL_STAMP(3);
      // ---- env step, one lane per env
      if (env_lane) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ACT + (int)threadIdx.x * 4);
        const float a0 = policy_act(av[0], a.p.out_act), a1 = policy_act(av[1], a.p.out_act), a2 = policy_act(av[2], a.p.out_act);
        policy_env_step<GENERAL>(a, i, e, t, L, g, a0, a1, a2, o);
      }
      POL_STAMP(4);
    }
  }
#ifdef EARL_POLICY_STAMPS
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) g_policy_prof[k] = prof[k];
  }
#endif
  if (env_lane) store_lane<1>(a.k, i, L);
}
#endif  // EARL_HOST_BUILD

}  // namespace earl

// tabletop_value.h -- the discounted score with a learned terminal value of earl_tabletop[3]_plan_mppi_value / earl_tabletop[3]_mpc_rollout_value
// (include/earl_tabletop.h, "discounted MPPI with a terminal value"): what a lane that owns one (branch, env) adds to plan_score_body / mpc_score.  Shared by the
// gfx950 kernels (tabletop_plan_value.hip, tabletop_mpc_value.hip) and by the host twin (tabletop_host.cpp, the same text under -DEARL_HOST_BUILD).
//
// value_accumulate   ret += d_t * r_t;  d_{t+1} = d_t * gamma: three float64 roundings, no fused multiply-add.
// value_forward      V(o) on the lane's OWN observation row, in registers: the policy contract's chains
//                    (acc = b_j; k ascending: acc = fmaf(x_k, W_jk, acc); relu_f32 / tanh_f32 of policy_math.h) evaluated by the lane itself.  No LDS, no cross-lane
//                    traffic.  Every lane of a wave reads the SAME W_jk: the weights are addressed through the constant address space (EARL_VALUE_W), so a
//                    wave-uniform address becomes a scalar load (s_load_dword .. x16) and one fetch feeds 64 lanes; plain `const __restrict__` was not relied
//                    on: the MPC kernel stores to global memory before the network runs.  Four independent chains at a time
//                    (two in the streamed second layer, where the held layer leaves no room for more) share every x_k, as pol_layer's do.
//                    The output is ONE number, so the last hidden layer is streamed into it: h_j is activated and consumed at once by
//                    acc = fmaf(act(h_j), W_out_j, acc), j ascending -- the contract's order -- and never stored.  Only the FIRST hidden layer of a two-hidden-layer
//                    network is held: h1[kValueMaxH1] registers, written and read by constant indices only (the loops over it are unrolled in tiles of 16 behind
//                    wave-uniform guards `tile < H1`; written for any cap that is a multiple of 16 up to 64, though only 16 fits the MPC kernels' 128 VGPRs
//                    without scratch -- include/earl_tabletop.h, EARL_PLAN_VALUE_MAX_H1).
//                    The observation row is made AGAIN after the look-ahead loop (make_obs on the state the last step left, that step's auto-reset left out:
//                    tabletop_step.h) instead of being kept through it.
// value_terminal     ret += d_H * (double)V.
#pragma once
#include "policy_math.h"

namespace earl {

constexpr int kValueMaxH1 = EARL_PLAN_VALUE_MAX_H1;   // the widest first hidden layer of a two-hidden-layer value network (the register budget of tabletop_mpc_value.hip's kernels)

// what a `_value` launch carries beside the planner's block.  net.params == NULL: no terminal term
struct ValueArgs {
  double discount;
  earl_mlp_policy net;
};

#ifdef EARL_HOST_BUILD
#define EARL_VALUE_W
#else
#define EARL_VALUE_W __attribute__((address_space(4)))
#endif
typedef const EARL_VALUE_W float* value_wptr;

// d_t depends on t only, so it is the same in every lane of a wave: on the device it is handed back through the scalar registers (two v_readfirstlane), which
// keeps two vector registers free through the look-ahead loop and the network
__device__ __forceinline__ double value_uniform(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t b = __builtin_bit_cast(uint64_t, d);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
#else
  return d;
#endif
}

__device__ __forceinline__ void value_accumulate(double& ret, double& d, float reward, double gamma) {
#pragma clang fp contract(off)
  const double term = d * (double)reward;
  ret = ret + term;
  d = value_uniform(d * gamma);
}

// acc = fmaf(x, w, acc) with w a wave-uniform weight.  On the device the instruction is written out: left to itself the compiler pairs the four chains into packed
// two-wide multiply-adds and keeps every x_k TWICE (both halves of a 64-bit register pair), which doubles the registers of the held layer.  v_fmac_f32 is the fused
// multiply-add the builtin compiles to (one rounding), so the bits are the host's.
__device__ __forceinline__ float value_fma(float x, float w, float acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "s"(w), "v"(x));
  return acc;
#else
  return __builtin_fmaf(x, w, acc);
#endif
}

// four rows j .. j + 3 of a layer whose K inputs x are registers: r_c = b[j + c]; k ascending: r_c = fmaf(x[k0 + k], w[(j + c) * ld + k0 + k], r_c) for the tiles the caller names
template <int K0, int KN, int NX>
__device__ __forceinline__ void value_chains(const float (&x)[NX], value_wptr w0, value_wptr w1, value_wptr w2, value_wptr w3, float& r0, float& r1, float& r2, float& r3) {
#pragma unroll
  for (int k = K0; k < K0 + KN; ++k) {
    r0 = value_fma(x[k], w0[k], r0);
    r1 = value_fma(x[k], w1[k], r1);
    r2 = value_fma(x[k], w2[k], r2);
    r3 = value_fma(x[k], w3[k], r3);
  }
}

template <int K0, int KN, int NX>
__device__ __forceinline__ void value_chains2(const float (&x)[NX], value_wptr w0, value_wptr w1, float& r0, float& r1) {
#pragma unroll
  for (int k = K0; k < K0 + KN; ++k) {
    r0 = value_fma(x[k], w0[k], r0);
    r1 = value_fma(x[k], w1[k], r1);
  }
}

template <int NOBS>
__device__ __forceinline__ float value_forward(const earl_mlp_policy& net, const float (&x)[NOBS]) {
#pragma clang fp contract(off)
  const value_wptr W0 = (value_wptr)(uintptr_t)net.params;   // [H1][NOBS]
  const int H1 = net.dims[1], hact = net.hidden_act;
  const value_wptr b0 = W0 + (size_t)H1 * NOBS;
  if (net.n_layers == 2) {                            // NOBS -> H1 -> 1: nothing held
    const value_wptr Wo = b0 + H1;
    float acc = Wo[H1];
#pragma unroll 1
    for (int j = 0; j < H1; j += 4) {
      float r0 = b0[j], r1 = b0[j + 1], r2 = b0[j + 2], r3 = b0[j + 3];
      const value_wptr w = W0 + (size_t)j * NOBS;
      value_chains<0, NOBS>(x, w, w + NOBS, w + 2 * NOBS, w + 3 * NOBS, r0, r1, r2, r3);
      acc = __builtin_fmaf(policy_act(r0, hact), Wo[j], acc);
      acc = __builtin_fmaf(policy_act(r1, hact), Wo[j + 1], acc);
      acc = __builtin_fmaf(policy_act(r2, hact), Wo[j + 2], acc);
      acc = __builtin_fmaf(policy_act(r3, hact), Wo[j + 3], acc);
    }
    return policy_act(acc, net.out_act);
  }
  // NOBS -> H1 -> H2 -> 1: h1 held, the second hidden layer streamed
  // h1 is written tile by tile (16 outputs, the tiles unrolled behind wave-uniform guards); inside a tile the four passes of four chains rotate a 16-register
  // buffer by four, as pol_layer rotates its arrays, so that no register array is indexed by the runtime j.
  constexpr int M = kValueMaxH1;
  float h1[M];
#pragma unroll
  for (int jt = 0; jt < M; jt += 16) {
    float t[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) t[c] = 0.0f;
    if (jt < H1) {                                    // (wave-uniform)
#pragma unroll 1
      for (int j = jt; j < jt + 16; j += 4) {
        float r0 = b0[j], r1 = b0[j + 1], r2 = b0[j + 2], r3 = b0[j + 3];
        const value_wptr w = W0 + (size_t)j * NOBS;
        value_chains<0, NOBS>(x, w, w + NOBS, w + 2 * NOBS, w + 3 * NOBS, r0, r1, r2, r3);
#pragma unroll
        for (int c = 0; c < 12; ++c) t[c] = t[c + 4];
        t[12] = policy_act(r0, hact);
        t[13] = policy_act(r1, hact);
        t[14] = policy_act(r2, hact);
        t[15] = policy_act(r3, hact);
      }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) h1[jt + c] = t[c];   // (tiles past H1: zeros, never read)
  }
  const int H2 = net.dims[2];
  const value_wptr W1 = b0 + H1;                      // [H2][H1]
  const value_wptr b1 = W1 + (size_t)H2 * H1;
  const value_wptr Wo = b1 + H2;
  float acc = Wo[H2];
#pragma unroll 1
  for (int j = 0; j < H2; j += 2) {
    float r0 = b1[j], r1 = b1[j + 1];
    const value_wptr w0 = W1 + (size_t)j * H1, w1 = w0 + H1;
    static_assert(M % 16 == 0 && M >= 16 && M <= 64, "the tiles below: 16 k each, ascending, behind wave-uniform guards");
    value_chains2<0, 16>(h1, w0, w1, r0, r1);
    if constexpr (M > 16) if (H1 > 16) value_chains2<(M > 16 ? 16 : 0), 16>(h1, w0, w1, r0, r1);
    if constexpr (M > 32) if (H1 > 32) value_chains2<(M > 32 ? 32 : 0), 16>(h1, w0, w1, r0, r1);
    if constexpr (M > 48) if (H1 > 48) value_chains2<(M > 48 ? 48 : 0), 16>(h1, w0, w1, r0, r1);
    acc = __builtin_fmaf(policy_act(r0, hact), Wo[j], acc);
    acc = __builtin_fmaf(policy_act(r1, hact), Wo[j + 1], acc);
  }
  return policy_act(acc, net.out_act);
}

// the score of a branch whose look-ahead ended with the discount d = d_H and the observation row o
template <int NOBS>
__device__ __forceinline__ double value_terminal(const ValueArgs& v, const float (&o)[NOBS], double ret, double d) {
#pragma clang fp contract(off)
  if (!v.net.params) return ret;
  const double term = d * (double)value_forward<NOBS>(v.net, o);
  return ret + term;
}

}  // namespace earl

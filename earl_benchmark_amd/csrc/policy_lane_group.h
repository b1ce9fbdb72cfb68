// policy_lane_group.h -- one layer of the in-kernel float32 MLP evaluated by the W lanes that own an env (W = 16: the Sawyer door / peg, physics_env_sawyer.h; W = 32: the
// minitaur, physics_env_minitaur.h), under the contract of policy_math.h / tabletop_policy.h: acc = b_j; for k ascending: acc = fmaf(x_k, W_jk, acc).
// Included inside the anonymous namespace of the stepper units, after policy_math.h.
//
// No LDS (the stepper's workgroups leave none): a layer's activations live in registers, element k on lane k & (W - 1) of the env's group in register k / W, and x_k
// reaches the group's other lanes by a width-W __shfl (ds_bpermute_b32: the LDS crossbar, no allocation).  Lane `sub` owns outputs j = W i + sub.  One pass of
// pol_layer's outer loop carries FOUR of them (i = 4 g .. 4 g + 3): four independent fmaf chains per lane share every x_k, so a shuffle feeds four multiply-adds and the
// chains hide one another's latency.  Weights come from global memory (params is [N][K] row-major, as torch.nn.Linear.weight): a lane walks its own rows in 16-byte
// pieces, so every cache line it touches is used whole over consecutive loads, and the env groups of a wave read the same addresses (one fetch serves them).  The network
// sits in L2 (14 -> 256 -> 256 -> 4: 280 KB).
// Register arrays are indexed by constants only: instead of indexing by the (runtime) k-tile / output-group number the arrays are rotated by one tile per iteration.
// W = 16: K is a multiple of the group width whenever VEC is set.  W = 32: hidden widths are multiples of 16, not of 32, so the last k-tile of a row may be half full:
// its 16-byte pieces past K are skipped (they would belong to the next row, or lie past the parameters).
//
// The STORED format of the parameters is the unit's: float32, or -- in the units compiled with EARL_POLICY_BF16 (physics_bf16.hip, physics_w8_bf16.hip, physics_mt_bf16.hip,
// physics_kitchen_policy_bf16.hip: earl_mlp_policy.precision == EARL_PRECISION_BF16) -- bf16, two bytes per element.  A stored bf16 value u is the float32 with the bit
// pattern u << 16 (exact; subnormals, +-0 and +-inf as they are) and enters the same fmaf chains in the same k order, so such a launch returns the bits of the float32
// launch fed with the widened values.  A 16-byte piece then carries EIGHT consecutive k (element 2 i in the low half of word i, element 2 i + 1 in the high half): half
// the load instructions, lines and bytes per row.  Without the define everything below is the float32 text as it always was.
#pragma once

#define EARL_KARG __attribute__((address_space(4)))

#ifdef EARL_POLICY_BF16
typedef uint16_t pol_elem;                              // one stored parameter
#define EARL_POL_WIDEN(u) __builtin_bit_cast(float, (uint32_t)(u) << 16)
#define EARL_POL_LO(word) __builtin_bit_cast(float, (uint32_t)(word) << 16)               // element 2 i of a piece's word i
#define EARL_POL_HI(word) __builtin_bit_cast(float, (uint32_t)(word) & 0xffff0000u)       // element 2 i + 1
#else
typedef float pol_elem;
#define EARL_POL_WIDEN(u) (u)
#endif

template <int W, bool VEC>
__device__ __forceinline__ void pol_layer(const pol_elem* __restrict__ Wt, const pol_elem* __restrict__ B, const int K, const int N, const int kind, const int sub,
                                          float (&h)[earl::kPolicyMaxWidth / W]) {
#pragma clang fp contract(off)
  static_assert(W == 16 || W == 32, "an env is owned by 16 or 32 lanes");
  constexpr int NR = earl::kPolicyMaxWidth / W;         // registers per lane that hold a layer's activations
  float out[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) out[i] = 0.f;
  constexpr int LG = W == 16 ? 4 : 5;                   // log2 W
  const int nt = (N + W - 1) >> LG, nk = (K + W - 1) >> LG;
#pragma unroll 1
  for (int g = 0; g < NR / 4; ++g) {
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
    if (4 * g < nt) {                                   // (wave-uniform)
      // rows past the layer's last one (a width that is not a multiple of 4 W; the narrow output layer) are clamped: computed on row N - 1 and never read
      const int j0 = min(4 * W * g + sub, N - 1), j1 = min(4 * W * g + W + sub, N - 1), j2 = min(4 * W * g + 2 * W + sub, N - 1), j3 = min(4 * W * g + 3 * W + sub, N - 1);
      const pol_elem* __restrict__ w0 = Wt + (size_t)j0 * K;
      const pol_elem* __restrict__ w1 = Wt + (size_t)j1 * K;
      const pol_elem* __restrict__ w2 = Wt + (size_t)j2 * K;
      const pol_elem* __restrict__ w3 = Wt + (size_t)j3 * K;
      r0 = EARL_POL_WIDEN(B[j0]); r1 = EARL_POL_WIDEN(B[j1]); r2 = EARL_POL_WIDEN(B[j2]); r3 = EARL_POL_WIDEN(B[j3]);
      float cur[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) cur[i] = h[i];
#pragma unroll 1
      for (int kt = 0; kt < nk; ++kt) {
        const float x = cur[0];
        if constexpr (VEC) {                            // K a multiple of 16, rows 16-byte aligned
#ifdef EARL_POLICY_BF16
#pragma unroll
          for (int kk = 0; kk < W; kk += 8) {               // two pieces per k-tile at W = 16, four at W = 32
            if (W > 16 && kk == 16 && W * kt + kk >= K) break;      // (wave-uniform; W = 32 only, as below)
            const uint4 v0 = *reinterpret_cast<const uint4*>(w0 + W * kt + kk), v1 = *reinterpret_cast<const uint4*>(w1 + W * kt + kk);
            const uint4 v2 = *reinterpret_cast<const uint4*>(w2 + W * kt + kk), v3 = *reinterpret_cast<const uint4*>(w3 + W * kt + kk);
            const float x0 = __shfl(x, kk, W), x1 = __shfl(x, kk + 1, W), x2 = __shfl(x, kk + 2, W), x3 = __shfl(x, kk + 3, W);
            const float x4 = __shfl(x, kk + 4, W), x5 = __shfl(x, kk + 5, W), x6 = __shfl(x, kk + 6, W), x7 = __shfl(x, kk + 7, W);
            r0 = __builtin_fmaf(x0, EARL_POL_LO(v0.x), r0); r1 = __builtin_fmaf(x0, EARL_POL_LO(v1.x), r1); r2 = __builtin_fmaf(x0, EARL_POL_LO(v2.x), r2); r3 = __builtin_fmaf(x0, EARL_POL_LO(v3.x), r3);
            r0 = __builtin_fmaf(x1, EARL_POL_HI(v0.x), r0); r1 = __builtin_fmaf(x1, EARL_POL_HI(v1.x), r1); r2 = __builtin_fmaf(x1, EARL_POL_HI(v2.x), r2); r3 = __builtin_fmaf(x1, EARL_POL_HI(v3.x), r3);
            r0 = __builtin_fmaf(x2, EARL_POL_LO(v0.y), r0); r1 = __builtin_fmaf(x2, EARL_POL_LO(v1.y), r1); r2 = __builtin_fmaf(x2, EARL_POL_LO(v2.y), r2); r3 = __builtin_fmaf(x2, EARL_POL_LO(v3.y), r3);
            r0 = __builtin_fmaf(x3, EARL_POL_HI(v0.y), r0); r1 = __builtin_fmaf(x3, EARL_POL_HI(v1.y), r1); r2 = __builtin_fmaf(x3, EARL_POL_HI(v2.y), r2); r3 = __builtin_fmaf(x3, EARL_POL_HI(v3.y), r3);
            r0 = __builtin_fmaf(x4, EARL_POL_LO(v0.z), r0); r1 = __builtin_fmaf(x4, EARL_POL_LO(v1.z), r1); r2 = __builtin_fmaf(x4, EARL_POL_LO(v2.z), r2); r3 = __builtin_fmaf(x4, EARL_POL_LO(v3.z), r3);
            r0 = __builtin_fmaf(x5, EARL_POL_HI(v0.z), r0); r1 = __builtin_fmaf(x5, EARL_POL_HI(v1.z), r1); r2 = __builtin_fmaf(x5, EARL_POL_HI(v2.z), r2); r3 = __builtin_fmaf(x5, EARL_POL_HI(v3.z), r3);
            r0 = __builtin_fmaf(x6, EARL_POL_LO(v0.w), r0); r1 = __builtin_fmaf(x6, EARL_POL_LO(v1.w), r1); r2 = __builtin_fmaf(x6, EARL_POL_LO(v2.w), r2); r3 = __builtin_fmaf(x6, EARL_POL_LO(v3.w), r3);
            r0 = __builtin_fmaf(x7, EARL_POL_HI(v0.w), r0); r1 = __builtin_fmaf(x7, EARL_POL_HI(v1.w), r1); r2 = __builtin_fmaf(x7, EARL_POL_HI(v2.w), r2); r3 = __builtin_fmaf(x7, EARL_POL_HI(v3.w), r3);
          }
#else
#pragma unroll
          for (int kk = 0; kk < W; kk += 4) {
            if (W > 16 && kk == 16 && W * kt + kk >= K) break;      // (wave-uniform; W = 32 only: K is a multiple of 16, so only the second half of a row's last tile can lie past it)
            const float4 v0 = *reinterpret_cast<const float4*>(w0 + W * kt + kk), v1 = *reinterpret_cast<const float4*>(w1 + W * kt + kk);
            const float4 v2 = *reinterpret_cast<const float4*>(w2 + W * kt + kk), v3 = *reinterpret_cast<const float4*>(w3 + W * kt + kk);
            const float x0 = __shfl(x, kk, W), x1 = __shfl(x, kk + 1, W), x2 = __shfl(x, kk + 2, W), x3 = __shfl(x, kk + 3, W);
            r0 = __builtin_fmaf(x0, v0.x, r0); r1 = __builtin_fmaf(x0, v1.x, r1); r2 = __builtin_fmaf(x0, v2.x, r2); r3 = __builtin_fmaf(x0, v3.x, r3);
            r0 = __builtin_fmaf(x1, v0.y, r0); r1 = __builtin_fmaf(x1, v1.y, r1); r2 = __builtin_fmaf(x1, v2.y, r2); r3 = __builtin_fmaf(x1, v3.y, r3);
            r0 = __builtin_fmaf(x2, v0.z, r0); r1 = __builtin_fmaf(x2, v1.z, r1); r2 = __builtin_fmaf(x2, v2.z, r2); r3 = __builtin_fmaf(x2, v3.z, r3);
            r0 = __builtin_fmaf(x3, v0.w, r0); r1 = __builtin_fmaf(x3, v1.w, r1); r2 = __builtin_fmaf(x3, v2.w, r2); r3 = __builtin_fmaf(x3, v3.w, r3);
          }
#endif
        } else {                                        // an input layer whose rows are no whole 16-byte pieces (the Sawyer's K = 14, the kitchen's K = 46: read element by element in either format)
#pragma unroll
          for (int kk = 0; kk < W; ++kk) {
            const int k = W * kt + kk;
            if (k < K) {                                // (wave-uniform)
              const float xk = __shfl(x, kk, W);
              r0 = __builtin_fmaf(xk, EARL_POL_WIDEN(w0[k]), r0); r1 = __builtin_fmaf(xk, EARL_POL_WIDEN(w1[k]), r1); r2 = __builtin_fmaf(xk, EARL_POL_WIDEN(w2[k]), r2); r3 = __builtin_fmaf(xk, EARL_POL_WIDEN(w3[k]), r3);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < NR - 1; ++i) cur[i] = cur[i + 1];
      }
      r0 = earl::policy_act(r0, kind); r1 = earl::policy_act(r1, kind); r2 = earl::policy_act(r2, kind); r3 = earl::policy_act(r3, kind);
    }
#pragma unroll
    for (int i = 0; i < NR - 4; ++i) out[i] = out[i + 4];   // after the NR / 4 passes group g's results stand at out[4 g .. 4 g + 3]
    out[NR - 4] = r0; out[NR - 3] = r1; out[NR - 2] = r2; out[NR - 1] = r3;
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) h[i] = out[i];
}

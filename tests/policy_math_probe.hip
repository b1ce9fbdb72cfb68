// policy_math_probe.hip -- test-only: the scalar functions of csrc/policy_math.h (tanh_f32, exp_f32, normal_quantile_f32, gaussian_head_action), one element per
// thread, behind extern "C" launchers that take raw device pointers, a count and a stream.  tests/policy_math_ref.py builds this file three ways:
//   hipcc, the Makefile's HIPFLAGS                           the tabletop units' context (-ffp-contract=off)              -> probe_*
//   hipcc, the same + -DEARL_PROBE_STEPPER_CONTEXT           `#pragma clang fp contract(fast)` at file scope BEFORE policy_math.h is included, the way
//                                                            physics_stepper.h precedes it in physics.hip / physics_w8.hip -> probe_*
//   g++ -x c++ -DEARL_HOST_BUILD, the host sweeps' flags     the host statement of the same header, OpenMP loops          -> fill_*
// The element functions below are shared by the three, so "device equals host" compares the same definition of every element.
#ifndef EARL_HOST_BUILD
#include <hip/hip_runtime.h>
#endif
#ifdef EARL_PROBE_STEPPER_CONTEXT
#pragma clang fp contract(fast)
#endif
#include "../earl_benchmark_amd/csrc/policy_math.h"

namespace {

// element i of a sweep: the i-th entry of `in`, or (in == NULL) the bit pattern / index first + i
__host__ __device__ __forceinline__ uint32_t probe_arg(const uint32_t* in, uint32_t first, long i) { return in ? in[i] : first + (uint32_t)i; }

__host__ __device__ __forceinline__ float probe_tanh_at(const uint32_t* in, uint32_t first, long i) {
  return earl::tanh_f32(__builtin_bit_cast(float, probe_arg(in, first, i)));
}
__host__ __device__ __forceinline__ float probe_exp_at(const uint32_t* in, uint32_t first, long i) {
  return earl::exp_f32(__builtin_bit_cast(float, probe_arg(in, first, i)));
}
__host__ __device__ __forceinline__ float probe_quantile_at(const uint32_t* in, uint32_t first, long i) {
  return earl::normal_quantile_f32(probe_arg(in, first, i));                 // (k < 2^24: the caller's)
}
// rows [n][3] = (mean, raw, eps)
__host__ __device__ __forceinline__ float probe_head_at(const earl_gaussian_head& h, int out_act, const float* rows, long i) {
  return earl::gaussian_head_action(h, out_act, rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]);
}

// NOT from the header: a multiply-add written in the unit itself, with no pragma of its own -- it shows which contraction mode the unit is compiled in
// (separately rounded in the plain build and on the host, fused under the stepper context)
__host__ __device__ __forceinline__ float probe_muladd_at(const float* rows, long i) { return rows[3 * i] * rows[3 * i + 1] + rows[3 * i + 2]; }

__host__ __device__ __forceinline__ earl_gaussian_head make_head(int mode, int log_std_map, float lo, float hi) {
  earl_gaussian_head h{};
  h.mode = mode;
  h.log_std_map = log_std_map;
  h.log_std_min = lo;
  h.log_std_max = hi;
  return h;
}

}  // namespace

#ifdef EARL_HOST_BUILD

extern "C" {
int probe_is_host() { return 1; }
void fill_tanh(const uint32_t* in, uint32_t first, float* out, long n) {
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) out[i] = probe_tanh_at(in, first, i);
}
void fill_exp(const uint32_t* in, uint32_t first, float* out, long n) {
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) out[i] = probe_exp_at(in, first, i);
}
void fill_quantile(const uint32_t* in, uint32_t first, float* out, long n) {
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) out[i] = probe_quantile_at(in, first, i);
}
void fill_head(int mode, int log_std_map, float lo, float hi, int out_act, const float* rows, float* out, long n) {
  const earl_gaussian_head h = make_head(mode, log_std_map, lo, hi);
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) out[i] = probe_head_at(h, out_act, rows, i);
}
void fill_muladd(const float* rows, float* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = probe_muladd_at(rows, i);
}
}  // extern "C"

#else

namespace {

constexpr int kProbeBlock = 256;
unsigned blocks_of(long n) { return (unsigned)((n + kProbeBlock - 1) / kProbeBlock); }

__global__ void k_tanh(const uint32_t* in, uint32_t first, float* out, long n) {
  const long i = (long)blockIdx.x * kProbeBlock + threadIdx.x;
  if (i < n) out[i] = probe_tanh_at(in, first, i);
}
__global__ void k_exp(const uint32_t* in, uint32_t first, float* out, long n) {
  const long i = (long)blockIdx.x * kProbeBlock + threadIdx.x;
  if (i < n) out[i] = probe_exp_at(in, first, i);
}
__global__ void k_quantile(const uint32_t* in, uint32_t first, float* out, long n) {
  const long i = (long)blockIdx.x * kProbeBlock + threadIdx.x;
  if (i < n) out[i] = probe_quantile_at(in, first, i);
}
__global__ void k_head(earl_gaussian_head h, int out_act, const float* rows, float* out, long n) {
  const long i = (long)blockIdx.x * kProbeBlock + threadIdx.x;
  if (i < n) out[i] = probe_head_at(h, out_act, rows, i);
}

__global__ void k_muladd(const float* rows, float* out, long n) {
  const long i = (long)blockIdx.x * kProbeBlock + threadIdx.x;
  if (i < n) out[i] = probe_muladd_at(rows, i);
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

}  // namespace

extern "C" {
int probe_is_host() { return 0; }
int probe_stepper_context() {
#ifdef EARL_PROBE_STEPPER_CONTEXT
  return 1;
#else
  return 0;
#endif
}
// every launcher: n in [1, 2^30]; out [n]; `in` [n] or NULL; -1 on a bad argument or a failed launch
int probe_tanh(const uint32_t* in, uint32_t first, float* out, long n, hipStream_t st) {
  if (!out || n <= 0 || n > (1L << 30)) return -1;
  hipLaunchKernelGGL(k_tanh, dim3(blocks_of(n)), dim3(kProbeBlock), 0, st, in, first, out, n);
  return launched();
}
int probe_exp(const uint32_t* in, uint32_t first, float* out, long n, hipStream_t st) {
  if (!out || n <= 0 || n > (1L << 30)) return -1;
  hipLaunchKernelGGL(k_exp, dim3(blocks_of(n)), dim3(kProbeBlock), 0, st, in, first, out, n);
  return launched();
}
int probe_quantile(const uint32_t* in, uint32_t first, float* out, long n, hipStream_t st) {
  if (!out || n <= 0 || n > (1L << 30)) return -1;
  hipLaunchKernelGGL(k_quantile, dim3(blocks_of(n)), dim3(kProbeBlock), 0, st, in, first, out, n);
  return launched();
}
int probe_head(int mode, int log_std_map, float lo, float hi, int out_act, const float* rows, float* out, long n, hipStream_t st) {
  if (!rows || !out || n <= 0 || n > (1L << 30)) return -1;
  hipLaunchKernelGGL(k_head, dim3(blocks_of(n)), dim3(kProbeBlock), 0, st, make_head(mode, log_std_map, lo, hi), out_act, rows, out, n);
  return launched();
}
int probe_muladd(const float* rows, float* out, long n, hipStream_t st) {
  if (!rows || !out || n <= 0 || n > (1L << 30)) return -1;
  hipLaunchKernelGGL(k_muladd, dim3(blocks_of(n)), dim3(kProbeBlock), 0, st, rows, out, n);
  return launched();
}
}  // extern "C"

#endif

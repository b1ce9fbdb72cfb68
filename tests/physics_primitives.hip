// physics_primitives.hip -- TEST INFRASTRUCTURE ONLY (tests/test_physics_primitives_gpu.py builds it on demand; nothing here is part of libearl_hip.so).
//
// One small kernel per numeric building block of the articulated-body stepper (csrc/physics_math.h, physics_scan.h, physics_solve.h, physics_lds.h and the
// top of minitaur_stepper.h), each calling the primitive THE WAY THE PRODUCT'S CALL SITE DOES: the template arguments the product instantiates, the lane layout
// (16 lanes per env and four envs per wave for nv <= 16, 32 lanes and two envs per wave for nv 22 / 23), the l / isl / ltri / grp conventions for the lanes
// beyond NV, matrices in SymLds<NV> in LDS (packed or square as SymLds<NV>::PACKED says), the diagonal term as dl[] / the diag functor.  Compiled with exactly the
// product's HIPFLAGS (csrc/Makefile); the stepper header's `#pragma clang fp contract(fast)` stays in force as in the five stepper units.  Built twice: as it is,
// and with -DEARL_DOOR_PACKED=1 (the storage layout of the door's eight-wave build, physics_w8.hip).
//
// Every launcher takes raw device pointers, a count and a stream and returns hipGetLastError().  Workgroups are ONE wavefront (64 threads).
#include "../earl_benchmark_amd/csrc/minitaur_device.h"
#include "../earl_benchmark_amd/csrc/physics_stepper.h"

namespace {
#include "../earl_benchmark_amd/csrc/minitaur_stepper.h"

// ------------------------------------------------------------------ A / B / C / F: elementwise, one thread per input row
enum { U_RCP_NR, U_RSQ_NR, U_RSQ2 };
template <int OP>
__global__ __launch_bounds__(64) void k_unary(const double* __restrict__ x, double* __restrict__ y, const long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  y[i] = OP == U_RCP_NR ? rcp_nr(x[i]) : (OP == U_RSQ_NR ? rsq_nr(x[i]) : rsq2(x[i]));
}
template <bool KC>
__global__ __launch_bounds__(64) void k_sincos(const double* __restrict__ x, double* __restrict__ sn, double* __restrict__ cs, const long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double s_, c_;
  if constexpr (KC) sincos_kc(x[i], s_, c_); else sincos_mod(x[i], s_, c_);
  sn[i] = s_; cs[i] = c_;
}
// in: rows of 9 = solref (2), solimp (5), r, dt.  out: rows of 7 = kb_of (k, b), kbimp (k, b, d), imp_of, imp_p2
__global__ __launch_bounds__(64) void k_impedance(const double* __restrict__ in, double* __restrict__ out, const long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double row[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) row[e] = in[i * 9 + e];
  double k0, b0, k1, b1, d1;
  kb_of(row, row + 2, row[8], k0, b0);
  kbimp(row, row + 2, row[7], row[8], k1, b1, d1);
  double* o = out + i * 7;
  o[0] = k0; o[1] = b0; o[2] = k1; o[3] = b1; o[4] = d1; o[5] = imp_of(row + 2, row[7]); o[6] = imp_p2(row + 2, row[7]);
}
// in: rows of 8 = w (5), j (3).  out: rows of 6 = cone_apply<false>, cone_apply<true>
__global__ __launch_bounds__(64) void k_cone_apply(const double* __restrict__ in, double* __restrict__ out, const long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double w[5];
#pragma unroll
  for (int e = 0; e < 5; ++e) w[e] = in[i * 8 + e];
  const double j0 = in[i * 8 + 5], j1 = in[i * 8 + 6], j2 = in[i * 8 + 7];
  double* o = out + i * 6;
  cone_apply<false>(w, j0, j1, j2, o[0], o[1], o[2]);
  cone_apply<true>(w, j0, j1, j2, o[3], o[4], o[5]);
}
// in: rows of 4 = r0, r1, r2, mu
__global__ __launch_bounds__(64) void k_cone_zone(const double* __restrict__ in, int* __restrict__ out, const long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  out[i] = cone_zone(in[i * 4], in[i * 4 + 1], in[i * 4 + 2], in[i * 4 + 3]);
}
// in: rows of 24 = qa (4), qb (4), v (3), w (3), I10 (10).  out: rows of 36 = qmul(qa, qb) (4), R = qmat(qa) (9), mulv(R, v) (3), mulvT(R, v) (3), cross(v, w) (3),
// iapply(I10, w, v) -> n, f (6), selv(i & 1, v, w) (3), selq(i & 1, qa, qb) (4), pick3(v, i % 3)
__global__ __launch_bounds__(64) void k_algebra(const double* __restrict__ in, double* __restrict__ out, const long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double* r = in + i * 24;
  const Q4 qa = ldq(r), qb = ldq(r + 4);
  const V3 v = ld3(r + 8), w = ld3(r + 11);
  double I[10];
#pragma unroll
  for (int e = 0; e < 10; ++e) I[e] = r[14 + e];
  double* o = out + i * 36;
  const Q4 qq = qmul(qa, qb);
  o[0] = qq.w; o[1] = qq.x; o[2] = qq.y; o[3] = qq.z;
  double R[3][3];
  qmat(qa, R);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) o[4 + 3 * a + b] = R[a][b];
  const V3 m0 = mulv(R, v), m1 = mulvT(R, v), cr = cross(v, w);
  o[13] = m0.x; o[14] = m0.y; o[15] = m0.z; o[16] = m1.x; o[17] = m1.y; o[18] = m1.z; o[19] = cr.x; o[20] = cr.y; o[21] = cr.z;
  V3 nn, ff;
  iapply(I, w, v, nn, ff);
  o[22] = nn.x; o[23] = nn.y; o[24] = nn.z; o[25] = ff.x; o[26] = ff.y; o[27] = ff.z;
  const V3 sv = selv((i & 1) != 0, v, w);
  const Q4 sq = selq((i & 1) != 0, qa, qb);
  o[28] = sv.x; o[29] = sv.y; o[30] = sv.z; o[31] = sq.w; o[32] = sq.x; o[33] = sq.y; o[34] = sq.z; o[35] = pick3(v, (int)(i % 3));
}

// ------------------------------------------------------------------ E: scans and lane moves, one wavefront = four 16-lane rows (= four envs)
// in / out: [lanes][6] = a (3), b (3) of every lane; sub = lane % LPE as in substep<NV, LPE> (nv 23: 32 lanes per env, the arm in lanes 0-8 of the env's first row)
template <int NV>
__global__ __launch_bounds__(64) void k_scan_anc(const double* __restrict__ in, double* __restrict__ out) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  const int sub = (threadIdx.x & 63) % Lim<NV>::LPE;
  V3 a = ld3(in + t * 6), b = ld3(in + t * 6 + 3);
  scan_anc<NV>(a, b, sub);
  double* o = out + t * 6;
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = b.x; o[4] = b.y; o[5] = b.z;
}
template <int NV, int N>
__global__ __launch_bounds__(64) void k_scan_desc(const double* __restrict__ in, double* __restrict__ out) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  const int sub = (threadIdx.x & 63) % Lim<NV>::LPE;
  double x[N];
#pragma unroll
  for (int e = 0; e < N; ++e) x[e] = in[t * N + e];
  scan_desc<NV, N>(x, sub);
#pragma unroll
  for (int e = 0; e < N; ++e) out[t * N + e] = x[e];
}
// in: [lanes]; out: [17][lanes] = dpp_row SHR 1 2 4, SHL 1 2 4; dpp_quad PARENT CHILD SWAP1 SWAP2 bcast 0-3; group_bcast 0 21 31
constexpr int N_MOVES = 17;
__global__ __launch_bounds__(64) void k_lane_moves(const double* __restrict__ in, double* __restrict__ out, const long lanes) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  const int grp = (threadIdx.x & 63) / 32;
  const double v = in[t];
  const double r[N_MOVES] = {dpp_row<DPP_SHR(1)>(v), dpp_row<DPP_SHR(2)>(v), dpp_row<DPP_SHR(4)>(v), dpp_row<DPP_SHL(1)>(v), dpp_row<DPP_SHL(2)>(v), dpp_row<DPP_SHL(4)>(v),
                             dpp_quad<QP_PARENT>(v), dpp_quad<QP_CHILD>(v), dpp_quad<QP_SWAP1>(v), dpp_quad<QP_SWAP2>(v),
                             dpp_quad<qp_bcast<0>()>(v), dpp_quad<qp_bcast<1>()>(v), dpp_quad<qp_bcast<2>()>(v), dpp_quad<qp_bcast<3>()>(v),
                             group_bcast<0>(v, grp), group_bcast<21>(v, grp), group_bcast<31>(v, grp)};
#pragma unroll
  for (int e = 0; e < N_MOVES; ++e) out[e * lanes + t] = r[e];
}

// ------------------------------------------------------------------ D: factorisations and solves
// Per-env LDS block: the Hessian, the diagonal term, the right-hand side, and the store the kitchen's helper wave leaves its factor in
template <int NV>
struct SolveBlk {
  SymLds<NV> H;
  double dl[NV], rc[NV];
  double kf[NV * (NV + 1) / 2];
};
enum { F_REGS, F_COOP, F_LOOP, F_ROWS, F_LEAD_REGS, F_LEAD_SPLIT, F_SCHUR };
// Hin [n][NV][NV] (symmetric, full square), dlin / bin / xout [n][NV]; one wavefront per 64 / LPE envs (the launcher refuses n that is not a multiple)
template <int NV, int FORM>
__global__ __launch_bounds__(64) void k_solve(const double* __restrict__ Hin, const double* __restrict__ dlin, const double* __restrict__ bin, double* __restrict__ xout) {
  constexpr int LPE = Lim<NV>::LPE, EPW = 64 / LPE, NA = Lim<NV>::NA;
  __shared__ SolveBlk<NV> blk[EPW];
  const int lane = threadIdx.x & 63, sub = lane % LPE, grp = lane / LPE;
  const long env = (long)blockIdx.x * EPW + grp;
  SolveBlk<NV>& s = blk[grp];
  const bool isl = sub < NV;
  const int l = isl ? sub : NV - 1;
  if (isl) {                                             // column l, as K9 stores it (physics_stepper.h: s.con.Hc.put(i, l, hcol[i], false))
#pragma unroll
    for (int i = 0; i < NV; ++i) s.H.put(i, l, Hin[(env * NV + i) * NV + l], false);
    s.dl[l] = dlin[env * NV + l];
    s.rc[l] = bin[env * NV + l];
  }
  fence();
  double a[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) a[i] = s.rc[i];
  [[maybe_unused]] auto diag = [&](int i) { return s.dl[i]; };
  if constexpr (FORM == F_REGS) {
    double L[NV * (NV + 1) / 2];
    load_tri<NV, NA>(L, s.H, diag);
    chol_regs<NV, NA, (NV > 10)>(L);
    solve_regs<NV, NA>(L, a);
  } else if constexpr (FORM == F_COOP) {
    chol_coop<NV>(s.H, s.dl, l, isl);
    solve_lds<NV>(s.H, a);
  } else if constexpr (FORM == F_LOOP) {
    chol_coop_loop<NV>(s.H, s.dl, l, isl);
    solve_lds_loop<NV>(s.H, s.rc);
    fence();
#pragma unroll
    for (int i = 0; i < NV; ++i) a[i] = s.rc[i];
  } else if constexpr (FORM == F_ROWS) {
    const double xl = chol_solve_rows<NV>(s.H, s.dl, s.rc[l], l, isl, grp);
    fence();
    if (isl) s.rc[l] = xl;
    fence();
#pragma unroll
    for (int i = 0; i < NV; ++i) a[i] = s.rc[i];
  } else if constexpr (FORM == F_LEAD_REGS) {
    solve_lead_regs<NV, NA>(s.H, diag, a);
  } else if constexpr (FORM == F_LEAD_SPLIT) {           // the kitchen's four-wave launches: the helper wave factorises, the owner substitutes (physics_stepper.h, barriers Y / Z)
    constexpr int NL = NA * (NA + 1) / 2;
    {
      double Lk[NL];
#pragma unroll
      for (int i = 0; i < NA; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) Lk[i * (i + 1) / 2 + j] = s.H.lo(i, j);
        Lk[i * (i + 1) / 2 + i] = s.H.lo(i, i) + pinned(s.dl[i]);
      }
      pin_batch(Lk);
      chol_regs<NA, NA, true>(Lk);
#pragma unroll
      for (int e = 0; e < NL; ++e) if (sub == (e % LPE)) s.kf[e] = Lk[e];
      fence();
    }
    double Lk[NL], y[NA];
#pragma unroll
    for (int e = 0; e < NL; ++e) Lk[e] = s.kf[e];
    pin_batch(Lk);
#pragma unroll
    for (int i = 0; i < NA; ++i) y[i] = a[i];
    solve_regs<NA, NA>(Lk, y);
#pragma unroll
    for (int i = 0; i < NA; ++i) a[i] = y[i];
  } else {
    solve_schur_regs<NV, NA>(s.H, diag, a);
  }
  double al = 0;
#pragma unroll
  for (int i = 0; i < NV; ++i) al = l == i ? a[i] : al;
  if (isl) xout[env * NV + l] = al;
}
// the minitaur's per-lane blocks: Lin [n][N (N + 1) / 2] (packed lower triangle), bin [n][N] -> the factor (diagonal inverted) and the solution
template <int N, bool SMALL>
__global__ __launch_bounds__(64) void k_small(const double* __restrict__ Lin, const double* __restrict__ bin, double* __restrict__ Lout, double* __restrict__ xout, const long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  constexpr int NL = N * (N + 1) / 2;
  double L[NL], x[N];
#pragma unroll
  for (int e = 0; e < NL; ++e) L[e] = Lin[i * NL + e];
#pragma unroll
  for (int e = 0; e < N; ++e) x[e] = bin[i * N + e];
  pin_batch(L); pin_batch(x);
  if constexpr (SMALL) chol_small<N>(L); else chol_regs<N, N, true>(L);
  solve_regs<N, N>(L, x);
#pragma unroll
  for (int e = 0; e < NL; ++e) Lout[i * NL + e] = L[e];
#pragma unroll
  for (int e = 0; e < N; ++e) xout[i * N + e] = x[e];
}

inline unsigned blocks_of(long n) { return (unsigned)((n + 63) / 64); }

}  // namespace

#define PRIM_BAD_ARG 1001     // (not a hipError_t the runtime returns for a launch)
extern "C" {

int prim_door_packed() { return EARL_DOOR_PACKED; }

#define PRIM_UNARY(name, OP)                                                                                    \
  int prim_##name(const double* x, double* y, long n, hipStream_t st) {                                         \
    if (!x || !y || n <= 0) return PRIM_BAD_ARG;                                                                \
    hipLaunchKernelGGL(k_unary<OP>, dim3(blocks_of(n)), dim3(64), 0, st, x, y, n);                              \
    return (int)hipGetLastError();                                                                              \
  }
PRIM_UNARY(rcp_nr, U_RCP_NR)
PRIM_UNARY(rsq_nr, U_RSQ_NR)
PRIM_UNARY(rsq2, U_RSQ2)

int prim_sincos_mod(const double* x, double* sn, double* cs, long n, hipStream_t st) {
  if (!x || !sn || !cs || n <= 0) return PRIM_BAD_ARG;
  hipLaunchKernelGGL(k_sincos<false>, dim3(blocks_of(n)), dim3(64), 0, st, x, sn, cs, n);
  return (int)hipGetLastError();
}
int prim_sincos_kc(const double* x, double* sn, double* cs, long n, hipStream_t st) {
  if (!x || !sn || !cs || n <= 0) return PRIM_BAD_ARG;
  hipLaunchKernelGGL(k_sincos<true>, dim3(blocks_of(n)), dim3(64), 0, st, x, sn, cs, n);
  return (int)hipGetLastError();
}
#define PRIM_ROWS(name, kernel, OUT_T)                                                                          \
  int prim_##name(const double* in, OUT_T* out, long n, hipStream_t st) {                                       \
    if (!in || !out || n <= 0) return PRIM_BAD_ARG;                                                             \
    hipLaunchKernelGGL(kernel, dim3(blocks_of(n)), dim3(64), 0, st, in, out, n);                                \
    return (int)hipGetLastError();                                                                              \
  }
PRIM_ROWS(impedance, k_impedance, double)
PRIM_ROWS(cone_apply, k_cone_apply, double)
PRIM_ROWS(cone_zone, k_cone_zone, int)
PRIM_ROWS(algebra, k_algebra, double)

// n = number of 16-lane rows (envs); a multiple of 4 (whole wavefronts)
#define PRIM_SCAN(name, kernel)                                                                                 \
  int prim_##name(const double* in, double* out, long n, hipStream_t st) {                                      \
    if (!in || !out || n <= 0 || n % 4) return PRIM_BAD_ARG;                                                    \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n / 4)), dim3(64), 0, st, in, out);                              \
    return (int)hipGetLastError();                                                                              \
  }
PRIM_SCAN(scan_anc_10, k_scan_anc<10>)
PRIM_SCAN(scan_anc_15, k_scan_anc<15>)
PRIM_SCAN(scan_anc_23, k_scan_anc<23>)
PRIM_SCAN(scan_desc_10_6, (k_scan_desc<10, 6>))
PRIM_SCAN(scan_desc_10_10, (k_scan_desc<10, 10>))
PRIM_SCAN(scan_desc_15_6, (k_scan_desc<15, 6>))
PRIM_SCAN(scan_desc_15_10, (k_scan_desc<15, 10>))
PRIM_SCAN(scan_desc_23_6, (k_scan_desc<23, 6>))
PRIM_SCAN(scan_desc_23_10, (k_scan_desc<23, 10>))
int prim_n_moves() { return N_MOVES; }
int prim_lane_moves(const double* in, double* out, long lanes, hipStream_t st) {      // lanes: a multiple of 64
  if (!in || !out || lanes <= 0 || lanes % 64) return PRIM_BAD_ARG;
  hipLaunchKernelGGL(k_lane_moves, dim3((unsigned)(lanes / 64)), dim3(64), 0, st, in, out, lanes);
  return (int)hipGetLastError();
}

// n = number of systems; a multiple of the envs per wavefront (4 for nv 10 / 15, 2 for nv 22 / 23)
#define PRIM_SOLVE(name, NV, FORM)                                                                              \
  int prim_solve_##name(const double* H, const double* dl, const double* b, double* x, long n, hipStream_t st) {\
    constexpr int EPW = 64 / Lim<NV>::LPE;                                                                      \
    if (!H || !dl || !b || !x || n <= 0 || n % EPW) return PRIM_BAD_ARG;                                        \
    hipLaunchKernelGGL((k_solve<NV, FORM>), dim3((unsigned)(n / EPW)), dim3(64), 0, st, H, dl, b, x);           \
    return (int)hipGetLastError();                                                                              \
  }
PRIM_SOLVE(regs_10, 10, F_REGS)
PRIM_SOLVE(coop_10, 10, F_COOP)
PRIM_SOLVE(regs_15, 15, F_REGS)
PRIM_SOLVE(coop_15, 15, F_COOP)
PRIM_SOLVE(schur_15, 15, F_SCHUR)
PRIM_SOLVE(coop_22, 22, F_COOP)
PRIM_SOLVE(loop_22, 22, F_LOOP)
PRIM_SOLVE(rows_22, 22, F_ROWS)
PRIM_SOLVE(coop_23, 23, F_COOP)
PRIM_SOLVE(loop_23, 23, F_LOOP)
PRIM_SOLVE(lead_regs_23, 23, F_LEAD_REGS)
PRIM_SOLVE(lead_split_23, 23, F_LEAD_SPLIT)

#define PRIM_SMALL(name, N, SMALL)                                                                              \
  int prim_##name(const double* L, const double* b, double* Lout, double* x, long n, hipStream_t st) {          \
    if (!L || !b || !Lout || !x || n <= 0) return PRIM_BAD_ARG;                                                 \
    hipLaunchKernelGGL((k_small<N, SMALL>), dim3(blocks_of(n)), dim3(64), 0, st, L, b, Lout, x, n);             \
    return (int)hipGetLastError();                                                                              \
  }
PRIM_SMALL(chol_small_4, 4, true)
PRIM_SMALL(chol_regs_4, 4, false)
PRIM_SMALL(chol_small_6, 6, true)
PRIM_SMALL(chol_regs_6, 6, false)

}  // extern "C"

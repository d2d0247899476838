// qd_col.hip — lean column kernels: Lindblad sweeps of density matrices with 33 <= N <= 64 rows and runtime level counts
// (BASELINE config 4: 3 x 20 levels, dim 3600, 3600 initial conditions).  gfx950 / CDNA4 only.
//
// Layout (as ColStencil of qd_device.h: lane = row I of rho, a wave owns EPT consecutive columns I', vectorised index
// it = I' N + I, util.cpp:150), rewritten for register and issue economy:
//   * the exchange vector lives in LDS with a PADDED column stride of 64 rows (1 KiB per column), double buffered: the address of
//     every neighbour is a thread invariant plus a compile-time immediate (slot j of the wave = + j KiB) - no per-slot address
//     registers, nothing for the compiler to hoist and spill;
//   * a neighbour that does not exist has a zero coefficient, and its address is folded onto the element itself ONCE (thread
//     invariants for the bra side, wave-uniform scalar offsets for the ket side), so no clamping happens in the hot loop;
//   * idle lanes (row >= N) and idle slots (column >= N) carry zeros through the same arithmetic: no divergence, no predication
//     except on global memory;
//   * the bra neighbours of the stride-1 oscillator are the adjacent lanes (DPP), its ket neighbours the adjacent slots
//     (registers); the other oscillators read LDS: ~5 ds_read_b128 per element and application for two oscillators;
//   * the state x is parked in its output buffer while a linear solve runs; the solver holds b and the iterate, nothing else;
//   * dipole-dipole coupling (any J_kl != 0; ColLean's HJ, kernels k_*_colj of qd_colj.hip): four more ds_read_b128 per pair and
//     element - the bra neighbours at rows I -+ post[k] +- post[l] through two more thread-invariant addresses, the ket neighbours at
//     columns I' -+ post[k] +- post[l] through two more scalar offsets, weights that carry J_kl, and cos / sin(eta_kl t) from the control
//     table row.  No diagonal entry: the diagonal-split solver's D, P and the column table are those of the uncoupled system.
//
// The device code (ColLean, ColTeam, the three kernels) is qd_col.h, shared with qd_colj.hip; this unit instantiates the kernels of
// systems without coupling, k_*_col, and holds the host side: availability, slicing, launchers.
//
// Reference semantics (paths relative to the reference repository): stencil include/mastereq.hpp:316-912 as instantiated by
// src/mastereq.cpp:1464-1709 (two oscillators) / :1713-2018 (three); IMR forward / adjoint src/timestepper.cpp:584-694,
// Neumann :697-727, time loops :96-253, penalties :256-339, gradient coefficients include/mastereq.hpp:553-604.
#define QD_COLK(base) base##_col
#define QD_COL_HJ false
#include "qd_col.h"

namespace qd {

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
int col_cu_count() {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
    if (ncu <= 0) ncu = 256;
  }
  return ncu;
}

// Slices of a sweep of nb initial conditions over ntime steps (1 = one workgroup per initial condition, no scheduler): the smallest power
// of two that brings the idle tail - (ceil(r) - r) / ceil(r) for r = nb k / #CUs rounds - below 1 %, keeping at least 32 steps per slice.
int col_slices(int nb, int ntime, const TuneOpts& o) {
  if (o.col_slices == 1) return 1;
  // (at most 255 slices: the scheduler word of an initial condition counts completed slices in its low byte, sched_wait / sched_done)
  if (o.col_slices > 1) return std::min(std::min(o.col_slices, 255), std::max(ntime, 1));
  const int ncu = col_cu_count();
  if (nb <= ncu) return 1;
  int best = 1;
  double best_waste = 1.0;
  for (int k = 1; k <= 64 && ntime / k >= 32; k *= 2) {
    const double r = (double)nb * k / ncu;
    const double waste = (ceil(r) - r) / ceil(r);
    if (waste < best_waste - 1e-12) {
      best_waste = waste;
      best = k;
    }
    if (waste < 0.01) break;
  }
  return best_waste < 0.01 || best > 1 ? best : 1;
}

// SweepArgs::kry of the Krylov kernels: GMRES_MR_G + 2 padded scratch vectors per RESIDENT workgroup (ColTeam::init_kry), in doubles
// (a sweep without time slices starts one workgroup per initial condition, a sliced one a resident grid: col_grid)
size_t col_krylov_doubles(int nb, int nslice) { return (size_t)(nslice > 1 ? std::min(nb * nslice, 2 * col_cu_count()) : nb) * (GMRES_MR_G + 2) * 2 * KRY_VEC; }

// Lindblad, matrix-free, runtime level counts that are not all 2, two or three oscillators, a density matrix of 33..64 rows (one lane
// per row), the last oscillator with stride 1 (always: post[Q-1] == 1).  With dipole-dipole coupling (any J_kl != 0: the k_*_colj
// kernels of qd_colj.hip) only from 44 rows on - where pick_config gives a coupled system the column variant anyway; coupled systems
// of 33..43 rows stay on variant 4 (nothing has been measured for them).  The coupled kernels are built in the diagonal-split form
// only: qd_handle::col_sweep sends a coupled sweep that asks for the plain Neumann iteration to the general column kernel.
bool collean_available(const DevSys& S, const TuneOpts& o) {
  if (o.no_collean) return false;
  if (!S.lindblad || S.dense || (S.Q != 2 && S.Q != 3) || S.N < 33 || S.N > 64 || (S.hasJ && S.N < 44)) return false;
  bool qubit = true;
  for (int k = 0; k < S.Q; k++) qubit = qubit && S.n[k] == 2;
  return !qubit && S.post[S.Q - 1] == 1;
}

template <int Q, int EPT, bool SPLIT>
static hipError_t go_fwd_col_s(const SweepArgs& a, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(a.S.N);
  // (SKIP: stopping tests skipped, see ColTeam::stage)
  // (implicit midpoint only: the predictor compares the pass count of a sub-step with its predecessor's, and the sub-steps of a composite
  //  step differ in size - IMR4 / IMR8 test every pass; nothing of this lives in the kernels)
  const bool skip = a.rel2 < 1e-30f && !a.col_noskip && a.nstages == 1, uslot = col_uslot<EPT>(a.S);
  auto kf = uslot ? (skip ? k_forward_col<Q, EPT, SPLIT, true, true> : k_forward_col<Q, EPT, SPLIT, true, false>)
                  : (skip ? k_forward_col<Q, EPT, SPLIT, false, true> : k_forward_col<Q, EPT, SPLIT, false, false>);
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(0, "k_forward_col", Q, EPT, SPLIT, uslot, skip, false);
  hipLaunchKernelGGL(kf, dim3(col_grid(kf, a, 64 * (ST::ncols(a.S.N) / EPT), lds)), dim3(64 * (ST::ncols(a.S.N) / EPT)), lds, st, a);
  return hipGetLastError();
}
// the Krylov kernels (SweepArgs::use_gmres)
template <int Q, int EPT>
static hipError_t go_fwd_col_k(const SweepArgs& a, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(a.S.N) + ColTeam<Q, EPT, true>::kry_lds_extra(a.S.N);
  const bool uslot = col_uslot<EPT>(a.S);
  auto kf = uslot ? k_forward_col<Q, EPT, true, true, false, true> : k_forward_col<Q, EPT, true, false, false, true>;
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(0, "k_forward_col", Q, EPT, true, uslot, false, true);
  hipLaunchKernelGGL(kf, dim3(col_grid(kf, a, 64 * (ST::ncols(a.S.N) / EPT), lds)), dim3(64 * (ST::ncols(a.S.N) / EPT)), lds, st, a);
  return hipGetLastError();
}
template <int Q, int EPT>
static hipError_t go_adj_col_k(const SweepArgs& a, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(a.S.N) + ColTeam<Q, EPT, true>::kry_lds_extra(a.S.N);
  const bool uslot = col_uslot<EPT>(a.S);
  auto kf = uslot ? k_adjoint_col<Q, EPT, true, true, false, true> : k_adjoint_col<Q, EPT, true, false, false, true>;
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(1, "k_adjoint_col", Q, EPT, true, uslot, false, true);
  hipLaunchKernelGGL(kf, dim3(col_grid(kf, a, 64 * (ST::ncols(a.S.N) / EPT), lds)), dim3(64 * (ST::ncols(a.S.N) / EPT)), lds, st, a);
  return hipGetLastError();
}
template <int Q, int EPT>
static hipError_t go_fwd_col(const SweepArgs& a, hipStream_t st) {
  if (a.use_gmres) return go_fwd_col_k<Q, EPT>(a, st);
  return a.neumann_split ? go_fwd_col_s<Q, EPT, true>(a, st) : go_fwd_col_s<Q, EPT, false>(a, st);
}
template <int Q, int EPT, bool SPLIT>
static hipError_t go_adj_col_s(const SweepArgs& a, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(a.S.N);
  // (implicit midpoint only: the predictor compares the pass count of a sub-step with its predecessor's, and the sub-steps of a composite
  //  step differ in size - IMR4 / IMR8 test every pass; nothing of this lives in the kernels)
  const bool skip = a.rel2 < 1e-30f && !a.col_noskip && a.nstages == 1, uslot = col_uslot<EPT>(a.S);
  auto kf = uslot ? (skip ? k_adjoint_col<Q, EPT, SPLIT, true, true> : k_adjoint_col<Q, EPT, SPLIT, true, false>)
                  : (skip ? k_adjoint_col<Q, EPT, SPLIT, false, true> : k_adjoint_col<Q, EPT, SPLIT, false, false>);
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(1, "k_adjoint_col", Q, EPT, SPLIT, uslot, skip, false);
  hipLaunchKernelGGL(kf, dim3(col_grid(kf, a, 64 * (ST::ncols(a.S.N) / EPT), lds)), dim3(64 * (ST::ncols(a.S.N) / EPT)), lds, st, a);
  return hipGetLastError();
}
template <int Q, int EPT>
static hipError_t go_adj_col(const SweepArgs& a, hipStream_t st) {
  if (a.use_gmres) return go_adj_col_k<Q, EPT>(a, st);
  return a.neumann_split ? go_adj_col_s<Q, EPT, true>(a, st) : go_adj_col_s<Q, EPT, false>(a, st);
}
template <int Q, int EPT>
static hipError_t go_app_col(const DevSys& S, const double* ctlrow, int tr, const double* x, double* y, int nb, bool split, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(S.N);
  // (the option neumann_split = 1 selects the kernel family that re-derives the diagonal from its compact form: test coverage)
  auto kf = split ? k_apply_col<Q, EPT, true> : k_apply_col<Q, EPT, false>;
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(2, "k_apply_col", Q, EPT, split);
  hipLaunchKernelGGL(kf, dim3(nb), dim3(64 * (ST::ncols(S.N) / EPT)), lds, st, S, ctlrow, tr, x, y);
  return hipGetLastError();
}

// Columns per wave.  Measured on the 3 x 20 workload (3600 initial conditions x 100 steps, forward sweep, one lease): 4 columns
// (15 waves, 128 VGPRs, 63 spills) 58.9 ms, 5 columns (12 waves, 168 VGPRs) 48.4 ms, 6 columns (10 waves, 59 spills) 62.9 ms,
// 8 columns (8 waves, 234 VGPRs, no spills) 53.4 ms; the general column kernel of qd_device.h 73.1 ms.  Five columns per wave cover
// N <= 60, eight the rest; only these two are built.
#define QD_COL_DISPATCH(FN, ...)                                                    \
  do {                                                                              \
    if (Qn == 2) return Nn <= 60 ? FN<2, 5>(__VA_ARGS__) : FN<2, 8>(__VA_ARGS__); \
    if (Qn == 3) return Nn <= 60 ? FN<3, 5>(__VA_ARGS__) : FN<3, 8>(__VA_ARGS__); \
    return hipErrorInvalidValue;                                                    \
  } while (0)

hipError_t launch_forward_col(const SweepArgs& a, hipStream_t st) {
  if (a.S.hasJ) return launch_forward_colj(a, st);
  const int Qn = a.S.Q, Nn = a.S.N;
  QD_COL_DISPATCH(go_fwd_col, a, st);
}
hipError_t launch_adjoint_col(const SweepArgs& a, hipStream_t st) {
  if (a.S.hasJ) return launch_adjoint_colj(a, st);
  const int Qn = a.S.Q, Nn = a.S.N;
  QD_COL_DISPATCH(go_adj_col, a, st);
}
hipError_t launch_apply_col(const DevSys& S, const double* ctlrow, int transpose, const double* x, double* y, int nb, const TuneOpts& o, hipStream_t st) {
  if (S.hasJ) return launch_apply_colj(S, ctlrow, transpose, x, y, nb, st);
  const int Qn = S.Q, Nn = S.N;
  QD_COL_DISPATCH(go_app_col, S, ctlrow, transpose, x, y, nb, o.neumann_split == 1, st);
}

}  // namespace qd

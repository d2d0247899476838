// qd_colj.hip — the lean column kernels for systems with dipole-dipole coupling (any J_kl != 0): k_forward_colj, k_adjoint_colj,
// k_apply_colj.  The same device code as qd_col.hip (qd_col.h: ColLean / ColTeam with HJ = true, the sweep bodies), in a translation
// unit of its own so that it compiles next to qd_col.o; only the kernel names and the flag differ (QD_COLK, QD_COL_HJ).  gfx950 / CDNA4 only.
//
// Per pair k < l and element the coupling adds four ds_read_b128 from the padded exchange buffer - two bra neighbours (rows
// I -+ post[k] +- post[l] of the same column: thread-invariant address and weight) and two ket neighbours (columns I' -+ post[k] +- post[l]
// of the same row: wave-uniform offset and weight in scalar registers) - and cos / sin(eta_kl t) of the sub-step from the control table
// row (scalar loads).  A neighbour that does not exist has weight zero and its address folded onto the element itself in init().
//
// What is built: two or three oscillators, five or eight columns per wave, both USLOT forms, the diagonal-split form (SPLIT = true) only,
// with two solvers - the stationary iteration testing every pass (no SKIP form) and the Krylov solver - plus one operator application
// per (Q, EPT): 36 kernels.  A coupled sweep that asks for the plain Neumann iteration (neumann_split = 0) is not served here:
// qd_handle::col_sweep keeps it on the general column kernel of qd_device.h.
//
// Reference semantics: Jkl_coupling, include/mastereq.hpp:632-741, called from src/mastereq.cpp:1553.
#define QD_COLK(base) base##_colj
#define QD_COL_HJ true
#include "qd_col.h"

namespace qd {

// KRY = SweepArgs::use_gmres; otherwise the diagonal-split stationary iteration (the plan has neumann_split = 1: qd_handle::col_sweep)
template <int Q, int EPT, bool KRY>
static hipError_t go_fwd_colj(const SweepArgs& a, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(a.S.N) + (KRY ? ColTeam<Q, EPT, true>::kry_lds_extra(a.S.N) : 0);
  const bool uslot = col_uslot<EPT>(a.S);
  auto kf = uslot ? k_forward_colj<Q, EPT, true, true, false, KRY> : k_forward_colj<Q, EPT, true, false, false, KRY>;
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(0, "k_forward_colj", Q, EPT, true, uslot, false, KRY);
  hipLaunchKernelGGL(kf, dim3(col_grid(kf, a, 64 * (ST::ncols(a.S.N) / EPT), lds)), dim3(64 * (ST::ncols(a.S.N) / EPT)), lds, st, a);
  return hipGetLastError();
}
template <int Q, int EPT, bool KRY>
static hipError_t go_adj_colj(const SweepArgs& a, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(a.S.N) + (KRY ? ColTeam<Q, EPT, true>::kry_lds_extra(a.S.N) : 0);
  const bool uslot = col_uslot<EPT>(a.S);
  auto kf = uslot ? k_adjoint_colj<Q, EPT, true, true, false, KRY> : k_adjoint_colj<Q, EPT, true, false, false, KRY>;
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(1, "k_adjoint_colj", Q, EPT, true, uslot, false, KRY);
  hipLaunchKernelGGL(kf, dim3(col_grid(kf, a, 64 * (ST::ncols(a.S.N) / EPT), lds)), dim3(64 * (ST::ncols(a.S.N) / EPT)), lds, st, a);
  return hipGetLastError();
}
template <int Q, int EPT>
static hipError_t go_app_colj(const DevSys& S, const double* ctlrow, int tr, const double* x, double* y, int nb, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(S.N);
  auto kf = k_apply_colj<Q, EPT, true>;
  hipError_t e = set_lds_col(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(2, "k_apply_colj", Q, EPT, true);
  hipLaunchKernelGGL(kf, dim3(nb), dim3(64 * (ST::ncols(S.N) / EPT)), lds, st, S, ctlrow, tr, x, y);
  return hipGetLastError();
}

// columns per wave as in qd_col.hip (QD_COL_DISPATCH): five for N <= 60, eight above
#define QD_COLJ_DISPATCH(FN, ...)                                                   \
  do {                                                                              \
    if (Qn == 2) return Nn <= 60 ? FN<2, 5>(__VA_ARGS__) : FN<2, 8>(__VA_ARGS__); \
    if (Qn == 3) return Nn <= 60 ? FN<3, 5>(__VA_ARGS__) : FN<3, 8>(__VA_ARGS__); \
    return hipErrorInvalidValue;                                                    \
  } while (0)

template <int Q, int EPT>
static hipError_t go_fwd_colj_any(const SweepArgs& a, hipStream_t st) {
  if (!a.use_gmres && !a.neumann_split) return hipErrorInvalidValue;  // (not built; never planned: qd_handle::col_sweep)
  return a.use_gmres ? go_fwd_colj<Q, EPT, true>(a, st) : go_fwd_colj<Q, EPT, false>(a, st);
}
template <int Q, int EPT>
static hipError_t go_adj_colj_any(const SweepArgs& a, hipStream_t st) {
  if (!a.use_gmres && !a.neumann_split) return hipErrorInvalidValue;
  return a.use_gmres ? go_adj_colj<Q, EPT, true>(a, st) : go_adj_colj<Q, EPT, false>(a, st);
}

hipError_t launch_forward_colj(const SweepArgs& a, hipStream_t st) {
  const int Qn = a.S.Q, Nn = a.S.N;
  QD_COLJ_DISPATCH(go_fwd_colj_any, a, st);
}
hipError_t launch_adjoint_colj(const SweepArgs& a, hipStream_t st) {
  const int Qn = a.S.Q, Nn = a.S.N;
  QD_COLJ_DISPATCH(go_adj_colj_any, a, st);
}
hipError_t launch_apply_colj(const DevSys& S, const double* ctlrow, int transpose, const double* x, double* y, int nb, hipStream_t st) {
  const int Qn = S.Q, Nn = S.N;
  QD_COLJ_DISPATCH(go_app_colj, S, ctlrow, transpose, x, y, nb, st);
}

}  // namespace qd

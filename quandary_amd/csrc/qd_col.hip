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
// The device code (ColLean, ColTeam, the three kernels) and the launchers (col_launch, col_sweep, col_apply) are qd_col.h, shared by
// every unit of the family (the list: the top of qd_col.h).  This unit is the plain one for systems without coupling, k_*_col - qd_col.h
// with its defaults -, and holds the rest of the host side: availability, slicing, the family's entry points.
//
// Reference semantics (paths relative to the reference repository): stencil include/mastereq.hpp:316-912 as instantiated by
// src/mastereq.cpp:1464-1709 (two oscillators) / :1713-2018 (three); IMR forward / adjoint src/timestepper.cpp:584-694,
// Neumann :697-727, time loops :96-253, penalties :256-339, gradient coefficients include/mastereq.hpp:553-604.
#include "qd_col.h"

namespace qd {

// Slices of a sweep of nb initial conditions over ntime steps (1 = one workgroup per initial condition, no scheduler): the smallest power
// of two that brings the idle tail - (ceil(r) - r) / ceil(r) for r = nb k / #CUs rounds - below 1 %, keeping at least 32 steps per slice.
int col_slices(int nb, int ntime, const TuneOpts& o) {
  if (o.col_slices == 1) return 1;
  // (at most 255 slices: the scheduler word of an initial condition counts completed slices in its low byte, sched_wait / sched_done)
  if (o.col_slices > 1) return std::min(std::min(o.col_slices, 255), std::max(ntime, 1));
  const int ncu = cu_count();
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
size_t col_krylov_doubles(int nb, int nslice) { return (size_t)(nslice > 1 ? std::min(nb * nslice, 2 * cu_count()) : nb) * (GMRES_MR_G + 2) * 2 * KRY_VEC; }

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

QD_COL_PART(2, 5)
QD_COL_PART(2, 8)
QD_COL_PART(3, 5)
QD_COL_PART(3, 8)

// The family's sweep entry point: the part of the unit (form, a.S.hasJ) for the system's <Q, EPT>.  The parts of the other units are
// objects of their own (qd_colj.hip, qd_col_form.hip); a unit that is not built - the pair form with coupling - is an error.
template <Form F, bool HJ>
static hipError_t col_unit(const SweepArgs& a, bool adjoint, hipStream_t st) {
  QD_COL_DISPATCH(a.S, col_sweep_part, ColUnit<F, HJ>{}, a, adjoint, st);
}
hipError_t launch_sweep_col(Form form, const SweepArgs& a, bool adjoint, hipStream_t st) {
  const bool hj = a.S.hasJ != 0;
  switch (form) {
    case Form::Plain: return hj ? col_unit<Form::Plain, true>(a, adjoint, st) : col_unit<Form::Plain, false>(a, adjoint, st);
    case Form::Sets: return hj ? col_unit<Form::Sets, true>(a, adjoint, st) : col_unit<Form::Sets, false>(a, adjoint, st);
    case Form::Vars: return hj ? col_unit<Form::Vars, true>(a, adjoint, st) : col_unit<Form::Vars, false>(a, adjoint, st);
    case Form::Sens: return hj ? col_unit<Form::Sens, true>(a, adjoint, st) : col_unit<Form::Sens, false>(a, adjoint, st);
    case Form::Pair: return hj ? hipErrorInvalidValue : col_unit<Form::Pair, false>(a, adjoint, st);
  }
  return hipErrorInvalidValue;
}
hipError_t launch_apply_col(const DevSys& S, const double* ctlrow, int transpose, const double* x, double* y, int nb, const TuneOpts& o, hipStream_t st) {
  if (S.hasJ) return launch_apply_colj(S, ctlrow, transpose, x, y, nb, st);
  QD_COL_DISPATCH(S, col_apply, S, ctlrow, transpose, x, y, nb, o.neumann_split == 1, st);
}

}  // namespace qd

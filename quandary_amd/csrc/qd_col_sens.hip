// qd_col_sens.hip - the sensitivity form of the lean column adjoint sweep, systems without dipole-dipole coupling: k_adjoint_col_sens,
// the template <Q, EPT, SPLIT = true, USLOT, SKIP, KRY = false> of qd_col.h compiled with the per-element sums of kbar^T (dM/d theta) z
// (QD_COL_SENS there; model-constant sensitivities, qd_optim_evalGradF_model with option sens_lean).  The adjoint kernel only - the
// forward sweep of the call is k_forward_col - and only the diagonal-split stationary instantiations: no plain-Neumann form, no Krylov
// instantiation, no operator application.  gfx950 / CDNA4 only.
//
// Built as five objects like qd_col_vars.hip: one per <Q, EPT> (-DQD_COL_SETS_Q= -DQD_COL_SETS_EPT=: 4 kernels each, compiled side by
// side) and, without the two defines, the entry point.
#define QD_COLK(base) base##_col_sens
#define QD_COL_HJ false
#define QD_COL_SENS 1
#include "qd_col.h"

#ifndef QD_COL_SETS_Q
namespace qd {

hipError_t launch_sweep_col_sens(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_sens_args_ok(a, adjoint)) return hipErrorInvalidValue;
  if (a.S.hasJ) return launch_sweep_colj_sens(a, adjoint, st);
  QD_COL_DISPATCH(a.S, QD_COLK(sweep_part), a, adjoint, st);
}

}  // namespace qd
#endif

// qd_col_vars.hip - the third form of the lean column sweeps, systems without dipole-dipole coupling: k_forward_col_vars /
// k_adjoint_col_vars, the templates <Q, EPT, SPLIT = true, USLOT, SKIP, KRY = false> of qd_col.h compiled with one block of model constants
// per variant (QD_COL_VARS there; model-parameter ensemble, qd_optim_evalGradF_ensemble_model).  Only the diagonal-split stationary
// instantiations: no plain-Neumann form, no Krylov instantiation, no operator application.  gfx950 / CDNA4 only.
//
// Built as five objects like qd_col_sets.hip: one per <Q, EPT> (-DQD_COL_SETS_Q= -DQD_COL_SETS_EPT=: 8 kernels each, compiled side by
// side) and, without the two defines, the entry point.
#define QD_COLK(base) base##_col_vars
#define QD_COL_HJ false
#define QD_COL_VARS 1
#include "qd_col.h"

#ifndef QD_COL_SETS_Q
namespace qd {

hipError_t launch_sweep_col_vars(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_vars_args_ok(a, adjoint)) return hipErrorInvalidValue;
  if (a.S.hasJ) return launch_sweep_colj_vars(a, adjoint, st);
  QD_COL_DISPATCH(a.S, QD_COLK(sweep_part), a, adjoint, st);
}

}  // namespace qd
#endif

// qd_colj_vars.hip - the third form of the lean column sweeps for systems with dipole-dipole coupling: k_forward_colj_vars /
// k_adjoint_colj_vars, the templates <Q, EPT, SPLIT = true, USLOT, SKIP = false, KRY = false> of qd_col.h compiled with one block of model
// constants per variant (QD_COL_VARS there).  A variant whose couplings are all zero runs here too, with zero weights.  No Krylov
// instantiation and no operator application.  gfx950 / CDNA4 only.
//
// Built as five objects like qd_col_vars.hip: one per <Q, EPT> (4 kernels each) and the entry point.
#define QD_COLK(base) base##_colj_vars
#define QD_COL_HJ true
#define QD_COL_VARS 1
#include "qd_col.h"

#ifndef QD_COL_SETS_Q
namespace qd {

hipError_t launch_sweep_colj_vars(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_vars_args_ok(a, adjoint) || !a.S.hasJ) return hipErrorInvalidValue;
  QD_COL_DISPATCH(a.S, QD_COLK(sweep_part), a, adjoint, st);
}

}  // namespace qd
#endif

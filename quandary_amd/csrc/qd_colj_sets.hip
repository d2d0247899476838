// qd_colj_sets.hip - the SETS form of the stationary-iteration sweeps of the lean column kernels for systems with dipole-dipole coupling:
// k_forward_colj_sets / k_adjoint_colj_sets, the templates <Q, EPT, SPLIT = true, USLOT, SKIP = false, KRY = false> of qd_col.h compiled a
// second time with one control table per parameter set (QD_COL_SETS there).  The pair columns cos / sin(eta_kl t) widen a table row, not
// the addressing.  No Krylov instantiation and no operator application.  gfx950 / CDNA4 only.
//
// Built as five objects like qd_col_sets.hip: one per <Q, EPT> (4 kernels each) and the entry point.
#define QD_COLK(base) base##_colj_sets
#define QD_COL_HJ true
#define QD_COL_SETS 1
#include "qd_col.h"

#ifndef QD_COL_SETS_Q
namespace qd {

hipError_t launch_sweep_colj_sets(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_sets_args_ok(a) || !a.S.hasJ) return hipErrorInvalidValue;
  QD_COL_DISPATCH(a.S, QD_COLK(sweep_part), a, adjoint, st);
}

}  // namespace qd
#endif

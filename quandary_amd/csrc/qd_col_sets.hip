// qd_col_sets.hip - the SETS form of the stationary-iteration sweeps of the lean column kernels, systems without dipole-dipole coupling:
// k_forward_col_sets / k_adjoint_col_sets, the templates <Q, EPT, SPLIT, USLOT, SKIP, KRY = false> of qd_col.h compiled a second time with
// one control table per parameter set (QD_COL_SETS there; parameter-set batch, qd_optim_evalGradF_batch with option batch_lean).  No Krylov
// instantiation and no operator application.  gfx950 / CDNA4 only.
//
// Built as five objects: one per <Q, EPT> (-DQD_COL_SETS_Q= -DQD_COL_SETS_EPT=: 16 kernels each, compiled side by side) and, without the
// two defines, the entry point.
#define QD_COLK(base) base##_col_sets
#define QD_COL_HJ false
#define QD_COL_SETS 1
#include "qd_col.h"

#ifndef QD_COL_SETS_Q
namespace qd {

hipError_t launch_sweep_col_sets(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_sets_args_ok(a)) return hipErrorInvalidValue;
  if (a.S.hasJ) return launch_sweep_colj_sets(a, adjoint, st);
  QD_COL_DISPATCH(a.S, QD_COLK(sweep_part), a, adjoint, st);
}

}  // namespace qd
#endif

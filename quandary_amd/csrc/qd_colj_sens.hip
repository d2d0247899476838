// qd_colj_sens.hip - the sensitivity form of the lean column adjoint sweep for systems with dipole-dipole coupling: k_adjoint_colj_sens,
// the template <Q, EPT, SPLIT = true, USLOT, SKIP = false, KRY = false> of qd_col.h compiled with the per-element sums of
// kbar^T (dM/d theta) z (QD_COL_SENS there).  The coupling has no part in dM/d theta of a detuning or a Kerr coefficient: the sums are
// those of the uncoupled unit, formed from this unit's kbar and z.  The adjoint kernel only; no Krylov instantiation and no operator
// application.  gfx950 / CDNA4 only.
//
// Built as five objects like qd_col_sens.hip: one per <Q, EPT> (2 kernels each) and the entry point.
#define QD_COLK(base) base##_colj_sens
#define QD_COL_HJ true
#define QD_COL_SENS 1
#include "qd_col.h"

#ifndef QD_COL_SETS_Q
namespace qd {

hipError_t launch_sweep_colj_sens(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_sens_args_ok(a, adjoint) || !a.S.hasJ) return hipErrorInvalidValue;
  QD_COL_DISPATCH(a.S, QD_COLK(sweep_part), a, adjoint, st);
}

}  // namespace qd
#endif

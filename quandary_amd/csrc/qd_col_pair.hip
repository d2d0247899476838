// qd_col_pair.hip - the pair form of the forward sweep of the lean column kernels, systems without dipole-dipole coupling:
// k_forward_col_pair, the templates <Q, EPT, SPLIT, USLOT, SKIP, KRY = false> of qd_col.h compiled once more with the penalty block that
// sums the two Hermitian members of a state apart (QD_COL_PAIR there; forward sweeps on Hermitian pairs, option pair_hermitian).  No
// adjoint kernel, no Krylov instantiation and no operator application.  gfx950 / CDNA4 only.
//
// Built as five objects: one per <Q, EPT> (-DQD_COL_SETS_Q= -DQD_COL_SETS_EPT=: eight kernels each, compiled side by side) and, without
// the two defines, the entry point.
#define QD_COLK(base) base##_col_pair
#define QD_COL_HJ false
#define QD_COL_PAIR 1
#include "qd_col.h"

#ifndef QD_COL_SETS_Q
namespace qd {

hipError_t launch_sweep_col_pair(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_pair_args_ok(a, adjoint)) return hipErrorInvalidValue;
  QD_COL_DISPATCH(a.S, QD_COLK(sweep_part), a, adjoint, st);
}

}  // namespace qd
#endif

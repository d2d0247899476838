// qd_colj.hip — the lean column kernels for systems with dipole-dipole coupling (any J_kl != 0): k_forward_colj, k_adjoint_colj,
// k_apply_colj.  The same device code and the same launchers as qd_col.hip (qd_col.h: ColLean / ColTeam with HJ = true, the sweep bodies,
// col_sweep / col_apply), in a translation unit of its own so that it compiles next to qd_col.o; only the kernel names and the flag differ
// (QD_COLK from QD_COL_HJ, which this file - the plain unit with coupling - sets itself).  gfx950 / CDNA4 only.
//
// Per pair k < l and element the coupling adds four ds_read_b128 from the padded exchange buffer - two bra neighbours (rows
// I -+ post[k] +- post[l] of the same column: thread-invariant address and weight) and two ket neighbours (columns I' -+ post[k] +- post[l]
// of the same row: wave-uniform offset and weight in scalar registers) - and cos / sin(eta_kl t) of the sub-step from the control table
// row (scalar loads).  A neighbour that does not exist has weight zero and its address folded onto the element itself in init().
//
// What is built: two or three oscillators, five or eight columns per wave, both USLOT forms, the diagonal-split form (SPLIT = true) only,
// with two solvers - the stationary iteration testing every pass (no SKIP form) and the Krylov solver - plus one operator application
// per (Q, EPT): 36 kernels (col_sweep's col_coupled branches).  A coupled sweep that asks for the plain Neumann iteration (neumann_split = 0)
// is not served here: qd_handle::col_sweep keeps it on the general column kernel of qd_device.h.
//
// Reference semantics: Jkl_coupling, include/mastereq.hpp:632-741, called from src/mastereq.cpp:1553.
#define QD_COL_HJ 1
#include "qd_col.h"

namespace qd {

QD_COL_PART(2, 5)
QD_COL_PART(2, 8)
QD_COL_PART(3, 5)
QD_COL_PART(3, 8)
hipError_t launch_apply_colj(const DevSys& S, const double* ctlrow, int transpose, const double* x, double* y, int nb, hipStream_t st) {
  QD_COL_DISPATCH(S, col_apply, S, ctlrow, transpose, x, y, nb, true, st);
}

}  // namespace qd

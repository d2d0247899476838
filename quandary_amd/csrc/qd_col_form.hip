// qd_col_form.hip - every unit of the lean column kernels beside the two plain ones (qd_col.hip, qd_colj.hip): qd_col.h compiled once per
// (form, coupling, Q, EPT), all four on the command line (the Makefile's COLUNITS x COL_KEYS):
//   -DQD_COL_FORM=  a value of qd::Form but the plain one       -DQD_COL_HJ=  0 | 1: systems without / with dipole-dipole coupling
//   -DQD_COL_Q= -DQD_COL_EPT=  the <Q, EPT> of this object: 2 | 3 oscillators, 5 | 8 columns per wave
// An object holds the sweep kernels of its unit for that <Q, EPT> - k_*_col_sets, k_adjoint_colj_sens, k_forward_col_pair, ...: what each
// form is and what is built of it, the top of qd_col.h - and the part of the sweep that launches them, which launch_sweep_col of
// qd_col.hip reaches.  No Krylov instantiation and no operator application.  gfx950 / CDNA4 only.
#if !defined(QD_COL_FORM) || !defined(QD_COL_HJ) || !defined(QD_COL_Q) || !defined(QD_COL_EPT)
#error "qd_col_form.hip: QD_COL_FORM, QD_COL_HJ, QD_COL_Q and QD_COL_EPT come from the command line"
#endif
#include "qd_col.h"

namespace qd {

static_assert(col_form != Form::Plain, "the plain units are qd_col.hip and qd_colj.hip");
QD_COL_PART(QD_COL_Q, QD_COL_EPT)

}  // namespace qd

// qd_col_vars.h - constants table of a model-parameter ensemble on the lean column kernels (qd_col.h, Form::Vars: k_*_col_vars /
// k_*_colj_vars; qd_optim_evalF_ensemble_model / qd_optim_evalGradF_ensemble_model).
//
// One control vector is evaluated on nvar variants of the standard Hamiltonian model that differ in transition frequencies, self-Kerr
// and cross-Kerr coefficients and dipole-dipole couplings.  DevSys travels by value as a kernel argument and holds ONE set of those
// constants; the variants' live in a device table, one block per variant, in rad/ns as qd_create converts them:
//   [nvar][2 Q + 2 npairs]:  detune_0 .. detune_{Q-1} | xi_0 .. xi_{Q-1} | xikl_0 .. xikl_{npairs-1} | J_0 .. J_{npairs-1}
// The states of a launch are nvar sets of SweepArgs::nb_set states; the task of state ic reads the block of variant ic / nb_set through
// the scalar path (wave-uniform address).  Everything else of DevSys - level counts, strides, decay and dephasing rates, hasJ - is the
// handle's and still comes from the kernel argument.
//
// The table reaches the kernels in S.hcr, the field a dense user Hamiltonian uses for Re(Hc_k): the lean column family is never dense
// (collean_available), and SweepArgs keeps its size and field offsets (qd_internal.h: some kernels keep a copy of the struct in
// scratch).  Only the accessors below name the alias.
#pragma once
#include "qd_device.h"

namespace qd {

__host__ __device__ inline int col_vars_stride(int Q, int npairs) { return 2 * Q + 2 * npairs; }  // doubles per variant
// (null = no variants: the host asks this of a matrix-free system only, S.dense == 0)
__host__ __device__ inline const double* col_vars_tab(const SweepArgs& A) { return A.S.hcr; }
inline void set_col_vars_tab(SweepArgs& A, const double* tab) { A.S.hcr = tab; }

// Time-sliced sweeps of this form carry the penalty sums of every thread from slice to slice instead of reducing them per slice
// (k_forward of qd_col.h): [nb][COL_VARS_PEN_STRIDE] doubles - one word per thread of the workgroup (at most 768), the last word the
// uniform part.  The buffer travels in SweepArgs::kry, which only the Krylov kernels read and this form never instantiates.
constexpr int COL_VARS_PEN_STRIDE = 1024;
__host__ __device__ inline double* col_vars_pen_carry(const SweepArgs& A) { return A.kry; }
inline void set_col_vars_pen_carry(SweepArgs& A, double* buf) { A.kry = buf; }

// one variant's block as ColLean::init reads the constants (ColSysConsts of qd_col.h is the kernel-argument form)
template <int Q>
struct ColVarConsts {
  static constexpr int NP = Q * (Q - 1) / 2;
  const double* blk;
  __device__ __forceinline__ double detune(int k) const { return kload(blk + k); }
  __device__ __forceinline__ double xi(int k) const { return kload(blk + Q + k); }
  __device__ __forceinline__ double xikl(int p) const { return kload(blk + 2 * Q + p); }
  __device__ __forceinline__ double J(int p) const { return kload(blk + 2 * Q + NP + p); }
};

}  // namespace qd

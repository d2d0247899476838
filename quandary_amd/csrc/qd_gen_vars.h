// qd_gen_vars.h - the constants of a model-parameter ensemble on the general kernels (qd_device.h: k_forward_vars / k_adjoint_vars,
// one workgroup per state; qd_inst.hip with -DQD_VARS=1).
//
// The states of a launch are A.nb / A.nb_set sets of A.nb_set states as in the SETS form, a set is a variant, and every set reads the one
// control table.  The workgroup of state ic0 reads the block [detune | xi | xikl | J] of variant ic0 / nb_set from the device table of
// qd_col_vars.h (its layout and stride, rad/ns; it travels in S.hcr, which the general family reads on a dense handle only and this form
// has no dense variants).  The stencils load detune / xi / xikl once, where init() forms the diagonal of the Hamiltonian, and J where
// the coupling terms read it; the address is wave-uniform, so the loads go through the scalar path (kload) and a variant whose J of a
// pair is 0 skips that pair as the single evaluation on a handle with those constants does.  Level counts, strides, decay and dephasing
// rates and hasJ remain the handle's, in the kernel argument.
#pragma once
#include "qd_col_vars.h"

namespace qd {

template <int Q>
struct ModelK<Q, true> {
  ColVarConsts<Q> v;
  __device__ __forceinline__ void bind(const SweepArgs& A, int ic0) {
    v.blk = col_vars_tab(A) + (size_t)(ic0 / A.nb_set) * col_vars_stride(Q, ColVarConsts<Q>::NP);
  }
  __device__ __forceinline__ double detune(const DevSys&, int k) const { return v.detune(k); }
  __device__ __forceinline__ double xi(const DevSys&, int k) const { return v.xi(k); }
  __device__ __forceinline__ double xikl(const DevSys&, int p) const { return v.xikl(p); }
  __device__ __forceinline__ double J(const DevSys&, int p) const { return v.J(p); }
};

}  // namespace qd

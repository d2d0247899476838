// qd_sens.h - model-constant sensitivities inside the general adjoint sweep (k_adjoint_sens of qd_device.h: qd_adjoint_body.h compiled
// with SENS = true, objects build/qd_sens_*.o from qd_inst.hip with -DQD_SENS=1; qd_optim_evalGradF_model).  Included INSIDE namespace qd
// of qd_device.h, behind Team.
//
// The operators dM/d(detune_k), dM/d(xi_k), dM/d(xi_kl) are diagonal and time-independent: of y = M x they touch only the term
// y_re += dw x_im, y_im -= dw x_re with dw = h(I) - h(I'), h(I) = sum_k detune_k i_k - xi_k / 2 i_k (i_k - 1) - sum_{k<l} xi_kl i_k i_l
// (GenStencil::init).  With the h-scaled adjoint stage kbar and the primal stage z of a sub-step - both in registers where the control-
// gradient coefficients are formed - and w = kbar.x z.y - kbar.y z.x, an element adds w times an INTEGER to each sum:
//   detune_k   i_k - i'_k                               [k]
//   xi_k       i_k (i_k - 1) - i'_k (i'_k - 1)          [Q + k]            (the factor -1/2 of h: on the host)
//   xi_kl      i_k i_l - i'_k i'_l                      [2 Q + pair]       (the factor -1: on the host; pairs in the order of qd_system)
// (Schroedinger: no ket digits).  The sums live in NS = 2 Q + Q (Q - 1) / 2 fp64 registers per thread for the whole sweep; nothing goes
// into the per-sub-step coefficient buffer.  Everything here works from the NATURAL element index (the one evalJ_part takes) and the
// level counts and strides of DevSys, so one helper serves every stencil of the general family.

constexpr int sens_count(int q) { return 2 * q + q * (q - 1) / 2; }

// level digits of the element with natural index e, packed like the stencils' own (packed_digit_bits): bra digits, ket digits
template <int Q, bool LIND>
__device__ __forceinline__ void sens_decode(const DevSys& S, int e, unsigned& bra, unsigned& ket) {
  constexpr int DB = packed_digit_bits(Q);
  const int I = LIND ? e % S.N : e, Ip = LIND ? e / S.N : 0;
  bra = 0;
  ket = 0;
#pragma unroll
  for (int k = 0; k < Q; k++) {
    bra |= (unsigned)((I / S.post[k]) % S.n[k]) << (DB * k);
    if (LIND) ket |= (unsigned)((Ip / S.post[k]) % S.n[k]) << (DB * k);
  }
}

// acc += (integer weights of the element) x w.  The weights are rebuilt from the packed digits at every use (opaque: as fp64 loop
// invariants they would cost 2 NS registers per element).
template <int Q, bool LIND>
__device__ __forceinline__ void sens_add(unsigned bra, unsigned ket, double w, double (&acc)[sens_count(Q)]) {
  constexpr int DB = packed_digit_bits(Q);
  constexpr unsigned MASK = (1u << DB) - 1u;
  bra = opaque(bra);
  if (LIND) ket = opaque(ket);
  int a[Q], ap[Q];
#pragma unroll
  for (int k = 0; k < Q; k++) {
    a[k] = (int)((bra >> (DB * k)) & MASK);
    ap[k] = LIND ? (int)((ket >> (DB * k)) & MASK) : 0;
  }
  int pair = 0;
#pragma unroll
  for (int k = 0; k < Q; k++) {
    acc[k] = fma((double)(a[k] - ap[k]), w, acc[k]);
    acc[Q + k] = fma((double)(a[k] * (a[k] - 1) - ap[k] * (ap[k] - 1)), w, acc[Q + k]);
#pragma unroll
    for (int l = k + 1; l < Q; l++) {
      acc[2 * Q + pair] = fma((double)(a[k] * a[l] - ap[k] * ap[l]), w, acc[2 * Q + pair]);
      pair++;
    }
  }
}

// Workgroup totals of the NS sums, stored to dst[0 .. NS) by one thread.  The reduction scratch of a team holds NRED values per slot:
// the sums go through it NRED at a time (the two slots alternate, so consecutive reductions need no barrier in between).
template <int NS, int C0 = 0, typename TM>
__device__ __forceinline__ void sens_store(TM& tm, const double (&acc)[NS], double* __restrict__ dst) {
  constexpr int n = NS - C0 < NRED ? NS - C0 : NRED;
  double v[n];
#pragma unroll
  for (int i = 0; i < n; i++) v[i] = acc[C0 + i];
  tm.template sum<n>(v);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < n; i++) dst[C0 + i] = v[i];
  }
  if constexpr (C0 + n < NS) sens_store<NS, C0 + n>(tm, acc, dst);
}

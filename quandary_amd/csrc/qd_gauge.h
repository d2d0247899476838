// qd_gauge.h - phasor table of the real-drive frame of the lean column forward sweeps (qd_col.h, k_forward / ColTeam::stage, GAUGE).
//
// In that frame the drive of oscillator k of a sub-step, c_k = q_k + i p_k = r_k e^{i theta_k}, is the real number r_k, and the state is
// rotated by the diagonal unitary of the row phasors w_i = prod_k u_k^{i_k}, u_k = conj(c_k) / r_k (i_k = level of oscillator k in row i).
// Both depend on the control row of the sub-step and on the row index only - not on the initial condition, the wave or the state - so they
// are tabulated once per parameter update, next to the control table they derive from (k_gauge of qd_kernels.hip, built where k_gmat builds
// G(t) for the dense systems), and the sweep reads them: r_k through the scalar path, phasors as one 16-byte load per lane.
//
// The frame PERSISTS between sub-steps: the sweep enters it once, with w(0), and from then on the state goes from the frame of sub-step s
// straight to the frame of sub-step s + 1 through the RELATIVE phasor v_i(s) = w_i(s + 1) conj(w_i(s)) - the rotation out of s and the
// rotation into s + 1 are two diagonal unitaries back to back, applied as their product.  w(nsub) = 1: the last row's relative phasor
// returns to the lab frame.  The rule of the arithmetic: x advances through the relative phasors only; everything in the lab frame
// (trajectory rows, stored stages, penalties that read off-diagonal elements) is a by-product formed with the absolute phasor w(s) and
// never feeds back into x.
//
// Layout, per row of the control table (GAUGE_STRIDE doubles, 2112 B: every block starts on a 64-byte boundary):
//   [0, 128)    w_i(s) as (re, im), i < 64; w_i = 1 on the padding rows i >= N, so that an idle lane never reads past the block or meets a NaN
//   [128, 136)  r_k, k < Q; 0 where the drive counts as absent (r_k^2 <= 1e-280: u_k = 1), and behind the last oscillator
//   [136, 264)  v_i(s) as (re, im), i < 64: the product of the two tabulated w, renormalised like them; 1 on the padding rows
// A parameter-set batch holds one table per set, a set stride apart (launch_gauge_sets), like the control and G(t) tables; the last row
// of every set returns to the lab frame.
//
// The table reaches the kernels in the two fields of SweepArgs the dense systems use for G(t), S.gtab and gtab_set: the lean column family
// is never dense (collean_available), a dense system never runs on it, and SweepArgs keeps its size and field offsets (qd_internal.h:
// some kernels keep a copy of the struct in scratch).  Only the accessors below name the alias.
#pragma once
#include "qd_device.h"

namespace qd {

constexpr int GAUGE_LANES = 64;                    // row phasors per table row: one per lane of a wave
constexpr int GAUGE_R = 2 * GAUGE_LANES;           // offset of r_0 in a table row
constexpr int GAUGE_V = GAUGE_R + QD_MAX_OSC;      // offset of the relative phasors v_i in a table row
constexpr int GAUGE_STRIDE = GAUGE_V + 2 * GAUGE_LANES;  // doubles per table row
static_assert(GAUGE_V % 8 == 0 && GAUGE_STRIDE % 8 == 0, "table rows and their blocks start on 64-byte boundaries");

__host__ __device__ inline const double* gauge_tab(const SweepArgs& A) { return A.S.gtab; }
__host__ __device__ inline unsigned gauge_set(const SweepArgs& A) { return A.gtab_set; }  // doubles between two sets' tables
inline void set_gauge_tab(SweepArgs& A, const double* tab, unsigned set_stride) {
  A.S.gtab = tab;
  A.gtab_set = set_stride;
}

// r_k and u_k of one oscillator from its control values p, q of the sub-step.  r_k^2 below 1e-280 counts as no drive (u_k = 1, r_k = 0):
// never a NaN.
__device__ __forceinline__ double gauge_osc(double p, double q, double2& u) {
  const double r2 = fma(p, p, q * q);
  const bool on = r2 > 1e-280;
  const double ir = rsqrt_nr(on ? r2 : 1.0);
  u = on ? make_double2(q * ir, -p * ir) : make_double2(1.0, 0.0);
  return on ? r2 * ir : 0.0;
}

// Row phasor w_i of row i < 64 for the control row `ctl` ([h, t, p_0.., q_0.., ...]): binary powering of u_k over the bits of the level
// index i_k, oscillators in order, |w| renormalised once to second order (|w| = 1 to a few ulp before).  THE definition of the phasor:
// the bits every sweep reads.
__device__ __forceinline__ double2 gauge_row_phasor(const DevSys& S, const double* ctl, int i) {
  double2 w = make_double2(1.0, 0.0);
  for (int k = 0; k < S.Q; k++) {
    double2 pw;  // u_k^(2^b)
    gauge_osc(ctl[2 + k], ctl[2 + S.Q + k], pw);
    const int e = i < S.N ? (i / S.post[k]) % S.n[k] : 0;
    const int n = S.n[k];
    for (int b = 1; b < n; b <<= 1) {
      if (e & b) w = make_double2(fma(w.x, pw.x, -w.y * pw.y), fma(w.x, pw.y, w.y * pw.x));
      pw = make_double2(fma(pw.x, pw.x, -pw.y * pw.y), 2.0 * pw.x * pw.y);
    }
  }
  const double nr = fma(-0.5, fma(w.x, w.x, w.y * w.y), 1.5);  // 1 / |w| to second order
  return make_double2(w.x * nr, w.y * nr);
}

// Relative phasor v_i(s) = w_i(s + 1) conj(w_i(s)) from the two tabulated row phasors (wn = w(s + 1), or 1 behind the last row),
// renormalised the same way: the bits every sweep reads.
__device__ __forceinline__ double2 gauge_rel_phasor(const double2 w, const double2 wn) {
  const double2 v = make_double2(fma(wn.x, w.x, wn.y * w.y), fma(wn.y, w.x, -wn.x * w.y));
  const double nr = fma(-0.5, fma(v.x, v.x, v.y * v.y), 1.5);
  return make_double2(v.x * nr, v.y * nr);
}

// the table of every row of a control table (qd_kernels.hip); the SETS form: set j reads table + j * ctl_set and writes gauge + j * gauge_set
hipError_t launch_gauge(const DevSys& S, const double* table, int cs, int nrows, double* gauge, hipStream_t st);
hipError_t launch_gauge_sets(const DevSys& S, const double* table, size_t ctl_set, int cs, int nrows, double* gauge, size_t gauge_set, int nset,
                             hipStream_t st);

}  // namespace qd

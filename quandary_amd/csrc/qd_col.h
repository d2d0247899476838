// qd_col.h - device code and launchers of the lean column kernels, shared by every translation unit of the family.  Layout and reference
// semantics: the comment at the top of qd_col.hip.
//
// A unit is this file compiled for one (form, coupling); both come from the compile line and default to the plain unit without coupling:
//   QD_COL_FORM  a value of qd::Form (QD_FORM_* of qd_internal.h)                                default QD_FORM_PLAIN
//   QD_COL_HJ    1: systems with dipole-dipole coupling (any J_kl != 0), 0: systems without        default 0
// The kernels are defined here, once per unit, as __global__ templates over <Q, EPT, SPLIT, USLOT, SKIP, KRY> / <Q, EPT, SPLIT>; form and
// coupling are part of the kernel's NAME (QD_COLK below), not template arguments of it.  So are their launchers (the end of this file):
// which instantiation a sweep runs is written once, for every unit and both directions.
//
// The units: qd_col.hip and qd_colj.hip are the plain ones, each one object with every <Q, EPT>, the operator application and (qd_col.hip)
// the family's entry points.  Every other unit is qd_col_form.hip compiled once per <Q, EPT> (objects qd_col_sets_3_5.o, ... - they
// compile side by side), and a form differs from the plain one in the device code only where an #if on QD_COL_FORM says so; with
// the plain form this file preprocesses to the text it had before the forms existed.
//   Sets  k_*_col_sets / k_*_colj_sets: the stationary-iteration sweeps, compiled a second time (16 kernels per object without coupling,
//         4 with).  The task of initial condition ic reads its step rows from the control table of set ic / SweepArgs::nb_set
//         (parameter-set batch, qd_optim_evalGradF_batch with option batch_lean), the addressing sweep_ctl<true> of qd_device.h gives the
//         general kernels: wave-uniform, so the rows stay scalar loads.  Trajectory, primal stages, coefficients, carry buffers and
//         scheduler words stay indexed by ic.  The table address and the kernel names are the only places where the device code differs;
//         with coupling, the pair columns cos / sin(eta_kl t) widen a table row, not the addressing.
//   Vars  k_*_col_vars / k_*_colj_vars: one block of model constants per variant (model-parameter ensemble,
//         qd_optim_evalGradF_ensemble_model; 8 kernels per object without coupling, 4 with).  The task of initial condition ic belongs to
//         variant ic / SweepArgs::nb_set: it reads that variant's control and phasor tables as the Sets form does, and its detunings,
//         Kerr coefficients and couplings from the device table of qd_col_vars.h through the scalar path.  Everything ColLean::init
//         derives from those constants is derived again, by the same text, when a workgroup's task belongs to another variant than its
//         previous one (col_vars_enter below).  A variant whose couplings are all zero runs on the coupled unit too, with zero weights.
//   Sens  k_adjoint_col_sens / k_adjoint_colj_sens: the ADJOINT sweep with the model-constant sensitivities (qd_optim_evalGradF_model
//         with option sens_lean; 4 kernels per object without coupling, 2 with).  dM/d theta of a detuning, a self-Kerr or a cross-Kerr
//         coefficient is diagonal and time-independent, so d objective / d theta is a weighted sum over the elements of W[e] = sum over
//         the sub-steps of kbar_e.x z_e.y - kbar_e.y z_e.x, with the integer weights of qd_sens.h.  A thread keeps W of its EPT elements
//         in fp64 registers across the time loop - two fma per element and sub-step where kbar and z are at hand, nothing per constant -
//         and weights, reduces and stores the sens_count(Q) sums once per task, to the task's own row of SweepArgs::S.tred
//         [nslice][nb][sens_count(Q)] (no atomics: the host adds the rows in a fixed order).  The coupling has no part in dM/d theta: the
//         coupled unit forms the same sums from its own kbar and z.  The forward sweep of the call is the plain kernel.
//   Pair  k_forward_col_pair: the FORWARD sweep on Hermitian pairs (option pair_hermitian; 8 kernels per object).  The Lindblad operator
//         is complex-linear on vec(rho) and maps Hermitian to Hermitian, and so is every step of the stationary solve: state ic of the
//         launch is X = rho_a + i rho_b of two Hermitian initial conditions, and the kernel propagates it like any other state.  The form
//         differs from the plain one in the per-time-step penalty block alone, which sums the two members apart - their diagonals are
//         the real and the imaginary part of X's - and in the two results it writes per state, pen_out[2 ic] and pen_out[2 ic + 1].
// What is built of each form: the properties below.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "qd_col_vars.h"
#include "qd_device.h"
#include "qd_gauge.h"

#ifndef QD_COL_FORM
#define QD_COL_FORM QD_FORM_PLAIN
#endif
#ifndef QD_COL_HJ
#define QD_COL_HJ 0
#endif
// A kernel of the unit: QD_COLK(k_forward) = k_forward_col, k_forward_colj_sets, ... (k_forward, k_adjoint, k_apply)
#if QD_COL_HJ
#define QD_COL_HJ_TAG _colj
#else
#define QD_COL_HJ_TAG _col
#endif
#if QD_COL_FORM == QD_FORM_PLAIN
#define QD_COL_FORM_TAG
#elif QD_COL_FORM == QD_FORM_SETS
#define QD_COL_FORM_TAG _sets
#elif QD_COL_FORM == QD_FORM_VARS
#define QD_COL_FORM_TAG _vars
#elif QD_COL_FORM == QD_FORM_SENS
#define QD_COL_FORM_TAG _sens
#elif QD_COL_FORM == QD_FORM_PAIR
#define QD_COL_FORM_TAG _pair
#else
#error "QD_COL_FORM: a value of qd::Form"
#endif
#define QD_COL_CAT_(a, b, c) a##b##c
#define QD_COL_CAT(a, b, c) QD_COL_CAT_(a, b, c)
#define QD_COLK(base) QD_COL_CAT(base, QD_COL_HJ_TAG, QD_COL_FORM_TAG)
// (col_per_set below, for the preprocessor: the table addresses are macros)
#define QD_COL_PER_SET (QD_COL_FORM == QD_FORM_SETS || QD_COL_FORM == QD_FORM_VARS)
#if QD_COL_PER_SET
#define QD_COL_CTL(A, ic) (A.ctl + (size_t)((unsigned)(ic) / (unsigned)A.nb_set) * A.ctl_set)
#define QD_COL_GAUGE_TAB(A, ic) (gauge_tab(A) + (size_t)((unsigned)(ic) / (unsigned)A.nb_set) * gauge_set(A))
#else
#define QD_COL_CTL(A, ic) A.ctl
#define QD_COL_GAUGE_TAB(A, ic) gauge_tab(A)
#endif

namespace qd {

// What the unit's form is, stated once: every test below names one of these (or, in device code, one form)
constexpr Form col_form = (Form)QD_COL_FORM;
constexpr bool col_coupled = QD_COL_HJ != 0;
constexpr bool col_per_set = QD_COL_PER_SET;                                    // reads the control and phasor tables of the task's set
constexpr bool col_per_variant = col_form == Form::Vars;                        // ... and the model constants of its variant
constexpr bool col_has_forward = col_form != Form::Sens;                        // the forward kernel is built
constexpr bool col_has_adjoint = col_form != Form::Pair;                        // the adjoint kernel is built
constexpr bool col_has_krylov = col_form == Form::Plain;                        // the Krylov instantiation (KRY = true)
// the plain-Neumann instantiations (SPLIT = false); every unit has the diagonal-split ones
constexpr bool col_has_plain_neumann = !col_coupled && (col_form == Form::Plain || col_form == Form::Sets || col_form == Form::Pair);
constexpr bool col_has_apply = col_form == Form::Plain;                         // the operator application
static_assert(!(col_coupled && col_form == Form::Pair), "no pair form of the coupled kernels: a unit that is not built");

constexpr unsigned COLB = 1024;  // bytes per padded column: 64 rows x 16 B
// Krylov solver of these kernels (ColTeam::kry_*): restart length.  Basis V[0 .. MR], preconditioned basis Z[0 .. MR - 1], the parked
// right-hand side, the parked total of a restart and the parked state: 2 MR + 4 = 32 vectors = the GMRES_MR_G + 2 slots per workgroup of
// SweepArgs::kry (krylov_doubles)
constexpr int KRY_MR = 14;
constexpr int KRY_NSC = gmres_nsc(KRY_MR);
constexpr size_t KRY_VEC = 64 * 64;  // double2 per scratch vector of a workgroup: the padded column layout (64 rows x at most 64 columns)
static_assert(2 * KRY_MR + 4 <= GMRES_MR_G + 2, "slots of the global-memory Krylov buffer");

// Largest workgroup of the EPT-columns-per-wave kernels = their register budget: 16 waves x 128, 12 x 168 (five columns per wave
// cover N <= 60), 11 x 168, 8 x 256 VGPRs
constexpr int col_max_threads(int ept) { return ept == 5 ? 768 : 64 * ((64 + ept - 1) / ept); }

__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Ket class of a wave by the level i'_0 of oscillator 0 that all its columns share (USLOT): at the bottom level there is no ket-down
// neighbour of oscillator 0, at the top level no ket-up neighbour and no T1 term.  KET_NONE: nothing known, every term is formed.
enum : int { KET_NONE = 0, KET_BOTTOM = 1, KET_INTERIOR = 2, KET_TOP = 3 };
// Wave order of the class-form forward kernel (ColTeam's KCLS): 0 = plain, 1 = one wave of every class per SIMD (COLFLAGS; measured
// slower on the 3 x 20 headline, 541.7 against 535.8 ms, profiles/ketedge_ab.txt: not the default)
#ifndef QD_COL_KET_PERMUTE
#define QD_COL_KET_PERMUTE 0
#endif
// Forward stage solve of the diagonal-split stationary solver without coupling in the frame where every drive coefficient is real
// (ColTeam::stage, GAUGE): 1 = on; 0 (COLFLAGS) = the complex form everywhere, the code this file had before the form existed
#ifndef QD_COL_GAUGE
#define QD_COL_GAUGE 1
#endif
// Where the frame change takes the relative phasors of the wave's COLUMNS from: 1 = the table row through the scalar path (the columns
// of a wave's slots are contiguous there and their address is wave-uniform, like r_k); 0 = lanes of the row-phasor register (four
// v_readlane per slot)
#ifndef QD_COL_GAUGE_SCOL
#define QD_COL_GAUGE_SCOL 1
#endif

// The model constants ColLean::init derives a kernel's values from, read from the kernel argument (every form but Vars)
struct ColSysConsts {
  const DevSys& S;
  __device__ __forceinline__ double detune(int k) const { return S.detune[k]; }
  __device__ __forceinline__ double xi(int k) const { return S.xi[k]; }
  __device__ __forceinline__ double xikl(int p) const { return S.xikl[p]; }
  __device__ __forceinline__ double J(int p) const { return S.J[p]; }
};

// SPLIT: the kernels of the diagonal-split solver keep (1 - alpha D)^-1 per element instead of the diagonal itself; the diagonal is then
// re-derived where the full operator is applied (once or twice per step) from a row part held by the thread and a column part in LDS
// USLOT: every column of a wave has the same level indices i'_k of the oscillators k < L (post[k] a multiple of EPT, no idle columns):
// the byte offsets to the ket neighbour columns are then one pair per oscillator instead of one per slot, and the compiler forms each
// neighbour address once per application instead of once per slot (12 of 300 vector instructions of a solver iteration on 3 x 20).
// HJ: the dipole-dipole coupling terms J_kl (a^dag_k a_l e^{i eta t} + h.c.) of every pair k < l (mastereq.hpp:632-741).  They have no
// diagonal entry: part of the off-diagonal operator C = M - D, and the diagonal-split solver's D is untouched.
template <int Q, int EPT, bool SPLIT = false, bool USLOT = false, bool HJ = false>
struct ColLean {
  static constexpr int L = Q - 1;  // the stride-1 oscillator (post[Q-1] == 1)
  static constexpr int NP = Q * (Q - 1) / 2, NPJ = HJ ? NP : 1;  // oscillator pairs (k, l), k < l, in the order of DevSys::J
  // thread invariants (functions of the row)
  double su[Q], sd[Q];    // sqrt(i_k + 1) (0 at the top level), sqrt(i_k)
  double g1u[Q], g1d[Q];  // gamma_1 su / gamma_1 sd: thread part of the T1 off-diagonal coefficient, forward / transposed
  double dw[SPLIT ? 1 : EPT], dd[SPLIT ? 1 : EPT];  // Delta = h(I) - h(I'), d = L2 + L1diag of the element in slot j (mastereq.hpp:316-433)
  double hrow, drow, g2ia[Q];  // SPLIT: h(I), the row part of d, gamma_2 i_k
  unsigned ctb;                // SPLIT: LDS byte address of the wave's first entry of the column table (h(I'), column part of d, i'_k)
  unsigned tb;              // LDS byte address of (row, first column of the wave) in the buffer being READ
  unsigned aru[Q], ard[Q];  // the same with the row moved up / down by post[k] where that bra neighbour exists (else tb)
  int dlt;                  // byte distance from the buffer being read to the other one (+- bufbytes)
  // HJ, per pair (k, l): J_kl sqrt(i_k) sqrt(i_l + 1) and J_kl sqrt(i_l) sqrt(i_k + 1), and tb with the row moved by -post[k] + post[l] /
  // +post[k] - post[l] where that bra neighbour exists (else weight 0 and tb itself)
  double sj1[NPJ], sj2[NPJ];
  unsigned aj1[NPJ], aj2[NPJ];
  // wave-uniform (functions of the wave's columns; scalar registers)
  double cx[EPT][Q], cy[EPT][Q];  // sqrt(i'_k + 1) (0 at the top level), sqrt(i'_k) of the column of slot j
  int ocu[USLOT ? 1 : EPT][Q], ocd[USLOT ? 1 : EPT][Q];  // byte offset to the ket neighbour column up / down (0 where there is none)
  // HJ, per slot and pair: the same two weights in the ket level indices and the byte offsets to those two columns (0 where there is none)
  double kj3[HJ ? EPT : 1][NPJ], kj4[HJ ? EPT : 1][NPJ];
  int oj3[HJ ? EPT : 1][NPJ], oj4[HJ ? EPT : 1][NPJ];
  // (USLOT: a pair without the stride-1 oscillator has the same ket levels in every column of the wave - one set instead of one per slot)
  static __device__ __forceinline__ constexpr int uj(int j, int pair) { return (USLOT && Q == 3 && pair == 0) ? 0 : j; }
  static __device__ __forceinline__ constexpr int us(int j) { return USLOT ? 0 : j; }
  // (USLOT: the level indices of the oscillators k < L are the same in every column of the wave, hence their square roots too - one
  //  scalar pair per oscillator instead of one per slot: 16 scalar registers less on 3 x 20, where the adjoint sweep spills ~160)
  __device__ __forceinline__ double cxv(int j, int k) const { return cx[(USLOT && k != L) ? 0 : j][k]; }
  // (USLOT, stride-1 oscillator: the columns of a wave are consecutive levels i', i' + 1, ... of it, so sqrt(i'_j) = sqrt(i'_{j-1} + 1):
  //  the down coefficient of slot j is the up coefficient of slot j - 1 - four more scalar pairs less: 594.9 -> 592.5 ms, gradient
  //  1209 -> 1202 ms in one lease)
  __device__ __forceinline__ double cyv(int j, int k) const {
    if (USLOT && k == L && j > 0) return cx[j - 1][k];
    return cy[(USLOT && k != L) ? 0 : j][k];
  }
  int N, row, col0;
  bool rowok;
  unsigned char* smem;

  __device__ __forceinline__ double2 ld(unsigned a) const { return *reinterpret_cast<const double2*>(smem + a); }
  __device__ __forceinline__ void st(unsigned a, const double2 v) const { *reinterpret_cast<double2*>(smem + a) = v; }
  __device__ __forceinline__ int colof(int j) const { return col0 + j; }
  __device__ __forceinline__ bool colok(int j) const { return col0 + j < N; }
  __device__ __forceinline__ bool ok(int j) const { return rowok && colok(j); }
  __device__ __forceinline__ int elem(int j) const { return (col0 + j) * N + row; }  // vectorised index (valid slots only)
  // the same, re-derived at the point of use: hoisted out of the time loop the per-slot indices are spilt and every global access
  // of a step starts with a scratch reload
  __device__ __forceinline__ int elem_now(int j) const { return (col0 + j) * N + opaque(row); }
  static __host__ __device__ int ncols(int N) { return (N + EPT - 1) / EPT * EPT; }
  static __host__ __device__ unsigned bufbytes(int N) { return (unsigned)ncols(N) * COLB; }
  static __host__ __device__ unsigned tab_off(int N) { return 2 * bufbytes(N) + 2 * (unsigned)sizeof(double) * NRED * (unsigned)(ncols(N) / EPT) + 128; }
  static size_t lds_bytes(int N) { return (size_t)tab_off(N) + 48 * (size_t)ncols(N); }

  // PERM (USLOT): wave w takes the column block EPT (w / n_0) of level w % n_0 of oscillator 0 - consecutive waves, which share a SIMD
  // every fourth, are of different ket classes
  // K: where the model constants (detuning, self- and cross-Kerr coefficients, couplings) are read - the kernel argument (ColSysConsts),
  // or one variant's block of the constants table (ColVarConsts of qd_col_vars.h, the third form).
  // FIRST = false: only what depends on those constants is derived again, for another variant - hrow, the column table, dw, the
  // coupling weights sj1 / sj2 / kj3 / kj4 and the address offsets aj1 / aj2 / oj3 / oj4 a non-zero weight selects - by THIS text: every
  // element gets the bits the plain kernel computes.  The caller holds the workgroup at a barrier before (the column table is rewritten)
  // and after, and resets ColTeam::palpha.
  template <bool PERM = false, bool FIRST = true, class KC = ColSysConsts>
  __device__ __forceinline__ void init(const DevSys& S, unsigned char* sm, const KC& K) {
    const int lane = threadIdx.x & 63;
    if constexpr (FIRST) {
      smem = sm;
      N = S.N;
      const int w = uniform_i((int)(threadIdx.x >> 6));
      col0 = w * EPT;
      if constexpr (PERM) {
        const int n0 = S.n[0];
        if ((int)(blockDim.x >> 6) % n0 == 0) col0 = uniform_i(S.post[0] * (w % n0) + EPT * (w / n0));
      }
      row = lane;
      rowok = lane < N;
      // zero the exchange buffers once: padding rows and idle columns are read (with zero coefficients) and must stay finite
      {
        const unsigned total = 2 * bufbytes(N);
        for (unsigned a = threadIdx.x * 16u; a < total; a += blockDim.x * 16u) st(a, make_double2(0.0, 0.0));
      }
      tb = (unsigned)col0 * COLB + (unsigned)lane * 16u;
      dlt = (int)bufbytes(N);
    }
    int ia[Q];
    double hd = 0.0;  // h(I)
#pragma unroll
    for (int k = 0; k < Q; k++) {
      ia[k] = rowok ? (row / S.post[k]) % S.n[k] : 0;
      if constexpr (FIRST) {
        su[k] = (rowok && ia[k] < S.n[k] - 1) ? sqrt((double)(ia[k] + 1)) : 0.0;
        sd[k] = rowok ? sqrt((double)ia[k]) : 0.0;
        g1u[k] = S.g1off[k] * su[k];
        g1d[k] = S.g1off[k] * sd[k];
        aru[k] = tb + (su[k] != 0.0 ? (unsigned)S.post[k] * 16u : 0u);
        ard[k] = tb - (sd[k] != 0.0 ? (unsigned)S.post[k] * 16u : 0u);
      }
    }
    if constexpr (HJ) {
      int pair = 0;
#pragma unroll
      for (int k = 0; k < Q; k++) {
#pragma unroll
        for (int l = k + 1; l < Q; l++, pair++) {
          // (a non-zero weight means 0 < i_k and i_l < n_l - 1, resp. 0 < i_l and i_k < n_k - 1: the neighbour row is inside the column)
          sj1[pair] = K.J(pair) * sd[k] * su[l];
          sj2[pair] = K.J(pair) * sd[l] * su[k];
          const unsigned d = (unsigned)(S.post[l] - S.post[k]) * 16u;
          aj1[pair] = tb + (sj1[pair] != 0.0 ? d : 0u);
          aj2[pair] = tb - (sj2[pair] != 0.0 ? d : 0u);
        }
      }
    }
    {
      int pair = 0;
#pragma unroll
      for (int k = 0; k < Q; k++) {
        hd += K.detune(k) * ia[k] - K.xi(k) / 2.0 * ia[k] * (ia[k] - 1);
#pragma unroll
        for (int l = k + 1; l < Q; l++) hd -= K.xikl(pair++) * ia[k] * ia[l];
      }
    }
    hrow = rowok ? hd : 0.0;
    if constexpr (FIRST) {
      drow = 0.0;
#pragma unroll
      for (int k = 0; k < Q; k++) {
        drow -= 0.5 * S.g2[k] * ia[k] * ia[k] + 0.5 * S.g1[k] * ia[k];
        g2ia[k] = rowok ? S.g2[k] * ia[k] : 0.0;
      }
      if (!rowok) drow = 0.0;
      ctb = tab_off(N) + (unsigned)col0 * 48u;
    }
    if (SPLIT) {  // column table: (h(I'), column part of d), (i'_0, i'_1), (i'_2, 0); zeros for idle columns
      for (int cc = threadIdx.x; cc < ncols(N); cc += blockDim.x) {
        double hc = 0.0, dc = 0.0, ip[3] = {0.0, 0.0, 0.0};
        if (cc < N) {
          int ipa[Q], pair = 0;
#pragma unroll
          for (int k = 0; k < Q; k++) ipa[k] = (cc / S.post[k]) % S.n[k];
#pragma unroll
          for (int k = 0; k < Q; k++) {
            hc += K.detune(k) * ipa[k] - K.xi(k) / 2.0 * ipa[k] * (ipa[k] - 1);
            dc -= 0.5 * S.g2[k] * ipa[k] * ipa[k] + 0.5 * S.g1[k] * ipa[k];
            ip[k] = (double)ipa[k];
#pragma unroll
            for (int l = k + 1; l < Q; l++) hc -= K.xikl(pair++) * ipa[k] * ipa[l];
          }
        }
        double2* t = reinterpret_cast<double2*>(smem + tab_off(N) + (unsigned)cc * 48u);
        t[0] = make_double2(hc, dc);
        t[1] = make_double2(ip[0], ip[1]);
        t[2] = make_double2(ip[2], 0.0);
      }
    }
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      const int cc = col0 + j;
      const bool cok = cc < N;
      int ipa[Q];
      double hdp = 0.0, d = 0.0;
      int pair = 0;
#pragma unroll
      for (int k = 0; k < Q; k++) ipa[k] = cok ? (cc / S.post[k]) % S.n[k] : 0;
#pragma unroll
      for (int k = 0; k < Q; k++) {
        hdp += K.detune(k) * ipa[k] - K.xi(k) / 2.0 * ipa[k] * (ipa[k] - 1);
        d += S.g2[k] * (ia[k] * ipa[k] - 0.5 * (ia[k] * ia[k] + ipa[k] * ipa[k])) - S.g1[k] / 2.0 * (ia[k] + ipa[k]);
#pragma unroll
        for (int l = k + 1; l < Q; l++) hdp -= K.xikl(pair++) * ipa[k] * ipa[l];
        if constexpr (FIRST) {
          const bool up = cok && ipa[k] < S.n[k] - 1, dn = cok && ipa[k] > 0;
          cx[j][k] = to_scalar(up ? sqrt((double)(ipa[k] + 1)) : 0.0);
          cy[j][k] = to_scalar(dn ? sqrt((double)ipa[k]) : 0.0);
          if (!USLOT || j == 0 || k == L) {
            // (USLOT: the offsets of the stride-1 oscillator are only used at the two edge slots, whose neighbours are not in registers:
            //  the up offset of the last slot, the down offset of the first)
            if (!USLOT || k != L || j == 0) ocd[us(j)][k] = uniform_i(dn ? -S.post[k] * (int)COLB : 0);
            if (!USLOT || k != L || j == EPT - 1 || EPT == 1) ocu[us(j)][k] = uniform_i(up ? S.post[k] * (int)COLB : 0);
          }
        }
      }
      if constexpr (HJ) {
        int pj = 0;
#pragma unroll
        for (int k = 0; k < Q; k++) {
#pragma unroll
          for (int l = k + 1; l < Q; l++, pj++) {
            if (uj(j, pj) != j) continue;
            const double w3 = K.J(pj) * cy[j][k] * cx[j][l], w4 = K.J(pj) * cy[j][l] * cx[j][k];
            kj3[j][pj] = to_scalar(w3);
            kj4[j][pj] = to_scalar(w4);
            oj3[j][pj] = uniform_i(w3 != 0.0 ? (S.post[l] - S.post[k]) * (int)COLB : 0);
            oj4[j][pj] = uniform_i(w4 != 0.0 ? (S.post[k] - S.post[l]) * (int)COLB : 0);
          }
        }
      }
      const bool live = rowok && cok;
      if (!SPLIT) {
        dw[j] = live ? hd - hdp : 0.0;
        if (FIRST) dd[j] = live ? d : 0.0;
      }
    }
  }
  template <bool PERM = false>
  __device__ __forceinline__ void init(const DevSys& S, unsigned char* sm) {
    init<PERM, true>(S, sm, ColSysConsts{S});
  }

  // diagonal of M at the element in slot j: (Delta, d)
  __device__ __forceinline__ void diag(int j, double& dwj, double& ddj) const {
    if (!SPLIT) {
      dwj = dw[j];
      ddj = dd[j];
    } else {
      const double2 t0 = ld(ctb + (unsigned)j * 48u), t1 = ld(ctb + (unsigned)j * 48u + 16u);
      dwj = hrow - t0.x;
      double d = drow + t0.y;
      d = fma(g2ia[0], t1.x, d);
      if (Q > 1) d = fma(g2ia[Q > 1 ? 1 : 0], t1.y, d);
      if (Q > 2) d = fma(g2ia[Q > 2 ? 2 : 0], ld(ctb + (unsigned)j * 48u + 32u).x, d);
      ddj = rowok ? d : 0.0;
      if (!rowok) dwj = 0.0;
    }
  }

  // the other buffer becomes the one being read
  __device__ __forceinline__ void flip() {
    tb += (unsigned)dlt;
#pragma unroll
    for (int k = 0; k < Q; k++) {
      aru[k] += (unsigned)dlt;
      ard[k] += (unsigned)dlt;
    }
    if constexpr (HJ) {
#pragma unroll
      for (int p = 0; p < NP; p++) {
        aj1[p] += (unsigned)dlt;
        aj2[p] += (unsigned)dlt;
      }
    }
    dlt = -dlt;
  }

  // the four ladder neighbours of oscillator k of the element in slot j: bra up / down (xu, xd), ket up / down (xup, xdp);
  // own / prev / next = the thread's elements of the vector being read in slots j, j - 1, j + 1
  __device__ __forceinline__ void nbrs(int k, int j, const double2 own, const double2 prev, const double2 next, double2& xu, double2& xd,
                                       double2& xup, double2& xdp) const {
    if (k == L) {
      xu = lane_shift<true>(own);
      xd = lane_shift<false>(own);
      xup = j < EPT - 1 ? next : ld(tb + (unsigned)ocu[us(j)][k] + (unsigned)j * COLB);
      xdp = j > 0 ? prev : ld(tb + (unsigned)ocd[us(j)][k] + (unsigned)j * COLB);
    } else {
      xu = ld(aru[k] + (unsigned)j * COLB);
      xd = ld(ard[k] + (unsigned)j * COLB);
      xup = ld(tb + (unsigned)ocu[us(j)][k] + (unsigned)j * COLB);
      xdp = ld(tb + (unsigned)ocd[us(j)][k] + (unsigned)j * COLB);
    }
  }

  // y = M x (TRANS = false) or M^T x at slot j (ColStencil::apply of qd_device.h; its S.hasJ block = HJ here)
  // NODIAG: only the off-diagonal part C = M - diag(M) (the diagonal-split solver applies the diagonal in closed form)
  // acc: added to the result (the accumulators start there: no extra instruction)
  // KC: ket class of the wave (forward NODIAG form only): the terms of oscillator 0 that the class does not have are not formed
  // RD: real drive (forward NODIAG form without coupling, on a vector in the rotated frame of ColTeam::stage): the coefficient of
  // oscillator k is the real number c.q[k] (= alpha r_k there; c.p[k] is not read) on e + f - one sum of the four ladder neighbours
  // and one fma per component instead of e, f and four: 10 fp64 instructions per oscillator and element instead of 16
  template <bool TRANS, bool NODIAG = false, int KC = KET_NONE, bool RD = false>
  __device__ __forceinline__ double2 apply(const StepC<Q>& c, int j, const double2 own, const double2 prev, const double2 next,
                                           const double2* acc = nullptr) const {
    static_assert(KC == KET_NONE || (!TRANS && NODIAG && USLOT && !HJ && Q > 1), "class forms: the forward stage pass");
    static_assert(!RD || (!TRANS && NODIAG && !HJ), "real drive: the forward stage pass without coupling");
    double ar = acc ? acc->x : 0.0, ai = acc ? acc->y : 0.0;
    if (!NODIAG) {
      double dwj, ddj;
      diag(j, dwj, ddj);
      if (TRANS) dwj = -dwj;
      ar = fma(dwj, own.y, acc ? fma(ddj, own.x, ar) : ddj * own.x);
      ai = fma(-dwj, own.x, acc ? fma(ddj, own.y, ai) : ddj * own.y);
    }
    if constexpr (KC != KET_NONE) {
      // oscillator 0 of a wave of known class (never the stride-1 oscillator): the bra neighbours, the ket neighbours there are, and
      // the T1 term with the coefficient set_alpha has formed whole
      const double2 xu = ld(aru[0] + (unsigned)j * COLB), xd = ld(ard[0] + (unsigned)j * COLB);
      if constexpr (RD) {
        double sr = fma(-sd[0], xd.x, su[0] * xu.x), si = fma(-sd[0], xd.y, su[0] * xu.y);  // e + f
        if constexpr (KC != KET_BOTTOM) {
          const double2 xdp = ld(tb + (unsigned)ocd[0][0] + (unsigned)j * COLB);
          sr = fma(-cy[0][0], xdp.x, sr);
          si = fma(-cy[0][0], xdp.y, si);
        }
        if constexpr (KC != KET_TOP) {
          const double2 xup = ld(tb + (unsigned)ocu[0][0] + (unsigned)j * COLB);
          sr = fma(cx[0][0], xup.x, sr);
          si = fma(cx[0][0], xup.y, si);
        }
        ar = fma(c.q[0], sr, ar);
        ai = fma(c.q[0], si, ai);
      } else {
        double er = su[0] * xu.x, ei = su[0] * xu.y;     // U1 - D2
        double fr = -sd[0] * xd.x, fi = -sd[0] * xd.y;  // U2 - D1
        if constexpr (KC != KET_BOTTOM) {
          const double2 xdp = ld(tb + (unsigned)ocd[0][0] + (unsigned)j * COLB);
          er = fma(-cy[0][0], xdp.x, er);
          ei = fma(-cy[0][0], xdp.y, ei);
        }
        if constexpr (KC != KET_TOP) {
          const double2 xup = ld(tb + (unsigned)ocu[0][0] + (unsigned)j * COLB);
          fr = fma(cx[0][0], xup.x, fr);
          fi = fma(cx[0][0], xup.y, fi);
        }
        ar = fma(c.q[0], er + fr, fma(c.p[0], ei - fi, ar));
        ai = fma(c.q[0], ei + fi, fma(-c.p[0], er - fr, ai));
      }
      if constexpr (KC != KET_TOP) {  // T1 off-diagonal term (the top class has none)
        const double2 xl = ld(aru[0] + (unsigned)ocu[0][0] + (unsigned)j * COLB);
        ar = fma(g1u[0], xl.x, ar);
        ai = fma(g1u[0], xl.y, ai);
      }
    }
#pragma unroll
    for (int k = KC != KET_NONE ? 1 : 0; k < Q; k++) {
      double2 xu, xd, xup, xdp;
      nbrs(k, j, own, prev, next, xu, xd, xup, xdp);
      if constexpr (RD) {
        const double sr = fma(cxv(j, k), xup.x, fma(-cyv(j, k), xdp.x, fma(-sd[k], xd.x, su[k] * xu.x)));  // e + f
        const double si = fma(cxv(j, k), xup.y, fma(-cyv(j, k), xdp.y, fma(-sd[k], xd.y, su[k] * xu.y)));
        ar = fma(c.q[k], sr, ar);
        ai = fma(c.q[k], si, ai);
      } else {
        const double er = fma(-cyv(j, k), xdp.x, su[k] * xu.x), ei = fma(-cyv(j, k), xdp.y, su[k] * xu.y);  // U1 - D2
        const double fr = fma(cxv(j, k), xup.x, -sd[k] * xd.x), fi = fma(cxv(j, k), xup.y, -sd[k] * xd.y);  // U2 - D1
        const double pk = TRANS ? -c.p[k] : c.p[k], qk = TRANS ? -c.q[k] : c.q[k];
        ar = fma(qk, er + fr, fma(pk, ei - fi, ar));
        ai = fma(qk, ei + fi, fma(-pk, er - fr, ai));
      }
      // T1 off-diagonal term: forward couples to (row + s, column + s), transposed to (row - s, column - s)
      double2 xl;
      if (k == L) {
        if (TRANS) xl = j > 0 ? lane_shift<false>(prev) : ld(ard[k] + (unsigned)ocd[us(j)][k] + (unsigned)j * COLB);
        else xl = j < EPT - 1 ? lane_shift<true>(next) : ld(aru[k] + (unsigned)ocu[us(j)][k] + (unsigned)j * COLB);
      } else {
        xl = TRANS ? ld(ard[k] + (unsigned)ocd[us(j)][k] + (unsigned)j * COLB) : ld(aru[k] + (unsigned)ocu[us(j)][k] + (unsigned)j * COLB);
      }
      const double l1 = TRANS ? g1d[k] * cyv(j, k) : g1u[k] * cxv(j, k);
      ar = fma(l1, xl.x, ar);
      ai = fma(l1, xl.y, ai);
    }
    if constexpr (HJ) {
      // dipole-dipole coupling of pair (k, l): x1, x2 the bra neighbours (same column), x3, x4 the ket neighbours (same row); with
      // a = w1 x1 - w2 x2 + w3 x3 - w4 x4, b = w1 x1 + w2 x2 - w3 x3 - w4 x4 (the weights carry J_kl) the term is
      // (sin a_re + cos b_im, sin a_im - cos b_re), part of the Hamiltonian: opposite sign in the transposed operator, like p and q
#pragma unroll
      for (int p = 0; p < NP; p++) {
        const double2 x1 = ld(aj1[p] + (unsigned)j * COLB), x2 = ld(aj2[p] + (unsigned)j * COLB);
        const double2 x3 = ld(tb + (unsigned)oj3[uj(j, p)][p] + (unsigned)j * COLB), x4 = ld(tb + (unsigned)oj4[uj(j, p)][p] + (unsigned)j * COLB);
        const double w3 = kj3[uj(j, p)][p], w4 = kj4[uj(j, p)][p];
        const double ur = fma(-w4, x4.x, sj1[p] * x1.x), ui = fma(-w4, x4.y, sj1[p] * x1.y);  // w1 x1 - w4 x4
        const double vr = fma(-w3, x3.x, sj2[p] * x2.x), vi = fma(-w3, x3.y, sj2[p] * x2.y);  // w2 x2 - w3 x3
        const double co = TRANS ? -c.cs[p] : c.cs[p], si = TRANS ? -c.sn[p] : c.sn[p];
        ar = fma(si, ur - vr, fma(co, ui + vi, ar));
        ai = fma(si, ui - vi, fma(-co, ur + vr, ai));
      }
    }
    return make_double2(ar, ai);
  }

  // gradient contraction (ColStencil::ladder): A = e + f, B = e - f with e = U1 - D2, f = U2 - D1 of the published vector
  __device__ __forceinline__ void ladder(int k, int j, const double2 own, const double2 prev, const double2 next, double2& A, double2& B) const {
    double2 xu, xd, xup, xdp;
    nbrs(k, j, own, prev, next, xu, xd, xup, xdp);
    const double er = fma(-cyv(j, k), xdp.x, su[k] * xu.x), ei = fma(-cyv(j, k), xdp.y, su[k] * xu.y);
    const double fr = fma(cxv(j, k), xup.x, -sd[k] * xd.x), fi = fma(cxv(j, k), xup.y, -sd[k] * xd.y);
    A.x = er + fr;
    A.y = ei + fi;
    B.x = er - fr;
    B.y = ei - fi;
  }

  // isGuardLevel (util.cpp:259-278) of the row's level combination; the leakage term sums the DIAGONAL elements of those rows
  __device__ __forceinline__ bool row_is_guard(const DevSys& S) const {
    bool g = false;
#pragma unroll
    for (int k = 0; k < Q; k++) {
      const int a = rowok ? (row / S.post[k]) % S.n[k] : 0;
      g = g || (a == S.n[k] - 1 && a >= S.ness[k]);
    }
    return g && rowok;
  }
};

typedef double col_d2 __attribute__((ext_vector_type(2)));

// per-workgroup machinery: buffers, reductions, the Neumann solver
// SKIP: the solver skips stopping tests (stage / neumann below) - an instantiation of its own (a request with a relative tolerance
// that can bind, rel2 >= 1e-30, keeps the test-every-pass kernels; with both forms in one kernel the second code path cost 11 %)
// KCLS: the forward kernel of the diagonal-split stationary solver on waves of one ket class each (USLOT, no coupling) - stage() runs
// the class form of the pass (and, under QD_COL_KET_PERMUTE, the waves are permuted: ColLean::init<PERM>)
template <int Q, int EPT, bool SPLIT = false, bool USLOT = false, bool SKIP = false, bool HJ = false, bool KCLS = false>
struct ColTeam {
  static_assert(!KCLS || (SPLIT && USLOT && !HJ && Q > 1), "ket classes: diagonal-split form, uniform slots, no coupling");
  typedef ColLean<Q, EPT, SPLIT, USLOT, HJ> ST;
  ST st;
  int kc;  // KCLS: the wave's ket class
  // GAUGE: stage() solves in the frame where the drive is real (diagonal-split form without coupling)
  static constexpr bool GAUGE = QD_COL_GAUGE && SPLIT && !HJ;
  double* red;
  float4* fred;  // two slots of 16 partial sums of the solver's fp32 norm reduction
  int redslot, nw;
  // diagonal-split solver: P = (1 - alpha D)^-1 of the thread's elements, D = diag(M) = d - i Delta (transposed: d + i Delta),
  // for the step size palpha (recomputed when the step size changes: composite steppers)
  double pr[SPLIT ? EPT : 1], pi[SPLIT ? EPT : 1], palpha;
  int lastn, lastna;  // passes of the previous forward sub-step (stage) / iterations of the previous linear solve (neumann)

  __device__ __forceinline__ void init(const DevSys& S, unsigned char* smem) {
    st.template init<KCLS && QD_COL_KET_PERMUTE>(S, smem);
    if constexpr (KCLS) {
      const int lv = st.col0 / S.post[0];
      kc = uniform_i(S.n[0] < 2 ? KET_NONE : lv == 0 ? KET_BOTTOM : lv == S.n[0] - 1 ? KET_TOP : KET_INTERIOR);
    }
    red = reinterpret_cast<double*>(smem + 2 * ST::bufbytes(S.N));
    redslot = 0;
    nw = (int)(blockDim.x >> 6);
    palpha = 0.0;
    lastn = lastna = 0;
#pragma unroll
    for (int j = 0; j < (SPLIT ? EPT : 1); j++) {
      pr[j] = 1.0;
      pi[j] = 0.0;
    }
    fred = reinterpret_cast<float4*>(red + 2 * NRED * nw);
    if (threadIdx.x < 32) reinterpret_cast<float*>(fred)[threadIdx.x] = 0.f;  // (16 partial sums are read whatever the number of waves)
    __syncthreads();  // zero fill complete
  }

#if QD_COL_FORM == QD_FORM_VARS
  // The task about to run belongs to variant ic / nb_set: where that is not the variant of the workgroup's previous task (*cur; -1 before
  // the first), everything init derived from the model constants is derived again from the variant's block (ColLean::init<.., false>).
  // Workgroup-uniform; the barriers fence the column table, which every wave reads.  palpha = 0: the next set_alpha forms
  // (1 - alpha D)^-1 anew - and, FOLD, the T1 factors, which do not depend on the variant, to the same bits.
  __device__ __forceinline__ void enter_variant(const SweepArgs& A, int ic, int* cur) {
    const int var = uniform_i((int)((unsigned)ic / (unsigned)A.nb_set));
    if (var == *cur) return;
    *cur = var;
    __syncthreads();
    st.template init<false, false>(A.S, st.smem, ColVarConsts<Q>{col_vars_tab(A) + (size_t)var * col_vars_stride(Q, ST::NP)});
    palpha = 0.0;
    __syncthreads();
  }
#endif

  // x becomes the vector being read
  __device__ __forceinline__ void publish(const double2 (&x)[EPT]) {
    const unsigned wa = st.tb + (unsigned)st.dlt;
#pragma unroll
    for (int j = 0; j < EPT; j++) st.st(wa + (unsigned)j * COLB, x[j]);
    st.flip();
    __syncthreads();
  }

  // slot of the wave's partial sums in the reduction buffers: its column block - the wave id, except under the permuted wave order of
  // KCLS, where the sums are still added in column order
  __device__ __forceinline__ int wslot() const { return KCLS ? uniform_i(st.col0 / EPT) : (int)(threadIdx.x >> 6); }
  template <int NV>
  __device__ __forceinline__ void sum(double (&v)[NV]) {
    if constexpr (KCLS) {  // block_sum with the partial sums in wslot()
      double* r = red + redslot * NRED * nw;
#pragma unroll
      for (int i = 0; i < NV; i++) v[i] = wave_sum(v[i]);
      if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NV; i++) r[i * nw + wslot()] = v[i];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NV; i++) {
        double t = 0.0;
        for (int w = 0; w < nw; w++) t += r[i * nw + w];
        v[i] = t;
      }
    } else {
      block_sum<NV, false>(v, red + redslot * NRED * nw);
    }
    redslot ^= 1;
  }
  // Workgroup sum of NV <= 4 values for the Krylov solver [r6]: the wave level is a reduce-scatter (row r of 16 lanes ends up with the
  // total of value r: ~30 vector instructions for three values where three wave_sum()s are ~70), and behind the barrier ONE LDS read per
  // lane - lane 16 i + w fetches the partial sum of value i of wave w - and four DPP adds inside the rows replace the nw x NV broadcast
  // reads and dependent adds of block_sum (36 + 36 for three values on twelve waves).  Every thread returns the same bits.
  template <int NV>
  __device__ __forceinline__ void sum_rows(double (&v)[NV]) {
    static_assert(NV <= 4, "one value per row of 16 lanes");
    double* r = red + redslot * NRED * nw;  // (NRED nw >= 64 doubles from four waves on)
    redslot ^= 1;
    double o[1];
    wave_reduce_scatter<NV>(v, o);
    const int lane = (int)(threadIdx.x & 63);
    if ((lane & 15) == 0) {
      const int g = wave_scatter_index<NV>(lane >> 4, 0);
      if (g >= 0) r[g * 16 + (int)(threadIdx.x >> 6)] = o[0];
    }
    __syncthreads();
    double t = ((lane >> 4) < NV && (lane & 15) < nw) ? r[lane] : 0.0;
    t += dpp_mov<0xB1>(t);
    t += dpp_mov<0x4E>(t);
    t += dpp_mov<0x124>(t);
    t += dpp_mov<0x128>(t);
    const int lo = __double2loint(t), hi = __double2hiint(t);
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * i), __builtin_amdgcn_readlane(lo, 16 * i));
  }
  // Workgroup sum in two halves, for values only a few threads need (the 2Q gradient coefficients of a step, written by threads 0 .. 2Q - 1):
  // every wave leaves its partial sums in LDS (wave_reduce_scatter: the total of value g ends up in one row of 16 lanes, 21 vector
  // instructions for the four values of a two-oscillator system where four wave_sum()s are ~120); AFTER a later barrier of the caller (the
  // one that publishes the next vector) thread i adds the partial sums of value i in wave order.  Saves the reduction's own barrier and the
  // nw x NV broadcast reads of every thread.
  double* pend;
  template <int NV>
  __device__ __forceinline__ void sum_post(const double (&v)[NV]) {
    pend = red + redslot * NRED * nw;
    redslot ^= 1;
    constexpr int K = ((NV + 1) / 2 + 1) / 2;
    double o[K];
    wave_reduce_scatter<NV>(v, o);
    const int lane = (int)(threadIdx.x & 63);
    if ((lane & 15) == 0) {
      const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
      for (int m = 0; m < K; m++) {
        const int g = wave_scatter_index<NV>(lane >> 4, m);
        if (g >= 0) pend[g * nw + wave] = o[m];
      }
    }
  }
  // (call after a __syncthreads() that follows sum_post; thread i < NV returns the sum of value i)
  __device__ __forceinline__ double sum_collect(int i) const {
    double t = 0.0;
    for (int w = 0; w < nw; w++) t += pend[i * nw + w];
    return t;
  }
  // workgroup sum of the solver's squared update norm (fp32; only compared with a threshold).  One barrier - the one that makes the
  // new iterate readable - and ONE round of LDS latency: the <= 16 partial sums are fetched by four broadcast reads and added as a tree
  // (a loop over the waves would chain 15 dependent LDS round trips in front of every stopping test).
  __device__ __forceinline__ float sum_f32(float v) {
    float4* rf = fred + redslot * 4;
    redslot ^= 1;
    v = wave_sum_f32(v);
    if ((threadIdx.x & 63) == 0) reinterpret_cast<float*>(rf)[wslot()] = v;
    __syncthreads();
    const float4 a = rf[0], b = rf[1], c = rf[2], d = rf[3];
    return (((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w))) + (((c.x + c.y) + (c.z + c.w)) + ((d.x + d.y) + (d.z + d.w)));
  }

  template <bool TRANS>
  __device__ __forceinline__ void apply_all(const StepC<Q>& c, const double2 (&x)[EPT], double2 (&y)[EPT]) const {
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      y[j] = st.template apply<TRANS>(c, j, x[j], x[j > 0 ? j - 1 : 0], x[j + 1 < EPT ? j + 1 : j]);
      slot_fence<EPT>();
    }
  }

  // FOLD (the forward kernels of the diagonal-split stationary solver, stage()): the step size is folded into the pass coefficients -
  // the thread's T1 factor g1u here, recomputed from alpha (never rescaled: a time-sliced sweep stays bit-identical to an unsliced one),
  // the sub-step's p, q (cs, sn) in stage().  (Without SPLIT the diagonal dw, dd would need the same; scaled in place by the ratio of
  // the step sizes of a composite stepper it would depend on the workgroup's task history, recomputed it costs more than it saves.)
  template <bool TRANS, bool FOLD = false>
  __device__ __forceinline__ void set_alpha(const DevSys& S, double alpha) {
    if (alpha == palpha) return;  // (uniform)
    if constexpr (FOLD) {
      static_assert(!TRANS && SPLIT, "the forward operator of the diagonal-split solver");
#pragma unroll
      for (int k = 0; k < Q; k++) st.g1u[k] = (alpha * S.g1off[k]) * st.su[k];
      // (KCLS: the ket factor of oscillator 0 is one per wave - the whole T1 coefficient, the product the pass would form)
      if constexpr (KCLS) st.g1u[0] *= st.cx[0][0];
    }
    palpha = alpha;
#pragma unroll
    for (int j = 0; j < (SPLIT ? EPT : 0); j++) {
      double dwj, ddj;
      st.diag(j, dwj, ddj);
      const double re = fma(-alpha, ddj, 1.0), im = (TRANS ? -alpha : alpha) * dwj;  // 1 - alpha D
      const double inv = 1.0 / fma(re, re, im * im);
      pr[j] = re * inv;
      pi[j] = -im * inv;
    }
  }

  // Solve (I - alpha M^{(T)}) y = b.  Returns the number of RHS applications; y in registers.
  // SPLIT = false: the reference's Neumann iteration y <- b + alpha M y (timestepper.cpp:697-727), started at y = b.
  // SPLIT = true: the same fixed point and the same stopping rule on the update norm, with the diagonal of M taken to the left-hand
  // side: y <- (1 - alpha D)^-1 (b + alpha (M - D) y), started at (1 - alpha D)^-1 b.  D carries the level energies (self- and
  // cross-Kerr shifts, detuning) and the diagonal decay: where those dominate the control Hamiltonian the contraction factor drops
  // from ||alpha M|| to ~||alpha (M - D)|| (3 x 20 workload: 12.4 -> 8.x iterations per solve) at the same cost per iteration.
  // The squared update norm is reduced in fp32 exactly as Team::neumann of qd_device.h.
  template <bool TRANS>
  __device__ __forceinline__ int neumann(const SweepArgs& A, const StepC<Q>& c, double alpha, const double2 (&b)[EPT], double2 (&y)[EPT]) {
    // (set_alpha<TRANS>(alpha) has been called at the top of the step: no control flow between an operator application and its use)
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      if (SPLIT) y[j] = make_double2(fma(pr[SPLIT ? j : 0], b[j].x, -pi[SPLIT ? j : 0] * b[j].y), fma(pr[SPLIT ? j : 0], b[j].y, pi[SPLIT ? j : 0] * b[j].x));
      else y[j] = b[j];
    }
    const double inv_abs2 = A.inv_abs2;
    float rel2 = A.rel2, thr = 1.f;
    if (A.stop_residual) {
      // in place of GMRES (qd_handle::gmres_as_split): stop when kappa^2 ||y_{m+1} - y_m||^2 <= max(rtol^2 ||b||^2, abstol^2)
      double nb2[1] = {0.0};
#pragma unroll
      for (int j = 0; j < EPT; j++) nb2[0] = fma(b[j].x, b[j].x, fma(b[j].y, b[j].y, nb2[0]));
      sum<1>(nb2);
      thr = (float)fmin(fmax(A.reltol * A.reltol * nb2[0] * inv_abs2, 1.0) / A.kappa2, 1e30);
      rel2 = 0.f;
    }
    publish(y);
    float d0 = 1.f, dprev = 1.f;
    const int skip = SKIP ? lastna - (A.standin_tau2 != 0.f ? 3 : 2) : 0;  // (one more tested pass where the error estimate needs a predecessor)
    int iter;
    for (iter = 0; iter < A.maxiter; iter++) {
      const unsigned wa = st.tb + (unsigned)st.dlt;
      double dl = 0.0;
      double2 prev = y[0];
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        const double2 own = y[j];
        const double2 t = st.template apply<TRANS, SPLIT>(c, j, own, prev, y[j + 1 < EPT ? j + 1 : j]);
        double2 w;
        w.x = fma(alpha, t.x, b[j].x);
        w.y = fma(alpha, t.y, b[j].y);
        if (SPLIT) w = make_double2(fma(pr[SPLIT ? j : 0], w.x, -pi[SPLIT ? j : 0] * w.y), fma(pr[SPLIT ? j : 0], w.y, pi[SPLIT ? j : 0] * w.x));
        const double dx = own.x - w.x, dy = own.y - w.y;
        dl = fma(dx, dx, fma(dy, dy, dl));
        prev = own;
        y[j] = w;
        st.st(wa + (unsigned)j * COLB, w);
        slot_fence<EPT>();
      }
      float d = 1e30f, dp;
      if constexpr (SKIP) {  // (see stage())
        const bool test = iter >= skip;
        if (test) d = sum_f32((float)fmin(dl * inv_abs2, 1e30));  // contains the barrier that makes the new iterate readable
        else __syncthreads();
        st.flip();
        if (!test) continue;
        d0 = (iter == 0 || iter == skip) ? d : d0;
        dp = (iter == 0 || iter == skip) ? d : dprev;
      } else {
        d = sum_f32((float)fmin(dl * inv_abs2, 1e30));  // contains the barrier that makes the new iterate readable
        st.flip();
        // (one exit branch per pass, first-iteration values by selects [r5]: 637.6 -> 632.3 ms on the 3600 x 2500 sweep, same counts)
        d0 = iter == 0 ? d : d0;
        dp = iter == 0 ? d : dprev;
      }
      const bool stop = (d < thr && standin_ok(A.standin_tau2, d, dp, thr)) | (d < rel2 * d0);
      dprev = d;
      if (stop) { iter++; break; }
    }
    if (SKIP) lastna = iter;
    return iter;
  }

  // GAUGE: what a sub-step reads from the phasor table (qd_gauge.h), row = the table row of the sub-step: r_k through the scalar path
  // like the control row (load_step_k), a thread's row phasor as one 16-byte load - lane = row of rho; the padding rows hold 1.
  // row: the table row itself (wave-uniform), from which stage() fetches the phasors it needs behind the pass loop
  struct GaugeRow {
    double r[Q];
    const double* row;
  };
  static __device__ __forceinline__ void gauge_load_r(const double* row, GaugeRow& g) {
#pragma unroll
    for (int k = 0; k < Q; k++) g.r[k] = kload(row + GAUGE_R + k);
  }
  // the thread's phasor of a 64-lane block of a table row: blk = row (the absolute w_i) or row + GAUGE_V (the relative v_i)
  static __device__ __forceinline__ double2 gauge_load_w(const double* blk) {
    const col_d2 t = *(reinterpret_cast<const col_d2*>(blk) + __lane_id());
    return make_double2(t.x, t.y);
  }

  // Forward sub-step in STAGE form.  The reference solves (I - alpha M) k = M x and sets x += h k (ImplMidpoint::evolveFWD,
  // timestepper.cpp:594-629, alpha = h / 2).  The iterates of its Neumann solver, y_0 = b = M x, y_{m+1} = b + alpha M y_m (SPLIT:
  // y_0 = P b, y_{m+1} = P (b + alpha C y_m), P = (1 - alpha D)^-1, C = M - D), map one to one onto iterates of the stage
  // z = x + alpha k:   z_m = x + alpha y_m   satisfies   z_{-1} = x,  z_m = x + alpha M z_{m-1}   (SPLIT: z_m = P (x + alpha C z_{m-1})),
  // (SPLIT: P x - x = alpha P D x, hence z_0 = P (x + alpha C x) = x + alpha P (D + C) x = x + alpha y_0.)  So the application that
  // forms b IS the first pass of the same loop, x itself is the right-hand side - it stays in registers and is never parked - and no
  // separate operator application, no b, no y_0 = P b is needed.  The update norms agree up to the factor alpha:
  // ||y_m - y_{m-1}|| = ||z_m - z_{m-1}|| / alpha, tested from the second pass on against the same thresholds.  On exit z = x + alpha k
  // (the primal stage the adjoint sweep reads) and x_{n+1} = 2 z - x.  Returns the RHS applications (passes).
  // In place of GMRES (A.stop_residual): threshold max(rtol^2 ||b||^2, abstol^2) / kappa^2 with ||b||^2 >= ||y_0||^2 (|1 - alpha D| >= 1:
  // the diagonal of M has a non-positive real part) taken from the first pass - never looser than the rule it stands for.
  // SPLIT: the step size is folded into the coefficients (set_alpha<false, true> has scaled the thread's part): a pass forms
  // x + alpha C z with its accumulators started at x - two fp64 instructions per element less.
  //
  // GAUGE (SPLIT without coupling): the solve runs in the frame where the drive of every oscillator is real.  With the sub-step's
  // c_k = q_k + i p_k = r_k e^{i theta_k} and the diagonal unitary U = (x)_k exp(-i theta_k n_k), rho~ = U rho U^dag is
  // rho~_ij = w_i conj(w_j) rho_ij, w_i = prod_k u_k^{i_k}, u_k = conj(c_k) / r_k.  In M rho the drive of oscillator k is
  // conj(c_k) E + c_k F with E the two neighbours whose i_k - j_k is one larger and F the two where it is one smaller: their phasors
  // differ from the element's own by conj(u_k) and u_k, so in the rotated frame the term is r_k (E~ + F~) (ColLean::apply, RD).
  // The diagonal - hence P - and the T1 term, which couples (i + 1, j + 1) to (i, j), do not change; the rotation is elementwise and
  // unitary, so iterate m of the rotated solve is U z_m U^dag and the update norms are the ones of the lab frame up to rounding: same
  // stopping rule, same pass counts.  The controls are constant within a sub-step, so this is exact for any phase jump between
  // sub-steps.  r_k and the row phasors w_i depend on the control row and the row index only: they come from the phasor table built
  // with the control table (qd_gauge.h, k_gauge).
  // The frame PERSISTS between sub-steps.  x is the state in the frame of the sub-step on entry (the sweep rotates the initial
  // condition in once, with w(0): k_forward), and stage() also makes the step and changes frame in one go: on exit
  //   x = x~(s + 1) = f_rel o (2 z~ - x~),   f_rel = v_row conj(v_col),   v_i(s) = w_i(s + 1) conj(w_i(s))   (the table's second block),
  // the next sub-step's right-hand side in ITS frame - the rotation out of s and into s + 1 are two diagonal unitaries back to back,
  // applied as their product: one phasor per element and sub-step, and nothing of the frame exists across the pass loop.  w(nsub) = 1:
  // the last sub-step leaves x in the lab frame.  THE RULE: x advances through the relative phasors only, by this one arithmetic path,
  // whatever else the launch stores; lab-frame values - the trajectory row and the weighted Jtrace / Jfrobenius penalties (k_forward),
  // the stored stage z = U^dag z~ U (here, A.ztraj only) - are by-products formed with the absolute phasor w(s), loaded only by the
  // launches that need them, and never feed back into x.  So a sweep returns the same bits with and without storage, and a time slice
  // hands on the rotated state as computed (k_forward): sliced and batched sweeps keep the bits of the unsliced single one.  The
  // caller neither publishes x nor combines.
  // r_k^2 below 1e-280 counts as no drive (u_k = 1, r_k = 0: gauge_osc of qd_gauge.h): never a NaN.
  // g: the table row of this sub-step and its r_k (gauge_load_r).  Unused without GAUGE.
  __device__ __forceinline__ int stage(const SweepArgs& A, const StepC<Q>& c, double alpha, double2 (&x)[EPT], double2 (&z)[EPT], const GaugeRow& g) {
    double sc = A.inv_abs2 / (alpha * alpha);
    if constexpr (KCLS) sc = to_scalar(sc);  // (wave-uniform: a scalar operand of the tested passes instead of a register pair of every pass)
    StepC<Q> ca = c;  // (alpha p, alpha q, alpha cs, alpha sn: scaled in VALU once per sub-step, back to scalar registers)
    if constexpr (GAUGE) {
#pragma unroll
      for (int k = 0; k < Q; k++) ca.q[k] = to_scalar(fma(alpha, g.r[k], 0.0));  // alpha r_k (a silent oscillator: + 0.0, also under alpha < 0)
      publish(x);  // z_{-1} = x~, as the previous sub-step left it
    }
#pragma unroll
    for (int k = 0; k < (SPLIT && !GAUGE ? Q : 0); k++) {
      ca.p[k] = to_scalar(alpha * c.p[k]);
      ca.q[k] = to_scalar(alpha * c.q[k]);
    }
    if constexpr (HJ && SPLIT) {
#pragma unroll
      for (int p = 0; p < ST::NP; p++) {
        ca.cs[p] = to_scalar(alpha * c.cs[p]);
        ca.sn[p] = to_scalar(alpha * c.sn[p]);
      }
    }
    float rel2 = A.rel2, thr = 1.f, d0 = 1.f, dprev = 1.f;
#pragma unroll
    for (int j = 0; j < EPT; j++) z[j] = x[j];
    const int skip = SKIP ? lastn - (A.standin_tau2 != 0.f ? 4 : 3) : 0;
    // KCLS: one copy of the pass loop per ket class behind a wave-uniform branch; everything above is computed once, in front of it, and
    // the copies share the exit below (a wave of an unclassified system, n_0 = 1, runs the interior copy: every term)
    int iter;
    if constexpr (KCLS) {
      if (kc == KET_TOP) iter = passes<KET_TOP>(A, ca, alpha, sc, skip, rel2, thr, d0, dprev, x, z);
      else if (kc == KET_BOTTOM) iter = passes<KET_BOTTOM>(A, ca, alpha, sc, skip, rel2, thr, d0, dprev, x, z);
      else iter = passes<KET_INTERIOR>(A, ca, alpha, sc, skip, rel2, thr, d0, dprev, x, z);
    } else {
      iter = passes<KET_NONE>(A, ca, alpha, sc, skip, rel2, thr, d0, dprev, x, z);
    }
    if (SKIP) lastn = iter + 1;
    if constexpr (GAUGE) {
      // (fetched here, behind the pass loop: nothing of the frame is held in a register or parked in LDS across the loop - a phasor
      //  fetched at the top of the sub-step and parked costs 32 B more scratch than the kernel had, profiles/relframe_kres.txt)
      const double2 v = gauge_load_w(g.row + GAUGE_V);
      // (the relative phasors of the wave's columns: scalar loads of the same block, or lanes of v)
      double2 vc[QD_COL_GAUGE_SCOL ? EPT : 1];
      if constexpr (QD_COL_GAUGE_SCOL) {
#pragma unroll
        for (int j = 0; j < EPT; j++) vc[j] = make_double2(kload(g.row + GAUGE_V + 2 * (st.col0 + j)), kload(g.row + GAUGE_V + 2 * (st.col0 + j) + 1));
      }
      const bool stages = A.ztraj != nullptr;
      double2 w = make_double2(1.0, 0.0);
      if (stages) w = gauge_load_w(g.row);
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        const double2 f = QD_COL_GAUGE_SCOL ? phasor(v, vc[QD_COL_GAUGE_SCOL ? j : 0]) : phasor(v, j);  // f_rel = v_row conj(v_col)
        const double tx = fma(2.0, z[j].x, -x[j].x), ty = fma(2.0, z[j].y, -x[j].y);
        x[j] = make_double2(fma(f.x, tx, -f.y * ty), fma(f.x, ty, f.y * tx));  // x~(s + 1) = f_rel (2 z~ - x~)
        if (stages) {  // by-product: the lab-frame stage conj(f_abs) z~
          const double2 fa = phasor(w, j);
          z[j] = make_double2(fma(fa.x, z[j].x, fa.y * z[j].y), fma(fa.x, z[j].y, -fa.y * z[j].x));
        }
        slot_fence_pin<EPT>(x[j]);  // (one slot's phasor at a time)
      }
    }
    return iter + 1;
  }
  // GAUGE: phasor w_row conj(w_col) of the thread's element; w = the thread's row phasor, wc = the one of the element's column
  static __device__ __forceinline__ double2 phasor(const double2 w, const double2 wc) {
    return make_double2(fma(w.x, wc.x, w.y * wc.y), fma(w.y, wc.x, -w.x * wc.y));
  }
  // ... of the thread's element in slot j, w = the row phasors of one 64-lane block, one per lane: the one of column col0 + j is lane
  // col0 + j of the same register (idle columns and padding rows: 1)
  __device__ __forceinline__ double2 phasor(const double2 w, int j) const {
    const int lc = st.col0 + j;
    const double cr = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(w.x), lc), __builtin_amdgcn_readlane(__double2loint(w.x), lc));
    const double ci = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(w.y), lc), __builtin_amdgcn_readlane(__double2loint(w.y), lc));
    return phasor(w, make_double2(cr, ci));
  }
  // GAUGE: into the frame (IN: x~ = f x) or out of it (conj(f) x~) with the thread's absolute row phasor w - the one entry of a sweep
  // (k_forward, slice 0) and its lab-frame by-products
  template <bool IN>
  __device__ __forceinline__ double2 rotate(const double2 w, int j, const double2 v) const {
    const double2 f = phasor(w, j);
    return IN ? make_double2(fma(f.x, v.x, -f.y * v.y), fma(f.x, v.y, f.y * v.x)) : make_double2(fma(f.x, v.x, f.y * v.y), fma(f.x, v.y, -f.y * v.x));
  }
  // the pass loop of stage() in the form of ket class KC (ColLean::apply), on stage()'s own variables; returns the index of the last pass
  template <int KC>
  __device__ __forceinline__ int passes(const SweepArgs& A, const StepC<Q>& c, double alpha, double sc, int skip, float& rel2, float& thr, float& d0,
                                        float& dprev, const double2 (&x)[EPT], double2 (&z)[EPT]) {
    int iter;
    for (iter = -1; iter < A.maxiter; iter++) {
      const unsigned wa = st.tb + (unsigned)st.dlt;
      double dl = 0.0;
      double2 prev = z[0];
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        const double2 own = z[j];
        double2 w;
        if constexpr (SPLIT) {
          w = st.template apply<false, true, KC, GAUGE>(c, j, own, prev, z[j + 1 < EPT ? j + 1 : j], &x[j]);  // x + alpha C z
        } else {
          const double2 t = st.template apply<false, false>(c, j, own, prev, z[j + 1 < EPT ? j + 1 : j]);
          w.x = fma(alpha, t.x, x[j].x);
          w.y = fma(alpha, t.y, x[j].y);
        }
        if (SPLIT) w = make_double2(fma(pr[SPLIT ? j : 0], w.x, -pi[SPLIT ? j : 0] * w.y), fma(pr[SPLIT ? j : 0], w.y, pi[SPLIT ? j : 0] * w.x));
        const double dx = own.x - w.x, dy = own.y - w.y;
        dl = fma(dx, dx, fma(dy, dy, dl));
        prev = own;
        z[j] = w;
        st.st(wa + (unsigned)j * COLB, w);
        slot_fence<EPT>();
      }
      // [r5] SKIP: the reduction of the update norm costs ~25 vector instructions and an LDS round trip behind the barrier.  Consecutive
      // sub-steps converge after the same number of passes (the controls move slowly): under the reference's plain update-norm rule the
      // passes up to two before the count of the previous sub-step only synchronise.  A solve that would have stopped earlier runs on to
      // the first tested pass: more passes than the reference, never fewer (3600 x 2500 sweep: 8.238 -> 8.240 passes per step, 635 -> 611 ms).
      // Under the rule that stands in for GMRES the error estimate of a tested pass needs the norm of its predecessor: one more pass is
      // tested there (without it the first tested pass compares with itself and passes are lost: 8.98 -> 9.60, 685 -> 697 ms; with it
      // 8.975 -> 8.979 passes, 675 -> 655 ms), and its first pass is reduced for ||y_0||.
      bool test = true;
      float d = 1e30f;
      if constexpr (SKIP) {
        test = iter < 0 ? A.stop_residual != 0 : iter >= skip;
        if (test) d = sum_f32((float)fmin(dl * sc, 1e30));  // contains the barrier that makes the new iterate readable
        else __syncthreads();
      } else {
        d = sum_f32((float)fmin(dl * sc, 1e30));  // contains the barrier that makes the new iterate readable
      }
      st.flip();
      if (iter < 0) {  // first pass: d = ||y_0||^2 / abstol^2
        if (A.stop_residual) {
          thr = (float)fmin(fmax(A.reltol * A.reltol * (double)d, 1.0) / A.kappa2, 1e30);  // (d is capped at 1e30: conservative)
          rel2 = 0.f;
        }
        continue;
      }
      if (SKIP && !test) continue;
      // (one exit branch per pass, first-iteration values by selects [r5]: 637.6 -> 632.3 ms on the 3600 x 2500 sweep, same counts)
      const bool first = iter == 0 || (SKIP && iter == skip);
      d0 = first ? d : d0;
      const float dp = first ? d : dprev;
      const bool stop = (d < thr && standin_ok(A.standin_tau2, d, dp, thr)) | (d < rel2 * d0);
      dprev = d;
      if (stop) { iter++; break; }
    }
    return iter;
  }

  // ---------------------------------------------------------------------------------------------
  // Krylov solver of the lean column kernels [r6]: linearsolver_type = gmres (KSPGMRES, src/timestepper.cpp:541-550, call sites :602,
  // :652, :674) where the stationary iteration does not stand in for it (option gmres_split = 0, or its gate has failed).
  //
  // GMRES on (I - alpha M) y = b, right-preconditioned with the polynomial of the diagonal-split iteration:
  //   I - alpha M = (I - alpha D) - alpha C,  P = (I - alpha D)^-1,  R_p = sum_{i<p} (P alpha C)^i P,  (I - alpha M) R_p = I - (alpha C P)^p.
  // The residual of the preconditioned system IS b - (I - alpha M) y, so the reference's stopping rule - residual <= max(rtol ||b||,
  // abstol) - is unchanged.  z = R_p v is Horner's rule z <- P (v + alpha C z) from z = P v: the SAME pass as the stationary iteration
  // (one NODIAG application, the iterate and the right-hand side in registers, nothing else live), without its reductions.
  //
  // Hot path (one Krylov vector suffices: the host tunes p for that, qd_handle::forward_finish): p passes, then ONE full application
  // w = (I - alpha M) z fused with the three dot products <b,b>, <r,b>, <r,r> of r = b - w in one workgroup reduction.  With v_0 = b / beta:
  //   h_00 = <w, v_0> = 1 - a,  a = <r,b> / <b,b>;   h_10^2 = ||w - h_00 v_0||^2 = <r,r> / <b,b> - a^2   (from r, not from ||w||^2 - h_00^2,
  //   which cancels to nothing at residuals of 1e-10);   y = h_00 / (h_00^2 + h_10^2) z,   residual = beta h_10 / sqrt(h_00^2 + h_10^2).
  // No basis vector is written, b never leaves its registers (adjoint) / is parked once per step (forward, stage form below).
  // Slow path (residual above the tolerance after one vector): the solve starts over in kry_generic - classical Gram-Schmidt, Givens
  // rotations, restart KRY_MR, every vector (basis V, preconditioned basis Z = R_p V, the parked right-hand side) in this WORKGROUP's 32
  // slots of SweepArgs::kry, each thread touching its own elements only.  Rare by construction of p; its cost is its own.
  // ---------------------------------------------------------------------------------------------
  double2* wg;  // this workgroup's scratch vectors in global memory, at this thread's element of slot 0: vector s, slot j = wg[s KRY_VEC + 64 j]
  // (the vectors keep the PADDED column layout of the exchange buffers - 64 rows per column: idle lanes and idle slots park their zeros
  //  like everybody else, no guard, no exec mask inside a slot loop, and one base address with immediate offsets per vector)
  double* ksc;  // Hessenberg scalars of kry_generic (LDS, behind the column table)
  // Forward hot path: b = M x is formed by the first pass and used by the last one for <b,b> and <r,b> only - quantities that enter
  // the solution as 1 - <r,b>/<b,b> with <r,b>/<b,b> ~ 1e-10: an fp32 copy serves.  Five columns per wave (N <= 60) leave room for it in
  // LDS (8 B per element in the padded layout, 30 KB); eight columns per wave (N = 61 .. 64) park b in slot SB, fetched two slots ahead.
  static constexpr bool BLDS = EPT == 5;
  unsigned b32;  // LDS byte address of this thread's element of slot 0 of the fp32 copy
  static __host__ __device__ size_t kry_lds_extra(int N) { return sizeof(double) * KRY_NSC + (BLDS ? 512u * (size_t)ST::ncols(N) : 0u); }
  static constexpr int SV = 0, SZ = KRY_MR + 1, SB = 2 * KRY_MR + 1, SY = 2 * KRY_MR + 2, SX = 2 * KRY_MR + 3;

  __device__ __forceinline__ void init_kry(const SweepArgs& A) {
    wg = reinterpret_cast<double2*>(A.kry) + (size_t)blockIdx.x * (GMRES_MR_G + 2) * KRY_VEC + (size_t)st.col0 * 64 + (threadIdx.x & 63);
    ksc = reinterpret_cast<double*>(st.smem + ST::tab_off(A.S.N) + 48u * (unsigned)ST::ncols(A.S.N));
    b32 = ST::tab_off(A.S.N) + 48u * (unsigned)ST::ncols(A.S.N) + (unsigned)sizeof(double) * KRY_NSC + (unsigned)st.col0 * 512u + (threadIdx.x & 63) * 8u;
  }
  __device__ __forceinline__ double2* vec(int s) const { return wg + (size_t)s * KRY_VEC; }
  __device__ __forceinline__ void vstore(int s, const double2 (&v)[EPT]) const {
    double2* p = vec(s);
#pragma unroll
    for (int j = 0; j < EPT; j++) p[64 * j] = v[j];
  }
  __device__ __forceinline__ void vload(int s, double2 (&v)[EPT]) const {
    const double2* p = vec(s);
#pragma unroll
    for (int j = 0; j < EPT; j++) v[j] = p[64 * j];
  }
  __device__ __forceinline__ double2 pmul(int j, const double2 w) const {
    return make_double2(fma(pr[SPLIT ? j : 0], w.x, -pi[SPLIT ? j : 0] * w.y), fma(pr[SPLIT ? j : 0], w.y, pi[SPLIT ? j : 0] * w.x));
  }
  // one pass of Horner's rule: y <- P (rhs + alpha C y); the published vector is y on entry and on exit
  template <bool TRANS>
  __device__ __forceinline__ void kry_pass(const StepC<Q>& c, double alpha, const double2 (&rhs)[EPT], double2 (&y)[EPT]) {
    const unsigned wa = st.tb + (unsigned)st.dlt;
    double2 prev = y[0];
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      const double2 own = y[j];
      const double2 t = st.template apply<TRANS, true>(c, j, own, prev, y[j + 1 < EPT ? j + 1 : j]);
      const double2 w = pmul(j, make_double2(fma(alpha, t.x, rhs[j].x), fma(alpha, t.y, rhs[j].y)));
      prev = own;
      y[j] = w;
      st.st(wa + (unsigned)j * COLB, w);
      slot_fence<EPT>();
    }
    __syncthreads();
    st.flip();
  }
  // h_00 / (h_00^2 + h_10^2) of the one-vector solve, or a negative value where its residual is above the tolerance
  __device__ __forceinline__ double kry_one_vector(const SweepArgs& A, const double (&d)[3]) const {
    const double bb = d[0], ab = d[1], ss = d[2];
    const double ttol2 = fmax(A.reltol * A.reltol * bb, A.abstol * A.abstol);
    if (bb <= ttol2) return 0.0;  // ||b|| <= tolerance: KSP returns the zero initial guess
    const double ibb = 1.0 / bb, a = ab * ibb, h00 = 1.0 - a, h10sq = fmax(fma(-a, a, ss * ibb), 0.0), den = fma(h00, h00, h10sq);
    const bool conv = bb * h10sq <= A.kry_tau2 * ttol2 * den || A.maxiter <= 1;  // (kry_tau: SweepArgs)
    return conv ? h00 / den : -1.0;
  }

  // the generic path: on entry the right-hand side is in v AND in slot SB; on exit y = solution, v = right-hand side
  template <bool TRANS>
  __device__ __forceinline__ int kry_generic(const SweepArgs& A, const StepC<Q>& c, double alpha, double2 (&v)[EPT], double2 (&y)[EPT]) {
    const int poly = A.gmres_poly > 1 ? A.gmres_poly : 1;
    const int mre = A.kry_restart >= 1 && A.kry_restart < KRY_MR ? A.kry_restart : KRY_MR;  // restart length (option krylov_restart)
    double* hc = ksc;                  // [MR + 2] current Hessenberg column
    double* cs = hc + (KRY_MR + 2);    // [MR]
    double* sn = cs + KRY_MR;          // [MR]
    double* g = sn + KRY_MR;           // [MR + 2]
    double* R = g + (KRY_MR + 2);      // [MR][MR] row-major upper triangle (reciprocal diagonal)
    double* yk = R + KRY_MR * KRY_MR;  // [MR]
    int napp = 0, its = 0;
    bool have_total = false;
    double ttol = 0.0;
    for (int cycle = 0;; cycle++) {
      double t1[1] = {0.0};
#pragma unroll
      for (int j = 0; j < EPT; j++) t1[0] = fma(v[j].x, v[j].x, fma(v[j].y, v[j].y, t1[0]));
      sum_rows<1>(t1);
      const double ibeta = t1[0] > 0.0 ? rsqrt_nr(t1[0]) : 0.0, beta = t1[0] * ibeta;
      // (the acceptance factor of the one-vector path - SweepArgs::kry_tau2 - here as well: a preconditioned vector takes the residual down
      //  by the contraction of p passes at once, but the LAST one of a solve lands anywhere below the tolerance; held to kry_tau x the
      //  tolerance the generic path is as accurate as the reference's GMRES typically is, profiles/r6_kry_seed_sweep.txt)
      if (cycle == 0) ttol = sqrt(A.kry_tau2) * fmax(A.reltol * beta, A.abstol);
#pragma unroll
      for (int j = 0; j < EPT; j++) y[j] = make_double2(0.0, 0.0);
      if (beta <= ttol || its >= A.maxiter) break;
#pragma unroll
      for (int j = 0; j < EPT; j++) v[j] = make_double2(v[j].x * ibeta, v[j].y * ibeta);
      vstore(SV, v);
      double gcur = beta;
      int jj = 0;
      bool conv = false;
      while (jj < mre) {
        // z = R_p v_jj, parked in Z_jj; w = (I - alpha M) z takes its registers
#pragma unroll
        for (int j = 0; j < EPT; j++) y[j] = pmul(j, v[j]);
        publish(y);
        for (int m = 1; m < poly; m++) kry_pass<TRANS>(c, alpha, v, y);
        {
          double2* zp = vec(SZ + jj);
          double2 prev = y[0];
#pragma unroll
          for (int j = 0; j < EPT; j++) {
            const double2 own = y[j];
            const double2 t = st.template apply<TRANS, false>(c, j, own, prev, y[j + 1 < EPT ? j + 1 : j]);
            zp[64 * j] = own;
            prev = own;
            y[j] = make_double2(fma(-alpha, t.x, own.x), fma(-alpha, t.y, own.y));
            slot_fence<EPT>();
          }
        }
        napp += poly;
        // classical Gram-Schmidt: every projection against the un-updated w, four per reduction; v_jj is in registers, v_k (k < jj) is read back
        for (int p0 = 0; p0 <= jj; p0 += 4) {
          double h4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int k = p0 + q;
            if (k == jj) {
#pragma unroll
              for (int j = 0; j < EPT; j++) h4[q] = fma(y[j].x, v[j].x, fma(y[j].y, v[j].y, h4[q]));
            } else if (k < jj) {
              const double2* vp = vec(SV + k);
#pragma unroll
              for (int j = 0; j < EPT; j++) {
                const double2 vk = vp[64 * j];
                h4[q] = fma(y[j].x, vk.x, fma(y[j].y, vk.y, h4[q]));
              }
            }
          }
          sum_rows<4>(h4);
#pragma unroll
          for (int q = 0; q < 4; q++)
            if (p0 + q <= jj) hc[p0 + q] = h4[q];
        }
        {
          const double h = hc[jj];
#pragma unroll
          for (int j = 0; j < EPT; j++) y[j] = make_double2(fma(-h, v[j].x, y[j].x), fma(-h, v[j].y, y[j].y));
        }
        for (int k = 0; k < jj; k++) {
          const double h = hc[k];
          const double2* vp = vec(SV + k);
#pragma unroll
          for (int j = 0; j < EPT; j++) {
            const double2 vk = vp[64 * j];
            y[j] = make_double2(fma(-h, vk.x, y[j].x), fma(-h, vk.y, y[j].y));
          }
        }
        double nn[1] = {0.0};
#pragma unroll
        for (int j = 0; j < EPT; j++) nn[0] = fma(y[j].x, y[j].x, fma(y[j].y, y[j].y, nn[0]));
        sum_rows<1>(nn);
        const double ihn = nn[0] > 0.0 ? rsqrt_nr(nn[0]) : 0.0, hn = nn[0] * ihn;
        // Givens rotations: redundantly by every thread on workgroup-uniform values, idempotent LDS writes only (Team::gmres_g of qd_device.h)
        double cur_h = hc[0];
        for (int k = 0; k < jj; k++) {
          const double a1 = hc[k + 1], ck = cs[k], sk = sn[k];
          R[k * KRY_MR + jj] = ck * cur_h + sk * a1;
          cur_h = -sk * cur_h + ck * a1;
        }
        const double s2 = cur_h * cur_h + hn * hn;
        const double irr = s2 > 0.0 ? rsqrt_nr(s2) : 0.0;
        const double cj = s2 > 0.0 ? cur_h * irr : 1.0, sj = hn * irr;
        cs[jj] = cj;
        sn[jj] = sj;
        R[jj * KRY_MR + jj] = irr;
        g[jj] = cj * gcur;
        gcur = -sj * gcur;
        its++;
        jj++;
        if (fabs(gcur) <= ttol || hn == 0.0) { conv = true; break; }
        if (its >= A.maxiter || jj >= mre) break;
#pragma unroll
        for (int j = 0; j < EPT; j++) v[j] = make_double2(y[j].x * ihn, y[j].y * ihn);
        vstore(SV + jj, v);
        __syncthreads();  // (the scalars of this column have been read by every thread before the next one overwrites hc)
      }
      for (int rw = jj - 1; rw >= 0; rw--) {
        double sacc = g[rw];
        for (int cc = rw + 1; cc < jj; cc++) sacc -= R[rw * KRY_MR + cc] * yk[cc];
        yk[rw] = sacc * R[rw * KRY_MR + rw];
      }
#pragma unroll
      for (int j = 0; j < EPT; j++) y[j] = make_double2(0.0, 0.0);
      for (int cc = 0; cc < jj; cc++) {
        const double f = yk[cc];
        const double2* zp = vec(SZ + cc);
#pragma unroll
        for (int j = 0; j < EPT; j++) {
          const double2 zk = zp[64 * j];
          y[j] = make_double2(fma(f, zk.x, y[j].x), fma(f, zk.y, y[j].y));
        }
      }
      if (conv || its >= A.maxiter) break;
      // restart: park the accumulated solution, r = b - (I - alpha M) y_total
      if (have_total) {
        const double2* tp = vec(SY);
#pragma unroll
        for (int j = 0; j < EPT; j++) {
          const double2 o = tp[64 * j];
          y[j].x += o.x;
          y[j].y += o.y;
        }
      }
      vstore(SY, y);
      have_total = true;
      publish(y);
      {
        const double2* bp = vec(SB);
        double2 prev = y[0];
#pragma unroll
        for (int j = 0; j < EPT; j++) {
          const double2 own = y[j];
          const double2 t = st.template apply<TRANS, false>(c, j, own, prev, y[j + 1 < EPT ? j + 1 : j]);
          const double2 bj = bp[64 * j];
          v[j] = make_double2(bj.x - fma(-alpha, t.x, own.x), bj.y - fma(-alpha, t.y, own.y));
          prev = own;
          slot_fence<EPT>();
        }
      }
      napp++;
      __syncthreads();  // every thread has read the scalars of this cycle before the next one overwrites them
    }
    if (have_total) {
      const double2* tp = vec(SY);
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        const double2 o = tp[64 * j];
        y[j].x += o.x;
        y[j].y += o.y;
      }
    }
    vload(SB, v);
    return napp;
  }

  // (I - alpha M^{(T)}) y = b for the adjoint sweep: b stays in registers.  Returns the RHS applications.
  template <bool TRANS>
  __device__ __forceinline__ int kry_solve(const SweepArgs& A, const StepC<Q>& c, double alpha, double2 (&b)[EPT], double2 (&y)[EPT]) {
    const int poly = A.gmres_poly > 1 ? A.gmres_poly : 1;
#pragma unroll
    for (int j = 0; j < EPT; j++) y[j] = pmul(j, b[j]);
    publish(y);
    for (int m = 1; m < poly; m++) kry_pass<TRANS>(c, alpha, b, y);
    double d[3] = {0.0, 0.0, 0.0};
    {
      double2 prev = y[0];
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        const double2 own = y[j];
        const double2 t = st.template apply<TRANS, false>(c, j, own, prev, y[j + 1 < EPT ? j + 1 : j]);
        const double rx = b[j].x - fma(-alpha, t.x, own.x), ry = b[j].y - fma(-alpha, t.y, own.y);  // r = b - (I - alpha M) z
        d[0] = fma(b[j].x, b[j].x, fma(b[j].y, b[j].y, d[0]));
        d[1] = fma(rx, b[j].x, fma(ry, b[j].y, d[1]));
        d[2] = fma(rx, rx, fma(ry, ry, d[2]));
        prev = own;
        slot_fence<EPT>();
      }
    }
    sum_rows<3>(d);
    const double fac = kry_one_vector(A, d);
    if (__builtin_expect(fac >= 0.0, 1)) {
#pragma unroll
      for (int j = 0; j < EPT; j++) y[j] = make_double2(fac * y[j].x, fac * y[j].y);
      return poly;
    }
#ifdef QD_KRY_NOCOLD
    return poly;
#else
    vstore(SB, b);
    return poly + kry_generic<TRANS>(A, c, alpha, b, y);
#endif
  }

  // Forward sub-step in stage form (see stage()): the passes run on z = x + alpha y with x as the right-hand side, so the application that
  // forms b = M x IS the first pass (b = C x + D x is parked in slot SB from there: 16 B per element and step through L2) and the iterate
  // of the k-system is y = (z - x) / alpha.  Residual of the k-system at y: r = b - (I - alpha M) y = M z - y.  On exit z = x + alpha k.
  __device__ __forceinline__ int kry_stage(const SweepArgs& A, const StepC<Q>& c, double alpha, double2 (&x)[EPT], double2 (&z)[EPT]) {
    const int poly = A.gmres_poly > 1 ? A.gmres_poly : 1;
    double2* bp = vec(SB);
    {  // first pass: z_0 = P (x + alpha C x), b = C x + D x
      const unsigned wa = st.tb + (unsigned)st.dlt;
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        const double2 own = x[j];
        const double2 t = st.template apply<false, true>(c, j, own, x[j > 0 ? j - 1 : 0], x[j + 1 < EPT ? j + 1 : j]);
        double dwj, ddj;
        st.diag(j, dwj, ddj);
        const double2 bj = make_double2(fma(dwj, own.y, fma(ddj, own.x, t.x)), fma(-dwj, own.x, fma(ddj, own.y, t.y)));
        if constexpr (BLDS) *reinterpret_cast<float2*>(st.smem + b32 + 512u * j) = make_float2((float)bj.x, (float)bj.y);
        else bp[64 * j] = bj;
        const double2 w = pmul(j, make_double2(fma(alpha, t.x, own.x), fma(alpha, t.y, own.y)));
        z[j] = w;
        st.st(wa + (unsigned)j * COLB, w);
        slot_fence<EPT>();
      }
      __syncthreads();
      st.flip();
    }
    for (int m = 1; m < poly; m++) kry_pass<false>(c, alpha, x, z);
    double d[3] = {0.0, 0.0, 0.0};
    {
      const double ia = 1.0 / alpha;
      double2 prev = z[0];
      double2 bq[2] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
      if constexpr (!BLDS) {
        bq[0] = bp[0];
        bq[1] = bp[EPT > 1 ? 64 : 0];
      }
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        const double2 own = z[j];
        double2 bj;
        if constexpr (BLDS) {
          const float2 f = *reinterpret_cast<const float2*>(st.smem + b32 + 512u * j);
          bj = make_double2((double)f.x, (double)f.y);
        } else {
          bj = bq[j & 1];
          if (j + 2 < EPT) bq[j & 1] = bp[64 * (j + 2 < EPT ? j + 2 : 0)];
        }
        const double2 t = st.template apply<false, false>(c, j, own, prev, z[j + 1 < EPT ? j + 1 : j]);
        const double rx = fma(-ia, own.x - x[j].x, t.x), ry = fma(-ia, own.y - x[j].y, t.y);  // r = M z - (z - x) / alpha
        d[0] = fma(bj.x, bj.x, fma(bj.y, bj.y, d[0]));
        d[1] = fma(rx, bj.x, fma(ry, bj.y, d[1]));
        d[2] = fma(rx, rx, fma(ry, ry, d[2]));
        prev = own;
        slot_fence<EPT>();
      }
    }
    sum_rows<3>(d);
    const double fac = kry_one_vector(A, d);
    if (__builtin_expect(fac >= 0.0, 1)) {
#pragma unroll
      for (int j = 0; j < EPT; j++) z[j] = make_double2(fma(fac, z[j].x - x[j].x, x[j].x), fma(fac, z[j].y - x[j].y, x[j].y));
      return poly + 1;
    }
#ifdef QD_KRY_NOCOLD
    return poly + 1;
#endif
    // the solve starts over on the k-system: b = M x again (in fp64), x parked, b in its registers
    publish(x);
    apply_all<false>(c, x, z);
    vstore(SX, x);
    vstore(SB, z);
#pragma unroll
    for (int j = 0; j < EPT; j++) x[j] = z[j];
    const int n = 1 + kry_generic<false>(A, c, alpha, x, z);
    vload(SX, x);
#pragma unroll
    for (int j = 0; j < EPT; j++) z[j] = make_double2(fma(alpha, z[j].x, x[j].x), fma(alpha, z[j].y, x[j].y));
    return poly + 1 + n;
  }
};

// ---------------------------------------------------------------------------------------------
// Time-sliced scheduling of the sweeps.  One workgroup owns one CU (two exchange buffers of N KiB), so a batch of nb initial conditions
// runs in nb / #CUs rounds of whole sweeps and the last round is as long as any other however few workgroups it holds: 3600 initial
// conditions on 256 CUs are 14.06 rounds - 6 % of the sweep with 240 CUs idle; the 450 of an eight-GPU shard 1.76 rounds - 12 %.  With
// A.sched set the sweep is cut into A.nslice slices of whole time steps and a resident grid draws (slice, initial condition) tasks from
// a counter, slice-major: the tail shrinks to one SLICE.  Slice k of an initial condition waits for slice k - 1 (a flag per initial
// condition, released at agent scope after the state has been written back; the predecessor was drawn earlier, hence is running or
// done: no deadlock whatever the dispatch order) and picks the state up from the carry buffer.  A wait that exceeds A.sched_ticks (4 s x
// the processes sharing the device x the slice length in thousands of steps, qd_handle::arm_slices) raises the error word instead of
// hanging the device.
//   sched[0] task counter | sched[1] error word | sched[2 + ic] slices of ic completed
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int sched_next(unsigned* sched, unsigned* slot) {
  __syncthreads();  // (the previous task's last reads of *slot)
  if (threadIdx.x == 0) *slot = atomicAdd(sched, 1u);
  __syncthreads();
  return __builtin_amdgcn_readfirstlane((int)*slot);
}
// wait until `want` slices of initial condition ic are complete; false after the time limit
// The word of an initial condition: slices completed in its low byte (at most 64 slices), above it a value the finished slice hands to
// its successor (*carry, through the LDS word `slot`): the solver's pass count of the last sub-step, so that a sliced sweep skips the
// same stopping tests as an unsliced one and the two stay bit-identical.
__device__ __forceinline__ bool sched_wait(unsigned* sched, int ic, unsigned want, unsigned long long limit, unsigned* slot, int* carry) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();  // 100 MHz
    unsigned v;
    while (((v = __hip_atomic_load(sched + 2 + ic, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xffu) < want) {
      __builtin_amdgcn_s_sleep(8);
      if (wall_clock64() - t0 > limit) {
        atomicExch(sched + 1, 1u);
        break;
      }
    }
    *slot = v >> 8;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  *carry = __builtin_amdgcn_readfirstlane((int)*slot);
  return __hip_atomic_load(sched + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
}
// the state of ic has been written: publish the completion of its slice
__device__ __forceinline__ void sched_done(unsigned* sched, int ic, unsigned done, int carry) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its stores have reached L2
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(sched + 2 + ic, done | ((unsigned)carry << 8), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// first sub-step of slice sl (whole time steps)
__device__ __forceinline__ int slice_start(const SweepArgs& A, int sl) {
  return (int)((long long)A.ntime * sl / A.nslice) * A.nstages;
}

// Pair form: where the owner of a diagonal element keeps member b's penalty sum - one double per thread behind the column
// table, the 8 x blockDim.x bytes col_launch adds to the launch.  A second accumulator in registers would live across the pass loop,
// which has none to spare.
template <class TM>
__device__ __forceinline__ double* col_pair_word(unsigned char* smem, int N) {
  return reinterpret_cast<double*>(smem + TM::ST::tab_off(N) + 48u * (unsigned)TM::ST::ncols(N));
}

// ---------------------------------------------------------------------------------------------
// forward sweep (TimeStepper::solveODE for every initial condition of the batch)
// ---------------------------------------------------------------------------------------------
template <int Q, int EPT, bool SPLIT, bool USLOT = false, bool SKIP = false, bool KRY = false>
__global__ void __launch_bounds__(col_max_threads(EPT)) QD_COLK(k_forward)(const SweepArgs A) {
  static_assert(!KRY || (SPLIT && !SKIP), "the Krylov solver runs on the diagonal-split form");
  constexpr bool HJ = col_coupled;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // (ket classes: where the waves share the level of oscillator 0 - stationary diagonal-split solver, no coupling)
  typedef ColTeam<Q, EPT, SPLIT, USLOT, SKIP, HJ, SPLIT && USLOT && !KRY && !HJ> TM;
  const DevSys& S = A.S;
  TM tm;
  tm.init(S, smem);
  if constexpr (KRY) tm.init_kry(A);
  __shared__ unsigned task_slot, carry_slot;
#if QD_COL_FORM == QD_FORM_VARS
  int curvar = -1;  // variant of the workgroup's previous task (ColTeam::enter_variant)
#endif
  const int dim = S.dim, ntask = A.nb * A.nslice;
  const bool pen_on = A.gamma_penalty > 1e-13;
  const bool wj_on = pen_on && A.penalty_param > 1e-13;
  const bool leak = pen_on && A.leak_on && tm.st.row_is_guard(S);
  for (int task = A.sched ? sched_next(A.sched, &task_slot) : (int)blockIdx.x; task < ntask; task = A.sched ? sched_next(A.sched, &task_slot) : ntask) {
  const int ic = task % A.nb, sl = task / A.nb;
#if QD_COL_FORM == QD_FORM_VARS
  tm.enter_variant(A, ic, &curvar);
#endif
  const int s_lo = slice_start(A, sl), s_hi = slice_start(A, sl + 1);
  tm.lastn = 0;  // (the pass count of the previous sub-step: none at t = 0, otherwise what the previous slice hands over)
  if (sl > 0 && !sched_wait(A.sched, ic, (unsigned)sl, A.sched_ticks, &carry_slot, &tm.lastn)) return;
  double2 x[EPT];
  {
    // slice 0 starts from the initial condition, every other one from where its predecessor left the state (the carry = xT)
    const double* x0 = (sl > 0 ? A.xT : A.x0) + (size_t)ic * 2 * dim;
#pragma unroll
    for (int j = 0; j < EPT; j++) x[j] = tm.st.ok(j) ? make_double2(x0[tm.st.elem(j)], x0[dim + tm.st.elem(j)]) : make_double2(0.0, 0.0);
  }
  double pen_local = 0.0, pen_uniform [[maybe_unused]] = 0.0;  // (no uniform part in the pair form)
  // (pair form: pen_local sums member a; member b's sum is the thread's word of LDS, touched by the owner of a diagonal element once
  //  per full time step and addressed where it is used - nothing of it lives across the pass loop)
  constexpr bool paired = col_form == Form::Pair;
  if constexpr (paired) col_pair_word<TM>(smem, S.N)[threadIdx.x] = 0.0;
#if QD_COL_FORM == QD_FORM_VARS
  // A time-sliced sweep of this form carries every thread's penalty sum from slice to slice (qd_col_vars.h: one block of
  // COL_VARS_PEN_STRIDE doubles per state, the uniform part in its last word) and reduces it once, behind the last slice: the additions
  // of a thread are those of the unsliced sweep in the same order, so a sliced call returns the bits of an unsliced one - penalties
  // included.  The predecessor's stores are visible like its state in A.xT (sched_done / sched_wait).
  // (the block's address is formed where it is used, from kernel arguments: nothing of it lives across the time loop)
  if (A.sched && sl > 0) {
    const double* pc = col_vars_pen_carry(A) + (size_t)ic * COL_VARS_PEN_STRIDE;
    pen_local = pc[threadIdx.x];
    // (the uniform part exists where the rotated-frame form does not fold it into the thread sums; wave-uniform: scalar registers)
    if constexpr (!TM::GAUGE) pen_uniform = to_scalar(pc[COL_VARS_PEN_STRIDE - 1]);
  }
#endif
  unsigned long long napply = 0;
  // global accesses of the thread's elements: one divergent region per call (rows), uniform branches inside (columns)
  auto store_state = [&](double* dst, const double2(&v)[EPT], bool nt) {
    if (tm.st.rowok) {
#pragma unroll
      for (int j = 0; j < EPT; j++)
        if (tm.st.colok(j)) {
          const int e = tm.st.elem_now(j);
          if (nt) {
            __builtin_nontemporal_store(v[j].x, dst + e);
            __builtin_nontemporal_store(v[j].y, dst + dim + e);
          } else {
            dst[e] = v[j].x;
            dst[dim + e] = v[j].y;
          }
        }
    }
  };

  // (GAUGE: the sweep runs in the real-drive frame, which persists between sub-steps (ColTeam::stage): x is the state in the frame of
  //  sub-step s at the top of the loop body, and row s of the phasor table gives r_k, the relative phasors that take x to the frame of
  //  s + 1, and the absolute ones for the lab-frame by-products.  Slice 0 enters the frame here, once; every other slice picks up the
  //  rotated state its predecessor left in the carry, as computed; the last sub-step of the sweep leaves x in the lab frame.)
  constexpr bool GAUGE = TM::GAUGE && !KRY;
  typename TM::GaugeRow grow;
  const double* gtab = GAUGE ? QD_COL_GAUGE_TAB(A, ic) : nullptr;
  if constexpr (GAUGE) {
    if (sl == 0) {
      const double2 w = TM::gauge_load_w(gtab);
#pragma unroll
      for (int j = 0; j < EPT; j++) x[j] = tm.template rotate<true>(w, j, x[j]);
    }
  }
  for (int s = s_lo; s < s_hi; s++) {
    StepC<Q> c;
    load_step_k<Q>(QD_COL_CTL(A, ic) + (size_t)s * A.cs, c, HJ);
    if constexpr (GAUGE) {
      grow.row = gtab + (size_t)s * GAUGE_STRIDE;
      TM::gauge_load_r(grow.row, grow);
    }
    if (SPLIT) tm.template set_alpha<false, SPLIT && !KRY>(S, 0.5 * c.h);
    if (A.traj) {
      if constexpr (GAUGE) {  // by-product: the lab-frame state conj(f_abs) x~
        const double2 w = TM::gauge_load_w(grow.row);
        double2 xl[EPT];
#pragma unroll
        for (int j = 0; j < EPT; j++) xl[j] = tm.template rotate<false>(w, j, x[j]);
        store_state(A.traj + ((size_t)s * A.nb + ic) * 2 * dim, xl, true);
      } else {
        store_state(A.traj + ((size_t)s * A.nb + ic) * 2 * dim, x, true);
      }
    }
    // the sub-step in stage form (ColTeam::stage): x is the right-hand side of the solve and stays in registers
    // (GAUGE: stage() publishes x itself, and returns with the step made and the frame changed)
    if constexpr (!GAUGE) tm.publish(x);
    // (GAUGE: on return x is x_{n+1} in the frame of the next sub-step, and z is the lab-frame stage ONLY where stages are stored
    //  (A.ztraj) - otherwise it is left in the rotated frame of this sub-step and must not be read; the stage store below is its one
    //  consumer)
    double2 z[EPT];
    if constexpr (KRY) napply += tm.kry_stage(A, c, 0.5 * c.h, x, z);
    else napply += tm.stage(A, c, 0.5 * c.h, x, z, grow);
    if (A.ztraj && tm.st.rowok) {  // the primal stage, read back by the adjoint sweep instead of repeating this solve: private to
      // this kernel pair, kept interleaved (one 16-byte streaming access per element; qd_handle tags the layout: ztraj_fmt)
      col_d2* dst = reinterpret_cast<col_d2*>(A.ztraj) + ((size_t)s * A.nb + ic) * dim;
#pragma unroll
      for (int j = 0; j < EPT; j++)
        if (tm.st.colok(j)) {
          const col_d2 t = {z[j].x, z[j].y};
          __builtin_nontemporal_store(t, dst + tm.st.elem_now(j));
        }
    }
#pragma unroll
    for (int j = 0; j < (GAUGE ? 0 : EPT); j++) {  // x_{n+1} = x + h k = 2 z - x
      x[j].x = fma(2.0, z[j].x, -x[j].x);
      x[j].y = fma(2.0, z[j].y, -x[j].y);
    }
    // ... of a Hermitian pair: the weighted Jmeasure and the leakage term read the diagonal, rho_a's in x.x and rho_b's in x.y (a
    // Hermitian member has a real diagonal, and the frame change leaves the diagonal alone).  The gate admits no other in-loop
    // penalty and tabulates the weights (A.wjw).
    if (paired && pen_on && (s + 1) % A.nstages == 0) {  // (paired is a constant of the form)
      const int n = (s + 1) / A.nstages - 1;
      const double wrow = wj_on ? kload(A.wjw + n) * A.dt * fabs((double)(tm.st.row - A.tg.purestate_id)) : 0.0;
#pragma unroll
      for (int j = 0; j < EPT; j++)
        if (tm.st.rowok && tm.st.colof(j) == tm.st.row) {
          double pb = 0.0;
          if (wj_on) {
            pen_local = fma(wrow, x[j].x, pen_local);
            pb = wrow * x[j].y;
          }
          if (leak) {
            pen_local += x[j].x * x[j].x / A.ntime;
            pb += x[j].y * x[j].y / A.ntime;
          }
          col_pair_word<TM>(smem, S.N)[threadIdx.x] += pb;
        }
    }
    // in-loop penalties at the end of a FULL time step (timestepper.cpp:141-154, :256-298)
    if (pen_on && !paired && (s + 1) % A.nstages == 0) {
      const int n = (s + 1) / A.nstages - 1;
      const double tstop = (n + 1) * A.dt;
      if (wj_on) {
        // (tabulated per time step: an exp() evaluated here, next to x and k, was spilt by the compiler and reloaded through seven
        // serialised scratch round trips - 3 us per workgroup and step, 12 % of the 3 x 20 forward sweep)
        double weight;
        if (A.wjw) {
          weight = kload(A.wjw + n);
        } else {
          const double a = (tstop - A.Tfinal) / A.penalty_param;
          weight = 1.0 / A.penalty_param * exp(-(a * a));
        }
        // finalizeJ is affine for Lindblad: J = jr (Jfrobenius, Jmeasure) or 1 - jr (Jtrace).  Jmeasure only sees the diagonal of rho,
        // which the column layout has at hand (the generic routine divides the vectorised index by N per element and step: ~12 % of
        // the 3 x 20 forward sweep)
        if (A.tg.objective_type == QD_OBJ_JMEASURE) {
          const double wrow = weight * A.dt * fabs((double)(tm.st.row - A.tg.purestate_id));
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.st.rowok && tm.st.colof(j) == tm.st.row) pen_local = fma(wrow, x[j].x, pen_local);
        } else if (tm.st.rowok) {
          // (GAUGE: Jtrace and Jfrobenius read off-diagonal elements - by-product: the lab-frame state conj(f_abs) x~ with the absolute
          //  phasor of the frame x is in now, the next sub-step's; behind the last sub-step that is the lab frame itself)
          double2 wl = make_double2(1.0, 0.0);
          if constexpr (GAUGE)
            if (s + 1 < A.nsub) wl = TM::gauge_load_w(gtab + (size_t)(s + 1) * GAUGE_STRIDE);
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.st.colok(j)) {
              double jr = 0.0, ji = 0.0;
              const double2 xl = GAUGE ? tm.template rotate<false>(wl, j, x[j]) : x[j];
              evalJ_part<true>(S, A.tg, ic, tm.st.elem_now(j), xl, jr, ji);
              pen_local += (A.tg.objective_type == QD_OBJ_JTRACE ? -1.0 : 1.0) * weight * A.dt * jr;
            }
        }
        // (GAUGE: the uniform part of the Jtrace penalty is added by the owner of element (0, 0) to its local sum - an accumulator of
        //  its own is one more register pair across the pass loop, and spilt)
        if (A.tg.objective_type == QD_OBJ_JTRACE) {
          if constexpr (GAUGE) pen_local += (tm.st.row == 0 && tm.st.colof(0) == 0) ? weight * A.dt : 0.0;
          else pen_uniform += weight * A.dt;
        }
      }
      if (leak) {
#pragma unroll
        for (int j = 0; j < EPT; j++)
          if (tm.st.colof(j) == tm.st.row) pen_local += (x[j].x * x[j].x + x[j].y * x[j].y) / A.ntime;
      }
    }
  }
  store_state(A.xT + (size_t)ic * 2 * dim, x, false);
  if (A.traj && sl == A.nslice - 1) store_state(A.traj + ((size_t)A.nsub * A.nb + ic) * 2 * dim, x, false);
#if QD_COL_FORM == QD_FORM_VARS
  if (A.sched && sl < A.nslice - 1) {  // not the last slice: the thread's sum travels on
    double* pcarry = col_vars_pen_carry(A) + (size_t)ic * COL_VARS_PEN_STRIDE;
    pcarry[threadIdx.x] = pen_local;
    if constexpr (!TM::GAUGE)
      if (threadIdx.x == 0) pcarry[COL_VARS_PEN_STRIDE - 1] = pen_uniform;
  }
  // (one path for every slice: the reduction of a slice that is not the last is not used - the last one's is the sweep's)
  double v[1] = {pen_local};
  tm.template sum<1>(v);
  if (threadIdx.x == 0) {
    A.pen_out[ic] = 0.0 + v[0] + pen_uniform;  // (the expression of the other forms at sl = 0)
    A.dpdm_out[ic] = 0.0;
    atomicAdd(A.napply, napply);
  }
#else
  double v[1] = {pen_local};
  tm.template sum<1>(v);
#if QD_COL_FORM == QD_FORM_PAIR
  // the members' sums apart (an odd batch has no second member in its last pair: A.paired = the number of members)
  double vb[1] = {col_pair_word<TM>(smem, S.N)[threadIdx.x]};
  tm.template sum<1>(vb);
  if (threadIdx.x == 0) {
    A.pen_out[2 * ic] = (sl > 0 ? A.pen_out[2 * ic] : 0.0) + v[0];
    if (2 * ic + 1 < A.paired) A.pen_out[2 * ic + 1] = (sl > 0 ? A.pen_out[2 * ic + 1] : 0.0) + vb[0];
    A.dpdm_out[ic] = 0.0;
    atomicAdd(A.napply, napply);
  }
#else
  if (threadIdx.x == 0) {
    A.pen_out[ic] = (sl > 0 ? A.pen_out[ic] : 0.0) + v[0] + pen_uniform;  // (slices of one initial condition run one after the other)
    A.dpdm_out[ic] = 0.0;  // the dpdm penalty is Schroedinger only (timestepper.cpp:143-146)
    atomicAdd(A.napply, napply);
  }
#endif
#endif
  if (A.sched) sched_done(A.sched, ic, (unsigned)(sl + 1), tm.lastn);
  }
}

// ---------------------------------------------------------------------------------------------
// adjoint sweep (TimeStepper::solveAdjointODE + ImplMidpoint::evolveBWD + compute_dRHS_dParams)
// ---------------------------------------------------------------------------------------------
template <int Q, int EPT, bool SPLIT, bool USLOT = false, bool SKIP = false, bool KRY = false>
__global__ void __launch_bounds__(col_max_threads(EPT)) QD_COLK(k_adjoint)(const SweepArgs A) {
  static_assert(!KRY || (SPLIT && !SKIP), "the Krylov solver runs on the diagonal-split form");
  constexpr bool HJ = col_coupled;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef ColTeam<Q, EPT, SPLIT, USLOT, SKIP, HJ> TM;
  const DevSys& S = A.S;
  TM tm;
  tm.init(S, smem);
  if constexpr (KRY) tm.init_kry(A);
  __shared__ unsigned task_slot, carry_slot;
#if QD_COL_FORM == QD_FORM_VARS
  int curvar = -1;  // variant of the workgroup's previous task (ColTeam::enter_variant)
#endif
  const int dim = S.dim, ntask = A.nb * A.nslice;
  const bool pen_on = A.gamma_penalty > 1e-13;
  const bool wj_on = pen_on && A.penalty_param > 1e-13;
  const bool leak = pen_on && A.leak_on && tm.st.row_is_guard(S);
  for (int task = A.sched ? sched_next(A.sched, &task_slot) : (int)blockIdx.x; task < ntask; task = A.sched ? sched_next(A.sched, &task_slot) : ntask) {
  // backwards in time: task slice sl covers the time slice nslice - 1 - sl
  const int ic = task % A.nb, sl = task / A.nb;
#if QD_COL_FORM == QD_FORM_VARS
  tm.enter_variant(A, ic, &curvar);
#endif
  const int s_lo = slice_start(A, A.nslice - 1 - sl), s_hi = slice_start(A, A.nslice - sl);
  tm.lastna = 0;
  if (sl > 0 && !sched_wait(A.sched, ic, (unsigned)sl, A.sched_ticks, &carry_slot, &tm.lastna)) return;
  double2 xb[EPT];
  {
    const double* xbT = (sl > 0 ? A.stash : A.xbarT) + (size_t)ic * 2 * dim;  // (the carry of the adjoint state: SweepArgs::stash)
#pragma unroll
    for (int j = 0; j < EPT; j++) xb[j] = tm.st.ok(j) ? make_double2(xbT[tm.st.elem(j)], xbT[dim + tm.st.elem(j)]) : make_double2(0.0, 0.0);
  }
  const double jbar_pen = A.jbar[ic * 3 + 0];
#if QD_COL_FORM == QD_FORM_SENS
  // W of the thread's elements over the sub-steps of this task (the sensitivity form, see the top of the file)
  double wacc[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) wacc[j] = 0.0;
#endif
  auto load_state = [&](const double* base, int s, double2(&dst)[EPT]) {
    const double* src = base + ((size_t)s * A.nb + ic) * 2 * dim;
#pragma unroll
    for (int j = 0; j < EPT; j++)
      dst[j] = tm.st.ok(j) ? make_double2(__builtin_nontemporal_load(src + tm.st.elem_now(j)), __builtin_nontemporal_load(src + dim + tm.st.elem_now(j)))
                           : make_double2(0.0, 0.0);
  };

  for (int s = s_hi - 1; s >= s_lo; s--) {
    // penalty adjoints at the end of a full step, with the primal x_n (timestepper.cpp:220-227, :300-339)
    if (pen_on && (s + 1) % A.nstages == 0 && (wj_on || leak)) {
      const int n = (s + 1) / A.nstages;
      const double tstop = n * A.dt;
      // (the weighted Jmeasure's adjoint is a constant per row: without guard levels this sweep never reads the states, and the
      // forward sweep of a gradient evaluation has not stored them - qd_handle::adjoint_reads_states)
      const bool need_xn = leak || (wj_on && A.tg.objective_type != QD_OBJ_JMEASURE);
      double2 xn[EPT];
      if (need_xn) {
        load_state(A.traj, s + 1, xn);
      } else {
#pragma unroll
        for (int j = 0; j < EPT; j++) xn[j] = make_double2(0.0, 0.0);
      }
      if (wj_on) {
        double weight;
        if (A.wjw) {
          weight = kload(A.wjw + (n - 1));
        } else {
          const double a = (tstop - A.Tfinal) / A.penalty_param;
          weight = 1.0 / A.penalty_param * exp(-(a * a));
        }
        double rb, ib;
        finalizeJ_diff<true>(A.tg, 0.0, 0.0, rb, ib);
        if (A.tg.objective_type == QD_OBJ_JMEASURE) {
          const double wrow = weight * rb * jbar_pen * A.dt * fabs((double)(tm.st.row - A.tg.purestate_id));
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.st.rowok && tm.st.colof(j) == tm.st.row) xb[j].x += wrow;
        } else {
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.st.ok(j)) evalJ_diff_elem<true>(S, A.tg, ic, tm.st.elem_now(j), xn[j], xb[j], weight * rb * jbar_pen * A.dt, weight * ib * jbar_pen * A.dt);
        }
      }
      if (leak) {
#pragma unroll
        for (int j = 0; j < EPT; j++)
          if (tm.st.colof(j) == tm.st.row) {
            xb[j].x += 2.0 * xn[j].x * jbar_pen / A.ntime;
            xb[j].y += 2.0 * xn[j].y * jbar_pen / A.ntime;
          }
      }
    }
    StepC<Q> c;
    load_step_k<Q>(QD_COL_CTL(A, ic) + (size_t)s * A.cs, c, HJ);
    // ImplMidpoint::evolveBWD (timestepper.cpp:631-694); the primal stage z of the sub-step was stored by the forward sweep
    if (SPLIT) tm.template set_alpha<true>(S, 0.5 * c.h);
    double2 kb[EPT];  // adjoint stage: (I - h/2 M)^T kbar = xbar ; kbar *= h
    if constexpr (KRY) tm.template kry_solve<true>(A, c, 0.5 * c.h, xb, kb);
    else tm.template neumann<true>(A, c, 0.5 * c.h, xb, kb);
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      kb[j].x *= c.h;
      kb[j].y *= c.h;
    }
    double cf[2 * Q];
#pragma unroll
    for (int i = 0; i < 2 * Q; i++) cf[i] = 0.0;
    {
      double2 z[EPT];
      {
        const col_d2* src = reinterpret_cast<const col_d2*>(A.ztraj) + ((size_t)s * A.nb + ic) * dim;
#pragma unroll
        for (int j = 0; j < EPT; j++) {
          if (tm.st.ok(j)) {
            const col_d2 t = __builtin_nontemporal_load(src + tm.st.elem_now(j));
            z[j] = make_double2(t.x, t.y);
          } else {
            z[j] = make_double2(0.0, 0.0);
          }
        }
      }
      tm.publish(z);
#if QD_COL_FORM == QD_FORM_SENS
      // kbar^T (dM/d theta) z of the diagonal model operators, before the weights: kbar (h-scaled) and z are in ONE frame here, the lab
      // frame - the adjoint solve knows no other, and the forward sweep stores the stage as the lab-frame by-product z = U^dag z~ U
      // whatever frame it solves in (ColTeam::stage, A.ztraj) - as the ladder contraction below already relies on.  Padding elements
      // hold zeros in both.
#pragma unroll
      for (int j = 0; j < EPT; j++) wacc[j] = fma(kb[j].x, z[j].y, fma(-kb[j].y, z[j].x, wacc[j]));
#endif
      // gradient coefficients x^T dM/dp_k z and x^T dM/dq_k z with x := kbar (mastereq.hpp:553-604)
#pragma unroll
      for (int j = 0; j < EPT; j++) {
#pragma unroll
        for (int k = 0; k < Q; k++) {
          double2 Av, Bv;
          tm.st.ladder(k, j, z[j], z[j > 0 ? j - 1 : 0], z[j + 1 < EPT ? j + 1 : j], Av, Bv);
          cf[2 * k] += Bv.y * kb[j].x - Bv.x * kb[j].y;
          cf[2 * k + 1] += Av.x * kb[j].x + Av.y * kb[j].y;
        }
        slot_fence<EPT>();
      }
    }
    tm.template sum_post<2 * Q>(cf);
    // xbar += M^T kbar
    tm.publish(kb);  // (its barrier also completes the coefficient sums)
    if (threadIdx.x < 2 * Q) A.coeff[((size_t)ic * A.nsub + s) * 2 * Q + threadIdx.x] = tm.sum_collect((int)threadIdx.x);
    double2 t[EPT];
    tm.template apply_all<true>(c, kb, t);
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      xb[j].x += t[j].x;
      xb[j].y += t[j].y;
    }
  }
  double* d0 = sl == A.nslice - 1 ? A.xbar0 : A.stash;
  if (d0) {
    d0 += (size_t)ic * 2 * dim;
#pragma unroll
    for (int j = 0; j < EPT; j++)
      if (tm.st.ok(j)) {
        d0[tm.st.elem(j)] = xb[j].x;
        d0[dim + tm.st.elem(j)] = xb[j].y;
      }
  }
#if QD_COL_FORM == QD_FORM_SENS
  {  // once per task: the integer weights of the thread's elements from their level digits (qd_sens.h), the workgroup totals, the row
    constexpr int NS = sens_count(Q);
    double sacc[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) sacc[i] = 0.0;
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      const bool live = tm.st.ok(j);  // (a padding element has no digits and adds nothing)
      unsigned bra = 0, ket = 0;
      if (live) sens_decode<Q, true>(S, tm.st.elem(j), bra, ket);
      sens_add<Q, true>(bra, ket, live ? wacc[j] : 0.0, sacc);
    }
    sens_store<NS>(tm, sacc, A.S.tred + ((size_t)sl * A.nb + ic) * NS);
  }
#endif
  if (A.sched) sched_done(A.sched, ic, (unsigned)(sl + 1), tm.lastna);
  }
}

// single operator application (test hook = MatMult / MatMultTranspose on the shell)
template <int Q, int EPT, bool SPLIT>
__global__ void __launch_bounds__(col_max_threads(EPT)) QD_COLK(k_apply)(const DevSys S, const double* __restrict__ ctlrow, int transpose, const double* __restrict__ xin,
                                                              double* __restrict__ yout) {
  constexpr bool HJ = col_coupled;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef ColTeam<Q, EPT, SPLIT, false, false, HJ> TM;
  TM tm;
  tm.init(S, smem);
  const int ic = blockIdx.x, dim = S.dim;
  double2 x[EPT], y[EPT];
  const double* x0 = xin + (size_t)ic * 2 * dim;
#pragma unroll
  for (int j = 0; j < EPT; j++) x[j] = tm.st.ok(j) ? make_double2(x0[tm.st.elem(j)], x0[dim + tm.st.elem(j)]) : make_double2(0.0, 0.0);
  StepC<Q> c;
  load_step_k<Q>(ctlrow, c, HJ);
  scalarize<Q>(c, HJ);
  tm.publish(x);
  if (transpose) tm.template apply_all<true>(c, x, y);
  else tm.template apply_all<false>(c, x, y);
  double* yo = yout + (size_t)ic * 2 * dim;
#pragma unroll
  for (int j = 0; j < EPT; j++)
    if (tm.st.ok(j)) {
      yo[tm.st.elem(j)] = y[j].x;
      yo[dim + tm.st.elem(j)] = y[j].y;
    }
}

// ---------------------------------------------------------------------------------------------
// host side: the launchers, one text for every unit - each instantiates them for its own kernels (QD_COLK), form and coupling
// ---------------------------------------------------------------------------------------------
// the operator application for systems with dipole-dipole coupling (qd_colj.hip); launch_apply_col forwards to it where S.hasJ
hipError_t launch_apply_colj(const DevSys& S, const double* ctlrow, int transpose, const double* x, double* y, int nb, hipStream_t st);

#define QD_COL_STR_(x) #x
#define QD_COL_STR(x) QD_COL_STR_(x)
#define QD_COLK_NAME(base) QD_COL_STR(QD_COLK(base))  // "k_forward_col" / "k_forward_colj_sets": the name note_kernel records

// the columns of a wave share the level indices of every oscillator but the stride-1 one (ColLean's USLOT)
template <int EPT>
static bool col_uslot(const DevSys& S) {
  if (S.N % EPT != 0) return false;
  for (int k = 0; k < S.Q - 1; k++)
    if (S.post[k] % EPT != 0) return false;
  return true;
}

// grid of a sweep: one workgroup per initial condition, or - time-sliced scheduling - as many workgroups as are resident at once
template <typename K>
static int col_grid(K kern, const SweepArgs& a, int threads, size_t lds) {
  if (!a.sched) return a.nb;
  int per_cu = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), threads, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  if (a.use_gmres) per_cu = std::min(per_cu, 2);  // (col_krylov_doubles)
  return std::min(a.nb * a.nslice, per_cu * cu_count());
}

// One sweep kernel, forward or adjoint, of the instantiation <Q, EPT, SPLIT, USLOT, SKIP, KRY>: the two kernels of an instantiation are a
// pair (the adjoint one reads the primal stages in the element order the forward one wrote), so the direction is the only thing left open.
template <int Q, int EPT, bool SPLIT, bool USLOT, bool SKIP, bool KRY>
static hipError_t col_launch(const SweepArgs& a, bool adjoint, hipStream_t st) {
  typedef ColLean<Q, EPT> ST;
  const int threads = 64 * (ST::ncols(a.S.N) / EPT);
  // (pair form: member b's penalty word per thread, col_pair_word; pairs are an error in every other form, and the other way round)
  if ((a.paired != 0) != (col_form == Form::Pair)) return hipErrorInvalidValue;
  const size_t lds = ST::lds_bytes(a.S.N) + (KRY ? ColTeam<Q, EPT, true>::kry_lds_extra(a.S.N) : 0) + (col_form == Form::Pair ? sizeof(double) * (size_t)threads : 0);
  // (a direction the form has no kernel for - the pair form's adjoint, the sensitivity form's forward sweep, which is the plain one's:
  //  an error, and nothing instantiated)
  if (adjoint ? !col_has_adjoint : !col_has_forward) return hipErrorInvalidValue;
  void (*kf)(const SweepArgs);
  if constexpr (!col_has_adjoint) kf = QD_COLK(k_forward)<Q, EPT, SPLIT, USLOT, SKIP, KRY>;
  else if constexpr (!col_has_forward) kf = QD_COLK(k_adjoint)<Q, EPT, SPLIT, USLOT, SKIP, KRY>;
  else kf = adjoint ? QD_COLK(k_adjoint)<Q, EPT, SPLIT, USLOT, SKIP, KRY> : QD_COLK(k_forward)<Q, EPT, SPLIT, USLOT, SKIP, KRY>;
  hipError_t e = set_lds(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(adjoint ? 1 : 0, adjoint ? QD_COLK_NAME(k_adjoint) : QD_COLK_NAME(k_forward), Q, EPT, SPLIT, USLOT, SKIP, KRY);
  hipLaunchKernelGGL(kf, dim3(col_grid(kf, a, threads, lds)), dim3(threads), lds, st, a);
  return hipGetLastError();
}

// What the unit's form asks of a sweep's arguments; a request the unit cannot serve is an error, never another kernel.
//   every unit   its own coupling, and a solver it has an instantiation of
//   Sets, Vars   a.nb states = a.nb / a.nb_set sets (Vars: a set is a variant), each reading its own control table
//   Vars         the constants table, never a dense handle; a time-sliced forward sweep needs the carry buffer of the penalty sums
//   Sens         the adjoint sweep of a single evaluation on the diagonal-split stationary iteration, with the stored stages and the buffer
//                of the sums
//   Pair         the forward sweep of a single evaluation on the stationary solvers, on a.nb = ceil(a.paired / 2) pairs, nothing stored,
//                no in-loop penalty that reads off-diagonal elements
static bool col_form_args_ok(const SweepArgs& a, bool adjoint) {
  if ((a.S.hasJ != 0) != col_coupled || (a.use_gmres && !col_has_krylov)) return false;
  if (col_per_set && !(a.nb_set >= 1 && a.nb % a.nb_set == 0)) return false;
  if (col_per_variant && !(col_vars_tab(a) && !a.S.dense && (adjoint || !a.sched || col_vars_pen_carry(a)))) return false;
  if (col_form == Form::Sens) return adjoint && a.neumann_split && a.nb_set == 0 && !a.stepper_ee && !a.S.dense && a.S.tred && a.ztraj;
  if (col_form == Form::Pair)
    return !adjoint && a.nb_set == 0 && !a.stepper_ee && !a.S.dense && a.paired >= 2 && a.nb == (a.paired + 1) / 2 && !a.traj && !a.ztraj &&
           (!(a.gamma_penalty > 1e-13 && a.penalty_param > 1e-13) || (a.wjw && a.tg.objective_type == QD_OBJ_JMEASURE));
  return true;
}

// The instantiation a sweep runs, from the run-time facts - the same for both directions and every form.  Built (the properties at the top
// of this file say for which unit): the Krylov solver (SweepArgs::use_gmres) in the diagonal-split form that tests every pass; the
// stationary iteration in the plain and the diagonal-split form (neumann_split), each with and without SKIP; every one of them in both
// USLOT forms.  With coupling the diagonal-split forms without SKIP only: a coupled sweep that asks for the plain Neumann iteration is
// never planned (qd_handle::col_sweep).  A Vars plan on the plain-Neumann or Krylov solver goes variant by variant (qd_optim.cpp), such a
// Sens plan takes the general family (qd_optim_evalGradF_model).  What is not built is an invalid value here, and nothing of it is
// instantiated.  (The order of the go() lines is the order in which the unit names its kernels: see go_sweep of qd_q32.hip.)
template <int Q, int EPT>
static hipError_t col_sweep(const SweepArgs& a, bool adjoint, hipStream_t st) {
  if (!col_form_args_ok(a, adjoint)) return hipErrorInvalidValue;
  const bool uslot = col_uslot<EPT>(a.S);
  auto go = [&](auto split, auto skip, auto kry) {
    constexpr bool SPLIT = decltype(split)::value, SKIP = decltype(skip)::value, KRY = decltype(kry)::value;
    return uslot ? col_launch<Q, EPT, SPLIT, true, SKIP, KRY>(a, adjoint, st) : col_launch<Q, EPT, SPLIT, false, SKIP, KRY>(a, adjoint, st);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (a.use_gmres) {
    if constexpr (col_has_krylov) return go(yes, no, yes);
    else return hipErrorInvalidValue;
  }
  // (SKIP: stopping tests skipped, see ColTeam::stage)
  // (implicit midpoint only: the predictor compares the pass count of a sub-step with its predecessor's, and the sub-steps of a composite
  //  step differ in size - IMR4 / IMR8 test every pass; nothing of this lives in the kernels)
  const bool skip = !col_coupled && a.rel2 < 1e-30f && !a.col_noskip && a.nstages == 1;
  if (a.neumann_split) {
    if constexpr (col_coupled) return go(yes, no, no);
    else return skip ? go(yes, yes, no) : go(yes, no, no);
  }
  if constexpr (col_has_plain_neumann) return skip ? go(no, yes, no) : go(no, no, no);
  else return hipErrorInvalidValue;
}

// One operator application.  SPLIT selects the kernel family that re-derives the diagonal from its compact form (uncoupled: the option
// neumann_split = 1, test coverage); the coupled kernels are built in that form only and their entry point passes split = true.
template <int Q, int EPT>
static hipError_t col_apply(const DevSys& S, const double* ctlrow, int tr, const double* x, double* y, int nb, bool split, hipStream_t st) {
  static_assert(col_has_apply && Q > 0, "the operator application belongs to the plain units");
  typedef ColLean<Q, EPT> ST;
  const size_t lds = ST::lds_bytes(S.N);
  auto kf = QD_COLK(k_apply)<Q, EPT, true>;
  if constexpr (!col_coupled)
    if (!split) kf = QD_COLK(k_apply)<Q, EPT, false>;
  hipError_t e = set_lds(kf, lds);
  if (e != hipSuccess) return e;
  note_kernel(2, QD_COLK_NAME(k_apply), Q, EPT, split);
  hipLaunchKernelGGL(kf, dim3(nb), dim3(64 * (ST::ncols(S.N) / EPT)), lds, st, S, ctlrow, tr, x, y);
  return hipGetLastError();
}

// Columns per wave.  Measured on the 3 x 20 workload (3600 initial conditions x 100 steps, forward sweep, one lease): 4 columns
// (15 waves, 128 VGPRs, 63 spills) 58.9 ms, 5 columns (12 waves, 168 VGPRs) 48.4 ms, 6 columns (10 waves, 59 spills) 62.9 ms,
// 8 columns (8 waves, 234 VGPRs, no spills) 53.4 ms; the general column kernel of qd_device.h 73.1 ms.  Five columns per wave cover
// N <= 60, eight the rest; only these two are built.
#define QD_COL_DISPATCH(S, FN, ...)                                                    \
  do {                                                                                 \
    if ((S).Q == 2) return (S).N <= 60 ? FN<2, 5>(__VA_ARGS__) : FN<2, 8>(__VA_ARGS__); \
    if ((S).Q == 3) return (S).N <= 60 ? FN<3, 5>(__VA_ARGS__) : FN<3, 8>(__VA_ARGS__); \
    return hipErrorInvalidValue;                                                       \
  } while (0)

// One object holds col_sweep<Q, EPT> of its unit and with it that case's kernels; the family's entry point (qd_col.hip) reaches it by the
// unit's tag and <Q, EPT> through QD_COL_DISPATCH.  The plain units define all four parts, an object of qd_col_form.hip its one.
template <Form F, bool HJ>
struct ColUnit {};
template <int Q, int EPT, Form F, bool HJ>
hipError_t col_sweep_part(ColUnit<F, HJ>, const SweepArgs& a, bool adjoint, hipStream_t st);
#define QD_COL_PART(Q, EPT)                                                                                                \
  template <>                                                                                                              \
  hipError_t col_sweep_part<Q, EPT>(ColUnit<col_form, col_coupled>, const SweepArgs& a, bool adjoint, hipStream_t st) { \
    return col_sweep<Q, EPT>(a, adjoint, st);                                                                              \
  }

}  // namespace qd

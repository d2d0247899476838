// qd_inst.hip — one translation unit per (number of oscillators, Schroedinger/Lindblad, general/qubit
// stencil): compiled with -DQD_Q=<1..5> -DQD_L=<0|1> -DQD_B=<0|1>.  Instantiates the persistent sweep
// kernels for the kernel variants that make sense for that case and exports plain launch functions
// for the dispatcher in qd_kernels.hip.
// With -DQD_SETS=1 (objects of their own, build/qd_sets_*.o): the SETS form of the same sweep kernels - one control table per set of
// SweepArgs::nb_set states (parameter-set batch, qd_optim_evalGradF_batch) - for the variants with one workgroup per state in LDS, of
// the standard Hamiltonian model (QD_B = 0 | 1) and of the dense user Hamiltonians (QD_B = 2: variants 11, 12, 13, 15, 17, one G(t) table
// per set as well, SweepArgs::gtab_set); no operator application, no global-memory kernels (variant 16).
// With -DQD_VARS=1 (build/qd_vars_*.o): the third form, k_forward_vars / k_adjoint_vars - one block of model constants per set of
// SweepArgs::nb_set states and one control table for all (model-parameter ensemble, qd_optim_evalGradF_ensemble_model; qd_gen_vars.h) -
// for the same LDS variants of the standard Hamiltonian model only (QD_B = 0 | 1): no dense variants, no variant 16.
// With -DQD_SENS=1 (build/qd_sens_*.o): the sensitivity form of the adjoint sweep, k_adjoint_sens (qd_sens.h; qd_optim_evalGradF_model) -
// the adjoint roles only (QD_PART = 1 | 3; the forward sweep is k_forward itself), for the instantiations k_adjoint_vars has.
#include "qd_device.h"
#include "qd_big.h"
#ifndef QD_VARS
#define QD_VARS 0
#endif
#if QD_VARS
#include "qd_gen_vars.h"
#if QD_B == 2 || defined(QD_SETS)
#error "QD_VARS: the standard Hamiltonian model only (QD_B = 0 | 1), and not together with QD_SETS"
#endif
#endif
#ifndef QD_SENS
#define QD_SENS 0
#endif
#if QD_SENS && (QD_B == 2 || defined(QD_SETS) || QD_VARS || (QD_PART != 1 && QD_PART != 3))
#error "QD_SENS: the adjoint roles (QD_PART = 1 | 3) of the standard Hamiltonian model only (QD_B = 0 | 1), and not together with QD_SETS or QD_VARS"
#endif

#if !defined(QD_Q) || !defined(QD_L) || !defined(QD_B) || !defined(QD_PART)
#error "compile with -DQD_Q=<1..8> -DQD_L=<0|1> -DQD_B=<0 general|1 qubit|2 dense> -DQD_PART=<0 forward + apply|1 adjoint|2 forward, GMRES kernels|3 adjoint, GMRES kernels>"
#endif
// (four objects per case: forward / adjoint x Neumann / GMRES kernels compile side by side - the five-oscillator Lindblad
// case alone took 13 minutes as one translation unit)
constexpr bool kGmPart = (QD_PART >= 2);
#ifndef QD_SETS
#define QD_SETS 0
#endif
constexpr bool kSets = (QD_SETS != 0);
constexpr bool kVars = (QD_VARS != 0);
[[maybe_unused]] constexpr bool kSens = (QD_SENS != 0);  // (read by the adjoint roles only)

namespace qd {

#define QD_CAT4(a, q, l, b) a##q##_##l##_##b
#define QD_NAME(base, q, l, b) QD_CAT4(base, q, l, b)

constexpr bool kQubit = (QD_B == 1);
constexpr bool kDense = (QD_B == 2);  // user-supplied dense Hamiltonians (DenseStencil)
constexpr bool kLind = (QD_L != 0);

// Sweeps of the global-memory kernels (qd_big.h).  One workgroup per initial condition: a plain launch.  Teams: the grid is
// padded to whole rounds of the 8 XCDs (the members of a team share an XCD), the team barriers spin, so the launch is cooperative -
// the runtime refuses a grid that cannot be resident instead of letting it hang.
[[maybe_unused]] static hipError_t launch_big(const void* kern, const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  SweepArgs b = a;
  b.S.team = cfg.team > 1 ? cfg.team : 1;
  b.S.team_spread = (cfg.spread ? 1 : 0) | (cfg.blocked == 1 ? 2 : cfg.blocked == 2 ? 4 : 0);
  void* args[] = {&b};
  if (b.S.team == 1) return hipLaunchKernel(kern, dim3(a.nb), dim3(cfg.block), args, cfg.lds, st);
  hipError_t e = hipMemsetAsync(b.S.tbar, 0, sizeof(unsigned long long) * BIG_BAR_STRIDE * (size_t)a.nb, st);
  if (e != hipSuccess) return e;
  const int teams = cfg.spread ? a.nb : (a.nb + 7) / 8 * 8;
  return hipLaunchCooperativeKernel(kern, dim3(teams * b.S.team), dim3(cfg.block), args, (unsigned)cfg.lds, st);
}

// The unit's form of the LDS sweep kernels (one workgroup per state), in the unit's direction: the kernel of <VAR, PLAIN> and the name
// note_kernel records for it.  k_forward / k_adjoint carry the SETS flag as their seventh argument, recorded for the SETS form only.
constexpr int kRole = (QD_PART & 1);  // 0 forward sweep, 1 adjoint sweep (note_kernel, plain_sweep)
#if QD_VARS
constexpr const char* kFormName = kRole ? "k_adjoint_vars" : "k_forward_vars";
#elif QD_SENS
constexpr const char* kFormName = "k_adjoint_sens";
#else
constexpr const char* kFormName = kRole ? "k_adjoint" : "k_forward";
#endif
template <int VAR, bool PLAIN>
constexpr auto form_kernel() {
#if QD_VARS && (QD_PART == 0 || QD_PART == 2)
  return k_forward_vars<QD_Q, kLind, VAR, kQubit, kGmPart, PLAIN>;
#elif QD_VARS
  return k_adjoint_vars<QD_Q, kLind, VAR, kQubit, kGmPart, PLAIN>;
#elif QD_SENS
  return k_adjoint_sens<QD_Q, kLind, VAR, kQubit, kGmPart, PLAIN>;
#elif QD_PART == 0 || QD_PART == 2
  return k_forward<QD_Q, kLind, VAR, kQubit, kGmPart, PLAIN, kSets>;
#else
  return k_adjoint<QD_Q, kLind, VAR, kQubit, kGmPart, PLAIN, kSets>;
#endif
}
// the launch sequence of every form and both directions (the general instantiation named before the PLAIN one)
template <int VAR>
static hipError_t go_lds(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  auto kf = form_kernel<VAR, false>();
  bool plain = false;
  if constexpr ((VAR == 0 || VAR == 1) && !kGmPart) {
    plain = plain_sweep(a, cfg, kRole);
    if (plain) kf = form_kernel<VAR, true>();
  }
  hipError_t e = set_lds(kf, cfg.lds);
  if (e != hipSuccess) return e;
  if constexpr (kSets) note_kernel(kRole, kFormName, QD_Q, kLind, VAR, kQubit, kGmPart, plain, true);
  else note_kernel(kRole, kFormName, QD_Q, kLind, VAR, kQubit, kGmPart, plain);
  hipLaunchKernelGGL(kf, dim3(a.nb), dim3(cfg.block), cfg.lds, st, a);
  return hipGetLastError();
}

#if QD_PART == 0 || QD_PART == 2
template <int VAR>
static hipError_t go_forward(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  if constexpr (VAR == 16 && !kSets && !kVars && variant_built(QD_Q, kLind, QD_B, VAR)) {
    note_kernel(0, "k_forward_big", QD_Q, kLind, kDense, kGmPart);
    return launch_big(reinterpret_cast<const void*>(k_forward_big<QD_Q, kLind, kDense, kGmPart>), a, cfg, st);
  } else if constexpr (VAR != 16 && variant_built(QD_Q, kLind, QD_B, VAR)) {
    return go_lds<VAR>(a, cfg, st);
  } else {
    return hipErrorInvalidValue;
  }
}
#endif
#if QD_PART == 0 && !QD_SETS && !QD_VARS
template <int VAR>
static hipError_t go_apply(const DevSys& S, const double* ctlrow, int transpose, const double* x, double* y, int nb,
                           const LaunchCfg& cfg, hipStream_t st) {
  if constexpr (VAR == 16 && variant_built(QD_Q, kLind, QD_B, VAR)) {
    DevSys S1 = S;  // one operator application: no exchange between workgroups after the load, no team needed
    S1.team = 1;
    note_kernel(2, "k_apply_big", QD_Q, kLind, kDense);
    hipLaunchKernelGGL((k_apply_big<QD_Q, kLind, kDense>), dim3(nb), dim3(cfg.block), cfg.lds, st, S1, ctlrow, transpose, x, y, nb);
    return hipGetLastError();
  } else if constexpr (variant_built(QD_Q, kLind, QD_B, VAR)) {
    auto kf = k_apply<QD_Q, kLind, VAR, kQubit>;
    hipError_t e = set_lds(kf, cfg.lds);
    if (e != hipSuccess) return e;
    note_kernel(2, "k_apply", QD_Q, kLind, VAR, kQubit);
    hipLaunchKernelGGL(kf, dim3(nb), dim3(cfg.block), cfg.lds, st, S, ctlrow, transpose, x, y, nb);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

#endif
#if QD_PART == 1 || QD_PART == 3
template <int VAR>
static hipError_t go_adjoint(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  if constexpr (VAR == 16 && !kSets && !kVars && !kSens && variant_built(QD_Q, kLind, QD_B, VAR)) {
    if constexpr (!kGmPart) {
      if (a.stepper_ee) {
        note_kernel(1, "k_adjoint_big", QD_Q, kLind, kDense, false, true);
        return launch_big(reinterpret_cast<const void*>(k_adjoint_big<QD_Q, kLind, kDense, false, true>), a, cfg, st);
      }
    }
    note_kernel(1, "k_adjoint_big", QD_Q, kLind, kDense, kGmPart, false);
    return launch_big(reinterpret_cast<const void*>(k_adjoint_big<QD_Q, kLind, kDense, kGmPart, false>), a, cfg, st);
  } else if constexpr (VAR != 16 && variant_built(QD_Q, kLind, QD_B, VAR)) {
    return go_lds<VAR>(a, cfg, st);
  } else {
    return hipErrorInvalidValue;
  }
}
#endif

#define QD_VAR_SWITCH(FN, ...)               \
  switch (cfg.var) {                         \
    case 0: return FN<0>(__VA_ARGS__);       \
    case 1: return FN<1>(__VA_ARGS__);       \
    case 2: return FN<2>(__VA_ARGS__);       \
    case 4: return FN<4>(__VA_ARGS__);       \
    case 9: return FN<9>(__VA_ARGS__);       \
    case 11: return FN<11>(__VA_ARGS__);     \
    case 12: return FN<12>(__VA_ARGS__);     \
    case 13: return FN<13>(__VA_ARGS__);     \
    case 14: return FN<14>(__VA_ARGS__);     \
    case 15: return FN<15>(__VA_ARGS__);     \
    case 17: return FN<17>(__VA_ARGS__);     \
    case 16: return FN<16>(__VA_ARGS__);     \
    default: return hipErrorInvalidValue;    \
  }

#if QD_VARS
#define QD_FWD inst_forwardvars_
#define QD_FWDGM inst_forwardgmvars_
#define QD_ADJ inst_adjointvars_
#define QD_ADJGM inst_adjointgmvars_
#elif QD_SENS
#define QD_ADJ inst_adjointsens_
#define QD_ADJGM inst_adjointgmsens_
#elif QD_SETS
#define QD_FWD inst_forwardsets_
#define QD_FWDGM inst_forwardgmsets_
#define QD_ADJ inst_adjointsets_
#define QD_ADJGM inst_adjointgmsets_
#else
#define QD_FWD inst_forward_
#define QD_FWDGM inst_forwardgm_
#define QD_ADJ inst_adjoint_
#define QD_ADJGM inst_adjointgm_
#endif
#if QD_PART == 0
hipError_t QD_NAME(QD_FWDGM, QD_Q, QD_L, QD_B)(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st);
hipError_t QD_NAME(QD_FWD, QD_Q, QD_L, QD_B)(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  if (cfg.gmres) return QD_NAME(QD_FWDGM, QD_Q, QD_L, QD_B)(a, cfg, st);  // GMRES kernels: another object
  QD_VAR_SWITCH(go_forward, a, cfg, st)
}
#if !QD_SETS && !QD_VARS
hipError_t QD_NAME(inst_apply_, QD_Q, QD_L, QD_B)(const DevSys& S, const double* ctlrow, int transpose, const double* x, double* y,
                                                  int nb, const LaunchCfg& cfg, hipStream_t st) {
  QD_VAR_SWITCH(go_apply, S, ctlrow, transpose, x, y, nb, cfg, st)
}
#endif
#elif QD_PART == 1
hipError_t QD_NAME(QD_ADJGM, QD_Q, QD_L, QD_B)(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st);
hipError_t QD_NAME(QD_ADJ, QD_Q, QD_L, QD_B)(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  if (cfg.gmres && !(cfg.var == 16 && a.stepper_ee)) return QD_NAME(QD_ADJGM, QD_Q, QD_L, QD_B)(a, cfg, st);  // (explicit Euler has no linear solve)
  QD_VAR_SWITCH(go_adjoint, a, cfg, st)
}
#elif QD_PART == 2
hipError_t QD_NAME(QD_FWDGM, QD_Q, QD_L, QD_B)(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  QD_VAR_SWITCH(go_forward, a, cfg, st)
}
#else
hipError_t QD_NAME(QD_ADJGM, QD_Q, QD_L, QD_B)(const SweepArgs& a, const LaunchCfg& cfg, hipStream_t st) {
  QD_VAR_SWITCH(go_adjoint, a, cfg, st)
}
#endif
#if QD_B == 0 && QD_PART == 0 && !QD_SETS && !QD_VARS
hipError_t QD_NAME(inst_bigtable_, QD_Q, QD_L, QD_B)(const DevSys& S, double* ecoef, unsigned* edig, hipStream_t st) {
  hipLaunchKernelGGL((k_big_table<QD_Q, kLind>), dim3((S.dim + 255) / 256), dim3(256), 0, st, S, reinterpret_cast<double2*>(ecoef),
                     reinterpret_cast<uint2*>(edig));
  return hipGetLastError();
}
#endif

}  // namespace qd

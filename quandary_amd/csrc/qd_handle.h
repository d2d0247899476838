// Host-side state behind the opaque qd_handle (one per GPU, single-threaded like the reference's
// TimeStepper/MasterEq objects).  Internal; the public boundary is include/quandary_amd.h.
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "qd_col_vars.h"
#include "qd_gauge.h"
#include "qd_internal.h"

#define QD_HIP(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) {                                                                            \
      qd::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                                \
      return (_e == hipErrorOutOfMemory) ? QD_ERR_NOMEM : QD_ERR_DEVICE;                               \
    }                                                                                                  \
  } while (0)

namespace qd {

// Entry points select the handle's device and drop whatever error an earlier, unrelated HIP call of this thread left behind
// (the launch wrappers report hipGetLastError(), which is sticky per thread).
inline hipError_t use_device(int device) {
  const hipError_t e = hipSetDevice(device);
  (void)hipGetLastError();
  return e;
}

// GHz -> rad/ns of the standard model's constants (src/mastereq.cpp:14-60): THE conversion - qd_create uses it for the handle's system,
// the model-parameter ensemble for its variants, so that a variant has the bits a handle created with its constants would have
inline double model_detune(double transfreq_ghz, double rotfreq_ghz) { return 2.0 * M_PI * (transfreq_ghz - rotfreq_ghz); }
inline double model_kerr(double ghz) { return 2.0 * M_PI * ghz; }
inline double model_coupling(double ghz) {  // threshold of Jkl_coupling (mastereq.hpp:633)
  const double j = 2.0 * M_PI * ghz;
  return std::fabs(j) > 1e-10 ? j : 0.0;
}

hipError_t launch_observables(const DevSys& S, const double* traj, int f32, int nb, int nstages, int stride, int nout, int nlev_total,
                              double* expected, double* population, double* expcomp, double* popcomp, hipStream_t st);

// sampled controls (qd_optim_evalF_sampled; kernels in qd_kernels.hip): the control table [nrows][cs] from samples [nsamp][Q][2] read
// by `mode` (QD_SAMPLED_*; T = ntime dt) - what launch_controls2 does from spline parameters, the energy-penalty table apart - and the
// gradient per sample, grad [nsamp][Q][2], from the row sums coeffsum [nrows][2 Q] the adjoint sweep leaves
hipError_t launch_table_sampled(const DevCtlDesc& d, int mode, int nsamp, const double* samples, double T, const double* times, const double* hs,
                                int nrows, double* table, int cs, unsigned long long* zero_me, hipStream_t st);
hipError_t launch_grad_sampled(int Q, int mode, int nsamp, double T, const double* table, int cs, int nrows, const double* coeffsum, double* grad,
                               hipStream_t st);

// growable device buffer of doubles
struct DBuf {
  double* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return QD_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    QD_HIP(hipMalloc(reinterpret_cast<void**>(&p), sizeof(double) * (n > 0 ? n : 1)));
    cap = n;
    return QD_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// growable PINNED host buffer: the target of the asynchronous result downloads (one stream
// synchronisation per sweep instead of one blocking copy per result array)
struct HBuf {
  double* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return QD_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    QD_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(double) * (n > 0 ? n : 1), hipHostMallocDefault));
    cap = n;
    return QD_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Kernel family of a sweep or an operator application.  The values 0-3 are also the layout tags of the stored primal stages
// (qd_handle::ztraj_fmt): 1 = fp32 pairs, 0 / 2 / 3 = fp64 pairs in the element order of the general / slot / lean column kernels.
// General: one workgroup per state, vectors in LDS (qd_device.h); F32 / Slot: slot kernels in fp32-mixed / fp64 ("lean64", qd_q32.hip);
// Col: lean column kernels (qd_col.hip); Global: vectors in global memory, teams of workgroups (qd_big.h, variant 16).
enum class Family { General = 0, F32 = 1, Slot = 2, Col = 3, Global = 4 };

// (Form, the second axis of the same decision: qd_internal.h, shared with the kernel units.)

// Gershgorin bounds of a row of M for the current parameters (qd_handle::row_bounds) and the largest alpha = |h| / 2 of the step
// schedule: what every solver gate looks at, computed once per plan
struct RowBound { double diag, off, amax; };

// Everything the host decides about one sweep before it launches it (qd_handle::plan_sweep)
struct SweepPlan {
  Family family;
  Form form;           // from the handle's state when the plan is made: nothing downstream looks at the sweep's arguments to find it out
  LaunchCfg cfg;       // final configuration (a stand-in for GMRES has re-picked it)
  int solver;          // QD_SOLVER_*: the iteration that solves the linear systems (qd_last_solver)
  int neumann_split, stop_residual, maxiter_factor;  // SweepArgs fields of the same names (maxiter: x linearsolver_maxiter); use_gmres = cfg.gmres
  double kappa2;
  float standin_tau2;
  int gated_poly;      // degree the contraction gate gives the Krylov solver of the picked configuration (adjoint: the forward sweep's, fwd_poly)
  int gmres_poly;      // degree handed to the kernel
  int tuner_poly;      // degree the tuner accounts the sweep's applications to (last_poly; 1 = not a preconditioned Krylov sweep)
  int team;            // workgroups per initial condition (qd_last_team)
  size_t kry_doubles;  // Krylov basis in global memory (SweepArgs::kry), 0 = none
  bool need_big;       // ensure_big before the launch
  // the global-memory kernels store the stages in the element order of the general ones
  Family stage_layout() const { return family == Family::Global ? Family::General : family; }
  // Kernels of the plan's form exist for its family and solver:
  // Sets: the general family - the standard model and the dense user Hamiltonians of the LDS kernels alike -, and under option batch_lean
  //   the lean slot, fp32-mixed and lean column families where the kernel's solver is a stationary iteration (their Krylov kernels have
  //   no SETS form);
  // Vars: the diagonal-split stationary iteration of the lean column family (k_*_col_vars), under option ensemble_general the general
  //   family - Neumann and both direct Krylov forms (k_forward_vars / k_adjoint_vars) -, under option ensemble_lean the lean slot and
  //   fp32-mixed families where the kernel's solver is a stationary iteration (k_forward_q32_vars / k_adjoint_q32_vars: a neumann request
  //   or a gmres request served by the Neumann stand-in; their Krylov kernels have no variants form);
  // Sens: the general family (k_adjoint_sens) and, under option sens_lean, the diagonal-split stationary iteration of the lean column
  //   family (k_adjoint_col_sens / k_adjoint_colj_sens: a neumann request, or a gmres request served by that iteration; their Krylov
  //   and plain-Neumann kernels have no sensitivity form); under option sens_slot the fp64 lean slot family where the kernel's solver is
  //   a stationary iteration (k_adjoint_q32_sens: a neumann request or a gmres request served by the stand-in; no Krylov and no
  //   fp32-mixed kernel has the form).
  bool form_built(const TuneOpts& o) const {
    const bool slot = family == Family::Slot || family == Family::F32, stationary = cfg.gmres == 0;
    switch (form) {
      case Form::Plain: return true;
      case Form::Sets: return family == Family::General || (o.batch_lean && (slot || family == Family::Col) && stationary);
      case Form::Vars:
        return (family == Family::Col && stationary && neumann_split) || (family == Family::General && o.ensemble_general) ||
               (o.ensemble_lean && slot && stationary);
      case Form::Sens:
        return family == Family::General || (o.sens_lean && family == Family::Col && stationary && neumann_split) ||
               (o.sens_slot && family == Family::Slot && stationary);
      case Form::Pair: return family == Family::Col && stationary;
    }
    return false;
  }
};

}  // namespace qd

struct qd_handle {
  int device = 0;
  int precision = QD_PRECISION_F64;  // qd_set_precision
  qd::TuneOpts opts;                 // qd_set_option (+ environment overrides read at qd_create)
  // ---- which kernel family and which linear solver a sweep runs on: decided once per launch, in plan_sweep (qd_handle.cpp) ----
  qd::SweepPlan plan_sweep(int nb, bool adjoint) const;
  qd::Family apply_family(const qd::LaunchCfg& cfg) const;  // the same choice for one operator application (qd_apply_rhs)
  // named steps of plan_sweep, described where they are defined; nothing else calls them
  qd::Family pick_family(const qd::LaunchCfg& cfg, bool slot, bool col) const;
  // the sweep runs on the lean column kernels (qd_col.hip, coupled systems qd_colj.hip); split = the plan's neumann_split
  bool col_sweep(const qd::LaunchCfg& cfg, const qd::RowBound& b, int split) const;
  int neumann_split_on(const qd::RowBound& b) const;  // diagonal-split Neumann iteration for the current parameters
  // linearsolver_type = gmres served by the diagonal-split iteration of the lean column kernels under GMRES's stopping rule;
  // *kappa2 = (1 + max alpha |D|)^2, the factor between the squared update norm and the bound of the squared residual
  bool gmres_as_split(const qd::LaunchCfg& cfg, const qd::RowBound& b, double* kappa2) const;
  bool gmres_as_neumann(const qd::LaunchCfg& cfg, const qd::RowBound& b) const;  // ... by the plain Neumann iteration of any other kernel family
  // the decision of the two gates, latched per handle: -1 undecided, 0 Krylov kernels, 1 diagonal-split iteration, 2 Neumann iteration
  mutable int sub_latch = -1;
  bool params_set = false;  // qd_set_params has been called (the gates look at the control amplitudes)
  bool latched_substitution(int kind, double bound) const;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;  // forward / adjoint kernel brackets
  qd::DevSys S{};
  qd_time tg{};
  qd_solver sol{};
  qd_penalty pen{};
  // controls (host description + device mirror)
  std::vector<qd::DevSeg> segs;
  std::vector<qd::DevOsc> oscs;
  std::vector<double> carriers, pulses;
  qd::DevCtlDesc dctl{};
  qd::DevSeg* d_segs = nullptr;
  qd::DevOsc* d_oscs = nullptr;
  double *d_carriers = nullptr, *d_pulses = nullptr;
  int ndesign = 0, dim_ess = 1;
  int last_team = 1;  // workgroups per initial condition of the last sweep (qd_big.h)
  int last_solver = 0;  // QD_SOLVER_* of the last sweep (qd_last_solver)
  std::string last_kernel[3];  // instantiation last launched per role: forward, adjoint, apply (qd_last_kernel)
  bool has_pipulse = false;
  bool has_ampbasis = false;  // a spline_amplitude segment: forward only (src/oscillator.cpp:350-356)
  std::vector<double> params;
  qd::DBuf d_params;
  qd::DBuf d_tbar, d_tred;  // team barrier counters / partial sums of the global-memory sweeps (qd_big.h)
  bool params_dirty = true;
  bool napply_zeroed = false;  // the control kernel of this parameter update has already reset d_napply
  // step schedule
  int nstages = 1, nsub = 0, cs = 0;
  std::vector<double> sched_t, sched_h, etimes;  // host copies
  qd::DBuf d_sched_t, d_sched_h, d_etimes, d_ezero, d_table, d_etable, d_onerow, d_onetime;
  qd::HBuf h_etable;  // energy-penalty table rows, downloaded with the sweep results
  qd::HBuf h_res;     // per-state results of the last forward sweep: [pen nb | dpdm nb | out4 4nb | napply]
  qd::HBuf h_params;  // staging copy of the control parameters
  // target for in-loop / final objective terms
  bool target_set = false;
  qd::DevTarget dtg{};
  qd::DBuf d_tstates, d_purity;
  int target_nb = 0;
  // sweep buffers
  qd::DBuf d_ztraj;  // stored primal stages (SweepArgs::ztraj)
  qd::DBuf d_wjw;    // Gaussian weights of the weighted-J penalty per time step (SweepArgs::wjw)
  double wjw_param = -1.0;
  int ensure_wj_weights();
  qd::DBuf d_x0, d_xT, d_traj, d_res, d_xbar, d_jbar, d_coeff, d_coeffsum, d_grad, d_y, d_stash, d_kry;
  qd::DBuf d_ecoef, d_edig, d_work;  // large states (qd_big.h): element table, work vectors
  qd::DBuf d_sched;                  // scheduler words of the time-sliced lean column sweeps (forward | adjoint)
  qd::HBuf h_sched;                  // their error words, downloaded with the sweep
  bool sliced_fwd = false, sliced_adj = false;
  int arm_slices(qd::SweepArgs& a, int nb, int which);
  int ensure_big(int nb);            // no-op unless the launch configuration is the large-state variant
  qd::DBuf d_g0, d_hcr, d_hci, d_gtab, d_gone;  // dense user-Hamiltonian path (qd_set_hamiltonian)
  // Phasor table of the real-drive frame (qd_gauge.h), one row per row of d_table: what the lean column forward kernels of the
  // diagonal-split solver without coupling read in place of forming r_k and the row phasors per wave and sub-step.  gauge_wanted: the
  // handle's plan can select such a kernel - whatever neumann_split says now, the option may change after qd_create; refresh_tables
  // then builds the table with the control table.  prepare_sweep builds it for a lean column sweep that finds it stale all the same
  // (an option that admits the family only later).  gauge_valid: d_gauge belongs to the current d_table.
  qd::DBuf d_gauge;
  bool gauge_valid = false;
  bool gauge_wanted() const;
  int gauge_table();
  // infinity norms of the uploaded Hamiltonians (row_bounds: the standard-model constants say nothing about a user Hamiltonian)
  double dense_hsys_norm = 0.0;
  std::vector<double> dense_hc_norm;  // per oscillator: ||Re Hc_k||_inf + ||Im Hc_k||_inf
  // d_res = [pen nb | dpdm nb | out4 4nb | napply]: one contiguous block, one download per sweep
  double *d_pen = nullptr, *d_dpdm = nullptr, *d_out4 = nullptr;
  unsigned long long* d_napply = nullptr;
  int last_nb = 0;
  bool traj_valid = false;
  qd::Family ztraj_fmt = qd::Family::General;  // layout of the stored primal stages = the family that wrote them (SweepPlan::stage_layout)
  double last_mean_applies = 0.0, last_fwd_ms = 0.0, last_adj_ms = 0.0;
  bool accumulate_fwd_ms = false;  // chunked re-propagation (qd_optim_adjoint_local): add the chunks' forward times up

  // ---- internal device-pointer API used by the objective level (qd_optim.cpp) -------------------
  int refresh_tables();
  mutable double hmax_cache = -1.0;  // max |h(I)| over the level combinations (system constant, computed on first use)
  double control_amplitude_bound(int k) const;       // max_t |p_k(t)|, |q_k(t)| for the current parameters
  void row_bounds(double* diag, double* off) const;  // Gershgorin bounds of a row of M over all sub-steps (current parameters)
  int gmres_poly_degree(bool lean_col, const qd::RowBound& b) const;  // > 1 where the Neumann series provably contracts for the current parameters, else 1
  // degree of the polynomial preconditioner, tuned from sweep to sweep (forward_finish): smallest degree with one Krylov vector per solve
  int poly_cur = 6, poly_lo = 1, poly_hi = 0, last_poly = 1, poly_steps = 0;
  int fwd_poly = 0;  // degree the last forward sweep ran on (the adjoint sweep of the same evaluation keeps it)
  int poly_start() const { return S.dim <= 1024 ? 3 : 6; }  // first degree the tuner tries (small systems contract fast)
  int poly_slow = 0;         // consecutive sweeps of a frozen degree with more than 1.5 Krylov vectors per solve
  bool poly_frozen = false;  // the bracket has closed: the degree no longer changes (reproducible evaluations)
  int traj_doubles(int nb, size_t* n) const;
  size_t ztraj_doubles(int nb) const;  // 0 for explicit Euler
  // forward sweep on device-resident states; results stay on the device (d_pen, d_dpdm, d_xT, d_out4)
  // (dxpair: the same states as Hermitian pairs, [(nb + 1) / 2][2 dim] - where the caller knows every state to be exactly Hermitian)
  int forward_dev(const double* dx0, int nb, bool store, const qd::DevTarget* tg, double* energy, const double* dxpair = nullptr);
  // the same in two halves: enqueue only / synchronise and collect (lets the caller queue the reductions, the adjoint
  // sweep and the collectives behind the forward sweep without a host round trip)
  int forward_launch(const double* dx0, int nb, bool store, const qd::DevTarget* tg, const double* dxpair = nullptr);
  int forward_finish(double* energy);
  // Hermitian pairs.  M(t) is complex-linear on vec(rho) and maps Hermitian to Hermitian, and so is every step of the lean column
  // stationary solve: for Hermitian rho_a, rho_b one sweep of X = rho_a + i rho_b carries both, rho_a(t) = (X + X^dagger) / 2 and
  // rho_b(t) = (X - X^dagger) / 2i.  A forward sweep that stores nothing then runs ceil(nb / 2) tasks on the same kernel, sums the
  // in-loop penalties of the members apart (qd_col.h) and un-pairs the final states into d_xT, where the objective kernels and every
  // caller find the nb states they find after an unpaired sweep.  pair_gate: the plan (made for the paired count) and the call admit
  // it, and the sweep then runs in the form Form::Pair - Lindblad without coupling, one control vector, nothing stored, the plain form of the lean column family with the stationary
  // solver serving a neumann request under the absolute rule alone (the stopping test then sees ||dX||^2 = ||d rho_a||^2 + ||d rho_b||^2:
  // each member meets the reference's rule), and no in-loop penalty that reads off-diagonal elements; option pair_hermitian.
  bool pair_gate(const qd::SweepPlan& plan, int nb, bool store, const qd::DevTarget* tg) const;
  qd::DBuf d_xpT;            // the propagated pairs: carry between time slices, source of the un-pairing
  bool last_paired = false;  // the last forward sweep ran on pairs
  int last_solved = 0;       // states its kernel propagated: last_nb, or (last_nb + 1) / 2 pairs
  int adjoint_launch(const double* dxbarT, const double* djbar, int nb, const qd::DevTarget* tg, bool accumulate);
  int adjoint_finish(bool accumulate);
  int gradient_launch(double ebar, double* dgrad);  // k_grad into a device buffer [ndesign]
  bool pending_store = false;
  // Gradient evaluations of the objective level (qd_optim.cpp) set stages_only: the forward sweep then stores the primal stages z only
  // (SweepArgs::ztraj) wherever the adjoint sweep of the same kernel family reads nothing else - half the store traffic and half the
  // trajectory memory.  traj_full: d_traj holds the states x_n of the last stored sweep (qd_get_state, qd_get_observables, penalties
  // with state-dependent adjoints, explicit Euler).
  bool stages_only = false, traj_full = false, pending_full = false;
  bool adjoint_reads_states(int nb, const qd::DevTarget* tg, const qd::SweepPlan* plan = nullptr) const;  // plan: the sweep's, where the caller has it
  // what the two launches share once the plan is made: SweepArgs from the handle and the plan, Krylov buffer, the records of the sweep
  int prepare_sweep(qd::SweepArgs& a, const qd::SweepPlan& p, int nb, const qd::DevTarget* tg);
  bool stores_full(int nb, const qd::DevTarget* tg) const { return !stages_only || adjoint_reads_states(nb, tg); }
  // adjoint sweep; dxbarT/djbar device pointers; coefficient sums accumulate into d_coeffsum
  int adjoint_dev(const double* dxbarT, const double* djbar, int nb, const qd::DevTarget* tg, bool accumulate);
  // gradient from d_coeffsum (+ energy term ebar); writes host grad[ndesign] - during a sampled call grad[samp_n][Q][2], per sample
  int gradient_from_coeffs(double ebar, double* grad);
  double energy_penalty_host() const;
  // ---- parameter-set batch (qd_optim_evalF_batch / qd_optim_evalGradF_batch, qd_optim.cpp) --------------------------------------
  // Several control vectors in one sweep launch: the batch of a sweep is `sets` sets of nb / sets states, set j reads the control
  // table batch_table() + j * batch_ctl_set().  While sets > 0 the sweeps use these tables and leave the handle's own (d_table) alone;
  // plan_sweep decides from batch_bound, the Gershgorin row bound maximised over all sets of the call.
  int sets = 0;                    // sets of the sweeps being launched (0 = ordinary sweeps)
  int batch_first = 0;             // first set of the group being swept (tables of all sets of the call are resident)
  qd::RowBound batch_bound{};
  qd::DBuf d_bparams, d_btable, d_betable, d_bgrad;
  // dense user Hamiltonians: the group's tables of G(t) = -i H(t), one per set, batch_gtab_set() doubles apart (batch_gtables; the
  // handle's own d_gtab and S.gtab are left alone like d_table)
  qd::DBuf d_bgtab;
  int bgtab_first = 0, bgtab_sets = 0;  // the sets whose tables d_bgtab holds (0 sets = none)
  // (the lean column systems, which are never dense: the group's phasor tables in the same buffer under the same bookkeeping, one per
  // set, rows x GAUGE_STRIDE doubles apart - memory that lies beside the trajectory and is weighed with it the same way)
  size_t batch_gtab_set() const {  // the rows of batch_ctl_set() x N^2 complex
    return S.dense ? sched_t.size() * (size_t)S.N * S.N * 2 : gauge_wanted() ? sched_t.size() * (size_t)qd::GAUGE_STRIDE : 0;
  }
  int batch_gtables(int first, int nsets);  // G(t) / phasor tables of the sets [first, first + nsets) from their control tables, one launch
  qd::HBuf h_bparams, h_betable, h_bgrad;
  // ensemble of system variants (qd_optim_evalF_ensemble / qd_optim_evalGradF_ensemble): one control vector, nvar matrices Hsys.  d_eg0
  // holds their G0 = -i Hsys, ens_g0_set() doubles apart.  While ens_g0 is set the G(t) tables are built from it instead of d_g0: set j of
  // a batch from ens_g0 + j * ens_g0_set() (batch_gtables: the variants of one launch), an ordinary sweep from ens_g0 itself
  // (refresh_tables: the variant-by-variant fallback).  dense_hsys_norm is the caller's to set beside it and to restore.
  qd::DBuf d_eg0;
  const double* ens_g0 = nullptr;
  size_t ens_g0_set() const { return (size_t)2 * S.N * S.N; }
  int ensemble_upload(int nvar, const double* hsys_re, const double* hsys_im, std::vector<double>& norms);  // norms: rowsum_max per variant
  // Model-parameter ensemble (qd_optim_evalF_ensemble_model / qd_optim_evalGradF_ensemble_model): one control vector, nvar variants of the
  // standard model's constants.  vars_host holds their blocks [nvar][col_vars_stride] in rad/ns (qd_col_vars.h; model_constants makes
  // them what qd_create would), d_vconst the device copy.  While vars_tab is set a batch on the lean column family reads variant j's
  // block for set j (prepare_sweep, launch_sweep: k_*_col_vars), and batch_begin takes vars_bound - the row bounds maximised over the
  // variants - in place of the handle's own: one plan for all of them.  The fallback points the handle at one variant after the other
  // (point_at_variant); ModelConstants is what it swaps and what the caller's scope restores.
  std::vector<double> rotfreq;  // GHz, as given to qd_create (a variant keeps the rotating frame)
  struct ModelConstants { double detune[QD_MAX_OSC], xi[QD_MAX_OSC], xikl[QD_MAX_PAIRS], J[QD_MAX_PAIRS]; double hmax; };
  ModelConstants model_constants_now() const;
  void set_model_constants(const ModelConstants& m);  // S and everything derived from it: the cached level-energy bound, the element table of the global-memory kernels
  void point_at_variant(int j);
  bool ecoef_valid = false;  // d_ecoef / d_edig belong to the current constants (ensure_big)
  std::vector<double> vars_host;
  qd::DBuf d_vconst;
  qd::DBuf d_pencarry;  // penalty sums carried between the time slices of such a launch (qd_col_vars.h)
  const double* vars_tab = nullptr;
  qd::RowBound vars_bound{};
  int variants_upload(int nvar, const double* blocks, const double* alpha);  // d_vconst, vars_host and vars_bound (at the control vector alpha)
  // Model-constant sensitivities (qd_optim_evalGradF_model): while sens is set the adjoint sweep runs on the sensitivity form of the
  // general family (k_adjoint_sens, qd_sens.h) or, under option sens_lean, of the lean column family (k_adjoint_col_sens /
  // k_adjoint_colj_sens, qd_col.h), under option sens_slot of the lean slot family (k_adjoint_q32_sens, qd_q32.hip) - any other plan is
  // an error - and leaves the sums over the states of
  // kbar^T (dM/d theta) z in d_senssum [2 Q + npairs]: detunings, self-Kerr, cross-Kerr coefficients, in rad/ns and without the factors
  // -1/2 and -1 of the Kerr terms (the caller applies them with the unit).  d_sens: the sums the kernel stores, one row per state
  // (lean column family: per state and time slice).
  bool sens = false;
  qd::DBuf d_sens, d_senssum;
  // Sampled controls (qd_optim_evalF_sampled / qd_optim_evalGradF_sampled): while samp_mode >= 0 the handle's controls are the samples
  // in d_samples [samp_n][Q][2], read by mode samp_mode (QD_SAMPLED_*), not the spline parameters: refresh_tables fills d_table from
  // them (k_table_sampled), control_amplitude_bound - and through it row_bounds and every solver gate - answers with samp_bound[k] =
  // max_j max(|p_jk|, |q_jk|) (each mode reads convex combinations of the samples, so this bounds every row), and gradient_from_coeffs
  // writes d objective / d sample [samp_n][Q][2] (k_grad_sampled).  `params` and d_params are not touched.
  int samp_mode = -1, samp_n = 0;
  qd::DBuf d_samples, d_sgrad;
  qd::HBuf h_samples;  // staging: the samples on their way up, the gradient on its way down
  std::vector<double> samp_bound;
  int sampled_begin(int mode, int nsamp, const double* samples);  // upload + bounds; the control table is stale from here on
  void sampled_end();                                             // back to the spline parameters: table stale, no stored trajectory
  size_t batch_ctl_set() const { return sched_t.size() * (size_t)cs; }    // rows the step table really has x cs
  size_t batch_etable_set() const { return etimes.size() * (size_t)cs; }
  const double* batch_table() const { return d_btable.p + (size_t)batch_first * batch_ctl_set(); }
  int batch_begin(const double* alphas, int nset);  // tables of all sets in one launch, row bound over all sets
  void batch_end();                                 // back to ordinary sweeps: stored trajectory invalid, control table stale
  double batch_energy_host(int set) const;          // energy_penalty_host of one set of the call
  int batch_gradient(double ebar, int nsets, double* grads);  // k_grad once per set of the group -> host grads [nsets][ndesign]
  const double* res_pen() const { return h_res.p; }
  const double* res_dpdm() const { return h_res.p + last_nb; }
  const double* res_out4() const { return h_res.p + 2 * (size_t)last_nb; }
};

// Communicator (qd_comm.cpp): one per process.  Backend RCCL (one process per GPU, ncclAllReduce over xGMI on the handle's stream) or
// HOST (ranks on one node reducing through a POSIX shared-memory segment: the same call sites, the same buffers, the same fixed summation
// order on every rank - for ranks that share a GPU, which RCCL refuses, and for nodes without RCCL).
namespace qd { struct HostRing; }
struct qd_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, nranks = 1, device = 0;
  int backend = 0;                // 0 RCCL, 1 host shared memory
  qd::HostRing* host = nullptr;   // backend 1
  hipStream_t stream = nullptr;  // for the host-staged convenience calls; the sweeps reduce on the handle's stream
  qd::DBuf dbuf;
  qd::HBuf hbuf;                 // backend 1: pinned staging buffer of the in-stream reductions
};
// in-place all-reduce of a device buffer on stream `st` (op 0 = sum, 1 = max); asynchronous
int qd_comm_allreduce_dev(qd_comm* c, double* dbuf, size_t n, int op, hipStream_t st);

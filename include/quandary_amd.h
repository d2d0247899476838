/*
 * quandary_amd.h — C ABI of the MI355X-native forward/adjoint propagator.
 *
 * This is the drop-in boundary for ONE hot path of LLNL/quandary: propagate a
 * batch of initial conditions through the Lindblad/Schroedinger time stepper,
 * sweep the discrete adjoint backwards and accumulate the control-parameter
 * gradient.  All entry points are extern "C", take plain pointers and sizes,
 * return 0 on success and a negative QD_ERR_* code on failure (the message is
 * available from qd_last_error()).  Nothing here calls exit().
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the reference repository):
 *
 *   qd_create / qd_destroy      MasterEq ctor + MatShellCtx  (src/mastereq.cpp:14-155,
 *                               include/mastereq.hpp:20-42), Oscillator ctor
 *                               (src/oscillator.cpp:10-214), ImplMidpoint ctor
 *                               (src/timestepper.cpp:522-556)
 *   qd_set_params               MasterEq::setControlAmplitudes (src/mastereq.cpp:693-707)
 *   qd_eval_controls            Oscillator::evalControl (src/oscillator.cpp:281-337)
 *   qd_apply_rhs                MatMult / MatMultTranspose on the MATSHELL, i.e.
 *                               applyRHS_matfree<...> and ..._transpose<...>
 *                               (src/mastereq.cpp:1278-2893, dispatch :2976-3239),
 *                               preceded by MasterEq::assemble_RHS(t) (:657-678)
 *   qd_forward                  TimeStepper::solveODE over the local batch
 *                               (src/timestepper.cpp:96-181) incl. the in-loop
 *                               penalties (:256-298, :342-369, :444-455)
 *   qd_adjoint                  TimeStepper::solveAdjointODE over the local batch
 *                               (src/timestepper.cpp:184-253), ImplMidpoint::evolveBWD
 *                               (:631-694), compute_dRHS_dParams_matfree
 *                               (src/mastereq.cpp:970-1276)
 *   qd_optim_*                  OptimProblem::evalF / evalGradF (src/optimproblem.cpp:224-538)
 *                               with OptimTarget (src/optimtarget.cpp:325-897) and
 *                               Gate::assembleGate/applyGate (src/gate.cpp:88-283)
 *
 * State layout (same as the reference, docs/mkdocs/user_guide.md:305-306): one
 * state is 2*dim doubles, blocked [u ; v] (all real parts, then all imaginary
 * parts); dim = N (Schroedinger) or N^2 (Lindblad, column-major vectorisation
 * vec index = row + col*N, src/util.cpp:150-152); oscillator 0 is the slowest
 * index inside a Hilbert-space index.  A batch is nb states back to back.
 *
 *   qd_set_hamiltonian          HamiltonianFileReader + initSparseMatSolver + applyRHS_sparsemat
 *                               (src/hamiltonianfilereader.cpp, src/mastereq.cpp:192-967) for
 *                               user-supplied Hamiltonians
 *
 * Units follow the reference config file: frequencies in GHz (multiplied by
 * 2*pi inside, src/mastereq.cpp:29-37, src/oscillator.cpp:15-21), times in ns.
 *
 * Supported sizes (QD_ERR_UNSUPPORTED beyond): state dimension dim <= QD_MAX_DIM = 2^22 (one
 * workgroup owns one initial condition; up to 4096 the state lives in the CU's LDS, above it the
 * vectors of a step live in global memory and are exchanged through L2; IMR family);
 * 1..8 oscillators, Schroedinger and Lindblad (the reference's matrix-free templates stop at five, its sparse-matrix path does
 * not: six to eight Lindblad oscillators run on the general stencil - 2^6, dim 4096, in LDS, anything larger in global memory);
 * at most 256 / 64 / 32 / 16 levels per oscillator for <= 4 / 5 / 6 / 7-8 oscillators; user-supplied
 * Hamiltonians: 1..8 oscillators, table of G(t) <= 16 GB.  Control segments: "spline", "spline0", "step" and
 * "spline_amplitude" (the last one forward only, as in the reference: src/oscillator.cpp:350-356).  There is no CPU
 * fallback.
 */
#ifndef QUANDARY_AMD_H
#define QUANDARY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QD_MAX_OSC 8
#define QD_MAX_PAIRS (QD_MAX_OSC * (QD_MAX_OSC - 1) / 2)
#define QD_MAX_DIM (1 << 22)

/* error codes */
#define QD_OK 0
#define QD_ERR_INVALID (-1)   /* bad argument / inconsistent description           */
#define QD_ERR_UNSUPPORTED (-2) /* valid in the reference but not built here       */
#define QD_ERR_DEVICE (-3)    /* HIP runtime error (no device, launch failure ...) */
#define QD_ERR_NOMEM (-4)     /* host or device allocation failed                  */
#define QD_ERR_STATE (-5)     /* call order violated (e.g. adjoint before forward) */

/* LindbladType, include/defs.hpp */
enum { QD_LINDBLAD_NONE = 0, QD_LINDBLAD_DECAY = 1, QD_LINDBLAD_DEPHASE = 2, QD_LINDBLAD_BOTH = 3 };
/* ControlType, include/defs.hpp.  BSPLINEAMP carries no gradient in the reference (src/oscillator.cpp:350-356):
 * the gradient entry points return QD_ERR_UNSUPPORTED for it. */
enum { QD_CTRL_NONE = 0, QD_CTRL_BSPLINE = 1, QD_CTRL_BSPLINE0 = 2, QD_CTRL_STEP = 3, QD_CTRL_BSPLINEAMP = 4 };
/* timestepper = IMR | IMR4 | IMR8 | EE, src/main.cpp:357-366 */
enum { QD_STEPPER_IMR = 0, QD_STEPPER_IMR4 = 1, QD_STEPPER_IMR8 = 2, QD_STEPPER_EE = 3 };
/* linearsolver_type = gmres | neumann, src/main.cpp:342-350 */
enum { QD_LINSOLVE_GMRES = 0, QD_LINSOLVE_NEUMANN = 1 };
/* InitialConditionType, include/defs.hpp / src/optimtarget.cpp:42-53 */
enum {
  QD_INIT_FROMFILE = 0, QD_INIT_PURE = 1, QD_INIT_ENSEMBLE = 2, QD_INIT_DIAGONAL = 3,
  QD_INIT_BASIS = 4, QD_INIT_THREESTATES = 5, QD_INIT_NPLUSONE = 6, QD_INIT_PERFORMANCE = 7
};
/* TargetType / ObjectiveType, include/defs.hpp */
enum { QD_TARGET_GATE = 0, QD_TARGET_PURE = 1, QD_TARGET_FROMFILE = 2 };
enum { QD_OBJ_JFROBENIUS = 0, QD_OBJ_JTRACE = 1, QD_OBJ_JMEASURE = 2 };

/* Physical system: the MatShellCtx parameter block (include/mastereq.hpp:20-42)
 * in config-file units (src/main.cpp:191-316).  Pair order is 01,02,...,0(Q-1),12,...
 * (src/mastereq.cpp:2432-2441). */
typedef struct qd_system {
  int32_t nosc;
  int32_t lindblad_type;               /* QD_LINDBLAD_*                      */
  int32_t nlevels[QD_MAX_OSC];
  int32_t nessential[QD_MAX_OSC];
  double transfreq[QD_MAX_OSC];        /* GHz                                */
  double rotfreq[QD_MAX_OSC];          /* GHz                                */
  double selfkerr[QD_MAX_OSC];         /* GHz                                */
  double crosskerr[QD_MAX_PAIRS];      /* GHz                                */
  double Jkl[QD_MAX_PAIRS];            /* GHz                                */
  double decay_time[QD_MAX_OSC];       /* T1 in ns, <=1e-14 disables         */
  double dephase_time[QD_MAX_OSC];     /* T2 in ns, <=1e-14 disables         */
} qd_system;

/* Control parameterisation (src/oscillator.cpp:45-132, src/controlbasis.cpp).
 * Segments are listed oscillator by oscillator; design vector layout per
 * oscillator is [segment][carrier][2*nsplines] for spline / spline0 (src/controlbasis.cpp:58-59),
 * [segment][carrier][nsplines amplitudes, phase] for spline_amplitude (:127-140) and one parameter
 * (the relative width of the step) for step (:195-206; one carrier: the reference's index
 * skip + 2*carrier runs past the segment's single parameter for more). */
typedef struct qd_controls {
  int32_t enforce_bc;                  /* control_enforceBC                  */
  int32_t nseg_total;
  const int32_t* seg_osc;              /* [nseg_total] owning oscillator     */
  const int32_t* seg_type;             /* [nseg_total] QD_CTRL_*             */
  const int32_t* seg_nsplines;         /* [nseg_total]                       */
  const double* seg_tstart;            /* [nseg_total] ns                    */
  const double* seg_tstop;             /* [nseg_total] ns                    */
  const int32_t* ncarrier;             /* [nosc]                             */
  const double* carrier_freq;          /* concatenated, GHz                  */
  int32_t npipulse;                    /* apply_pipulse entries, already expanded
                                          to every oscillator (src/main.cpp:249-277) */
  const int32_t* pipulse_osc;          /* [npipulse]                         */
  const double* pipulse_tstart;        /* [npipulse]                         */
  const double* pipulse_tstop;         /* [npipulse]                         */
  const double* pipulse_amp;           /* [npipulse] (0 for non-target osc)  */
  const double* seg_param;             /* [nseg_total][3] or NULL.  step: amp1, amp2 (rad/ns, as given in the
                                          config), tramp (ns); spline_amplitude: scaling, -, -         */
} qd_controls;

typedef struct qd_time {
  int32_t ntime;
  double dt;
} qd_time;

typedef struct qd_solver {
  int32_t stepper;                     /* QD_STEPPER_*                       */
  int32_t linsolve;                    /* QD_LINSOLVE_*                      */
  int32_t maxiter;                     /* linearsolver_maxiter               */
  double abstol;                       /* reference: 1e-10 (timestepper.cpp:536) */
  double reltol;                       /* reference: 1e-20 (timestepper.cpp:535) */
  /* Stopping tests.  Neumann (timestepper.cpp:716-717): the update norm ||y_{m+1} - y_m|| against abstol, and against reltol times the
   * first update.  The sweep kernels accumulate the squared update per thread in fp64, scale it by 1 / abstol^2 and reduce it over the
   * workgroup in FP32 (one DPP / LDS round instead of two fp64 ones): the value is only compared with 1, so the fp32 reduction moves the
   * stopping point by at most one part in 1e7 of the tolerance - the iteration counts equal the oracle's on every tested shape
   * (tests assert |applications per step - oracle| < 0.25).  GMRES (Krylov kernels): Hessenberg problem, projections and the
   * recurrence residual in fp64, stop at max(reltol ||b||, abstol) as KSPGMRES (timestepper.cpp:541-550). */
} qd_solver;

/* What the forward sweep needs to evaluate objective-dependent terms inside
 * the time loop (weighted-J penalty, src/timestepper.cpp:262-270) and at the
 * end (OptimTarget::evalJ, src/optimtarget.cpp:712-799). */
typedef struct qd_target {
  int32_t target_type;                 /* QD_TARGET_*                        */
  int32_t objective_type;              /* QD_OBJ_*                           */
  int32_t purestate_id;                /* Hilbert-space index m for PURE     */
  const double* target_states;         /* [nb][2*dim] for GATE/FROMFILE, else NULL */
  const double* purity;                /* [nb] Tr(rho0^2) (optimtarget.cpp:705-707) */
} qd_target;

typedef struct qd_penalty {
  double gamma_penalty;                /* optim_penalty                      */
  double penalty_param;                /* optim_penalty_param                */
  double gamma_penalty_dpdm;           /* optim_penalty_dpdm (Schroedinger)  */
  double gamma_penalty_energy;         /* optim_penalty_energy               */
} qd_penalty;

/* Per-initial-condition results of one forward sweep. */
typedef struct qd_forward_out {
  double* final_states;                /* [nb][2*dim] or NULL                */
  double* penalty_integral;            /* [nb] TimeStepper::penalty_integral */
  double* penalty_dpdm;                /* [nb] TimeStepper::penalty_dpdm     */
  double* energy_penalty;              /* [1]  TimeStepper::energy_penalty_integral */
  double* J_re;                        /* [nb] OptimTarget::evalJ            */
  double* J_im;                        /* [nb]                               */
  double* fid_re;                      /* [nb] HilbertSchmidtOverlap(.,false) */
  double* fid_im;                      /* [nb]                               */
} qd_forward_out;

typedef struct qd_handle qd_handle;

const char* qd_last_error(void);
const char* qd_version(void);
/* number of HIP devices visible, or a negative QD_ERR_DEVICE */
int qd_device_count(void);

int qd_create(const qd_system* sys, const qd_controls* ctl, const qd_time* tg, const qd_solver* sol,
              int device_ordinal, qd_handle** out);
void qd_destroy(qd_handle* h);

/* sizes derived from the description */
int qd_dim(const qd_handle* h);        /* dim = N or N^2                       */
int qd_dim_rho(const qd_handle* h);    /* N                                    */
int qd_dim_ess(const qd_handle* h);    /* prod nessential                      */
int qd_ndesign(const qd_handle* h);    /* number of control parameters         */

/* User-supplied Hamiltonians, the reference's `hamiltonian_file_Hsys` / `hamiltonian_file_Hc` model
 * (src/hamiltonianfilereader.cpp, applied by applyRHS_sparsemat src/mastereq.cpp:743-967): dense complex
 * N x N matrices (N = qd_dim_rho), row-major, in rad/ns.  hc_re / hc_im hold nosc matrices back to back
 * (NULL = no control Hamiltonians, the reference's "none").  They REPLACE the standard Hamiltonian model of
 * the qd_system description - detuning, Kerr terms, dipole coupling, ladder-operator controls:
 *     H(t) = Hsys + sum_k p_k(t) Re(Hc_k) + i q_k(t) Im(Hc_k),
 * the T1/T2 dissipators of qd_system stay.  Call before the first sweep. */
int qd_set_hamiltonian(qd_handle* h, const double* hsys_re, const double* hsys_im, const double* hc_re, const double* hc_im);

int qd_set_params(qd_handle* h, const double* alpha, int ndesign);
/* p_k(t), q_k(t) for every oscillator at nt times; pq is [nt][nosc][2] */
int qd_eval_controls(qd_handle* h, const double* times, int nt, double* pq);
/* y = M(t) x (transpose=0) or M(t)^T x (transpose=1) for nb states */
int qd_apply_rhs(qd_handle* h, double t, int transpose, const double* x, double* y, int nb);

/* Trajectory access after qd_forward(..., store_trajectory=1): copies state n
 * (0..ntime) of every local initial condition, [nb][2*dim]. */
int qd_get_state(qd_handle* h, int timestep, double* x);

/* Observables of the stored trajectory, reduced on the device (Oscillator::expectedEnergy / population
 * src/oscillator.cpp:430-566, MasterEq::expectedEnergy / population src/mastereq.cpp:2897-2974; what
 * Output::writeTrajectoryDataFiles prints, src/output.cpp:203-273) for the time steps 0, stride, 2 stride, ... <= ntime
 * (nout = ntime / stride + 1 of them) of every local initial condition.  Any output pointer may be NULL.
 *   expected             [nout][nb][nosc]              expected energy level of oscillator k
 *   population           [nout][nb][sum_k nlevels[k]]  level populations, oscillator k's block after those of 0..k-1
 *   expected_composite   [nout][nb]                    sum_I I P(I)
 *   population_composite [nout][nb][N]                 P(I) = rho_II or |psi_I|^2 */
int qd_get_observables(qd_handle* h, int stride, double* expected, double* population, double* expected_composite,
                       double* population_composite);

int qd_set_target(qd_handle* h, const qd_target* tgt, int nb);
int qd_set_penalty(qd_handle* h, const qd_penalty* pen);

int qd_forward(qd_handle* h, const double* x0, int nb, int store_trajectory, qd_forward_out* out);
/* xbarT: [nb][2*dim] terminal adjoint seed; jbar: [nb][3] = beta_i*{gamma_penalty,
 * gamma_dpdm, gamma_energy} as passed to solveAdjointODE (timestepper.cpp:184);
 * grad: [ndesign] summed over the local batch (overwritten). */
int qd_adjoint(qd_handle* h, const double* xbarT, const double* jbar, int nb, double* grad);

/* Mean number of RHS applications per time step and initial condition in the
 * last forward sweep (1 + linear-solver iterations). */
double qd_last_mean_applies(const qd_handle* h);
/* Milliseconds spent in device kernels of the last forward / adjoint sweep
 * (hipEvent bracket on the handle's stream). */
double qd_last_forward_ms(const qd_handle* h);
double qd_last_adjoint_ms(const qd_handle* h);
/* Workgroups per initial condition in the last sweep: 1, or the team size when a large state (dim > 4096) with few
 * initial conditions was spread over several CUs. */
int qd_last_team(const qd_handle* h);
/* Which iteration solved the linear systems of the last sweep: QD_SOLVER_NEUMANN (requested), QD_SOLVER_KRYLOV (the in-kernel GMRES,
 * KSPGMRES iteration for iteration, src/timestepper.cpp:541-550), QD_SOLVER_GMRES_AS_SPLIT / QD_SOLVER_GMRES_AS_NEUMANN (a gmres
 * request served by a stationary iteration under GMRES's stopping rule: option gmres_split), QD_SOLVER_NONE (explicit Euler). */
#define QD_SOLVER_NONE 0
#define QD_SOLVER_NEUMANN 1
#define QD_SOLVER_KRYLOV 2
#define QD_SOLVER_GMRES_AS_SPLIT 3
#define QD_SOLVER_GMRES_AS_NEUMANN 4
int qd_last_solver(const qd_handle* h);
/* Test hook: the kernel instantiation last launched on this handle for `which` = 0 (forward sweep), 1 (adjoint sweep) or 2 (operator
 * application, qd_apply_rhs), spelled as `nm -C` prints it without namespace and arguments, e.g. "k_forward_col<3, 8, true, false, false,
 * false>" (a system with dipole-dipole coupling on the lean column kernels: "k_forward_colj<2, 5, true, true, false, false>"); "" before
 * the first such launch.  The string belongs to the handle and stays valid until its next launch of that role. */
const char* qd_last_kernel(const qd_handle* h, int which);
/* Measurement hook for the secondary (fp64 vector) roofline: runs a register-only
 * v_fma_f64 micro-benchmark on the device and returns the sustained TFLOP/s in
 * *tflops (the fp64 peak is to be measured, not quoted). */
int qd_measure_fp64_peak(int device_ordinal, double* tflops);
/* the same with v_pk_fma_f32 (fp32-mixed sweeps: the packed form is what the 157.3 TFLOP/s fp32 vector peak is quoted for) */
int qd_measure_fp32_peak(int device_ordinal, double* tflops);

/* ---------------------------------------------------------------------------
 * Objective level: OptimProblem::evalF / evalGradF over the local shard of
 * initial conditions (src/optimproblem.cpp:224-538).
 * ------------------------------------------------------------------------- */
typedef struct qd_objective {
  int32_t initcond_type;               /* QD_INIT_*                          */
  int32_t n_init_ids;                  /* entries after the keyword          */
  int32_t init_ids[QD_MAX_OSC];        /* oscillator ids (or levels for PURE) */
  const double* init_data;             /* FROMFILE: file content, 2*dim_ess(^2) */
  int32_t target_type;                 /* QD_TARGET_*                        */
  int32_t target_pure_levels[QD_MAX_OSC]; /* PURE: level per oscillator      */
  const double* gate_re;               /* GATE: V (dim_ess x dim_ess, row-major), lab frame */
  const double* gate_im;
  double gate_rot_freq[QD_MAX_OSC];    /* GHz                                */
  const double* target_data;           /* FROMFILE: file content             */
  int32_t objective_type;              /* QD_OBJ_*                           */
  int32_t nweights;                    /* optim_weights entries              */
  const double* weights;
  double gamma_tik;                    /* optim_regul                        */
  int32_t tik0;                        /* optim_regul_tik0                   */
  const double* alpha0;                /* [ndesign] initial guess for tik0   */
  qd_penalty penalty;
  double gamma_penalty_variation;      /* optim_penalty_variation            */
} qd_objective;

/* The seven partial sums the reference all-reduces over comm_init
 * (src/optimproblem.cpp:292-298, :454-460), in this order. */
enum { QD_SUM_PENALTY = 0, QD_SUM_DPDM = 1, QD_SUM_ENERGY = 2, QD_SUM_COST_RE = 3,
       QD_SUM_COST_IM = 4, QD_SUM_FID_RE = 5, QD_SUM_FID_IM = 6, QD_NSUMS = 7 };

typedef struct qd_objective_value {
  double objective;                    /* getObjective                       */
  double cost;                         /* getCostT                           */
  double regul;                        /* getRegul                           */
  double penalty;                      /* getPenalty                         */
  double penalty_dpdm;                 /* getPenaltyDpDm                     */
  double penalty_energy;               /* getPenaltyEnergy                   */
  double penalty_variation;            /* getPenaltyVariation                */
  double fidelity;                     /* getFidelity                        */
} qd_objective_value;

typedef struct qd_optim qd_optim;

/* ninit_global initial conditions are sharded contiguously over nranks
 * (iinit_global = rank*ninit_local + iinit, src/optimproblem.cpp:248). */
int qd_optim_create(qd_handle* h, const qd_objective* obj, int rank, int nranks, qd_optim** out);
void qd_optim_destroy(qd_optim* o);
int qd_optim_ninit(const qd_optim* o);        /* global                        */
int qd_optim_ninit_local(const qd_optim* o);
/* initial state / id of local initial condition i: x0 is [2*dim] */
int qd_optim_initial_state(qd_optim* o, int iinit_local, double* x0, int* initid);
int qd_optim_target_state(qd_optim* o, int iinit_local, double* xtarget);

/* Forward sweep of the local shard; partial[QD_NSUMS] are this rank's sums. */
int qd_optim_forward_local(qd_optim* o, const double* alpha, int store_trajectory, double* partial);
/* Objective from the globally reduced sums. */
int qd_optim_finalize(qd_optim* o, const double* alpha, const double* global_sums, qd_objective_value* val);
/* Adjoint sweep of the local shard seeded from the GLOBAL sums
 * (src/optimproblem.cpp:495-519); grad_local[ndesign] still has to be summed
 * over ranks (:527).  Rank 0 adds the Tikhonov / variation terms (:356-372). */
int qd_optim_adjoint_local(qd_optim* o, const double* alpha, const double* global_sums, double* grad_local);

/* Both sweeps of the local shard in ONE call, no collective, for a host that reduces by itself (the reference's two MPI_Allreduce,
 * src/optimproblem.cpp:454-460 and :527): partial[QD_NSUMS] and grad_local[ndesign] are this rank's sums, WITHOUT the regularisation
 * terms (:356-372; the caller adds them once after its reduction, then qd_optim_finalize on the reduced sums).  A shard whose stored
 * stages exceed HBM is propagated and reversed in chunks in one pass - the two-call form above has to propagate it twice.  Available
 * wherever the adjoint seeds do not depend on the reduced cost (src/optimtarget.cpp:889-895): QD_ERR_STATE for Schroedinger + Jtrace. */
int qd_optim_gradient_local(qd_optim* o, const double* alpha, double* partial, double* grad_local);

/* Single-rank convenience wrappers (nranks must be 1). */
int qd_optim_evalF(qd_optim* o, const double* alpha, qd_objective_value* val);
int qd_optim_evalGradF(qd_optim* o, const double* alpha, qd_objective_value* val, double* grad);
/* Chunks of the last gradient evaluation: 1 when the shard's stored trajectory fitted in HBM; otherwise the shard was propagated and
 * reversed in this many batches of initial conditions (the storage problem of src/timestepper.cpp:38-48 at 288 GB) - in one pass
 * (forward + adjoint per chunk) wherever the adjoint seeds do not depend on the reduced cost, i.e. everywhere but Schroedinger + Jtrace. */
int qd_optim_last_chunks(const qd_optim* o);
/* 1 where the last forward sweep of the local shard (forward_local, evalF, evalF_dist) propagated its initial conditions as Hermitian
 * pairs rho_2p + i rho_2p+1 (option pair_hermitian), else 0.  qd_last_mean_applies then counts per propagated pair and time step. */
int qd_optim_last_paired(const qd_optim* o);
/* Per local initial condition, from the last forward sweep of the whole local shard: the in-loop penalty integral, penalty [nlocal], and
 * (J_re, J_im, fidelity_re, fidelity_im), out4 [nlocal][4] - what the seven partial sums weigh and add.  Either pointer may be null.
 * QD_ERR_STATE where no such sweep is at hand. */
int qd_optim_last_local_results(const qd_optim* o, double* penalty, double* out4);

/* OptimProblem::evalF / evalGradF (src/optimproblem.cpp:224-538) at nset control vectors at once: the trial steps of a line search,
 * the starts of a multi-start optimisation, finite-difference probes, amplitude scans.  alphas [nset][ndesign]; vals [nset];
 * grads [nset][ndesign].  Set j's results are those of the single evaluation at alphas[j].  Single rank only (QD_ERR_STATE for an
 * objective created with nranks > 1); nset < 1 or a null pointer: QD_ERR_INVALID; whatever a single evaluation rejects is rejected
 * the same way (gradient of pi-pulses or of the spline_amplitude parameterisation: QD_ERR_UNSUPPORTED).
 * Concurrent path: where a sweep runs on the general kernel family with one workgroup per state (the small Schroedinger and Lindblad
 * systems that leave most of the device idle), fp64 and a shard that needs no chunking, all sets
 * share ONE launch per sweep - nset x ninit states, each set reading a control table of its own; one plan is made for all sets, from
 * the row bound maximised over them.  User Hamiltonians (qd_set_hamiltonian) on the LDS kernels - N <= 32 Lindblad, dim <= 1024
 * Schroedinger - are served the same way by default: every set of a launch also reads a table of G(t) = -i H(t) of its own.
 * Sets whose stored trajectories - and, for a user Hamiltonian, G(t) tables - together exceed what one evaluation may allocate (option
 * traj_budget_mb) are swept in equal groups of the largest size that fits; the G(t) tables of one group stay within the 16 GB
 * qd_set_hamiltonian allows one table, in forward-only calls too.
 * Option batch_lean (qd_set_option; 0 = default, 1 = on): the concurrent path also serves the lean slot family (2^4 / 2^5 all-qubit
 * Lindblad systems, fp64), the fp32-mixed sweeps and the lean column family (Lindblad systems of two or three oscillators with 33..64
 * rows, with or without dipole-dipole coupling: the 3 x 20 class), wherever the kernel's linear solver is a stationary iteration - a
 * neumann request, or a gmres request served by the stand-in; their Krylov kernels (gmres_split = 0) keep going set by set.  A lean
 * column batch is time-sliced by the states of the whole launch (option col_slices), so it may be sliced where the single evaluation is
 * not: the same arithmetic per step, the penalty sums added slice by slice.  The uncoupled 2^5 system
 * picks one or two elements per thread from the states of the whole launch, nset x ninit, so a batch may run another instantiation
 * than the single evaluation of the same shard (option lean64_sb pins it for both).  Off by default (profiles/param_batch_probe.txt has what it buys).
 * Fallback: every other configuration - global-memory kernels (user Hamiltonians beyond dim 1024 among them), lean slot, fp32-mixed
 * and lean column kernels without batch_lean, teams of workgroups, chunked shards - is served set by set through the single
 * evaluation: the same results, no speed-up.
 * After either call the handle holds no stored trajectory (the state and observable getters and the operator-level adjoint sweep return
 * QD_ERR_STATE) and its control table is stale: the next single evaluation returns what it returned before.  qd_last_mean_applies is
 * the mean over all sets, qd_last_kernel names the sweep kernels that ran. */
int qd_optim_evalF_batch(qd_optim* o, const double* alphas, int nset, qd_objective_value* vals);
int qd_optim_evalGradF_batch(qd_optim* o, const double* alphas, int nset, qd_objective_value* vals, double* grads);
/* Sets that shared one sweep launch in the last batch call: nset (or the group size) on the concurrent path, 1 where the call was
 * served set by set. */
int qd_optim_last_batch_sets(const qd_optim* o);

/* Risk-neutral (robust) objective: ONE control vector on an ensemble of nvar systems that differ in Hsys - sampled transition
 * frequencies or couplings of a device whose parameters are not known exactly - and the weighted mean of their objectives and
 * gradients.  hsys_re / hsys_im [nvar][N*N] row-major, rad/ns.  Variant j is the handle's system with Hsys replaced by hsys[j]; the
 * control Hamiltonians, dissipators, target, penalties and initial conditions are the handle's and the objective's.  vals [nvar] (may
 * be NULL) and grads [nvar][ndesign] (may be NULL: then only ndesign doubles leave the device) are what qd_optim_evalGradF(alpha)
 * returns on a handle whose qd_set_hamiltonian received hsys[j].  weights [nvar] are the caller's quadrature weights, used as given
 * (not normalised); NULL = 1/nvar each.  Every field of *mean is sum_j w_j vals[j].field; grad_mean [ndesign] = sum_j w_j grads[j],
 * one fma per variant in variant order (k_ensemble_mean; the regularisation terms are added to every variant's gradient before the
 * weighting).
 * The handle must be a user-Hamiltonian handle (qd_set_hamiltonian supplies the Hc_k): otherwise QD_ERR_STATE.  nvar < 1, a null alpha,
 * hsys_re, hsys_im, mean or grad_mean, a negative or non-finite weight: QD_ERR_INVALID.  An objective created with nranks > 1:
 * QD_ERR_STATE.  Whatever a single evaluation rejects is rejected the same way.
 * The variants are the sets of a parameter-set batch (qd_optim_evalF_batch) whose control vectors are all alpha: on the LDS kernels
 * (dim <= 1024) they share one launch per sweep, each reading a table of G(t) built from its own Hsys; groups, the one plan for all
 * sets (the row bound of the variant with the largest row sum) and the fallback - variant by variant through the single evaluation,
 * the same results - are those of the batch, and qd_optim_last_batch_sets reports the variants per launch.  After the call the state
 * is that of a batch call; the handle's own Hsys is untouched and the next single evaluation returns what it returned before. */
int qd_optim_evalF_ensemble(qd_optim* o, const double* alpha, int nvar, const double* hsys_re, const double* hsys_im,
                            const double* weights, qd_objective_value* vals, qd_objective_value* mean);
int qd_optim_evalGradF_ensemble(qd_optim* o, const double* alpha, int nvar, const double* hsys_re, const double* hsys_im,
                                const double* weights, qd_objective_value* vals, qd_objective_value* mean, double* grads,
                                double* grad_mean);

/* The same for the STANDARD Hamiltonian model (a handle without qd_set_hamiltonian): ONE control vector on nvar variants of the model's
 * constants - transition frequencies and self-Kerr coefficients [nvar][nosc], cross-Kerr coefficients and dipole-dipole couplings
 * [nvar][npairs], GHz, in the pair order of qd_system.  Any of the four arrays may be NULL: the handle's own values for every variant.
 * Variant j is the system of a handle created from the same qd_system with those arrays replaced (converted to rad/ns by the function
 * qd_create uses); rotation frequencies - and with them the frame and the control table -, level counts, T1/T2, controls, target,
 * penalties and initial conditions stay the handle's and the objective's.  vals, grads, mean, grad_mean, weights and
 * qd_optim_last_batch_sets mean exactly what they mean for qd_optim_evalF_ensemble / qd_optim_evalGradF_ensemble (NULL weights = 1/nvar,
 * vals and grads may be NULL, grad_mean by k_ensemble_mean).
 * Errors: a user-Hamiltonian handle: QD_ERR_STATE (that handle uses the call above); an objective created with nranks > 1: QD_ERR_STATE;
 * nvar < 1, a null alpha, mean or grad_mean, a non-finite constant, a negative or non-finite weight: QD_ERR_INVALID; a variant with
 * |Jkl| > 1e-10 on a handle whose system has no coupling: QD_ERR_UNSUPPORTED (create the handle with a coupling; on a coupled handle a
 * variant whose couplings are all zero is fine and stays on the coupled kernels, with zero weights).
 * Shared launches: wherever the plan's sweep is a diagonal-split stationary iteration of the lean column family (Lindblad systems of two
 * or three oscillators with 33..64 rows, the 3 x 20 class; a neumann request, or a gmres request served by the stand-in) all variants
 * share one launch per sweep - k_forward_col_vars / k_adjoint_col_vars (coupled: k_*_colj_vars), each task reading its variant's
 * constants from a device table; one plan for all variants from the largest row bounds among them; groups as in the batch.  Option
 * batch_lean is not consulted; option ensemble_loop = 1 serves the call variant by variant instead (A/B switch).
 * Option ensemble_general (qd_set_option; 0 = default, 1 = on): the variants share launches on the general kernel family as well (one
 * workgroup per state in LDS, fp64: two to five coupled qubits or qutrits, Schroedinger or Lindblad, and the 3 x 20 class under
 * no_collean) - k_forward_vars / k_adjoint_vars, the workgroup of a state reading its variant's constants through scalar loads; a
 * neumann request, a gmres request on the Krylov kernels (basis in LDS or in global memory) and one served by the Neumann stand-in
 * alike.  With the default 0 that family goes variant by variant.
 * Option ensemble_lean (qd_set_option; 0 = default, 1 = on): the variants share launches on the lean slot and fp32-mixed families as
 * well (all-qubit Lindblad systems: 2^4 and 2^5 in fp64, 2x2x2, 2^4 and 2^5 in QD_PRECISION_F32MIXED, with or without dipole-dipole
 * coupling) where the sweep's solver is a stationary iteration - a neumann request, or a gmres request served by the Neumann stand-in -
 * on k_forward_q32_vars / k_adjoint_q32_vars, the workgroup of a state reading its variant's constants through scalar loads.  A Krylov
 * plan (gmres_split = 0) goes variant by variant.  The uncoupled 2^5 system picks its elements per thread from all states of the launch
 * (variants x initial conditions), as the parameter-set batch does: option lean64_sb pins it.  With the default 0 those families go
 * variant by variant.  Every other
 * configuration - general, slot and fp32-mixed (without their options), Krylov plans of the latter two, global-memory families, plain-Neumann or Krylov column plans, chunked shards - goes
 * variant by variant through the single evaluation with the handle pointed at one variant after the other: the numbers of a fresh
 * handle, qd_optim_last_batch_sets = 1.
 * After the call the state is that of a batch call; the handle's own constants, its solver latch and every table derived from them are
 * what they were, and the next single evaluation returns what it returned before. */
int qd_optim_evalF_ensemble_model(qd_optim* o, const double* alpha, int nvar, const double* transfreq, const double* selfkerr,
                                  const double* crosskerr, const double* Jkl, const double* weights, qd_objective_value* vals,
                                  qd_objective_value* mean);
int qd_optim_evalGradF_ensemble_model(qd_optim* o, const double* alpha, int nvar, const double* transfreq, const double* selfkerr,
                                      const double* crosskerr, const double* Jkl, const double* weights, qd_objective_value* vals,
                                      qd_objective_value* mean, double* grads, double* grad_mean);

/* Objective, gradient and the derivatives of the objective with respect to the constants of the STANDARD Hamiltonian model, from ONE
 * forward and ONE adjoint sweep.  val and grad are those of qd_optim_evalGradF(alpha).  d_transfreq [nosc], d_selfkerr [nosc] and
 * d_crosskerr [npairs, in the pair order of qd_system] receive d objective / d constant per GHz of the qd_system field; any of the
 * three may be NULL.  The function differentiated is the one qd_optim_evalF_ensemble_model samples: a constant is moved as on a handle
 * created from the same qd_system with that one entry changed, while rotation frequencies (the frame and the control table), level
 * counts, T1/T2, Jkl, controls, target and penalties are held fixed; the Tikhonov and control-variation terms do not depend on the
 * constants.  The derivative is the discrete one of the implicit-midpoint family, exact to the tolerance of the linear solver like the
 * control gradient: with the h-scaled adjoint stage kbar_s and the stored primal stage z_s of sub-step s,
 *   d objective / d theta = sum over the initial conditions and sub-steps of kbar_s^T (dM / d theta) z_s,
 * where dM / d theta is diagonal and time-independent: for the element with bra digits i_k and ket digits i'_k (Schroedinger: no ket
 * digits) w = kbar.x z.y - kbar.y z.x times 2 pi (i_k - i'_k) for transfreq[k], - pi (i_k (i_k - 1) - i'_k (i'_k - 1)) for selfkerr[k]
 * and - 2 pi (i_k i_l - i'_k i'_l) for crosskerr[kl].  kbar is never stored, so the sums are formed inside the adjoint kernel: the call
 * plans BOTH sweeps on the general kernel family (one workgroup per state in LDS, as options no_collean / no_lean64 would - systems that
 * otherwise run on a lean family included), the forward sweep on k_forward, the adjoint sweep on its sensitivity form k_adjoint_sens
 * (qd_last_kernel).  The handle's options, solver latch and tuner state are restored afterwards: the next qd_optim_evalGradF returns
 * what it returned before, on the kernels it ran on before.
 * Option sens_lean = 1 (qd_set_option; 0 = default, under which nothing changes): where the handle's own plan puts the adjoint sweep on
 * the diagonal-split stationary iteration of the lean column kernels (3x20-class Lindblad systems, with or without Jkl; a gmres request
 * served by that iteration included), the call stays there - the forward sweep on k_forward_col / k_forward_colj as planned, the adjoint
 * sweep on its sensitivity form k_adjoint_col_sens / k_adjoint_colj_sens, which sums w per element over the sub-steps and weights the
 * sums once per task.  val and grad are then bit for bit those of qd_optim_evalGradF on that handle.  Any other plan - the lean column
 * Krylov kernels (gmres_split = 0), the plain Neumann form (neumann_split = 0), the lean slot systems - takes the general family as above.
 * Option sens_slot = 1 (0 = default, under which nothing changes; deliberately a key of its own, sens_lean names the column family
 * alone): where the handle's own plan puts both sweeps on the fp64 lean slot kernels (2^4 / 2^5 all-qubit Lindblad systems, with or
 * without Jkl) and the adjoint sweep on their stationary iteration (a neumann request, or a gmres request served by the stand-in), the
 * call stays there - the forward sweep on k_forward_q32 as planned, the adjoint sweep on k_adjoint_q32_sens of the same instantiation,
 * which sums w per element over the sub-steps and weights the sums once per state.  val and grad are then bit for bit those of
 * qd_optim_evalGradF on that handle.  A Krylov plan of that family (gmres_split = 0) takes the general family as above.
 * Errors: a null o, alpha, val or grad: QD_ERR_INVALID; a user-Hamiltonian handle or an objective created with nranks > 1:
 * QD_ERR_STATE; explicit Euler, QD_PRECISION_F32MIXED, a state beyond one CU's LDS (the global-memory kernels, dim > 4096), a shard
 * whose stored trajectory would need chunking, and whatever qd_optim_evalGradF rejects: QD_ERR_UNSUPPORTED, the message naming the
 * reason; no sweep is launched for any of them.
 * Not built: d / d Jkl (off-diagonal), d / d T1, T2, a sensitivity form of the Krylov kernels of either lean family, of the
 * plain-Neumann lean column kernels and of the fp32-mixed kernels, sensitivities of an ensemble mean, several ranks. */
int qd_optim_evalGradF_model(qd_optim* o, const double* alpha, qd_objective_value* val, double* grad, double* d_transfreq,
                             double* d_selfkerr, double* d_crosskerr);

/* Sampled controls: OptimProblem::evalF / evalGradF (src/optimproblem.cpp:224-538) with p_k(t), q_k(t) given as samples in place of the
 * spline parameters alpha - pulses from an AWG sample file, the piecewise-constant amplitudes of a GRAPE-style optimiser, the output of
 * a filter chain or a pulse-generating model - and the gradient per sample.  Every sweep kernel reads its controls from the control
 * table, one row per sub-step of the stepper (IMR: ntime rows, row n at t_n + dt / 2; IMR4 / IMR8: stages x ntime rows at the stage
 * midpoints, which are not uniform); qd_sampled_nrows is the number of rows of this handle's table (QD_ERR_UNSUPPORTED for explicit
 * Euler), qd_sampled_times copies the time t [nrows] and the signed length hstep [nrows, may be NULL] of every row, in ns.
 * samples [nsamp][nosc][2] = (p, q) in rad/ns in the rotating frame: the layout and the unit of qd_eval_controls.  A table row at time t
 * in (0, T), T = ntime dt, reads its (p_k, q_k) by mode:
 *   QD_SAMPLED_ROWS    nsamp == nrows; row s reads sample s.
 *   QD_SAMPLED_HOLD    nsamp >= 1 equal slots (the zero-order hold of an AWG); the row reads slot min(nsamp - 1, floor(t nsamp / T)).
 *   QD_SAMPLED_LINEAR  nsamp >= 2 knots tau_j = j T / (nsamp - 1); the row reads the linear interpolant between the two neighbouring knots.
 * The table is filled on the device (k_table_sampled) and the sweeps, the plan and the kernel families are those of the single evaluation
 * - standard model and user Hamiltonians (qd_set_hamiltonian) alike, chunked shards included; the solver gates decide from the amplitude
 * bound max_j max(|p_jk|, |q_jk|) of the samples, which bounds every row under all three modes (a handle that never saw qd_set_params
 * is fine).  *val is what qd_optim_evalF returns for a control function with those table rows, except that the Tikhonov term `regul` and
 * `penalty_variation` are defined on alpha: both are 0 here and carry no gradient.  The forward sweep of qd_optim_evalF_sampled is the
 * one of qd_optim_evalF: it may propagate Hermitian pairs where option pair_hermitian admits them (nothing in the pairing reads alpha).
 * grad_samples [nsamp][nosc][2] = d objective / d sample: the discrete gradient, exact to the tolerance of the linear solver like the
 * control gradient.  The adjoint sweep leaves d objective / d p_k(t_s), d q_k(t_s) per table row; ROWS returns those sums themselves,
 * HOLD and LINEAR the transpose of the interpolation applied to them (k_grad_sampled: one wave per entry, lanes over the rows in the
 * support of the sample, reduced in a fixed order - two calls return the same bits; a sample with no row in its support gets exactly 0).
 * Errors, none of which launches a sweep: a null o, samples, val or grad_samples, an unknown mode, nsamp out of range for the mode
 * (ROWS: nsamp != nrows), a non-finite sample: QD_ERR_INVALID; an objective created with nranks > 1: QD_ERR_STATE; explicit Euler (its
 * table has a row more, at other times), a handle with pi-pulses (they would overwrite the samples), gamma_penalty_energy > 1e-13 (that
 * penalty reads the controls on a time grid of its own, which the samples do not define), QD_PRECISION_F32MIXED (not built for this
 * call): QD_ERR_UNSUPPORTED, the message naming the reason.
 * After either call the handle holds no stored trajectory and its control table is stale, as after a batch call; the solver latch,
 * the tuner of the polynomial degree and the handle's own parameters are what they were: the next qd_optim_evalGradF(alpha) returns what
 * it returned before, on the kernels it ran on before.
 * Not built: explicit Euler, the energy penalty, pi-pulses, several ranks, sampled controls in the batch / ensemble / sensitivity calls,
 * device-pointer variants, a config key of the driver. */
enum { QD_SAMPLED_ROWS = 0, QD_SAMPLED_HOLD = 1, QD_SAMPLED_LINEAR = 2 };
int qd_sampled_nrows(const qd_handle* h);
int qd_sampled_times(const qd_handle* h, double* t, double* hstep);
int qd_optim_evalF_sampled(qd_optim* o, int mode, int nsamp, const double* samples, qd_objective_value* val);
int qd_optim_evalGradF_sampled(qd_optim* o, int mode, int nsamp, const double* samples, qd_objective_value* val, double* grad_samples);

/* ---------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, initial conditions sharded over the ranks.
 * Replaces the reference's comm_init communicator (src/main.cpp:133-177) and its
 * MPI_Allreduce calls (src/optimproblem.cpp:292-298, :454-460, :527) by RCCL
 * (ncclAllReduce over xGMI) on the handle's HIP stream; partial sums and the
 * gradient never leave HBM between the sweeps and the collectives.
 * ------------------------------------------------------------------------- */
#define QD_COMM_ID_BYTES 128           /* = NCCL_UNIQUE_ID_BYTES                */
typedef struct qd_comm qd_comm;
/* rank 0: generate the id (ncclGetUniqueId) and hand its bytes to every rank by any means */
int qd_comm_unique_id(unsigned char id[QD_COMM_ID_BYTES]);
int qd_comm_create(const unsigned char id[QD_COMM_ID_BYTES], int rank, int nranks, int device_ordinal, qd_comm** out);
/* MPI-free bootstrap through a path every rank can see.  RCCL backend: rank 0 writes the id file, every other rank echoes the token it read
 * together with a nonce of its own (path.ack<rank>) and rank 0 answers each echo with path.go<rank> carrying that nonce; a rank enters
 * ncclCommInitRank only on a go file that returns its own nonce - leftover files of a crashed run are never acted upon;
 * QD_JOB_ID (when the launcher sets one) additionally separates jobs.  Host backend (below): the path only names the shared-memory segment.
 * Backend: environment QD_COMM_BACKEND = rccl | host | auto (default auto: host when the ranks OF THIS NODE - QD_LOCAL_SIZE, set by the
 * launchers; nranks without it - exceed the visible GPUs, i.e. when ranks share a device, which RCCL refuses; refused when such a launch
 * spans nodes). */
int qd_comm_create_from_file(const char* path, int rank, int nranks, int device_ordinal, double timeout_s, qd_comm** out);
/* HOST backend: the ranks of ONE node reduce through a POSIX shared-memory segment named after `name` (the same string on every rank of a
 * job, different for concurrent jobs).  Same call sites and buffers as the RCCL backend (qd_optim_evalF_dist / evalGradF_dist,
 * qd_comm_allreduce), summation in rank order on every rank (bit-identical results on all ranks); the reduction buffer makes one round
 * trip HBM -> pinned host -> HBM per collective.  For ranks that share a GPU (mpirun -np 4 on a one-GPU box) and nodes without RCCL.
 * Replaces the same MPI_Allreduce calls (src/optimproblem.cpp:292-298, :454-460, :527).  At most 64 ranks. */
int qd_comm_create_host(const char* name, int rank, int nranks, int device_ordinal, double timeout_s, qd_comm** out);
/* 0 = RCCL, 1 = host shared memory */
int qd_comm_backend(const qd_comm* c);
void qd_comm_destroy(qd_comm* c);
int qd_comm_size(const qd_comm* c);
int qd_comm_rank(const qd_comm* c);
/* host convenience: in-place all-reduce of n doubles, op 0 = sum, 1 = max (staged through HBM, blocking) */
int qd_comm_allreduce(qd_comm* c, double* buf, int n, int op);
int qd_comm_barrier(qd_comm* c);
/* evalF / evalGradF over ALL ranks (every rank calls with its own shard `o` created with the same rank / nranks as
 * `c`); every rank receives the same value and the complete gradient.  allreduce_ms (NULL or [2]): device time of the
 * objective-sum and the gradient collective. */
int qd_optim_evalF_dist(qd_optim* o, qd_comm* c, const double* alpha, qd_objective_value* val, double* allreduce_ms);
int qd_optim_evalGradF_dist(qd_optim* o, qd_comm* c, const double* alpha, qd_objective_value* val, double* grad, double* allreduce_ms);

/* ---------------------------------------------------------------------------
 * Arithmetic of the sweeps.  QD_PRECISION_F64 (default): everything IEEE double like the reference.
 * QD_PRECISION_F32MIXED (BASELINE config 5): the exchange vector in LDS, the stencil arithmetic, the linear-solver
 * iterates and the stored trajectory are fp32; the state / adjoint-state accumulators, every norm, objective sum and
 * gradient coefficient are fp64.  Built for all-qubit Lindblad systems with 4 or 5 oscillators, both linear solvers
 * (GMRES: Krylov basis as float2, Hessenberg problem in fp64), IMR family; QD_ERR_UNSUPPORTED elsewhere.  Call before
 * the first sweep.
 * ------------------------------------------------------------------------- */
enum { QD_PRECISION_F64 = 0, QD_PRECISION_F32MIXED = 1 };
int qd_set_precision(qd_handle* h, int precision);
/* Tuning and test options of a handle, as "key", "value" strings (the counterpart of PETSc's options database the reference is
 * steered with, e.g. -ksp_* for the linear solver of src/timestepper.cpp:541-550).  Integer values unless noted; "auto" restores
 * the default.  Keys: neumann_split (diagonal of M on the left-hand side of the Neumann iteration: same fixed point and stopping
 * rule, fewer iterations on systems whose level energies dominate; auto = where it pays, 0 = the reference's iteration everywhere),
 * gmres_split (linearsolver_type = gmres served by a stationary iteration under GMRES's stopping rule wherever that iteration provably
 * contracts fast - the reference's Neumann iteration, or the diagonal-split one on 3x20-class systems and on states beyond LDS: auto = there, 0 = always the
 * Krylov kernels), gmres_poly (degree of the polynomial preconditioner, 0 = tuned then frozen, 1 = none), krylov_tau (double: the one-vector
 * path of the lean kernels' Krylov solvers accepts at residual <= krylov_tau x the reference's tolerance, default 0.1), krylov_restart (restart length of those solvers' generic path, 1 .. 14), force_neumann, var (kernel variant), no_mfma,
 * no_lean64, lean64_sb, no_collean, no_col_krylov, col_min_n, big_team, big_spread, big_blocked, traj_budget_mb (double), batch_lean (the parameter-set
 * batch shares launches on the lean slot, fp32-mixed and lean column families too: see qd_optim_evalF_batch; 0 = default), ensemble_general (a model-parameter ensemble shares launches on the general kernel family too: see
 * qd_optim_evalF_ensemble_model; 0 = default), ensemble_lean (... and on the stationary iterations of the lean slot and
 * fp32-mixed families; 0 = default), ensemble_loop (a model-parameter
 * ensemble goes variant by variant even where it could share launches: see qd_optim_evalF_ensemble_model; 0 = default), sens_lean (qd_optim_evalGradF_model
 * stays on the lean column kernels where their sensitivity form is built: see there; 0 = default), sens_slot (... and on the fp64 lean
 * slot kernels; 0 = default), pair_hermitian (forward sweeps that store nothing - qd_optim_evalF, qd_optim_evalF_dist,
 * qd_optim_forward_local without storage - propagate exactly Hermitian Lindblad initial conditions two at a time as rho_a + i rho_b
 * where the plan is the lean column family's stationary solver serving a neumann request under the absolute rule and the in-loop
 * penalty, if any, reads the diagonal only (weighted Jmeasure, leakage): auto = shards of more states than the device has compute
 * units, 1 = wherever those conditions hold, 0 = never; see qd_optim_last_paired).  Every key is also read from the
 * environment variable QD_<KEY> once, at qd_create (tests, measurements).  Unknown keys: QD_ERR_INVALID. */
int qd_set_option(qd_handle* h, const char* key, const char* value);
int qd_get_precision(const qd_handle* h);
/* Measurement hook: nrep chained forward applications y <- M(t) (1e-3 y) on nb states, starting from x, in fp32 by the
 * stencil kernel (mfma = 0) or as the dense Kronecker-factor product G rho - rho G on the fp32 matrix cores (mfma = 1,
 * five qubits only); *ms = device time of the launch.  profiles/HISTORY.md (section 4) records the comparison. */
int qd_bench_apply_f32(qd_handle* h, double t, const double* x, double* y, int nb, int nrep, int mfma, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* QUANDARY_AMD_H */

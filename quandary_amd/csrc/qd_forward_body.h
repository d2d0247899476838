// qd_forward_body.h - the body of the forward sweep kernels of qd_device.h, included inside k_forward and k_forward_vars: the text of a
// kernel stands in the kernel itself (a device function that takes the kernel argument by reference changes where the compiler reads
// the arguments, and with it the register allocation of every existing instantiation).  In scope where it is included: the template
// arguments Q, LIND, VAR, QUBIT, GM, PLAIN, the constants SETS and VARS, the kernel argument `const SweepArgs A`.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef Team<Q, LIND, VAR, QUBIT, GM, VARS> TM;
  constexpr int EPT = TM::EPT;
  const DevSys& S = A.S;
  TM tm;
  if constexpr (VARS) tm.st.mc.bind(A, (int)blockIdx.x);
  tm.init(S, smem, A.use_gmres);
  const int dim = S.dim;
  double2 x[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const double* x0 = A.x0 + (size_t)tm.ic0 * 2 * dim;
    x[j] = make_double2(x0[tm.st.it[j]], x0[dim + tm.st.it[j]]);
  }
  team_sync<TM::V::ONEWAVE>();  // coefficient tables written by init()
  tm.publish(x);
  // penalty bookkeeping
  const bool ee = PLAIN ? false : A.stepper_ee != 0;
  const bool pen_on = PLAIN ? false : A.gamma_penalty > 1e-13;
  const bool wj_on = pen_on && A.penalty_param > 1e-13;
  // Schroedinger Jtrace is the only objective whose finalizeJ is nonlinear in the per-state sums:
  // it needs a block reduction per step; everything else accumulates thread-locally.
  const bool wj_reduce = wj_on && !LIND && A.tg.objective_type == QD_OBJ_JTRACE;
  const bool dpdm_on = PLAIN ? false : (A.gamma_dpdm > 1e-13 && !LIND);
  const bool jpairs = S.npairs > 0;
  bool guard[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) guard[j] = A.leak_on && tm.ok(j) && tm.st.is_guard(S, j);
  double pen_local = 0.0, dpdm_local = 0.0, pen_uniform = 0.0;
  double2 xm1[EPT], xm2[EPT];  // dpdm history (x_n, x_{n-1})
#pragma unroll
  for (int j = 0; j < EPT; j++) xm1[j] = xm2[j] = x[j];
  unsigned long long napply = 0;
  double* traj = A.traj;
  const double dtinv4 = 1.0 / (A.dt * A.dt * A.dt * A.dt);
  // latency-bound variants prefetch the next table row; the throughput variants (several waves per
  // SIMD) load the row where it is used and keep it in scalar registers
  constexpr bool PREFETCH = !TM::V::LEAN;
  constexpr bool XSTASH = TM::V::LEAN;  // explicit staging of the state through L2/HBM instead of compiler spills
  StepC<Q> c, cn;
  if (PREFETCH) load_step<Q>(sweep_ctl<SETS>(A, tm.ic0), cn, jpairs);

  vm_drain();
  for (int s = 0; s < A.nsub; s++) {
    if (PREFETCH) {
      c = cn;
      if (s + 1 < A.nsub) load_step<Q>(sweep_ctl<SETS>(A, tm.ic0) + (size_t)(s + 1) * A.cs, cn, jpairs);  // prefetch the next row
    } else {
      load_step<Q>(sweep_ctl<SETS>(A, tm.ic0) + (size_t)s * A.cs, c, jpairs);
      scalarize<Q>(c, jpairs);
    }
    c.g = S.dense ? reinterpret_cast<const double2*>(sweep_gtab<SETS>(A, S, tm.ic0)) + (size_t)s * S.N * S.N : nullptr;
    tm.st.prep(S, tm.L, c);
    if (traj) {
#pragma unroll
      for (int j = 0; j < EPT; j++)
        if (tm.ok(j)) {
          double* dst = traj + ((size_t)s * A.nb + tm.ic0) * 2 * dim;  // written once, read by the adjoint sweep much later:
          __builtin_nontemporal_store(x[j].x, dst + tm.st.it[j]);        // streaming stores, the caches keep the solver's vectors
          __builtin_nontemporal_store(x[j].y, dst + dim + tm.st.it[j]);
        }
    }
    // rhs = M x   (ImplMidpoint::evolveFWD, timestepper.cpp:594; ExplEuler :502)
    double2 rhs[EPT];
    tm.template apply_all<false>(S, c, x, rhs);
    napply++;
    if (XSTASH && !ee) {  // x is not needed during the linear solve: park it in the output buffer
#pragma unroll
      for (int j = 0; j < EPT; j++)
        if (tm.ok(j)) {
          double* xs = A.xT + (size_t)tm.ic0 * 2 * dim;
          const int e = at_use<EPT>(tm.st.it[j]);
          xs[e] = x[j].x;
          xs[dim + e] = x[j].y;
        }
    }
    if (ee) {
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        x[j].x = fma(c.h, rhs[j].x, x[j].x);
        x[j].y = fma(c.h, rhs[j].y, x[j].y);
      }
    } else {
      double2 k[EPT];
      napply += tm.template solve<false>(A, c, 0.5 * c.h, rhs, k);
      if (XSTASH) {
#pragma unroll
        for (int j = 0; j < EPT; j++) {
          const double* xs = A.xT + (size_t)tm.ic0 * 2 * dim;
          const int e = at_use<EPT>(tm.st.it[j]);
          x[j] = make_double2(xs[e], xs[dim + e]);
        }
      }
      if (A.ztraj) {  // the primal stage z = x + h/2 k: read back by the adjoint sweep instead of repeating this solve
#pragma unroll
        for (int j = 0; j < EPT; j++)
          if (tm.ok(j)) stage_store(A.ztraj, (size_t)s * A.nb + tm.ic0, dim, tm.st.it[j], fma(0.5 * c.h, k[j].x, x[j].x), fma(0.5 * c.h, k[j].y, x[j].y));
      }
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        x[j].x = fma(c.h, k[j].x, x[j].x);
        x[j].y = fma(c.h, k[j].y, x[j].y);
      }
    }
    tm.publish(x);

    // in-loop penalties, evaluated at the end of a FULL time step (timestepper.cpp:141-154)
    if ((pen_on || dpdm_on) && (s + 1) % A.nstages == 0) {
      const int n = (s + 1) / A.nstages - 1;  // step index n: state is x_{n+1}
      const double tstop = (n + 1) * A.dt;
      if (pen_on) {
        double weight = 0.0;
        if (wj_on) {
          if (A.wjw) {  // tabulated per time step (qd_handle::ensure_wj_weights): no exp() next to the state registers
            weight = to_scalar(A.wjw[n]);
          } else {
            const double a = (tstop - A.Tfinal) / A.penalty_param;
            weight = 1.0 / A.penalty_param * exp(-(a * a));
          }
        }
        if (wj_reduce) {
          double v[2] = {0.0, 0.0};
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.ok(j)) evalJ_part<LIND>(S, A.tg, tm.ic0, at_use<EPT>(tm.st.it[j]), x[j], v[0], v[1]);
          tm.template sum<2>(v);
          pen_uniform += weight * finalizeJ<LIND>(A.tg, v[0], v[1]) * A.dt;
        } else if (wj_on) {
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.ok(j)) {
              double jr = 0.0, ji = 0.0;
              evalJ_part<LIND>(S, A.tg, tm.ic0, at_use<EPT>(tm.st.it[j]), x[j], jr, ji);
              // finalizeJ is affine here: J = jr (Jfrobenius, Jmeasure) or 1 - jr (Lindblad Jtrace)
              pen_local += (A.tg.objective_type == QD_OBJ_JTRACE ? -1.0 : 1.0) * weight * A.dt * jr;
            }
          if (A.tg.objective_type == QD_OBJ_JTRACE) pen_uniform += weight * A.dt;
        }
#pragma unroll
        for (int j = 0; j < EPT; j++)
          if (guard[j]) pen_local += (x[j].x * x[j].x + x[j].y * x[j].y) / A.ntime;
      }
      if (dpdm_on) {
        if (n > 0) {
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.ok(j)) {
              const double t1 = x[j].x * x[j].x - 2.0 * xm1[j].x * xm1[j].x + xm2[j].x * xm2[j].x;
              const double t2 = x[j].y * x[j].y - 2.0 * xm1[j].y * xm1[j].y + xm2[j].y * xm2[j].y;
              dpdm_local += dtinv4 * (t1 + t2) * (t1 + t2);
            }
        }
#pragma unroll
        for (int j = 0; j < EPT; j++) {
          xm2[j] = xm1[j];
          xm1[j] = x[j];
        }
      }
    }
  }
  // final state (+ last trajectory slot)
#pragma unroll
  for (int j = 0; j < EPT; j++)
    if (tm.ok(j)) {
      double* xT = A.xT + (size_t)tm.ic0 * 2 * dim;
      xT[tm.st.it[j]] = x[j].x;
      xT[dim + tm.st.it[j]] = x[j].y;
      if (traj) {
        double* dst = traj + ((size_t)A.nsub * A.nb + tm.ic0) * 2 * dim;
        dst[tm.st.it[j]] = x[j].x;
        dst[dim + tm.st.it[j]] = x[j].y;
      }
    }
  double v[2] = {pen_local, dpdm_local};
  tm.template sum<2>(v);
  if (threadIdx.x == 0) {
    A.pen_out[tm.ic0] = v[0] + pen_uniform;
    A.dpdm_out[tm.ic0] = v[1] / A.ntime;
    atomicAdd(A.napply, napply);
  }

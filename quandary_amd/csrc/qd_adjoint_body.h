// qd_adjoint_body.h - the body of the adjoint sweep kernels of qd_device.h, included inside k_adjoint and k_adjoint_vars (see
// qd_forward_body.h) and k_adjoint_sens.  In scope where it is included: the template arguments Q, LIND, VAR, QUBIT, GM, PLAIN, the
// constants SETS, VARS and SENS (the sensitivity form, qd_sens.h: false in k_adjoint and k_adjoint_vars, whose code is that of the body
// without it), the kernel argument `const SweepArgs A`.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef Team<Q, LIND, VAR, QUBIT, GM, VARS> TM;
  constexpr int EPT = TM::EPT;
  const DevSys& S = A.S;
  TM tm;
  if constexpr (VARS) tm.st.mc.bind(A, (int)blockIdx.x);
  tm.init(S, smem, A.use_gmres);
  team_sync<TM::V::ONEWAVE>();
  const int dim = S.dim;
  double2 xb[EPT], xn[EPT];  // adjoint state, primal state x_n (end of the step being reversed)
  const double* traj = A.traj;
  auto load_state = [&](int s, double2(&dst)[EPT]) {
#pragma unroll
    for (int j = 0; j < EPT; j++) {
      const double* src = traj + ((size_t)s * A.nb + tm.ic0) * 2 * dim;
      dst[j] = make_double2(__builtin_nontemporal_load(src + tm.st.it[j]), __builtin_nontemporal_load(src + dim + tm.st.it[j]));
    }
  };
#pragma unroll
  for (int j = 0; j < EPT; j++) {
    const double* xbT = A.xbarT + (size_t)tm.ic0 * 2 * dim;
    xb[j] = make_double2(xbT[tm.st.it[j]], xbT[dim + tm.st.it[j]]);
  }
  const bool jpairs = S.npairs > 0;
  const bool ee = PLAIN ? false : A.stepper_ee != 0;
  if (ee && !LIND) {
    // Schroedinger runs of the reference do not store the forward states: the adjoint loop re-computes the primal
    // backwards with the FORWARD stepper and a negative step, xprimal <- xprimal + (tstart - tstop) M(tstop) xprimal
    // (src/timestepper.cpp:229-231 with ExplEuler::evolveFWD :496-507), and so do the dpdm states (:207-211, :236-243).
    // That is exact for the symmetric IMR family but O(dt) away from the forward states for explicit Euler, and the
    // reference's EE gradient is defined on this backward chain.  Reproduce it: overwrite the stored trajectory with
    // the chain x_N, B_N x_N, B_{N-1} B_N x_N, ... (every thread only touches its own elements), then run the
    // ordinary adjoint loop on it.
    double* trajw = const_cast<double*>(traj);
    double2 xp[EPT];
    load_state(A.nsub, xp);
    for (int s = A.nsub - 1; s >= 0; s--) {
      StepC<Q> c1;
      load_step<Q>(sweep_ctl<SETS>(A, tm.ic0) + (size_t)(s + 1) * A.cs, c1, jpairs);  // M(tstop of step s) = row s + 1
      if (TM::V::LEAN) scalarize<Q>(c1, jpairs);
      c1.g = S.dense ? reinterpret_cast<const double2*>(sweep_gtab<SETS>(A, S, tm.ic0)) + (size_t)(s + 1) * S.N * S.N : nullptr;
      tm.st.prep(S, tm.L, c1);
      const double hneg = -sweep_ctl<SETS>(A, tm.ic0)[(size_t)s * A.cs];
      tm.publish(xp);
      double2 t[EPT];
      tm.template apply_all<false>(S, c1, xp, t);
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        xp[j].x = fma(hneg, t[j].x, xp[j].x);
        xp[j].y = fma(hneg, t[j].y, xp[j].y);
        if (tm.ok(j)) {
          double* dst = trajw + ((size_t)s * A.nb + tm.ic0) * 2 * dim;
          const int e = at_use<EPT>(tm.st.it[j]);
          dst[e] = xp[j].x;
          dst[dim + e] = xp[j].y;
        }
      }
    }
    __threadfence_block();
    team_sync<TM::V::ONEWAVE>();
  }
  // Latency-bound variants (few elements per thread) carry x_{n+1} in registers and prefetch x_{n-1} one
  // step ahead; the throughput variants re-read them (L2 / HBM) to keep the register footprint small.
  constexpr bool CARRY = !TM::V::LEAN && !PLAIN;  // (PLAIN: nothing in the sweep reads the primal states)
  if (CARRY) load_state(A.nsub, xn);
  const int bq = min(tm.ic0, A.nb - 1);
  const double jbar_pen = A.jbar[bq * 3 + 0], jbar_dpdm = A.jbar[bq * 3 + 1];
  const bool pen_on = PLAIN ? false : A.gamma_penalty > 1e-13;
  const bool wj_on = pen_on && A.penalty_param > 1e-13;
  const bool wj_reduce = wj_on && !LIND && A.tg.objective_type == QD_OBJ_JTRACE;
  const bool dpdm_on = PLAIN ? false : (A.gamma_dpdm > 1e-13 && !LIND);
  bool guard[EPT];
#pragma unroll
  for (int j = 0; j < EPT; j++) guard[j] = A.leak_on && tm.ok(j) && tm.st.is_guard(S, j);
  const double dtinv4 = 1.0 / (A.dt * A.dt * A.dt * A.dt);
  const int ntime = A.ntime;
  double2 x[EPT], xnext[CARRY ? EPT : 1];
  if (CARRY) load_state(A.nsub - 1, reinterpret_cast<double2(&)[EPT]>(xnext));  // primal at the start of the last sub-step
  // Latency-bound variants: the primal stage z and the control row of sub-step s - 1 are fetched while sub-step s is being reversed.
  // Loaded where they are used, each costs a full global / scalar memory round trip on the critical path of EVERY step of a sweep
  // that is nothing but one dependent chain per initial condition.
  constexpr bool ZAHEAD = !TM::V::LEAN;
  double2 znext[ZAHEAD ? EPT : 1];
  StepC<Q> cn;
  auto load_stage = [&](int ss, double2(&dst)[ZAHEAD ? EPT : 1]) {
#pragma unroll
    for (int j = 0; j < (ZAHEAD ? EPT : 0); j++) dst[j] = stage_load(A.ztraj, (size_t)ss * A.nb + tm.ic0, dim, tm.st.it[j]);
  };
  if (ZAHEAD && !ee && A.nsub > 0) {
    load_stage(A.nsub - 1, znext);
    load_step<Q>(sweep_ctl<SETS>(A, tm.ic0) + (size_t)(A.nsub - 1) * A.cs, cn, jpairs);
  }
  // sensitivity form: packed level digits of the thread's elements (from their natural index), the NS sums of the whole sweep
  constexpr int NSENS = SENS ? sens_count(Q) : 1;
  double sacc[NSENS];
  unsigned sbra[SENS ? EPT : 1], sket[SENS ? EPT : 1];
  if constexpr (SENS) {
#pragma unroll
    for (int i = 0; i < NSENS; i++) sacc[i] = 0.0;
#pragma unroll
    for (int j = 0; j < EPT; j++) sens_decode<Q, LIND>(S, at_use<EPT>(tm.st.it[j]), sbra[j], sket[j]);
  }

  vm_drain();
  for (int s = A.nsub - 1; s >= 0; s--) {
    if (CARRY) {
#pragma unroll
      for (int j = 0; j < EPT; j++) x[j] = xnext[CARRY ? j : 0];
      if (s > 0) load_state(s - 1, reinterpret_cast<double2(&)[EPT]>(xnext));
    } else if (ee) {
      load_state(s, x);
    }
    // ---- penalty adjoints at the end of a full step, using the primal x_n (timestepper.cpp:220-227)
    if ((pen_on || dpdm_on) && (s + 1) % A.nstages == 0) {
      const int n = (s + 1) / A.nstages;
      const double tstop = n * A.dt;
      if (!CARRY) load_state(s + 1, xn);
      if (dpdm_on) {  // penaltyDpDm_diff (timestepper.cpp:372-442); all five states come from HBM
        double2 m2[EPT], m1[EPT], p1[EPT], p2[EPT];
        if (n > 1) load_state((n - 2) * A.nstages, m2);
        if (n > 0) load_state((n - 1) * A.nstages, m1);
        if (n < ntime) load_state((n + 1) * A.nstages, p1);
        if (n < ntime - 1) load_state((n + 2) * A.nstages, p2);
#pragma unroll
        for (int j = 0; j < EPT; j++) {
          const double Jb = jbar_dpdm / ntime;
          const double xr = xn[j].x, xi = xn[j].y;
          double acc = 0.0;
          if (n > 1) {
            const double t1 = m2[j].x * m2[j].x - 2.0 * m1[j].x * m1[j].x + xr * xr;
            const double t2 = m2[j].y * m2[j].y - 2.0 * m1[j].y * m1[j].y + xi * xi;
            acc += 2.0 * (t1 + t2);
          }
          if (n > 0 && n < ntime) {
            const double t1 = m1[j].x * m1[j].x - 2.0 * xr * xr + p1[j].x * p1[j].x;
            const double t2 = m1[j].y * m1[j].y - 2.0 * xi * xi + p1[j].y * p1[j].y;
            acc += -4.0 * (t1 + t2);
          }
          if (n < ntime - 1) {
            const double t1 = xr * xr - 2.0 * p1[j].x * p1[j].x + p2[j].x * p2[j].x;
            const double t2 = xi * xi - 2.0 * p1[j].y * p1[j].y + p2[j].y * p2[j].y;
            acc += 2.0 * (t1 + t2);
          }
          xb[j].x += acc * 2.0 * xr * dtinv4 * Jb;
          xb[j].y += acc * 2.0 * xi * dtinv4 * Jb;
        }
      }
      if (pen_on) {  // penaltyIntegral_diff (timestepper.cpp:300-339)
        if (wj_on) {
          double weight;
          if (A.wjw) {
            weight = to_scalar(A.wjw[n - 1]);
          } else {
            const double a = (tstop - A.Tfinal) / A.penalty_param;
            weight = 1.0 / A.penalty_param * exp(-(a * a));
          }
          double rb, ib;
          if (wj_reduce) {
            double v[2] = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < EPT; j++)
              if (tm.ok(j)) evalJ_part<LIND>(S, A.tg, tm.ic0, at_use<EPT>(tm.st.it[j]), xn[j], v[0], v[1]);
            tm.template sum<2>(v);
            finalizeJ_diff<LIND>(A.tg, v[0], v[1], rb, ib);
          } else {
            finalizeJ_diff<LIND>(A.tg, 0.0, 0.0, rb, ib);
          }
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.ok(j))
              evalJ_diff_elem<LIND>(S, A.tg, tm.ic0, at_use<EPT>(tm.st.it[j]), xn[j], xb[j], weight * rb * jbar_pen * A.dt,
                                    weight * ib * jbar_pen * A.dt);
        }
#pragma unroll
        for (int j = 0; j < EPT; j++)
          if (guard[j]) {
            xb[j].x += 2.0 * xn[j].x * jbar_pen / ntime;
            xb[j].y += 2.0 * xn[j].y * jbar_pen / ntime;
          }
      }
    }
    StepC<Q> c;
    double2 znow[ZAHEAD ? EPT : 1];
    if (ZAHEAD && !ee) {
      c = cn;
#pragma unroll
      for (int j = 0; j < (ZAHEAD ? EPT : 0); j++) znow[j] = znext[j];
      if (s > 0) {
        load_stage(s - 1, znext);
        load_step<Q>(sweep_ctl<SETS>(A, tm.ic0) + (size_t)(s - 1) * A.cs, cn, jpairs);
      }
    } else {
      load_step<Q>(sweep_ctl<SETS>(A, tm.ic0) + (size_t)s * A.cs, c, jpairs);
    }
    if (TM::V::LEAN) scalarize<Q>(c, jpairs);
    c.g = S.dense ? reinterpret_cast<const double2*>(sweep_gtab<SETS>(A, S, tm.ic0)) + (size_t)s * S.N * S.N : nullptr;
    tm.st.prep(S, tm.L, c);
    double cf[2 * Q];
#pragma unroll
    for (int i = 0; i < 2 * Q; i++) cf[i] = 0.0;
    // (the coefficient sums are completed behind the barrier that publishes the next vector: store_coeffs, tm.publish, collect_coeffs)
    auto coeff_dst = [&](int g) -> double* { return A.coeff + ((size_t)tm.ic0 * A.nsub + s) * 2 * Q + g; };
    auto store_coeffs = [&]() { tm.template sum_store_post<2 * Q>(cf, coeff_dst); };
    auto collect_coeffs = [&]() { tm.template sum_store_collect<2 * Q>(coeff_dst); };
    if (ee) {
      // ExplEuler::evolveBWD (timestepper.cpp:506-520): gradient with dt * x_adj against x_{n-1}, then
      // x_adj += dt M(tstop)^T x_adj.  The table row of sub-step s holds M(tstart); M(tstop) is row s+1
      // (the last row is followed by one extra row for t = T).
      tm.publish(x);
#pragma unroll
      for (int j = 0; j < EPT; j++)
        if (tm.ok(j)) {
#pragma unroll
          for (int k = 0; k < Q; k++) {
            double2 Av, Bv;
            tm.st.ladder(S, tm.L, tm.vec(), k, j, Av, Bv);
            cf[2 * k] += c.h * (Bv.y * xb[j].x - Bv.x * xb[j].y);
            cf[2 * k + 1] += c.h * (Av.x * xb[j].x + Av.y * xb[j].y);
          }
        }
      store_coeffs();
      StepC<Q> c1;
      load_step<Q>(sweep_ctl<SETS>(A, tm.ic0) + (size_t)(s + 1) * A.cs, c1, jpairs);
      c1.g = S.dense ? reinterpret_cast<const double2*>(sweep_gtab<SETS>(A, S, tm.ic0)) + (size_t)(s + 1) * S.N * S.N : nullptr;
      tm.st.prep(S, tm.L, c1);
      tm.publish(xb);
      collect_coeffs();
      double2 t[EPT];
      tm.template apply_all<true>(S, c1, xb, t);
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        xb[j].x = fma(c.h, t[j].x, xb[j].x);
        xb[j].y = fma(c.h, t[j].y, xb[j].y);
      }
    } else {
      // ImplMidpoint::evolveBWD (timestepper.cpp:631-694).  The reference repeats the forward solve of the sub-step to get the
      // primal stage z = x + h/2 k (:640-652); here the forward sweep has stored z next to the trajectory (SweepArgs::ztraj,
      // the same solve on the same data: identical values), so only the adjoint solve remains and neither x nor z is alive
      // while it runs.
      double2 kb[EPT];  // adjoint stage: (I - h/2 M)^T kbar = xbar ; kbar *= h
      tm.template solve<true>(A, c, 0.5 * c.h, xb, kb);
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        kb[j].x *= c.h;
        kb[j].y *= c.h;
      }
      double2 z[EPT];
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        if (ZAHEAD) {
          z[j] = znow[ZAHEAD ? j : 0];
        } else {
          z[j] = stage_load(A.ztraj, (size_t)s * A.nb + tm.ic0, dim, tm.st.it[j]);
        }
      }
      tm.publish(z);
      // gradient coefficients: x^T dM/dp_k z and x^T dM/dq_k z with x := kbar
      if constexpr (TM::ST::WHOLE) {  // matrix-core stencils: the commutators of all the thread's elements at once per oscillator
        typename TM::ST::ZOps zo;
        tm.st.ladder_fetch(tm.vec(), zo);
#pragma unroll
        for (int k = 0; k < Q; k++) {
          double2 Av[EPT], Bv[EPT];
          tm.st.ladder_whole(S, zo, k, Av, Bv);
#pragma unroll
          for (int j = 0; j < EPT; j++)
            if (tm.ok(j)) {
              cf[2 * k] += Bv[j].y * kb[j].x - Bv[j].x * kb[j].y;
              cf[2 * k + 1] += Av[j].x * kb[j].x + Av[j].y * kb[j].y;
            }
        }
      } else {
#pragma unroll
        for (int j = 0; j < EPT; j++)
          if (tm.ok(j)) {
#pragma unroll
            for (int k = 0; k < Q; k++) {
              double2 Av, Bv;
              tm.st.ladder(S, tm.L, tm.vec(), k, j, Av, Bv);
              cf[2 * k] += Bv.y * kb[j].x - Bv.x * kb[j].y;
              cf[2 * k + 1] += Av.x * kb[j].x + Av.y * kb[j].y;
            }
          }
      }
      if constexpr (SENS) {  // kbar^T (dM/d theta) z of the diagonal, time-independent model operators (qd_sens.h)
#pragma unroll
        for (int j = 0; j < EPT; j++)
          sens_add<Q, LIND>(sbra[j], sket[j], tm.ok(j) ? kb[j].x * z[j].y - kb[j].y * z[j].x : 0.0, sacc);
      }
      store_coeffs();
      // xbar += M^T kbar
      tm.publish(kb);
      collect_coeffs();
      double2 t[EPT];
      tm.template apply_all<true>(S, c, kb, t);
#pragma unroll
      for (int j = 0; j < EPT; j++) {
        xb[j].x += t[j].x;
        xb[j].y += t[j].y;
      }
    }
    if (CARRY) {
#pragma unroll
      for (int j = 0; j < EPT; j++) xn[j] = x[j];
    }
  }
  if constexpr (SENS) sens_store<NSENS>(tm, sacc, A.S.tred + (size_t)tm.ic0 * NSENS);  // [nb][NS], summed over the states on the host side
  if (A.xbar0) {
#pragma unroll
    for (int j = 0; j < EPT; j++)
      if (tm.ok(j)) {
        double* d0 = A.xbar0 + (size_t)tm.ic0 * 2 * dim;
        d0[tm.st.it[j]] = xb[j].x;
        d0[dim + tm.st.it[j]] = xb[j].y;
      }
  }

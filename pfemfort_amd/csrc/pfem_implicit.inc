// pfem_implicit.inc -- implicit time stepping on an assembled system (pfem_dynamics_run_implicit; DESIGN.md section 12): Newmark
// (beta, gamma) and the theta-method on the lumped mass of pfem_dynamics_setup.  Included once by pfem_device.hip after
// pfem_dynamics.inc.  Every step is one solve (K + sigma diag(m)) d = b from d = 0 by a Jacobi-PCG whose operator is the SpMV in
// effect plus a diagonal; the preconditioner is ALWAYS the point Jacobi of the shifted operator, whatever the solver's pc.  A
// path beside the solve: it reads the assembled matrix, the load and the mass, and writes only the buffers of Imp -- not the
// solution vector, d_dinv and its codes, the solve's control block and history, last_its / last_reason / last_rnorm, the
// timings or the solver's CG graphs (the control loop below is its own for that reason; cg_iterate writes those).

namespace {

constexpr int kImpGraphIters = 8;          // iterations of one captured graph
constexpr int kImpChunk = 32;              // iterations enqueued between two reads of the control block

unsigned imp_grid(int64_t n) { return static_cast<unsigned>(std::min<int64_t>(kMaxGrid, std::max<int64_t>(1, (n + kDynBlockRows - 1) / kDynBlockRows))); }

int imp_check_args(int scheme, double dt, int64_t n_steps, double p0, double p1, double alpha, int64_t sample_every)
{
    if (!(dt > 0.0) || !std::isfinite(dt) || n_steps < 0 || sample_every < 0 || !(alpha >= 0.0) || !std::isfinite(alpha)) return PFEM_ERR_ARG;
    if (scheme == PFEM_SCHEME_NEWMARK) {
        if (!(p0 > 0.0) || !std::isfinite(p0) || !(p1 >= 0.5) || !std::isfinite(p1)) return PFEM_ERR_ARG;
    } else if (scheme == PFEM_SCHEME_THETA) {
        if (!(p0 > 0.0) || !(p0 <= 1.0) || alpha != 0.0) return PFEM_ERR_ARG;
    } else {
        return PFEM_ERR_ARG;
    }
    return PFEM_OK;
}

ImpPar imp_par(int64_t n, int scheme, double dt, double p0, double p1, double alpha)
{
    ImpPar P{};
    P.n = n;
    P.scheme = scheme;
    P.dt = dt;
    P.alpha = alpha;
    if (scheme == PFEM_SCHEME_NEWMARK) {
        P.bdt2 = p0 * (dt * dt);
        P.gdt = p1 * dt;
        P.sigma = (1.0 + P.gdt * alpha) / P.bdt2;
        P.cu = (dt * dt) * (0.5 - p0);
        P.cv = dt * (1.0 - p1);
        P.theta = 0.0;
    } else {
        P.theta = p0;
        P.sigma = 1.0 / (p0 * dt);
    }
    return P;
}

// the preconditions pfem_dynamics_run has, with its texts
int imp_needs(pfem_solver *s, const char *who)
{
    int c = 0;
    pfem_device_count(&c);
    if (c == 0) return PFEM_ERR_NOGPU;
    PFEM_TRY(needs_dynamics(s, who));
    if (s->status < PFEM_ASSEMBLY_OK) {
        set_last_error(std::string(who) + ": no assembled matrix (pfem_assemble after the last pfem_solver_set_zero)");
        return PFEM_ERR_STATE;
    }
    return PFEM_OK;
}

// the run's own buffers, at the first implicit run on this mass
int imp_ensure(pfem_solver *s)
{
    Dyn &D = *s->dyn;
    if (D.imp) return PFEM_OK;
    auto I = std::make_unique<Imp>();
    const int64_t n = D.n;
    const size_t len = static_cast<size_t>(std::max<int64_t>(n, 1));
    I->n = n;
    for (DevBuf<double> *g : {&I->s_u, &I->s_ut, &I->s_p}) {
        PFEM_TRY(g->alloc(len + 2 * kVecGuard));
        PFEM_HIP(hipMemsetAsync(g->p, 0, (len + 2 * kVecGuard) * sizeof(double), s->stream));
    }
    I->u = I->s_u.p + kVecGuard;
    I->ut = I->s_ut.p + kVecGuard;
    I->p = I->s_p.p + kVecGuard;
    for (DevBuf<double> *g : {&I->v, &I->a, &I->vt, &I->d, &I->r, &I->w, &I->dinv}) {
        PFEM_TRY(g->alloc(len));
        PFEM_HIP(hipMemsetAsync(g->p, 0, len * sizeof(double), s->stream));
    }
    PFEM_TRY(I->part.alloc(7 * static_cast<size_t>(kMaxGrid)));          // (r,z) | (z,z) | sigma m p^2 | folded (p,Kp) | T, S, W
    PFEM_TRY(I->hist0.alloc(1));
    PFEM_TRY(I->ctl.alloc(1));
    PFEM_HIP(hipMemsetAsync(I->ctl.p, 0, sizeof(CgCtl), s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    D.imp = std::move(I);
    return PFEM_OK;
}

struct ImpRun {
    pfem_solver *s;
    Imp &I;
    ImpPar P;
    DynPar C;                // the load curve (dyn_lambda reads n_curve, ct, cl)
    unsigned gv, gs;
    double *part_rz, *part_zz, *part_mp, *scal_pw, *part_e;
    int maxits;
};

ImpRun imp_run_setup(pfem_solver *s, const ImpPar &P, int maxits)
{
    Dyn &D = *s->dyn;
    Imp &I = *D.imp;
    DynPar C{};
    C.n_curve = D.n_curve;
    C.ct = D.d_ct.p;
    C.cl = D.d_cl.p;
    double *part = I.part.p;
    return ImpRun{s, I, P, C, imp_grid(D.n), spmv_blocks(s), part, part + kMaxGrid, part + 2 * kMaxGrid, part + 3 * kMaxGrid, part + 4 * kMaxGrid, maxits};
}

// dinv of the shifted operator: the diagonal of the row form, then 1 / (K_ii + sigma m_i)
int imp_form_dinv(const ImpRun &R)
{
    pfem_solver *s = R.s;
    const int64_t n = R.P.n;
    if (n > 0) {
        launch(k_extract_diag, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, s->sell(), R.I.dinv.p);
        launch(k_imp_dinv, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, R.P.sigma, s->dyn->d_m.p, R.I.dinv.p);
    }
    return check_kernel("k_imp_dinv");
}

// one iteration, enqueued: w = K p with the (p, Kp) partials, update, direction.  it < 0: inside a graph
void imp_enqueue_iteration(const ImpRun &R, int it)
{
    pfem_solver *s = R.s;
    Imp &I = R.I;
    const double *m = s->dyn->d_m.p;
    launch_spmv<true>(s, I.p, I.w.p, R.P.n, I.part_pw.p, I.ctl.p);
    const double *pw_parts;
    int pw_n;
    cg_fold(s, I.part_pw.p, R.gs, R.scal_pw, I.ctl.p, &pw_parts, &pw_n);
    launch(k_imp_update, dim3(R.gv), dim3(kBlock), 0, s->stream, nullptr, nullptr, I.ctl.p, it, R.P, pw_parts, pw_n, R.part_mp, static_cast<int>(R.gv), I.p,
           I.w.p, m, I.dinv.p, I.r.p, R.part_rz, R.part_zz);
    launch(k_imp_direction, dim3(R.gv), dim3(kBlock), 0, s->stream, nullptr, nullptr, I.ctl.p, it, R.P, R.part_rz, R.part_zz, static_cast<int>(R.gv), I.r.p,
           I.dinv.p, m, I.p, I.d.p, R.maxits, R.part_mp);
}

// predictor, K ut, right-hand side and the start of the CG for the step n -> n + 1 (rtol / abstol / dtol: the stopping rule)
void imp_enqueue_start(const ImpRun &R, long long n, double t_base, double rtol, double abstol, double dtol)
{
    pfem_solver *s = R.s;
    Imp &I = R.I;
    const Dyn &D = *s->dyn;
    const bool nm = R.P.scheme == PFEM_SCHEME_NEWMARK;
    const double tn0 = t_base + static_cast<double>(n) * R.P.dt, tn1 = t_base + static_cast<double>(n + 1) * R.P.dt;
    if (nm) launch(k_imp_predict, dim3(R.gv), dim3(kBlock), 0, s->stream, nullptr, nullptr, R.P, I.u, I.v.p, I.a.p, I.ut, I.vt.p);
    launch_spmv<false>(s, nm ? I.ut : I.u, I.w.p, 0, nullptr, nullptr);
    launch(k_imp_rhs, dim3(R.gv), dim3(kBlock), 0, s->stream, nullptr, nullptr, R.P, R.C, tn0, nm ? 0.0 : 1.0 - R.P.theta, tn1, nm ? 1.0 : R.P.theta, s->d_rhs.p,
           D.d_m.p, nm ? I.vt.p : nullptr, I.w.p, I.dinv.p, I.d.p, I.r.p, I.p, R.part_rz, R.part_zz, R.part_mp);
    launch(k_cg_start, dim3(1), dim3(kBlock), 0, s->stream, nullptr, nullptr, I.ctl.p, R.part_rz, R.part_zz, static_cast<int>(R.gv), nullptr, rtol, abstol, dtol,
           I.hist0.p);
}

std::vector<uint64_t> imp_graph_key(const ImpRun &R)
{
    const pfem_solver *s = R.s;
    const Imp &I = R.I;
    auto ptr = [](const void *p) { return reinterpret_cast<uint64_t>(p); };
    return {ptr(I.p), ptr(I.w.p), ptr(I.r.p), ptr(I.d.p), ptr(I.dinv.p), ptr(I.part.p), ptr(I.part_pw.p), ptr(I.ctl.p), ptr(s->dyn->d_m.p),
            ptr(s->d_vals.p), ptr(s->d_cols.p), ptr(s->d_rvals.p), ptr(s->d_gvals.p), ptr(s->d_dwords.p), ptr(s->stream),
            static_cast<uint64_t>(R.P.n), static_cast<uint64_t>(R.gv), static_cast<uint64_t>(R.gs), static_cast<uint64_t>(R.maxits),
            dyn_bits(R.P.sigma), spmv_key(s), spmv_form(s).kernel_id()};
}

// The control loop of one step's solve: enqueue a chunk, read the control block, stop on its flag or at maxits.  *h: the block
// as last read.  use_graph: whole units of kImpGraphIters iterations replay the captured graph.
int imp_iterate(const ImpRun &R, bool use_graph, CgCtl *h)
{
    pfem_solver *s = R.s;
    for (int it = 0;;) {
        const int it_end = std::min(it + kImpChunk, R.maxits);
        while (it < it_end) {
            if (use_graph && it + kImpGraphIters <= it_end) {
                PFEM_HIP(hipGraphLaunch(R.I.graph.exec[0], s->stream));
                it += kImpGraphIters;
            } else {
                imp_enqueue_iteration(R, it);
                ++it;
            }
        }
        PFEM_TRY(check_kernel("implicit pcg iteration"));
        PFEM_HIP(hipMemcpyAsync(s->h_ctl, R.I.ctl.p, sizeof(CgCtl), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        *h = *s->h_ctl;
        if (h->flag != 0) break;
        if (it >= R.maxits) { h->flag = -3; break; }
    }
    return PFEM_OK;
}

int imp_ensure_graph(const ImpRun &R, bool *use_graph)
{
    pfem_solver *s = R.s;
    *use_graph = false;
    if (R.P.n <= 0 || s->stream == nullptr) return PFEM_OK;
    return R.I.graph.ensure(s->stream, imp_graph_key(R), {}, [&](int) {
        for (int k = 0; k < kImpGraphIters; ++k) imp_enqueue_iteration(R, -1);
        return hipGetLastError() == hipSuccess;
    }, use_graph);
}

}  // namespace

extern "C" int pfem_dynamics_run_implicit(pfem_solver *s, int scheme, double dt, int64_t n_steps, double p0, double p1, double alpha,
                                          int64_t sample_every, double *history, int64_t *rows, int32_t *iterations, int64_t *steps_done)
{
    if (rows) *rows = 0;
    if (steps_done) *steps_done = 0;
    if (!s) return PFEM_ERR_ARG;
    PFEM_TRY(imp_check_args(scheme, dt, n_steps, p0, p1, alpha, sample_every));
    PFEM_TRY(imp_needs(s, "pfem_dynamics_run_implicit"));
    Dyn &D = *s->dyn;
    if (D.mode != kDynFresh && D.mode != scheme + 1) {
        set_last_error(D.mode == kDynExplicit ? "pfem_dynamics_run_implicit: an implicit run after an explicit one needs a new pfem_dynamics_set_state"
                                              : "pfem_dynamics_run_implicit: another scheme than the run before needs a new pfem_dynamics_set_state");
        return PFEM_ERR_STATE;
    }
    const long long every = sample_every > 0 ? sample_every : (1LL << 62);          // 0: no rows, ever
    const int64_t n_rows = n_steps / every;
    const int ncol = 4 + 2 * D.n_probe;
    if (n_rows > 0 && !history) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    PFEM_TRY(imp_ensure(s));
    Imp &I = *D.imp;
    if (n_rows > 0 && D.d_hist.n < static_cast<size_t>(n_rows * ncol)) PFEM_TRY(D.d_hist.alloc(static_cast<size_t>(n_rows * ncol)));
    // the SpMV's copies of the matrix values, as every product outside a solve brings them up to date
    mark_group_vals(s);
    PFEM_TRY(refresh_group_vals(s));
    const unsigned gs = spmv_blocks(s);
    if (I.part_pw.n < gs + 2) PFEM_TRY(I.part_pw.alloc(gs + 2));
    const ImpRun R = imp_run_setup(s, imp_par(D.n, scheme, dt, p0, p1, alpha), s->maxits);
    const size_t bytes = sizeof(double) * static_cast<size_t>(std::max<int64_t>(D.n, 1));
    if (D.mode == kDynFresh) {             // the state of pfem_dynamics_set_state; Newmark: a_0 from it
        PFEM_HIP(hipMemcpyAsync(I.u, D.u[0], bytes, hipMemcpyDeviceToDevice, s->stream));
        PFEM_HIP(hipMemcpyAsync(I.v.p, D.d_v0.p, bytes, hipMemcpyDeviceToDevice, s->stream));
        I.t_base = D.t0;
        I.n_since = 0;
        I.dt = dt;
        if (scheme == PFEM_SCHEME_NEWMARK) {
            launch_spmv<false>(s, I.u, I.w.p, 0, nullptr, nullptr);
            launch(k_imp_accel0, dim3(grid_for(D.n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, R.P, R.C, I.t_base, s->d_rhs.p, D.d_m.p, I.v.p, I.w.p, I.a.p);
            PFEM_TRY(check_kernel("k_imp_accel0"));
        }
        D.mode = scheme + 1;
    } else if (dt != I.dt) {               // a one-step method: another dt continues from (u, v, a) at the time reached
        I.t_base = I.t_base + static_cast<double>(I.n_since) * I.dt;
        I.n_since = 0;
        I.dt = dt;
    }
    PFEM_TRY(imp_form_dinv(R));
    bool use_graph = false;
    PFEM_TRY(imp_ensure_graph(R, &use_graph));
    int rc = PFEM_OK;
    int64_t done = 0, rows_done = 0;
    for (; done < n_steps; ++done) {
        imp_enqueue_start(R, I.n_since, I.t_base, s->rtol, s->abstol, s->dtol);
        CgCtl h{};
        PFEM_TRY(imp_iterate(R, use_graph, &h));
        if (h.flag < 0) {
            set_last_error("pfem_dynamics_run_implicit: the solve of step " + std::to_string(done) + " ended with reason " + std::to_string(h.flag) +
                           " after " + std::to_string(h.its) + " iterations; the state is that of the last completed step");
            rc = PFEM_ERR_DIVERGED;
            break;
        }
        if (iterations) iterations[done] = h.its;
        launch(k_imp_correct, dim3(R.gv), dim3(kBlock), 0, s->stream, nullptr, nullptr, R.P, I.ut, I.vt.p, I.d.p, I.u, I.v.p, I.a.p);
        ++I.n_since;
        ++D.step;
        if ((done + 1) % every == 0) {     // a sampled step: one more product, K u_{n+1}
            launch_spmv<false>(s, I.u, I.w.p, 0, nullptr, nullptr);
            launch(k_imp_energy, dim3(R.gv), dim3(kBlock), 0, s->stream, nullptr, nullptr, R.P, s->d_rhs.p, D.d_m.p, I.u, I.v.p, I.w.p, R.part_e);
            launch(k_imp_row, dim3(1), dim3(kBlock), 0, s->stream, nullptr, nullptr, I.t_base + static_cast<double>(I.n_since) * dt, R.part_e,
                   static_cast<int>(R.gv), D.n_probe, D.d_probe.p, I.u, I.v.p, D.d_hist.p + rows_done * ncol);
            ++rows_done;
        }
        PFEM_TRY(check_kernel("k_imp_correct"));
    }
    if (rows_done > 0)
        PFEM_HIP(hipMemcpyAsync(history, D.d_hist.p, sizeof(double) * static_cast<size_t>(rows_done * ncol), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    if (rows) *rows = rows_done;
    if (steps_done) *steps_done = done;
    return rc;
}

// time of one iteration of the shifted CG loop in microseconds: `iterations` iterations (whole graph units where the stream can
// be captured) between two events with no convergence exit, on the first step from the state at hand (tools/lab/
// implicit_measure.py).  The state does not advance.
extern "C" int pfem_dynamics_bench_implicit(pfem_solver *s, int scheme, double dt, double p0, double p1, int iterations, double *us_per_iteration)
{
    if (!s || iterations < 1 || !us_per_iteration) return PFEM_ERR_ARG;
    PFEM_TRY(imp_check_args(scheme, dt, 0, p0, p1, 0.0, 0));
    PFEM_TRY(imp_needs(s, "pfem_dynamics_bench_implicit"));
    Dyn &D = *s->dyn;
    PFEM_TRY(use_device(s));
    const bool fresh = !D.imp;
    PFEM_TRY(imp_ensure(s));
    Imp &I = *D.imp;
    if (fresh || D.mode <= kDynExplicit) {          // no implicit state yet: time the first step from the state as set
        const size_t bytes = sizeof(double) * static_cast<size_t>(std::max<int64_t>(D.n, 1));
        PFEM_HIP(hipMemcpyAsync(I.u, D.u[0], bytes, hipMemcpyDeviceToDevice, s->stream));
        PFEM_HIP(hipMemcpyAsync(I.v.p, D.d_v0.p, bytes, hipMemcpyDeviceToDevice, s->stream));
        PFEM_HIP(hipMemsetAsync(I.a.p, 0, bytes, s->stream));
    }
    mark_group_vals(s);
    PFEM_TRY(refresh_group_vals(s));
    const unsigned gs = spmv_blocks(s);
    if (I.part_pw.n < gs + 2) PFEM_TRY(I.part_pw.alloc(gs + 2));
    const ImpRun R = imp_run_setup(s, imp_par(D.n, scheme, dt, p0, p1, 0.0), std::numeric_limits<int>::max());
    PFEM_TRY(imp_form_dinv(R));
    bool use_graph = false;
    PFEM_TRY(imp_ensure_graph(R, &use_graph));
    // rtol = 0, abstol < 0, dtol = inf: only an exactly zero residual or a breakdown ends the loop
    auto start = [&] { imp_enqueue_start(R, 0, D.t0, 0.0, -1.0, std::numeric_limits<double>::infinity()); };
    auto loop = [&](int count) -> int {
        int it = 0;
        while (it < count) {
            if (use_graph && it + kImpGraphIters <= count) {
                PFEM_HIP(hipGraphLaunch(I.graph.exec[0], s->stream));
                it += kImpGraphIters;
            } else {
                imp_enqueue_iteration(R, it);
                ++it;
            }
        }
        return check_kernel("implicit pcg iteration");
    };
    start();
    PFEM_TRY(loop(kImpGraphIters));                 // warm up
    start();
    PFEM_HIP(hipEventRecord(s->ev0, s->stream));
    PFEM_TRY(loop(iterations));
    PFEM_HIP(hipEventRecord(s->ev1, s->stream));
    double ms = 0.0;
    PFEM_TRY(elapsed(s, &ms));
    PFEM_HIP(hipMemcpyAsync(s->h_ctl, I.ctl.p, sizeof(CgCtl), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    if (s->h_ctl->its != iterations) {
        set_last_error("pfem_dynamics_bench_implicit: the loop ended after " + std::to_string(s->h_ctl->its) + " iterations (reason " +
                       std::to_string(s->h_ctl->flag) + "): zero load and state, or a breakdown");
        return PFEM_ERR_STATE;
    }
    *us_per_iteration = 1e3 * ms / static_cast<double>(iterations);
    return PFEM_OK;
}

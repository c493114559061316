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

// What the launches of a step read and write: the vectors, the partials, the control block and the load curve.  The run fills it
// from the buffers of Imp, Dyn and the solver (imp_view), a probe (pfem_imp_probe_*) from vectors of its own; both launch through
// imp_run_of and the imp_launch_* functions below.
struct ImpView {
    int64_t n = 0;
    const double *f = nullptr, *m = nullptr;
    double *u = nullptr, *v = nullptr, *a = nullptr, *ut = nullptr, *vt = nullptr, *d = nullptr, *r = nullptr, *p = nullptr, *w = nullptr, *dinv = nullptr;
    double *part_rz = nullptr, *part_zz = nullptr, *part_mp = nullptr, *scal_pw = nullptr, *part_e = nullptr;          // part_e: [3][gv]
    CgCtl *ctl = nullptr;
    double *hist0 = nullptr;
    int n_curve = 0;
    const double *ct = nullptr, *cl = nullptr;
    int n_probe = 0;
    const int32_t *probe = nullptr;
};

ImpView imp_view(const pfem_solver *s)
{
    const Dyn &D = *s->dyn;
    const Imp &I = *D.imp;
    ImpView V;
    V.n = D.n;
    V.f = s->d_rhs.p;
    V.m = D.d_m.p;
    V.u = I.u; V.v = I.v.p; V.a = I.a.p; V.ut = I.ut; V.vt = I.vt.p; V.d = I.d.p; V.r = I.r.p; V.p = I.p; V.w = I.w.p; V.dinv = I.dinv.p;
    double *part = I.part.p;               // (r,z) | (z,z) | sigma m p^2 | folded (p,Kp) | T, S, W
    V.part_rz = part; V.part_zz = part + kMaxGrid; V.part_mp = part + 2 * kMaxGrid; V.scal_pw = part + 3 * kMaxGrid; V.part_e = part + 4 * kMaxGrid;
    V.ctl = I.ctl.p;
    V.hist0 = I.hist0.p;
    V.n_curve = D.n_curve;
    V.ct = D.d_ct.p;
    V.cl = D.d_cl.p;
    V.n_probe = D.n_probe;
    V.probe = D.d_probe.p;
    return V;
}

struct ImpRun {
    pfem_solver *s;
    ImpView V;
    ImpPar P;
    DynPar C;                // the load curve (dyn_lambda reads n_curve, ct, cl)
    unsigned gv, gs;
    int maxits;
};

// the grid of the vector kernels and the curve's block for a view; gs: the blocks of the SpMV whose partials cg_fold folds
ImpRun imp_run_of(pfem_solver *s, const ImpView &V, const ImpPar &P, unsigned gs, int maxits)
{
    DynPar C{};
    C.n_curve = V.n_curve;
    C.ct = V.ct;
    C.cl = V.cl;
    return ImpRun{s, V, P, C, imp_grid(V.n), gs, maxits};
}

ImpRun imp_run_setup(pfem_solver *s, const ImpPar &P, int maxits) { return imp_run_of(s, imp_view(s), P, spmv_blocks(s), maxits); }

// dinv of the shifted operator: the diagonal of the row form, then 1 / (K_ii + sigma m_i)
int imp_form_dinv(const ImpRun &R)
{
    pfem_solver *s = R.s;
    const int64_t n = R.P.n;
    if (n > 0) {
        launch(k_extract_diag, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, s->sell(), R.V.dinv);
        launch(k_imp_dinv, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, R.P.sigma, R.V.m, R.V.dinv);
    }
    return check_kernel("k_imp_dinv");
}

// the update of iteration `it` on w = K p, whose (p, Kp) is the sum of the pw_n doubles at pw_parts.  it < 0: inside a graph
void imp_launch_update(const ImpRun &R, int it, const double *pw_parts, int pw_n)
{
    const ImpView &V = R.V;
    launch(k_imp_update, dim3(R.gv), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, V.ctl, it, R.P, pw_parts, pw_n, V.part_mp, static_cast<int>(R.gv), V.p, V.w,
           V.m, V.dinv, V.r, V.part_rz, V.part_zz);
}

void imp_launch_direction(const ImpRun &R, int it)
{
    const ImpView &V = R.V;
    launch(k_imp_direction, dim3(R.gv), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, V.ctl, it, R.P, V.part_rz, V.part_zz, static_cast<int>(R.gv), V.r, V.dinv,
           V.m, V.p, V.d, R.maxits, V.part_mp);
}

// one iteration, enqueued: w = K p with the (p, Kp) partials, update, direction.  it < 0: inside a graph
void imp_enqueue_iteration(const ImpRun &R, int it)
{
    pfem_solver *s = R.s;
    Imp &I = *s->dyn->imp;
    launch_spmv<true>(s, R.V.p, R.V.w, R.P.n, I.part_pw.p, R.V.ctl);
    const double *pw_parts;
    int pw_n;
    cg_fold(s, I.part_pw.p, R.gs, R.V.scal_pw, R.V.ctl, &pw_parts, &pw_n);
    imp_launch_update(R, it, pw_parts, pw_n);
    imp_launch_direction(R, it);
}

// Newmark's predictor for the step from (u, v, a)
void imp_launch_predict(const ImpRun &R)
{
    const ImpView &V = R.V;
    launch(k_imp_predict, dim3(R.gv), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, R.P, V.u, V.v, V.a, V.ut, V.vt);
}

// right-hand side and the start of the CG for the step n -> n + 1 on w = K ut (theta-method: K u_n); rtol / abstol / dtol: the
// stopping rule
void imp_launch_rhs(const ImpRun &R, long long n, double t_base, double rtol, double abstol, double dtol)
{
    const ImpView &V = R.V;
    const bool nm = R.P.scheme == PFEM_SCHEME_NEWMARK;
    const double tn0 = t_base + static_cast<double>(n) * R.P.dt, tn1 = t_base + static_cast<double>(n + 1) * R.P.dt;
    launch(k_imp_rhs, dim3(R.gv), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, R.P, R.C, tn0, nm ? 0.0 : 1.0 - R.P.theta, tn1, nm ? 1.0 : R.P.theta, V.f, V.m,
           nm ? V.vt : nullptr, V.w, V.dinv, V.d, V.r, V.p, V.part_rz, V.part_zz, V.part_mp);
    launch(k_cg_start, dim3(1), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, V.ctl, V.part_rz, V.part_zz, static_cast<int>(R.gv), nullptr, rtol, abstol, dtol,
           V.hist0);
}

// predictor, K ut, right-hand side and the start of the CG for the step n -> n + 1
void imp_enqueue_start(const ImpRun &R, long long n, double t_base, double rtol, double abstol, double dtol)
{
    const bool nm = R.P.scheme == PFEM_SCHEME_NEWMARK;
    if (nm) imp_launch_predict(R);
    launch_spmv<false>(R.s, nm ? R.V.ut : R.V.u, R.V.w, 0, nullptr, nullptr);
    imp_launch_rhs(R, n, t_base, rtol, abstol, dtol);
}

void imp_launch_correct(const ImpRun &R)
{
    const ImpView &V = R.V;
    launch(k_imp_correct, dim3(R.gv), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, R.P, V.ut, V.vt, V.d, V.u, V.v, V.a);
}

// the history row of the state (u, v) at time t on w = K u: the partials of the sums, then the one block that adds them
void imp_launch_row(const ImpRun &R, double t, double *row)
{
    const ImpView &V = R.V;
    launch(k_imp_energy, dim3(R.gv), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, R.P, V.f, V.m, V.u, V.v, V.w, V.part_e);
    launch(k_imp_row, dim3(1), dim3(kBlock), 0, R.s->stream, nullptr, nullptr, t, V.part_e, static_cast<int>(R.gv), V.n_probe, V.probe, V.u, V.v, row);
}

std::vector<uint64_t> imp_graph_key(const ImpRun &R)
{
    const pfem_solver *s = R.s;
    const ImpView &V = R.V;
    auto ptr = [](const void *p) { return reinterpret_cast<uint64_t>(p); };
    return {ptr(V.p), ptr(V.w), ptr(V.r), ptr(V.d), ptr(V.dinv), ptr(V.part_rz), ptr(s->dyn->imp->part_pw.p), ptr(V.ctl), ptr(V.m),
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
                PFEM_HIP(hipGraphLaunch(s->dyn->imp->graph.exec[0], s->stream));
                it += kImpGraphIters;
            } else {
                imp_enqueue_iteration(R, it);
                ++it;
            }
        }
        PFEM_TRY(check_kernel("implicit pcg iteration"));
        PFEM_HIP(hipMemcpyAsync(s->h_ctl, R.V.ctl, sizeof(CgCtl), hipMemcpyDeviceToHost, s->stream));
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
    return s->dyn->imp->graph.ensure(s->stream, imp_graph_key(R), {}, [&](int) {
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
    const long long every = dyn_every(sample_every);
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
        imp_launch_correct(R);
        ++I.n_since;
        ++D.step;
        if ((done + 1) % every == 0) {     // a sampled step: one more product, K u_{n+1}
            launch_spmv<false>(s, I.u, I.w.p, 0, nullptr, nullptr);
            imp_launch_row(R, I.t_base + static_cast<double>(I.n_since) * dt, D.d_hist.p + rows_done * ncol);
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

// ---- one launch of a kernel of the implicit stepper on vectors of the caller's (pfem_amd_diag.h) -----------------------------------
namespace {

CgCtl imp_ctl_in(const pfem_cg_ctl &c)
{
    CgCtl k{};
    k.beta[0] = c.beta[0]; k.beta[1] = c.beta[1];
    k.rn0 = c.rn0; k.ttol = c.ttol; k.rn = c.rn; k.dtol = c.dtol; k.alpha = c.alpha;
    k.flag = c.flag; k.its = c.its; k.its_dir = c.its_dir;
    return k;
}

void imp_ctl_out(const CgCtl &k, pfem_cg_ctl *c)
{
    c->beta[0] = k.beta[0]; c->beta[1] = k.beta[1];
    c->rn0 = k.rn0; c->ttol = k.ttol; c->rn = k.rn; c->dtol = k.dtol; c->alpha = k.alpha;
    c->flag = k.flag; c->its = k.its; c->its_dir = k.its_dir;
}

// the vectors of one implicit probe: every one an allocation of its own between quiet NaNs
struct ImpProbe {
    pfem_solver *s;
    const char *who;
    size_t rows;
    std::vector<std::unique_ptr<ProbeBlock>> blocks;
    std::vector<double *> outs;
    DevBuf<CgCtl> ctl;
    int rc = PFEM_OK;
    ImpProbe(pfem_solver *s, const char *who, int64_t n) : s(s), who(who), rows(static_cast<size_t>(n)) {}
    // host == nullptr: an output (NaN throughout); keep: the launch takes it as const; out: where it comes back to
    double *add(const char *name, const double *host, size_t len, bool keep, double *out)
    {
        blocks.push_back(std::make_unique<ProbeBlock>());
        outs.push_back(out);
        if (rc == PFEM_OK) rc = probe_upload(s, *blocks.back(), name, host, len, kProbeBack, kProbeFront, keep);
        return rc == PFEM_OK ? blocks.back()->p() : nullptr;
    }
    double *in(const char *name, const double *host) { return add(name, host, rows, true, nullptr); }
    double *io(const char *name, double *host) { return add(name, host, rows, false, host); }
    double *out(const char *name, double *host) { return add(name, nullptr, rows, false, host); }
    int put_ctl(const pfem_cg_ctl *c)
    {
        PFEM_TRY(ctl.alloc(1));
        const CgCtl k = c ? imp_ctl_in(*c) : CgCtl{};
        PFEM_HIP(hipMemcpyAsync(ctl.p, &k, sizeof k, hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        return PFEM_OK;
    }
    int get_ctl(pfem_cg_ctl *c)
    {
        CgCtl k{};
        PFEM_HIP(hipMemcpyAsync(&k, ctl.p, sizeof k, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        imp_ctl_out(k, c);
        return PFEM_OK;
    }
    // every block back, with the check of its guards and of what had to stay
    int finish()
    {
        for (size_t k = 0; k < blocks.size(); ++k) PFEM_TRY(probe_download(s, *blocks[k], outs[k], who));
        return PFEM_OK;
    }
};

}  // namespace

extern "C" int pfem_imp_probe_predict(pfem_solver *s, int64_t n, double dt, double beta, double gamma, const double *u, const double *v, const double *a,
                                      double *ut, double *vt)
{
    if (!s || n < 1 || !u || !v || !a || !ut || !vt) return PFEM_ERR_ARG;
    PFEM_TRY(imp_check_args(PFEM_SCHEME_NEWMARK, dt, 0, beta, gamma, 0.0, 0));
    PFEM_TRY(use_device(s));
    ImpProbe Q(s, "pfem_imp_probe_predict", n);
    ImpView V;
    V.n = n;
    V.u = Q.in("u", u); V.v = Q.in("v", v); V.a = Q.in("a", a);
    V.ut = Q.out("ut", ut); V.vt = Q.out("vt", vt);
    PFEM_TRY(Q.rc);
    const ImpRun R = imp_run_of(s, V, imp_par(n, PFEM_SCHEME_NEWMARK, dt, beta, gamma, 0.0), 0, 0);
    imp_launch_predict(R);
    PFEM_TRY(check_kernel("k_imp_predict"));
    return Q.finish();
}

extern "C" int pfem_imp_probe_rhs(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, int n_curve, const double *ct,
                                  const double *cl, double t_base, int64_t step, double rtol, double abstol, double dtol, const double *f, const double *m,
                                  const double *vt, const double *w, const double *dinv, double *d, double *r, double *p, double *part_rz, double *part_zz,
                                  double *part_mp, int *gv, pfem_cg_ctl *ctl)
{
    if (!s || n < 1 || n_curve < 0 || (n_curve > 0 && (!ct || !cl)) || step < 0 || !std::isfinite(t_base)) return PFEM_ERR_ARG;
    if (!f || !m || !w || !dinv || !d || !r || !p || !part_rz || !part_zz || !part_mp || !gv || !ctl) return PFEM_ERR_ARG;
    PFEM_TRY(imp_check_args(scheme, dt, 0, p0, p1, alpha, 0));
    if (scheme == PFEM_SCHEME_NEWMARK && !vt) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    ImpProbe Q(s, "pfem_imp_probe_rhs", n);
    ImpView V;
    V.n = n;
    V.f = Q.in("f", f); V.m = Q.in("m", m);
    if (scheme == PFEM_SCHEME_NEWMARK) V.vt = Q.in("vt", vt);
    V.w = Q.in("w", w); V.dinv = Q.in("dinv", dinv);
    V.d = Q.out("d", d); V.r = Q.out("r", r); V.p = Q.out("p", p);
    V.part_rz = Q.add("part_rz", nullptr, kMaxGrid, false, part_rz);
    V.part_zz = Q.add("part_zz", nullptr, kMaxGrid, false, part_zz);
    V.part_mp = Q.add("part_mp", nullptr, kMaxGrid, false, part_mp);
    V.hist0 = Q.add("hist0", nullptr, 1, false, nullptr);
    V.n_curve = n_curve;
    if (n_curve > 0) {
        V.ct = Q.add("ct", ct, static_cast<size_t>(n_curve), true, nullptr);
        V.cl = Q.add("cl", cl, static_cast<size_t>(n_curve), true, nullptr);
    }
    PFEM_TRY(Q.rc);
    PFEM_TRY(Q.put_ctl(nullptr));
    V.ctl = Q.ctl.p;
    const ImpRun R = imp_run_of(s, V, imp_par(n, scheme, dt, p0, p1, alpha), 0, 0);
    imp_launch_rhs(R, step, t_base, rtol, abstol, dtol);
    PFEM_TRY(check_kernel("k_imp_rhs"));
    PFEM_TRY(Q.get_ctl(ctl));
    *gv = static_cast<int>(R.gv);
    return Q.finish();
}

extern "C" int pfem_imp_probe_update(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, pfem_cg_ctl *ctl, int it_arg,
                                     int n_pw, const double *part_pw, int n_mp, const double *part_mp, const double *p, const double *w, const double *m,
                                     const double *dinv, double *r, double *part_rz, double *part_zz)
{
    if (!s || n < 1 || !ctl || it_arg < -1 || n_pw < 1 || !part_pw || !part_mp || !p || !w || !m || !dinv || !r || !part_rz || !part_zz) return PFEM_ERR_ARG;
    PFEM_TRY(imp_check_args(scheme, dt, 0, p0, p1, alpha, 0));
    if (n_mp != static_cast<int>(imp_grid(n))) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    ImpProbe Q(s, "pfem_imp_probe_update", n);
    ImpView V;
    V.n = n;
    const double *d_pw = Q.add("part_pw", part_pw, static_cast<size_t>(n_pw), true, nullptr);
    V.part_mp = Q.add("part_mp", part_mp, static_cast<size_t>(n_mp), true, nullptr);
    V.p = Q.in("p", p); V.w = Q.in("w", w); V.m = Q.in("m", m); V.dinv = Q.in("dinv", dinv);
    V.r = Q.io("r", r);
    V.part_rz = Q.add("part_rz", nullptr, kMaxGrid, false, part_rz);
    V.part_zz = Q.add("part_zz", nullptr, kMaxGrid, false, part_zz);
    PFEM_TRY(Q.rc);
    PFEM_TRY(Q.put_ctl(ctl));
    V.ctl = Q.ctl.p;
    const ImpRun R = imp_run_of(s, V, imp_par(n, scheme, dt, p0, p1, alpha), 0, 0);
    imp_launch_update(R, it_arg, d_pw, n_pw);
    PFEM_TRY(check_kernel("k_imp_update"));
    PFEM_TRY(Q.get_ctl(ctl));
    return Q.finish();
}

extern "C" int pfem_imp_probe_direction(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, pfem_cg_ctl *ctl, int it_arg,
                                        int n_parts, const double *part_rz, const double *part_zz, const double *r, const double *dinv, const double *m,
                                        double *p, double *d, int maxits, double *part_mp)
{
    if (!s || n < 1 || !ctl || it_arg < -1 || !part_rz || !part_zz || !r || !dinv || !m || !p || !d || !part_mp) return PFEM_ERR_ARG;
    PFEM_TRY(imp_check_args(scheme, dt, 0, p0, p1, alpha, 0));
    if (n_parts != static_cast<int>(imp_grid(n))) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    ImpProbe Q(s, "pfem_imp_probe_direction", n);
    ImpView V;
    V.n = n;
    V.part_rz = Q.add("part_rz", part_rz, static_cast<size_t>(n_parts), true, nullptr);
    V.part_zz = Q.add("part_zz", part_zz, static_cast<size_t>(n_parts), true, nullptr);
    V.r = Q.in("r", r); V.dinv = Q.in("dinv", dinv); V.m = Q.in("m", m);
    V.p = Q.io("p", p); V.d = Q.io("d", d);
    V.part_mp = Q.add("part_mp", nullptr, kMaxGrid, false, part_mp);
    PFEM_TRY(Q.rc);
    PFEM_TRY(Q.put_ctl(ctl));
    V.ctl = Q.ctl.p;
    const ImpRun R = imp_run_of(s, V, imp_par(n, scheme, dt, p0, p1, alpha), 0, maxits);
    imp_launch_direction(R, it_arg);
    PFEM_TRY(check_kernel("k_imp_direction"));
    PFEM_TRY(Q.get_ctl(ctl));
    return Q.finish();
}

extern "C" int pfem_imp_probe_correct(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, const double *ut, const double *vt,
                                      const double *d, double *u, double *v, double *a)
{
    if (!s || n < 1 || !d || !u || !v || !a) return PFEM_ERR_ARG;
    PFEM_TRY(imp_check_args(scheme, dt, 0, p0, p1, alpha, 0));
    const bool nm = scheme == PFEM_SCHEME_NEWMARK;
    if (nm && (!ut || !vt)) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    ImpProbe Q(s, "pfem_imp_probe_correct", n);
    ImpView V;
    V.n = n;
    if (nm) { V.ut = Q.in("ut", ut); V.vt = Q.in("vt", vt); }
    V.d = Q.in("d", d);
    V.u = nm ? Q.out("u", u) : Q.io("u", u);
    V.v = Q.out("v", v); V.a = Q.out("a", a);
    PFEM_TRY(Q.rc);
    const ImpRun R = imp_run_of(s, V, imp_par(n, scheme, dt, p0, p1, alpha), 0, 0);
    imp_launch_correct(R);
    PFEM_TRY(check_kernel("k_imp_correct"));
    return Q.finish();
}

extern "C" int pfem_imp_probe_energy(pfem_solver *s, int scheme, int64_t n, const double *f, const double *m, const double *u, const double *v, const double *w,
                                     int n_probe, const int32_t *probe, double t, double *row, double *part, int *gv)
{
    if (!s || n < 1 || !f || !m || !u || !v || !w || n_probe < 0 || (n_probe > 0 && !probe) || !row || !part || !gv) return PFEM_ERR_ARG;
    if (scheme != PFEM_SCHEME_NEWMARK && scheme != PFEM_SCHEME_THETA) return PFEM_ERR_ARG;
    for (int k = 0; k < n_probe; ++k)
        if (probe[k] < 0 || probe[k] >= n) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    ImpProbe Q(s, "pfem_imp_probe_energy", n);
    const unsigned g = imp_grid(n);
    ImpView V;
    V.n = n;
    V.f = Q.in("f", f); V.m = Q.in("m", m); V.u = Q.in("u", u); V.v = Q.in("v", v); V.w = Q.in("w", w);
    V.part_e = Q.add("part", nullptr, 3 * static_cast<size_t>(g), false, part);
    double *d_row = Q.add("row", nullptr, static_cast<size_t>(4 + 2 * n_probe), false, row);
    PFEM_TRY(Q.rc);
    DevBuf<int32_t> d_probe;
    PFEM_TRY(d_probe.alloc(static_cast<size_t>(std::max(n_probe, 1))));
    if (n_probe > 0) {
        PFEM_HIP(hipMemcpyAsync(d_probe.p, probe, sizeof(int32_t) * static_cast<size_t>(n_probe), hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
    }
    V.n_probe = n_probe;
    V.probe = d_probe.p;
    // the two kernels read the scheme and the row count of the parameter block, nothing else of it
    const ImpRun R = imp_run_of(s, V, scheme == PFEM_SCHEME_NEWMARK ? imp_par(n, scheme, 1.0, 0.25, 0.5, 0.0) : imp_par(n, scheme, 1.0, 1.0, 0.0, 0.0), 0, 0);
    imp_launch_row(R, t, d_row);
    PFEM_TRY(check_kernel("k_imp_energy"));
    *gv = static_cast<int>(R.gv);
    return Q.finish();
}

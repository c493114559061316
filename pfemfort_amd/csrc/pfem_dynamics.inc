// pfem_dynamics.inc -- explicit central-difference dynamics on an assembled system (pfem_dynamics_*; DESIGN.md section 11).
// Included once by pfem_device.hip, after the SpMV launch and the post-processing helpers it uses.  A path beside the solve:
// it reads the assembled matrix (by launch_spmv in the form in effect) and right-hand side and writes only its own buffers.

namespace {

constexpr int kDynGraphSteps = 48;         // steps of one captured graph: a multiple of 3 (buffer rotation) and of 2 (DynCtl parity)

int needs_dynamics(pfem_solver *s, const char *who)
{
    PFEM_TRY(needs_one_rank(s, who));
    if (!s->dyn || !s->have_pattern) {
        set_last_error(std::string(who) + ": pfem_dynamics_setup first (after every pattern build)");
        return PFEM_ERR_STATE;
    }
    return PFEM_OK;
}

// host array of the owned rows in the caller's order (pfem_solver_get_solution's) -> device vector in the internal order
int dyn_upload_rows(pfem_solver *s, const double *in, double *d_vec)
{
    const int64_t n = s->n_owned;
    std::vector<double> tmp;
    if (s->reordered) {
        tmp.assign(static_cast<size_t>(n), 0.0);
        for (int64_t i = 0; i < n; ++i) tmp[static_cast<size_t>(to_internal(s, i))] = in[i];
    }
    PFEM_HIP(hipMemcpyAsync(d_vec, tmp.empty() ? in : tmp.data(), sizeof(double) * static_cast<size_t>(n), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));       // (tmp goes out of scope)
    return PFEM_OK;
}

// blocks of a step launch = partial sums per quantity, and the doubles its [2][3][nb] partials need (never fewer than kMaxGrid:
// the mass total and the Gershgorin bound leave up to that many partials in the same buffer)
int dyn_blocks(int64_t n) { return static_cast<int>(std::max<int64_t>(1, (n + kDynBlockRows - 1) / kDynBlockRows)); }
size_t dyn_part_len(int nb) { return static_cast<size_t>(std::max(6 * nb, kMaxGrid)); }
// sample_every as the kernels take it (0: no rows, ever)
long long dyn_every(int64_t sample_every) { return sample_every > 0 ? sample_every : (1LL << 62); }

// What the launches of a step read and write: the run fills it from the buffers of Dyn and of the solver (dyn_view), a probe
// (pfem_dyn_probe_step) from vectors of its own; both launch through dyn_par, dyn_launch_step and dyn_launch_flush.
struct DynView {
    int64_t n = 0;
    int nb = 0;
    double t0 = 0.0, dt = 0.0;
    int n_curve = 0;
    const double *ct = nullptr, *cl = nullptr;
    int n_probe = 0;
    const int32_t *probe = nullptr;
    double *hist = nullptr, *part = nullptr;
    DynCtl *ctl = nullptr;
    const double *f = nullptr, *m = nullptr, *minv = nullptr, *w = nullptr;
    double *u[3] = {nullptr, nullptr, nullptr};          // u_n in u[n % 3], u_{n-1} in u[(n + 2) % 3]
};

DynView dyn_view(const pfem_solver *s)
{
    const Dyn &D = *s->dyn;
    DynView V;
    V.n = D.n;
    V.nb = D.nb;
    V.t0 = D.t0;
    V.dt = D.dt;
    V.n_curve = D.n_curve;
    V.ct = D.d_ct.p;
    V.cl = D.d_cl.p;
    V.n_probe = D.n_probe;
    V.probe = D.d_probe.p;
    V.hist = D.d_hist.p;
    V.part = D.d_part.p;
    V.ctl = D.d_ctl.p;
    V.f = s->d_rhs.p;
    V.m = D.d_m.p;
    V.minv = D.d_minv.p;
    V.w = s->d_w.p;
    for (int b = 0; b < 3; ++b) V.u[b] = D.u[b];
    return V;
}

// the parameter block of a run's launches
DynPar dyn_par(const DynView &V, double alpha, long long sample_every)
{
    DynPar P{};
    P.n = V.n;
    P.t0 = V.t0;
    P.dt = V.dt;
    P.c0 = 1.0 / (V.dt * V.dt);
    P.c1 = alpha / (2.0 * V.dt);
    P.a = P.c0 + P.c1;
    P.sample_every = sample_every;
    P.n_curve = V.n_curve;
    P.ct = V.ct;
    P.cl = V.cl;
    P.n_probe = V.n_probe;
    P.probe = V.probe;
    P.hist = V.hist;
    P.nb = V.nb;
    P.part = V.part;
    return P;
}

inline uint64_t dyn_bits(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

// k_dyn_step for n -> n + 1 on w = K u_n.  in_graph: the step index comes from the control block (the launch is replayed), else
// it is an argument.
void dyn_launch_step(pfem_solver *s, const DynView &V, const DynPar &P, long long step, bool in_graph)
{
    const double *u = V.u[step % 3], *up = V.u[(step + 2) % 3];
    double *un = V.u[(step + 1) % 3];
    launch(k_dyn_step, dim3(static_cast<unsigned>(V.nb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, P, V.ctl, static_cast<int>(step & 1),
           in_graph ? -1LL : step, V.f, V.m, V.minv, V.w, u, up, un);
}

// the history row of a run's last step n - 1 -> n = `step`, when that was a sampled one: no later launch writes it
void dyn_launch_flush(pfem_solver *s, const DynView &V, const DynPar &P, long long step, long long run_start)
{
    launch(k_dyn_flush, dim3(1), dim3(kBlock), 0, s->stream, nullptr, nullptr, P, step, run_start, static_cast<const double *>(V.u[step % 3]),
           static_cast<const double *>(V.u[(step + 2) % 3]));
}

// step n -> n + 1, enqueued: w = K u_n by the SpMV form in effect, then k_dyn_step
void dyn_enqueue_step(pfem_solver *s, const DynView &V, const DynPar &P, long long step, bool in_graph)
{
    launch_spmv<false>(s, V.u[step % 3], s->d_w.p, 0, nullptr, nullptr);
    dyn_launch_step(s, V, P, step, in_graph);
}

}  // namespace

// Lumped mass of the mesh on the device: m and 1 / m per matrix row, the total mass of the body (all nodes, constrained ones
// included).  density: one entry per material row, or one entry without a map.
extern "C" int pfem_dynamics_setup(pfem_solver *s, const double *elemData, const double *density, double *total_mass)
{
    if (!s || !density) return PFEM_ERR_ARG;
    PFEM_TRY(needs_pattern(s, "pfem_dynamics_setup"));
    if (s->status < PFEM_ASSEMBLY_OK) {
        set_last_error("pfem_dynamics_setup: assemble the matrix first");
        return PFEM_ERR_STATE;
    }
    const MeshDev &m = s->mesh;
    if ((m.kind == PFEM_ELAST_TRIA || s->n_mat > 0) && !elemData) return PFEM_ERR_ARG;
    for (int k = 0; k < std::max(s->n_mat, 1); ++k)
        if (!(density[k] > 0.0) || !std::isfinite(density[k])) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    auto D = std::make_unique<Dyn>();
    const int64_t n = s->n_loc, nn = m.nNode;
    D->n = n;
    D->nb = dyn_blocks(n);
    PFEM_TRY(D->d_mnode.alloc(static_cast<size_t>(std::max<int64_t>(nn, 1))));
    PFEM_TRY(D->d_m.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
    PFEM_TRY(D->d_minv.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
    PFEM_TRY(D->d_v0.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
    PFEM_TRY(D->d_part.alloc(dyn_part_len(D->nb)));
    PFEM_TRY(D->d_ctl.alloc(1));
    for (int b = 0; b < 3; ++b) {
        const size_t len = static_cast<size_t>(n) + 2 * kVecGuard;
        PFEM_TRY(D->d_ustore[b].alloc(len));
        PFEM_HIP(hipMemsetAsync(D->d_ustore[b].p, 0, len * sizeof(double), s->stream));
        D->u[b] = D->d_ustore[b].p + kVecGuard;
    }
    PFEM_HIP(hipMemsetAsync(D->d_v0.p, 0, sizeof(double) * static_cast<size_t>(std::max<int64_t>(n, 1)), s->stream));
    PFEM_HIP(hipMemsetAsync(D->d_m.p, 0, sizeof(double) * static_cast<size_t>(std::max<int64_t>(n, 1)), s->stream));
    PFEM_HIP(hipMemsetAsync(D->d_minv.p, 0, sizeof(double) * static_cast<size_t>(std::max<int64_t>(n, 1)), s->stream));
    DevBuf<double> d_dens;
    DynDens dens{nullptr, density[0]};
    if (s->n_mat > 0) {
        PFEM_TRY(d_dens.alloc(static_cast<size_t>(s->n_mat)));
        PFEM_HIP(hipMemcpyAsync(d_dens.p, density, sizeof(double) * static_cast<size_t>(s->n_mat), hipMemcpyHostToDevice, s->stream));
        dens.tab = d_dens.p;
    }
    const int rc = with_elem_prm(s, elemData, nullptr, [&](const auto &prm) -> int {
        using PRM = std::decay_t<decltype(prm)>;
        const dim3 block(kBlock);
        PFEM_HIP(hipMemsetAsync(s->d_err.p, 0, sizeof(int), s->stream));
        PFEM_TRY(node_accumulate(
            s, "k_dyn_mass", {{D->d_mnode.p, nn}},
            [&](auto kind, dim3 grid, const uint8_t *hubs) {
                launch(k_dyn_mass_gather<decltype(kind)::value, PRM>, grid, block, 0, s->stream, nullptr, nullptr, m, prm, dens, s->d_inc_ptr.p, s->d_inc_cnt.p,
                       s->d_inc_rec.p, hubs, D->d_mnode.p, s->d_err.p);
            },
            [&](auto kind, dim3 grid, const uint8_t *hubs) {
                launch(k_dyn_mass_scatter<decltype(kind)::value, PRM>, grid, block, 0, s->stream, nullptr, nullptr, m, prm, dens, hubs, D->d_mnode.p,
                       s->d_err.p);
            }));
        if (m.nElem > 0) {
            launch(k_dyn_mass_rows, dim3(grid_for(m.nElem * m.nsize)), block, 0, s->stream, nullptr, nullptr, m, D->d_mnode.p, D->d_m.p, D->d_minv.p);
            PFEM_TRY(check_kernel("k_dyn_mass_rows"));
        }
        const unsigned gv = vec_grid(nn);
        launch(k_dyn_mass_total, dim3(gv), block, 0, s->stream, nullptr, nullptr, nn, D->d_mnode.p, D->d_part.p);
        PFEM_TRY(check_kernel("k_dyn_mass_total"));
        std::vector<double> h(gv);
        PFEM_HIP(hipMemcpyAsync(h.data(), D->d_part.p, sizeof(double) * gv, hipMemcpyDeviceToHost, s->stream));
        int err = 0;
        PFEM_TRY(fetch_err(s, &err));         // (waits for the stream)
        D->total_mass = 0.0;
        for (double v : h) D->total_mass += v;          // the blocks' partials in block order
        return err;
    });
    if (rc != PFEM_OK) return rc;
    // the default state: at rest at t = 0
    const DynCtl c0{{0, 0}, 0};
    PFEM_HIP(hipMemcpyAsync(D->d_ctl.p, &c0, sizeof c0, hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    if (total_mass) *total_mass = D->total_mass;
    s->dyn = std::move(D);
    return PFEM_OK;
}

// m per owned dof, in pfem_solver_get_solution's order
extern "C" int pfem_dynamics_get_mass(pfem_solver *s, double *mass_owned)
{
    if (!s || !mass_owned) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_get_mass"));
    PFEM_TRY(use_device(s));
    return download_external(s, s->dyn->d_m.p, mass_owned, s->n_owned);
}

// dt = 2 / sqrt(max_i sum_j |K_ij| / m_i): Gershgorin's bound on the largest eigenvalue of M^-1 K, so never above 2 / omega_max.
// One pass over the assembled matrix in its row form (the form every assembly writes).
extern "C" int pfem_dynamics_stable_dt(pfem_solver *s, double *dt)
{
    if (!s || !dt) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_stable_dt"));
    PFEM_TRY(use_device(s));
    Dyn &D = *s->dyn;
    const unsigned gv = vec_grid(D.n);
    launch(k_dyn_gershgorin, dim3(gv), dim3(kBlock), 0, s->stream, nullptr, nullptr, s->sell(), D.n, D.d_minv.p, D.d_part.p);
    PFEM_TRY(check_kernel("k_dyn_gershgorin"));
    std::vector<double> h(gv);
    PFEM_HIP(hipMemcpyAsync(h.data(), D.d_part.p, sizeof(double) * gv, hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    const double best = *std::max_element(h.begin(), h.end());
    if (!(best > 0.0)) {
        set_last_error("pfem_dynamics_stable_dt: the matrix has no entries (or no mass)");
        return PFEM_ERR_STATE;
    }
    *dt = 2.0 / std::sqrt(best);
    return PFEM_OK;
}

// State at t0: u0, v0 per owned dof in pfem_solver_get_solution's order (NULL: zeros).  u_{-1} is formed at the next run.
extern "C" int pfem_dynamics_set_state(pfem_solver *s, double t0, const double *u0, const double *v0)
{
    if (!s || !std::isfinite(t0)) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_set_state"));
    PFEM_TRY(use_device(s));
    Dyn &D = *s->dyn;
    const size_t nb = sizeof(double) * static_cast<size_t>(std::max<int64_t>(D.n, 1));
    if (u0) PFEM_TRY(dyn_upload_rows(s, u0, D.u[0]));
    else PFEM_HIP(hipMemsetAsync(D.u[0], 0, nb, s->stream));
    if (v0) PFEM_TRY(dyn_upload_rows(s, v0, D.d_v0.p));
    else PFEM_HIP(hipMemsetAsync(D.d_v0.p, 0, nb, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    D.t0 = t0;
    D.step = 0;
    D.dt = 0.0;
    D.started = false;
    D.mode = kDynFresh;
    return PFEM_OK;
}

// lambda(t): piecewise linear through (t[k], lambda[k]), t strictly ascending, constant outside; n = 0: lambda = 1.  It scales
// the assembled right-hand side as a whole.
extern "C" int pfem_dynamics_set_load_curve(pfem_solver *s, int n, const double *t, const double *lambda)
{
    if (!s || n < 0 || (n > 0 && (!t || !lambda))) return PFEM_ERR_ARG;
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(t[k]) || !std::isfinite(lambda[k]) || (k > 0 && !(t[k] > t[k - 1]))) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_set_load_curve"));
    PFEM_TRY(use_device(s));
    Dyn &D = *s->dyn;
    if (n > 0) {
        PFEM_TRY(D.d_ct.alloc(static_cast<size_t>(n)));
        PFEM_TRY(D.d_cl.alloc(static_cast<size_t>(n)));
        PFEM_HIP(hipMemcpyAsync(D.d_ct.p, t, sizeof(double) * static_cast<size_t>(n), hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipMemcpyAsync(D.d_cl.p, lambda, sizeof(double) * static_cast<size_t>(n), hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
    }
    D.n_curve = n;
    D.graph.invalidate();          // (the table may sit where the last one sat)
    return PFEM_OK;
}

// probes: GLOBAL free-dof ids, as pfem_rhs_add_values takes them
extern "C" int pfem_dynamics_set_probes(pfem_solver *s, int n, const int64_t *global_dof)
{
    if (!s || n < 0 || (n > 0 && !global_dof)) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_set_probes"));
    std::vector<int32_t> rows(static_cast<size_t>(n));
    for (int k = 0; k < n; ++k) {
        const int64_t g = global_dof[k];
        if (g < s->row_start || g >= s->row_start + s->n_owned) return PFEM_ERR_ARG;
        rows[static_cast<size_t>(k)] = to_internal(s, g - s->row_start);
    }
    PFEM_TRY(use_device(s));
    Dyn &D = *s->dyn;
    if (n > 0) {
        PFEM_TRY(D.d_probe.alloc(static_cast<size_t>(n)));
        PFEM_HIP(hipMemcpyAsync(D.d_probe.p, rows.data(), sizeof(int32_t) * static_cast<size_t>(n), hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
    }
    D.n_probe = n;
    D.graph.invalidate();
    return PFEM_OK;
}

// n_steps central-difference steps of size dt with damping C = alpha M.  history: n_steps / sample_every rows of
// 4 + 2 n_probe doubles (may be NULL with rows), copied back once after the last step; nothing in between waits for the device.
extern "C" int pfem_dynamics_run(pfem_solver *s, double dt, int64_t n_steps, double alpha, int64_t sample_every, double *history, int64_t *rows)
{
    if (!s || !(dt > 0.0) || !std::isfinite(dt) || n_steps < 0 || !(alpha >= 0.0) || !std::isfinite(alpha) || sample_every < 0) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_run"));
    Dyn &D = *s->dyn;
    if (D.mode > kDynExplicit) {
        set_last_error("pfem_dynamics_run: an explicit run after an implicit one needs a new pfem_dynamics_set_state");
        return PFEM_ERR_STATE;
    }
    if (D.started && dt != D.dt) {
        set_last_error("pfem_dynamics_run: another dt than the run before needs a new pfem_dynamics_set_state");
        return PFEM_ERR_STATE;
    }
    if (s->status < PFEM_ASSEMBLY_OK) {
        set_last_error("pfem_dynamics_run: no assembled matrix (pfem_assemble after the last pfem_solver_set_zero)");
        return PFEM_ERR_STATE;
    }
    PFEM_TRY(use_device(s));
    const long long every = dyn_every(sample_every);
    const int64_t n_rows = n_steps / every;
    const int ncol = 4 + 2 * D.n_probe;
    if (rows) *rows = n_rows;
    if (n_rows > 0 && !history) return PFEM_ERR_ARG;
    if (n_rows > 0 && D.d_hist.n < static_cast<size_t>(n_rows * ncol)) PFEM_TRY(D.d_hist.alloc(static_cast<size_t>(n_rows * ncol)));
    D.dt = dt;
    D.mode = kDynExplicit;
    const DynView V = dyn_view(s);          // (after d_hist has its size and D.dt its value)
    const DynPar P = dyn_par(V, alpha, every);
    // the SpMV's copies of the matrix values, as every product outside a solve brings them up to date
    mark_group_vals(s);
    PFEM_TRY(refresh_group_vals(s));
    const DynCtl c{{D.step, D.step}, D.step};
    PFEM_HIP(hipMemcpyAsync(D.d_ctl.p, &c, sizeof c, hipMemcpyHostToDevice, s->stream));
    if (!D.started) {
        launch_spmv<false>(s, D.u[0], s->d_w.p, 0, nullptr, nullptr);
        launch(k_dyn_start, dim3(grid_for(D.n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, P, s->d_rhs.p, D.d_minv.p, s->d_w.p, D.u[0], D.d_v0.p, D.u[2]);
        PFEM_TRY(check_kernel("k_dyn_start"));
        D.started = true;
    }
    const long long end = D.step + n_steps;
    // up to the next multiple of the graph's period by stream launches, whole graphs, the rest by stream launches
    while (D.step < end && (D.step % kDynGraphSteps != 0 || end - D.step < kDynGraphSteps)) {
        dyn_enqueue_step(s, V, P, D.step, false);
        ++D.step;
    }
    PFEM_TRY(check_kernel("k_dyn_step"));
    if (end - D.step >= kDynGraphSteps) {
        std::vector<uint64_t> key = {
            reinterpret_cast<uint64_t>(D.u[0]), reinterpret_cast<uint64_t>(D.u[1]), reinterpret_cast<uint64_t>(D.u[2]), reinterpret_cast<uint64_t>(s->d_w.p),
            reinterpret_cast<uint64_t>(s->d_rhs.p), reinterpret_cast<uint64_t>(D.d_m.p), reinterpret_cast<uint64_t>(D.d_minv.p),
            reinterpret_cast<uint64_t>(D.d_ctl.p), reinterpret_cast<uint64_t>(D.d_part.p), reinterpret_cast<uint64_t>(D.d_hist.p),
            reinterpret_cast<uint64_t>(D.d_ct.p), reinterpret_cast<uint64_t>(D.d_cl.p), reinterpret_cast<uint64_t>(D.d_probe.p),
            reinterpret_cast<uint64_t>(s->d_vals.p), reinterpret_cast<uint64_t>(s->d_cols.p), reinterpret_cast<uint64_t>(s->d_rvals.p),
            reinterpret_cast<uint64_t>(s->d_gvals.p), reinterpret_cast<uint64_t>(s->d_dwords.p), reinterpret_cast<uint64_t>(s->stream),
            static_cast<uint64_t>(D.n), static_cast<uint64_t>(D.nb), static_cast<uint64_t>(D.n_curve), static_cast<uint64_t>(D.n_probe),
            static_cast<uint64_t>(every), dyn_bits(P.t0), dyn_bits(P.dt), dyn_bits(P.c1), spmv_key(s), spmv_form(s).kernel_id()};
        bool use_graph = false;
        PFEM_TRY(D.graph.ensure(s->stream, std::move(key), {}, [&](int) {
            for (int j = 0; j < kDynGraphSteps; ++j) dyn_enqueue_step(s, V, P, j, true);
            return hipGetLastError() == hipSuccess;
        }, &use_graph));
        while (end - D.step >= kDynGraphSteps) {
            if (use_graph) {
                PFEM_HIP(hipGraphLaunch(D.graph.exec[0], s->stream));
            } else {          // a stream that cannot be captured (the legacy default stream): the same launches, one by one
                for (int j = 0; j < kDynGraphSteps; ++j) dyn_enqueue_step(s, V, P, D.step + j, false);
                PFEM_TRY(check_kernel("k_dyn_step"));
            }
            D.step += kDynGraphSteps;
        }
        while (D.step < end) {
            dyn_enqueue_step(s, V, P, D.step, false);
            ++D.step;
        }
        PFEM_TRY(check_kernel("k_dyn_step"));
    }
    if (n_rows > 0) {
        if (n_steps % every == 0) {          // the last step was a sampled one: no later launch writes its row
            dyn_launch_flush(s, V, P, D.step, end - n_steps);
            PFEM_TRY(check_kernel("k_dyn_flush"));
        }
        PFEM_HIP(hipMemcpyAsync(history, D.d_hist.p, sizeof(double) * static_cast<size_t>(n_rows * ncol), hipMemcpyDeviceToHost, s->stream));
    }
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

// t_n, u_n and v_{n-1/2} = (u_n - u_{n-1}) / dt per owned dof in pfem_solver_get_solution's order (before the first run: the
// u0 and v0 of pfem_dynamics_set_state); any output may be NULL
extern "C" int pfem_dynamics_get_state(pfem_solver *s, double *t, int64_t *step, double *u, double *v)
{
    if (!s) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_get_state"));
    PFEM_TRY(use_device(s));
    Dyn &D = *s->dyn;
    if (D.mode > kDynExplicit) {          // after an implicit run: (t_n, u_n, v_n), v at the integer step
        const Imp &I = *D.imp;
        if (t) *t = I.t_base + static_cast<double>(I.n_since) * I.dt;
        if (step) *step = D.step;
        if (u) PFEM_TRY(download_external(s, I.u, u, s->n_owned));
        if (v) PFEM_TRY(download_external(s, I.v.p, v, s->n_owned));
        return PFEM_OK;
    }
    if (t) *t = D.t0 + static_cast<double>(D.step) * D.dt;
    if (step) *step = D.step;
    if (u) PFEM_TRY(download_external(s, D.u[D.step % 3], u, s->n_owned));
    if (v) {
        if (!D.started) return download_external(s, D.d_v0.p, v, s->n_owned);
        DevBuf<double> dv;
        PFEM_TRY(dv.alloc(static_cast<size_t>(std::max<int64_t>(D.n, 1))));
        launch(k_dyn_velocity, dim3(grid_for(D.n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, D.n, D.dt, static_cast<const double *>(D.u[D.step % 3]),
               static_cast<const double *>(D.u[(D.step + 2) % 3]), dv.p);
        PFEM_TRY(check_kernel("k_dyn_velocity"));
        PFEM_TRY(download_external(s, dv.p, v, s->n_owned));
    }
    return PFEM_OK;
}

// time of one step in microseconds, measured inside graph replays: `graphs` replays of kDynGraphSteps steps between two events,
// after one replay to warm up (tools/lab/dynamics_measure.py).  The state advances like a run of as many steps without history.
extern "C" int pfem_dynamics_bench(pfem_solver *s, double dt, int graphs, double *us_per_step, int *steps_per_graph)
{
    if (!s || graphs < 1 || !us_per_step) return PFEM_ERR_ARG;
    PFEM_TRY(needs_dynamics(s, "pfem_dynamics_bench"));
    Dyn &D = *s->dyn;
    const long long rem = (kDynGraphSteps - D.step % kDynGraphSteps) % kDynGraphSteps;
    PFEM_TRY(pfem_dynamics_run(s, dt, rem + kDynGraphSteps, 0.0, 0, nullptr, nullptr));          // align, capture, warm up
    if (!D.graph.exec[0] || D.graph.off) {
        set_last_error("pfem_dynamics_bench: the step loop could not be captured on this stream");
        return PFEM_ERR_STATE;
    }
    PFEM_HIP(hipEventRecord(s->ev0, s->stream));
    for (int g = 0; g < graphs; ++g) PFEM_HIP(hipGraphLaunch(D.graph.exec[0], s->stream));
    PFEM_HIP(hipEventRecord(s->ev1, s->stream));
    D.step += static_cast<long long>(graphs) * kDynGraphSteps;
    double ms = 0.0;
    PFEM_TRY(elapsed(s, &ms));
    *us_per_step = 1e3 * ms / (static_cast<double>(graphs) * kDynGraphSteps);
    if (steps_per_graph) *steps_per_graph = kDynGraphSteps;
    return PFEM_OK;
}

// ---- one launch of the step kernel on vectors of the caller's (pfem_amd_diag.h) ---------------------------------------------------
namespace {
constexpr size_t kProbeFront = 8, kProbeBack = kDynBlockRows;          // quiet NaNs before and behind every vector of a stepper probe
constexpr int64_t kProbeMaxRows = 64;                                  // history rows a step probe allocates at most
}  // namespace

extern "C" int pfem_dyn_probe_step(pfem_solver *s, int64_t n, double dt, double alpha, double t0, int n_curve, const double *ct, const double *cl,
                                   int64_t step, int64_t run_start, int64_t sample_every, int n_probe, const int32_t *probe, int use_ctl,
                                   const double *f, const double *m, const double *minv, const double *w, const double *u, const double *up, double *un,
                                   double *row, int *have_row, double *part, int *nb_out, int64_t *ctl_step)
{
    if (!s || n < 1 || !(dt > 0.0) || !std::isfinite(dt) || !(alpha >= 0.0) || !std::isfinite(alpha) || !std::isfinite(t0)) return PFEM_ERR_ARG;
    if (n_curve < 0 || (n_curve > 0 && (!ct || !cl)) || n_probe < 0 || (n_probe > 0 && !probe) || sample_every < 0) return PFEM_ERR_ARG;
    if (step < 0 || run_start < 0 || run_start > step) return PFEM_ERR_ARG;
    if (!f || !m || !minv || !w || !u || !up || !un || !row || !have_row || !part || !nb_out || !ctl_step) return PFEM_ERR_ARG;
    for (int k = 0; k < n_probe; ++k)
        if (probe[k] < 0 || probe[k] >= n) return PFEM_ERR_ARG;
    const long long every = dyn_every(sample_every);
    const int64_t n_rows = (step + 1 - run_start) / every;             // rows of a run from run_start up to the state step + 1
    if (n_rows > kProbeMaxRows) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_dyn_probe_step";
    const size_t rows = static_cast<size_t>(n), ncol = static_cast<size_t>(4 + 2 * n_probe);
    const int nb = dyn_blocks(n);
    ProbeBlock bf, bm, bq, bw, bu, bp, bn, bpart, bhist, bct, bcl;
    PFEM_TRY(probe_upload(s, bf, "f", f, rows, kProbeBack, kProbeFront, true));
    PFEM_TRY(probe_upload(s, bm, "m", m, rows, kProbeBack, kProbeFront, true));
    PFEM_TRY(probe_upload(s, bq, "minv", minv, rows, kProbeBack, kProbeFront, true));
    PFEM_TRY(probe_upload(s, bw, "w", w, rows, kProbeBack, kProbeFront, true));
    PFEM_TRY(probe_upload(s, bu, "u", u, rows, kProbeBack, kProbeFront, true));
    PFEM_TRY(probe_upload(s, bp, "up", up, rows, kProbeBack, kProbeFront, true));
    PFEM_TRY(probe_upload(s, bn, "un", nullptr, rows, kProbeBack, kProbeFront));
    PFEM_TRY(probe_upload(s, bpart, "part", nullptr, dyn_part_len(nb), kProbeBack, kProbeFront));
    PFEM_TRY(probe_upload(s, bhist, "hist", nullptr, static_cast<size_t>(std::max<int64_t>(n_rows, 1)) * ncol, kProbeBack, kProbeFront));
    if (n_curve > 0) {
        PFEM_TRY(probe_upload(s, bct, "ct", ct, static_cast<size_t>(n_curve), kProbeFront, kProbeFront, true));
        PFEM_TRY(probe_upload(s, bcl, "cl", cl, static_cast<size_t>(n_curve), kProbeFront, kProbeFront, true));
    }
    DevBuf<int32_t> d_probe;
    DevBuf<DynCtl> d_ctl;
    PFEM_TRY(d_probe.alloc(static_cast<size_t>(std::max(n_probe, 1))));
    PFEM_TRY(d_ctl.alloc(1));
    DynCtl c{{ctl_step[0], ctl_step[1]}, run_start};
    if (n_probe > 0) PFEM_HIP(hipMemcpyAsync(d_probe.p, probe, sizeof(int32_t) * static_cast<size_t>(n_probe), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipMemcpyAsync(d_ctl.p, &c, sizeof c, hipMemcpyHostToDevice, s->stream));
    DynView V;
    V.n = n;
    V.nb = nb;
    V.t0 = t0;
    V.dt = dt;
    V.n_curve = n_curve;
    V.ct = n_curve > 0 ? bct.p() : nullptr;
    V.cl = n_curve > 0 ? bcl.p() : nullptr;
    V.n_probe = n_probe;
    V.probe = d_probe.p;
    V.hist = bhist.p();
    V.part = bpart.p();
    V.ctl = d_ctl.p;
    V.f = bf.p(); V.m = bm.p(); V.minv = bq.p(); V.w = bw.p();
    V.u[step % 3] = bu.p();
    V.u[(step + 2) % 3] = bp.p();
    V.u[(step + 1) % 3] = bn.p();
    const DynPar P = dyn_par(V, alpha, every);
    dyn_launch_step(s, V, P, step, use_ctl != 0);
    PFEM_TRY(check_kernel("k_dyn_step"));
    const bool sampled = (step + 1 - run_start) % every == 0;
    if (sampled) {                         // as at the end of a run whose last step was a sampled one
        dyn_launch_flush(s, V, P, step + 1, run_start);
        PFEM_TRY(check_kernel("k_dyn_flush"));
    }
    PFEM_HIP(hipMemcpyAsync(&c, d_ctl.p, sizeof c, hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    for (const ProbeBlock *B : {&bf, &bm, &bq, &bw, &bu, &bp}) PFEM_TRY(probe_download(s, *B, nullptr, who));
    if (n_curve > 0) {
        PFEM_TRY(probe_download(s, bct, nullptr, who));
        PFEM_TRY(probe_download(s, bcl, nullptr, who));
    }
    PFEM_TRY(probe_download(s, bn, un, who));
    std::vector<double> h_part(bpart.len), h_hist(bhist.len);
    PFEM_TRY(probe_download(s, bpart, h_part.data(), who));
    PFEM_TRY(probe_download(s, bhist, h_hist.data(), who));
    // the partials of the step's parity come back; those of the other parity and what lies behind both must be as they were
    const size_t mine = static_cast<size_t>(step & 1) * 3 * static_cast<size_t>(nb);
    for (size_t i = 0; i < h_part.size(); ++i)
        if ((i < mine || i >= mine + 3 * static_cast<size_t>(nb)) && !std::isnan(h_part[i])) {
            set_last_error(std::string(who) + ": the launch wrote partial " + std::to_string(i) + " outside the [3][nb] of the step's parity");
            return PFEM_ERR_HIP;
        }
    std::memcpy(part, h_part.data() + mine, sizeof(double) * 3 * static_cast<size_t>(nb));
    *have_row = sampled ? 1 : 0;
    if (sampled) std::memcpy(row, h_hist.data() + static_cast<size_t>(n_rows - 1) * ncol, sizeof(double) * ncol);
    *nb_out = nb;
    ctl_step[0] = c.step[0];
    ctl_step[1] = c.step[1];
    return PFEM_OK;
}

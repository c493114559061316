// pfem_multi.inc -- several right-hand sides in one solve (pfem_solver_solve_multi; DESIGN.md section 16): independent
// preconditioned CG iterations on panels of MB = 4 / 8 columns that share one pass over the matrix per iteration (k_spmm_dot).
// Included once by pfem_device.hip after pfem_buckling.inc.  A path beside the solve, like the modal and buckling solves: it reads
// the matrix in its row form (s->sell()) and writes only the buffers of Multi -- not the solution or the right-hand side,
// last_its / last_reason / last_rnorm, the history, the timings, the CG graphs, the status, the state of the steppers, of the
// modal, buckling or thermal paths.  One stream, plain launches, no graph.  With gamg in effect and its numeric set-up current the
// preconditioner is the cycle of the last gamg solve (amg_apply as it stands, one running column at a time); then the cycle's
// work vectors and the SpMV's value copies are written as well, as by the modal solve.

namespace {

constexpr int kMcgChunk = 16;              // iterations enqueued between two copies of the control block (point Jacobi)

template <class F>
void with_mcg_mb(int mb, F &&f)
{
    if (mb == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

unsigned mcg_vec_grid(int64_t entries) { return static_cast<unsigned>(std::min<int64_t>(kMcgVecBlocks, std::max<int64_t>(1, (entries + kBlock - 1) / kBlock))); }

// What one launch of the kernels of pfem_multi_kernels.hpp reads and writes.  The solve fills it from the buffers of Multi
// (mcg_view), a probe (pfem_multi_probe_*) from blocks of its own: both launch through the functions below.
struct McgView {
    int mb = 0;
    int64_t n = 0;
    const double *B = nullptr, *dinv = nullptr;          // dinv == nullptr: gamg (Z is the stored T R)
    double *X = nullptr, *R = nullptr, *P = nullptr, *W = nullptr, *Z = nullptr;
    double *vec = nullptr;                 // n doubles: a column of R on its way through gamg's cycle
    double *part = nullptr, *part_pw = nullptr, *fold_pw = nullptr;
    McgCtl *ctl = nullptr;
};

McgView mcg_view(Multi &M, bool gamg)
{
    McgView V;
    V.mb = M.mb;
    V.n = M.n;
    V.B = M.B.p;
    V.dinv = gamg ? nullptr : M.dinv.p;
    V.X = M.X.p; V.R = M.R.p; V.P = M.P.p; V.W = M.W.p; V.Z = gamg ? M.Z.p : nullptr;
    V.vec = M.vec.p;
    V.part = M.part.p; V.part_pw = M.part_pw.p; V.fold_pw = M.fold_pw.p;
    V.ctl = M.ctl.p;
    return V;
}

unsigned mcg_init(pfem_solver *s, const McgView &V)
{
    const unsigned g = mcg_vec_grid(V.n * V.mb);
    with_mcg_mb(V.mb, [&](auto MB) {
        launch(k_mcg_init<decltype(MB)::value>, dim3(g), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.B, V.dinv, V.X, V.R, V.P, V.part);
    });
    return g;
}
void mcg_start(pfem_solver *s, const McgView &V, unsigned nparts, double rtol, double abstol)
{
    launch(k_mcg_start, dim3(1), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.ctl, V.mb, V.part, static_cast<int>(nparts), rtol, abstol);
}
// W = K P with the partials of (p, Kp), then their fold to kFoldBlocks rows; ctl == nullptr: whatever the control block says
void mcg_product(pfem_solver *s, const McgView &V, const SellDev &A, const McgCtl *ctl)
{
    const unsigned gp = grid_for(A.n_rows);
    with_mcg_mb(V.mb, [&](auto MB) {
        launch(k_spmm_dot<decltype(MB)::value>, dim3(gp), dim3(kBlock), 0, s->stream, nullptr, nullptr, ctl, A, V.P, V.W, V.part_pw);
        launch(k_mcg_fold<decltype(MB)::value>, dim3(kFoldBlocks), dim3(kBlock), 0, s->stream, nullptr, nullptr, ctl, V.part_pw, static_cast<int>(gp), V.fold_pw);
    });
}
unsigned mcg_update(pfem_solver *s, const McgView &V)
{
    const unsigned g = mcg_vec_grid(V.n * V.mb);
    with_mcg_mb(V.mb, [&](auto MB) {
        launch(k_mcg_update<decltype(MB)::value>, dim3(g), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.ctl, V.n, V.fold_pw, V.W, V.dinv, V.R, V.part);
    });
    return g;
}
unsigned mcg_dots(pfem_solver *s, const McgView &V, const McgCtl *ctl, const double *fold_pw)
{
    const unsigned g = mcg_vec_grid(V.n * V.mb);
    with_mcg_mb(V.mb, [&](auto MB) {
        launch(k_mcg_dots<decltype(MB)::value>, dim3(g), dim3(kBlock), 0, s->stream, nullptr, nullptr, ctl, V.n, fold_pw, V.R, V.Z, V.part);
    });
    return g;
}
void mcg_verdict(pfem_solver *s, const McgView &V, unsigned nparts, double dtol, int maxits)
{
    launch(k_mcg_verdict, dim3(1), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.ctl, V.mb, V.part, static_cast<int>(nparts), dtol, maxits);
}
void mcg_direction(pfem_solver *s, const McgView &V)
{
    with_mcg_mb(V.mb, [&](auto MB) {
        launch(k_mcg_direction<decltype(MB)::value>, dim3(mcg_vec_grid(V.n * V.mb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.ctl, V.n, V.R, V.dinv, V.Z,
               V.P, V.X);
    });
}

// Z_j <- the cycle of the last gamg solve on column j of R: amg_apply as it stands, through the contiguous vector V.vec and the
// cycle's own output vector.  false: the cycle failed.
bool mcg_cycle_column(pfem_solver *s, const McgView &V, int j)
{
    bool ok = true;
    with_mcg_mb(V.mb, [&](auto MB) {
        launch(k_modal_pack<decltype(MB)::value>, dim3(grid_for(V.n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.R, j, V.vec);
        const double *z = amg_apply(s, *s->amg, V.vec, nullptr);
        if (!z) { ok = false; return; }
        launch(k_modal_unpack<decltype(MB)::value>, dim3(grid_for(V.n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, z, j, V.Z);
    });
    return ok;
}

// the run's own buffers for panels of mb columns
int mcg_ensure(pfem_solver *s, int mb, bool gamg)
{
    const int64_t n = s->n_loc;
    if (s->multi && s->multi->mb == mb && s->multi->n == n && (!gamg || s->multi->Z.p)) return PFEM_OK;
    s->multi.reset();
    auto M = std::make_unique<Multi>();
    M->mb = mb;
    M->n = n;
    const size_t rows = static_cast<size_t>(std::max<int64_t>(n, 1)), len = rows * static_cast<size_t>(mb);
    for (DevBuf<double> *g : {&M->B, &M->X, &M->R, &M->P, &M->W}) PFEM_TRY(g->alloc(len));
    if (gamg) PFEM_TRY(M->Z.alloc(len));
    PFEM_TRY(M->dinv.alloc(rows));
    PFEM_TRY(M->vec.alloc(rows));
    PFEM_TRY(M->part.alloc(static_cast<size_t>(kMcgVecBlocks) * 2 * mb));
    PFEM_TRY(M->part_pw.alloc(static_cast<size_t>(grid_for(n)) * mb));
    PFEM_TRY(M->fold_pw.alloc(static_cast<size_t>(kFoldBlocks) * mb));
    PFEM_TRY(M->ctl.alloc(1));
    if (hipHostMalloc(reinterpret_cast<void **>(&M->h_ctl), sizeof(McgCtl)) != hipSuccess) {
        (void)hipGetLastError();
        set_last_error("pfem_solver_solve_multi: no pinned host memory for the copies of the control block");
        return PFEM_ERR_NOMEM;
    }
    s->multi = std::move(M);
    return PFEM_OK;
}

int mcg_fetch_ctl(pfem_solver *s, Multi &M)
{
    PFEM_HIP(hipMemcpyAsync(M.h_ctl, M.ctl.p, sizeof(McgCtl), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

// One panel: columns j0 .. j0 + ncols - 1 of B (case-major, the caller's order) in a panel of M.mb columns, the rest zero.
// e0 / e1 (may be nullptr): events recorded after the upload and after the last copy of the control block.
int mcg_panel(pfem_solver *s, Multi &M, bool gamg, int ncols, const double *B, double *X, int *its, int *reason, double *rnorm, hipEvent_t e0, hipEvent_t e1)
{
    const int mb = M.mb;
    const int64_t n = M.n;
    const McgView V = mcg_view(M, gamg);
    const SellDev A = s->sell();
    const size_t len = static_cast<size_t>(n) * mb;
    std::vector<double> h(len, 0.0);
    for (int c = 0; c < ncols; ++c) {
        const double *b = B + static_cast<int64_t>(c) * n;
        for (int64_t i = 0; i < n; ++i) h[static_cast<size_t>(to_internal(s, i)) * mb + c] = b[i];
    }
    PFEM_HIP(hipMemcpyAsync(M.B.p, h.data(), sizeof(double) * len, hipMemcpyHostToDevice, s->stream));
    if (e0) PFEM_HIP(hipEventRecord(e0, s->stream));
    // the start: x = 0, r = b, z = T r, p = z, the tolerances
    unsigned gv = mcg_init(s, V);
    if (gamg) {
        PFEM_HIP(hipMemsetAsync(V.Z, 0, sizeof(double) * len, s->stream));
        for (int j = 0; j < ncols; ++j)
            if (!mcg_cycle_column(s, V, j)) return PFEM_ERR_HIP;
        PFEM_HIP(hipMemcpyAsync(V.P, V.Z, sizeof(double) * len, hipMemcpyDeviceToDevice, s->stream));
        gv = mcg_dots(s, V, nullptr, nullptr);
    }
    mcg_start(s, V, gv, s->rtol, s->abstol);
    PFEM_TRY(check_kernel("k_mcg_start"));
    PFEM_TRY(mcg_fetch_ctl(s, M));
    const int chunk = gamg ? 1 : kMcgChunk;              // (gamg: the host skips the cycles of the columns that have finished)
    while (M.h_ctl->running > 0 && M.h_ctl->step <= std::max(s->maxits, 1)) {
        for (int c = 0; c < chunk; ++c) {
            mcg_product(s, V, A, V.ctl);
            gv = mcg_update(s, V);
            if (gamg) {
                for (int j = 0; j < mb; ++j)
                    if (M.h_ctl->flag[j] == 0 && !mcg_cycle_column(s, V, j)) return PFEM_ERR_HIP;
                gv = mcg_dots(s, V, V.ctl, V.fold_pw);
            }
            mcg_verdict(s, V, gv, s->dtol, s->maxits);
            mcg_direction(s, V);
        }
        PFEM_TRY(check_kernel("k_mcg_direction"));
        PFEM_TRY(mcg_fetch_ctl(s, M));
    }
    if (e1) PFEM_HIP(hipEventRecord(e1, s->stream));
    const McgCtl &C = *M.h_ctl;
    for (int c = 0; c < ncols; ++c) {
        its[c] = C.its[c];
        reason[c] = (C.flag[c] == 2 && C.rn[c] <= s->abstol) ? 3 : C.flag[c];
        rnorm[c] = C.rn[c];
    }
    PFEM_HIP(hipMemcpyAsync(h.data(), M.X.p, sizeof(double) * len, hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    for (int c = 0; c < ncols; ++c) {
        double *x = X + static_cast<int64_t>(c) * n;
        for (int64_t i = 0; i < n; ++i) x[i] = h[static_cast<size_t>(to_internal(s, i)) * mb + c];
    }
    return PFEM_OK;
}

// the preconditions of pfem_solver_solve_multi after its argument checks, with their texts; *gamg: the T in effect
int mcg_needs(pfem_solver *s, int pc, const char *who, bool *gamg)
{
    int count = 0;
    pfem_device_count(&count);
    if (count == 0) return PFEM_ERR_NOGPU;
    PFEM_TRY(needs_one_rank(s, who));
    if (!s->have_pattern) {
        set_last_error(std::string(who) + ": no pattern (pfem_pattern_build, or the first assembly of the MatSetValues path)");
        return PFEM_ERR_STATE;
    }
    if (s->host_values_dirty) {
        set_last_error(std::string(who) + ": the staged MatSetValues values are not on the device yet (a pfem_solver_solve uploads them)");
        return PFEM_ERR_STATE;
    }
    if (s->status < PFEM_ASSEMBLY_OK) {
        set_last_error(std::string(who) + ": no assembled matrix (pfem_assemble after the last pfem_solver_set_zero)");
        return PFEM_ERR_STATE;
    }
    const bool want_gamg = pc == PFEM_PC_GAMG || (pc == -1 && s->pc == PFEM_PC_GAMG);
    *gamg = want_gamg && modal_gamg_current(s);
    if (pc == PFEM_PC_GAMG && !*gamg) {
        set_last_error(std::string(who) + ": pc = gamg needs a gamg solve since the last assemble (its numeric set-up is the T)");
        return PFEM_ERR_STATE;
    }
    return PFEM_OK;
}

// the panels of a call, one after the other: nrhs <= 4 one panel of 4, else panels of 8 and a last one of 4 where at most 4
// columns remain.  ms (may be nullptr): the device time between the events of the panels, summed.
int mcg_run(pfem_solver *s, int nrhs, const double *B, bool gamg, double *X, int *its, int *reason, double *rnorm, double *ms)
{
    PFEM_TRY(use_device(s));
    const int64_t n = s->n_loc;
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events()
        {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    if (ms) {
        *ms = 0.0;
        PFEM_HIP(hipEventCreate(&ev.e0));
        PFEM_HIP(hipEventCreate(&ev.e1));
    }
    int tail_build = 0;
    if (gamg) {                            // the cycle's fine-level products run in the SpMV form in effect: its copies of the values
        mark_group_vals(s);
        PFEM_TRY(refresh_group_vals(s));
        tail_build = s->amg->tail_build;
    }
    int rc = PFEM_OK;
    for (int j0 = 0; j0 < nrhs && rc == PFEM_OK;) {
        const int left = nrhs - j0, mb = left <= 4 ? 4 : 8, ncols = std::min(left, mb);
        rc = mcg_ensure(s, mb, gamg);
        if (rc != PFEM_OK) break;
        Multi &M = *s->multi;
        M.pc_used = gamg ? PFEM_PC_GAMG : PFEM_PC_JACOBI;
        // T = 1 / K_ii from the row form, in the run's own buffer
        launch(k_extract_diag, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, s->sell(), M.dinv.p);
        launch(k_modal_invert, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, M.dinv.p);
        rc = check_kernel("k_modal_invert");
        if (rc != PFEM_OK) break;
        rc = mcg_panel(s, M, gamg, ncols, B + static_cast<int64_t>(j0) * n, X + static_cast<int64_t>(j0) * n, its + j0, reason + j0, rnorm + j0, ev.e0, ev.e1);
        if (rc == PFEM_OK && ms) {
            float f = 0.f;
            if (hipEventSynchronize(ev.e1) != hipSuccess || hipEventElapsedTime(&f, ev.e0, ev.e1) != hipSuccess) rc = PFEM_ERR_HIP;
            *ms += f;
        }
        j0 += ncols;
    }
    if (gamg) s->amg->tail_build = tail_build;           // (what the last SOLVE's cycle launched, pfem_solver_amg_tail_from)
    return rc;
}

bool mcg_pc_known(int pc) { return pc == -1 || pc == PFEM_PC_JACOBI || pc == PFEM_PC_NODE_BLOCK_JACOBI || pc == PFEM_PC_GAMG; }

}  // namespace

extern "C" int pfem_solver_solve_multi(pfem_solver *s, int nrhs, const double *B, int pc, double *X, int *its, int *reason, double *rnorm)
{
    if (!s || !B || !X || !its || !reason || !rnorm) return PFEM_ERR_ARG;
    if (nrhs < 1 || nrhs > PFEM_MULTI_MAX_RHS || !mcg_pc_known(pc)) return PFEM_ERR_ARG;
    bool gamg = false;
    PFEM_TRY(mcg_needs(s, pc, "pfem_solver_solve_multi", &gamg));
    return mcg_run(s, nrhs, B, gamg, X, its, reason, rnorm, nullptr);
}

// the T of the last pfem_solver_solve_multi on this handle: PFEM_PC_JACOBI or PFEM_PC_GAMG (pfem_amd_diag.h)
extern "C" int pfem_multi_last_pc(pfem_solver *s, int *pc)
{
    if (!s || !pc) return PFEM_ERR_ARG;
    if (!s->multi) return PFEM_ERR_STATE;
    *pc = s->multi->pc_used;
    return PFEM_OK;
}

// device time [ms] of `reps` multi solves of the assembled right-hand side scaled by j + 1, each after the upload of its panels
// and up to the last copy of a control block; the iteration counts of the last one (pfem_amd_diag.h)
extern "C" int pfem_multi_bench(pfem_solver *s, int nrhs, int reps, int pc, double *ms, int *its)
{
    if (!s || !ms || !its || reps < 1) return PFEM_ERR_ARG;
    if (nrhs < 1 || nrhs > PFEM_MULTI_MAX_RHS || !mcg_pc_known(pc)) return PFEM_ERR_ARG;
    bool gamg = false;
    PFEM_TRY(mcg_needs(s, pc, "pfem_multi_bench", &gamg));
    PFEM_TRY(use_device(s));
    const int64_t n = s->n_loc;
    std::vector<double> b(static_cast<size_t>(n)), B(static_cast<size_t>(n) * nrhs), X(B.size()), rn(static_cast<size_t>(nrhs));
    std::vector<int> why(static_cast<size_t>(nrhs));
    PFEM_TRY(download_external(s, s->d_rhs.p, b.data(), n));
    for (int j = 0; j < nrhs; ++j)
        for (int64_t i = 0; i < n; ++i) B[static_cast<size_t>(j) * n + i] = b[static_cast<size_t>(i)] * (j + 1);
    for (int r = 0; r < reps; ++r) PFEM_TRY(mcg_run(s, nrhs, B.data(), gamg, X.data(), its, why.data(), rn.data(), ms + r));
    return PFEM_OK;
}

// ---- one launch of a kernel of the multi solve on panels of the caller's (pfem_amd_diag.h) -------------------------------------
namespace {

static_assert(sizeof(pfem_mcg_ctl) == sizeof(McgCtl) && offsetof(pfem_mcg_ctl, flag) == offsetof(McgCtl, flag) &&
                  offsetof(pfem_mcg_ctl, step) == offsetof(McgCtl, step),
              "pfem_mcg_ctl is McgCtl as a plain struct");

bool mcg_probe_args(const pfem_solver *s, int mb, int64_t n) { return s && n >= 1 && (mb == 4 || mb == 8); }

int mcg_ctl_up(pfem_solver *s, DevBuf<McgCtl> &d, const pfem_mcg_ctl *ctl)
{
    PFEM_TRY(d.alloc(1));
    PFEM_HIP(hipMemcpyAsync(d.p, ctl, sizeof(McgCtl), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}
int mcg_ctl_down(pfem_solver *s, const DevBuf<McgCtl> &d, pfem_mcg_ctl *ctl)
{
    PFEM_HIP(hipMemcpyAsync(ctl, d.p, sizeof(McgCtl), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}
// the partials of a vector kernel: the whole capacity goes up as NaN, the first gv rows of 2 mb come back
int mcg_part_down(pfem_solver *s, const ProbeBlock &bp, unsigned gv, int mb, double *part_out, const char *who)
{
    std::vector<double> h(bp.len);
    PFEM_TRY(probe_download(s, bp, h.data(), who));
    std::memcpy(part_out, h.data(), sizeof(double) * gv * 2 * mb);
    return PFEM_OK;
}

}  // namespace

extern "C" int pfem_multi_probe_init(pfem_solver *s, int mb, int64_t n, const double *B, const double *dinv, double *X_out, double *R_out, double *P_out,
                                     double *part_out, int *gv_out)
{
    if (!mcg_probe_args(s, mb, n) || !B || !X_out || !R_out || !P_out || !part_out || !gv_out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_probe_init";
    const size_t rows = static_cast<size_t>(n), tile = kBlock;
    ProbeBlock bb, bd, bx, br, bp, bpart;
    PFEM_TRY(probe_upload(s, bb, "B", B, rows * mb, tile, 0, true));
    if (dinv) PFEM_TRY(probe_upload(s, bd, "dinv", dinv, rows, tile, 0, true));
    PFEM_TRY(probe_upload(s, bx, "X", nullptr, rows * mb, tile));
    PFEM_TRY(probe_upload(s, br, "R", nullptr, rows * mb, tile));
    PFEM_TRY(probe_upload(s, bp, "P", nullptr, rows * mb, tile));
    PFEM_TRY(probe_upload(s, bpart, "part", nullptr, static_cast<size_t>(kMcgVecBlocks) * 2 * mb, tile));
    McgView V;
    V.mb = mb;
    V.n = n;
    V.B = bb.p();
    V.dinv = dinv ? bd.p() : nullptr;
    V.X = bx.p(); V.R = br.p(); V.P = bp.p();
    V.part = bpart.p();
    const unsigned gv = mcg_init(s, V);
    PFEM_TRY(check_kernel("k_mcg_init"));
    PFEM_TRY(probe_download(s, bb, nullptr, who));
    if (dinv) PFEM_TRY(probe_download(s, bd, nullptr, who));
    PFEM_TRY(probe_download(s, bx, X_out, who));
    PFEM_TRY(probe_download(s, br, R_out, who));
    PFEM_TRY(probe_download(s, bp, P_out, who));
    PFEM_TRY(mcg_part_down(s, bpart, gv, mb, part_out, who));
    *gv_out = static_cast<int>(gv);
    return PFEM_OK;
}

extern "C" int pfem_multi_probe_start(pfem_solver *s, int mb, int nparts, const double *part, double rtol, double abstol, pfem_mcg_ctl *ctl)
{
    if (!mcg_probe_args(s, mb, 1) || nparts < 1 || nparts > kMcgVecBlocks || !part || !ctl) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_probe_start";
    ProbeBlock bpart;
    PFEM_TRY(probe_upload(s, bpart, "part", part, static_cast<size_t>(nparts) * 2 * mb, kBlock, 0, true));
    DevBuf<McgCtl> d;
    PFEM_TRY(mcg_ctl_up(s, d, ctl));
    McgView V;
    V.mb = mb;
    V.part = bpart.p();
    V.ctl = d.p;
    mcg_start(s, V, static_cast<unsigned>(nparts), rtol, abstol);
    PFEM_TRY(check_kernel("k_mcg_start"));
    PFEM_TRY(probe_download(s, bpart, nullptr, who));
    return mcg_ctl_down(s, d, ctl);
}

extern "C" int pfem_multi_probe_fold(pfem_solver *s, int mb, int nb, const double *part_pw, double *fold_out)
{
    if (!mcg_probe_args(s, mb, 1) || nb < 1 || !part_pw || !fold_out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_probe_fold";
    ProbeBlock bpw, bf;
    PFEM_TRY(probe_upload(s, bpw, "part_pw", part_pw, static_cast<size_t>(nb) * mb, kBlock, 0, true));
    PFEM_TRY(probe_upload(s, bf, "fold_pw", nullptr, static_cast<size_t>(kFoldBlocks) * mb, kBlock));
    with_mcg_mb(mb, [&](auto MB) {
        launch(k_mcg_fold<decltype(MB)::value>, dim3(kFoldBlocks), dim3(kBlock), 0, s->stream, nullptr, nullptr, static_cast<const McgCtl *>(nullptr), bpw.p(), nb,
               bf.p());
    });
    PFEM_TRY(check_kernel("k_mcg_fold"));
    PFEM_TRY(probe_download(s, bpw, nullptr, who));
    return probe_download(s, bf, fold_out, who);
}

extern "C" int pfem_multi_probe_update(pfem_solver *s, int mb, int64_t n, pfem_mcg_ctl *ctl, const double *fold_pw, const double *W, const double *dinv,
                                       double *R, double *part_out, int *gv_out)
{
    if (!mcg_probe_args(s, mb, n) || !ctl || !fold_pw || !W || !R || !part_out || !gv_out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_probe_update";
    const size_t rows = static_cast<size_t>(n), tile = kBlock;
    ProbeBlock bf, bw, bd, br, bpart;
    PFEM_TRY(probe_upload(s, bf, "fold_pw", fold_pw, static_cast<size_t>(kFoldBlocks) * mb, tile, 0, true));
    PFEM_TRY(probe_upload(s, bw, "W", W, rows * mb, tile, 0, true));
    if (dinv) PFEM_TRY(probe_upload(s, bd, "dinv", dinv, rows, tile, 0, true));
    PFEM_TRY(probe_upload(s, br, "R", R, rows * mb, tile));
    PFEM_TRY(probe_upload(s, bpart, "part", nullptr, static_cast<size_t>(kMcgVecBlocks) * 2 * mb, tile));
    DevBuf<McgCtl> d;
    PFEM_TRY(mcg_ctl_up(s, d, ctl));
    McgView V;
    V.mb = mb;
    V.n = n;
    V.fold_pw = bf.p();
    V.W = bw.p();
    V.dinv = dinv ? bd.p() : nullptr;
    V.R = br.p();
    V.part = bpart.p();
    V.ctl = d.p;
    const unsigned gv = mcg_update(s, V);
    PFEM_TRY(check_kernel("k_mcg_update"));
    PFEM_TRY(probe_download(s, bf, nullptr, who));
    PFEM_TRY(probe_download(s, bw, nullptr, who));
    if (dinv) PFEM_TRY(probe_download(s, bd, nullptr, who));
    PFEM_TRY(probe_download(s, br, R, who));
    PFEM_TRY(mcg_part_down(s, bpart, gv, mb, part_out, who));
    *gv_out = static_cast<int>(gv);
    return mcg_ctl_down(s, d, ctl);
}

extern "C" int pfem_multi_probe_dots(pfem_solver *s, int mb, int64_t n, const pfem_mcg_ctl *ctl, const double *fold_pw, const double *R, const double *Z,
                                     double *part_out, int *gv_out)
{
    if (!mcg_probe_args(s, mb, n) || !R || !Z || !part_out || !gv_out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_probe_dots";
    const size_t rows = static_cast<size_t>(n), tile = kBlock;
    ProbeBlock bf, br, bz, bpart;
    if (fold_pw) PFEM_TRY(probe_upload(s, bf, "fold_pw", fold_pw, static_cast<size_t>(kFoldBlocks) * mb, tile, 0, true));
    PFEM_TRY(probe_upload(s, br, "R", R, rows * mb, tile, 0, true));
    PFEM_TRY(probe_upload(s, bz, "Z", Z, rows * mb, tile, 0, true));
    PFEM_TRY(probe_upload(s, bpart, "part", nullptr, static_cast<size_t>(kMcgVecBlocks) * 2 * mb, tile));
    DevBuf<McgCtl> d;
    if (ctl) PFEM_TRY(mcg_ctl_up(s, d, ctl));
    McgView V;
    V.mb = mb;
    V.n = n;
    V.R = br.p(); V.Z = bz.p();
    V.part = bpart.p();
    const unsigned gv = mcg_dots(s, V, ctl ? d.p : nullptr, fold_pw ? bf.p() : nullptr);
    PFEM_TRY(check_kernel("k_mcg_dots"));
    if (fold_pw) PFEM_TRY(probe_download(s, bf, nullptr, who));
    PFEM_TRY(probe_download(s, br, nullptr, who));
    PFEM_TRY(probe_download(s, bz, nullptr, who));
    PFEM_TRY(mcg_part_down(s, bpart, gv, mb, part_out, who));
    *gv_out = static_cast<int>(gv);
    return PFEM_OK;
}

extern "C" int pfem_multi_probe_verdict(pfem_solver *s, int mb, pfem_mcg_ctl *ctl, int nparts, const double *part, double dtol, int maxits)
{
    if (!mcg_probe_args(s, mb, 1) || nparts < 1 || nparts > kMcgVecBlocks || !part || !ctl) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_probe_verdict";
    ProbeBlock bpart;
    PFEM_TRY(probe_upload(s, bpart, "part", part, static_cast<size_t>(nparts) * 2 * mb, kBlock, 0, true));
    DevBuf<McgCtl> d;
    PFEM_TRY(mcg_ctl_up(s, d, ctl));
    McgView V;
    V.mb = mb;
    V.part = bpart.p();
    V.ctl = d.p;
    mcg_verdict(s, V, static_cast<unsigned>(nparts), dtol, maxits);
    PFEM_TRY(check_kernel("k_mcg_verdict"));
    PFEM_TRY(probe_download(s, bpart, nullptr, who));
    return mcg_ctl_down(s, d, ctl);
}

extern "C" int pfem_multi_probe_direction(pfem_solver *s, int mb, int64_t n, pfem_mcg_ctl *ctl, const double *R, const double *dinv, const double *Z, double *P,
                                          double *X)
{
    if (!mcg_probe_args(s, mb, n) || !ctl || !R || (!dinv && !Z) || !P || !X) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_probe_direction";
    const size_t rows = static_cast<size_t>(n), tile = kBlock;
    ProbeBlock br, bd, bz, bp, bx;
    PFEM_TRY(probe_upload(s, br, "R", R, rows * mb, tile, 0, true));
    if (dinv) PFEM_TRY(probe_upload(s, bd, "dinv", dinv, rows, tile, 0, true));
    else PFEM_TRY(probe_upload(s, bz, "Z", Z, rows * mb, tile, 0, true));
    PFEM_TRY(probe_upload(s, bp, "P", P, rows * mb, tile));
    PFEM_TRY(probe_upload(s, bx, "X", X, rows * mb, tile));
    DevBuf<McgCtl> d;
    PFEM_TRY(mcg_ctl_up(s, d, ctl));
    McgView V;
    V.mb = mb;
    V.n = n;
    V.R = br.p();
    V.dinv = dinv ? bd.p() : nullptr;
    V.Z = dinv ? nullptr : bz.p();
    V.P = bp.p(); V.X = bx.p();
    V.ctl = d.p;
    mcg_direction(s, V);
    PFEM_TRY(check_kernel("k_mcg_direction"));
    PFEM_TRY(probe_download(s, br, nullptr, who));
    if (dinv) PFEM_TRY(probe_download(s, bd, nullptr, who));
    else PFEM_TRY(probe_download(s, bz, nullptr, who));
    PFEM_TRY(probe_download(s, bp, P, who));
    PFEM_TRY(probe_download(s, bx, X, who));
    return mcg_ctl_down(s, d, ctl);
}

// W = K P by k_spmm_dot<mb> and the folded (p, Kp) per column for a host panel of n_local x mb doubles, row-major, in the caller's
// dof order, on the handle's assembled matrix (pfem_amd_diag.h)
extern "C" int pfem_multi_spmm_dot(pfem_solver *s, int mb, const double *P, double *W_out, double *pw_out)
{
    if (!s || !P || !W_out || !pw_out || (mb != 4 && mb != 8)) return PFEM_ERR_ARG;
    PFEM_TRY(needs_one_rank(s, "pfem_multi_spmm_dot"));
    if (!s->have_pattern || s->status < PFEM_ASSEMBLY_OK || s->host_values_dirty) return PFEM_ERR_STATE;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_multi_spmm_dot";
    const int64_t n = s->n_loc;
    const size_t len = static_cast<size_t>(std::max<int64_t>(n, 1)) * mb;
    std::vector<double> h(len, 0.0);
    for (int64_t i = 0; i < n; ++i) std::memcpy(&h[static_cast<size_t>(to_internal(s, i)) * mb], P + i * mb, sizeof(double) * mb);
    ProbeBlock bp, bw, bpw, bf;
    PFEM_TRY(probe_upload(s, bp, "P", h.data(), len, kBlock, 0, true));
    PFEM_TRY(probe_upload(s, bw, "W", nullptr, len, kBlock));
    PFEM_TRY(probe_upload(s, bpw, "part_pw", nullptr, static_cast<size_t>(grid_for(n)) * mb, kBlock));
    PFEM_TRY(probe_upload(s, bf, "fold_pw", nullptr, static_cast<size_t>(kFoldBlocks) * mb, kBlock));
    McgView V;
    V.mb = mb;
    V.n = n;
    V.P = bp.p(); V.W = bw.p();
    V.part_pw = bpw.p(); V.fold_pw = bf.p();
    mcg_product(s, V, s->sell(), nullptr);
    PFEM_TRY(check_kernel("k_spmm_dot"));
    PFEM_TRY(probe_download(s, bp, nullptr, who));
    PFEM_TRY(probe_download(s, bw, h.data(), who));
    PFEM_TRY(probe_download(s, bpw, nullptr, who));
    std::vector<double> f(static_cast<size_t>(kFoldBlocks) * mb);
    PFEM_TRY(probe_download(s, bf, f.data(), who));
    for (int64_t i = 0; i < n; ++i) std::memcpy(W_out + i * mb, &h[static_cast<size_t>(to_internal(s, i)) * mb], sizeof(double) * mb);
    for (int j = 0; j < mb; ++j) {         // in index order, as k_mcg_update re-sums them
        double a = 0.0;
        for (int b = 0; b < kFoldBlocks; ++b) a += f[static_cast<size_t>(b) * mb + j];
        pw_out[j] = a;
    }
    return PFEM_OK;
}

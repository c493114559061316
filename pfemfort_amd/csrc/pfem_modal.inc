// pfem_modal.inc -- modal analysis on an assembled system (pfem_modal_solve; DESIGN.md section 13): the lowest eigenpairs of
// (K, diag(m)) by LOBPCG on blocks of MB vectors.  Included once by pfem_device.hip after pfem_implicit.inc.  A path beside the
// solve and the steppers: it reads the matrix in its row form (s->sell(), current after every assemble), the lumped mass and the
// diagonal, and writes only the buffers of Modal -- not the solution or the right-hand side, last_its / last_reason /
// last_rnorm, the history, the timings, the CG graphs, the state of Dyn or Imp.  One stream, plain launches, no graph; the
// Rayleigh-Ritz step runs on the host (pfem_dense_sym_geneig) between one device -> host and one host -> device copy, both
// through the pinned buffers of Modal.  With gamg in effect and its numeric set-up current the preconditioner is the cycle of
// the last gamg solve (amg_apply as it stands, a column at a time); then the cycle's work vectors are written as well.

namespace {

constexpr int kModalRefresh = 10;          // every 10th iteration K X is a product, not the recurrence
constexpr double kModalFloor = 1e-12;      // smallest squared pivot of the scaled mass Gram matrix before P is dropped

int modal_block(int n_modes, int block, int *mb)
{
    if (n_modes < 1 || n_modes > PFEM_MODAL_MAX_MODES) return PFEM_ERR_ARG;
    const int pick = n_modes <= 2 ? 4 : (n_modes <= 6 ? 8 : 16);
    if (block != 0 && block != 4 && block != 8 && block != 16) return PFEM_ERR_ARG;
    if (block != 0 && block < pick) return PFEM_ERR_ARG;
    *mb = std::max(pick, block);
    return PFEM_OK;
}

template <class F>
void with_mb(int mb, F &&f)
{
    if (mb == 4) f(std::integral_constant<int, 4>{});
    else if (mb == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

unsigned modal_vec_grid(int64_t entries) { return static_cast<unsigned>(std::min<int64_t>(kModalVecBlocks, std::max<int64_t>(1, (entries + kBlock - 1) / kBlock))); }
unsigned modal_gram_grid(int64_t n) { return static_cast<unsigned>(std::min<int64_t>(kModalGramBlocks, std::max<int64_t>(1, (n + kModalGramTile - 1) / kModalGramTile))); }
unsigned modal_update_grid(int64_t n, int mb)
{
    const int64_t tr = kBlock / mb;
    return static_cast<unsigned>(std::min<int64_t>(kModalVecBlocks, std::max<int64_t>(1, (n + tr - 1) / tr)));
}

// What one launch of the Gram, residual and update kernels reads and writes: the six blocks of n rows x mb columns, the mass and
// the inverse diagonal by row, the coefficient block, the partials and the summed output on the device and its host copy.  The
// solve fills it from the buffers of Modal (modal_view), a probe (pfem_modal_probe_*) from blocks of its own: both launch
// through the three functions below.
struct ModalView {
    int mb = 0;
    int64_t n = 0;
    double *X = nullptr, *W = nullptr, *P = nullptr, *KX = nullptr, *KW = nullptr, *KP = nullptr;
    const double *m = nullptr, *dinv = nullptr;
    double *vec = nullptr;                 // n doubles: a column of W on its way through gamg's cycle
    double *coef = nullptr, *part_gram = nullptr, *part_res = nullptr, *out = nullptr;
    double *h_out = nullptr;               // modal_out_len(mb) doubles on the host
};

ModalView modal_view(const pfem_solver *s, Modal &M)
{
    ModalView V;
    V.mb = M.mb;
    V.n = M.n;
    V.X = M.X.p; V.W = M.W.p; V.P = M.P.p; V.KX = M.KX.p; V.KW = M.KW.p; V.KP = M.KP.p;
    V.m = s->dyn->d_m.p;
    V.dinv = M.dinv.p;
    V.vec = M.vec.p;
    V.coef = M.coef.p; V.part_gram = M.part_gram.p; V.part_res = M.part_res.p; V.out = M.out.p;
    V.h_out = M.h_out;
    return V;
}

// the run's own buffers for blocks of mb columns
int modal_ensure(pfem_solver *s, int mb)
{
    Dyn &D = *s->dyn;
    if (D.modal && D.modal->mb == mb && D.modal->n == D.n) return PFEM_OK;
    D.modal.reset();
    auto M = std::make_unique<Modal>();
    M->mb = mb;
    M->n = D.n;
    const size_t len = static_cast<size_t>(std::max<int64_t>(D.n, 1)) * static_cast<size_t>(mb);
    for (DevBuf<double> *g : {&M->X, &M->W, &M->P, &M->KX, &M->KW, &M->KP}) PFEM_TRY(g->alloc(len));
    PFEM_TRY(M->dinv.alloc(static_cast<size_t>(std::max<int64_t>(D.n, 1))));
    PFEM_TRY(M->vec.alloc(static_cast<size_t>(std::max<int64_t>(D.n, 1))));
    PFEM_TRY(M->part_gram.alloc(static_cast<size_t>(kModalGramBlocks) * modal_gram_len(mb)));
    PFEM_TRY(M->part_res.alloc(static_cast<size_t>(kModalVecBlocks) * 3 * mb));
    PFEM_TRY(M->out.alloc(static_cast<size_t>(modal_out_len(mb))));
    PFEM_TRY(M->coef.alloc(static_cast<size_t>(modal_coef_len(mb))));
    if (hipHostMalloc(reinterpret_cast<void **>(&M->h_out), sizeof(double) * modal_out_len(mb)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&M->h_coef), sizeof(double) * modal_coef_len(mb)) != hipSuccess) {
        (void)hipGetLastError();
        set_last_error("pfem_modal_solve: no pinned host memory for the per-iteration copies");
        return PFEM_ERR_NOMEM;
    }
    D.modal = std::move(M);
    return PFEM_OK;
}

void modal_spmm(pfem_solver *s, int mb, const double *X, double *Y)
{
    with_mb(mb, [&](auto MB) {
        launch(k_spmm<decltype(MB)::value>, dim3(grid_for(s->n_loc)), dim3(kBlock), 0, s->stream, nullptr, nullptr, s->sell(), X, Y);
    });
}

// the Gram pass over the six blocks and the sums of its partials and (with_res) of the residual kernel's; then the copy to the
// host buffer and the wait for it
int modal_gram_to_host(pfem_solver *s, const ModalView &V, bool with_gram, unsigned res_blocks)
{
    const int mb = V.mb, n_gram = modal_gram_len(mb), n_res = 3 * mb;
    const unsigned gg = modal_gram_grid(V.n);
    if (with_gram)
        with_mb(mb, [&](auto MB) {
            launch(k_modal_gram<decltype(MB)::value>, dim3(gg), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.X, V.W, V.P, V.KX, V.KW, V.KP, V.m, V.part_gram);
        });
    launch(k_modal_sum, dim3(grid_for(n_gram + n_res)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n_gram, with_gram ? static_cast<int>(gg) : 0, V.part_gram,
           n_res, static_cast<int>(res_blocks), V.part_res, V.out);
    PFEM_TRY(check_kernel("k_modal_gram"));
    PFEM_HIP(hipMemcpyAsync(V.h_out, V.out, sizeof(double) * modal_out_len(mb), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

// W <- the cycle of the last gamg solve on every column of W in turn: amg_apply as it stands, through the contiguous vector V.vec
// and the cycle's own output vector (pfem_modal_solve, pfem_buckling_solve).  false: the cycle failed.
bool modal_cycle_columns(pfem_solver *s, const ModalView &V)
{
    Amg &A = *s->amg;
    const int tail_build = A.tail_build;
    for (int j = 0; j < V.mb; ++j) {
        with_mb(V.mb, [&](auto MB) {
            launch(k_modal_pack<decltype(MB)::value>, dim3(grid_for(V.n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.W, j, V.vec);
        });
        const double *z = amg_apply(s, A, V.vec, nullptr);
        if (!z) return false;
        with_mb(V.mb, [&](auto MB) {
            launch(k_modal_unpack<decltype(MB)::value>, dim3(grid_for(V.n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, z, j, V.W);
        });
    }
    A.tail_build = tail_build;             // (what the last SOLVE's cycle launched, pfem_solver_amg_tail_from)
    return true;
}

// R, the norms' partials and W = T R: the point Jacobi inside the residual kernel, or (gamg) the cycle of the last gamg solve on
// every column in turn -- amg_apply as it stands, through the contiguous vector V.vec and the cycle's own output vector
unsigned modal_residual(pfem_solver *s, const ModalView &V, bool gamg)
{
    const unsigned gr = modal_vec_grid(V.n * V.mb);
    with_mb(V.mb, [&](auto MB) {
        launch(k_modal_residual<decltype(MB)::value>, dim3(gr), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.KX, V.X, V.m, gamg ? nullptr : V.dinv,
               V.coef + 3 * V.mb * V.mb, V.W, V.part_res);
    });
    if (gamg && !modal_cycle_columns(s, V)) return 0;
    return gr;
}

// gamg's cycle can stand for T: one rank's own hierarchy whose numeric set-up was made for the values now assembled
bool modal_gamg_current(const pfem_solver *s)
{
    const Amg *A = s->amg.get();
    return A && A->symbolic_ok && !A->coupled && !A->rep && A->numeric_epoch == s->values_epoch && !A->lev.empty() && A->lev[0]->x && A->lev[0]->lam.p &&
           A->lev[0]->dinv.p;
}

// Rayleigh-Ritz on the leading ns x ns blocks of the Gram matrices in h_out: theta and the coefficients into h_coef (rows of C
// beyond ns zero).  *singular as pfem_dense_sym_geneig's status.
int modal_rayleigh_ritz(Modal &M, int ns, int *singular)
{
    const int mb = M.mb, NS = 3 * mb;
    double A[PFEM_GENEIG_MAX * PFEM_GENEIG_MAX], B[PFEM_GENEIG_MAX * PFEM_GENEIG_MAX], w[PFEM_GENEIG_MAX], C[PFEM_GENEIG_MAX * PFEM_GENEIG_MAX];
    const double *gk = M.h_out, *gm = M.h_out + NS * NS;
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b < ns; ++b) {     // (the upper triangles are what the device wrote and what the routine reads)
            A[a * ns + b] = gk[a * NS + b];
            B[a * ns + b] = gm[a * NS + b];
        }
    PFEM_TRY(pfem_dense_sym_geneig(ns, A, B, kModalFloor, w, C, singular));
    if (*singular) return PFEM_OK;
    for (int k = 0; k < NS; ++k)
        for (int j = 0; j < mb; ++j) M.h_coef[k * mb + j] = k < ns ? C[k * ns + j] : 0.0;
    for (int j = 0; j < mb; ++j) M.h_coef[NS * mb + j] = w[j];
    return PFEM_OK;
}

// h_coef (modal_coef_len(mb) doubles on the host: C, then theta) to the device, then the update of the six blocks in place
int modal_update(pfem_solver *s, const ModalView &V, const double *h_coef)
{
    PFEM_HIP(hipMemcpyAsync(V.coef, h_coef, sizeof(double) * modal_coef_len(V.mb), hipMemcpyHostToDevice, s->stream));
    with_mb(V.mb, [&](auto MB) {
        launch(k_modal_update<decltype(MB)::value>, dim3(modal_update_grid(V.n, V.mb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.coef, V.X, V.W, V.P,
               V.KX, V.KW, V.KP);
    });
    return check_kernel("k_modal_update");
}

// res_j from the three norms^2 of column j in h_out
double modal_res(const Modal &M, int j, double theta)
{
    const double *nr = M.h_out + modal_gram_len(M.mb);
    const double r = std::sqrt(nr[j]), den = std::sqrt(nr[M.mb + j]) + std::fabs(theta) * std::sqrt(nr[2 * M.mb + j]);
    return r == 0.0 ? 0.0 : r / den;
}

// caller's rows (n_owned x mb, row-major) -> the device block in the internal order
int modal_upload_block(pfem_solver *s, int mb, const double *in, double *d_block)
{
    const int64_t n = s->n_owned;
    std::vector<double> tmp;
    if (s->reordered) {
        tmp.resize(static_cast<size_t>(n) * mb);
        for (int64_t i = 0; i < n; ++i) std::memcpy(&tmp[static_cast<size_t>(to_internal(s, i)) * mb], in + i * mb, sizeof(double) * mb);
    }
    PFEM_HIP(hipMemcpyAsync(d_block, tmp.empty() ? in : tmp.data(), sizeof(double) * static_cast<size_t>(n) * mb, hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));       // (tmp goes out of scope)
    return PFEM_OK;
}

}  // namespace

extern "C" int pfem_modal_solve(pfem_solver *s, int n_modes, int block, double tol, int max_iterations, int pc, const double *x0, double *omega2, double *modes,
                                double *residuals, int *iterations, int *restarts, int *reason)
{
    if (iterations) *iterations = 0;
    if (restarts) *restarts = 0;
    if (reason) *reason = 0;
    if (!s || !omega2 || !residuals || !iterations || !restarts || !reason) return PFEM_ERR_ARG;
    int mb = 0;
    PFEM_TRY(modal_block(n_modes, block, &mb));
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iterations < 1) return PFEM_ERR_ARG;
    if (pc != -1 && pc != PFEM_PC_JACOBI && pc != PFEM_PC_NODE_BLOCK_JACOBI && pc != PFEM_PC_GAMG) return PFEM_ERR_ARG;
    if (mb > s->n_owned) return PFEM_ERR_ARG;
    PFEM_TRY(imp_needs(s, "pfem_modal_solve"));
    // T: the cycle of the last gamg solve when gamg is the preconditioner in effect (or asked for) and its numeric set-up is
    // current -- a solve has run since the last assemble -- else the point Jacobi.  Asked for by name and not current: an error.
    const bool want_gamg = pc == PFEM_PC_GAMG || (pc == -1 && s->pc == PFEM_PC_GAMG);
    const bool gamg = want_gamg && modal_gamg_current(s);
    if (pc == PFEM_PC_GAMG && !gamg) {
        set_last_error("pfem_modal_solve: pc = gamg needs a gamg solve since the last assemble (its numeric set-up is the T)");
        return PFEM_ERR_STATE;
    }
    PFEM_TRY(use_device(s));
    Dyn &D = *s->dyn;
    const int64_t n = D.n;
    // the mass on the host, in the caller's order: every entry positive; the normalisation at the end reads it again
    std::vector<double> h_m(static_cast<size_t>(n));
    PFEM_TRY(download_external(s, D.d_m.p, h_m.data(), n));
    for (double v : h_m)
        if (!(v > 0.0) || !std::isfinite(v)) {
            set_last_error("pfem_modal_solve: a dof without mass (every m_i must be positive)");
            return PFEM_ERR_STATE;
        }
    PFEM_TRY(modal_ensure(s, mb));
    Modal &M = *D.modal;
    const ModalView V = modal_view(s, M);
    M.pc_used = gamg ? PFEM_PC_GAMG : PFEM_PC_JACOBI;
    if (gamg) {                            // the cycle's fine-level products run in the SpMV form in effect: its copies of the values
        mark_group_vals(s);
        PFEM_TRY(refresh_group_vals(s));
    }
    const int NS = 3 * mb;
    const size_t block_bytes = sizeof(double) * static_cast<size_t>(n) * mb;
    // T = 1 / K_ii from the row form, in the run's own buffer
    launch(k_extract_diag, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, s->sell(), M.dinv.p);
    launch(k_modal_invert, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, M.dinv.p);
    PFEM_TRY(check_kernel("k_modal_invert"));
    // the start: X0, zero W and P and their products, K X0, one Rayleigh-Ritz on X0 alone
    if (x0) {
        PFEM_TRY(modal_upload_block(s, mb, x0, M.X.p));
    } else {
        with_mb(mb, [&](auto MB) {
            launch(k_modal_init<decltype(MB)::value>, dim3(grid_for(n * mb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, s->row_start,
                   s->reordered ? static_cast<const int32_t *>(s->d_perm.p) : nullptr, M.X.p);
        });
    }
    for (DevBuf<double> *g : {&M.W, &M.P, &M.KW, &M.KP}) PFEM_HIP(hipMemsetAsync(g->p, 0, block_bytes, s->stream));
    PFEM_HIP(hipMemsetAsync(M.out.p, 0, sizeof(double) * modal_out_len(mb), s->stream));
    modal_spmm(s, mb, M.X.p, M.KX.p);
    PFEM_TRY(modal_gram_to_host(s, V, true, 0));
    double theta[16];
    int its = 0, n_restarts = 0, why = 0, singular = 0;
    bool have_p = false;
    PFEM_TRY(modal_rayleigh_ritz(M, mb, &singular));
    if (singular) {                        // the start block is rank-deficient: its Rayleigh quotients are all there is
        why = -2;
        for (int j = 0; j < mb; ++j) theta[j] = M.h_out[j * NS + j] / M.h_out[NS * NS + j * NS + j];
        for (int k = 0; k < NS * mb; ++k) M.h_coef[k] = (k / mb == k % mb) ? 1.0 : 0.0;
        for (int j = 0; j < mb; ++j) M.h_coef[NS * mb + j] = theta[j];
    } else {
        for (int j = 0; j < mb; ++j) theta[j] = M.h_coef[NS * mb + j];
    }
    PFEM_TRY(modal_update(s, V, M.h_coef));
    while (why == 0) {
        // R, W = T R and the norms; K W; the Gram matrices of [X W P]; one copy back
        const unsigned gr = modal_residual(s, V, gamg);
        if (gr == 0) return PFEM_ERR_HIP;
        modal_spmm(s, mb, M.W.p, M.KW.p);
        PFEM_TRY(modal_gram_to_host(s, V, true, gr));
        bool done = true;
        for (int j = 0; j < n_modes; ++j) done = done && modal_res(M, j, theta[j]) <= tol;
        if (done) { why = 1; break; }
        if (its >= max_iterations) { why = -1; break; }
        ++its;
        PFEM_TRY(modal_rayleigh_ritz(M, have_p ? NS : 2 * mb, &singular));
        if (singular && have_p) {          // drop P for this iteration: a restart
            ++n_restarts;
            PFEM_TRY(modal_rayleigh_ritz(M, 2 * mb, &singular));
        }
        if (singular) { why = -2; break; }
        for (int j = 0; j < mb; ++j) theta[j] = M.h_coef[NS * mb + j];
        PFEM_TRY(modal_update(s, V, M.h_coef));
        have_p = true;
        if (its % kModalRefresh == 0) modal_spmm(s, mb, M.X.p, M.KX.p);
    }
    // the end: residuals from an explicit K X (theta is ascending as the Rayleigh-Ritz step left it)
    modal_spmm(s, mb, M.X.p, M.KX.p);
    const unsigned gr = modal_residual(s, V, false);
    PFEM_TRY(modal_gram_to_host(s, V, false, gr));
    for (int j = 0; j < n_modes; ++j) {
        omega2[j] = theta[j];
        residuals[j] = modal_res(M, j, theta[j]);
    }
    *iterations = its;
    *restarts = n_restarts;
    *reason = why;
    if (modes) {
        // phi^T M phi = 1, the entry of largest magnitude positive (the lowest index on ties): on the host, in the caller's order
        std::vector<double> h_x(static_cast<size_t>(n) * mb);
        PFEM_HIP(hipMemcpyAsync(h_x.data(), M.X.p, block_bytes, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        for (int j = 0; j < n_modes; ++j) {
            double *out = modes + static_cast<int64_t>(j) * n;
            double mass = 0.0, big = -1.0;
            bool negative = false;
            for (int64_t l = 0; l < n; ++l) {
                const double v = h_x[static_cast<size_t>(to_internal(s, l)) * mb + j];
                out[l] = v;
                mass += h_m[static_cast<size_t>(l)] * (v * v);
                if (std::fabs(v) > big) { big = std::fabs(v); negative = v < 0.0; }
            }
            const double scale = (negative ? -1.0 : 1.0) / std::sqrt(mass);
            for (int64_t l = 0; l < n; ++l) out[l] *= scale;
        }
    }
    return PFEM_OK;
}

// the T of the last pfem_modal_solve on this handle: PFEM_PC_JACOBI or PFEM_PC_GAMG (pfem_amd_diag.h)
extern "C" int pfem_modal_last_pc(pfem_solver *s, int *pc)
{
    if (!s || !pc) return PFEM_ERR_ARG;
    if (!s->dyn || !s->dyn->modal) return PFEM_ERR_STATE;
    *pc = s->dyn->modal->pc_used;
    return PFEM_OK;
}

// Y = K X by k_spmm<mb> for host blocks of n_local x mb doubles, row-major, in the caller's dof order (pfem_amd_diag.h)
extern "C" int pfem_modal_spmm(pfem_solver *s, int mb, const double *x, double *y)
{
    if (!s || !x || !y || (mb != 4 && mb != 8 && mb != 16)) return PFEM_ERR_ARG;
    PFEM_TRY(needs_one_rank(s, "pfem_modal_spmm"));
    if (!s->have_pattern || s->status < PFEM_ASSEMBLY_OK) return PFEM_ERR_STATE;
    PFEM_TRY(use_device(s));
    const int64_t n = s->n_loc;
    const size_t len = static_cast<size_t>(std::max<int64_t>(n, 1)) * mb;
    DevBuf<double> dx, dy;
    PFEM_TRY(dx.alloc(len));
    PFEM_TRY(dy.alloc(len));
    PFEM_TRY(modal_upload_block(s, mb, x, dx.p));
    modal_spmm(s, mb, dx.p, dy.p);
    PFEM_TRY(check_kernel("k_spmm"));
    std::vector<double> h(len);
    PFEM_HIP(hipMemcpyAsync(h.data(), dy.p, sizeof(double) * len, hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    for (int64_t i = 0; i < n; ++i) std::memcpy(y + i * mb, &h[static_cast<size_t>(to_internal(s, i)) * mb], sizeof(double) * mb);
    return PFEM_OK;
}

// ---- one launch of a modal kernel on blocks of the caller's (pfem_amd_diag.h) ---------------------------------------------------
namespace {

// (ProbeBlock, probe_upload and probe_download: pfem_probe.inc)
bool probe_args(const pfem_solver *s, int mb, int64_t n) { return s && n >= 1 && (mb == 4 || mb == 8 || mb == 16); }

}  // namespace

// k_modal_gram<mb> on modal_gram_grid(n) blocks, then k_modal_sum: out = the 2 NS NS doubles of h_out (pfem_amd_diag.h)
extern "C" int pfem_modal_probe_gram(pfem_solver *s, int mb, int64_t n, const double *X, const double *W, const double *P, const double *KX, const double *KW,
                                     const double *KP, const double *m, double *out)
{
    if (!probe_args(s, mb, n) || !X || !W || !P || !KX || !KW || !KP || !m || !out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_modal_probe_gram";
    const size_t rows = static_cast<size_t>(n), tile = kModalGramTile;
    ProbeBlock B[6], bm;
    const double *in[6] = {X, W, P, KX, KW, KP};
    const char *names[6] = {"X", "W", "P", "KX", "KW", "KP"};
    for (int k = 0; k < 6; ++k) PFEM_TRY(probe_upload(s, B[k], names[k], in[k], rows * mb, tile * mb));
    PFEM_TRY(probe_upload(s, bm, "m", m, rows, tile));
    DevBuf<double> part_gram, part_res, d_out;
    PFEM_TRY(part_gram.alloc(static_cast<size_t>(kModalGramBlocks) * modal_gram_len(mb)));
    PFEM_TRY(part_res.alloc(1));
    PFEM_TRY(d_out.alloc(static_cast<size_t>(modal_out_len(mb))));
    PFEM_HIP(hipMemsetAsync(d_out.p, 0, sizeof(double) * modal_out_len(mb), s->stream));
    std::vector<double> h_out(static_cast<size_t>(modal_out_len(mb)));
    ModalView V;
    V.mb = mb;
    V.n = n;
    V.X = B[0].d.p; V.W = B[1].d.p; V.P = B[2].d.p; V.KX = B[3].d.p; V.KW = B[4].d.p; V.KP = B[5].d.p;
    V.m = bm.d.p;
    V.part_gram = part_gram.p; V.part_res = part_res.p; V.out = d_out.p;
    V.h_out = h_out.data();
    PFEM_TRY(modal_gram_to_host(s, V, true, 0));
    for (int k = 0; k < 6; ++k) PFEM_TRY(probe_download(s, B[k], nullptr, who));
    PFEM_TRY(probe_download(s, bm, nullptr, who));
    std::memcpy(out, h_out.data(), sizeof(double) * modal_gram_len(mb));
    return PFEM_OK;
}

// k_modal_residual<mb> on modal_vec_grid(n mb) blocks, then k_modal_sum: W and the 3 mb norms^2 (pfem_amd_diag.h)
extern "C" int pfem_modal_probe_residual(pfem_solver *s, int mb, int64_t n, const double *KX, const double *X, const double *m, const double *dinv,
                                         const double *theta, double *W_out, double *norms_out)
{
    if (!probe_args(s, mb, n) || !KX || !X || !m || !theta || !W_out || !norms_out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_modal_probe_residual";
    const size_t rows = static_cast<size_t>(n), tile = kBlock / mb;
    ProbeBlock bkx, bx, bw, bm, bd;
    PFEM_TRY(probe_upload(s, bkx, "KX", KX, rows * mb, tile * mb));
    PFEM_TRY(probe_upload(s, bx, "X", X, rows * mb, tile * mb));
    PFEM_TRY(probe_upload(s, bw, "W", nullptr, rows * mb, tile * mb));
    PFEM_TRY(probe_upload(s, bm, "m", m, rows, tile));
    if (dinv) PFEM_TRY(probe_upload(s, bd, "dinv", dinv, rows, tile));
    std::vector<double> h_coef(static_cast<size_t>(modal_coef_len(mb)), 0.0), h_out(static_cast<size_t>(modal_out_len(mb)));
    std::memcpy(&h_coef[static_cast<size_t>(3 * mb * mb)], theta, sizeof(double) * mb);
    DevBuf<double> coef, part_gram, part_res, d_out;
    PFEM_TRY(coef.alloc(h_coef.size()));
    PFEM_TRY(part_gram.alloc(1));
    PFEM_TRY(part_res.alloc(static_cast<size_t>(kModalVecBlocks) * 3 * mb));
    PFEM_TRY(d_out.alloc(h_out.size()));
    PFEM_HIP(hipMemcpyAsync(coef.p, h_coef.data(), sizeof(double) * h_coef.size(), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipMemsetAsync(d_out.p, 0, sizeof(double) * h_out.size(), s->stream));
    ModalView V;
    V.mb = mb;
    V.n = n;
    V.KX = bkx.d.p; V.X = bx.d.p; V.W = bw.d.p;
    V.m = bm.d.p;
    V.dinv = dinv ? bd.d.p : nullptr;
    V.coef = coef.p; V.part_gram = part_gram.p; V.part_res = part_res.p; V.out = d_out.p;
    V.h_out = h_out.data();
    const unsigned gr = modal_residual(s, V, false);
    PFEM_TRY(check_kernel("k_modal_residual"));
    PFEM_TRY(modal_gram_to_host(s, V, false, gr));   // (waits for the stream: h_coef has been read)
    PFEM_TRY(probe_download(s, bkx, nullptr, who));
    PFEM_TRY(probe_download(s, bx, nullptr, who));
    PFEM_TRY(probe_download(s, bw, W_out, who));
    PFEM_TRY(probe_download(s, bm, nullptr, who));
    if (dinv) PFEM_TRY(probe_download(s, bd, nullptr, who));
    std::memcpy(norms_out, h_out.data() + modal_gram_len(mb), sizeof(double) * 3 * mb);
    return PFEM_OK;
}

// k_modal_update<mb> on modal_update_grid(n, mb) blocks: the six blocks as the launch left them (pfem_amd_diag.h)
extern "C" int pfem_modal_probe_update(pfem_solver *s, int mb, int64_t n, const double *coef, double *X, double *W, double *P, double *KX, double *KW, double *KP)
{
    if (!probe_args(s, mb, n) || !coef || !X || !W || !P || !KX || !KW || !KP) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_modal_probe_update";
    const size_t rows = static_cast<size_t>(n), tile = kBlock / mb;
    ProbeBlock B[6];
    double *io[6] = {X, W, P, KX, KW, KP};
    const char *names[6] = {"X", "W", "P", "KX", "KW", "KP"};
    for (int k = 0; k < 6; ++k) PFEM_TRY(probe_upload(s, B[k], names[k], io[k], rows * mb, tile * mb));
    std::vector<double> h_coef(static_cast<size_t>(modal_coef_len(mb)), 0.0);
    std::memcpy(h_coef.data(), coef, sizeof(double) * 3 * mb * mb);
    DevBuf<double> d_coef;
    PFEM_TRY(d_coef.alloc(h_coef.size()));
    ModalView V;
    V.mb = mb;
    V.n = n;
    V.X = B[0].d.p; V.W = B[1].d.p; V.P = B[2].d.p; V.KX = B[3].d.p; V.KW = B[4].d.p; V.KP = B[5].d.p;
    V.coef = d_coef.p;
    PFEM_TRY(modal_update(s, V, h_coef.data()));
    for (int k = 0; k < 6; ++k) PFEM_TRY(probe_download(s, B[k], io[k], who));       // (each waits for the stream)
    return PFEM_OK;
}

// microseconds of one k_spmm<mb> launch and of mb launches of the SpMV form in effect, `reps` of each between two events after
// a warm-up of each, on the same handle (tools/lab/modal_measure.py)
extern "C" int pfem_modal_bench_spmm(pfem_solver *s, int mb, int reps, double *us_spmm, double *us_mb_spmv)
{
    if (!s || reps < 1 || !us_spmm || !us_mb_spmv || (mb != 4 && mb != 8 && mb != 16)) return PFEM_ERR_ARG;
    PFEM_TRY(needs_one_rank(s, "pfem_modal_bench_spmm"));
    if (!s->have_pattern || s->status < PFEM_ASSEMBLY_OK) return PFEM_ERR_STATE;
    PFEM_TRY(use_device(s));
    const int64_t n = s->n_loc;
    const size_t len = static_cast<size_t>(std::max<int64_t>(n, 1)) * mb;
    DevBuf<double> dx, dy;
    PFEM_TRY(dx.alloc(len));
    PFEM_TRY(dy.alloc(len));
    with_mb(mb, [&](auto MB) {
        launch(k_modal_init<decltype(MB)::value>, dim3(grid_for(n * mb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, 0, nullptr, dx.p);
    });
    mark_group_vals(s);
    PFEM_TRY(refresh_group_vals(s));
    PFEM_HIP(hipMemcpyAsync(s->d_p.p, s->d_rhs.p, sizeof(double) * static_cast<size_t>(n), hipMemcpyDeviceToDevice, s->stream));
    double ms = 0.0;
    modal_spmm(s, mb, dx.p, dy.p);
    PFEM_HIP(hipEventRecord(s->ev0, s->stream));
    for (int i = 0; i < reps; ++i) modal_spmm(s, mb, dx.p, dy.p);
    PFEM_HIP(hipEventRecord(s->ev1, s->stream));
    PFEM_TRY(check_kernel("k_spmm"));
    PFEM_TRY(elapsed(s, &ms));
    *us_spmm = 1e3 * ms / reps;
    launch_spmv<false>(s, s->d_p.p, s->d_w.p, 0, nullptr, nullptr);
    PFEM_HIP(hipEventRecord(s->ev0, s->stream));
    for (int i = 0; i < reps * mb; ++i) launch_spmv<false>(s, s->d_p.p, s->d_w.p, 0, nullptr, nullptr);
    PFEM_HIP(hipEventRecord(s->ev1, s->stream));
    PFEM_TRY(check_kernel("k_spmv"));
    PFEM_TRY(elapsed(s, &ms));
    *us_mb_spmv = 1e3 * ms / reps;
    return PFEM_OK;
}

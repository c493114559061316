// pfem_buckling.inc -- linear buckling on an assembled elasticity system (pfem_buckling_setup / pfem_buckling_solve; DESIGN.md
// section 15).  Included once by pfem_device.hip after pfem_modal.inc, whose host pieces it shares: the block choice, the grids,
// the Rayleigh-Ritz step on the host, the column-by-column gamg cycle.  The set-up writes K_g's values into a second fp64 array on
// K's row form (scatter form: f64 atomics); the solve is pfem_modal_solve's LOBPCG on the pencil (K_g, K): A = K_g, and K S where
// that routine has m o S.  A path beside everything else: it reads K's row form, K_g and the diagonal and writes only the buffers
// of Buck (under gamg also the cycle's work vectors and the SpMV's copies of the values, as the modal solve).

namespace {

// The nine blocks of one launch: ModalView's six (KX, KW, KP are the K-products), and the K_g-products
struct BuckView {
    ModalView V;
    double *GX = nullptr, *GW = nullptr, *GP = nullptr;
};

bool buck_kind(int kind) { return kind == PFEM_ELAST_TET || kind == PFEM_ELAST_TRIA; }

SellDev buck_sell(const pfem_solver *s)
{
    SellDev G = s->sell();
    G.vals = s->buck->kg.p;
    return G;
}

// the run's own buffers for blocks of mb columns
int buck_ensure(pfem_solver *s, int mb)
{
    Buck &B = *s->buck;
    const int64_t n = s->n_loc;
    if (B.blocks && B.blocks->mb == mb && B.blocks->n == n) return PFEM_OK;
    B.blocks.reset();
    B.ran = false;
    auto M = std::make_unique<Modal>();
    M->mb = mb;
    M->n = n;
    const size_t len = static_cast<size_t>(std::max<int64_t>(n, 1)) * static_cast<size_t>(mb);
    for (DevBuf<double> *g : {&M->X, &M->W, &M->P, &M->KX, &M->KW, &M->KP, &B.GX, &B.GW, &B.GP}) PFEM_TRY(g->alloc(len));
    PFEM_TRY(M->dinv.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
    PFEM_TRY(M->vec.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
    PFEM_TRY(M->part_gram.alloc(static_cast<size_t>(kModalGramBlocks) * modal_gram_len(mb)));
    PFEM_TRY(M->part_res.alloc(static_cast<size_t>(kModalVecBlocks) * 3 * mb));
    PFEM_TRY(M->out.alloc(static_cast<size_t>(modal_out_len(mb))));
    PFEM_TRY(M->coef.alloc(static_cast<size_t>(modal_coef_len(mb))));
    if (hipHostMalloc(reinterpret_cast<void **>(&M->h_out), sizeof(double) * modal_out_len(mb)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&M->h_coef), sizeof(double) * modal_coef_len(mb)) != hipSuccess) {
        (void)hipGetLastError();
        set_last_error("pfem_buckling_solve: no pinned host memory for the per-iteration copies");
        return PFEM_ERR_NOMEM;
    }
    B.blocks = std::move(M);
    return PFEM_OK;
}

BuckView buck_view(Buck &B)
{
    Modal &M = *B.blocks;
    BuckView Q;
    ModalView &V = Q.V;
    V.mb = M.mb;
    V.n = M.n;
    V.X = M.X.p; V.W = M.W.p; V.P = M.P.p; V.KX = M.KX.p; V.KW = M.KW.p; V.KP = M.KP.p;
    V.dinv = M.dinv.p;
    V.vec = M.vec.p;
    V.coef = M.coef.p; V.part_gram = M.part_gram.p; V.part_res = M.part_res.p; V.out = M.out.p;
    V.h_out = M.h_out;
    Q.GX = B.GX.p; Q.GW = B.GW.p; Q.GP = B.GP.p;
    return Q;
}

// Y = A X by k_spmm<mb>, A the row form with K's values (s->sell()) or K_g's (buck_sell)
void buck_spmm(pfem_solver *s, int mb, const SellDev &A, const double *X, double *Y)
{
    with_mb(mb, [&](auto MB) {
        launch(k_spmm<decltype(MB)::value>, dim3(grid_for(A.n_rows)), dim3(kBlock), 0, s->stream, nullptr, nullptr, A, X, Y);
    });
}

// the Gram pass over the nine blocks and the sums of its partials and (res_blocks > 0) of the residual kernel's; then the copy to
// the host buffer and the wait for it
int buck_gram_to_host(pfem_solver *s, const BuckView &Q, bool with_gram, unsigned res_blocks)
{
    const ModalView &V = Q.V;
    const int mb = V.mb, n_gram = modal_gram_len(mb), n_res = 3 * mb;
    const unsigned gg = modal_gram_grid(V.n);
    if (with_gram)
        with_mb(mb, [&](auto MB) {
            launch(k_buck_gram<decltype(MB)::value>, dim3(gg), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.X, V.W, V.P, V.KX, V.KW, V.KP, Q.GX, Q.GW, Q.GP,
                   V.part_gram);
        });
    launch(k_modal_sum, dim3(grid_for(n_gram + n_res)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n_gram, with_gram ? static_cast<int>(gg) : 0, V.part_gram,
           n_res, static_cast<int>(res_blocks), V.part_res, V.out);
    PFEM_TRY(check_kernel("k_buck_gram"));
    PFEM_HIP(hipMemcpyAsync(V.h_out, V.out, sizeof(double) * modal_out_len(mb), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

// R, the norms' partials and W = T R: the point Jacobi of K inside the residual kernel, or (gamg) the cycle on every column
unsigned buck_residual(pfem_solver *s, const BuckView &Q, bool gamg)
{
    const ModalView &V = Q.V;
    const unsigned gr = modal_vec_grid(V.n * V.mb);
    with_mb(V.mb, [&](auto MB) {
        launch(k_buck_residual<decltype(MB)::value>, dim3(gr), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, Q.GX, V.KX, gamg ? nullptr : V.dinv,
               V.coef + 3 * V.mb * V.mb, V.W, V.part_res);
    });
    if (gamg && !modal_cycle_columns(s, V)) return 0;
    return gr;
}

// h_coef (C, then theta) to the device, then the update of the nine blocks in place
int buck_update(pfem_solver *s, const BuckView &Q, const double *h_coef)
{
    const ModalView &V = Q.V;
    PFEM_HIP(hipMemcpyAsync(V.coef, h_coef, sizeof(double) * modal_coef_len(V.mb), hipMemcpyHostToDevice, s->stream));
    with_mb(V.mb, [&](auto MB) {
        launch(k_buck_update<decltype(MB)::value>, dim3(modal_update_grid(V.n, V.mb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, V.n, V.coef, V.X, V.W, V.P,
               V.KX, V.KW, V.KP, Q.GX, Q.GW, Q.GP);
    });
    return check_kernel("k_buck_update");
}

}  // namespace

extern "C" int pfem_buckling_setup(pfem_solver *s, const double *elemData, const double *u_nodal, const double *elem_stress)
{
    if (!s) return PFEM_ERR_ARG;
    const char *who = "pfem_buckling_setup";
    PFEM_TRY(needs_mesh(s, who));
    const MeshDev &m = s->mesh;
    if (!buck_kind(m.kind)) {
        set_last_error(std::string(who) + ": a geometric stiffness exists for PFEM_ELAST_TET and PFEM_ELAST_TRIA only");
        return PFEM_ERR_ARG;
    }
    if (!elemData) return PFEM_ERR_ARG;
    PFEM_TRY(needs_pattern(s, who));
    if (s->status < PFEM_ASSEMBLY_OK) {
        set_last_error(std::string(who) + ": no assembled matrix (pfem_assemble after the last pfem_solver_set_zero)");
        return PFEM_ERR_STATE;
    }
    PFEM_TRY(use_device(s));
    auto B = std::make_unique<Buck>();
    const int ng = post_components(m.kind);
    const size_t ne = static_cast<size_t>(m.nElem), entries = std::max<size_t>(s->d_vals.n, 1);
    PFEM_TRY(B->kg.alloc(entries));
    PFEM_TRY(B->stress.alloc(std::max<size_t>(ne * ng, 1)));
    DevBuf<double> u;
    if (elem_stress) {
        PFEM_HIP(hipMemcpyAsync(B->stress.p, elem_stress, sizeof(double) * ne * ng, hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
    } else {
        PFEM_TRY(post_nodal_field(s, u_nodal, u, who));
    }
    return with_post_prm(s, elemData, nullptr, [&](const auto &prm) -> int {
        using PRM = std::decay_t<decltype(prm)>;
        const auto &base = [&]() -> const auto & {
            if constexpr (PrmThermal<PRM>::value) return prm.base;
            else return prm;
        }();
        using BASE = std::decay_t<decltype(base)>;
        SellDev G = s->sell();
        G.vals = B->kg.p;
        PFEM_HIP(hipMemsetAsync(s->d_err.p, 0, sizeof(int), s->stream));
        PFEM_HIP(hipEventRecord(s->ev0, s->stream));
        PFEM_HIP(hipMemsetAsync(B->kg.p, 0, sizeof(double) * entries, s->stream));
        if (m.nElem > 0) {
            with_kind(m.kind, [&](auto kind) {
                constexpr int K = decltype(kind)::value;
                if constexpr (K == PFEM_ELAST_TET || K == PFEM_ELAST_TRIA) {
                    // the stresses pfem_post_elements would return (D (strain - eps_th) under a thermal state), left on the device
                    if (!elem_stress)
                        launch(k_post_elements<K, PRM>, dim3(grid_for(m.nElem)), dim3(kBlock), 0, s->stream, nullptr, nullptr, m, prm, u.p,
                               static_cast<double *>(nullptr), B->stress.p, static_cast<double *>(nullptr), s->d_err.p);
                    launch(k_geo_assemble<K, BASE>, dim3(grid_for(m.nElem)), dim3(kBlock), 0, s->stream, nullptr, nullptr, m, G, base, B->stress.p, s->d_err.p);
                }
            });
            PFEM_TRY(check_kernel("k_geo_assemble"));
        }
        PFEM_HIP(hipEventRecord(s->ev1, s->stream));
        int err = 0;
        PFEM_TRY(fetch_err(s, &err));
        PFEM_TRY(elapsed(s, &B->setup_ms));
        if (err) return err;
        s->buck = std::move(B);            // (a new set-up replaces the old one, its blocks included)
        return PFEM_OK;
    });
}

extern "C" int pfem_buckling_get_geometric(pfem_solver *s, double *vals)
{
    if (!s || !vals) return PFEM_ERR_ARG;
    if (!s->buck || !s->have_pattern) {
        set_last_error("pfem_buckling_get_geometric: pfem_buckling_setup first (after every pattern build)");
        return PFEM_ERR_STATE;
    }
    PFEM_TRY(use_device(s));
    return get_csr_of(s, buck_sell(s), nullptr, nullptr, vals);
}

extern "C" int pfem_buckling_setup_ms(pfem_solver *s, double *ms)
{
    if (!s || !ms) return PFEM_ERR_ARG;
    if (!s->buck) return PFEM_ERR_STATE;
    *ms = s->buck->setup_ms;
    return PFEM_OK;
}

extern "C" int pfem_buckling_solve(pfem_solver *s, int n_modes, int block, double tol, int max_iterations, int pc, const double *x0, double *theta_out,
                                   double *factor, double *modes, double *residuals, int *iterations, int *restarts, int *reason)
{
    if (iterations) *iterations = 0;
    if (restarts) *restarts = 0;
    if (reason) *reason = 0;
    if (!s || !theta_out || !factor || !residuals || !iterations || !restarts || !reason) return PFEM_ERR_ARG;
    int mb = 0;
    PFEM_TRY(modal_block(n_modes, block, &mb));
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iterations < 1) return PFEM_ERR_ARG;
    if (pc != -1 && pc != PFEM_PC_JACOBI && pc != PFEM_PC_NODE_BLOCK_JACOBI && pc != PFEM_PC_GAMG) return PFEM_ERR_ARG;
    if (mb > s->n_owned) return PFEM_ERR_ARG;
    const char *who = "pfem_buckling_solve";
    int count = 0;
    pfem_device_count(&count);
    if (count == 0) return PFEM_ERR_NOGPU;
    PFEM_TRY(needs_one_rank(s, who));
    if (!s->buck || !s->have_pattern) {
        set_last_error(std::string(who) + ": pfem_buckling_setup first (after every pattern build)");
        return PFEM_ERR_STATE;
    }
    if (s->status < PFEM_ASSEMBLY_OK) {
        set_last_error(std::string(who) + ": no assembled matrix (pfem_assemble after the last pfem_solver_set_zero)");
        return PFEM_ERR_STATE;
    }
    // T as pfem_modal_solve chooses it: the cycle of the last gamg solve where it is current, else the point Jacobi of K
    const bool want_gamg = pc == PFEM_PC_GAMG || (pc == -1 && s->pc == PFEM_PC_GAMG);
    const bool gamg = want_gamg && modal_gamg_current(s);
    if (pc == PFEM_PC_GAMG && !gamg) {
        set_last_error(std::string(who) + ": pc = gamg needs a gamg solve since the last assemble (its numeric set-up is the T)");
        return PFEM_ERR_STATE;
    }
    PFEM_TRY(use_device(s));
    PFEM_TRY(buck_ensure(s, mb));
    Buck &B = *s->buck;
    Modal &M = *B.blocks;
    const BuckView Q = buck_view(B);
    const int64_t n = M.n;
    const SellDev K = s->sell(), G = buck_sell(s);
    M.pc_used = gamg ? PFEM_PC_GAMG : PFEM_PC_JACOBI;
    B.ran = true;
    if (gamg) {                            // the cycle's fine-level products run in the SpMV form in effect: its copies of the values
        mark_group_vals(s);
        PFEM_TRY(refresh_group_vals(s));
    }
    const int NS = 3 * mb;
    const size_t block_bytes = sizeof(double) * static_cast<size_t>(n) * mb;
    // T = 1 / K_ii from the row form, in the run's own buffer
    launch(k_extract_diag, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, K, M.dinv.p);
    launch(k_modal_invert, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, M.dinv.p);
    PFEM_TRY(check_kernel("k_modal_invert"));
    // the start: X0, zero W and P and their products, K X0 and K_g X0, one Rayleigh-Ritz on X0 alone
    if (x0) {
        PFEM_TRY(modal_upload_block(s, mb, x0, M.X.p));
    } else {
        with_mb(mb, [&](auto MB) {
            launch(k_modal_init<decltype(MB)::value>, dim3(grid_for(n * mb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, s->row_start,
                   s->reordered ? static_cast<const int32_t *>(s->d_perm.p) : nullptr, M.X.p);
        });
    }
    for (DevBuf<double> *g : {&M.W, &M.P, &M.KW, &M.KP, &B.GW, &B.GP}) PFEM_HIP(hipMemsetAsync(g->p, 0, block_bytes, s->stream));
    PFEM_HIP(hipMemsetAsync(M.out.p, 0, sizeof(double) * modal_out_len(mb), s->stream));
    buck_spmm(s, mb, K, M.X.p, M.KX.p);
    buck_spmm(s, mb, G, M.X.p, B.GX.p);
    PFEM_TRY(buck_gram_to_host(s, Q, true, 0));
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
    PFEM_TRY(buck_update(s, Q, M.h_coef));
    while (why == 0) {
        // R, W = T R and the norms; K W and K_g W; the Gram matrices of [X W P]; one copy back
        const unsigned gr = buck_residual(s, Q, gamg);
        if (gr == 0) return PFEM_ERR_HIP;
        buck_spmm(s, mb, K, M.W.p, M.KW.p);
        buck_spmm(s, mb, G, M.W.p, B.GW.p);
        PFEM_TRY(buck_gram_to_host(s, Q, true, gr));
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
        PFEM_TRY(buck_update(s, Q, M.h_coef));
        have_p = true;
        if (its % kModalRefresh == 0) {
            buck_spmm(s, mb, K, M.X.p, M.KX.p);
            buck_spmm(s, mb, G, M.X.p, B.GX.p);
        }
    }
    // the end: residuals from explicit products (theta is ascending as the Rayleigh-Ritz step left it)
    buck_spmm(s, mb, K, M.X.p, M.KX.p);
    buck_spmm(s, mb, G, M.X.p, B.GX.p);
    const unsigned gr = buck_residual(s, Q, false);
    PFEM_TRY(buck_gram_to_host(s, Q, false, gr));
    for (int j = 0; j < n_modes; ++j) {
        theta_out[j] = theta[j];
        factor[j] = theta[j] < 0.0 ? -1.0 / theta[j] : static_cast<double>(INFINITY);
        residuals[j] = modal_res(M, j, theta[j]);
    }
    *iterations = its;
    *restarts = n_restarts;
    *reason = why;
    if (modes) {
        // phi^T K phi = 1 by the explicit K X, the entry of largest magnitude positive (the lowest index on ties): on the host, in
        // the caller's order
        std::vector<double> h_x(static_cast<size_t>(n) * mb), h_kx(static_cast<size_t>(n) * mb);
        PFEM_HIP(hipMemcpyAsync(h_x.data(), M.X.p, block_bytes, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipMemcpyAsync(h_kx.data(), M.KX.p, block_bytes, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        for (int j = 0; j < n_modes; ++j) {
            double *out = modes + static_cast<int64_t>(j) * n;
            double energy = 0.0, big = -1.0;
            bool negative = false;
            for (int64_t l = 0; l < n; ++l) {
                const size_t at = static_cast<size_t>(to_internal(s, l)) * mb + j;
                const double v = h_x[at];
                out[l] = v;
                energy += v * h_kx[at];
                if (std::fabs(v) > big) { big = std::fabs(v); negative = v < 0.0; }
            }
            const double scale = (negative ? -1.0 : 1.0) / std::sqrt(energy);
            for (int64_t l = 0; l < n; ++l) out[l] *= scale;
        }
    }
    return PFEM_OK;
}

// the T of the last pfem_buckling_solve on this handle: PFEM_PC_JACOBI or PFEM_PC_GAMG (pfem_amd_diag.h)
extern "C" int pfem_buckling_last_pc(pfem_solver *s, int *pc)
{
    if (!s || !pc) return PFEM_ERR_ARG;
    if (!s->buck || !s->buck->blocks || !s->buck->ran) return PFEM_ERR_STATE;
    *pc = s->buck->blocks->pc_used;
    return PFEM_OK;
}

// ---- one launch of a buckling kernel on blocks of the caller's (pfem_amd_diag.h) -----------------------------------------------
// k_buck_gram<mb> on modal_gram_grid(n) blocks, then k_modal_sum: out = the 2 NS NS doubles of h_out
extern "C" int pfem_buck_probe_gram(pfem_solver *s, int mb, int64_t n, const double *X, const double *W, const double *P, const double *KX, const double *KW,
                                    const double *KP, const double *GX, const double *GW, const double *GP, double *out)
{
    if (!probe_args(s, mb, n) || !X || !W || !P || !KX || !KW || !KP || !GX || !GW || !GP || !out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_buck_probe_gram";
    const size_t rows = static_cast<size_t>(n), tile = kModalGramTile;
    ProbeBlock B[9];
    const double *in[9] = {X, W, P, KX, KW, KP, GX, GW, GP};
    const char *names[9] = {"X", "W", "P", "KX", "KW", "KP", "GX", "GW", "GP"};
    for (int k = 0; k < 9; ++k) PFEM_TRY(probe_upload(s, B[k], names[k], in[k], rows * mb, tile * mb));
    DevBuf<double> part_gram, part_res, d_out;
    PFEM_TRY(part_gram.alloc(static_cast<size_t>(kModalGramBlocks) * modal_gram_len(mb)));
    PFEM_TRY(part_res.alloc(1));
    PFEM_TRY(d_out.alloc(static_cast<size_t>(modal_out_len(mb))));
    PFEM_HIP(hipMemsetAsync(d_out.p, 0, sizeof(double) * modal_out_len(mb), s->stream));
    std::vector<double> h_out(static_cast<size_t>(modal_out_len(mb)));
    BuckView Q;
    ModalView &V = Q.V;
    V.mb = mb;
    V.n = n;
    V.X = B[0].d.p; V.W = B[1].d.p; V.P = B[2].d.p; V.KX = B[3].d.p; V.KW = B[4].d.p; V.KP = B[5].d.p;
    Q.GX = B[6].d.p; Q.GW = B[7].d.p; Q.GP = B[8].d.p;
    V.part_gram = part_gram.p; V.part_res = part_res.p; V.out = d_out.p;
    V.h_out = h_out.data();
    PFEM_TRY(buck_gram_to_host(s, Q, true, 0));
    for (int k = 0; k < 9; ++k) PFEM_TRY(probe_download(s, B[k], nullptr, who));
    std::memcpy(out, h_out.data(), sizeof(double) * modal_gram_len(mb));
    return PFEM_OK;
}

// k_buck_residual<mb> on modal_vec_grid(n mb) blocks, then k_modal_sum: W and the 3 mb norms^2
extern "C" int pfem_buck_probe_residual(pfem_solver *s, int mb, int64_t n, const double *GX, const double *KX, const double *dinv, const double *theta,
                                        double *W_out, double *norms_out)
{
    if (!probe_args(s, mb, n) || !GX || !KX || !theta || !W_out || !norms_out) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_buck_probe_residual";
    const size_t rows = static_cast<size_t>(n), tile = kBlock / mb;
    ProbeBlock bgx, bkx, bw, bd;
    PFEM_TRY(probe_upload(s, bgx, "GX", GX, rows * mb, tile * mb));
    PFEM_TRY(probe_upload(s, bkx, "KX", KX, rows * mb, tile * mb));
    PFEM_TRY(probe_upload(s, bw, "W", nullptr, rows * mb, tile * mb));
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
    BuckView Q;
    ModalView &V = Q.V;
    V.mb = mb;
    V.n = n;
    Q.GX = bgx.d.p; V.KX = bkx.d.p; V.W = bw.d.p;
    V.dinv = dinv ? bd.d.p : nullptr;
    V.coef = coef.p; V.part_gram = part_gram.p; V.part_res = part_res.p; V.out = d_out.p;
    V.h_out = h_out.data();
    const unsigned gr = buck_residual(s, Q, false);
    PFEM_TRY(check_kernel("k_buck_residual"));
    PFEM_TRY(buck_gram_to_host(s, Q, false, gr));    // (waits for the stream: h_coef has been read)
    PFEM_TRY(probe_download(s, bgx, nullptr, who));
    PFEM_TRY(probe_download(s, bkx, nullptr, who));
    PFEM_TRY(probe_download(s, bw, W_out, who));
    if (dinv) PFEM_TRY(probe_download(s, bd, nullptr, who));
    std::memcpy(norms_out, h_out.data() + modal_gram_len(mb), sizeof(double) * 3 * mb);
    return PFEM_OK;
}

// k_buck_update<mb> on modal_update_grid(n, mb) blocks: the nine blocks as the launch left them
extern "C" int pfem_buck_probe_update(pfem_solver *s, int mb, int64_t n, const double *coef, double *X, double *W, double *P, double *KX, double *KW, double *KP,
                                      double *GX, double *GW, double *GP)
{
    if (!probe_args(s, mb, n) || !coef || !X || !W || !P || !KX || !KW || !KP || !GX || !GW || !GP) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const char *who = "pfem_buck_probe_update";
    const size_t rows = static_cast<size_t>(n), tile = kBlock / mb;
    ProbeBlock B[9];
    double *io[9] = {X, W, P, KX, KW, KP, GX, GW, GP};
    const char *names[9] = {"X", "W", "P", "KX", "KW", "KP", "GX", "GW", "GP"};
    for (int k = 0; k < 9; ++k) PFEM_TRY(probe_upload(s, B[k], names[k], io[k], rows * mb, tile * mb));
    std::vector<double> h_coef(static_cast<size_t>(modal_coef_len(mb)), 0.0);
    std::memcpy(h_coef.data(), coef, sizeof(double) * 3 * mb * mb);
    DevBuf<double> d_coef;
    PFEM_TRY(d_coef.alloc(h_coef.size()));
    BuckView Q;
    ModalView &V = Q.V;
    V.mb = mb;
    V.n = n;
    V.X = B[0].d.p; V.W = B[1].d.p; V.P = B[2].d.p; V.KX = B[3].d.p; V.KW = B[4].d.p; V.KP = B[5].d.p;
    Q.GX = B[6].d.p; Q.GW = B[7].d.p; Q.GP = B[8].d.p;
    V.coef = d_coef.p;
    PFEM_TRY(buck_update(s, Q, h_coef.data()));
    for (int k = 0; k < 9; ++k) PFEM_TRY(probe_download(s, B[k], io[k], who));       // (each waits for the stream)
    return PFEM_OK;
}

// microseconds of one launch of k_buck_gram (+ sum), k_buck_update, k_modal_gram (+ sum), k_modal_update on hashed blocks of n rows,
// `reps` of each between two events after a warm-up launch (tools/lab/buckling_measure.py)
extern "C" int pfem_buckling_bench_kernels(pfem_solver *s, int mb, int64_t n, int reps, double *us)
{
    if (!probe_args(s, mb, n) || reps < 1 || !us) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    const size_t len = static_cast<size_t>(n) * mb;
    DevBuf<double> blk[9], mass, part_gram, part_res, d_out, coef;
    for (DevBuf<double> &b : blk) {
        PFEM_TRY(b.alloc(len));
        with_mb(mb, [&](auto MB) {
            launch(k_modal_init<decltype(MB)::value>, dim3(grid_for(n * mb)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, static_cast<int64_t>(&b - blk) * n,
                   static_cast<const int32_t *>(nullptr), b.p);
        });
    }
    PFEM_TRY(mass.alloc(static_cast<size_t>(n)));
    PFEM_TRY(part_gram.alloc(static_cast<size_t>(kModalGramBlocks) * modal_gram_len(mb)));
    PFEM_TRY(part_res.alloc(1));
    PFEM_TRY(d_out.alloc(static_cast<size_t>(modal_out_len(mb))));
    PFEM_TRY(coef.alloc(static_cast<size_t>(modal_coef_len(mb))));
    PFEM_HIP(hipMemsetAsync(mass.p, 0, sizeof(double) * static_cast<size_t>(n), s->stream));
    PFEM_HIP(hipMemsetAsync(coef.p, 0, sizeof(double) * modal_coef_len(mb), s->stream));     // (C = 0: the blocks stay finite over the repetitions)
    std::vector<double> h_out(static_cast<size_t>(modal_out_len(mb))), h_coef(static_cast<size_t>(modal_coef_len(mb)), 0.0);
    BuckView Q;
    ModalView &V = Q.V;
    V.mb = mb;
    V.n = n;
    V.X = blk[0].p; V.W = blk[1].p; V.P = blk[2].p; V.KX = blk[3].p; V.KW = blk[4].p; V.KP = blk[5].p;
    Q.GX = blk[6].p; Q.GW = blk[7].p; Q.GP = blk[8].p;
    V.m = mass.p;
    V.coef = coef.p; V.part_gram = part_gram.p; V.part_res = part_res.p; V.out = d_out.p;
    V.h_out = h_out.data();
    // one pass through the solve's own launch code (grids, sums, copies), then the kernels alone between the events
    PFEM_TRY(buck_gram_to_host(s, Q, true, 0));
    PFEM_TRY(buck_update(s, Q, h_coef.data()));
    PFEM_TRY(modal_gram_to_host(s, V, true, 0));
    PFEM_TRY(modal_update(s, V, h_coef.data()));
    const unsigned gg = modal_gram_grid(n), gu = modal_update_grid(n, mb);
    const int n_gram = modal_gram_len(mb);
    for (int which = 0; which < 4; ++which) {
        double ms = 0.0;
        PFEM_HIP(hipEventRecord(s->ev0, s->stream));
        for (int i = 0; i < reps; ++i)
            with_mb(mb, [&](auto MB) {
                constexpr int B = decltype(MB)::value;
                if (which == 0)
                    launch(k_buck_gram<B>, dim3(gg), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, V.X, V.W, V.P, V.KX, V.KW, V.KP, Q.GX, Q.GW, Q.GP, V.part_gram);
                else if (which == 1)
                    launch(k_buck_update<B>, dim3(gu), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, V.coef, V.X, V.W, V.P, V.KX, V.KW, V.KP, Q.GX, Q.GW, Q.GP);
                else if (which == 2)
                    launch(k_modal_gram<B>, dim3(gg), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, V.X, V.W, V.P, V.KX, V.KW, V.KP, V.m, V.part_gram);
                else
                    launch(k_modal_update<B>, dim3(gu), dim3(kBlock), 0, s->stream, nullptr, nullptr, n, V.coef, V.X, V.W, V.P, V.KX, V.KW, V.KP);
                if (which % 2 == 0)
                    launch(k_modal_sum, dim3(grid_for(n_gram)), dim3(kBlock), 0, s->stream, nullptr, nullptr, n_gram, static_cast<int>(gg), V.part_gram, 0, 0,
                           V.part_res, V.out);
            });
        PFEM_HIP(hipEventRecord(s->ev1, s->stream));
        PFEM_TRY(check_kernel("pfem_buckling_bench_kernels"));
        PFEM_TRY(elapsed(s, &ms));
        us[which] = 1e3 * ms / reps;
    }
    return PFEM_OK;
}

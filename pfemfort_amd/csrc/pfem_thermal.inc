// pfem_thermal.inc -- thermal strains of the elasticity kinds (pfem_thermal_* / pfem_rhs_add_thermal_load; DESIGN.md section 14).
// Included once by pfem_device.hip, after the post-processing helpers it uses (node_accumulate, post_nodal_field,
// post_nodes_to_caller, thermal_prm).  A path beside the solve: the state is a nodal field and a few coefficients on the handle,
// the load adds to the assembled right-hand side like a surface load, and the post-processing calls read the state while it is set.

namespace {

int needs_thermal_kind(const pfem_solver *s, const char *who)
{
    PFEM_TRY(needs_pattern(s, who));
    if (s->mesh.kind != PFEM_ELAST_TET && s->mesh.kind != PFEM_ELAST_TRIA) {
        set_last_error(std::string(who) + ": thermal strains are defined for the elasticity kinds only");
        return PFEM_ERR_ARG;
    }
    return PFEM_OK;
}

// n_alpha against the material map, the coefficients finite; a fresh state with the coefficients in place and theta allocated
int thermal_new_state(pfem_solver *s, int n_alpha, const double *alpha, const char *who, std::unique_ptr<Thermal> *out)
{
    if (n_alpha != std::max(s->n_mat, 1)) {
        set_last_error(std::string(who) + ": n_alpha must be 1 without a material map and n_mat with one");
        return PFEM_ERR_ARG;
    }
    for (int k = 0; k < n_alpha; ++k)
        if (!std::isfinite(alpha[k])) return PFEM_ERR_ARG;
    PFEM_TRY(use_device(s));
    auto T = std::make_unique<Thermal>();
    T->h_alpha.assign(alpha, alpha + n_alpha);
    PFEM_TRY(T->d_theta.alloc(static_cast<size_t>(s->mesh.nNode)));
    if (s->n_mat > 0) {
        PFEM_TRY(T->d_alpha.alloc(static_cast<size_t>(n_alpha)));
        PFEM_HIP(hipMemcpyAsync(T->d_alpha.p, T->h_alpha.data(), sizeof(double) * static_cast<size_t>(n_alpha), hipMemcpyHostToDevice, s->stream));
    }
    *out = std::move(T);
    return PFEM_OK;
}

}  // namespace

extern "C" int pfem_thermal_set(pfem_solver *s, int n_alpha, const double *alpha, const double *theta_nodal)
{
    if (!s || !alpha || !theta_nodal || n_alpha < 1) return PFEM_ERR_ARG;
    PFEM_TRY(needs_thermal_kind(s, "pfem_thermal_set"));
    std::unique_ptr<Thermal> T;
    PFEM_TRY(thermal_new_state(s, n_alpha, alpha, "pfem_thermal_set", &T));
    const int64_t nn = s->mesh.nNode;
    std::vector<double> tmp;
    if (!s->h_nperm.empty()) {
        tmp.resize(static_cast<size_t>(nn));
        for (int64_t n = 0; n < nn; ++n) tmp[static_cast<size_t>(s->h_nperm[static_cast<size_t>(n)])] = theta_nodal[n];
    }
    PFEM_HIP(hipMemcpyAsync(T->d_theta.p, tmp.empty() ? theta_nodal : tmp.data(), sizeof(double) * static_cast<size_t>(nn), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));       // (tmp and the caller's arrays are free again)
    s->thermal = std::move(T);
    return PFEM_OK;
}

extern "C" int pfem_thermal_set_from_solver(pfem_solver *dst, int n_alpha, const double *alpha, pfem_solver *src, double T_ref)
{
    if (!dst || !src || dst == src || !alpha || n_alpha < 1 || !std::isfinite(T_ref)) return PFEM_ERR_ARG;
    PFEM_TRY(needs_thermal_kind(dst, "pfem_thermal_set_from_solver"));
    PFEM_TRY(needs_mesh(src, "pfem_thermal_set_from_solver (source)"));
    if (src->mesh.ndof != 1 || src->mesh.nNode != dst->mesh.nNode) {
        set_last_error("pfem_thermal_set_from_solver: the source must be a handle of a one-dof kind with the same number of nodes");
        return PFEM_ERR_ARG;
    }
    if (src->device != dst->device) {
        set_last_error("pfem_thermal_set_from_solver: the two handles live on different devices");
        return PFEM_ERR_ARG;
    }
    if (!src->have_pattern || !src->solved) {
        set_last_error("pfem_thermal_set_from_solver: the source has no solve of its pattern");
        return PFEM_ERR_STATE;
    }
    std::unique_ptr<Thermal> T;
    PFEM_TRY(thermal_new_state(dst, n_alpha, alpha, "pfem_thermal_set_from_solver", &T));
    const int64_t nn = dst->mesh.nNode;
    // the source's field in the source's device order, on the source's stream
    DevBuf<double> field;
    PFEM_TRY(post_nodal_field(src, nullptr, field, "pfem_thermal_set_from_solver"));
    // map[dst device node] = src device node: through the caller's numbering, which the two handles share
    DevBuf<int32_t> d_map;
    std::vector<int32_t> map;
    if (!dst->h_niperm.empty() || !src->h_nperm.empty()) {
        map.resize(static_cast<size_t>(nn));
        for (int64_t i = 0; i < nn; ++i) {
            const int32_t c = dst->h_niperm.empty() ? static_cast<int32_t>(i) : dst->h_niperm[static_cast<size_t>(i)];
            map[static_cast<size_t>(i)] = src->h_nperm.empty() ? c : src->h_nperm[static_cast<size_t>(c)];
        }
        PFEM_TRY(d_map.alloc(static_cast<size_t>(nn)));
        PFEM_HIP(hipMemcpyAsync(d_map.p, map.data(), sizeof(int32_t) * static_cast<size_t>(nn), hipMemcpyHostToDevice, dst->stream));
    }
    // the receiving stream waits for the field
    hipEvent_t ready = nullptr;
    PFEM_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    hipError_t he = hipEventRecord(ready, src->stream);
    if (he == hipSuccess) he = hipStreamWaitEvent(dst->stream, ready, 0);
    if (he != hipSuccess) {
        (void)hipEventDestroy(ready);
        set_last_error(std::string("pfem_thermal_set_from_solver: ") + hipGetErrorString(he));
        return PFEM_ERR_HIP;
    }
    launch(k_thermal_carry, dim3(grid_for(nn)), dim3(kBlock), 0, dst->stream, nullptr, nullptr, nn, static_cast<const int32_t *>(d_map.p),
           static_cast<const double *>(field.p), T_ref, T->d_theta.p);
    const int rc = check_kernel("k_thermal_carry");
    he = hipStreamSynchronize(dst->stream);           // (field, the map and the event go out of scope)
    (void)hipEventDestroy(ready);
    if (rc != PFEM_OK) return rc;
    if (he != hipSuccess) {
        set_last_error(std::string("pfem_thermal_set_from_solver: ") + hipGetErrorString(he));
        return PFEM_ERR_HIP;
    }
    dst->thermal = std::move(T);
    return PFEM_OK;
}

extern "C" int pfem_thermal_get(pfem_solver *s, int *n_alpha, double *alpha, double *theta_nodal)
{
    if (!s) return PFEM_ERR_ARG;
    if (!s->thermal) {
        set_last_error("pfem_thermal_get: no thermal state set");
        return PFEM_ERR_STATE;
    }
    const Thermal &T = *s->thermal;
    if (n_alpha) *n_alpha = static_cast<int>(T.h_alpha.size());
    if (alpha) std::copy(T.h_alpha.begin(), T.h_alpha.end(), alpha);
    if (!theta_nodal) return PFEM_OK;
    PFEM_TRY(use_device(s));
    return post_nodes_to_caller(s, T.d_theta.p, 1, theta_nodal);
}

extern "C" int pfem_thermal_clear(pfem_solver *s)
{
    if (!s) return PFEM_ERR_ARG;
    s->thermal.reset();
    return PFEM_OK;
}

extern "C" int pfem_rhs_add_thermal_load(pfem_solver *s, const double *elemData)
{
    if (!s || !elemData) return PFEM_ERR_ARG;
    PFEM_TRY(needs_thermal_kind(s, "pfem_rhs_add_thermal_load"));
    if (!s->thermal) {
        set_last_error("pfem_rhs_add_thermal_load: pfem_thermal_set first (after every pattern build)");
        return PFEM_ERR_STATE;
    }
    PFEM_TRY(use_device(s));
    const MeshDev &m = s->mesh;
    DevBuf<double> dF;
    return with_elem_prm(s, elemData, nullptr, [&](const auto &base) -> int {
        const auto prm = thermal_prm(s, base);
        using PRM = std::decay_t<decltype(prm)>;
        const int64_t nv = m.nNode * m.ndof;
        const dim3 block(kBlock);
        PFEM_TRY(dF.alloc(static_cast<size_t>(std::max<int64_t>(nv, 1))));
        PFEM_HIP(hipMemsetAsync(s->d_err.p, 0, sizeof(int), s->stream));
        NodePass pass;
        PFEM_TRY(node_accumulate(
            s, "k_thermal_load", {},
            [&](auto kind, dim3 grid, const uint8_t *hubs) {
                if constexpr (prm_fits_kind<PRM>(decltype(kind)::value))
                    launch(k_thermal_load_gather<decltype(kind)::value, PRM>, grid, block, 0, s->stream, nullptr, nullptr, m, prm, s->d_inc_ptr.p, s->d_inc_cnt.p,
                           s->d_inc_rec.p, hubs, dF.p, s->d_err.p);
            },
            [&](auto kind, dim3 grid, const uint8_t *hubs) {
                if constexpr (prm_fits_kind<PRM>(decltype(kind)::value))
                    launch(k_thermal_load_scatter<decltype(kind)::value, PRM>, grid, block, 0, s->stream, nullptr, nullptr, m, prm, hubs, s->d_rhs.p, s->d_err.p);
            },
            &pass));
        if (pass.gather) {
            // the node sums into the rows of the free dofs (the hub nodes' entries are zeros: their rows took the element pass)
            launch(k_thermal_load_rows, dim3(grid_for(nv)), block, 0, s->stream, nullptr, nullptr, nv, static_cast<const int32_t *>(s->d_node_row.p),
                   static_cast<const double *>(dF.p), s->d_rhs.p);
            PFEM_TRY(check_kernel("k_thermal_load_rows"));
        }
        int err = 0;
        PFEM_TRY(fetch_err(s, &err));         // (waits for the stream)
        return err;
    });
}

// pfem_amg.inc -- aggregation multigrid as the preconditioner of the CG solve (-pc_type gamg), host side.
// Included by pfem_device.hip inside its anonymous namespace, after launch_spmv.
//
// WHY.  solverpetsc.F:187,206 runs KSPCG + PCBJACOBI/ILU(0): 110 iterations on the 200^3 Poisson box, 1 122 on the beam,
// where point Jacobi -- what north_star names and what the default remains -- needs 370 and 5 207, doubling with every
// doubling of the mesh.  The Jacobi iteration already runs at the HBM roofline, so fewer iterations are the only lever
// left on one GPU.  ILU(0) itself was measured and refused in round 2 (sequential triangular solves: 346 ms per
// application).  Probed this round on the oracle's matrices (profiles/r03/preconditioner_probe.json): Chebyshev-Jacobi as
// a polynomial preconditioner never lowers the SpMV count (CG is optimal in the Krylov space); multicolour SGS halves the
// iterations at twice the cost; a plain-aggregation multigrid V-cycle needs 15-25 iterations at ~5 SpMV-equivalents each
// and its count grows only slowly with the mesh.  PETSc's name for this family is PCGAMG; what is built here is its
// simplest member, chosen because every piece streams:
//
//   * aggregates: three passes of pairing, i.e. up to 8 nodes per aggregate: along one axis per pass when the mesh has a
//     lattice (k_amg_lat_*: exact 2x2x2 bricks, aligned on every level), else pairwise matching on the strength graph
//     (locally dominant edges, k_amg_match_*, ties along a Morton curve).  Dofs of one node (the row groups the SpMV
//     found) stay together; the coarse space has one vector per component (piecewise-constant prolongation);
//   * Galerkin coarse operators P^T A P: with piecewise-constant P every coarse entry is a plain sum of fine entries.
//     The symbolic phase sorts (coarse row, coarse col, fine slot) once; the numeric phase (every solve: the matrix may
//     have new values) is one gather pass per level, fixed summation order, no atomics;
//   * smoother: Chebyshev of degree 2 on D^-1 A over [lmax/8, lmax], lmax = the Gershgorin bound max_i sum_j|a_ij|/a_ii
//     (one pass over the matrix, no power iteration, no reductions inside the cycle);
//   * coarsest level (<= 128 rows): dense inverse by Gauss-Jordan in LDS, applied as a matrix-vector product;
//   * V(1,1) cycle, symmetric (same polynomial before and after) -> an SPD preconditioner, plain CG stays valid.
//
// The aggregates depend on the matrix VALUES of the first solve after a pattern build and are reused while the pattern
// lives (PETSc: -pc_gamg_reuse_interpolation true); everything numeric is redone in every solve, inside its timer.
// Several ranks: one hierarchy across the ranks (amg_couple_level, amg_replicate, amg_apply_coupled) or, on request, one
// per rank (block Jacobi over the ranks); see run_pcg_amg.

constexpr int kAmgMaxLevels = 14;
constexpr int kAmgMatchRounds = 8;
constexpr int kAmgPasses = 3;
// coupled hierarchy: a level this small (rows over all ranks) is assembled on every rank.  Self-peer probe at 200^3 over RCCL
// (profiles/r04/coupled_cycle_rccl_self_peer.json): the 125 000-row level carried by the rank alone instead of exchanged
// 1.547 -> 1.488 ms per iteration (10 -> 6 exchanges per cycle); a 1 000 000-row level would cost every rank what a whole
// level 1 costs (~0.25 ms) to save four exchanges: not worth it.  Was 32 768 in round 3.
constexpr int64_t kAmgReplicateRows = 150000;
constexpr int kAmgRetryBlock = -7701;       // internal: the coupled hierarchy cannot be formed on this partition, all ranks fall back together

inline bool amg_in_effect(const pfem_solver *s)
{
    return s->pc == PFEM_PC_GAMG;
}
// PFEM_AMG_VERBOSE: the symbolic phase says on stderr where its time goes and why a level leaves the brick path (read at every call)
inline bool amg_verbose()
{
    return std::getenv("PFEM_AMG_VERBOSE") != nullptr;
}
// PFEM_AMG_BRICK_SORT: brick and node-brick levels take the sorted route to their maps (A/B; the bricks also take it for rows too
// long for 16-bit counters).  Read once per process.
inline bool amg_brick_sort()
{
    static const bool v = std::getenv("PFEM_AMG_BRICK_SORT") != nullptr;
    return v;
}

// level 0 = the rank's OWNED block of its matrix: the owned rows come first in the local numbering, so the block is the
// first n_owned rows with the columns below n_owned (the kernels that walk rows take the column limit)
// (rows: L.n = the owned dofs, the domain of the aggregation and the block of a per-rank hierarchy; L.n_loc = all local
// rows, what a rank-coupled hierarchy works on.  They differ on level 0 of any multi-rank solve and on every level of a
// coupled hierarchy.)
inline SellDev amg_sell(const pfem_solver *s, const AmgLevel &L, int64_t rows)
{
    SellDev A;
    if (L.fine) {
        A = s->sell();
    } else {
        A.slice_off = L.slice_off.p;
        A.rowlen = L.rowlen.p;
        A.cols = L.cols.p;
        A.vals = L.vals.p;
    }
    A.n_rows = rows;
    A.n_slices = (rows + 63) / 64;
    return A;
}
inline SellDev amg_sell(const pfem_solver *s, const AmgLevel &L)
{
    return amg_sell(s, L, L.n);
}
// the rows the numeric phase and the cycle work on
inline int64_t amg_rows(const Amg &M, const AmgLevel &L)
{
    return M.coupled ? L.n_loc : L.n;
}
inline PlanRef amg_plan(const pfem_solver *s, const AmgLevel &L)
{
    if (L.fine) return plan_of(s);
    const AmgPlan &P = L.plan;
    return PlanRef{static_cast<int>(P.peers.size()), P.peers.data(), P.peer_off.data(), P.n_send, P.n_sh,
                   P.d_send_lidx.p, P.d_sh_lidx.p, P.d_sh_ptr.p, P.d_sh_src.p, P.d_row_sh.p};
}

// y = A_level x (level 0: whatever form the solver's SpMV has picked); a coupled hierarchy gets this rank's share of the
// product over all its local rows -- the caller sums over the holders (exchange_sum) where it needs the product itself
inline void amg_spmv(pfem_solver *s, const Amg &M, AmgLevel &L, const double *x, double *y)
{
    if (L.fine) {
        launch_spmv<false>(s, x, y, 0, nullptr, nullptr);
    } else {
        const SellDev A = amg_sell(s, L, amg_rows(M, L));
        if (M.coupled && L.vd.ok && L.vcodes.p)         // the level's values as dictionary codes (amg_value_codes): same product, 4 + 2 B a slot
            hipLaunchKernelGGL(k_amg_spmv_pack_vd, dim3(spmv_grid(A.n_slices)), dim3(kBlock), sizeof(double) * static_cast<size_t>(L.vd.n), s->stream, A,
                               static_cast<const uint16_t *>(L.vcodes.p), static_cast<const double *>(L.vd.dict.p), L.vd.n, x, y,
                               ShareSum{nullptr, nullptr, nullptr, nullptr}, static_cast<double *>(nullptr), static_cast<const CgCtl *>(nullptr));
        else
        hipLaunchKernelGGL(k_spmv<false>, dim3(spmv_grid(A.n_slices)), dim3(kBlock), 0, s->stream, A, x, y,
                           static_cast<int64_t>(0), static_cast<double *>(nullptr), static_cast<const CgCtl *>(nullptr), SliceSel{nullptr, 0});
    }
}

// PFEM_AMG_VERBOSE: where the symbolic phase spends its time -- the time since the last mark, after a synchronisation
struct AmgPhaseClock {
    hipStream_t stream;
    bool verbose;
    std::chrono::steady_clock::time_point tick;
    void operator()(int lvl, const char *what)
    {
        if (!verbose) return;
        (void)hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "  gamg symbolic level %d %-28s %9.2f ms\n", lvl, what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
    }
};

// small host vectors summed over the ranks (symbolic phase of a coupled hierarchy: level sizes, verdicts); collective
int amg_allreduce_host(pfem_solver *s, double *v, int n)
{
    Amg &M = *s->amg;
    if (M.lam_all.n < static_cast<size_t>(n)) { PFEM_HIP(hipStreamSynchronize(s->stream)); PFEM_TRY(M.lam_all.alloc(static_cast<size_t>(std::max(n, 256)))); }
    PFEM_HIP(hipMemcpyAsync(M.lam_all.p, v, sizeof(double) * static_cast<size_t>(n), hipMemcpyHostToDevice, s->stream));
    PFEM_TRY(s->comm->allreduce(M.lam_all.p, n, s->stream));
    PFEM_HIP(hipMemcpyAsync(v, M.lam_all.p, sizeof(double) * static_cast<size_t>(n), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

// Coupled symbolic phase: a stretch of rank-local work (allocations, size checks) ends here.  All ranks learn whether any of
// them failed it and return together -- a rank that left alone would leave the others waiting in the next collective
// (broadcast_rccl_id in pfemfort_amd/distributed.py exists for the same reason).  Collective.
int amg_agree(pfem_solver *s, int rc_local)
{
    double bad = rc_local == PFEM_OK ? 0.0 : 1.0;
    const int rc = amg_allreduce_host(s, &bad, 1);
    if (rc != PFEM_OK) return rc;
    if (rc_local != PFEM_OK) return rc_local;
    if (bad > 0.0) { set_last_error("gamg symbolic phase: another rank failed (allocation or size limit); all ranks stop together"); return PFEM_ERR_COMM; }
    return PFEM_OK;
}

// ---- lattice bookkeeping of the brick levels (host; identical on every rank: computed from all-reduced data only) ----------
// the axis sequence of a level's passes: x, y, z, x, ... skipping axes without extent; shift = halvings per axis
inline int lat_sim_passes(const int hi_in[3], int axis_in, int shift[3], int hi_out[3], int *axis_out)
{
    int hi[3] = {hi_in[0], hi_in[1], hi_in[2]}, axis = axis_in, halved = 0;
    shift[0] = shift[1] = shift[2] = 0;
    for (int pass = 0; pass < kAmgPasses; ++pass) {
        int k = 0;
        for (; k < 3 && hi[axis] < 1; ++k) axis = (axis + 1) % 3;
        if (k == 3) break;
        ++shift[axis];
        hi[axis] >>= 1;
        axis = (axis + 1) % 3;
        ++halved;
    }
    for (int d = 0; d < 3; ++d) hi_out[d] = hi[d];
    *axis_out = axis;
    return halved;
}
// Positions 0..hi[d] with stretches of one owner starting at cuts[d][k] (ascending, [0] = 0) -> padded positions in which no
// brick of the level (1 << shift[d] positions along axis d, shift from the axis sequence on the PADDED extents: iterated, it
// only grows) holds positions of two stretches.  table[1024 d + p] = padded position of p.  false: beyond 10 bits per axis.
// WHERE THE ODD ONE GOES.  A stretch of odd length leaves one position without a partner.  Always at the stretch's end, a
// stretch of 49 -> 25 -> 13 -> 7 planes (rank 7 of config 5 on 8 ranks) kept ONE fine plane as a brick of its own through
// every level: on the level that is replicated it sat next to bricks eight planes thick, its couplings failed the strength
// check, the level left the brick path and the hierarchy took 16 iterations and ten levels instead of 14 and seven.  So the
// odd one alternates: at the start of the stretch (the stretch starts on an ODD position, behind a free one) when the last
// odd one went to the end, and the other way round -- the thin brick of one level is paired on the next.  single[d][k] = 1:
// the last odd one of stretch k went to the start.  The first stretch starts at position 0 on every level (one rank: the
// one-rank hierarchy, entry for entry); axes that are halved twice or more in one level keep the plain alignment.
struct LatPad {
    std::vector<int32_t> table;
    std::vector<int> cuts[3];
    std::vector<char> single[3];
    int hi[3] = {0, 0, 0};
    int shift[3] = {0, 0, 0};           // what the padding was made for: a level that takes other bricks leaves the brick path
};
// occ: lowest and highest OCCUPIED position per axis (x, y, z lows, then highs) -- a Dirichlet plane at either end of the lattice
// has a position and no dofs; the length that decides about the odd one counts occupied positions
inline bool lat_pad(const std::vector<int> cuts[3], const std::vector<char> single_in[3], const int hi[3], const int occ[6], int axis, LatPad &out)
{
    int shift[3] = {0, 0, 0};
    out.table.assign(3 * 1024, 0);
    for (int iter = 0; iter < 5; ++iter) {
        for (int d = 0; d < 3; ++d) {
            out.cuts[d].clear();
            out.single[d].clear();
            int next = 0;
            const size_t ns = std::max<size_t>(cuts[d].size(), 1);
            for (size_t k = 0; k < ns; ++k) {
                const int start = cuts[d].empty() ? 0 : cuts[d][k];
                const int end = k + 1 < ns ? cuts[d][k + 1] : hi[d] + 1;
                const int len = end - start, len_occ = std::min(end, occ[3 + d] + 1) - std::max(start, occ[d]);
                const char prev = k < single_in[d].size() ? single_in[d][k] : 0;
                const int a = 1 << shift[d];
                int base = k == 0 ? 0 : (next + a - 1) / a * a;
                char now = shift[d] == 0 ? prev : 0;
                if (k > 0 && shift[d] == 1 && len_occ > 0 && (len_occ & 1) && prev == 0) {        // the odd one to the start: behind a free position
                    base = (next + 1) | 1;
                    now = 1;
                }
                out.cuts[d].push_back(base);
                out.single[d].push_back(now);
                if (base + len > 1024) return false;
                for (int p = start; p < end; ++p) out.table[static_cast<size_t>(1024 * d + p)] = base + (p - start);
                next = base + len;
            }
            out.hi[d] = next - 1;
        }
        int s2[3], h2[3], a2 = 0;
        lat_sim_passes(out.hi, axis, s2, h2, &a2);
        bool same = true;
        for (int d = 0; d < 3; ++d) { if (s2[d] > shift[d]) { shift[d] = s2[d]; same = false; } }
        if (same) {
            for (int d = 0; d < 3; ++d) out.shift[d] = shift[d];
            return true;
        }
    }
    return false;
}

int lattice_distinct(pfem_solver *s, int count[3], std::vector<double> &h_uniq, bool *ok);
int lattice_assign(pfem_solver *s, const std::vector<double> &h_uniq, const int count[3], int64_t n_rows, DevBuf<int32_t> &pos, int fill);
// Level 0 of a scalar hierarchy across ranks: GLOBAL lattice positions of all local dofs (owned and ghost) in L0.hint -- the
// ranks' distinct coordinate values merged, every rank's owned dofs checked to fill a box of positions, the planes between
// the boxes padded onto even positions (lat_pad).  *is_lattice = false (nothing touched): no lattice, or owned sets that are
// not boxes (the pairing passes take the hierarchy).  Collective; every verdict is formed from all-reduced data.
// `nodes` (displacement problems, L0.bs dofs to the node, rigid-body transfer): the positions of the local NODES, unpadded --
// node bricks are described by a table position -> brick coordinate per axis, cut at the owners' borders (node_brick_axis), so
// nothing has to be aligned; L0.lat_str = the occupied stretches of one owner per axis, L0.lat_tlo / lat_thi = this rank's box.
// `split` (scalar problems whose ranks' dofs do NOT fill boxes -- a METIS-like partition; round 6): the positions as they are, no
// box asked of anybody, nothing padded: a rank's aggregate is ITS part of a brick (amg_split_bricks).  L0.lat_tlo / lat_thi =
// the box of this rank's owned positions.
// Bricks are refused where the couplings inside them are weak (below a quarter of the row's strongest): a verdict about the LEVEL.
// Cells stretched along an axis make every row's coupling along it weak; a few nodes moved off their sites (a lattice by
// numbering, lattice_positions_by_numbering) make a few such rows, and the bricks stay.  Refused from this share of the rows on
// (kAmgBrickWeakPercent; round 5 refused them from any row).
constexpr double kAmgBrickWeakPercent = 5.0;
inline bool amg_too_many_weak(double weak, double rows)
{
    return weak > 0.0 && weak * 100.0 > kAmgBrickWeakPercent * rows;
}

int lattice_positions_global(pfem_solver *s, AmgLevel &L0, bool *is_lattice, bool nodes = false, bool split = false)
{
    *is_lattice = false;
    const int bs0 = nodes ? std::max(L0.bs, 1) : 1;
    const int nr = s->nranks, me = s->rank, ndim = s->have_mesh ? s->mesh.ndim : 3;
    int count[3] = {1, 1, 1};
    std::vector<double> h_uniq;
    bool ok = false;
    // (a rank that holds nothing -- an idle rank of a partition with fewer parts than ranks -- has no values to add and no say)
    const bool empty_rank = s->n_loc == 0 || !s->have_mesh || s->mesh.nElem < 1;
    if (empty_rank && s->n_owned == 0) {
        h_uniq.assign(3 * 1024, 0.0);
        count[0] = count[1] = count[2] = 0;
        ok = true;
        PFEM_TRY(amg_agree(s, PFEM_OK));
    } else {
        PFEM_TRY(amg_agree(s, lattice_distinct(s, count, h_uniq, &ok)));
    }
    const size_t per = 4 + 3 * 1024;
    std::vector<double> all(static_cast<size_t>(nr) * per, 0.0);
    {
        double *mine = all.data() + static_cast<size_t>(me) * per;
        mine[0] = ok ? 0.0 : 1.0;
        for (int d = 0; d < 3; ++d) mine[1 + d] = count[d];
        if (ok) std::copy(h_uniq.begin(), h_uniq.end(), mine + 4);
    }
    PFEM_TRY(amg_allreduce_host(s, all.data(), static_cast<int>(all.size())));
    int gcount[3] = {1, 1, 1};
    std::vector<double> g_uniq(3 * 1024, 0.0);
    for (int q = 0; q < nr; ++q)
        if (all[static_cast<size_t>(q) * per] != 0.0) return PFEM_OK;
    (void)ndim;
    for (int d = 0; d < 3; ++d) {                   // (an axis nobody has values for -- plane problems' z -- keeps one position)
        std::vector<double> vals;
        for (int q = 0; q < nr; ++q) {
            const double *his = all.data() + static_cast<size_t>(q) * per;
            const int c = static_cast<int>(his[1 + d]);
            vals.insert(vals.end(), his + 4 + 1024 * d, his + 4 + 1024 * d + c);
        }
        std::sort(vals.begin(), vals.end());
        vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
        if (vals.size() > 1024) return PFEM_OK;
        if (vals.empty()) continue;
        gcount[d] = static_cast<int>(vals.size());
        std::copy(vals.begin(), vals.end(), g_uniq.begin() + 1024 * d);
    }
    // positions among the merged values, then every rank's box of owned positions
    DevBuf<int32_t> raw;
    DevBuf<int> d_box;
    int box[6] = {1023, 1023, 1023, 0, 0, 0};
    int unplaced = 0;
    auto local = [&]() -> int {
        if (empty_rank && s->n_owned == 0) return PFEM_OK;
        PFEM_TRY(lattice_assign(s, g_uniq, gcount, s->n_loc, raw, split ? 0xff : 0));
        PFEM_TRY(d_box.alloc(8));
        PFEM_HIP(hipMemcpyAsync(d_box.p, box, sizeof box, hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipMemsetAsync(d_box.p + 6, 0, 2 * sizeof(int), s->stream));
        if (split && s->n_owned > 0)              // an owned dof without a position (no node of this rank's mesh carries it): no bricks
            hipLaunchKernelGGL(k_lat_count_unplaced, dim3(grid_for(s->n_owned)), dim3(kBlock), 0, s->stream, s->n_owned, static_cast<const int32_t *>(raw.p), d_box.p + 6);
        if (s->n_owned > 0 && !split)
            hipLaunchKernelGGL(k_lat_bbox, dim3(std::min<unsigned>(grid_for(s->n_owned), kLatBoxBlocks)), dim3(kBlock), 0, s->stream, s->n_owned, static_cast<const int32_t *>(raw.p), d_box.p);
        PFEM_TRY(check_kernel("k_lat_bbox"));
        PFEM_HIP(hipMemcpyAsync(&unplaced, d_box.p + 6, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        if (split && s->n_owned > 0 && !unplaced) {
            hipLaunchKernelGGL(k_lat_bbox, dim3(std::min<unsigned>(grid_for(s->n_owned), kLatBoxBlocks)), dim3(kBlock), 0, s->stream, s->n_owned, static_cast<const int32_t *>(raw.p), d_box.p);
            PFEM_TRY(check_kernel("k_lat_bbox"));
        }
        PFEM_HIP(hipMemcpyAsync(box, d_box.p, sizeof box, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        return PFEM_OK;
    };
    PFEM_TRY(amg_agree(s, local()));
    if (split) {                                  // (one verdict for all)
        double bad = unplaced ? 1.0 : 0.0;
        PFEM_TRY(amg_allreduce_host(s, &bad, 1));
        if (bad > 0.0) {
            if (amg_verbose()) std::fprintf(stderr, "  gamg symbolic: some rank owns dofs that none of its own mesh nodes carries: no split bricks\n");
            return PFEM_OK;
        }
    }
    std::vector<double> boxes(static_cast<size_t>(nr) * 7, 0.0);
    for (int k = 0; k < 6; ++k) boxes[static_cast<size_t>(me) * 7 + k] = box[k];
    boxes[static_cast<size_t>(me) * 7 + 6] = static_cast<double>(s->n_owned / bs0);
    PFEM_TRY(amg_allreduce_host(s, boxes.data(), static_cast<int>(boxes.size())));
    int gmin[3] = {1023, 1023, 1023}, gmax[3] = {0, 0, 0};
    for (int q = 0; q < nr; ++q) {
        const double *b = boxes.data() + static_cast<size_t>(q) * 7;
        if (b[6] < 1.0) continue;
        double vol = 1.0;
        for (int d = 0; d < 3; ++d) {
            vol *= b[3 + d] - b[d] + 1.0;
            gmin[d] = std::min(gmin[d], static_cast<int>(b[d]));
            gmax[d] = std::max(gmax[d], static_cast<int>(b[3 + d]));
        }
        if (vol != b[6] && !split) {                   // a rank's owned dofs do not fill a box of the lattice
            if (amg_verbose())
                std::fprintf(stderr, "  gamg symbolic: rank %d owns %g %s in a box of %g positions: no bricks across the ranks\n", q, b[6], nodes ? "nodes" : "dofs", vol);
            return PFEM_OK;
        }
    }
    std::vector<int> cuts[3];
    int hi_raw[3];
    for (int d = 0; d < 3; ++d) {
        hi_raw[d] = gcount[d] - 1;
        cuts[d].push_back(0);
        for (int q = 0; q < nr; ++q) {
            const double *b = boxes.data() + static_cast<size_t>(q) * 7;
            if (b[6] < 1.0) continue;
            if (static_cast<int>(b[d]) > gmin[d]) cuts[d].push_back(static_cast<int>(b[d]));
            if (static_cast<int>(b[3 + d]) < gmax[d]) cuts[d].push_back(static_cast<int>(b[3 + d]) + 1);
        }
        std::sort(cuts[d].begin(), cuts[d].end());
        cuts[d].erase(std::unique(cuts[d].begin(), cuts[d].end()), cuts[d].end());
    }
    LatPad P;
    const std::vector<char> no_single[3];
    const int occ_raw[6] = {gmin[0], gmin[1], gmin[2], gmax[0], gmax[1], gmax[2]};
    if (split)
        for (int d = 0; d < 3; ++d) cuts[d].assign(1, 0);        // (no borders to honour)
    if (nodes || split) {        // positions as they are
        P.table.assign(3 * 1024, 0);
        for (int d = 0; d < 3; ++d) {
            for (int p = 0; p < 1024; ++p) P.table[static_cast<size_t>(1024 * d + p)] = p;
            P.cuts[d] = cuts[d];
            P.single[d].assign(cuts[d].size(), 0);
            P.hi[d] = hi_raw[d];
        }
    } else if (!lat_pad(cuts, no_single, hi_raw, occ_raw, 0, P)) return PFEM_OK;
    DevBuf<int32_t> table;
    int lbox[6] = {1023, 1023, 1023, 0, 0, 0};
    auto finish = [&]() -> int {
        if (empty_rank && s->n_owned == 0) {
            PFEM_TRY(L0.hint.alloc(1));
            for (int k = 0; k < 6; ++k) lbox[k] = 0;
            return PFEM_OK;
        }
        PFEM_TRY(table.alloc(P.table.size()));
        PFEM_HIP(hipMemcpyAsync(table.p, P.table.data(), sizeof(int32_t) * P.table.size(), hipMemcpyHostToDevice, s->stream));
        PFEM_TRY(L0.hint.alloc(static_cast<size_t>(std::max<int64_t>(s->n_loc / bs0, 1))));
        if (nodes)               // one position per node (its dofs share it): all local nodes, owned first
            hipLaunchKernelGGL(k_amg_node_hint, dim3(grid_for(s->n_loc)), dim3(kBlock), 0, s->stream, s->n_loc, static_cast<const int32_t *>(L0.node_of.p),
                               static_cast<const int32_t *>(L0.comp_of.p), static_cast<const int32_t *>(raw.p), 1, L0.hint.p);
        else
        hipLaunchKernelGGL(k_lat_remap, dim3(grid_for(s->n_loc)), dim3(kBlock), 0, s->stream, s->n_loc, static_cast<const int32_t *>(raw.p),
                           static_cast<const int32_t *>(table.p), L0.hint.p);
        PFEM_HIP(hipMemcpyAsync(d_box.p, lbox, sizeof lbox, hipMemcpyHostToDevice, s->stream));
        if (s->n_loc > 0)
            hipLaunchKernelGGL(k_lat_bbox, dim3(std::min<unsigned>(grid_for(s->n_loc / bs0), kLatBoxBlocks)), dim3(kBlock), 0, s->stream, s->n_loc / bs0, static_cast<const int32_t *>(L0.hint.p), d_box.p);
        PFEM_TRY(check_kernel("k_lat_remap"));
        PFEM_HIP(hipMemcpyAsync(lbox, d_box.p, sizeof lbox, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        return PFEM_OK;
    };
    PFEM_TRY(amg_agree(s, finish()));
    for (int d = 0; d < 3; ++d) {
        L0.lat_hi[d] = P.hi[d];
        L0.lat_cuts[d] = P.cuts[d];
        L0.lat_single[d] = P.single[d];
        L0.lat_shift[d] = P.shift[d];
        L0.lat_occ[d] = P.table[static_cast<size_t>(1024 * d + gmin[d])];
        L0.lat_occ[3 + d] = P.table[static_cast<size_t>(1024 * d + gmax[d])];
    }
    for (int k = 0; k < 6; ++k) L0.lat_box[k] = lbox[k];
    L0.lat_coord.assign(3 * 1024, 0.0);
    for (int d = 0; d < 3; ++d)
        for (int p = 0; p < gcount[d]; ++p) L0.lat_coord[static_cast<size_t>(1024 * d + P.table[static_cast<size_t>(1024 * d + p)])] = g_uniq[static_cast<size_t>(1024 * d + p)];
    L0.lat_global = !nodes && !split;
    if (split) {
        L0.lat_split = true;
        for (int d = 0; d < 3; ++d) { L0.lat_tlo[d] = box[d]; L0.lat_thi[d] = box[3 + d]; }
    }
    if (nodes) {
        // occupied stretches of one owner per axis (inclusive ends), this rank's box of owned nodes
        L0.lat_nodes_global = true;
        L0.lat_full = true;              // (every rank's owned nodes fill their box: checked above)
        for (int d = 0; d < 3; ++d) {
            std::vector<int> b;
            b.push_back(gmin[d]);
            for (int c : cuts[d]) if (c > gmin[d] && c <= gmax[d]) b.push_back(c);
            b.push_back(gmax[d] + 1);
            L0.lat_str[d].clear();
            for (size_t k = 0; k + 1 < b.size(); ++k) L0.lat_str[d].push_back({b[k], b[k + 1] - 1});
            L0.lat_tlo[d] = box[d];
            L0.lat_thi[d] = box[3 + d];
        }
    }
    *is_lattice = true;
    return PFEM_OK;
}

// Work buffers of the symbolic phase, allocated once (level 0 is the largest user) and reused by every pass of every
// level: a hipMalloc / hipFree pair costs 0.2-0.4 ms with its implicit synchronisation, and the six small levels of a
// hierarchy went through ~300 of them -- half of the phase's 100 ms at config 3.
struct AmgGraph {
    int64_t n = 0, nnz = 0;
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> col;
    DevBuf<double> w, diag;
    int reserve(int64_t rows, int64_t entries)
    {
        n = rows;
        nnz = entries;
        PFEM_TRY(ptr.reserve(static_cast<size_t>(n) + 1));
        PFEM_TRY(col.reserve(static_cast<size_t>(std::max<int64_t>(nnz, 1))));
        PFEM_TRY(w.reserve(static_cast<size_t>(std::max<int64_t>(nnz, 1))));
        return diag.reserve(static_cast<size_t>(std::max<int64_t>(n, 1)));
    }
};
struct AmgWork {
    DevBuf<char> temp;
    DevBuf<int32_t> head, rank, match, cand, is_root, mrank, slots, step, flag, crank, cnt, idx, skey32;
    DevBuf<uint64_t> keys, skeys, ukeys;
    DevBuf<uint32_t> keys32, skeys32;
    DevBuf<double> vals, svals, sums;
    DevBuf<int64_t> start, slice_entries;
    AmgGraph graphs[2];
};

template <class T>
int amg_exclusive_sum(pfem_solver *s, DevBuf<char> &temp, const T *in, T *out, int64_t n)
{
    size_t tb = 0;
    PFEM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, static_cast<int>(n), s->stream));
    if (tb > temp.n) { PFEM_HIP(hipStreamSynchronize(s->stream)); PFEM_TRY(temp.alloc(tb)); }
    PFEM_HIP(hipcub::DeviceScan::ExclusiveSum(temp.p, tb, in, out, static_cast<int>(n), s->stream));
    return PFEM_OK;
}

// (key, value) pairs sorted by bits [0, end_bit) of the key; the stream is synchronised before temp is regrown: a pooled block
// may still be read
template <class K, class V>
int amg_sort_pairs(pfem_solver *s, DevBuf<char> &temp, const K *keys_in, K *keys_out, const V *vals_in, V *vals_out, int64_t count, int end_bit)
{
    size_t tb = 0;
    const int ni = static_cast<int>(count);
    PFEM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in, keys_out, vals_in, vals_out, ni, 0, end_bit, s->stream));
    if (tb > temp.n) { PFEM_HIP(hipStreamSynchronize(s->stream)); PFEM_TRY(temp.alloc(tb)); }
    PFEM_HIP(hipcub::DeviceRadixSort::SortPairs(temp.p, tb, keys_in, keys_out, vals_in, vals_out, ni, 0, end_bit, s->stream));
    return PFEM_OK;
}

// Runs of equal keys of a SORTED array: unique keys (ascending) and the start of every run (m + 1 entries).  Flags + one
// exclusive scan + a scatter -- hipcub's ReduceByKey / RunLengthEncode did the same job in 80 ms one time and in 3 s the
// next on the 1e9-entry graphs of config 5 (decoupled look-back stalling), which made the symbolic phase erratic.
int amg_unique_runs(pfem_solver *s, AmgWork &W, const uint64_t *skeys, int64_t count, DevBuf<uint64_t> &ukeys, DevBuf<int64_t> &start,
                    int64_t *n_unique, bool exact = true)
{
    DevBuf<char> &temp = W.temp;
    DevBuf<int32_t> &head = W.head, &rank = W.rank;
    PFEM_TRY(head.reserve(static_cast<size_t>(count) + 1));
    PFEM_TRY(rank.reserve(static_cast<size_t>(count) + 1));
    hipLaunchKernelGGL(k_amg_run_heads, dim3(grid_for(count + 1)), dim3(kBlock), 0, s->stream, count, skeys, head.p);
    PFEM_TRY(amg_exclusive_sum(s, temp, head.p, rank.p, count + 1));
    int32_t m32 = 0;
    PFEM_HIP(hipMemcpyAsync(&m32, rank.p + count, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    const int64_t m = m32;
    if (exact) {          // the outputs stay with a level
        PFEM_TRY(ukeys.alloc(static_cast<size_t>(std::max<int64_t>(m, 1))));
        PFEM_TRY(start.alloc(static_cast<size_t>(m) + 1));
    } else {
        PFEM_TRY(ukeys.reserve(static_cast<size_t>(std::max<int64_t>(m, 1))));
        PFEM_TRY(start.reserve(static_cast<size_t>(m) + 1));
    }
    hipLaunchKernelGGL(k_amg_run_scatter, dim3(grid_for(count + 1)), dim3(kBlock), 0, s->stream, count, skeys, static_cast<const int32_t *>(head.p),
                       static_cast<const int32_t *>(rank.p), ukeys.p, start.p);
    PFEM_TRY(check_kernel("k_amg_run_scatter"));
    *n_unique = m;
    return PFEM_OK;
}

// The padding entries collapse into one run of the all-ones sentinel key at the end of the unique keys: dropped (its slots are
// never read).  (On the solver's stream: the scatter that wrote ukeys is still in flight, and no hipFree synchronises for us.)
int amg_drop_sentinel_run(pfem_solver *s, const uint64_t *ukeys, int64_t *m)
{
    if (*m < 1) return PFEM_OK;
    uint64_t last = 0;
    PFEM_HIP(hipMemcpyAsync(&last, ukeys + (*m - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    if (last == ~0ull) --*m;
    return PFEM_OK;
}

// (key, double) pairs -> sorted, reduced by key: unique keys and sums; the all-ones sentinel key, if any, is dropped
int amg_sort_reduce(pfem_solver *s, AmgWork &W, DevBuf<uint64_t> &keys, DevBuf<double> &vals, int64_t count,
                    DevBuf<uint64_t> &ukeys, DevBuf<double> &sums, int64_t *n_unique)
{
    if (count > INT_MAX) { set_last_error("gamg: more than 2^31-1 graph entries on one device"); return PFEM_ERR_ARG; }
    DevBuf<uint64_t> &skeys = W.skeys;
    DevBuf<double> &svals = W.svals;
    PFEM_TRY(skeys.reserve(static_cast<size_t>(count)));
    PFEM_TRY(svals.reserve(static_cast<size_t>(count)));
    PFEM_TRY(amg_sort_pairs(s, W.temp, keys.p, skeys.p, vals.p, svals.p, count, 64));
    DevBuf<int64_t> &start = W.start;
    int64_t m = 0;
    PFEM_TRY(amg_unique_runs(s, W, skeys.p, count, ukeys, start, &m, false));
    PFEM_TRY(sums.reserve(static_cast<size_t>(std::max<int64_t>(m, 1))));
    if (m > 0) {
        hipLaunchKernelGGL(k_amg_run_sums, dim3(grid_for(m)), dim3(kBlock), 0, s->stream, m, static_cast<const int64_t *>(start.p),
                           static_cast<const double *>(svals.p), static_cast<const uint64_t *>(ukeys.p), sums.p);
        PFEM_TRY(check_kernel("k_amg_run_sums"));
        PFEM_TRY(amg_drop_sentinel_run(s, ukeys.p, &m));
    }
    *n_unique = m;
    return PFEM_OK;
}

// The sorted route to a coarse pattern.  The caller has emitted `count` (key, slot) pairs into W.keys / W.slots; here they are
// sorted (the slots in key order: src_slot, `count` of them) and the runs of equal keys found: ukeys, as long as the coarse
// pattern has entries, and the start of every run in src_ptr.  *nnz_c = the runs.  A caller whose pairs cover padding slots
// drops the sentinel's run (amg_drop_sentinel_run: a word back to the host, which the other callers do not pay for); the
// pattern's storage is the caller's too (amg_store_pattern, or the block split of a rigid-body level).
int amg_pattern_from_keys(pfem_solver *s, AmgWork &W, int64_t count, int32_t *src_slot, DevBuf<int64_t> &src_ptr, DevBuf<uint64_t> &ukeys, int64_t *nnz_c)
{
    PFEM_TRY(W.skeys.reserve(static_cast<size_t>(count)));
    PFEM_TRY(amg_sort_pairs(s, W.temp, W.keys.p, W.skeys.p, W.slots.p, src_slot, count, 64));
    return amg_unique_runs(s, W, W.skeys.p, count, ukeys, src_ptr, nnz_c);
}

int amg_graph_from_unique(pfem_solver *s, DevBuf<uint64_t> &ukeys, DevBuf<double> &sums, int64_t m, int64_t n, int squared, AmgGraph &G)
{
    PFEM_TRY(G.reserve(n, m));
    PFEM_HIP(hipMemsetAsync(G.diag.p, 0, sizeof(double) * std::max<int64_t>(n, 1), s->stream));
    hipLaunchKernelGGL(k_row_bounds, dim3(grid_for(std::max<int64_t>(m, n + 1))), dim3(kBlock), 0, s->stream, ukeys.p, m, n, G.ptr.p);
    PFEM_TRY(check_kernel("k_row_bounds (gamg graph)"));
    if (m > 0) {
        hipLaunchKernelGGL(k_amg_graph_from_keys, dim3(grid_for(m)), dim3(kBlock), 0, s->stream, m, static_cast<const uint64_t *>(ukeys.p),
                           static_cast<const double *>(sums.p), squared, G.col.p, G.w.p, G.diag.p);
        PFEM_TRY(check_kernel("k_amg_graph_from_keys"));
    }
    return PFEM_OK;
}

// a pairing pass over n nodes, either kind.  Begins: W.match = nobody matched yet, W.cand for the proposals.  Ends: the roots of
// the pairs and singles in W.match are numbered -- agg_step[node] = aggregate, *na = their number.
int amg_match_begin(pfem_solver *s, AmgWork &W, int64_t n)
{
    PFEM_TRY(W.match.reserve(static_cast<size_t>(n)));
    PFEM_TRY(W.cand.reserve(static_cast<size_t>(n)));
    PFEM_TRY(W.is_root.reserve(static_cast<size_t>(n) + 1));
    PFEM_TRY(W.mrank.reserve(static_cast<size_t>(n) + 1));
    PFEM_HIP(hipMemsetAsync(W.match.p, 0xff, sizeof(int32_t) * n, s->stream));
    return PFEM_OK;
}
int amg_match_end(pfem_solver *s, AmgWork &W, int64_t n, DevBuf<int32_t> &agg_step, int64_t *na)
{
    DevBuf<int32_t> &match = W.match, &is_root = W.is_root, &rank = W.mrank;
    PFEM_HIP(hipMemsetAsync(is_root.p + n, 0, sizeof(int32_t), s->stream));
    hipLaunchKernelGGL(k_amg_match_finish, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, match.p, is_root.p);
    PFEM_TRY(amg_exclusive_sum(s, W.temp, is_root.p, rank.p, n + 1));
    PFEM_TRY(agg_step.reserve(static_cast<size_t>(n)));
    hipLaunchKernelGGL(k_amg_agg_ids, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, static_cast<const int32_t *>(match.p),
                       static_cast<const int32_t *>(rank.p), agg_step.p);
    PFEM_TRY(check_kernel("k_amg_agg_ids"));
    int32_t total = 0;
    PFEM_HIP(hipMemcpyAsync(&total, rank.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    *na = total;
    return PFEM_OK;
}

// one pass of pairwise matching on G: agg_step[node] = aggregate (pairs and singles), *na = their number
int amg_match(pfem_solver *s, AmgWork &W, const AmgGraph &G, const int32_t *hint, DevBuf<int32_t> &agg_step, int64_t *na)
{
    const int64_t n = G.n;
    DevBuf<int32_t> &match = W.match, &cand = W.cand;
    PFEM_TRY(amg_match_begin(s, W, n));
    // small graphs are dense (every aggregate touches most others): many nodes propose to the same neighbour and few
    // proposals are mutual per round, so they get more rounds (they cost nothing)
    const int rounds = n < 8192 ? 8 * kAmgMatchRounds : kAmgMatchRounds;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_amg_match_pick, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, static_cast<const int64_t *>(G.ptr.p),
                           static_cast<const int32_t *>(G.col.p), static_cast<const double *>(G.w.p), static_cast<const double *>(G.diag.p),
                           hint, static_cast<const int32_t *>(match.p), cand.p);
        hipLaunchKernelGGL(k_amg_match_commit, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, static_cast<const int32_t *>(cand.p), match.p);
    }
    PFEM_TRY(check_kernel("k_amg_match"));
    return amg_match_end(s, W, n, agg_step, na);
}

// one pass of pairing along one axis of the lattice (hint = positions); same outputs as amg_match, plus the roots in
// W.match for the positions of the aggregates
int amg_match_lattice(pfem_solver *s, AmgWork &W, const AmgGraph &G, const int32_t *pos, int axis, bool absorb, DevBuf<int32_t> &agg_step, int64_t *na)
{
    const int64_t n = G.n;
    const int shift = 10 * axis;
    DevBuf<int32_t> &match = W.match, &cand = W.cand;
    PFEM_TRY(amg_match_begin(s, W, n));
    const int64_t *gptr = G.ptr.p;
    const int32_t *gcol = G.col.p;
    const double *gw = G.w.p, *gd = G.diag.p;
    hipLaunchKernelGGL(k_amg_lat_pick, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, gptr, gcol, gw, gd, pos, shift, cand.p);
    hipLaunchKernelGGL(k_amg_match_commit, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, static_cast<const int32_t *>(cand.p), match.p);
    // The node a line of odd length leaves over: alone (a thin cell at the end of the line; every level stays aligned, and
    // that is what converges best: 200^3 12 iterations, with the node joined to its neighbour's pair 15) or in a brick of 3
    // (smaller coarse levels; on the 3-dof beam the cheaper cycle outweighs the iterations: 155 against 166 ms).
    if (absorb) {
        hipLaunchKernelGGL(k_amg_lat_absorb, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, gptr, gcol, gw, gd, pos, shift,
                           static_cast<const int32_t *>(match.p), cand.p);
        hipLaunchKernelGGL(k_amg_lat_join, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, static_cast<const int32_t *>(cand.p), match.p);
    }
    PFEM_TRY(check_kernel("k_amg_lat_*"));
    return amg_match_end(s, W, n, agg_step, na);
}

// wave-sliced storage of a coarse matrix from its sorted unique (row << 32 | col) keys
int amg_sell_from_keys(pfem_solver *s, AmgWork &W, const uint64_t *ukeys, int64_t nnz, AmgLevel &C)
{
    DevBuf<char> &temp = W.temp;
    const int64_t n = C.n_loc;
    C.nnz = nnz;
    C.n_slices = (n + 63) / 64;
    PFEM_TRY(C.rowptr.alloc(static_cast<size_t>(n) + 1));
    PFEM_TRY(C.rowlen.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
    PFEM_TRY(C.slice_off.alloc(static_cast<size_t>(C.n_slices) + 1));
    DevBuf<int64_t> &slice_entries = W.slice_entries;
    PFEM_TRY(slice_entries.reserve(static_cast<size_t>(C.n_slices) + 1));
    hipLaunchKernelGGL(k_row_bounds, dim3(grid_for(std::max<int64_t>(nnz, n + 1))), dim3(kBlock), 0, s->stream, ukeys, nnz, n, C.rowptr.p);
    hipLaunchKernelGGL(k_slice_sizes, dim3(grid_for(C.n_slices * 64)), dim3(kBlock), 0, s->stream, static_cast<const int64_t *>(C.rowptr.p), n,
                       C.n_slices, C.rowlen.p, slice_entries.p);
    PFEM_TRY(check_kernel("k_slice_sizes (gamg)"));
    PFEM_TRY(amg_exclusive_sum(s, temp, slice_entries.p, C.slice_off.p, C.n_slices + 1));
    int64_t stored = 0;
    PFEM_HIP(hipMemcpyAsync(&stored, C.slice_off.p + C.n_slices, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    C.stored = stored;
    PFEM_TRY(C.cols.alloc(static_cast<size_t>(std::max<int64_t>(stored, 1))));
    PFEM_TRY(C.vals.alloc(static_cast<size_t>(std::max<int64_t>(stored, 1))));
    hipLaunchKernelGGL(k_fill_sell, dim3(grid_for(C.n_slices * 64)), dim3(kBlock), 0, s->stream, ukeys, static_cast<const int64_t *>(C.rowptr.p), n,
                       C.n_slices, static_cast<const int64_t *>(C.slice_off.p), C.cols.p);
    PFEM_TRY(check_kernel("k_fill_sell (gamg)"));
    PFEM_HIP(hipMemsetAsync(C.vals.p, 0, sizeof(double) * std::max<int64_t>(stored, 1), s->stream));
    return PFEM_OK;
}

// the coarse pattern's wave-sliced storage (C) and, per coarse entry, its slot there: where the numeric product puts its sum
int amg_store_pattern(pfem_solver *s, AmgWork &W, const uint64_t *ukeys, int64_t nnz_c, AmgLevel &C, DevBuf<int64_t> &dst_slot)
{
    PFEM_TRY(amg_sell_from_keys(s, W, ukeys, nnz_c, C));
    PFEM_TRY(dst_slot.alloc(static_cast<size_t>(std::max<int64_t>(nnz_c, 1))));
    hipLaunchKernelGGL(k_amg_dst_slots, dim3(grid_for(nnz_c)), dim3(kBlock), 0, s->stream, nnz_c, ukeys, static_cast<const int64_t *>(C.rowptr.p),
                       static_cast<const int64_t *>(C.slice_off.p), dst_slot.p);
    return check_kernel("k_amg_dst_slots");
}

// Members of every coarse dof (restriction as a gather), ascending: L.mem_ptr (n_coarse + 1) and L.mem_idx.  key[i] = the coarse
// dof of member i, sorted by its bits below end_bit.  skip_empty: without members nothing is numbered or sorted.
int amg_member_lists(pfem_solver *s, AmgWork &W, AmgLevel &L, const int32_t *key, int64_t n_members, int64_t n_coarse, int end_bit,
                     bool skip_empty = false)
{
    DevBuf<int32_t> &cnt = W.cnt, &idx = W.idx, &skey = W.skey32;
    PFEM_TRY(cnt.reserve(static_cast<size_t>(n_coarse) + 1));
    PFEM_TRY(idx.reserve(static_cast<size_t>(std::max<int64_t>(n_members, 1))));
    PFEM_TRY(skey.reserve(static_cast<size_t>(std::max<int64_t>(n_members, 1))));
    PFEM_TRY(L.mem_ptr.alloc(static_cast<size_t>(n_coarse) + 1));
    PFEM_TRY(L.mem_idx.alloc(static_cast<size_t>(std::max<int64_t>(n_members, 1))));
    PFEM_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * (n_coarse + 1), s->stream));
    hipLaunchKernelGGL(k_amg_count, dim3(grid_for(n_members)), dim3(kBlock), 0, s->stream, n_members, key, cnt.p);
    PFEM_TRY(amg_exclusive_sum(s, W.temp, cnt.p, L.mem_ptr.p, n_coarse + 1));
    if (skip_empty && n_members < 1) return PFEM_OK;
    hipLaunchKernelGGL(k_amg_iota, dim3(grid_for(n_members)), dim3(kBlock), 0, s->stream, n_members, idx.p);
    return amg_sort_pairs(s, W.temp, key, skey.p, static_cast<const int32_t *>(idx.p), L.mem_idx.p, n_members, end_bit);
}

// Counts and two scans instead of a sort (k_lat_codes_*, k_rbm_codes_*).  `count` launches the caller's count kernel, which
// leaves per coarse row (n of them) its coarse entries in W.head and its fine entries in W.rank and raises *d_fail; the
// exclusive sums of the two go to W.cnt and W.idx (what the caller's fill kernel reads) and the totals and the verdict come back.
int amg_count_scans(pfem_solver *s, AmgWork &W, int64_t n, const std::function<void()> &count, const char *what, const int *d_fail,
                    int32_t *n_entries, int32_t *n_pairs, int *fail)
{
    DevBuf<int32_t> &entries = W.head, &pairs = W.rank, &entry_off = W.cnt, &pair_off = W.idx;
    PFEM_TRY(entries.reserve(static_cast<size_t>(n) + 1));
    PFEM_TRY(pairs.reserve(static_cast<size_t>(n) + 1));
    PFEM_TRY(entry_off.reserve(static_cast<size_t>(n) + 1));
    PFEM_TRY(pair_off.reserve(static_cast<size_t>(n) + 1));
    count();
    PFEM_TRY(check_kernel(what));
    PFEM_TRY(amg_exclusive_sum(s, W.temp, entries.p, entry_off.p, n + 1));
    PFEM_TRY(amg_exclusive_sum(s, W.temp, pairs.p, pair_off.p, n + 1));
    PFEM_HIP(hipMemcpyAsync(n_entries, entry_off.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipMemcpyAsync(n_pairs, pair_off.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipMemcpyAsync(fail, d_fail, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

int amg_alloc_vectors(pfem_solver *s, AmgLevel &L)
{
    // level 0 on several ranks: the SpMV runs over ALL local rows and reads the ghost columns, so its input and output
    // vectors span the local numbering; with one hierarchy per rank their ghost part stays zero (the block has no ghost columns)
    const size_t n = static_cast<size_t>(std::max<int64_t>(L.n_loc, 1));
    const size_t g = L.fine ? static_cast<size_t>(kVecGuard) : 0;
    const size_t nv = n;
    PFEM_TRY(L.dinv.alloc(n));
    PFEM_TRY(L.t.alloc(nv));
    PFEM_TRY(L.r.alloc(n));
    if (!L.fine) PFEM_TRY(L.b.alloc(n));
    PFEM_TRY(L.x_store.alloc(nv + 2 * g));
    PFEM_TRY(L.dd_store.alloc(nv + 2 * g));
    PFEM_HIP(hipMemsetAsync(L.x_store.p, 0, sizeof(double) * (nv + 2 * g), s->stream));
    PFEM_HIP(hipMemsetAsync(L.dd_store.p, 0, sizeof(double) * (nv + 2 * g), s->stream));
    L.x = L.x_store.p + g;
    L.dd = L.dd_store.p + g;
    PFEM_TRY(L.lam.alloc(1));
    PFEM_TRY(L.part_max.alloc(static_cast<size_t>(grid_for((L.n_loc + 63) / 64 * 64))));
    return PFEM_OK;
}

// numeric Galerkin product of level L into level C (A = L's matrix)
inline bool amg_galerkin_by_entry()
{
    static const bool v = std::getenv("PFEM_AMG_GALERKIN_MAPS") != nullptr;        // A/B: the map-driven kernel on brick levels too (same bits)
    return v;
}
// `extras` (numeric phase of a one-rank hierarchy): the product also leaves C's inverse diagonal and Gershgorin ratios (C.dinv,
// C.t) and, where C streams value codes and has a dictionary with its hash table, C's codes (verdict word `vstate`, reset here)
// `from_codes` (level 0, amg_level0_codes said yes): the values are read as the SpMV's 16-bit codes instead of the row form's doubles
// `bound` (with extras; a word some kernel before this one has zeroed): the product also leaves the maximum of the ratios there --
// C's Gershgorin bound, C.bound_done -- and zeroes `zero` for the product after it.  Returns whether it did.
// `st`: the stream the product goes to (amg_galerkin: the solver's own)
inline bool amg_galerkin_on(hipStream_t st, pfem_solver *s, const AmgLevel &L, AmgLevel &C, const SellDev &A, bool extras = false, VdState *vstate = nullptr,
                            bool from_codes = false, double *bound = nullptr, double *zero = nullptr)
{
    C.bound_fresh = C.vd_direct = C.bound_done = false;
    if (L.code_of.p && !amg_galerkin_by_entry()) {
        if (C.n_loc < 1) return false;              // (a rank that holds nothing of this level)
        LatGalExtra X{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (extras && C.dinv.p && C.t.p && C.n_loc == C.n) {
            X.dinv_out = C.dinv.p;
            X.ratio_out = C.t.p;
            C.bound_fresh = true;
            if (bound) { X.bound = bound; X.zero = zero; C.bound_done = true; }
            if (vstate && C.vd.have && C.vd.hash_ok && C.vd.hash.p && C.vcodes.p && C.vcodes.n >= static_cast<size_t>(C.stored) && !C.vd.refused) {
                (void)C.vd.enqueue_against_standing(st, vstate);
                X.vhash = C.vd.hash.p;
                X.codes = C.vcodes.p;
                X.vstate = vstate;
                C.vd_direct = true;
            }
        }
        if (from_codes) {
            hipLaunchKernelGGL(k_lat_galerkin_codes, dim3(static_cast<unsigned>((C.n_loc + kLatGalThreads - 1) / kLatGalThreads)), dim3(kLatGalThreads),
                               sizeof(double) * static_cast<size_t>(std::max(s->vd.n, 1)), st, C.n_loc, static_cast<const int32_t *>(L.mem_ptr.p),
                               static_cast<const int32_t *>(L.mem_idx.p), static_cast<const int64_t *>(s->d_rslice_off.p),
                               static_cast<const unsigned long long *>(s->d_vcodes.p), static_cast<const uint32_t *>(L.glat.p),
                               static_cast<const double *>(s->vd.dict.p), s->vd.n, static_cast<const uint32_t *>(L.code_mask.p),
                               static_cast<const int64_t *>(C.slice_off.p), C.vals.p, X);
            return C.bound_done;
        }
        hipLaunchKernelGGL(k_lat_galerkin, dim3(static_cast<unsigned>((C.n_loc + kLatGalThreads - 1) / kLatGalThreads)), dim3(kLatGalThreads), 0, st, A, C.n_loc,
                           static_cast<const int32_t *>(L.mem_ptr.p), static_cast<const int32_t *>(L.mem_idx.p), static_cast<const uint8_t *>(L.code_of.p),
                           static_cast<const uint32_t *>(L.code_mask.p), static_cast<const int64_t *>(C.slice_off.p), C.vals.p, X);
        return C.bound_done;
    }
    hipLaunchKernelGGL(k_amg_galerkin, dim3(grid_for(L.nnz_c)), dim3(kBlock), 0, st, L.nnz_c, static_cast<const int64_t *>(L.src_ptr.p),
                       static_cast<const int32_t *>(L.src_slot.p), static_cast<const int64_t *>(L.dst_slot.p),
                       static_cast<const double *>(A.vals), C.vals.p);
    return false;
}
inline bool amg_galerkin(pfem_solver *s, const AmgLevel &L, AmgLevel &C, const SellDev &A, bool extras = false, VdState *vstate = nullptr,
                         bool from_codes = false, double *bound = nullptr, double *zero = nullptr)
{
    return amg_galerkin_on(s->stream, s, L, C, A, extras, vstate, from_codes, bound, zero);
}

// Coupled hierarchy, one level (collective): the ghosts of level L learn their aggregates from the owners; the coarse
// level C gets its ghosts (the neighbours' aggregates that dofs held here belong to), its local numbering -- owned dofs
// first, ghosts after them by global number -- and its neighbour plan.  A coarse dof is held by every rank that holds one
// of its fine dofs; two of its holders need not share a FINE dof (a third rank's aggregate reaching into both), so the
// owner -- who knows all holders of its fine dofs from the level's plan, and so all holders of its aggregates -- tells
// them: a second sum-exchange carries the holder set of every aggregate (one bit per rank in a double: <= 52 ranks).  With
// every other holder of a coarse dof a rank then shares that dof; both sides list what they share by global number.
// kAmgRetryBlock when the ranks cannot do this (more than 52 of them, or plan and ownership disagree somewhere).
// With rigid-body modes (cb > 0: coarse dofs come cb to the node, every rank's owned coarse dofs are whole nodes, nc_of =
// owned coarse dofs of every rank) a fine node names only the translation dofs of its aggregate; ghosts, holder sets and
// shared lists are widened to whole coarse nodes.
int amg_couple_level(pfem_solver *s, AmgWork &W, AmgLevel &L, AmgLevel &C, bool overlap, int cb, const std::vector<double> *nc_of)
{
    // first dof of the coarse node that global coarse dof g belongs to (ranks' blocks are whole nodes)
    std::vector<int64_t> rank_off;
    if (cb > 0 && nc_of) {
        rank_off.assign(nc_of->size() + 1, 0);
        for (size_t q = 0; q < nc_of->size(); ++q) rank_off[q + 1] = rank_off[q] + static_cast<int64_t>((*nc_of)[q]);
    }
    auto node_base = [&](int64_t g) -> int64_t {
        const size_t q = static_cast<size_t>(std::upper_bound(rank_off.begin(), rank_off.end(), g) - rank_off.begin()) - 1;
        return rank_off[q] + (g - rank_off[q]) / cb * cb;
    };
    const PlanRef P = amg_plan(s, L);
    const std::vector<int32_t> &fine_lidx = L.fine ? s->h_send_lidx : L.plan.send_lidx;
    const int64_t n = L.n, n_loc = L.n_loc, n_ghost = n_loc - n, nc = C.n;
    double bad = s->nranks > 52 ? 1.0 : 0.0;
    DevBuf<double> &v = W.vals;
    DevBuf<double> &w = W.svals;
    DevBuf<double> d_mask, d_gm;
    DevBuf<int32_t> d_table;
    // (the ghosts' side runs on the device: their aggregates' distinct global numbers through a sort, not through a host map --
    // at 200^3 the host's map over 79 000 shared dofs was 5 of this function's 7 ms, and a rank of config 5 shares 320 000)
    DevBuf<uint64_t> &gkeys = W.keys, &gskeys = W.skeys, &gukeys = W.ukeys;
    DevBuf<int32_t> &gidx = W.idx, &gsidx = W.skey32;
    DevBuf<int64_t> &gstart = W.start;
    {       // every allocation that sits between this function's collectives, before the first of them -- and agreed on
        int rc = v.reserve(static_cast<size_t>(std::max<int64_t>(n_loc, 1)));
        if (rc == PFEM_OK) rc = w.reserve(static_cast<size_t>(std::max<int64_t>(n_loc, 1)));
        if (rc == PFEM_OK) rc = d_mask.alloc(static_cast<size_t>(std::max<int64_t>(nc, 1)));
        if (rc == PFEM_OK) rc = d_gm.alloc(static_cast<size_t>(std::max<int64_t>(n_ghost, 1)));
        if (rc == PFEM_OK) rc = d_table.alloc(static_cast<size_t>(std::max<int64_t>(n_ghost, 1)));
        if (rc == PFEM_OK) rc = gkeys.reserve(static_cast<size_t>(std::max<int64_t>(n_ghost, 1)));
        if (rc == PFEM_OK) rc = gskeys.reserve(static_cast<size_t>(std::max<int64_t>(n_ghost, 1)));
        if (rc == PFEM_OK) rc = gidx.reserve(static_cast<size_t>(std::max<int64_t>(n_ghost, 1)));
        if (rc == PFEM_OK) rc = gsidx.reserve(static_cast<size_t>(std::max<int64_t>(n_ghost, 1)));
        if (rc == PFEM_OK) rc = W.head.reserve(static_cast<size_t>(n_ghost) + 1);
        if (rc == PFEM_OK) rc = W.rank.reserve(static_cast<size_t>(n_ghost) + 1);
        if (rc == PFEM_OK) rc = gukeys.reserve(static_cast<size_t>(std::max<int64_t>(n_ghost, 1)));
        if (rc == PFEM_OK) rc = gstart.reserve(static_cast<size_t>(n_ghost) + 1);
        if (rc == PFEM_OK && n_ghost > 0) {
            size_t tb = 0;
            if (hipcub::DeviceRadixSort::SortPairs(nullptr, tb, gkeys.p, gskeys.p, gidx.p, gsidx.p, static_cast<int>(n_ghost), 0, 40, s->stream) != hipSuccess) rc = PFEM_ERR_HIP;
            if (rc == PFEM_OK && tb > W.temp.n) { (void)hipStreamSynchronize(s->stream); rc = W.temp.alloc(tb); }
            size_t ts = 0;
            if (rc == PFEM_OK && hipcub::DeviceScan::ExclusiveSum(nullptr, ts, W.head.p, W.rank.p, static_cast<int>(n_ghost + 1), s->stream) != hipSuccess) rc = PFEM_ERR_HIP;
            if (rc == PFEM_OK && ts > W.temp.n) { (void)hipStreamSynchronize(s->stream); rc = W.temp.alloc(ts); }
        }
        PFEM_TRY(amg_agree(s, rc));
    }
    // (timing probes only, PFEM_DEBUG_SELF_PEER: the rank is its own neighbour on every level, and every sum it receives
    // holds its own value twice)
    bool self_peer = false;
    for (int k = 0; k < P.np; ++k) self_peer = self_peer || P.peers[k] == s->rank;
    const double undo = self_peer ? 0.5 : 1.0;
    auto as_id = [undo](double x) { return static_cast<int64_t>(undo * x + 0.5); };
    hipLaunchKernelGGL(k_amg_gid_vector, dim3(grid_for(n_loc)), dim3(kBlock), 0, s->stream, n, n_loc, static_cast<const int32_t *>(L.agg.p), C.gid_off, v.p);
    PFEM_TRY(check_kernel("k_amg_gid_vector"));
    PFEM_TRY(exchange_sum(s, P, v.p, overlap));
    std::vector<double> h_sh(static_cast<size_t>(P.n_send));
    std::vector<uint64_t> h_ug;
    int64_t m_g = 0;
    {
        auto ghosts = [&]() -> int {       // rank-local stretch (its allocations were made above)
            if (P.n_send > 0) {
                hipLaunchKernelGGL(k_pack_send, dim3(grid_for(P.n_send)), dim3(kBlock), 0, s->stream, static_cast<const double *>(v.p), P.send_lidx, P.n_send,
                                   s->d_send.p, static_cast<const CgCtl *>(nullptr));
                PFEM_HIP(hipMemcpyAsync(h_sh.data(), s->d_send.p, sizeof(double) * h_sh.size(), hipMemcpyDeviceToHost, s->stream));
            }
            if (n_ghost > 0) {
                hipLaunchKernelGGL(k_amg_ghost_keys, dim3(grid_for(n_ghost)), dim3(kBlock), 0, s->stream, n_ghost, static_cast<const double *>(v.p + n), undo,
                                   gkeys.p, gidx.p);
                size_t tb = W.temp.n;
                PFEM_HIP(hipcub::DeviceRadixSort::SortPairs(W.temp.p, tb, gkeys.p, gskeys.p, gidx.p, gsidx.p, static_cast<int>(n_ghost), 0, 40, s->stream));
                PFEM_TRY(amg_unique_runs(s, W, gskeys.p, n_ghost, gukeys, gstart, &m_g, false));
                h_ug.resize(static_cast<size_t>(m_g));
                if (m_g > 0) PFEM_HIP(hipMemcpyAsync(h_ug.data(), gukeys.p, sizeof(uint64_t) * h_ug.size(), hipMemcpyDeviceToHost, s->stream));
            }
            PFEM_HIP(hipStreamSynchronize(s->stream));
            return PFEM_OK;
        };
        const int rc = ghosts();
        if (rc != PFEM_OK) bad = 1.0;              // (reaches every rank through the all-reduce of `bad` below)
    }
    // the coarse ghosts: the distinct aggregates of the ghost dofs, ascending by global number; with rigid-body modes whole
    // coarse nodes (the rotation dofs of a neighbour's aggregate are ghosts too).  local index of run k of the sorted ghost
    // dofs: nc + k, or (whole nodes) through a table
    std::vector<int32_t> table;
    C.ghost_gid.clear();
    if (cb > 0) {
        table.resize(h_ug.size());
        int64_t last_base = -1;
        for (size_t k = 0; k < h_ug.size(); ++k) {
            const int64_t g = static_cast<int64_t>(h_ug[k]), b = node_base(g);
            if (b != last_base) {
                for (int q = 0; q < cb; ++q) C.ghost_gid.push_back(b + q);
                last_base = b;
            }
            table[k] = static_cast<int32_t>(nc + static_cast<int64_t>(C.ghost_gid.size()) - cb + (g - b));
        }
    } else {
        C.ghost_gid.assign(h_ug.begin(), h_ug.end());
    }
    C.n_loc = nc + static_cast<int64_t>(C.ghost_gid.size());
    for (int64_t g : C.ghost_gid)
        if (g >= C.gid_off && g < C.gid_off + nc) { bad = 1.0; break; }          // a ghost in one of this rank's own aggregates: plan and ownership disagree
    auto local_of = [&](int64_t g) -> int32_t {
        if (g >= C.gid_off && g < C.gid_off + nc) return static_cast<int32_t>(g - C.gid_off);
        auto it = std::lower_bound(C.ghost_gid.begin(), C.ghost_gid.end(), g);
        if (it == C.ghost_gid.end() || *it != g) { bad = 1.0; return 0; }
        return static_cast<int32_t>(nc + (it - C.ghost_gid.begin()));
    };
    (void)local_of;
    if (n_ghost > 0 && bad == 0.0) {
        if (cb > 0 && !table.empty())
            (void)hipMemcpyAsync(d_table.p, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, s->stream);
        hipLaunchKernelGGL(k_amg_ghost_agg, dim3(grid_for(n_ghost)), dim3(kBlock), 0, s->stream, n_ghost, static_cast<const int32_t *>(gsidx.p),
                           static_cast<const int32_t *>(W.head.p), static_cast<const int32_t *>(W.rank.p),
                           cb > 0 ? static_cast<const int32_t *>(d_table.p) : static_cast<const int32_t *>(nullptr), static_cast<int32_t>(nc), L.agg.p + n);
    }
    // holder sets of this rank's own aggregates: the ranks its owned fine dofs are shared with
    const uint64_t me = 1ull << (s->rank & 63);
    std::vector<uint64_t> m_own(static_cast<size_t>(std::max<int64_t>(nc, 1)), 0);
    std::vector<double> mask_c(static_cast<size_t>(std::max<int64_t>(nc, 1)), 0.0);
    {
        for (int k = 0; k < P.np; ++k)
            for (int64_t i = P.peer_off[k]; i < P.peer_off[k + 1]; ++i)
                if (fine_lidx[static_cast<size_t>(i)] < n) {
                    const int64_t c = as_id(h_sh[static_cast<size_t>(i)]) - C.gid_off;
                    if (c < 0 || c >= nc) { bad = 1.0; continue; }
                    m_own[static_cast<size_t>(c)] |= me | (1ull << (P.peers[k] & 63));
                }
        if (cb > 0)                // every dof of a coarse node is held by the holders of the node
            for (int64_t c0 = 0; c0 + cb <= nc; c0 += cb) {
                uint64_t u = 0;
                for (int k = 0; k < cb; ++k) u |= m_own[static_cast<size_t>(c0 + k)];
                for (int k = 0; k < cb; ++k) m_own[static_cast<size_t>(c0 + k)] = u;
            }
        for (int64_t c = 0; c < nc; ++c) mask_c[static_cast<size_t>(c)] = static_cast<double>(m_own[static_cast<size_t>(c)]);
    }
    PFEM_HIP(hipMemcpyAsync(d_mask.p, mask_c.data(), sizeof(double) * mask_c.size(), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_amg_mask_vector, dim3(grid_for(n_loc)), dim3(kBlock), 0, s->stream, n, n_loc, static_cast<const int32_t *>(L.agg.p),
                       static_cast<const double *>(d_mask.p), w.p);
    PFEM_TRY(check_kernel("k_amg_mask_vector"));
    PFEM_TRY(exchange_sum(s, P, w.p, overlap));
    // the holder sets of the ghosts' aggregates, as their owners sent them: one per run of the sorted ghost dofs
    std::vector<double> h_gm(static_cast<size_t>(m_g), 0.0);
    if (m_g > 0 && bad == 0.0) {
        hipLaunchKernelGGL(k_amg_ghost_masks, dim3(grid_for(m_g)), dim3(kBlock), 0, s->stream, m_g, static_cast<const int64_t *>(gstart.p),
                           static_cast<const int32_t *>(gsidx.p), static_cast<const double *>(w.p + n), d_gm.p);
        if (hipMemcpyAsync(h_gm.data(), d_gm.p, sizeof(double) * h_gm.size(), hipMemcpyDeviceToHost, s->stream) != hipSuccess) bad = 1.0;
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess) bad = 1.0;
    std::vector<uint64_t> m_gh(C.ghost_gid.size(), 0);
    for (size_t k = 0; k < h_gm.size() && bad == 0.0; ++k) {
        const uint64_t mk = static_cast<uint64_t>(undo * h_gm[k] + 0.5);
        if (!(mk & me)) { bad = 1.0; break; }                   // the owner does not know this rank holds the dof
        if (cb > 0) {
            const size_t b0 = static_cast<size_t>(table[k] - nc) / static_cast<size_t>(cb) * static_cast<size_t>(cb);
            for (int q = 0; q < cb; ++q) m_gh[b0 + static_cast<size_t>(q)] = mk;
        } else {
            m_gh[k] = mk;
        }
    }
    // the coarse level's send list: per neighbour (ascending rank) the coarse dofs shared with it, ascending by global number
    // on both sides -- ghosts below this rank's own numbers, its own shared aggregates, ghosts above
    AmgPlan &Q = C.plan;
    Q.peers.clear();
    Q.peer_off.assign(1, 0);
    Q.send_lidx.clear();
    {
        std::vector<std::vector<int32_t>> per(64);
        auto emit = [&](int32_t lc, uint64_t mask) {
            while (mask) {
                const int q = __builtin_ctzll(mask);
                mask &= mask - 1;
                if (q == (s->rank & 63) && !self_peer) continue;
                per[static_cast<size_t>(q)].push_back(lc);
            }
        };
        const size_t split = static_cast<size_t>(std::lower_bound(C.ghost_gid.begin(), C.ghost_gid.end(), C.gid_off) - C.ghost_gid.begin());
        for (size_t k = 0; k < split; ++k) emit(static_cast<int32_t>(nc + static_cast<int64_t>(k)), m_gh[k]);
        for (int64_t c = 0; c < nc; ++c)
            if (m_own[static_cast<size_t>(c)]) emit(static_cast<int32_t>(c), m_own[static_cast<size_t>(c)]);
        for (size_t k = split; k < m_gh.size(); ++k) emit(static_cast<int32_t>(nc + static_cast<int64_t>(k)), m_gh[k]);
        for (int q = 0; q < s->nranks && q < 64; ++q) {
            if (per[static_cast<size_t>(q)].empty()) continue;
            Q.send_lidx.insert(Q.send_lidx.end(), per[static_cast<size_t>(q)].begin(), per[static_cast<size_t>(q)].end());
            Q.peers.push_back(q);
            Q.peer_off.push_back(static_cast<int64_t>(Q.send_lidx.size()));
        }
    }
    PFEM_TRY(amg_allreduce_host(s, &bad, 1));
    if (bad > 0.0) return kAmgRetryBlock;
    auto rest = [&]() -> int {             // rank-local from here on; its verdict is agreed on below
    if (static_cast<size_t>(Q.send_lidx.size()) > s->d_send.n) {          // (more pairs than on the matrix's level can only come with many holders per dof)
        PFEM_HIP(hipStreamSynchronize(s->stream));
        if (s->comm_stream) PFEM_HIP(hipStreamSynchronize(s->comm_stream));
        DevBuf<double> a, b;
        PFEM_TRY(a.alloc(Q.send_lidx.size()));
        PFEM_TRY(b.alloc(Q.send_lidx.size()));
        s->d_send.swap(a);
        s->d_recv.swap(b);
        s->mgraph.invalidate();            // (a captured Jacobi iteration points at the old buffers)
    }
    std::vector<int32_t> sh_lidx, sh_ptr, sh_src;
    plan_unpack_lists(s->rank, static_cast<int>(Q.peers.size()), Q.peers.data(), Q.peer_off.data(), Q.send_lidx, sh_lidx, sh_ptr, sh_src);
    Q.n_send = static_cast<int64_t>(Q.send_lidx.size());
    Q.n_sh = static_cast<int64_t>(sh_lidx.size());
    PFEM_TRY(Q.d_send_lidx.alloc(std::max<size_t>(Q.send_lidx.size(), 1)));
    PFEM_TRY(Q.d_sh_lidx.alloc(std::max<size_t>(sh_lidx.size(), 1)));
    PFEM_TRY(Q.d_sh_ptr.alloc(sh_ptr.size()));
    PFEM_TRY(Q.d_sh_src.alloc(std::max<size_t>(sh_src.size(), 1)));
    if (!Q.send_lidx.empty()) PFEM_HIP(hipMemcpyAsync(Q.d_send_lidx.p, Q.send_lidx.data(), sizeof(int32_t) * Q.send_lidx.size(), hipMemcpyHostToDevice, s->stream));
    if (!sh_lidx.empty()) PFEM_HIP(hipMemcpyAsync(Q.d_sh_lidx.p, sh_lidx.data(), sizeof(int32_t) * sh_lidx.size(), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipMemcpyAsync(Q.d_sh_ptr.p, sh_ptr.data(), sizeof(int32_t) * sh_ptr.size(), hipMemcpyHostToDevice, s->stream));
    if (!sh_src.empty()) PFEM_HIP(hipMemcpyAsync(Q.d_sh_src.p, sh_src.data(), sizeof(int32_t) * sh_src.size(), hipMemcpyHostToDevice, s->stream));
    PFEM_TRY(Q.d_row_sh.alloc(static_cast<size_t>(std::max<int64_t>(C.n_loc, 1))));
    PFEM_HIP(hipMemsetAsync(Q.d_row_sh.p, 0xff, sizeof(int32_t) * static_cast<size_t>(std::max<int64_t>(C.n_loc, 1)), s->stream));
    if (Q.n_sh > 0)
        hipLaunchKernelGGL(k_amg_fill_row_sh, dim3(grid_for(Q.n_sh)), dim3(kBlock), 0, s->stream, Q.n_sh, static_cast<const int32_t *>(Q.d_sh_lidx.p), Q.d_row_sh.p);
    PFEM_TRY(check_kernel("k_amg_fill_row_sh"));
    PFEM_HIP(hipStreamSynchronize(s->stream));           // (the host vectors go out of scope)
    return PFEM_OK;
    };
    return amg_agree(s, rest());
}

int amg_build_levels(pfem_solver *s, Amg &M, AmgWork &W, bool coupled, bool overlap);
int amg_finish_levels(pfem_solver *s, Amg &M, bool coupled);

// global number of every local dof of a coupled level, on the device
int amg_level_gids(pfem_solver *s, AmgLevel &L)
{
    std::vector<int32_t> gid(static_cast<size_t>(std::max<int64_t>(L.n_loc, 1)), 0);
    for (int64_t i = 0; i < L.n; ++i) gid[static_cast<size_t>(i)] = static_cast<int32_t>(L.gid_off + i);
    for (size_t g = 0; g < L.ghost_gid.size(); ++g) gid[static_cast<size_t>(L.n) + g] = static_cast<int32_t>(L.ghost_gid[g]);
    PFEM_TRY(L.gid.alloc(gid.size()));
    PFEM_HIP(hipMemcpyAsync(L.gid.p, gid.data(), sizeof(int32_t) * gid.size(), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

// the values of the replicated level: every rank's share of the distributed level's entries, concatenated by an
// all-reduce over a zeroed buffer, then summed entry by entry in a fixed order (the Galerkin gather kernel does it)
int amg_replicate_values(pfem_solver *s, Amg &M)
{
    AmgLevel &C = *M.lev.back();
    AmgLevel &R0 = *M.rep->lev[0];
    PFEM_HIP(hipMemsetAsync(M.rep_buf.p, 0, sizeof(double) * static_cast<size_t>(M.rep_total), s->stream));
    if (M.rep_mine > 0)
        hipLaunchKernelGGL(k_amg_pack_values, dim3(grid_for(M.rep_mine)), dim3(kBlock), 0, s->stream, M.rep_mine, static_cast<const double *>(C.vals.p),
                           static_cast<const int32_t *>(M.rep_pack_slot.p), M.rep_buf.p + M.rep_off);
    PFEM_TRY(s->comm->allreduce(M.rep_buf.p, M.rep_total, s->stream));
    hipLaunchKernelGGL(k_amg_galerkin, dim3(grid_for(C.nnz_c)), dim3(kBlock), 0, s->stream, C.nnz_c, static_cast<const int64_t *>(C.src_ptr.p),
                       static_cast<const int32_t *>(C.src_slot.p), static_cast<const int64_t *>(C.dst_slot.p),
                       static_cast<const double *>(M.rep_buf.p), R0.vals.p);
    PFEM_TRY(check_kernel("replicated level values"));
    return PFEM_OK;
}

// Coupled hierarchy: level C (n_global rows over all ranks) is small enough for every rank to hold it assembled.  The
// ranks' entries (global row, global column) are concatenated, sorted and merged into the replicated level's pattern;
// the maps of that merge serve every solve (amg_replicate_values).  From there on an ordinary one-rank hierarchy,
// identical on all ranks (same input, same deterministic kernels).  Collective.
int amg_replicate(pfem_solver *s, Amg &M, AmgWork &W, AmgLevel &C, int64_t n_global, bool overlap)
{
    PFEM_TRY(amg_level_gids(s, C));
    // entries of every rank
    std::vector<double> cnt(static_cast<size_t>(s->nranks) * 2, 0.0);         // [entries | nodes] of every rank
    cnt[static_cast<size_t>(s->rank)] = static_cast<double>(C.nnz);
    cnt[static_cast<size_t>(s->nranks + s->rank)] = static_cast<double>(C.n_nodes);
    PFEM_TRY(amg_allreduce_host(s, cnt.data(), 2 * s->nranks));
    int64_t total = 0, off = 0, node_off = 0, nodes_total = 0;
    for (int q = 0; q < s->nranks; ++q) {
        if (q < s->rank) { off += static_cast<int64_t>(cnt[static_cast<size_t>(q)]); node_off += static_cast<int64_t>(cnt[static_cast<size_t>(s->nranks + q)]); }
        total += static_cast<int64_t>(cnt[static_cast<size_t>(q)]);
        nodes_total += static_cast<int64_t>(cnt[static_cast<size_t>(s->nranks + q)]);
    }
    if (total > INT_MAX / 2) return PFEM_ERR_ARG;
    M.rep_total = total;
    M.rep_off = off;
    M.rep_mine = C.nnz;
    PFEM_TRY(M.rep_buf.alloc(static_cast<size_t>(std::max<int64_t>(2 * total, 2 * n_global))));
    PFEM_TRY(M.rep_pack_slot.alloc(static_cast<size_t>(std::max<int64_t>(C.nnz, 1))));
    PFEM_HIP(hipMemsetAsync(M.rep_buf.p, 0, sizeof(double) * static_cast<size_t>(2 * total), s->stream));
    if (C.n_loc > 0)
        hipLaunchKernelGGL(k_amg_emit_global_entries, dim3(grid_for(C.n_loc)), dim3(kBlock), 0, s->stream, amg_sell(s, C, C.n_loc),
                           static_cast<const int64_t *>(C.rowptr.p), static_cast<const int32_t *>(C.gid.p), M.rep_buf.p + off, M.rep_buf.p + total + off,
                           M.rep_pack_slot.p);
    PFEM_TRY(check_kernel("k_amg_emit_global_entries"));
    PFEM_TRY(s->comm->allreduce(M.rep_buf.p, 2 * total, s->stream));
    // merged pattern + the maps of the merge (kept in C's Galerkin fields: C has no distributed level below it)
    DevBuf<uint64_t> &keys = W.keys;
    DevBuf<uint64_t> ukeys;
    DevBuf<int32_t> &pos = W.slots;
    PFEM_TRY(keys.reserve(static_cast<size_t>(total)));
    PFEM_TRY(pos.reserve(static_cast<size_t>(total)));
    PFEM_TRY(C.src_slot.alloc(static_cast<size_t>(total)));
    hipLaunchKernelGGL(k_amg_keys_from_pairs, dim3(grid_for(total)), dim3(kBlock), 0, s->stream, total, static_cast<const double *>(M.rep_buf.p),
                       static_cast<const double *>(M.rep_buf.p + total), keys.p, pos.p);
    PFEM_TRY(check_kernel("k_amg_keys_from_pairs"));
    int64_t nnz_rep = 0;
    PFEM_TRY(amg_pattern_from_keys(s, W, total, C.src_slot.p, C.src_ptr, ukeys, &nnz_rep));
    C.nnz_c = nnz_rep;
    M.rep.reset(new (std::nothrow) Amg());
    if (!M.rep) return PFEM_ERR_NOMEM;
    Amg &R = *M.rep;
    R.cheb_degree = M.cheb_degree;
    R.fine_degree = 0;                     // its first level is a coarse level of the whole hierarchy
    R.eig_ratio = M.eig_ratio;
    R.coarse_scale = M.coarse_scale;
    R.coarsest_sweeps = M.coarsest_sweeps;
    std::unique_ptr<AmgLevel> R0p(new (std::nothrow) AmgLevel());
    if (!R0p) return PFEM_ERR_NOMEM;
    AmgLevel &R0 = *R0p;
    R0.n = R0.n_loc = n_global;
    R0.bs = C.bs;
    R0.n_nodes = C.bs > 1 ? nodes_total : n_global;
    PFEM_TRY(amg_store_pattern(s, W, ukeys.p, nnz_rep, R0, C.dst_slot));
    if (C.bs > 1) {        // dofs of one node stay together on the replicated levels too: node and component of every dof, by global number
        double *node_g = M.rep_buf.p, *comp_g = M.rep_buf.p + n_global;
        PFEM_HIP(hipMemsetAsync(M.rep_buf.p, 0, sizeof(double) * static_cast<size_t>(2 * n_global), s->stream));
        if (C.n > 0)
            hipLaunchKernelGGL(k_amg_emit_global_nodes, dim3(grid_for(C.n)), dim3(kBlock), 0, s->stream, C.n, static_cast<const int32_t *>(C.gid.p),
                               static_cast<const int32_t *>(C.node_of.p), static_cast<const int32_t *>(C.comp_of.p), node_off, node_g, comp_g);
        PFEM_TRY(s->comm->allreduce(M.rep_buf.p, 2 * n_global, s->stream));
        PFEM_TRY(R0.node_of.alloc(static_cast<size_t>(n_global)));
        PFEM_TRY(R0.comp_of.alloc(static_cast<size_t>(n_global)));
        hipLaunchKernelGGL(k_amg_round_to_int, dim3(grid_for(n_global)), dim3(kBlock), 0, s->stream, n_global, static_cast<const double *>(node_g), R0.node_of.p);
        hipLaunchKernelGGL(k_amg_round_to_int, dim3(grid_for(n_global)), dim3(kBlock), 0, s->stream, n_global, static_cast<const double *>(comp_g), R0.comp_of.p);
        PFEM_TRY(check_kernel("replicated level nodes"));
    }
    if (C.dim > 0 && C.cen.p) {          // rigid-body modes go on below: the replicated level's nodes are the ranks' coarse nodes, rank after rank
        const int64_t n_nodes_g = n_global / C.bs;
        R0.dim = C.dim;
        R0.n_nodes = n_nodes_g;
        PFEM_TRY(R0.cen.alloc(static_cast<size_t>(3 * n_nodes_g)));
        PFEM_HIP(hipMemsetAsync(R0.cen.p, 0, sizeof(double) * static_cast<size_t>(3 * n_nodes_g), s->stream));
        if (C.n_nodes > 0)
            hipLaunchKernelGGL(k_rbm_emit_global_cen, dim3(grid_for(C.n_nodes)), dim3(kBlock), 0, s->stream, C.n_nodes, C.gid_off / C.bs, C.n_loc / C.bs,
                               static_cast<const double *>(C.cen.p), n_nodes_g, R0.cen.p);
        PFEM_TRY(check_kernel("k_rbm_emit_global_cen"));
        PFEM_TRY(s->comm->allreduce(R0.cen.p, 3 * n_nodes_g, s->stream));
    }
    // a level of the brick path (its positions are global already: the same verdict on every rank): the replicated level takes
    // them as they are -- one all-reduce of a number per dof; no coordinates, no sorts on the host
    const bool from_pos = (C.lat_global || C.lat_split) && C.lattice && C.bs == 1 && C.hint.p;
    if (from_pos) {
        DevBuf<double> gp;
        int rc = gp.alloc(static_cast<size_t>(std::max<int64_t>(n_global, 1)));
        if (rc == PFEM_OK) rc = R0.hint.alloc(static_cast<size_t>(std::max<int64_t>(n_global, 1)));
        PFEM_TRY(amg_agree(s, rc));
        PFEM_HIP(hipMemsetAsync(gp.p, 0, sizeof(double) * static_cast<size_t>(n_global), s->stream));
        if (C.n > 0)
            hipLaunchKernelGGL(k_lat_emit_global_pos, dim3(grid_for(C.n)), dim3(kBlock), 0, s->stream, C.n, static_cast<const int32_t *>(C.gid.p),
                               static_cast<const int32_t *>(C.hint.p), gp.p);
        PFEM_TRY(check_kernel("k_lat_emit_global_pos"));
        PFEM_TRY(s->comm->allreduce(gp.p, n_global, s->stream));
        hipLaunchKernelGGL(k_amg_round_to_int, dim3(grid_for(n_global)), dim3(kBlock), 0, s->stream, n_global, static_cast<const double *>(gp.p), R0.hint.p);
        PFEM_TRY(check_kernel("replicated level positions"));
        // The padding that kept bricks inside one owner has no purpose on a level every rank holds whole, and its gaps cost:
        // with them config 5 on 8 ranks coarsened 140 000 -> 21 250 -> 6 282 -> 1 557 -> ... in ten levels and 16 iterations instead of
        // 140 000 -> 17 500 -> 2 366 -> 343 -> 64 and 14.  The positions are closed up: rank among the OCCUPIED positions per axis.
        DevBuf<int32_t> used;
        PFEM_TRY(used.alloc(3 * 1024));
        PFEM_HIP(hipMemsetAsync(used.p, 0, sizeof(int32_t) * 3 * 1024, s->stream));
        hipLaunchKernelGGL(k_lat_mark_used, dim3(grid_for(n_global)), dim3(kBlock), 0, s->stream, n_global, static_cast<const int32_t *>(R0.hint.p), used.p);
        std::vector<int32_t> h_used(3 * 1024);
        PFEM_HIP(hipMemcpyAsync(h_used.data(), used.p, sizeof(int32_t) * h_used.size(), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));        // (gp goes out of scope)
        R0.lattice = true;
        for (int d = 0; d < 3; ++d) {
            int next = 0;
            for (int p = 0; p < 1024; ++p) {
                const bool u = h_used[static_cast<size_t>(1024 * d + p)] != 0;
                h_used[static_cast<size_t>(1024 * d + p)] = next;
                if (u) ++next;
            }
            R0.lat_hi[d] = std::max(next - 1, 0);
        }
        PFEM_HIP(hipMemcpyAsync(used.p, h_used.data(), sizeof(int32_t) * h_used.size(), hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_lat_remap, dim3(grid_for(n_global)), dim3(kBlock), 0, s->stream, n_global, static_cast<const int32_t *>(R0.hint.p),
                           static_cast<const int32_t *>(used.p), R0.hint.p);
        PFEM_TRY(check_kernel("replicated level positions closed up"));
        PFEM_HIP(hipStreamSynchronize(s->stream));        // (used goes out of scope)
        R0.lat_axis = C.lat_axis;
    }
    // (decided by all ranks together: a rank that owns nodes of this level but carries no corners for them -- its mesh has
    // no lattice -- rules the lattice out for everybody; a rank that owns nothing just takes part)
    const bool from_cen = R0.dim > 0 && R0.cen.p;            // (with rigid-body modes the centroids are at hand, gathered above)
    double no_xyz = (from_pos || (C.n_nodes > 0 && !C.xyz.p && !from_cen)) ? 1.0 : 0.0;
    PFEM_TRY(amg_allreduce_host(s, &no_xyz, 1));
    if (no_xyz == 0.0) {
        // the replicated level's own lattice, from the corners the ranks' aggregates carry (global node numbers: dofs when
        // every dof is its own node, else the node numbers handed out above); small: found on the host
        const int64_t n_nodes_g = R0.n_nodes;
        DevBuf<double> gx;
        PFEM_TRY(gx.alloc(static_cast<size_t>(3 * n_nodes_g)));
        PFEM_HIP(hipMemsetAsync(gx.p, 0, sizeof(double) * static_cast<size_t>(3 * n_nodes_g), s->stream));
        if (C.n_nodes > 0 && C.xyz.p)
            hipLaunchKernelGGL(k_amg_emit_global_xyz, dim3(grid_for(C.n_nodes)), dim3(kBlock), 0, s->stream, C.n_nodes,
                               C.bs > 1 ? static_cast<const int32_t *>(nullptr) : static_cast<const int32_t *>(C.gid.p), node_off,
                               static_cast<const double *>(C.xyz.p), n_nodes_g, gx.p);
        PFEM_TRY(s->comm->allreduce(gx.p, 3 * n_nodes_g, s->stream));
        std::vector<double> h(static_cast<size_t>(3 * n_nodes_g));
        PFEM_HIP(hipMemcpyAsync(h.data(), from_cen ? R0.cen.p : gx.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        std::vector<double> u[3];
        bool ok = true;
        int64_t prod = 1;
        // (centroids are means: the same position comes out with different last bits from bricks of 8 and of 12 nodes, so
        // values closer than 1e-9 of the axis' extent count as one; corners are exact and never merge)
        double tol[3] = {0.0, 0.0, 0.0};
        for (int d = 0; d < 3 && ok; ++d) {
            u[d].assign(h.begin() + d * n_nodes_g, h.begin() + (d + 1) * n_nodes_g);
            std::sort(u[d].begin(), u[d].end());
            if (from_cen && !u[d].empty()) tol[d] = 1e-9 * (u[d].back() - u[d].front());
            const double t = tol[d];
            u[d].erase(std::unique(u[d].begin(), u[d].end(), [t](double a, double b) { return b - a <= t; }), u[d].end());
            ok = !u[d].empty() && u[d].size() <= 1024;
            prod *= static_cast<int64_t>(u[d].size());
        }
        if (ok && prod <= 2 * std::max<int64_t>(n_nodes_g, 1)) {
            std::vector<int32_t> pos(static_cast<size_t>(n_nodes_g));
            for (int64_t i = 0; i < n_nodes_g; ++i) {
                int32_t p = 0;
                for (int d = 0; d < 3; ++d) {
                    const double v = h[static_cast<size_t>(d * n_nodes_g + i)];
                    size_t k = static_cast<size_t>(std::lower_bound(u[d].begin(), u[d].end(), v - tol[d]) - u[d].begin());
                    if (k >= u[d].size()) k = u[d].size() - 1;
                    p |= static_cast<int32_t>(k) << (10 * d);
                }
                pos[static_cast<size_t>(i)] = p;
            }
            PFEM_TRY(R0.hint.alloc(pos.size()));
            PFEM_HIP(hipMemcpyAsync(R0.hint.p, pos.data(), sizeof(int32_t) * pos.size(), hipMemcpyHostToDevice, s->stream));
            PFEM_HIP(hipStreamSynchronize(s->stream));
            R0.lattice = true;
            for (int d = 0; d < 3; ++d) R0.lat_hi[d] = static_cast<int>(u[d].size()) - 1;
            // (node bricks across the ranks leave a full tensor grid of centroids behind: the replicated levels go on in bricks)
            if (from_cen && prod == n_nodes_g) {
                R0.lat_full = true;
                for (int d = 0; d < 3; ++d) { R0.lat_tlo[d] = 0; R0.lat_thi[d] = R0.lat_hi[d]; }
                if (C.lat_nodes_global) R0.lat_axis = C.lat_axis;          // (the turn of the axes goes on where the distributed levels left it)
            }
        }
    }
    PFEM_HIP(hipStreamSynchronize(s->stream));        // (ukeys goes out of scope)
    R.lev.push_back(std::move(R0p));
    PFEM_TRY(amg_replicate_values(s, M));             // the next strength graph needs the values
    PFEM_TRY(amg_build_levels(s, R, W, false, overlap));
    PFEM_TRY(amg_finish_levels(s, R, false));
    PFEM_TRY(M.bx_glob.alloc(static_cast<size_t>(std::max<int64_t>(n_global, 2 * kAmgDense))));
    return PFEM_OK;
}

// ---- rigid-body modes (pfem_amg_rbm.hpp) ------------------------------------------------------------------------------
// WHY.  With one coarse dof per component a coarse function is piecewise constant: it cannot follow the rotation of a
// cross-section, which is what bending is, so the slender beam of config 4 needed 169 iterations where the Poisson cube
// needs 12.  tools/probe_rbm.py (scipy, geometric bricks): translations only 165 iterations on the 16x96x16 beam; with the
// three rotations about every aggregate's centroid as further coarse dofs 16-23, operator complexity 1.47 instead of 1.13;
// smoothing the prolongator once more gets 14 at a complexity of 2.28 and is not worth its SpMVs.  PETSc: the near null
// space PCGAMG is given through MatSetNearNullSpace / PCSetCoordinates (tetraelasticityparallelimpl1.F:894-902 solves with
// whatever -pc_type says).
constexpr int kAmgLastLevel = -7702;        // internal: the coarsening has stalled, the current level is the last one

#define PFEM_RBM_DISPATCH(FBV, DIMV, ...)                                                         \
    do {                                                                                          \
        if ((DIMV) == 3 && (FBV) == 3) { constexpr int FB = 3, DIM = 3; __VA_ARGS__; }            \
        else if ((DIMV) == 3 && (FBV) == 6) { constexpr int FB = 6, DIM = 3; __VA_ARGS__; }       \
        else if ((DIMV) == 2 && (FBV) == 2) { constexpr int FB = 2, DIM = 2; __VA_ARGS__; }       \
        else { constexpr int FB = 3, DIM = 2; __VA_ARGS__; }                                      \
    } while (0)

inline void amg_rbm_galerkin(pfem_solver *s, const AmgLevel &L, AmgLevel &C, const SellDev &A)
{
    if (L.nnz_c < 1) return;
    const SellDev Cs{C.n_loc, (C.n_loc + 63) / 64, C.slice_off.p, C.rowlen.p, C.cols.p, C.vals.p};
    PFEM_RBM_DISPATCH(L.bs, L.dim, hipLaunchKernelGGL((k_rbm_galerkin<FB, DIM>), dim3(grid_for(L.nnz_c * kRbmLanes)), dim3(kBlock), 0, s->stream, L.nnz_c,
        static_cast<const int64_t *>(L.src_ptr.p), static_cast<const int32_t *>(L.src_slot.p), A, static_cast<const int64_t *>(L.gptr.p),
        static_cast<const int32_t *>(L.gcol.p), static_cast<const int32_t *>(L.brow.p), static_cast<const double *>(L.roff.p), A.n_rows / L.bs, Cs,
        static_cast<const int64_t *>(C.gptr.p), static_cast<const int32_t *>(C.brow.p), static_cast<const int32_t *>(C.gcol.p), C.n / C.bs));
}

// the level below L from the aggregates of its nodes (node_agg, na of them): centroids and offsets, member lists, the
// coarse block pattern with the maps of the numeric product, the coarse matrix in wave-sliced storage, one numeric product.
// Several ranks (coupled): the aggregates are the owned nodes'; the ghost nodes learn theirs, the centroids and the rotation
// verdicts from the owners (amg_couple_level + two more sum-exchanges); everything else runs over all local nodes.
int amg_couple_level(pfem_solver *s, AmgWork &W, AmgLevel &L, AmgLevel &C, bool overlap, int cb, const std::vector<double> *nc_of);
int amg_rbm_level(pfem_solver *s, Amg &M, AmgWork &W, AmgLevel &L, DevBuf<int32_t> &node_agg, int64_t na, const int32_t *hint,
                  bool on_lattice, const int lat_hi[3], int lat_axis, AmgPhaseClock &phase, int l, bool coupled, bool overlap, double *n_global,
                  const int *brick_box = nullptr /* node bricks (one rank): bricks along x, y, z of the box the aggregates are numbered in */)
{
    DevBuf<char> &temp = W.temp;
    const int64_t R = coupled ? L.n_loc : L.n;
    const int64_t nn_own = L.n_nodes, nn = R / L.bs;         // owned nodes / all local nodes (the stride of the per-node arrays)
    const int cb = L.dim + (L.dim == 3 ? 3 : 1);
    const int64_t nc = na * cb;
    std::vector<double> nc_of;
    double nc_global = static_cast<double>(nc);
    if (coupled) {
        nc_of.assign(static_cast<size_t>(s->nranks), 0.0);
        nc_of[static_cast<size_t>(s->rank)] = static_cast<double>(nc);
        PFEM_TRY(amg_allreduce_host(s, nc_of.data(), s->nranks));
        nc_global = 0.0;
        for (double v : nc_of) nc_global += v;
        if (nc_global < 1.0 || nc_global * 10.0 > *n_global * 8.0 || nc_global > static_cast<double>(INT_MAX - 8)) return kAmgLastLevel;
    } else if (na < 1 || nc * 10 > L.n * 8 || nc > INT_MAX - 8) {
        return kAmgLastLevel;
    }
    // Several ranks: the stretches between two collectives run rank-locally (allocations, size limits); their verdicts are
    // agreed (amg_agree) before the next collective, so that no rank leaves the others waiting in an exchange.
    auto agreed = [&](int rc) { return coupled ? amg_agree(s, rc) : rc; };
    L.nc = nc;
    std::unique_ptr<AmgLevel> Cp(new (std::nothrow) AmgLevel());
    auto stretch_a = [&]() -> int {
    if (!Cp) return PFEM_ERR_NOMEM;
    PFEM_TRY(L.node_agg.alloc(static_cast<size_t>(std::max<int64_t>(nn, 1))));
    if (nn_own > 0) PFEM_HIP(hipMemcpyAsync(L.node_agg.p, node_agg.p, sizeof(int32_t) * static_cast<size_t>(nn_own), hipMemcpyDeviceToDevice, s->stream));
    PFEM_TRY(L.agg.alloc(static_cast<size_t>(std::max<int64_t>(R, 1))));
    hipLaunchKernelGGL(k_rbm_dof_agg, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, L.n, L.bs, cb, static_cast<const int32_t *>(L.node_agg.p), L.agg.p);
    PFEM_TRY(check_kernel("k_rbm_dof_agg"));
    return PFEM_OK;
    };
    PFEM_TRY(agreed(stretch_a()));
    AmgLevel &C = *Cp;
    C.n = C.n_loc = nc;
    if (coupled) {
        for (int q = 0; q < s->rank; ++q) C.gid_off += static_cast<int64_t>(nc_of[static_cast<size_t>(q)]);
        const int rc = amg_couple_level(s, W, L, C, overlap, cb, &nc_of);          // (ends in an agreed verdict itself)
        if (rc != PFEM_OK) return rc;
    }
    const int64_t nc_loc = C.n_loc, na_loc = nc_loc / cb;
    DevBuf<int32_t> &rot_ok = W.flag;
    DevBuf<double> &cv = W.vals, &cw = W.svals;
    auto stretch_b = [&]() -> int {
    if (coupled) {
        hipLaunchKernelGGL(k_rbm_node_agg_from_dofs, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, L.bs, cb, static_cast<const int32_t *>(L.agg.p), L.node_agg.p);
        PFEM_TRY(check_kernel("k_rbm_node_agg_from_dofs"));
    }
    C.bs = cb;
    C.dim = L.dim;
    C.n_nodes = na;
    PFEM_TRY(C.node_of.alloc(static_cast<size_t>(std::max<int64_t>(nc_loc, 1))));
    PFEM_TRY(C.comp_of.alloc(static_cast<size_t>(std::max<int64_t>(nc_loc, 1))));
    hipLaunchKernelGGL(k_rbm_node_comp, dim3(grid_for(nc_loc)), dim3(kBlock), 0, s->stream, nc_loc, cb, C.node_of.p, C.comp_of.p);
    PFEM_TRY(check_kernel("k_rbm_node_comp"));
    if (hint) {                     // the next level pairs on along the same curve / on the coarser lattice
        C.lattice = L.lattice && on_lattice;
        for (int d = 0; d < 3; ++d) C.lat_hi[d] = lat_hi[d];
        C.lat_axis = lat_axis;
        PFEM_TRY(C.hint.alloc(static_cast<size_t>(std::max<int64_t>(na, 1))));
        if (na > 0) PFEM_HIP(hipMemcpyAsync(C.hint.p, hint, sizeof(int32_t) * static_cast<size_t>(na), hipMemcpyDeviceToDevice, s->stream));
    }
    // ---- member nodes of every coarse node (ghosts included), ascending
    PFEM_TRY(amg_member_lists(s, W, L, L.node_agg.p, nn, na_loc, 32, true));
    // ---- centroids (the coarse nodes' coordinates) and the nodes' offsets from them
    {
        PFEM_TRY(rot_ok.reserve(static_cast<size_t>(na_loc) + 1));
        PFEM_TRY(C.cen.alloc(static_cast<size_t>(std::max<int64_t>(3 * na_loc, 1))));
        PFEM_TRY(L.roff.alloc(static_cast<size_t>(std::max<int64_t>(3 * nn, 1))));
        PFEM_HIP(hipMemsetAsync(C.cen.p, 0, sizeof(double) * static_cast<size_t>(std::max<int64_t>(3 * na_loc, 1)), s->stream));
        hipLaunchKernelGGL(k_rbm_centroids, dim3(grid_for(na)), dim3(kBlock), 0, s->stream, na, L.dim, nn, static_cast<const int32_t *>(L.mem_ptr.p),
                           static_cast<const int32_t *>(L.mem_idx.p), static_cast<const double *>(L.cen.p), na_loc, C.cen.p, rot_ok.p, L.bs == L.dim ? 1 : 0);
        PFEM_TRY(check_kernel("k_rbm_centroids"));
        if (!coupled) {
            hipLaunchKernelGGL(k_rbm_offsets, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, static_cast<const int32_t *>(L.node_agg.p),
                               static_cast<const double *>(L.cen.p), na_loc, static_cast<const double *>(C.cen.p), static_cast<const int32_t *>(rot_ok.p), L.roff.p);
        } else {
            PFEM_TRY(cv.reserve(static_cast<size_t>(std::max<int64_t>(R, 1))));
            PFEM_TRY(cw.reserve(static_cast<size_t>(std::max<int64_t>(R, 1))));
            hipLaunchKernelGGL(k_rbm_centroid_vectors, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, nn_own, L.bs, L.dim,
                               static_cast<const int32_t *>(L.node_agg.p), na_loc, static_cast<const double *>(C.cen.p), static_cast<const int32_t *>(rot_ok.p), cv.p, cw.p);
        }
        PFEM_TRY(check_kernel("k_rbm_offsets / k_rbm_centroid_vectors"));
    }
    return PFEM_OK;
    };
    PFEM_TRY(agreed(stretch_b()));
    if (coupled) {
        const PlanRef P = amg_plan(s, L);
        PFEM_TRY(exchange_sum(s, P, cv.p, overlap));
        PFEM_TRY(exchange_sum(s, P, cw.p, overlap));
    }
    auto stretch_c = [&]() -> int {
    if (coupled) {
        const PlanRef P = amg_plan(s, L);
        bool self_peer = false;                        // (timing probes only: every received sum holds the own value twice)
        for (int k = 0; k < P.np; ++k) self_peer = self_peer || P.peers[k] == s->rank;
        hipLaunchKernelGGL(k_rbm_offsets_coupled, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, nn_own, L.bs, L.dim,
                           static_cast<const int32_t *>(L.node_agg.p), static_cast<const double *>(L.cen.p), na_loc, C.cen.p,
                           static_cast<const int32_t *>(rot_ok.p), static_cast<const double *>(cv.p), static_cast<const double *>(cw.p),
                           self_peer ? 0.5 : 1.0, L.roff.p);
        PFEM_TRY(check_kernel("k_rbm_offsets_coupled"));
    }
    phase(l, "rbm: members + centroids");
    // ---- coarse block pattern: (coarse row node, coarse col node, fine block) sorted; the maps of the numeric product
    {
        DevBuf<uint64_t> &keys = W.keys;
        DevBuf<uint64_t> ukeys;
        DevBuf<int32_t> &idx = W.slots;
        const int64_t nblk = L.nblk;
        int64_t nblk_c = 0;
        PFEM_TRY(L.src_slot.alloc(static_cast<size_t>(std::max<int64_t>(nblk, 1))));
        bool by_codes = false;
        if (nblk > 0 && brick_box && !coupled && na > 0 && !amg_brick_sort()) {
            // node bricks: the 27 bricks around a coarse node are its only possible columns -- counts and two scans, no sort
            DevBuf<uint16_t> code_cnt;
            DevBuf<int> d_fail;
            DevBuf<int32_t> &n_entries = W.head, &n_pairs = W.rank, &entry_off = W.cnt, &pair_off = W.idx;
            PFEM_TRY(code_cnt.alloc(static_cast<size_t>(kRbmCodes) * na));
            PFEM_TRY(d_fail.alloc(1));
            PFEM_HIP(hipMemsetAsync(d_fail.p, 0, sizeof(int), s->stream));
            int32_t tot[2] = {0, 0};
            int fail = 0;
            PFEM_TRY(amg_count_scans(s, W, na, [&] {
                hipLaunchKernelGGL(k_rbm_codes_count, dim3(grid_for(na + 1)), dim3(kBlock), 0, s->stream, na, static_cast<const int32_t *>(L.mem_ptr.p),
                                   static_cast<const int32_t *>(L.mem_idx.p), static_cast<const int64_t *>(L.gptr.p), static_cast<const int32_t *>(L.gcol.p),
                                   static_cast<const int32_t *>(L.node_agg.p), brick_box[0], brick_box[1], code_cnt.p, n_entries.p, n_pairs.p, d_fail.p);
            }, "k_rbm_codes_count", d_fail.p, &tot[0], &tot[1], &fail));
            if (!fail && tot[1] == nblk) {
                nblk_c = tot[0];
                PFEM_TRY(ukeys.alloc(static_cast<size_t>(std::max<int64_t>(nblk_c, 1))));
                PFEM_TRY(L.src_ptr.alloc(static_cast<size_t>(nblk_c) + 1));
                hipLaunchKernelGGL(k_rbm_codes_fill, dim3(grid_for(na)), dim3(kBlock), 0, s->stream, na, static_cast<const int32_t *>(L.mem_ptr.p),
                                   static_cast<const int32_t *>(L.mem_idx.p), static_cast<const int64_t *>(L.gptr.p), static_cast<const int32_t *>(L.gcol.p),
                                   static_cast<const int32_t *>(L.node_agg.p), brick_box[0], brick_box[1], static_cast<const uint16_t *>(code_cnt.p),
                                   static_cast<const int32_t *>(entry_off.p), static_cast<const int32_t *>(pair_off.p), ukeys.p, L.src_ptr.p, L.src_slot.p);
                PFEM_TRY(check_kernel("k_rbm_codes_fill"));
                by_codes = true;
            }
            PFEM_HIP(hipStreamSynchronize(s->stream));       // (code_cnt, d_fail go out of scope)
        }
        if (by_codes) {
        } else if (nblk > 0) {
            PFEM_TRY(keys.reserve(static_cast<size_t>(nblk)));
            PFEM_TRY(idx.reserve(static_cast<size_t>(nblk)));
            hipLaunchKernelGGL(k_rbm_emit_block_keys, dim3(grid_for(nblk)), dim3(kBlock), 0, s->stream, nblk, static_cast<const int32_t *>(L.brow.p),
                               static_cast<const int32_t *>(L.gcol.p), static_cast<const int32_t *>(L.node_agg.p), keys.p, idx.p);
            PFEM_TRY(check_kernel("k_rbm_emit_block_keys"));
            PFEM_TRY(amg_pattern_from_keys(s, W, nblk, L.src_slot.p, L.src_ptr, ukeys, &nblk_c));
        } else {
            PFEM_TRY(L.src_ptr.alloc(1));
            PFEM_HIP(hipMemsetAsync(L.src_ptr.p, 0, sizeof(int64_t), s->stream));
            PFEM_TRY(ukeys.alloc(1));
        }
        if (nblk_c * cb * cb > INT_MAX) return PFEM_ERR_ARG;
        L.nnz_c = nblk_c;
        C.nblk = nblk_c;
        PFEM_TRY(C.gptr.alloc(static_cast<size_t>(na_loc) + 1));
        PFEM_TRY(C.gcol.alloc(static_cast<size_t>(std::max<int64_t>(nblk_c, 1))));
        PFEM_TRY(C.brow.alloc(static_cast<size_t>(std::max<int64_t>(nblk_c, 1))));
        hipLaunchKernelGGL(k_row_bounds, dim3(grid_for(std::max<int64_t>(nblk_c, na_loc + 1))), dim3(kBlock), 0, s->stream,
                           static_cast<const uint64_t *>(ukeys.p), nblk_c, na_loc, C.gptr.p);
        if (nblk_c > 0)
            hipLaunchKernelGGL(k_rbm_split_keys, dim3(grid_for(nblk_c)), dim3(kBlock), 0, s->stream, nblk_c, static_cast<const uint64_t *>(ukeys.p), C.brow.p, C.gcol.p);
        PFEM_TRY(check_kernel("k_rbm_split_keys"));
        PFEM_HIP(hipStreamSynchronize(s->stream));       // (ukeys goes out of scope)
    }
    // ---- the coarse matrix: wave-sliced storage straight from the node graph
    {
        C.nnz = C.nblk * cb * cb;
        C.n_slices = (nc_loc + 63) / 64;
        PFEM_TRY(C.rowptr.alloc(static_cast<size_t>(nc_loc) + 1));
        PFEM_TRY(C.rowlen.alloc(static_cast<size_t>(std::max<int64_t>(nc_loc, 1))));
        PFEM_TRY(C.slice_off.alloc(static_cast<size_t>(C.n_slices) + 1));
        DevBuf<int64_t> &slice_entries = W.slice_entries;
        PFEM_TRY(slice_entries.reserve(static_cast<size_t>(C.n_slices) + 1));
        hipLaunchKernelGGL(k_rbm_rowptr, dim3(grid_for(nc_loc + 1)), dim3(kBlock), 0, s->stream, na_loc, cb, static_cast<const int64_t *>(C.gptr.p), C.rowptr.p);
        hipLaunchKernelGGL(k_slice_sizes, dim3(grid_for(C.n_slices * 64)), dim3(kBlock), 0, s->stream, static_cast<const int64_t *>(C.rowptr.p), nc_loc,
                           C.n_slices, C.rowlen.p, slice_entries.p);
        PFEM_TRY(check_kernel("k_slice_sizes (rbm)"));
        PFEM_TRY(amg_exclusive_sum(s, temp, slice_entries.p, C.slice_off.p, C.n_slices + 1));
        int64_t stored = 0;
        PFEM_HIP(hipMemcpyAsync(&stored, C.slice_off.p + C.n_slices, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        if (stored > INT_MAX) return PFEM_ERR_ARG;
        C.stored = stored;
        PFEM_TRY(C.cols.alloc(static_cast<size_t>(std::max<int64_t>(stored, 1))));
        PFEM_TRY(C.vals.alloc(static_cast<size_t>(std::max<int64_t>(stored, 1))));
        hipLaunchKernelGGL(k_rbm_fill_cols, dim3(grid_for(C.n_slices * 64)), dim3(kBlock), 0, s->stream, nc_loc, C.n_slices, cb,
                           static_cast<const int64_t *>(C.slice_off.p), static_cast<const int64_t *>(C.gptr.p), static_cast<const int32_t *>(C.gcol.p), C.cols.p);
        PFEM_TRY(check_kernel("k_rbm_fill_cols"));
        PFEM_HIP(hipMemsetAsync(C.vals.p, 0, sizeof(double) * std::max<int64_t>(stored, 1), s->stream));
    }
    phase(l, "rbm: coarse pattern + maps");
    M.lev.push_back(std::move(Cp));
    amg_rbm_galerkin(s, L, *M.lev.back(), amg_sell(s, L, R));          // the next level's strength graph needs this level's values
    PFEM_TRY(check_kernel("k_rbm_galerkin (symbolic)"));
    return PFEM_OK;
    };
    PFEM_TRY(agreed(stretch_c()));
    *n_global = nc_global;
    return PFEM_OK;
}

// ---- bricks in one step (k_lat_*): a scalar level on a lattice whose sibling couplings are all strong --------------------
// WHY.  PCSetUp is inside the reference's solve timer (tetrapoissonparallelimpl1.F:898-902 -> solverpetsc.F:476), so the
// first step after a pattern build counts: at config 3 it took 91 ms, 72 of them this phase -- three passes of pairing with
// a sorted aggregate graph each (24 ms on level 0) and the 64-bit sort of (coarse row, coarse col, fine slot) (10 ms).  When
// every pair would be accepted the passes end in the bricks position >> shift anyway.  *done = false: the level is left to
// the passes (weak couplings along an axis, couplings beyond the neighbouring bricks).
int amg_bricks_level(pfem_solver *s, Amg &M, AmgWork &W, AmgLevel &L, const SellDev &A, AmgPhaseClock &phase, int l, bool *done, bool coupled, bool overlap,
                     double *n_global)
{
    *done = false;
    DevBuf<char> &temp = W.temp;
    // Several ranks (coupled; L.lat_global): the positions are global and cover this rank's ghosts too, the planes between the
    // ranks' nodes are aligned with the bricks, so a brick's nodes have one owner: the owner numbers its bricks (among its
    // owned dofs, z, y, x order), the ghosts' bricks get their numbers from the owners (amg_couple_level, which also forms the
    // coarse level's neighbour plan), and from there the maps below run over ALL local rows exactly as on one rank.
    const int64_t n = L.n, R = coupled ? L.n_loc : L.n;
    const SellDev Ar = amg_sell(s, L, R);
    LatBricks B{};
    int hi[3], axis = 0;
    const int halved = lat_sim_passes(L.lat_hi, L.lat_axis, B.shift, hi, &axis);
    if (!halved) return PFEM_OK;                        // (the lattice's extents are the same on every rank)
    int64_t nbricks = 1;
    for (int d = 0; d < 3; ++d) {
        B.lo[d] = coupled ? (L.lat_box[d] >> B.shift[d]) : 0;
        B.nb[d] = ((coupled ? L.lat_box[3 + d] : L.lat_hi[d]) >> B.shift[d]) - B.lo[d] + 1;
        nbricks *= std::max(B.nb[d], 1);
    }
    bool not_here = nbricks > INT_MAX - 8 || nbricks > 4 * R + 4096;
    if (coupled)                                        // (a level that was padded for other bricks than it now takes)
        for (int d = 0; d < 3; ++d) not_here = not_here || B.shift[d] != L.lat_shift[d];
    if (not_here && !coupled) return PFEM_OK;
    DevBuf<double> &diag = W.sums;
    DevBuf<int32_t> &flag = W.flag, &rank = W.crank;
    DevBuf<int> d_fail;
    int fail = 0;
    int32_t na32 = 0;
    auto check = [&]() -> int {
        if (not_here) return PFEM_OK;
        PFEM_TRY(diag.reserve(static_cast<size_t>(std::max<int64_t>(R, 1))));
        PFEM_TRY(flag.reserve(static_cast<size_t>(nbricks) + 1));
        PFEM_TRY(rank.reserve(static_cast<size_t>(nbricks) + 1));
        PFEM_TRY(d_fail.alloc(4));
        PFEM_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t) * (nbricks + 1), s->stream));
        PFEM_HIP(hipMemsetAsync(d_fail.p, 0, 4 * sizeof(int), s->stream));
        if (coupled && !L.fine) hipLaunchKernelGGL(k_extract_diag_scan, dim3(grid_for(R)), dim3(kBlock), 0, s->stream, Ar, diag.p);
        else hipLaunchKernelGGL(k_extract_diag, dim3(grid_for(R)), dim3(kBlock), 0, s->stream, Ar, diag.p);
        hipLaunchKernelGGL(k_lat_check, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, A, static_cast<const int32_t *>(L.hint.p), static_cast<const double *>(diag.p),
                           B, flag.p, d_fail.p);
        PFEM_TRY(check_kernel("k_lat_check"));
        PFEM_TRY(amg_exclusive_sum(s, temp, flag.p, rank.p, nbricks + 1));
        int why[4] = {0, 0, 0, 0};
        PFEM_HIP(hipMemcpyAsync(why, d_fail.p, sizeof why, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipMemcpyAsync(&na32, rank.p + nbricks, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        // (weak couplings inside the bricks: a verdict about the level -- refused from kAmgBrickWeakPercent of the rows on,
        // amg_node_bricks; a coupling beyond the neighbouring bricks: one is enough, the 27 offset codes cannot hold it)
        fail = why[2] > 0 || amg_too_many_weak(why[1], n);
        if (why[0] && amg_verbose())
            std::fprintf(stderr, "  gamg symbolic level %d bricks%s: %d of %lld rows with a weak sibling coupling, %d with a coupling beyond the neighbouring bricks (shifts %d %d %d, positions up to %d %d %d)\n",
                         l, fail ? " refused" : " kept", why[1], static_cast<long long>(n), why[2], B.shift[0], B.shift[1], B.shift[2], L.lat_hi[0], L.lat_hi[1], L.lat_hi[2]);
        return PFEM_OK;
    };
    const int rc_check = check();
    std::vector<double> nc_of;
    double nc_global = 0.0;
    if (coupled) {                                      // one all-reduce: anybody's refusal, and every rank's number of bricks
        std::vector<double> v(static_cast<size_t>(s->nranks) + 2, 0.0);
        v[0] = (fail || not_here) ? 1.0 : 0.0;
        v[1] = rc_check != PFEM_OK ? 1.0 : 0.0;
        v[2 + static_cast<size_t>(s->rank)] = static_cast<double>(na32);
        PFEM_TRY(amg_allreduce_host(s, v.data(), static_cast<int>(v.size())));
        if (rc_check != PFEM_OK) return rc_check;
        if (v[1] > 0.0) { set_last_error("gamg symbolic phase: another rank failed (allocation or size limit); all ranks stop together"); return PFEM_ERR_COMM; }
        if (v[0] > 0.0) return PFEM_OK;
        nc_of.assign(v.begin() + 2, v.end());
        for (double x : nc_of) nc_global += x;
    } else {
        PFEM_TRY(rc_check);
        if (fail) return PFEM_OK;
        nc_global = static_cast<double>(na32);
    }
    const int64_t na = na32;
    *done = true;
    if (coupled ? (nc_global < 1.0 || nc_global * 10.0 > *n_global * 8.0) : (na < 1 || na * 10 > n * 8 || 27 * na + 1 > 0xfffffff0LL)) return kAmgLastLevel;
    phase(l, "bricks: check + ranks");
    L.nc = na;
    L.agg_kind = kAggBricks;
    std::unique_ptr<AmgLevel> Cp(new (std::nothrow) AmgLevel());
    if (!Cp) return PFEM_ERR_NOMEM;
    AmgLevel &C = *Cp;
    C.n = C.n_loc = na;
    C.bs = 1;
    C.lattice = true;
    // brick coordinates of every coarse dof: on one rank they ARE its position on the next level; across ranks the next
    // level's positions are padded once more (below) and the coordinates live in a buffer of their own
    DevBuf<int32_t> bc_buf;
    int32_t *bc = nullptr;
    {
        int rc = L.agg.alloc(static_cast<size_t>(std::max<int64_t>(R, 1)));
        if (rc == PFEM_OK) {
            if (coupled) { rc = bc_buf.alloc(static_cast<size_t>(std::max<int64_t>(na + (R - n), 1))); bc = bc_buf.p; }
            else { rc = C.hint.alloc(static_cast<size_t>(na)); bc = C.hint.p; }
        }
        if (coupled) PFEM_TRY(amg_agree(s, rc));
        else PFEM_TRY(rc);
    }
    if (n > 0)
        hipLaunchKernelGGL(k_lat_assign, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, static_cast<const int32_t *>(L.hint.p), B,
                           static_cast<const int32_t *>(rank.p), L.agg.p, bc);
    PFEM_TRY(check_kernel("k_lat_assign"));
    if (coupled) {
        for (int q = 0; q < s->rank; ++q) C.gid_off += static_cast<int64_t>(nc_of[static_cast<size_t>(q)]);
        const int rc = amg_couple_level(s, W, L, C, overlap, 0, nullptr);
        if (rc != PFEM_OK) return rc;
        if (R > n)
            hipLaunchKernelGGL(k_lat_ghost_bricks, dim3(grid_for(R - n)), dim3(kBlock), 0, s->stream, n, R, static_cast<const int32_t *>(L.hint.p), B,
                               static_cast<const int32_t *>(L.agg.p), rank.p, bc);
        PFEM_TRY(check_kernel("k_lat_ghost_bricks"));
        phase(l, "bricks: ghosts + coarse plan");
    }
    const int64_t nal = C.n_loc;                        // coarse rows held here: owned, then the neighbours' that local dofs belong to
    C.n_nodes = na;
    for (int d = 0; d < 3; ++d) C.lat_hi[d] = hi[d];
    C.lat_axis = axis;
    // ---- members of every coarse dof (restriction as a gather)
    {
        int bits = 1;
        while ((1LL << bits) < nal) ++bits;
        PFEM_TRY(amg_member_lists(s, W, L, L.agg.p, R, nal, bits));
    }
    phase(l, "bricks: aggregates + member lists");
    // ---- Galerkin maps.  From the member lists, no sort (k_lat_codes_*): two walks of every coarse row's member rows and two
    // scans over the coarse rows instead of a 32-bit sort of every stored entry (config 3, level 0: 6.4 -> see LAB_NOTES).
    bool maps_done = false;
    if (!amg_brick_sort() && L.stored <= INT_MAX) {
        DevBuf<uint16_t> code_cnt;
        DevBuf<int32_t> &n_entries = W.head, &n_pairs = W.rank, &entry_off = W.cnt, &pair_off = W.idx;
        DevBuf<uint64_t> ukeys;
        PFEM_TRY(code_cnt.alloc(static_cast<size_t>(kLatCodes) * nal));
        int32_t tot[2] = {0, 0};
        int too_long = 0;
        PFEM_TRY(amg_count_scans(s, W, nal, [&] {
            hipLaunchKernelGGL(k_lat_codes_count, dim3(grid_for(nal + 1)), dim3(kBlock), 0, s->stream, Ar, static_cast<const int32_t *>(L.hint.p), B, nal,
                               static_cast<const int32_t *>(L.mem_ptr.p), static_cast<const int32_t *>(L.mem_idx.p), static_cast<const int32_t *>(bc),
                               code_cnt.p, n_entries.p, n_pairs.p, d_fail.p);
        }, "k_lat_codes_count", d_fail.p, &tot[0], &tot[1], &too_long));
        maps_done = !too_long;
        const int64_t nnz_c = tot[0];
        if (maps_done) {
        const bool maps = amg_galerkin_by_entry();
        PFEM_TRY(ukeys.alloc(static_cast<size_t>(std::max<int64_t>(nnz_c, 1))));
        if (maps) {
            PFEM_TRY(L.src_ptr.alloc(static_cast<size_t>(nnz_c) + 1));
            PFEM_TRY(L.src_slot.alloc(static_cast<size_t>(std::max<int64_t>(tot[1], 1))));
        }
        PFEM_TRY(L.code_of.alloc(static_cast<size_t>(std::max<int64_t>(L.stored, 1))));
        PFEM_TRY(L.code_mask.alloc(static_cast<size_t>(std::max<int64_t>(nal, 1))));
#define PFEM_LAT_FILL(MAPS)                                                                                                                                   \
        hipLaunchKernelGGL(k_lat_codes_fill<MAPS>, dim3(grid_for(nal)), dim3(kBlock), 0, s->stream, Ar, static_cast<const int32_t *>(L.hint.p), B, nal,     \
                           static_cast<const int32_t *>(L.mem_ptr.p), static_cast<const int32_t *>(L.mem_idx.p), static_cast<const int32_t *>(bc),    \
                           static_cast<const int32_t *>(rank.p), static_cast<const uint16_t *>(code_cnt.p), static_cast<const int32_t *>(entry_off.p),       \
                           static_cast<const int32_t *>(pair_off.p), ukeys.p, L.src_ptr.p, L.src_slot.p, L.code_of.p, L.code_mask.p)
        if (maps) PFEM_LAT_FILL(true);
        else PFEM_LAT_FILL(false);
#undef PFEM_LAT_FILL
        PFEM_TRY(check_kernel("k_lat_codes_fill"));
        L.nnz_c = nnz_c;
        if (maps) PFEM_TRY(amg_store_pattern(s, W, ukeys.p, nnz_c, C, L.dst_slot));
        else PFEM_TRY(amg_sell_from_keys(s, W, ukeys.p, nnz_c, C));
        }
        PFEM_HIP(hipStreamSynchronize(s->stream));       // (ukeys, code_cnt go out of scope)
    }
    if (!maps_done) {
        // (27 * coarse row + offset code, fine slot) sorted on 32-bit keys, runs = coarse entries.  The one sorted route that does not
        // go through amg_pattern_from_keys: its run kernels (k_lat_run_*) read 32-bit keys and decode them into the 64-bit ones.
        DevBuf<uint32_t> &keys = W.keys32, &skeys = W.skeys32;
        DevBuf<int32_t> &slots = W.slots, &head = W.head, &hrank = W.rank;
        DevBuf<uint64_t> ukeys;
        const int64_t cnt = L.stored;
        const uint32_t sentinel = static_cast<uint32_t>(27 * nal);
        PFEM_TRY(keys.reserve(static_cast<size_t>(cnt)));
        PFEM_TRY(skeys.reserve(static_cast<size_t>(cnt)));
        PFEM_TRY(slots.reserve(static_cast<size_t>(cnt)));
        PFEM_TRY(L.src_slot.alloc(static_cast<size_t>(cnt)));
        PFEM_TRY(head.reserve(static_cast<size_t>(cnt) + 1));
        PFEM_TRY(hrank.reserve(static_cast<size_t>(cnt) + 1));
        PFEM_HIP(hipMemsetAsync(keys.p, 0xff, sizeof(uint32_t) * static_cast<size_t>(cnt), s->stream));
        PFEM_HIP(hipMemsetAsync(slots.p, 0, sizeof(int32_t) * static_cast<size_t>(cnt), s->stream));
        hipLaunchKernelGGL(k_lat_emit_keys, dim3(grid_for(Ar.n_slices * 64)), dim3(kBlock), 0, s->stream, Ar, static_cast<const int32_t *>(L.hint.p),
                           static_cast<const int32_t *>(L.agg.p), B, sentinel, keys.p, slots.p);
        PFEM_TRY(check_kernel("k_lat_emit_keys"));
        int bits = 1;
        while ((1ULL << bits) <= sentinel) ++bits;
        // (slots of slices beyond this level's rows keep the 0xffffffff fill: above the sentinel, they sort behind it with all 32 bits;
        // the level's own storage has none, so the sentinel's bits suffice)
        PFEM_TRY(amg_sort_pairs(s, temp, keys.p, skeys.p, slots.p, L.src_slot.p, cnt, bits));
        hipLaunchKernelGGL(k_lat_run_heads, dim3(grid_for(cnt + 1)), dim3(kBlock), 0, s->stream, cnt, static_cast<const uint32_t *>(skeys.p), head.p);
        PFEM_TRY(amg_exclusive_sum(s, temp, head.p, hrank.p, cnt + 1));
        int32_t m32 = 0;
        PFEM_HIP(hipMemcpyAsync(&m32, hrank.p + cnt, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        int64_t nnz_c = m32;
        PFEM_TRY(ukeys.alloc(static_cast<size_t>(std::max<int64_t>(nnz_c, 1))));
        PFEM_TRY(L.src_ptr.alloc(static_cast<size_t>(nnz_c) + 1));
        hipLaunchKernelGGL(k_lat_run_scatter, dim3(grid_for(cnt + 1)), dim3(kBlock), 0, s->stream, cnt, static_cast<const uint32_t *>(skeys.p),
                           static_cast<const int32_t *>(head.p), static_cast<const int32_t *>(hrank.p), sentinel, static_cast<const int32_t *>(bc), B,
                           static_cast<const int32_t *>(rank.p), ukeys.p, L.src_ptr.p);
        PFEM_TRY(check_kernel("k_lat_run_scatter"));
        PFEM_TRY(amg_drop_sentinel_run(s, ukeys.p, &nnz_c));
        L.nnz_c = nnz_c;
        PFEM_TRY(amg_store_pattern(s, W, ukeys.p, nnz_c, C, L.dst_slot));
        PFEM_HIP(hipStreamSynchronize(s->stream));       // (ukeys goes out of scope)
    }
    phase(l, "bricks: Galerkin maps + coarse pattern");
    if (coupled) {
        // the next level's positions: brick coordinates, padded again where the owner changes (same table on every rank)
        std::vector<int> cb[3];
        for (int d = 0; d < 3; ++d)
            for (int c : L.lat_cuts[d]) cb[d].push_back(c >> B.shift[d]);
        LatPad P;
        int occ_c[6];
        for (int d = 0; d < 3; ++d) { occ_c[d] = L.lat_occ[d] >> B.shift[d]; occ_c[3 + d] = L.lat_occ[3 + d] >> B.shift[d]; }
        const bool pad_ok = lat_pad(cb, L.lat_single, hi, occ_c, axis, P);           // (same verdict on every rank)
        DevBuf<int32_t> table;
        auto place = [&]() -> int {
            if (C.stored > INT_MAX || 27 * nal + 1 > 0xfffffff0LL) return PFEM_ERR_ARG;
            PFEM_TRY(C.hint.alloc(static_cast<size_t>(std::max<int64_t>(nal, 1))));
            if (pad_ok) {
                PFEM_TRY(table.alloc(P.table.size()));
                PFEM_HIP(hipMemcpyAsync(table.p, P.table.data(), sizeof(int32_t) * P.table.size(), hipMemcpyHostToDevice, s->stream));
                hipLaunchKernelGGL(k_lat_remap, dim3(grid_for(nal)), dim3(kBlock), 0, s->stream, nal, static_cast<const int32_t *>(bc),
                                   static_cast<const int32_t *>(table.p), C.hint.p);
            } else {
                PFEM_HIP(hipMemcpyAsync(C.hint.p, bc, sizeof(int32_t) * static_cast<size_t>(nal), hipMemcpyDeviceToDevice, s->stream));
            }
            PFEM_TRY(check_kernel("k_lat_remap (coarse positions)"));
            PFEM_HIP(hipStreamSynchronize(s->stream));          // (table goes out of scope)
            return PFEM_OK;
        };
        PFEM_TRY(amg_agree(s, place()));
        if (pad_ok) {
            C.lat_global = true;
            for (int d = 0; d < 3; ++d) {
                C.lat_hi[d] = P.hi[d];
                C.lat_cuts[d] = P.cuts[d];
                C.lat_single[d] = P.single[d];
                C.lat_shift[d] = P.shift[d];
                C.lat_occ[d] = P.table[static_cast<size_t>(1024 * d + occ_c[d])];
                C.lat_occ[3 + d] = P.table[static_cast<size_t>(1024 * d + occ_c[3 + d])];
                C.lat_box[d] = P.table[static_cast<size_t>(1024 * d + (L.lat_box[d] >> B.shift[d]))];
                C.lat_box[3 + d] = P.table[static_cast<size_t>(1024 * d + (L.lat_box[3 + d] >> B.shift[d]))];
            }
            C.lat_coord.assign(3 * 1024, 0.0);
            if (L.lat_coord.size() == 3 * 1024)
                for (int d = 0; d < 3; ++d)
                    for (int pc = 0; pc <= hi[d]; ++pc)
                        C.lat_coord[static_cast<size_t>(1024 * d + P.table[static_cast<size_t>(1024 * d + pc)])] = L.lat_coord[static_cast<size_t>(1024 * d + std::min(pc << B.shift[d], 1023))];
        } else {
            C.lattice = false;                                  // (positions beyond 10 bits after padding: the passes take the rest)
        }
    } else if (C.stored > INT_MAX) {
        return PFEM_ERR_ARG;
    }
    M.lev.push_back(std::move(Cp));
    amg_galerkin(s, L, *M.lev.back(), Ar);           // the next level's check needs this level's values
    PFEM_TRY(check_kernel("k_amg_galerkin (bricks)"));
    *n_global = nc_global;
    return PFEM_OK;
}

// ---- node bricks in one step (levels that take the rigid-body transfer; one rank) --------------------------------------------
// WHY.  Config 4's first step cost 46-56 ms against 28.7 for the steps after it; 6 of the difference were the three pairing
// passes of every level with their sorted aggregate graphs (profiles/r05/beam_symbolic_phases.txt).  On a lattice whose lines are
// full the passes end in bricks known beforehand: pairs 2k | 2k + 1 along every halved axis, the node an odd line leaves over
// joined to the pair next to it (3-dof problems: k_amg_lat_absorb).  Per axis a table position -> brick coordinate, composed
// halving by halving on the host; one check of the level's node graph (k_rbm_lat_check); the aggregates numbered in z, y, x
// order of the bricks.  *done = false: the level is left to the passes.
struct NodeBricks {
    DevBuf<int32_t> node_agg, hint;
    int64_t na = 0;
    int hi[3] = {0, 0, 0}, axis = 0, tlo[3] = {0, 0, 0}, thi[3] = {0, 0, 0};
    int nbk[3] = {1, 1, 1};            // bricks along every axis: aggregate = bx + nbk[0] (by + nbk[1] bz), coordinates relative to the box
    std::vector<std::pair<int, int>> str[3];       // across ranks: the stretches of one owner in BRICK coordinates (the next level's lat_str)
};
// One axis of a node-brick level.  The occupied positions come in stretches of one owner (`str`, inclusive ends, ascending; one
// rank: ONE stretch, the box the nodes fill); inside a stretch the bricks are what the pairing passes end in -- f positions to
// the brick, aligned on multiples of f, a brick at either end of the stretch that would hold at most f / 2 positions joined to
// its neighbour --, `halvings` times over when f = 2.  table[p] = brick coordinate of position p: the first stretch keeps the
// numbers the one-rank form has always had (brick = position / f), every further stretch goes on where the one before it ended,
// so no brick holds positions of two stretches (= of two owners) and the coordinates are the same on every rank.  out[k] = the
// bricks of stretch k.  Level 0 of a displacement problem takes f = 3 from an extent of 6 on, 4 from 24 on (per stretch).
inline void node_brick_axis(const std::vector<std::pair<int, int>> &str, bool fine, int halvings, int first_max, int32_t *table /* [1024] */,
                            std::vector<std::pair<int, int>> &out)
{
    out.clear();
    int base = 0;
    for (size_t k = 0; k < str.size(); ++k) {
        const int s0 = str[k].first, s1 = str[k].second;
        int lo = s0, hi = s1;
        std::vector<int> map(static_cast<size_t>(s1 - s0 + 1));
        for (int p = s0; p <= s1; ++p) map[static_cast<size_t>(p - s0)] = p;
        const int extent = s1 - s0 + 1;
        const int want = extent >= 24 ? 4 : (extent >= 6 ? 3 : 2);
        const int f = (fine && halvings > 0) ? std::max(2, std::min(want, std::min(first_max, extent / 2))) : 2;
        for (int h = 0; h < (f > 2 ? 1 : halvings); ++h) {
            // a brick at either end that would hold at most f / 2 nodes joins its neighbour (f = 2: the single node of an odd line)
            const int bmin = lo / f + ((f - lo % f) <= f / 2 ? 1 : 0), bmax = hi / f - ((hi % f + 1) <= f / 2 ? 1 : 0);
            const bool pairs = bmin <= bmax;                       // (a line without a whole brick: its nodes stay single)
            for (int &m : map) {
                const int b = m / f;
                m = pairs ? std::min(std::max(b, bmin), bmax) : b;
            }
            lo = pairs ? bmin : lo / f;
            hi = pairs ? bmax : hi / f;
        }
        if (k == 0) base = lo;
        for (int p = s0; p <= s1; ++p) table[p] = map[static_cast<size_t>(p - s0)] - lo + base;
        out.push_back({base, base + (hi - lo)});
        base += hi - lo + 1;
    }
}
// `coupled`: one hierarchy across the ranks (L.lat_nodes_global: global positions, L.lat_str the owners' stretches): the same
// table on every rank, this rank's bricks = the bricks of its own box, numbered z, y, x inside it; the verdict is agreed.  Collective then.
int amg_node_bricks(pfem_solver *s, AmgLevel &L, const AmgGraph &G, NodeBricks &N, bool *done, bool coupled = false)
{
    *done = false;
    const int64_t nn = L.n_nodes;
    int shift[3];
    const int halved = lat_sim_passes(L.lat_hi, L.lat_axis, shift, N.hi, &N.axis);
    if (!halved) return PFEM_OK;                        // (the lattice's extents are the same on every rank)
    // Level 0 of a displacement problem: bricks of THREE nodes along every axis that has at least six, of FOUR along an axis of 24
    // and more, instead of two.  With rigid-body modes the coarse space follows a large aggregate nearly as well as a small one
    // (the oracle's restatement on a 16x96x16 beam: 22 iterations with 2x2x2, 23 with 3x3x3 first, 25 with 4x4x4; config 4 on the
    // device: 18 / 22 / 22, then 27 / 41 / 54 with 5 / 6 / 8), while level 1 -- whose 6x6 blocks of fp64 made it the dearest level
    // of the cycle once the matrix itself streamed dictionary codes (54 M entries against 103 M two-byte codes) -- shrinks 3.3 /
    // 7.7 times: config 4 24.8 -> 20.9 -> 19.2 ms per step.  Scalar problems keep 2x2x2 (piecewise-constant coarse space: 10 -> 12
    // iterations at 60^3, and level 1 is cheap there).  first_max = the largest brick edge allowed (2: round 4's bricks).
    constexpr int first_max = 4;
    std::vector<int32_t> table(3 * 1024, 0);
    const bool have = nn > 0;                           // (a rank that owns nothing of this level takes part in the verdict only)
    int64_t na = 1;
    int nbk[3] = {1, 1, 1};
    for (int d = 0; d < 3; ++d) {
        std::vector<std::pair<int, int>> one{{L.lat_tlo[d], L.lat_thi[d]}};
        const std::vector<std::pair<int, int>> &str = coupled ? L.lat_str[d] : one;
        if (str.empty()) { N.str[d].clear(); continue; }
        node_brick_axis(str, L.fine, shift[d], first_max, table.data() + 1024 * d, N.str[d]);
        if (coupled) {
            N.hi[d] = N.str[d].back().second;
        } else {
            const int extent = L.lat_thi[d] - L.lat_tlo[d] + 1;
            const int want = extent >= 24 ? 4 : (extent >= 6 ? 3 : 2);
            const int f = (L.fine && shift[d] > 0) ? std::max(2, std::min(want, std::min(first_max, extent / 2))) : 2;
            if (f > 2) N.hi[d] = L.lat_hi[d] / f;
        }
        if (have) {
            N.tlo[d] = table[static_cast<size_t>(1024 * d + L.lat_tlo[d])];
            N.thi[d] = table[static_cast<size_t>(1024 * d + L.lat_thi[d])];
        }
        nbk[d] = have ? N.thi[d] - N.tlo[d] + 1 : 0;
        N.nbk[d] = nbk[d];
        na *= nbk[d];
    }
    if (!have) na = 0;
    if (!coupled && (na < 1 || na > INT_MAX - 8 || na * 10 > nn * 8)) return PFEM_OK;       // (a level that hardly shrinks: the passes decide whether it is the last)
    DevBuf<int32_t> d_table;
    DevBuf<int> d_fail;
    int fail = 0;
    auto local = [&]() -> int {
        if (!have) return PFEM_OK;
        if (na < 1 || na > INT_MAX - 8) { fail = 1; return PFEM_OK; }
        PFEM_TRY(d_table.alloc(table.size()));
        PFEM_TRY(d_fail.alloc(1));
        PFEM_HIP(hipMemcpyAsync(d_table.p, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, s->stream));
        PFEM_HIP(hipMemsetAsync(d_fail.p, 0, sizeof(int), s->stream));
        hipLaunchKernelGGL(k_rbm_lat_check, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, static_cast<const int64_t *>(G.ptr.p),
                           static_cast<const int32_t *>(G.col.p), static_cast<const double *>(G.w.p), static_cast<const double *>(G.diag.p),
                           static_cast<const int32_t *>(L.hint.p), static_cast<const int32_t *>(d_table.p), d_fail.p);
        PFEM_TRY(check_kernel("k_rbm_lat_check"));
        PFEM_TRY(N.node_agg.alloc(static_cast<size_t>(std::max<int64_t>(nn, 1))));
        PFEM_TRY(N.hint.alloc(static_cast<size_t>(na)));
        hipLaunchKernelGGL(k_rbm_lat_assign, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, static_cast<const int32_t *>(L.hint.p),
                           static_cast<const int32_t *>(d_table.p), N.tlo[0], N.tlo[1], N.tlo[2], nbk[0], nbk[1], N.node_agg.p);
        hipLaunchKernelGGL(k_rbm_lat_coarse_pos, dim3(grid_for(na)), dim3(kBlock), 0, s->stream, na, N.tlo[0], N.tlo[1], N.tlo[2], nbk[0], nbk[1], N.hint.p);
        PFEM_TRY(check_kernel("k_rbm_lat_assign"));
        PFEM_HIP(hipMemcpyAsync(&fail, d_fail.p, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        return PFEM_OK;
    };
    const int rc = local();
    // (weak couplings inside the bricks: a verdict about the level, amg_too_many_weak)
    if (coupled) {               // one verdict for all: anybody's failure or refusal, and whether the level shrinks at all
        double v[4] = {rc != PFEM_OK ? 1.0 : 0.0, static_cast<double>(fail), static_cast<double>(na), static_cast<double>(nn)};
        PFEM_TRY(amg_allreduce_host(s, v, 4));
        if (rc != PFEM_OK) return rc;
        if (v[0] > 0.0) { set_last_error("gamg symbolic phase: another rank failed (allocation or size limit); all ranks stop together"); return PFEM_ERR_COMM; }
        if (amg_verbose() && v[1] > 0.0) std::fprintf(stderr, "  gamg symbolic: node bricks across ranks: %g of %g nodes with a weak coupling inside their brick\n", v[1], v[3]);
        if (amg_too_many_weak(v[1], v[3]) || v[2] < 1.0 || v[2] * 10.0 > v[3] * 8.0) {
            if (amg_verbose())
                std::fprintf(stderr, "  gamg symbolic: node bricks across ranks refused (%g nodes with a weak coupling inside a brick, %g bricks for %g nodes)\n", v[1], v[2], v[3]);
            return PFEM_OK;
        }
        if (!have) { PFEM_TRY(N.node_agg.alloc(1)); PFEM_TRY(N.hint.alloc(1)); }
    } else {
        PFEM_TRY(rc);
        if (amg_verbose() && fail) std::fprintf(stderr, "  gamg symbolic: node bricks: %d of %lld nodes with a weak coupling inside their brick\n", fail, static_cast<long long>(nn));
        if (amg_too_many_weak(fail, static_cast<double>(nn))) {
            if (amg_verbose()) std::fprintf(stderr, "  gamg symbolic: node bricks refused (weak couplings inside the bricks): the passes take the level\n");
            return PFEM_OK;
        }
    }
    N.na = na;
    *done = true;
    return PFEM_OK;
}

// ---- bricks across ranks whose dofs do not fill boxes (scalar problems; round 6) -------------------------------------------
// WHY.  north_star shards along "the existing METIS partition" (tetrapoissonparallelimpl1.F:464): its parts are not boxes of the
// lattice, so the bricks-in-one-step of amg_bricks_level (which pads the planes between the owners onto brick borders) gave up
// for everybody and the ranks paired in three passes with a sorted aggregate graph each (70-126 ms of symbolic phase per rank
// at 200^3).  Here a brick may hold dofs of several owners and every owner's part of it is an aggregate of its own: positions
// GLOBAL and unpadded, aggregate = rank of the dof's brick among the bricks THIS rank owns a dof of (z, y, x order), one check
// of the owned rows (k_lat_check_split).  The ghosts learn their aggregates from the owners and the Galerkin maps come from the
// sorted (coarse row, coarse column, slot) keys exactly as for matched aggregates (the caller goes on with node_agg).
// Collective; *done = false: the level is left to the passes.
int amg_split_bricks(pfem_solver *s, AmgWork &W, AmgLevel &L, const SellDev &A, bool *done, DevBuf<int32_t> &agg, DevBuf<int32_t> &pos_c, int64_t *na_out,
                     int hi_out[3], int *axis_out, int shift_out[3])
{
    *done = false;
    DevBuf<char> &temp = W.temp;
    const int64_t n = L.n;
    LatBricks B{};
    if (!lat_sim_passes(L.lat_hi, L.lat_axis, B.shift, hi_out, axis_out)) return PFEM_OK;          // (the same on every rank)
    for (int d = 0; d < 3; ++d) shift_out[d] = B.shift[d];
    const bool have = n > 0;
    int64_t nbricks = have ? 1 : 0;
    for (int d = 0; d < 3; ++d) {
        B.lo[d] = have ? (L.lat_tlo[d] >> B.shift[d]) : 0;
        B.nb[d] = have ? (L.lat_thi[d] >> B.shift[d]) - B.lo[d] + 1 : 0;
        nbricks *= std::max(B.nb[d], have ? 1 : 0);
    }
    DevBuf<double> &diag = W.sums;
    DevBuf<int32_t> &flag = W.flag, &rank = W.crank;
    DevBuf<int> d_fail;
    int fail = 0;
    int32_t na32 = 0;
    auto local = [&]() -> int {
        if (!have) return PFEM_OK;
        if (nbricks > INT_MAX - 8 || nbricks > 8 * n + 4096) { fail = 1; return PFEM_OK; }        // (owned dofs scattered over a huge box: not worth a table)
        PFEM_TRY(diag.reserve(static_cast<size_t>(std::max<int64_t>(L.n_loc, 1))));
        PFEM_TRY(flag.reserve(static_cast<size_t>(nbricks) + 1));
        PFEM_TRY(rank.reserve(static_cast<size_t>(nbricks) + 1));
        PFEM_TRY(d_fail.alloc(4));
        PFEM_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t) * (nbricks + 1), s->stream));
        PFEM_HIP(hipMemsetAsync(d_fail.p, 0, 4 * sizeof(int), s->stream));
        if (!L.fine) hipLaunchKernelGGL(k_extract_diag_scan, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, A, diag.p);
        else hipLaunchKernelGGL(k_extract_diag, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, A, diag.p);
        hipLaunchKernelGGL(k_lat_check_split, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, A, static_cast<const int32_t *>(L.hint.p),
                           static_cast<const double *>(diag.p), B, flag.p, d_fail.p);
        PFEM_TRY(check_kernel("k_lat_check_split"));
        PFEM_TRY(amg_exclusive_sum(s, temp, flag.p, rank.p, nbricks + 1));
        int why[4] = {0, 0, 0, 0};
        PFEM_HIP(hipMemcpyAsync(why, d_fail.p, sizeof why, hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipMemcpyAsync(&na32, rank.p + nbricks, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        fail = amg_too_many_weak(why[1], n);
        if (fail && amg_verbose())
            std::fprintf(stderr, "  gamg symbolic: split bricks refused on this rank: %d of %lld owned rows with a weak sibling coupling\n", why[1], static_cast<long long>(n));
        return PFEM_OK;
    };
    const int rc = local();
    double v[4] = {rc != PFEM_OK ? 1.0 : 0.0, fail ? 1.0 : 0.0, static_cast<double>(na32), static_cast<double>(n)};
    PFEM_TRY(amg_allreduce_host(s, v, 4));
    if (rc != PFEM_OK) return rc;
    if (v[0] > 0.0) { set_last_error("gamg symbolic phase: another rank failed (allocation or size limit); all ranks stop together"); return PFEM_ERR_COMM; }
    if (v[1] > 0.0 || v[2] < 1.0 || v[2] * 10.0 > v[3] * 8.0) return PFEM_OK;             // (hardly shrinks: the passes decide whether it is the last)
    auto assign = [&]() -> int {
        PFEM_TRY(agg.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
        PFEM_TRY(pos_c.alloc(static_cast<size_t>(std::max<int64_t>(na32, 1))));
        if (have) {
            hipLaunchKernelGGL(k_lat_assign, dim3(grid_for(n)), dim3(kBlock), 0, s->stream, n, static_cast<const int32_t *>(L.hint.p), B,
                               static_cast<const int32_t *>(rank.p), agg.p, pos_c.p);
            PFEM_TRY(check_kernel("k_lat_assign (split bricks)"));
        }
        PFEM_HIP(hipStreamSynchronize(s->stream));        // (d_fail goes out of scope)
        return PFEM_OK;
    };
    PFEM_TRY(amg_agree(s, assign()));
    *na_out = na32;
    *done = true;
    return PFEM_OK;
}

// ---- the levels below M.lev.back(): aggregates, transfer maps, coarse patterns (and one numeric product each) ----------
int amg_finish_levels(pfem_solver *s, Amg &M, bool coupled);
int amg_replicate(pfem_solver *s, Amg &M, AmgWork &W, AmgLevel &C, int64_t n_global, bool overlap);
// What the steps of one level hand each other (amg_build_levels): the aggregates of the level's nodes, and where they sit
struct AmgLevelBuild {
    DevBuf<int32_t> node_agg;                // node -> aggregate so far
    int64_t na = 0;                          // aggregates so far
    const int32_t *hint = nullptr;           // their places along the curve / positions on the lattice (null: indices), held by one of
    DevBuf<int32_t> hint_a, hint_b;          //   these (pass by pass), by NB or by sb_pos
    int lat_hi[3] = {0, 0, 0}, lat_axis = 0;
    bool on_lattice = false;
    bool rbm = false, have_graph = false;    // the level takes the rigid-body transfer / came with its node graph
    AmgGraph *G = nullptr;                   // the strength graph the next pass pairs on (two objects in the work set, used alternately)
    int gcur = 0;
    bool node_bricks = false;
    NodeBricks NB;
    bool split_bricks = false;
    DevBuf<int32_t> sb_agg, sb_pos;
    int64_t sb_na = 0;
    int sb_hi[3] = {0, 0, 0}, sb_axis = 0, sb_shift[3] = {0, 0, 0};
};

// small enough for every rank to hold it whole: the rest of the hierarchy is replicated (*done)
int amg_replicate_rest(pfem_solver *s, Amg &M, AmgWork &W, bool coupled, double n_global, bool overlap, AmgPhaseClock &phase, int l, bool *done)
{
    const char *e = std::getenv("PFEM_AMG_REPLICATE_ROWS");
    const int64_t replicate_rows = e ? std::atoll(e) : kAmgReplicateRows;
    *done = coupled && n_global > kAmgDense && n_global <= static_cast<double>(replicate_rows);
    if (!*done) return PFEM_OK;
    PFEM_TRY(amg_replicate(s, M, W, *M.lev.back(), static_cast<int64_t>(n_global), overlap));
    phase(l, "replicated levels");
    return PFEM_OK;
}

// several ranks whose dofs do not fill boxes: a rank's aggregate = its part of a brick (amg_split_bricks); collective
int amg_level_split_bricks(pfem_solver *s, AmgWork &W, AmgLevel &L, const SellDev &A, bool coupled, AmgLevelBuild &B, AmgPhaseClock &phase, int l)
{
    const int64_t nn = L.n_nodes;
    if (coupled && L.lat_split && L.lattice && L.bs == 1 && (L.hint.p || L.n == 0)) {
        PFEM_TRY(amg_split_bricks(s, W, L, A, &B.split_bricks, B.sb_agg, B.sb_pos, &B.sb_na, B.sb_hi, &B.sb_axis, B.sb_shift));
        if (B.split_bricks) phase(l, "split bricks: check + aggregates");
    }
    // (a level that leaves the brick path on several ranks: the corners the replicated level will want, from the positions)
    if (coupled && (L.lat_global || (L.lat_split && !B.split_bricks)) && L.bs == 1 && !L.xyz.p && nn > 0 && L.hint.p && L.lat_coord.size() == 3 * 1024) {
        DevBuf<double> coord;
        PFEM_TRY(coord.alloc(3 * 1024));
        PFEM_TRY(L.xyz.alloc(static_cast<size_t>(3 * nn)));
        PFEM_HIP(hipMemcpyAsync(coord.p, L.lat_coord.data(), sizeof(double) * 3 * 1024, hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_lat_xyz_from_pos, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, static_cast<const int32_t *>(L.hint.p),
                           static_cast<const double *>(coord.p), L.xyz.p);
        PFEM_TRY(check_kernel("k_lat_xyz_from_pos"));
        PFEM_HIP(hipStreamSynchronize(s->stream));
    }
    return PFEM_OK;
}

// the level's strength graph on its nodes, in B.G: the node graph of a rigid-body level (all local, or the owned nodes' rows of
// it), the matrix itself (scalar problem), or the dofs' entries summed node by node; none where split bricks gave the aggregates.
// Decides B.rbm on the way.
int amg_level_graph(pfem_solver *s, Amg &M, AmgWork &W, AmgLevel &L, const SellDev &A, bool coupled, AmgLevelBuild &B)
{
    const int64_t R = coupled ? L.n_loc : L.n, nn = L.n_nodes;
    B.gcur = 0;
    B.G = &W.graphs[0];
    const int32_t col_limit = static_cast<int32_t>(L.n);       // coarse levels: every column; level 0: the owned ones
    // rigid-body modes: the level qualifies when its dofs come bs to the node in a block-regular matrix (checked here for
    // the assembled matrix; a coarse level of this kind is block regular by construction)
    // (several ranks, one hierarchy across them: the node graph spans all local nodes -- owned first, ghosts after them --, the
    // pairing sees the owned nodes' rows without their ghost columns; one hierarchy per rank: not a candidate)
    const int64_t nn_loc = L.bs > 0 ? R / L.bs : 0;
    bool rbm_here = L.dim > 0 && L.cen.p && (coupled || L.n_loc == L.n) && L.n == nn * L.bs && R == nn_loc * L.bs;
    double rbm_bad = 0.0;
    // (a level that amg_rbm_level built comes with its node graph -- the coarse block pattern it was stored from: nothing to check)
    B.have_graph = rbm_here && !L.fine && L.gptr.p && L.gcol.p && L.brow.p && L.nblk > 0 && L.gptr.n == static_cast<size_t>(nn_loc) + 1;
    if (rbm_here && !B.have_graph) {
        const SellDev Ar = amg_sell(s, L, R);
        DevBuf<int64_t> deg;
        DevBuf<int> d_bad;
        PFEM_TRY(deg.alloc(static_cast<size_t>(nn_loc) + 1));
        PFEM_TRY(d_bad.alloc(1));
        PFEM_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), s->stream));
        hipLaunchKernelGGL(k_rbm_check_rows, dim3(grid_for(R + 1)), dim3(kBlock), 0, s->stream, Ar, L.bs, nn_loc, deg.p, d_bad.p);
        PFEM_TRY(check_kernel("k_rbm_check_rows"));
        PFEM_TRY(L.gptr.alloc(static_cast<size_t>(nn_loc) + 1));
        PFEM_TRY(amg_exclusive_sum(s, W.temp, deg.p, L.gptr.p, nn_loc + 1));
        int bad = 0;
        int64_t nblk = 0;
        PFEM_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipMemcpyAsync(&nblk, L.gptr.p + nn_loc, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        if (bad || nblk > INT_MAX || (nblk < 1 && nn_loc > 0)) rbm_bad = 1.0;
        L.nblk = nblk;
    }
    if (coupled && L.dim > 0) {              // all ranks take the same transfer
        double v[2] = {rbm_here ? 0.0 : 1.0, rbm_bad};
        PFEM_TRY(amg_allreduce_host(s, v, 2));
        rbm_here = v[0] == 0.0 && v[1] == 0.0;
    } else if (rbm_bad > 0.0) {
        rbm_here = false;
    }
    if (!rbm_here) L.gptr.release();
    L.rbm = B.rbm = rbm_here;
    if (B.split_bricks) {
        // (no strength graph: the aggregates are there)
    } else if (B.rbm) {
        const SellDev Ar = amg_sell(s, L, R);
        M.rbm = true;
        if (!B.have_graph) {
            PFEM_TRY(L.gcol.alloc(static_cast<size_t>(std::max<int64_t>(L.nblk, 1))));
            PFEM_TRY(L.brow.alloc(static_cast<size_t>(std::max<int64_t>(L.nblk, 1))));
        }
        // (DIM lanes per node, 64 / DIM nodes per wave)
        auto graph_fill = [&](int64_t nodes, double *gw, double *gd) {
            const int npw = 64 / L.dim;
            const unsigned blocks = static_cast<unsigned>(((nodes + npw - 1) / npw * 64 + kBlock - 1) / kBlock);
            if (L.dim == 3) hipLaunchKernelGGL(k_rbm_graph_fill_rows<3>, dim3(std::max(blocks, 1u)), dim3(kBlock), 0, s->stream, Ar, L.bs, nodes,
                                               static_cast<const int64_t *>(L.gptr.p), L.gcol.p, L.brow.p, gw, gd);
            else hipLaunchKernelGGL(k_rbm_graph_fill_rows<2>, dim3(std::max(blocks, 1u)), dim3(kBlock), 0, s->stream, Ar, L.bs, nodes,
                                    static_cast<const int64_t *>(L.gptr.p), L.gcol.p, L.brow.p, gw, gd);
        };
        if (nn_loc == nn) {
            PFEM_TRY(B.G->reserve(nn, L.nblk));
            graph_fill(nn, B.G->w.p, B.G->diag.p);
            PFEM_TRY(check_kernel("k_rbm_graph_fill"));
            PFEM_HIP(hipMemcpyAsync(B.G->ptr.p, L.gptr.p, sizeof(int64_t) * (nn + 1), hipMemcpyDeviceToDevice, s->stream));
            if (L.nblk > 0) PFEM_HIP(hipMemcpyAsync(B.G->col.p, L.gcol.p, sizeof(int32_t) * L.nblk, hipMemcpyDeviceToDevice, s->stream));
        } else {
            // all local nodes' graph first (weights in the work set), then the owned nodes' rows without ghost columns
            DevBuf<double> &w_all = W.svals, &d_all = W.sums;
            DevBuf<int64_t> odeg;
            PFEM_TRY(w_all.reserve(static_cast<size_t>(std::max<int64_t>(L.nblk, 1))));
            PFEM_TRY(d_all.reserve(static_cast<size_t>(std::max<int64_t>(nn_loc, 1))));
            PFEM_TRY(odeg.alloc(static_cast<size_t>(nn) + 1));
            graph_fill(nn_loc, w_all.p, d_all.p);
            hipLaunchKernelGGL(k_rbm_owned_degree, dim3(grid_for(nn + 1)), dim3(kBlock), 0, s->stream, nn, static_cast<const int64_t *>(L.gptr.p),
                               static_cast<const int32_t *>(L.gcol.p), odeg.p);
            PFEM_TRY(check_kernel("k_rbm_owned_degree"));
            B.G->n = nn;
            PFEM_TRY(B.G->ptr.reserve(static_cast<size_t>(nn) + 1));
            PFEM_TRY(amg_exclusive_sum(s, W.temp, odeg.p, B.G->ptr.p, nn + 1));
            int64_t onnz = 0;
            PFEM_HIP(hipMemcpyAsync(&onnz, B.G->ptr.p + nn, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
            PFEM_HIP(hipStreamSynchronize(s->stream));
            B.G->nnz = onnz;
            PFEM_TRY(B.G->col.reserve(static_cast<size_t>(std::max<int64_t>(onnz, 1))));
            PFEM_TRY(B.G->w.reserve(static_cast<size_t>(std::max<int64_t>(onnz, 1))));
            PFEM_TRY(B.G->diag.reserve(static_cast<size_t>(std::max<int64_t>(nn, 1))));
            hipLaunchKernelGGL(k_rbm_owned_graph, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, static_cast<const int64_t *>(L.gptr.p),
                               static_cast<const int32_t *>(L.gcol.p), static_cast<const double *>(w_all.p), static_cast<const int64_t *>(B.G->ptr.p),
                               B.G->col.p, B.G->w.p);
            PFEM_TRY(check_kernel("k_rbm_owned_graph"));
            if (nn > 0) PFEM_HIP(hipMemcpyAsync(B.G->diag.p, d_all.p, sizeof(double) * nn, hipMemcpyDeviceToDevice, s->stream));
            PFEM_HIP(hipStreamSynchronize(s->stream));        // (odeg goes out of scope)
        }
    } else if (L.bs == 1 && L.n_loc == L.n) {
        // scalar problem: the matrix itself (rows are sorted and unique already)
        PFEM_TRY(B.G->reserve(L.n, L.nnz));
        const int64_t *rowptr = L.fine ? s->d_rowptr.p : L.rowptr.p;
        PFEM_HIP(hipMemcpyAsync(B.G->ptr.p, rowptr, sizeof(int64_t) * (L.n + 1), hipMemcpyDeviceToDevice, s->stream));
        hipLaunchKernelGGL(k_sell_to_csr, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, A, static_cast<const int64_t *>(B.G->ptr.p), B.G->col.p, B.G->w.p);
        hipLaunchKernelGGL(k_extract_diag, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, A, B.G->diag.p);
        PFEM_TRY(check_kernel("gamg scalar graph"));
    } else {
        DevBuf<uint64_t> &keys = W.keys, &ukeys = W.ukeys;
        DevBuf<double> &vals = W.vals, &sums = W.sums;
        PFEM_TRY(keys.reserve(static_cast<size_t>(L.stored)));
        PFEM_TRY(vals.reserve(static_cast<size_t>(L.stored)));
        const int64_t cnt = L.stored;      // slots of rows beyond this block keep the sentinel key
        PFEM_HIP(hipMemsetAsync(keys.p, 0xff, sizeof(uint64_t) * static_cast<size_t>(L.stored), s->stream));
        PFEM_HIP(hipMemsetAsync(vals.p, 0, sizeof(double) * static_cast<size_t>(L.stored), s->stream));
        hipLaunchKernelGGL(k_amg_emit_node_keys, dim3(grid_for(A.n_slices * 64)), dim3(kBlock), 0, s->stream, A,
                           L.bs > 1 ? static_cast<const int32_t *>(L.node_of.p) : static_cast<const int32_t *>(nullptr), col_limit,
                           L.bs > 1 ? 1 : 0, keys.p, vals.p);
        PFEM_TRY(check_kernel("k_amg_emit_node_keys"));
        int64_t m = 0;
        PFEM_TRY(amg_sort_reduce(s, W, keys, vals, cnt, ukeys, sums, &m));
        PFEM_TRY(amg_graph_from_unique(s, ukeys, sums, m, nn, L.bs > 1 ? 1 : 0, *B.G));
    }
    return PFEM_OK;
}

// the aggregates of the level's nodes (B.node_agg, B.na, their places in B.hint): node bricks in one step, the split bricks found
// before, or passes of pairwise matching -- along the lattice's axes while that pairs, then on the strength graph
int amg_level_aggregates(pfem_solver *s, AmgWork &W, AmgLevel &L, bool coupled, AmgLevelBuild &B, AmgPhaseClock &phase, int l)
{
    const int64_t nn = L.n_nodes, nn_loc = L.bs > 0 ? (coupled ? L.n_loc : L.n) / L.bs : 0;
    PFEM_TRY(B.node_agg.alloc(static_cast<size_t>(std::max<int64_t>(nn, 1))));
    hipLaunchKernelGGL(k_amg_iota, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, B.node_agg.p);
    B.na = nn;
    B.hint = L.hint.p;                              // null: indices
    for (int d = 0; d < 3; ++d) B.lat_hi[d] = L.lat_hi[d];
    B.lat_axis = L.lat_axis;
    B.on_lattice = L.lattice;
    // level 0 of a displacement problem on one rank: five passes, aggregates of up to 32 nodes -- the rigid-body coarse space
    // carries them (see amg_node_bricks for the lattice's case), and level 1 with its 6x6 blocks is the dearest of the cycle:
    // the beam with its nodes moved off the lattice 67 iterations / 116 ms with three passes, 52 / 74 with four, 61 / 72 with
    // five, 59 / 71 with six (profiles/r05/beam_level0_aggregate_sizes.txt)
    const int n_passes = (L.fine && B.rbm && !coupled) ? 5 : kAmgPasses;
    // levels with the rigid-body transfer on a full lattice (one rank): the bricks the passes would end in, in one step
    // (several ranks, round 6: the same across the ranks when the positions are global and every rank's nodes fill a box --
    // L.lat_nodes_global is set from all-reduced verdicts only, the same on every rank)
    if (B.rbm && (coupled ? L.lat_nodes_global : nn_loc == nn) && L.lattice && L.lat_full && (L.hint.p || nn == 0)) {
        PFEM_TRY(amg_node_bricks(s, L, *B.G, B.NB, &B.node_bricks, coupled));
        if (B.node_bricks) {
            B.node_agg.swap(B.NB.node_agg);
            B.na = B.NB.na;
            B.hint = B.NB.hint.p;
            for (int d = 0; d < 3; ++d) B.lat_hi[d] = B.NB.hi[d];
            B.lat_axis = B.NB.axis;
            phase(l, "node bricks: check + aggregates");
        }
    }
    if (B.split_bricks) {
        B.node_agg.swap(B.sb_agg);
        B.na = B.sb_na;
        B.hint = B.sb_pos.p;
        for (int d = 0; d < 3; ++d) B.lat_hi[d] = B.sb_hi[d];
        B.lat_axis = B.sb_axis;
    }
    for (int pass = 0; pass < ((B.node_bricks || B.split_bricks) ? 0 : n_passes); ++pass) {
        DevBuf<int32_t> &step = W.step;
        int64_t na_new = 0;
        bool lattice_pass = L.lattice && B.on_lattice;
        int axis = B.lat_axis;
        if (lattice_pass) {
            // the next axis that still has an extent (a beam runs out of x and z long before y) and along which the nodes
            // do pair: an axis across which the couplings are weak (anisotropic operator) pairs next to nothing and is
            // passed over -- semi-coarsening along the strong axes, still on the lattice
            bool paired = false;
            for (int k = 0; k < 3 && !paired; ++k, axis = (axis + 1) % 3) {
                if (B.lat_hi[axis] < 1) continue;
                PFEM_TRY(amg_match_lattice(s, W, *B.G, B.hint, axis, L.bs > 1, step, &na_new));
                if (na_new * 10 <= B.G->n * 8) { paired = true; break; }
            }
            phase(l, "  lattice pairing");
            if (!paired) {
                // no axis left, or couplings too uneven for the strength threshold everywhere (thin cells of a replicated
                // level): from here on the matching on the strength graph, ties by index
                lattice_pass = B.on_lattice = false;
                B.hint = nullptr;
            }
        }
        if (lattice_pass) {
            DevBuf<int32_t> &nh = (pass & 1) ? B.hint_b : B.hint_a;
            PFEM_TRY(nh.alloc(static_cast<size_t>(std::max<int64_t>(na_new, 1))));
            hipLaunchKernelGGL(k_amg_lat_coarsen, dim3(grid_for(B.G->n)), dim3(kBlock), 0, s->stream, B.G->n, B.hint, static_cast<const int32_t *>(W.match.p),
                               static_cast<const int32_t *>(step.p), 10 * axis, nh.p);
            PFEM_TRY(check_kernel("k_amg_lat_coarsen"));
            B.hint = nh.p;
            B.lat_hi[axis] >>= 1;
            B.lat_axis = (axis + 1) % 3;
        } else {
        PFEM_TRY(amg_match(s, W, *B.G, B.hint, step, &na_new));
        phase(l, "  matching rounds");
        }
        if (B.hint && !lattice_pass) {
            DevBuf<int32_t> &nh = (pass & 1) ? B.hint_b : B.hint_a;
            PFEM_TRY(nh.alloc(static_cast<size_t>(na_new)));
            PFEM_HIP(hipMemsetAsync(nh.p, 0x7f, sizeof(int32_t) * static_cast<size_t>(na_new), s->stream));
            hipLaunchKernelGGL(k_amg_hint_coarsen, dim3(grid_for(B.G->n)), dim3(kBlock), 0, s->stream, B.G->n, B.hint, static_cast<const int32_t *>(step.p), nh.p);
            PFEM_TRY(check_kernel("k_amg_hint_coarsen"));
            B.hint = nh.p;
        }
        hipLaunchKernelGGL(k_amg_compose, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, B.node_agg.p, static_cast<const int32_t *>(step.p));
        PFEM_TRY(check_kernel("k_amg_compose"));
        const bool last = pass + 1 == n_passes || na_new <= 1;
        if (!last) {
            // graph of the aggregates
            DevBuf<uint64_t> &keys = W.keys, &ukeys = W.ukeys;
            DevBuf<double> &vals = W.vals, &sums = W.sums;
            const int64_t cnt = B.G->nnz + B.G->n;
            PFEM_TRY(keys.reserve(static_cast<size_t>(cnt)));
            PFEM_TRY(vals.reserve(static_cast<size_t>(cnt)));
            hipLaunchKernelGGL(k_amg_emit_coarse_graph, dim3(grid_for(B.G->n)), dim3(kBlock), 0, s->stream, B.G->n, B.G->nnz,
                               static_cast<const int64_t *>(B.G->ptr.p), static_cast<const int32_t *>(B.G->col.p), static_cast<const double *>(B.G->w.p),
                               static_cast<const double *>(B.G->diag.p), static_cast<const int32_t *>(step.p), L.bs > 1 ? 1 : 0, keys.p, vals.p);
            PFEM_TRY(check_kernel("k_amg_emit_coarse_graph"));
            int64_t m = 0;
            phase(l, "  emit aggregate graph");
            PFEM_TRY(amg_sort_reduce(s, W, keys, vals, cnt, ukeys, sums, &m));
            phase(l, "  sort + reduce by key");
            B.gcur ^= 1;                                  // the aggregates' graph goes into the other graph object
            PFEM_TRY(amg_graph_from_unique(s, ukeys, sums, m, na_new, 0, W.graphs[B.gcur]));
            B.G = &W.graphs[B.gcur];
        }
        B.na = na_new;
        if (last) break;
    }
    L.agg_kind = B.node_bricks ? kAggNodeBricks : (B.split_bricks ? kAggSplitBricks : (B.on_lattice ? kAggLatticePasses : kAggMatching));
    phase(l, "3 passes of matching");
    return PFEM_OK;
}

// the coarse dofs -- the (aggregate, component) pairs that occur -- and the level they make (Cp): its rows, across ranks its
// neighbour plan, its nodes and their places.  kAmgLastLevel: the coarsening has stalled.
int amg_level_coarse_dofs(pfem_solver *s, AmgWork &W, AmgLevel &L, bool coupled, bool overlap, AmgLevelBuild &B, double n_global,
                          std::unique_ptr<AmgLevel> &Cp, double *nc_global_out)
{
    const int64_t R = coupled ? L.n_loc : L.n, nn = L.n_nodes;
    const int64_t nslots = B.na * L.bs;
    if (coupled) PFEM_TRY(amg_agree(s, nslots > INT_MAX - 8 ? PFEM_ERR_ARG : PFEM_OK));
    else if (nslots > INT_MAX - 8) return PFEM_ERR_ARG;
    DevBuf<int32_t> &flag = W.flag, &rank = W.crank;
    PFEM_TRY(flag.reserve(static_cast<size_t>(nslots) + 1));
    PFEM_TRY(rank.reserve(static_cast<size_t>(nslots) + 1));
    PFEM_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t) * (nslots + 1), s->stream));
    const int32_t *node_of = L.bs > 1 ? L.node_of.p : nullptr, *comp_of = L.bs > 1 ? L.comp_of.p : nullptr;
    hipLaunchKernelGGL(k_amg_mark_cdofs, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, L.n, node_of, comp_of,
                       static_cast<const int32_t *>(B.node_agg.p), L.bs, flag.p);
    PFEM_TRY(amg_exclusive_sum(s, W.temp, flag.p, rank.p, nslots + 1));
    int32_t nc32 = 0;
    PFEM_HIP(hipMemcpyAsync(&nc32, rank.p + nslots, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    const int64_t nc = nc32;
    std::vector<double> nc_of;                   // coupled: coarse dofs of every rank
    double nc_global = static_cast<double>(nc);
    if (coupled) {
        nc_of.assign(static_cast<size_t>(s->nranks), 0.0);
        nc_of[static_cast<size_t>(s->rank)] = static_cast<double>(nc);
        PFEM_TRY(amg_allreduce_host(s, nc_of.data(), s->nranks));
        nc_global = 0.0;
        for (double v : nc_of) nc_global += v;
        if (nc_global < 1.0 || nc_global * 10.0 > n_global * 8.0) return kAmgLastLevel;      // (decided by all ranks alike)
    } else if (nc < 1 || nc * 10 > L.n * 8) {
        return kAmgLastLevel;                    // the coarsening has stalled: this level is the last one
    }
    L.nc = nc;
    PFEM_TRY(L.agg.alloc(static_cast<size_t>(std::max<int64_t>(R, 1))));
    hipLaunchKernelGGL(k_amg_assign_cdofs, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, L.n, node_of, comp_of,
                       static_cast<const int32_t *>(B.node_agg.p), L.bs, static_cast<const int32_t *>(rank.p), L.agg.p);
    PFEM_TRY(check_kernel("k_amg_assign_cdofs"));
    Cp.reset(new (std::nothrow) AmgLevel());
    if (!Cp) return PFEM_ERR_NOMEM;
    AmgLevel &C = *Cp;
    C.n = nc;
    C.n_loc = nc;
    if (coupled) {
        for (int q = 0; q < s->rank; ++q) C.gid_off += static_cast<int64_t>(nc_of[static_cast<size_t>(q)]);
        const int rc = amg_couple_level(s, W, L, C, overlap, 0, nullptr);
        if (rc != PFEM_OK) return rc;
    }
    C.bs = L.bs;
    C.n_nodes = L.bs > 1 ? B.na : nc;
    if (B.hint && C.n_nodes == B.na) {                  // the next level pairs on along the same curve / on the coarser lattice
        C.lattice = L.lattice && B.on_lattice;
        for (int d = 0; d < 3; ++d) C.lat_hi[d] = B.lat_hi[d];
        C.lat_axis = B.lat_axis;
        if (L.xyz.p && B.na > 0) {
            DevBuf<unsigned long long> keys;
            PFEM_TRY(keys.alloc(static_cast<size_t>(3 * B.na)));
            PFEM_TRY(C.xyz.alloc(static_cast<size_t>(3 * B.na)));
            PFEM_HIP(hipMemsetAsync(keys.p, 0xff, sizeof(unsigned long long) * static_cast<size_t>(3 * B.na), s->stream));
            hipLaunchKernelGGL(k_amg_xyz_min, dim3(grid_for(nn)), dim3(kBlock), 0, s->stream, nn, static_cast<const int32_t *>(B.node_agg.p),
                               static_cast<const double *>(L.xyz.p), B.na, keys.p);
            hipLaunchKernelGGL(k_amg_xyz_decode, dim3(grid_for(3 * B.na)), dim3(kBlock), 0, s->stream, 3 * B.na,
                               static_cast<const unsigned long long *>(keys.p), C.xyz.p);
            PFEM_TRY(check_kernel("k_amg_xyz_min"));
            PFEM_HIP(hipStreamSynchronize(s->stream));
        }
        PFEM_TRY(C.hint.alloc(static_cast<size_t>(std::max<int64_t>(B.na, 1))));
        if (B.na > 0) PFEM_HIP(hipMemcpyAsync(C.hint.p, B.hint, sizeof(int32_t) * static_cast<size_t>(B.na), hipMemcpyDeviceToDevice, s->stream));
        if (B.split_bricks) {             // the next level splits its bricks the same way: the box of this rank's owned coarse positions, the positions' coordinates
            C.lat_split = true;
            for (int d = 0; d < 3; ++d) { C.lat_tlo[d] = L.lat_tlo[d] >> B.sb_shift[d]; C.lat_thi[d] = L.lat_thi[d] >> B.sb_shift[d]; }
            C.lat_coord.assign(3 * 1024, 0.0);
            if (L.lat_coord.size() == 3 * 1024)
                for (int d = 0; d < 3; ++d)
                    for (int pc = 0; pc <= B.lat_hi[d] && pc < 1024; ++pc) C.lat_coord[static_cast<size_t>(1024 * d + pc)] = L.lat_coord[static_cast<size_t>(1024 * d + std::min(pc << B.sb_shift[d], 1023))];
        }
    }
    if (L.bs > 1) {
        PFEM_TRY(C.node_of.alloc(static_cast<size_t>(nc)));
        PFEM_TRY(C.comp_of.alloc(static_cast<size_t>(nc)));
        hipLaunchKernelGGL(k_amg_coarse_nodes, dim3(grid_for(nslots)), dim3(kBlock), 0, s->stream, nslots, L.bs,
                           static_cast<const int32_t *>(flag.p), static_cast<const int32_t *>(rank.p), C.node_of.p, C.comp_of.p);
        PFEM_TRY(check_kernel("k_amg_coarse_nodes"));
    }
    *nc_global_out = nc_global;
    return PFEM_OK;
}

// coarse pattern and the maps of the numeric Galerkin product: (coarse row, coarse col, fine slot) triples, sorted.
// (A formulation by coarse rows -- one thread per coarse row, its column set and its sums in LDS, the fine matrix read in
// its own order, no sort -- was built and measured in round 3: numeric phase 3.96 instead of 2.28 ms at config 3, the
// thread's chain of dependent loads over its 8 member rows is latency-bound.  Dropped.)
int amg_level_maps(pfem_solver *s, AmgWork &W, AmgLevel &L, AmgLevel &C, int64_t R)
{
    DevBuf<uint64_t> &keys = W.keys;
    DevBuf<uint64_t> ukeys;                       // (as long as the coarse matrix has entries: exact)
    DevBuf<int32_t> &slots = W.slots;
    PFEM_TRY(keys.reserve(static_cast<size_t>(L.stored)));
    PFEM_TRY(slots.reserve(static_cast<size_t>(L.stored)));
    PFEM_HIP(hipMemsetAsync(keys.p, 0xff, sizeof(uint64_t) * static_cast<size_t>(L.stored), s->stream));   // slots of ghost rows
    PFEM_HIP(hipMemsetAsync(slots.p, 0, sizeof(int32_t) * static_cast<size_t>(L.stored), s->stream));
    const SellDev Ar = amg_sell(s, L, R);
    hipLaunchKernelGGL(k_amg_emit_rap_keys, dim3(grid_for(Ar.n_slices * 64)), dim3(kBlock), 0, s->stream, Ar,
                       static_cast<const int32_t *>(L.agg.p), static_cast<int32_t>(R), keys.p, slots.p);
    PFEM_TRY(check_kernel("k_amg_emit_rap_keys"));
    PFEM_TRY(L.src_slot.alloc(static_cast<size_t>(L.stored)));
    int64_t nnz_c = 0;
    PFEM_TRY(amg_pattern_from_keys(s, W, L.stored, L.src_slot.p, L.src_ptr, ukeys, &nnz_c));
    PFEM_TRY(amg_drop_sentinel_run(s, ukeys.p, &nnz_c));          // (the slots of ghost rows and of the padding)
    L.nnz_c = nnz_c;
    PFEM_TRY(amg_store_pattern(s, W, ukeys.p, nnz_c, C, L.dst_slot));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    return PFEM_OK;
}

int amg_build_levels(pfem_solver *s, Amg &M, AmgWork &W, bool coupled, bool overlap)
{
    AmgPhaseClock phase{s->stream, amg_verbose(), std::chrono::steady_clock::now()};
    phase(-1, "level 0 nodes + curve places");
    double n_global = static_cast<double>(M.lev[0]->n);       // rows of the current level over all ranks (coupled)
    if (coupled) PFEM_TRY(amg_allreduce_host(s, &n_global, 1));
    for (int l = 0; l + 1 < kAmgMaxLevels; ++l) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        if (coupled ? n_global <= kAmgDense : L.n <= kAmgDense) break;
        const SellDev A = amg_sell(s, L);
        const int64_t R = coupled ? L.n_loc : L.n;           // rows (and columns) that take part in the Galerkin product
        bool replicated = false;
        // ---- a scalar level on a lattice: bricks in one step
        // (several ranks: L.lat_global is the same on every rank -- set from all-reduced verdicts only)
        if (L.lattice && L.bs == 1 && (coupled ? L.lat_global : L.n_loc == L.n) && L.hint.p) {
            bool done = false;
            const int rc = amg_bricks_level(s, M, W, L, A, phase, l, &done, coupled, overlap, &n_global);
            if (rc == kAmgLastLevel) break;
            if (rc != PFEM_OK) return rc;
            if (done) {
                if (!coupled) n_global = static_cast<double>(M.lev.back()->n);
                PFEM_TRY(amg_replicate_rest(s, M, W, coupled, n_global, overlap, phase, l, &replicated));
                if (replicated) break;
                continue;
            }
        }
        // ---- the aggregates of the level's nodes
        AmgLevelBuild B;
        PFEM_TRY(amg_level_split_bricks(s, W, L, A, coupled, B, phase, l));
        PFEM_TRY(amg_level_graph(s, M, W, L, A, coupled, B));
        phase(l, "strength graph");
        PFEM_TRY(amg_level_aggregates(s, W, L, coupled, B, phase, l));
        // ---- the level below, with the rigid-body transfer ...
        if (B.rbm) {
            const int rc = amg_rbm_level(s, M, W, L, B.node_agg, B.na, B.hint, B.on_lattice, B.lat_hi, B.lat_axis, phase, l, coupled, overlap, &n_global,
                                         B.node_bricks ? B.NB.nbk : nullptr);
            if (rc == kAmgLastLevel) break;
            if (rc != PFEM_OK) return rc;
            if (B.node_bricks) {              // the coarse nodes fill their box of positions again
                AmgLevel &Cn = *M.lev.back();
                Cn.lat_full = true;
                for (int d = 0; d < 3; ++d) { Cn.lat_tlo[d] = B.NB.tlo[d]; Cn.lat_thi[d] = B.NB.thi[d]; }
                if (coupled) {              // ... every rank's, in the same global brick coordinates: the next level cuts its bricks at the same borders
                    Cn.lat_nodes_global = true;
                    for (int d = 0; d < 3; ++d) Cn.lat_str[d] = B.NB.str[d];
                }
            }
            PFEM_TRY(amg_replicate_rest(s, M, W, coupled, n_global, overlap, phase, l, &replicated));
            if (replicated) break;
            continue;
        }
        // ---- ... or with one coarse dof per aggregate and component: coarse dofs, member lists, maps and pattern
        std::unique_ptr<AmgLevel> Cp;
        double nc_global = 0.0;
        const int rc = amg_level_coarse_dofs(s, W, L, coupled, overlap, B, n_global, Cp, &nc_global);
        if (rc == kAmgLastLevel) break;
        if (rc != PFEM_OK) return rc;
        PFEM_TRY(amg_member_lists(s, W, L, L.agg.p, R, Cp->n_loc, 32));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        phase(l, "coarse dofs + member lists");
        PFEM_TRY(amg_level_maps(s, W, L, *Cp, R));
        phase(l, "Galerkin maps + coarse pattern");
        if (coupled) PFEM_TRY(amg_agree(s, Cp->stored > INT_MAX ? PFEM_ERR_ARG : PFEM_OK));
        else if (Cp->stored > INT_MAX) return PFEM_ERR_ARG;
        M.lev.push_back(std::move(Cp));
        // the next level's strength graph needs this level's VALUES: one numeric product right away
        amg_galerkin(s, L, *M.lev.back(), A);
        PFEM_TRY(check_kernel("k_amg_galerkin (symbolic)"));
        n_global = nc_global;
        PFEM_TRY(amg_replicate_rest(s, M, W, coupled, n_global, overlap, phase, l, &replicated));
        if (replicated) break;
    }
    M.n_last_global = coupled ? static_cast<int64_t>(n_global) : M.lev.back()->n;
    return PFEM_OK;
}

// What the tail's LDS layout depends on (tail_view): the levels' rows, their transfers' kind, the first level's stored slots.
void amg_tail_shape(const Amg &M, int tail, AmgTail &T)
{
    T.nlev = static_cast<int>(M.lev.size()) - tail;
    for (int q = 0; q < T.nlev; ++q) {
        const AmgLevel &L = *M.lev[static_cast<size_t>(tail + q)];
        T.lev[q].n = L.n;
        T.lev[q].rbm_dim = L.rbm ? L.dim : 0;
        T.lev[q].stored = L.stored;
        T.lev[q].A.n_slices = (L.n + 63) / 64;
    }
}
// dynamic LDS of k_amg_tail: the vectors alone decide whether the tail works out of LDS (64 KB of them at most, as before the lists
// came); the LDS builds then take vectors + index lists (vec_b, up to 16 KB more) and, when it fits beside them, the first level's matrix
struct TailLds { size_t vecs_b, vec_b, mat_b; };
TailLds tail_lds_bytes(const AmgTail &T)
{
    int64_t rows = 0, ints = 0;
    for (int q = 0; q < T.nlev; ++q) { rows += T.lev[q].n; ints += tail_idx_ints(T, q); }
    TailLds W;
    W.vecs_b = static_cast<size_t>(6 * rows) * sizeof(double);
    W.vec_b = static_cast<size_t>(6 * rows + ((ints + 1) >> 1)) * sizeof(double);
    const AmgTailLevel &t0 = T.lev[0];
    W.mat_b = (T.nlev > 1 && t0.stored > 0) ? static_cast<size_t>(t0.stored) * 12 + static_cast<size_t>(t0.A.n_slices + 2) * 8 : 0;
    return W;
}
constexpr size_t kAmgTailLdsMax = 156 * 1024;

// vectors of every level, the dense bottom, which levels the fused kernels take
int amg_finish_levels(pfem_solver *s, Amg &M, bool coupled)
{
    for (auto &L : M.lev) PFEM_TRY(amg_alloc_vectors(s, *L));
    AmgLevel &last = *M.lev.back();
    const int64_t n_last = M.n_last_global;
    M.dense = n_last >= 1 && n_last <= kAmgDense && M.lev.size() > 1 && !M.rep;
    if (M.dense) {
        PFEM_TRY(M.dense_inv.alloc(static_cast<size_t>(n_last * n_last)));
        const int bytes = static_cast<int>(n_last * n_last * sizeof(double));
        if (bytes > 65536) {
            PFEM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_amg_dense_inverse), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
            PFEM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_amg_dense_inverse_of), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        }
        if (coupled) {          // the last level's operator is summed over the ranks into one dense matrix every rank inverts
            PFEM_TRY(M.dense_glob.alloc(static_cast<size_t>(n_last * n_last)));
            PFEM_TRY(M.bx_glob.alloc(static_cast<size_t>(2 * kAmgDense)));
            PFEM_TRY(amg_level_gids(s, last));
        }
    }
    if (coupled) PFEM_TRY(M.lam_all.alloc(static_cast<size_t>(std::max<int64_t>(256, 2 * static_cast<int64_t>(M.lev.size()) * s->nranks))));
    M.fused = !coupled && [] { const char *e = std::getenv("PFEM_AMG_FUSED"); return e ? std::atoi(e) != 0 : true; }();
    M.tail_from = -1;
    for (size_t l = 1; l < M.lev.size() && !coupled; ++l)
        // (and few nonzeros: one workgroup is latency-bound, and a level of 6-dof nodes has 100+ entries per row -- the beam's
        // 918-row level inside the tail cost 186 us per cycle, three fused launches outside it cost less: 46.6 -> 44.0 ms per step)
        if (M.lev[l]->n <= kAmgTailRows && M.lev[l]->nnz <= kAmgTailNnz && M.lev.size() - l <= static_cast<size_t>(kAmgTailLevels)) { M.tail_from = static_cast<int>(l); break; }
    M.w_to = M.tail_from > 0 ? M.tail_from : static_cast<int>(M.lev.size()) - 2;
    // the tail kernel works out of LDS (k_amg_tail): more than 64 KB of dynamic LDS has to be allowed per kernel, here, outside any
    // stream capture -- the build with the matrix for vectors + lists + matrix, the build without it for vectors + lists
    M.tail_lds_allowed = M.tail_vec_allowed = 0;
    M.tail_build = 0;
    if (M.tail_from > 0) {
        AmgTail T{};
        amg_tail_shape(M, M.tail_from, T);
        const TailLds W = tail_lds_bytes(T);
        const size_t need = W.vec_b + W.mat_b;
        auto allow = [](const void *k) {
            if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kAmgTailLdsMax)) == hipSuccess) return kAmgTailLdsMax;
            (void)hipGetLastError();
            return static_cast<size_t>(0);
        };
        if (W.vecs_b <= 65536 && W.mat_b > 0 && need > 65536 && need <= kAmgTailLdsMax) M.tail_lds_allowed = allow(reinterpret_cast<const void *>(k_amg_tail<true, true>));
        if (W.vecs_b <= 65536 && W.vec_b > 65536) M.tail_vec_allowed = allow(reinterpret_cast<const void *>(k_amg_tail<true, false>));
    }
    return PFEM_OK;
}


// The smoothing interval and the coarse-grid scale in effect: the switch, else the value pfem_solver_set_amg_options gave, else
// the automatic one of the last symbolic phase.  Taken at the symbolic and at every numeric phase: a knob the caller returns to
// automatic on a hierarchy that is kept gets that hierarchy's automatic value, not the one it was given before.
void amg_knobs(Amg &M)
{
    const char *er = std::getenv("PFEM_AMG_EIG_RATIO"), *cs = std::getenv("PFEM_AMG_COARSE_SCALE");
    M.eig_ratio = er ? std::max(1.5, std::atof(er)) : (M.eig_ratio_given ? M.eig_ratio_opt : M.eig_ratio_auto);
    M.coarse_scale = cs ? std::atof(cs) : (M.coarse_scale_given ? M.coarse_scale_opt : M.coarse_scale_auto);
    if (M.rep) { M.rep->eig_ratio = M.eig_ratio; M.rep->coarse_scale = M.coarse_scale; }      // (the replicated tail: a copy at set-up)
}

// ---- symbolic phase: aggregates and Galerkin maps of every level (needs the matrix values: strength of connection) ----
int amg_symbolic(pfem_solver *s, bool multi, bool overlap)
{
    if (!s->amg) s->amg.reset(new (std::nothrow) Amg());
    if (!s->amg) return PFEM_ERR_NOMEM;
    Amg &M = *s->amg;
    const auto t0 = std::chrono::steady_clock::now();
    const bool verbose = amg_verbose();
    const size_t malloc_calls0 = dev_pool().st_malloc_calls;         // (PFEM_POOL_VERBOSE: what the phase spent inside hipMalloc)
    const size_t malloc_bytes0 = dev_pool().st_malloc;
    const double malloc_ms0 = dev_pool().st_malloc_ms;
    const size_t reused0 = dev_pool().st_reused;
    auto since_t0 = [&](const char *what) {          // PFEM_AMG_VERBOSE: where the symbolic phase is, on stderr
        if (!verbose) return;
        (void)hipStreamSynchronize(s->stream);
        std::fprintf(stderr, "  gamg symbolic: %-40s at %9.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    // several ranks: one hierarchy across the ranks unless PFEM_AMG_COUPLED=0 asks for one per rank (block Jacobi) or the
    // ranks cannot form it (more than 52 of them; found below, by all ranks together)
    M.coupled = multi && !M.coupled_refused && [] { const char *e = std::getenv("PFEM_AMG_COUPLED"); return e ? std::atoi(e) != 0 : true; }();
    const bool coupled = M.coupled;
    if (const char *e = std::getenv("PFEM_AMG_CHEB_DEGREE")) M.cheb_degree = std::max(1, std::min(6, std::atoi(e)));
    if (const char *e = std::getenv("PFEM_AMG_FINE_DEGREE")) M.fine_degree = std::max(0, std::min(6, std::atoi(e)));
    M.lev.clear();
    M.rep.reset();
    M.cc_builds = 0;
    M.cc_used.clear();
    M.rbm = false;
    M.symbolic_ok = false;
    M.dense = false;
    M.graph.invalidate();
    {
        const int rc_size = s->stored > INT_MAX ? PFEM_ERR_ARG : PFEM_OK;
        if (rc_size != PFEM_OK) set_last_error("gamg: more than 2^31-1 stored matrix entries on one device");
        if (coupled) PFEM_TRY(amg_agree(s, rc_size));          // (several ranks: they stop together)
        else PFEM_TRY(rc_size);
    }
    std::unique_ptr<AmgWork> Wp(new (std::nothrow) AmgWork());
    if (!Wp) return PFEM_ERR_NOMEM;
    AmgWork &W = *Wp;
    {
        std::unique_ptr<AmgLevel> L0(new (std::nothrow) AmgLevel());
        if (!L0) return PFEM_ERR_NOMEM;
        L0->fine = true;
        L0->n = s->n_owned;                      // one rank: all rows; several ranks: the rows this rank owns
        L0->n_loc = s->n_loc;
        L0->gid_off = s->row_start;
        L0->n_slices = (s->n_owned + 63) / 64;
        L0->stored = s->stored;                  // slots of the whole local matrix are addressable
        L0->nnz = s->nnz;
        // dofs of one node: the row groups the SpMV found (consecutive rows with identical column sets, at most 3)
        // (several ranks: a node's dofs are all owned or all ghosts and the owned rows come first, so the owned nodes are the
        // groups that start below n_owned)
        int64_t owned_groups = s->n_groups;
        if (s->grouped && s->n_groups > 0 && s->n_ghost > 0) {
            std::vector<int32_t> row0(static_cast<size_t>(s->n_groups));
            PFEM_HIP(hipMemcpyAsync(row0.data(), s->d_group_row0.p, sizeof(int32_t) * row0.size(), hipMemcpyDeviceToHost, s->stream));
            PFEM_HIP(hipStreamSynchronize(s->stream));
            owned_groups = std::lower_bound(row0.begin(), row0.end(), static_cast<int32_t>(s->n_owned)) - row0.begin();
        }
        if (s->grouped && owned_groups > 0 && owned_groups < s->n_owned) {
            L0->bs = kGroupRows;
            L0->n_nodes = owned_groups;
            PFEM_TRY(L0->node_of.alloc(static_cast<size_t>(s->n_loc)));
            PFEM_TRY(L0->comp_of.alloc(static_cast<size_t>(s->n_loc)));
            hipLaunchKernelGGL(k_row_group_index, dim3(grid_for(s->n_groups)), dim3(kBlock), 0, s->stream,
                               static_cast<const int32_t *>(s->d_group_row0.p), s->n_groups, L0->node_of.p);
            hipLaunchKernelGGL(k_amg_comp_of, dim3(grid_for(s->n_loc)), dim3(kBlock), 0, s->stream, s->n_loc,
                               static_cast<const int32_t *>(L0->node_of.p), static_cast<const int32_t *>(s->d_group_row0.p), L0->comp_of.p);
            PFEM_TRY(check_kernel("k_amg_comp_of"));
        } else {
            L0->bs = 1;
            L0->n_nodes = s->n_owned;
        }
        // displacement problems (as many dofs per node as space dimensions) whose nodes are whole -- all dofs of a node free and
        // consecutive --: candidates for the rigid-body-mode coarse space; nodes = runs of ndof dofs, coordinates from the mesh
        // (one rank for now: a hierarchy across the ranks keeps the translations)
        // (several ranks: for the hierarchy across the ranks, ghost nodes included; the ranks decide together)
        if (!multi || coupled) {
            const int nd = s->mesh.ndof;
            bool cand = s->have_mesh && nd == s->mesh.ndim && nd >= 2 && s->n_owned % nd == 0 && s->n_loc % nd == 0 && (multi || s->n_owned >= 2 * nd);
            const int64_t nn0 = cand ? s->n_loc / nd : 0;
            if (cand) {
                DevBuf<int> d_bad;
                PFEM_TRY(d_bad.alloc(1));
                PFEM_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), s->stream));
                PFEM_TRY(L0->cen.alloc(static_cast<size_t>(std::max<int64_t>(3 * nn0, 1))));
                PFEM_HIP(hipMemsetAsync(L0->cen.p, 0, sizeof(double) * static_cast<size_t>(std::max<int64_t>(3 * nn0, 1)), s->stream));
                if (s->mesh.nElem > 0)
                    hipLaunchKernelGGL(k_rbm_mesh_xyz, dim3(grid_for(s->mesh.nElem * s->mesh.npe)), dim3(kBlock), 0, s->stream, s->mesh, nn0, L0->cen.p, d_bad.p);
                PFEM_TRY(check_kernel("k_rbm_mesh_xyz"));
                int bad = 0;
                PFEM_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s->stream));
                PFEM_HIP(hipStreamSynchronize(s->stream));
                cand = !bad;
            }
            if (multi) {
                double no = cand ? 0.0 : 1.0;
                PFEM_TRY(amg_allreduce_host(s, &no, 1));
                cand = cand && no == 0.0;
            }
            if (cand) {
                L0->dim = nd;
                L0->bs = nd;
                L0->n_nodes = s->n_owned / nd;
                PFEM_TRY(L0->node_of.alloc(static_cast<size_t>(std::max<int64_t>(s->n_loc, 1))));
                PFEM_TRY(L0->comp_of.alloc(static_cast<size_t>(std::max<int64_t>(s->n_loc, 1))));
                hipLaunchKernelGGL(k_rbm_node_comp, dim3(grid_for(s->n_loc)), dim3(kBlock), 0, s->stream, s->n_loc, nd, L0->node_of.p, L0->comp_of.p);
                PFEM_TRY(check_kernel("k_rbm_node_comp"));
            } else {
                L0->cen.release();
            }
        }
        // the mesh came with coordinates (and was not renumbered along the curve already): the pairing breaks its ties by the
        // nodes' places along a Morton curve instead of their indices -- on the 200^3 lattice, whose lines have an odd
        // number of nodes, that makes 2x2x2 bricks where index parity leaves halves over: 23 -> 18 iterations
        bool lattice = false;
        // (a lattice is a property of the coordinates: found under any numbering, the library's own Morton renumbering included)
        // Scalar problem, one hierarchy across the ranks: GLOBAL positions of all local dofs, so that the levels can take their
        // bricks in one step there too (amg_bricks_level; collective -- every rank of such a solve comes through here)
        bool lattice_global = false, lattice_split = false;
        if (coupled && L0->bs == 1 && L0->dim == 0) {
            since_t0("nodes of level 0");
            PFEM_TRY(lattice_positions_global(s, *L0, &lattice_global));
            since_t0("global lattice looked for");
            lattice = lattice_global;
            if (!lattice_global && !std::getenv("PFEM_AMG_SPLIT_BRICKS_OFF")) {
                // a lattice, but some rank's dofs do not fill a box of it (a METIS-like partition): the bricks are split between their owners
                PFEM_TRY(lattice_positions_global(s, *L0, &lattice_split, false, true));
                since_t0("global lattice looked for again, without boxes");
                lattice = lattice_split;
            }
        }
        // Displacement problem with the rigid-body transfer, one hierarchy across the ranks (round 6): GLOBAL positions of the nodes,
        // so that level 0 -- and every level below it while it stays distributed -- takes its node bricks in one step as on one rank
        // (amg_node_bricks; without this the ranks paired in three passes and kept the 2x2x2 aggregates whose 6x6-block level 1 is
        // the dearest of the cycle).  (L0->dim is agreed above; collective.)
        if (coupled && L0->dim > 0 && L0->bs == L0->dim) {
            since_t0("nodes of level 0");
            PFEM_TRY(lattice_positions_global(s, *L0, &lattice_global, true));
            since_t0("global lattice of the nodes looked for");
            lattice = lattice_global;
        }
        if (s->have_mesh && (s->n_owned > 1 || lattice_global || lattice_split)) {
            DevBuf<int32_t> pos;
            int hi[3] = {0, 0, 0};
            since_t0("nodes of level 0");
            if (!lattice_global && !lattice_split) PFEM_TRY(lattice_positions(s, pos, &lattice, hi));
            since_t0("lattice looked for");
            if (lattice) {
                L0->lattice = true;
                if (!lattice_global && !lattice_split) {
                for (int d = 0; d < 3; ++d) L0->lat_hi[d] = hi[d];
                PFEM_TRY(L0->hint.alloc(static_cast<size_t>(L0->n_nodes)));
                PFEM_HIP(hipMemsetAsync(L0->hint.p, 0, sizeof(int32_t) * static_cast<size_t>(L0->n_nodes), s->stream));
                hipLaunchKernelGGL(k_amg_node_hint, dim3(grid_for(L0->n)), dim3(kBlock), 0, s->stream, L0->n,
                                   L0->bs > 1 ? static_cast<const int32_t *>(L0->node_of.p) : static_cast<const int32_t *>(nullptr),
                                   L0->bs > 1 ? static_cast<const int32_t *>(L0->comp_of.p) : static_cast<const int32_t *>(nullptr),
                                   static_cast<const int32_t *>(pos.p), 1, L0->hint.p);
                PFEM_TRY(check_kernel("k_amg_node_hint (lattice)"));
                if (!coupled && L0->dim > 0 && L0->n_nodes > 0) {       // do the nodes fill a box of positions?  (node bricks in one step)
                    DevBuf<int> d_box;
                    int box[6] = {1023, 1023, 1023, 0, 0, 0};
                    PFEM_TRY(d_box.alloc(6));
                    PFEM_HIP(hipMemcpyAsync(d_box.p, box, sizeof box, hipMemcpyHostToDevice, s->stream));
                    hipLaunchKernelGGL(k_lat_bbox, dim3(std::min<unsigned>(grid_for(L0->n_nodes), kLatBoxBlocks)), dim3(kBlock), 0, s->stream, L0->n_nodes,
                                       static_cast<const int32_t *>(L0->hint.p), d_box.p);
                    PFEM_TRY(check_kernel("k_lat_bbox (nodes)"));
                    PFEM_HIP(hipMemcpyAsync(box, d_box.p, sizeof box, hipMemcpyDeviceToHost, s->stream));
                    PFEM_HIP(hipStreamSynchronize(s->stream));
                    int64_t vol = 1;
                    for (int d = 0; d < 3; ++d) { L0->lat_tlo[d] = box[d]; L0->lat_thi[d] = box[3 + d]; vol *= box[3 + d] - box[d] + 1; }
                    L0->lat_full = vol == L0->n_nodes;
                }
                }
                if (coupled && L0->n_nodes > 0 && !lattice_global && !lattice_split) {          // coordinates travel down the levels: the replicated level finds its own lattice from them
                    PFEM_TRY(L0->xyz.alloc(static_cast<size_t>(3 * L0->n_nodes)));
                    PFEM_HIP(hipMemsetAsync(L0->xyz.p, 0, sizeof(double) * static_cast<size_t>(3 * L0->n_nodes), s->stream));
                    hipLaunchKernelGGL(k_amg_node_xyz, dim3(grid_for(s->mesh.nElem * s->mesh.npe)), dim3(kBlock), 0, s->stream, s->mesh, s->n_owned,
                                       L0->bs > 1 ? static_cast<const int32_t *>(L0->node_of.p) : static_cast<const int32_t *>(nullptr), L0->n_nodes, L0->xyz.p);
                    PFEM_TRY(check_kernel("k_amg_node_xyz"));
                }
                PFEM_HIP(hipStreamSynchronize(s->stream));
            }
        }
        if (!lattice && s->have_mesh && !s->reordered && s->n_owned > 1) {
            DevBuf<int32_t> rank;
            if (morton_rank(s, rank) == PFEM_OK) {
                PFEM_TRY(L0->hint.alloc(static_cast<size_t>(L0->n_nodes)));
                PFEM_HIP(hipMemsetAsync(L0->hint.p, 0, sizeof(int32_t) * static_cast<size_t>(L0->n_nodes), s->stream));
                hipLaunchKernelGGL(k_amg_node_hint, dim3(grid_for(L0->n)), dim3(kBlock), 0, s->stream, L0->n,
                                   L0->bs > 1 ? static_cast<const int32_t *>(L0->node_of.p) : static_cast<const int32_t *>(nullptr),
                                   L0->bs > 1 ? static_cast<const int32_t *>(L0->comp_of.p) : static_cast<const int32_t *>(nullptr),
                                   static_cast<const int32_t *>(rank.p), L0->bs, L0->hint.p);
                PFEM_TRY(check_kernel("k_amg_node_hint"));
                PFEM_HIP(hipStreamSynchronize(s->stream));
            }
        }
        // (with rigid-body modes the coarse space is no longer piecewise constant in what matters: the over-correction goes back to 1.5)
        M.coarse_scale_auto = (L0->bs == kGroupRows && L0->dim == 0) ? 1.8 : 1.5;
        // (smoothing interval: measured per kind -- with rigid-body modes the beam takes 24 iterations at 8, 18 at 16 and at 30)
        M.eig_ratio_auto = (L0->bs > 1 && L0->dim == 0) ? 8.0 : 16.0;
        amg_knobs(M);
        M.lev.push_back(std::move(L0));
    }
    since_t0("level 0 described (nodes, lattice)");
    PFEM_TRY(amg_build_levels(s, M, W, coupled, overlap));
    since_t0("levels built");
    PFEM_TRY(amg_finish_levels(s, M, coupled));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    since_t0("vectors, tail, bottom solve");
    Wp.reset();                  // the phase's work buffers go back to the device
    M.symbolic_ok = true;
    M.galerkin_fresh = true;
    if (M.rep) M.rep->galerkin_fresh = true;
    M.symbolic_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (std::getenv("PFEM_POOL_VERBOSE"))
        std::fprintf(stderr, "  gamg symbolic phase %.2f ms: %zu hipMalloc calls of %.3f GB taking %.2f ms, %.2f GB taken from the pool\n", M.symbolic_ms,
                     dev_pool().st_malloc_calls - malloc_calls0, (dev_pool().st_malloc - malloc_bytes0) / 1e9, dev_pool().st_malloc_ms - malloc_ms0,
                     (dev_pool().st_reused - reused0) / 1e9);
    since_t0("work buffers released");
    return PFEM_OK;
}
// ---- numeric phase, every solve: coarse values, inverse diagonals, eigenvalue bounds, the coarsest inverse -------------
// coupled hierarchy: diagonals and absolute row sums are summed over the holders, the bounds maximised over the ranks, the
// last level's operator summed into one dense matrix that every rank inverts
int amg_numeric(pfem_solver *s, Amg &M, bool overlap);
int amg_value_codes(pfem_solver *s, Amg &M);
int amg_numeric_coupled(pfem_solver *s, Amg &M, bool overlap)
{
    const int nl = static_cast<int>(M.lev.size());
    const bool fresh = M.galerkin_fresh;          // (the same on every rank: set by the symbolic phase of this very solve)
    M.galerkin_fresh = false;
    PFEM_HIP(hipMemsetAsync(M.lam_all.p, 0, sizeof(double) * static_cast<size_t>(2 * nl) * s->nranks, s->stream));
    for (int l = 0; l < nl; ++l) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        const SellDev A = amg_sell(s, L, L.n_loc);
        if (l + 1 < nl && !fresh) {
            if (L.rbm) amg_rbm_galerkin(s, L, *M.lev[static_cast<size_t>(l) + 1], A);
            else amg_galerkin(s, L, *M.lev[static_cast<size_t>(l) + 1], A);
        }
        const unsigned g = grid_for(L.n_loc);
        hipLaunchKernelGGL(k_amg_diag_abs, dim3(g), dim3(kBlock), 0, s->stream, A, L.t.p, L.r.p);
        PFEM_TRY(check_kernel("k_amg_diag_abs"));
        PFEM_TRY(exchange_sum(s, amg_plan(s, L), L.t.p, overlap));
        PFEM_TRY(exchange_sum(s, amg_plan(s, L), L.r.p, overlap));
        hipLaunchKernelGGL(k_amg_dinv_ratio, dim3(g), dim3(kBlock), 0, s->stream, L.n_loc, static_cast<const double *>(L.t.p),
                           static_cast<const double *>(L.r.p), L.dinv.p, L.part_max.p);
        hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, s->stream, static_cast<const double *>(L.part_max.p), static_cast<int64_t>(g),
                           M.lam_all.p + static_cast<size_t>(l) * s->nranks + s->rank);
        if (M.rbm) {          // second bound: the shares' |.| row sums of the symmetrically scaled operator, summed over the holders
            hipLaunchKernelGGL(k_rbm_bound_sym, dim3(g), dim3(kBlock), 0, s->stream, A, static_cast<int32_t>(L.n_loc), static_cast<const double *>(L.dinv.p),
                               L.r.p, L.part_max.p);
            PFEM_TRY(check_kernel("k_rbm_bound_sym"));
            PFEM_TRY(exchange_sum(s, amg_plan(s, L), L.r.p, overlap));
            hipLaunchKernelGGL(k_rbm_block_max, dim3(g), dim3(kBlock), 0, s->stream, L.n_loc, static_cast<const double *>(L.r.p), L.part_max.p);
            hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, s->stream, static_cast<const double *>(L.part_max.p), static_cast<int64_t>(g),
                               M.lam_all.p + static_cast<size_t>(nl + l) * s->nranks + s->rank);
        }
    }
    PFEM_TRY(check_kernel("gamg numeric (coupled)"));
    PFEM_TRY(s->comm->allreduce(M.lam_all.p, static_cast<int64_t>(M.rbm ? 2 * nl : nl) * s->nranks, s->stream));
    for (int l = 0; l < nl; ++l) {
        hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, s->stream, static_cast<const double *>(M.lam_all.p + static_cast<size_t>(l) * s->nranks),
                           static_cast<int64_t>(s->nranks), M.lev[static_cast<size_t>(l)]->lam.p);
        if (M.rbm) {
            if (!M.lam2.p) PFEM_TRY(M.lam2.alloc(1));
            hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, s->stream, static_cast<const double *>(M.lam_all.p + static_cast<size_t>(nl + l) * s->nranks),
                               static_cast<int64_t>(s->nranks), M.lam2.p);
            hipLaunchKernelGGL(k_rbm_min2, dim3(1), dim3(64), 0, s->stream, static_cast<const double *>(M.lam2.p), M.lev[static_cast<size_t>(l)]->lam.p);
        }
    }
    if (M.dense) {
        AmgLevel &L = *M.lev.back();
        const int ng = static_cast<int>(M.n_last_global);
        PFEM_HIP(hipMemsetAsync(M.dense_glob.p, 0, sizeof(double) * static_cast<size_t>(ng) * ng, s->stream));
        hipLaunchKernelGGL(k_amg_dense_scatter, dim3(grid_for(L.n_loc)), dim3(kBlock), 0, s->stream, amg_sell(s, L, L.n_loc),
                           static_cast<const int32_t *>(L.gid.p), ng, M.dense_glob.p);
        PFEM_TRY(s->comm->allreduce(M.dense_glob.p, static_cast<int64_t>(ng) * ng, s->stream));
        hipLaunchKernelGGL(k_amg_dense_inverse_of, dim3(1), dim3(1024), static_cast<size_t>(ng) * ng * sizeof(double), s->stream,
                           static_cast<const double *>(M.dense_glob.p), ng, M.dense_inv.p);
        PFEM_TRY(check_kernel("k_amg_dense_inverse_of"));
    }
    if (M.rep) {
        if (!fresh) PFEM_TRY(amg_replicate_values(s, M));
        PFEM_TRY(amg_numeric(s, *M.rep, overlap));
    }
    return amg_value_codes(s, M);
}

// Value codes of the coarse operators (pfem_valdict.hpp), after every numeric phase of a one-rank hierarchy: the scalar levels
// of at least 2^20 slots whose fused SpMVs would stream them (smaller levels cost their launches, not their bytes; node-block
// levels do not repeat their values: the beam's level 1 has 81 000 distinct ones among 3.2 M at 20x120x20).  First the levels
// that have a dictionary are encoded against it, one read of the verdicts; then those without one, or with a value it lacks,
// collect theirs -- a second read, in the first solve of a pattern only.  Config 3: level 1 (17.6 M slots, ~400 values).
constexpr int64_t kAmgVdMinSlots = 1 << 20;

// Column codes of the levels that take the value dictionary (one rank; AmgLevel::ccodes): do level l's fused products read them?
inline bool amg_level_col_codes(const Amg &M, const AmgLevel &L)
{
    return M.col_codes && !M.coupled && L.vd.ok && L.vcodes.p && L.cc_ok && L.ccodes.p && L.cdelta.p && L.cd_n > 0;
}
// Built once per hierarchy, at the first numeric phase that wants them (PFEM_AMG_COL_CODES not 0): the distinct  col - row  of the
// level collected (k_cc_collect; more than the cap -- 256, PFEM_AMG_COL_CODES_MAX=<n> lowers it -- refuses the level), sorted, every
// slot encoded, and every slot decoded again and compared with `cols` (k_cc_verify).  All on the stream; the verdict travels with the
// value codes' verdicts (read_states of amg_value_codes), so the phase waits for the device no more often than it did.
int amg_column_codes_enqueue(pfem_solver *s, Amg &M, int l)
{
    AmgLevel &L = *M.lev[static_cast<size_t>(l)];
    const size_t nl = M.lev.size();
    if (M.cc_states.n < nl) PFEM_TRY(M.cc_states.alloc(nl));
    if (!M.cc_hash.p) PFEM_TRY(M.cc_hash.alloc(kCcHash));
    int cap = kCcMax;
    if (const char *e = std::getenv("PFEM_AMG_COL_CODES_MAX")) cap = std::max(1, std::min(kCcMax, std::atoi(e)));
    const size_t words = static_cast<size_t>(std::max<int64_t>(cc_words(L.stored, L.n_slices), 64));
    PFEM_TRY(L.ccodes.alloc(words));
    PFEM_TRY(L.cdelta.alloc(kCcMax));
    const CcState init{0, 0, 0, cap};
    CcState *st = M.cc_states.p + l;
    PFEM_HIP(hipMemcpyAsync(st, &init, sizeof init, hipMemcpyHostToDevice, s->stream));
    const SellDev A = amg_sell(s, L);
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(1, (A.n_slices + 3) / 4), 4096));
    hipLaunchKernelGGL(k_cc_fill, dim3(kCcHash / kBlock), dim3(kBlock), 0, s->stream, M.cc_hash.p, kCcHash, kCcEmpty);
    hipLaunchKernelGGL(k_cc_collect, dim3(grid), dim3(kBlock), 0, s->stream, A, M.cc_hash.p, st);
    hipLaunchKernelGGL(k_cc_finish, dim3(1), dim3(kCcHash), 0, s->stream, static_cast<const int32_t *>(M.cc_hash.p), L.cdelta.p, st);
    hipLaunchKernelGGL(k_cc_encode, dim3(grid), dim3(kBlock), 0, s->stream, A, static_cast<const int32_t *>(L.cdelta.p), st, L.ccodes.p);
    hipLaunchKernelGGL(k_cc_verify, dim3(grid), dim3(kBlock), 0, s->stream, A, static_cast<const int32_t *>(L.cdelta.p),
                       static_cast<const uint32_t *>(L.ccodes.p), st);
    PFEM_TRY(check_kernel("k_cc_collect / k_cc_finish / k_cc_encode / k_cc_verify"));
    L.cc_pending = true;
    ++M.cc_builds;
    return PFEM_OK;
}
// ... after the read: no level runs a form that was not compared word for word
void amg_column_codes_verdict(Amg &M, int l, const CcState &v)
{
    AmgLevel &L = *M.lev[static_cast<size_t>(l)];
    L.cc_pending = false;
    if (v.fail || v.mismatch || v.count < 1 || v.count > kCcMax || v.count > v.cap) {
        L.cc_ok = false;
        L.cc_refused = true;              // (for this hierarchy)
        L.ccodes.release();
        L.cdelta.release();
        L.cd_n = 0;
    } else {
        L.cd_n = v.count;
        L.cc_ok = true;
    }
    if (vd_verbose())
        std::fprintf(stderr, "  column codes, level %d: %d distinct offsets among %lld slots%s\n", l, v.count, static_cast<long long>(L.stored),
                     L.cc_ok ? "" : (v.mismatch ? " -- the check failed, the level keeps its int32 columns" : " -- the level keeps its int32 columns"));
}

// Is level l (1 .. last - 1) a candidate for the value dictionary in this solve?  Known before the numeric phase enqueues anything.
// (a hierarchy across ranks, round 6: its distributed levels too -- k_amg_spmv_pack_vd; every rank has its own dictionaries
// and its own verdicts: the product is the same product either way, and no collective depends on which kernel ran)
inline bool amg_vd_candidate(const Amg &M, int l)
{
    const AmgLevel &L = *M.lev[static_cast<size_t>(l)];
    return valdict_enabled() && (M.coupled || (M.fused && M.cheb_degree == 2)) && !L.fine && L.bs == 1 && !L.gptr.p && L.stored >= kAmgVdMinSlots &&
           !L.vd.refused && (M.tail_from < 0 || l < M.tail_from);
}

int amg_value_codes(pfem_solver *s, Amg &M)
{
    const int nl = static_cast<int>(M.lev.size());
    std::vector<int> cand;
    for (int l = 1; l + 1 < nl; ++l) {
        if (amg_vd_candidate(M, l)) cand.push_back(l);
        else M.lev[static_cast<size_t>(l)]->vd.skip();
    }
    if (cand.empty()) return PFEM_OK;
    if (M.vd_states.n < static_cast<size_t>(nl)) PFEM_TRY(M.vd_states.alloc(static_cast<size_t>(nl)));
    std::vector<VdState> st(static_cast<size_t>(nl));
    // the same levels' column codes, when this hierarchy has none yet (their verdict rides on the first read below)
    std::vector<int> cc_wait;
    if (M.col_codes && !M.coupled && &M == s->amg.get() && !cg_multi(s))
        for (int l : cand) {
            AmgLevel &L = *M.lev[static_cast<size_t>(l)];
            if (L.cc_ok || L.cc_refused) continue;
            PFEM_TRY(amg_column_codes_enqueue(s, M, l));
            cc_wait.push_back(l);
        }
    std::vector<CcState> cst(cc_wait.empty() ? 0 : static_cast<size_t>(nl));
    auto encode = [&](AmgLevel &L, int l) -> int { return enqueue_vd_encode16(s->stream, L.vd, L.vals.p, L.stored, M.vd_states.p + l, L.vcodes.p); };
    auto read_states = [&]() -> int {
        PFEM_HIP(hipMemcpyAsync(st.data(), M.vd_states.p, sizeof(VdState) * static_cast<size_t>(nl), hipMemcpyDeviceToHost, s->stream));
        if (!cc_wait.empty())
            PFEM_HIP(hipMemcpyAsync(cst.data(), M.cc_states.p, sizeof(CcState) * static_cast<size_t>(nl), hipMemcpyDeviceToHost, s->stream));
        PFEM_HIP(hipStreamSynchronize(s->stream));
        for (int l : cc_wait) amg_column_codes_verdict(M, l, cst[static_cast<size_t>(l)]);
        cc_wait.clear();
        return PFEM_OK;
    };
    std::vector<int> build;
    bool any_old = false;
    for (int l : cand) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        if (L.vcodes.n < static_cast<size_t>(L.stored)) PFEM_TRY(L.vcodes.alloc(static_cast<size_t>(L.stored)));
        PFEM_TRY(L.vd.reserve(false));
        if (L.vd.have && L.vd_direct) {
            any_old = true;               // (the Galerkin product wrote the codes itself: only its verdict is read)
        } else if (L.vd.have) {
            PFEM_TRY(L.vd.enqueue_against_standing(s->stream, M.vd_states.p + l));
            PFEM_TRY(encode(L, l));
            any_old = true;
        } else {
            build.push_back(l);
        }
        L.vd_direct = false;
    }
    if (any_old) {
        PFEM_TRY(read_states());
        for (int l : cand) {
            AmgLevel &L = *M.lev[static_cast<size_t>(l)];
            if (!L.vd.have) continue;
            if (st[static_cast<size_t>(l)].miss) build.push_back(l);
            else L.vd.accept(st[static_cast<size_t>(l)], true);          // ({n, 0, 0, 0}: the dictionary that stood)
        }
    }
    if (build.empty()) return PFEM_OK;
    for (int l : build) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        const unsigned grid = static_cast<unsigned>(std::min<int64_t>((L.stored + kBlock - 1) / kBlock, 4096));
        // with the dictionary's hash table: from the next solve on the Galerkin product looks the codes up itself (k_lat_galerkin)
        PFEM_TRY(L.vd.reserve(true));
        PFEM_TRY(L.vd.enqueue_build(s->stream, L.vals.p, L.stored, grid, M.vd_states.p + l, true));
        PFEM_TRY(encode(L, l));
    }
    PFEM_TRY(read_states());
    for (int l : build) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        const VdState &v = st[static_cast<size_t>(l)];
        const bool taken = L.vd.accept(v, true);          // (or refused for this hierarchy)
        if (vd_verbose())
            std::fprintf(stderr, "  value dictionary, level %d: %d distinct values among %lld slots%s\n", l, v.count, static_cast<long long>(L.stored),
                         taken ? "" : " -- the level keeps its fp64 values");
    }
    return PFEM_OK;
}

// May this numeric phase form level 1 from the SpMV's value codes (k_lat_galerkin_codes)?  One rank, a scalar brick level 0 without
// hubs whose SpMV streams the 4-row relative-group form's 16-bit codes, and those codes hold THIS assembly's values against the
// dictionary in place: vd.ok && vd_current, the very condition under which the CG's products read them (refresh_group_vals ran
// before this phase: the assembly kernel's verdict has been read and was clean, or k_vd_encode has encoded the fp64 copy).  A step
// whose assembly met a value the dictionary lacked keeps the fp64 kernel (vd_miss_step), like every other case.
// PFEM_AMG_GALERKIN_CODES=0 (read at every phase): k_lat_galerkin as before.  The form's lattice codes are built at the first yes.
int amg_level0_codes(pfem_solver *s, Amg &M, AmgLevel &L, bool *yes)
{
    *yes = false;
    const char *e = std::getenv("PFEM_AMG_GALERKIN_CODES");
    if (e && std::atoi(e) == 0) return PFEM_OK;
    if (&M != s->amg.get() || M.coupled || M.rbm || cg_multi(s) || !L.fine || L.rbm || L.bs != 1 || !L.code_of.p || !L.code_mask.p || amg_galerkin_by_entry() ||
        s->n_hubs != 0 || L.stored != s->stored || L.glat_refused)
        return PFEM_OK;
    const SpmvForm f = spmv_form(s);
    if (!valdict_enabled() || f.layout != SpmvLayout::Rel4 || !f.codes || !s->vd.have || s->vd_miss_step ||
        s->vd.n < 1 || s->vd.n > kVdMax || !s->d_vcodes.p || !s->vd.dict.p || !s->d_relk.p || !s->d_rslice_off.p || s->r_stored < 1 ||
        s->d_vcodes.n < static_cast<size_t>(s->r_stored))
        return PFEM_OK;
    if (!L.glat.p || L.glat_for != s->r_stored) {
        PFEM_TRY(L.glat.alloc(static_cast<size_t>(s->r_stored)));
        L.glat_for = -1;
        PFEM_HIP(hipMemsetAsync(L.glat.p, 0xff, sizeof(uint32_t) * static_cast<size_t>(s->r_stored), s->stream));
        PFEM_HIP(hipMemsetAsync(s->d_err.p, 0, sizeof(int), s->stream));
        hipLaunchKernelGGL(k_lat_group_codes, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, amg_sell(s, L), static_cast<const uint8_t *>(L.code_of.p),
                           static_cast<const uint8_t *>(s->d_relk.p), static_cast<const int64_t *>(s->d_rslice_off.p), reinterpret_cast<uint8_t *>(L.glat.p),
                           s->d_err.p);
        PFEM_TRY(check_kernel("k_lat_group_codes"));
        int bad = 0;
        PFEM_TRY(fetch_err(s, &bad));
        PFEM_HIP(hipMemsetAsync(s->d_err.p, 0, sizeof(int), s->stream));
        if (bad) { L.glat.release(); L.glat_refused = true; return PFEM_OK; }
        L.glat_for = s->r_stored;
    }
    *yes = true;
    return PFEM_OK;
}

int amg_numeric(pfem_solver *s, Amg &M, bool overlap)
{
    M.galerkin_from_codes = false;
    if (M.coupled) return amg_numeric_coupled(s, M, overlap);
    const bool fresh = M.galerkin_fresh;
    M.galerkin_fresh = false;
    // A coarse level's bound without launches of its own (PFEM_AMG_FUSED not 0, plain transfers): the Galerkin product that writes the
    // level's ratios leaves their maximum in the level's lam itself (LatGalExtra::bound).  The word has to be zero when that product
    // starts, and it is zeroed inside this chain: level 1's by level 0's k_amg_max, which therefore runs BEFORE the first product
    // (it reads what the assembly left, not what the product writes), level l + 2's by the product that forms level l + 1.
    // `zeroed` = the level whose lam some kernel enqueued above has zeroed (0: none).
    const bool own_bounds = M.fused && !M.rbm && !fresh && M.lev.size() > 1;
    size_t zeroed = 0;
    M.bounds_by_products = 0;
    // The tail of this chain on a stream of its own (one rank, the conditions of own_bounds; PFEM_AMG_SIDE_STREAM=0: off).  The
    // products from a few thousand rows down and the dense inverse are latency chains of a few workgroups each; the first cycle's
    // upper levels, which stream the large matrices, need nothing of what they write.  side_from = the first level no kernel form of
    // which is decided by a verdict (amg_value_codes: no dictionary, no column codes from there on), at least 2 -- level 1 is what the
    // cycle wants first, and the product that forms it fills the chip.  From the product that forms level side_from on, everything
    // here goes to M.side_stream, forked off the solver's stream behind the product that formed level side_from - 1: the chain in
    // which each product zeroes the next level's lam stays on one stream from there.  amg_apply waits for ev_side1 in front of the
    // first kernel that touches such a level; run_pcg_amg makes sure no return leaves the chain unjoined.
    M.side_used = false;
    M.side_first = 0;
    size_t side_from = 0;
    if (own_bounds && M.side_on && &M == s->amg.get() && !cg_multi(s)) {
        size_t k = 2;
        for (size_t l = 1; l + 1 < M.lev.size(); ++l)
            if (amg_vd_candidate(M, static_cast<int>(l))) k = l + 1;
        if (k < M.lev.size()) side_from = k;
    }
    // where the kernels that write level l go
    auto stream_of = [&](size_t l) { return M.side_used && l >= side_from ? M.side_stream : s->stream; };
    auto fork = [&]() -> int {
        if (!M.side_stream) PFEM_HIP(hipStreamCreateWithFlags(&M.side_stream, hipStreamNonBlocking));
        if (!M.ev_fork) PFEM_HIP(hipEventCreateWithFlags(&M.ev_fork, hipEventDisableTiming));
        if (!M.ev_side0) PFEM_HIP(hipEventCreate(&M.ev_side0));
        if (!M.ev_side1) PFEM_HIP(hipEventCreate(&M.ev_side1));
        PFEM_HIP(hipEventRecord(M.ev_fork, s->stream));
        PFEM_HIP(hipStreamWaitEvent(M.side_stream, M.ev_fork, 0));
        PFEM_HIP(hipEventRecord(M.ev_side0, M.side_stream));
        M.side_used = M.side_pending = true;
        M.side_first = static_cast<int>(side_from);
        return PFEM_OK;
    };
    // level l's bound from its stored matrix, or from what the assembly (level 0) / the Galerkin product left in L.t
    auto level_bound = [&](size_t l, double *zero) -> int {
        AmgLevel &L = *M.lev[l];
        const hipStream_t st = stream_of(l);
        const SellDev A = amg_sell(s, L);
        const unsigned g = grid_for(A.n_slices * 64);
        if (!L.fine && L.bound_fresh && !fresh) {
            // the product that formed this level's values left its inverse diagonal in L.dinv and the rows' ratios in L.t (k_lat_galerkin)
            L.bound_fresh = false;
            if (L.bound_done) { ++M.bounds_by_products; return PFEM_OK; }          // ... and their maximum in L.lam
            if (L.n > 65536) {
                const unsigned gm = std::min<unsigned>(g, 512u);
                hipLaunchKernelGGL(k_amg_max_rows, dim3(gm), dim3(kBlock), 0, st, static_cast<const double *>(L.t.p), L.n, L.part_max.p);
                hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, st, static_cast<const double *>(L.part_max.p), static_cast<int64_t>(gm), L.lam.p, zero);
            } else {
                hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, st, static_cast<const double *>(L.t.p), L.n, L.lam.p, zero);
            }
            return PFEM_OK;
        }
        if (L.fine && s->asm_bound_fresh && &M == s->amg.get()) {
            // the assembly kernel left the inverse diagonal in L.dinv and every row's sum |a_ij| / a_ii in L.t while the rows were in
            // LDS (k_gather_poisson_tet4): the maximum of the ratios is all that is left to do -- no pass over the assembled matrix
            const unsigned gm = std::min<unsigned>(g, 2048u);
            hipLaunchKernelGGL(k_amg_max_rows, dim3(gm), dim3(kBlock), 0, st, static_cast<const double *>(L.t.p), L.n, L.part_max.p);
            hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, st, static_cast<const double *>(L.part_max.p), static_cast<int64_t>(gm), L.lam.p, zero);
            s->asm_bound_fresh = false;
        } else {
            hipLaunchKernelGGL(k_amg_diag_bound, dim3(g), dim3(kBlock), 0, st, A, static_cast<int32_t>(L.n), L.dinv.p, L.part_max.p);
            hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, st, static_cast<const double *>(L.part_max.p), static_cast<int64_t>(g), L.lam.p, zero);
        }
        if (M.rbm) {            // the bound on the symmetrically scaled operator; the smaller of the two is taken (k_rbm_bound_sym)
            if (!M.lam2.p) PFEM_TRY(M.lam2.alloc(1));
            hipLaunchKernelGGL(k_rbm_bound_sym, dim3(g), dim3(kBlock), 0, st, A, static_cast<int32_t>(L.n), static_cast<const double *>(L.dinv.p),
                               static_cast<double *>(nullptr), L.part_max.p);
            hipLaunchKernelGGL(k_amg_max, dim3(1), dim3(1024), 0, st, static_cast<const double *>(L.part_max.p), static_cast<int64_t>(g), M.lam2.p);
            hipLaunchKernelGGL(k_rbm_min2, dim3(1), dim3(64), 0, st, static_cast<const double *>(M.lam2.p), L.lam.p);
        }
        return PFEM_OK;
    };
    for (size_t l = 0; l < M.lev.size(); ++l) {
        AmgLevel &L = *M.lev[l];
        const SellDev A = amg_sell(s, L);
        const bool bound_first = own_bounds && l == 0;
        if (bound_first) {
            PFEM_TRY(level_bound(0, M.lev[1]->lam.p));
            zeroed = 1;
        }
        if (l + 1 < M.lev.size() && !fresh) {
            AmgLevel &C = *M.lev[l + 1];
            if (L.rbm) amg_rbm_galerkin(s, L, C, A);
            else {
                bool from_codes = false;
                if (l == 0) PFEM_TRY(amg_level0_codes(s, M, L, &from_codes));
                const bool mine = own_bounds && zeroed == l + 1;
                double *next = mine && l + 2 < M.lev.size() ? M.lev[l + 2]->lam.p : nullptr;
                if (side_from && l + 1 == side_from) PFEM_TRY(fork());
                if (amg_galerkin_on(stream_of(l + 1), s, L, C, A, !M.rbm && !M.coupled, M.vd_states.p ? M.vd_states.p + (l + 1) : nullptr, from_codes, mine ? C.lam.p : nullptr, next) && next)
                    zeroed = l + 2;
                if (from_codes) M.galerkin_from_codes = true;
                if (l == 0 && vd_verbose())
                    std::fprintf(stderr, "  gamg numeric: level 1 summed from %s\n", from_codes ? "the SpMV's value codes" : "the fp64 row form");
            }
        }
        if (!bound_first) PFEM_TRY(level_bound(l, nullptr));
    }
    PFEM_TRY(check_kernel("gamg numeric"));
    if (M.dense) {
        AmgLevel &L = *M.lev.back();
        hipLaunchKernelGGL(k_amg_dense_inverse, dim3(1), dim3(1024), static_cast<size_t>(L.n * L.n) * sizeof(double), stream_of(M.lev.size() - 1),
                           amg_sell(s, L), M.dense_inv.p);
        PFEM_TRY(check_kernel("k_amg_dense_inverse"));
    }
    if (M.side_used) PFEM_HIP(hipEventRecord(M.ev_side1, M.side_stream));          // the chain's end: what the first cycle waits for
    return amg_value_codes(s, M);
}

// restriction with the rigid-body transfer: a thread per coarse node, or -- aggregates of 16 nodes and more on average (level 0 in
// bricks of 3 and 4 to the edge) -- kRbmWide lanes per coarse node (k_rbm_restrict_wide); decided from the level's sizes alone
inline void amg_rbm_restrict_launch(pfem_solver *s, const AmgLevel &L, AmgLevel &C, int64_t nc_nodes, int64_t nn, const double *b, const double *t, double ratio,
                                    double *dd_c, double *x_c, const CgCtl *ctl, int64_t n_own_nodes)
{
    static const bool wide_on = [] { const char *e = std::getenv("PFEM_RBM_RESTRICT_WIDE"); return e ? std::atoi(e) != 0 : true; }();
    const bool wide = wide_on && nc_nodes > 0 && nn >= 16 * nc_nodes;
    if (wide) {
        PFEM_RBM_DISPATCH(L.bs, L.dim, hipLaunchKernelGGL((k_rbm_restrict_wide<FB, DIM>), dim3(grid_for(nc_nodes * kRbmWide)), dim3(kBlock), 0, s->stream, nc_nodes,
            static_cast<const int32_t *>(L.mem_ptr.p), static_cast<const int32_t *>(L.mem_idx.p), static_cast<const double *>(L.roff.p), nn,
            b, t, C.b.p, static_cast<const double *>(C.dinv.p), static_cast<const double *>(C.lam.p), ratio, dd_c, x_c, ctl, n_own_nodes));
    } else {
        PFEM_RBM_DISPATCH(L.bs, L.dim, hipLaunchKernelGGL((k_rbm_restrict<FB, DIM>), dim3(grid_for(nc_nodes)), dim3(kBlock), 0, s->stream, nc_nodes,
            static_cast<const int32_t *>(L.mem_ptr.p), static_cast<const int32_t *>(L.mem_idx.p), static_cast<const double *>(L.roff.p), nn,
            b, t, C.b.p, static_cast<const double *>(C.dinv.p), static_cast<const double *>(C.lam.p), ratio, dd_c, x_c, ctl, n_own_nodes));
    }
}

// Chebyshev smoothing of degree `deg` on level L: x <- x + p(D^-1 A) D^-1 (b - A x); zero_guess: x = 0 on entry (not read)
// (coupled hierarchy: over all local rows, and every product is summed over the holders before it is used)
int amg_smooth(pfem_solver *s, const Amg &M, AmgLevel &L, const double *b, bool zero_guess, int deg, const CgCtl *ctl, bool first_done = false,
               bool overlap = false)
{
    const int64_t nv = amg_rows(M, L);
    const unsigned gv = vec_grid(nv);
    const double *t0 = nullptr;
    // one hierarchy across the ranks, fused form: the product's shared rows go into the send buffer as the SpMV's epilogue
    // (coarse levels; the assembled matrix keeps its SpMV forms and a pack kernel), the exchange moves them, and the vector
    // step that uses the product sums the holders' shares on the fly -- 3 launches per product instead of 5, same bits
    const PlanRef P = M.coupled ? amg_plan(s, L) : PlanRef{};
    const bool cf = M.coupled && M.coupled_fused && P.row_sh != nullptr;
    const ShareSum S = cf ? ShareSum{P.row_sh, P.sh_ptr, P.sh_src, s->d_recv.p} : ShareSum{nullptr, nullptr, nullptr, nullptr};
    auto product = [&](const double *x) -> int {          // L.t = this rank's share of A x, on its way to the holders
        if (!cf) {
            amg_spmv(s, M, L, x, L.t.p);
            if (M.coupled) PFEM_TRY(exchange_sum(s, P, L.t.p, overlap, ctl));
            return PFEM_OK;
        }
        if (L.fine) {
            amg_spmv(s, M, L, x, L.t.p);
            if (P.n_send > 0)
                hipLaunchKernelGGL(k_pack_send, dim3(grid_for(P.n_send)), dim3(kBlock), 0, s->stream, static_cast<const double *>(L.t.p), P.send_lidx, P.n_send,
                                   s->d_send.p, ctl);
        } else {
            const SellDev A = amg_sell(s, L, nv);
            if (L.vd.ok && L.vcodes.p)
                hipLaunchKernelGGL(k_amg_spmv_pack_vd, dim3(spmv_grid(A.n_slices)), dim3(kBlock), sizeof(double) * static_cast<size_t>(L.vd.n), s->stream, A,
                                   static_cast<const uint16_t *>(L.vcodes.p), static_cast<const double *>(L.vd.dict.p), L.vd.n, x, L.t.p, S, s->d_send.p, ctl);
            else
            hipLaunchKernelGGL(k_amg_spmv_pack, dim3(spmv_grid(A.n_slices)), dim3(kBlock), 0, s->stream, A, x, L.t.p, S, s->d_send.p, ctl);
        }
        return exchange_only(s, P, overlap);
    };
    if (!zero_guess) {
        PFEM_TRY(product(L.x));
        t0 = L.t.p;
    }
    // with a zero guess the residual before step 1 is b itself: no copy is made
    double *r_store = (deg > 1 && !zero_guess) ? L.r.p : nullptr;
    if (!first_done)      // (step 0 with a zero guess may have ridden on the CG's update kernel)
        hipLaunchKernelGGL(k_amg_cheb_first, dim3(gv), dim3(kBlock), 0, s->stream, nv, b, t0, static_cast<const double *>(L.dinv.p),
                           static_cast<const double *>(L.lam.p), M.eig_ratio, r_store, deg > 1 ? L.dd : static_cast<double *>(nullptr), L.x, ctl, S);
    const double *r_in = zero_guess ? b : L.r.p;
    for (int k = 1; k < deg; ++k) {
        PFEM_TRY(product(L.dd));
        const bool more = k + 1 < deg;
        hipLaunchKernelGGL(k_amg_cheb_next, dim3(gv), dim3(kBlock), 0, s->stream, nv, k, r_in, static_cast<const double *>(L.t.p),
                           static_cast<const double *>(L.dinv.p), static_cast<const double *>(L.lam.p), M.eig_ratio, more ? L.r.p : nullptr,
                           static_cast<const double *>(L.dd), more ? L.dd : nullptr, L.x, ctl, S);
        r_in = L.r.p;
    }
    return PFEM_OK;
}

// z = M^-1 r with ONE hierarchy across the ranks.  Every vector of the cycle is consistent (a dof has the same value on
// all its holders); a level's matrix holds this rank's share of the entries, so a product is the sum of the holders'
// shares -- one neighbour exchange behind every SpMV whose result is used as such.  The residual that goes down is not:
// its restriction is linear, so each rank restricts  [owned part of b] - [its own share of A x]  and the COARSE vector is
// summed over the holders instead -- one exchange on the smaller level where two on the larger would be needed.
// Level by level with plain kernels (no fused epilogues, no single-workgroup tail: both end at a rank's border).
// what amg_apply leaves of level 0's last post-smoothing step to its caller (fine degree 1): nothing; the step itself, t = A x
// being in L0.t (k_pc_post_dots); or the product runs with the step and the CG's sums as its epilogue (Level0Ep: z in L0.t)
enum { kLast0Smooth = 0, kLast0Product = 1, kLast0Epilogue = 2 };
double *amg_apply(pfem_solver *s, Amg &M, const double *r, const CgCtl *ctl, bool first0_done = false, int last0 = kLast0Smooth, int join_level = 0,
                  hipEvent_t join_ev = nullptr);
double *amg_apply_coupled(pfem_solver *s, Amg &M, const double *r, const CgCtl *ctl, bool overlap)
{
    const int nl = static_cast<int>(M.lev.size());
    // what one cycle costs in communication (for the bench line): SpMV exchanges of the smoother + one per restriction
    {
        int ex = 0, ar = 0;
        auto smooth_ex = [](int deg, bool zero_guess) { return (zero_guess ? 0 : 1) + (deg - 1); };
        for (int l = 0; l < nl; ++l) {
            const int deg = (l == 0 && M.fine_degree > 0) ? M.fine_degree : M.cheb_degree;
            if (l == nl - 1) {
                if (M.rep || M.dense) ar += 1;
                else ex += smooth_ex(nl == 1 ? M.cheb_degree : M.coarsest_sweeps, true);
            } else {
                ex += smooth_ex(deg, true) + 1 + smooth_ex(deg, false);
            }
        }
        M.cycle_exchanges = ex;
        M.cycle_allreduces = ar;
    }
    auto deg_of = [&](int l) { return (l == 0 && M.fine_degree > 0) ? M.fine_degree : M.cheb_degree; };
    for (int l = 0; l < nl; ++l) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        const double *b = l == 0 ? r : L.b.p;
        s->xprof_level = l;
        if (l == nl - 1) {
            if (M.rep) {
                // the level assembled on every rank: its right-hand side gathered by one all-reduce, the rest of the cycle
                // without any exchange (identical on all ranks), the correction picked up by global number
                const int64_t ng = M.n_last_global;
                double *bg = M.bx_glob.p;
                hipLaunchKernelGGL(k_amg_zero, dim3(grid_for(ng)), dim3(kBlock), 0, s->stream, ng, bg, ctl);
                hipLaunchKernelGGL(k_amg_scatter_gid, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, L.n, b, static_cast<const int32_t *>(L.gid.p), bg, ctl);
                if (xprof_begin(s, 1, ng, s->stream) != PFEM_OK || s->comm->allreduce(bg, ng, s->stream) != PFEM_OK || xprof_end(s, s->stream) != PFEM_OK) return nullptr;
                const double *xg = amg_apply(s, *M.rep, bg, ctl);
                if (!xg) return nullptr;
                hipLaunchKernelGGL(k_amg_gather_gid, dim3(grid_for(L.n_loc)), dim3(kBlock), 0, s->stream, L.n_loc, xg,
                                   static_cast<const int32_t *>(L.gid.p), L.x, ctl);
            } else if (M.dense) {
                const int ng = static_cast<int>(M.n_last_global);
                double *bg = M.bx_glob.p, *xg = M.bx_glob.p + kAmgDense;
                hipLaunchKernelGGL(k_amg_zero, dim3(1), dim3(kBlock), 0, s->stream, static_cast<int64_t>(ng), bg, ctl);
                hipLaunchKernelGGL(k_amg_scatter_gid, dim3(grid_for(L.n)), dim3(kBlock), 0, s->stream, L.n, b, static_cast<const int32_t *>(L.gid.p), bg, ctl);
                if (xprof_begin(s, 1, ng, s->stream) != PFEM_OK || s->comm->allreduce(bg, ng, s->stream) != PFEM_OK || xprof_end(s, s->stream) != PFEM_OK) return nullptr;
                hipLaunchKernelGGL(k_amg_dense_apply, dim3(1), dim3(kAmgDense), 0, s->stream, ng, static_cast<const double *>(M.dense_inv.p),
                                   static_cast<const double *>(bg), xg, ctl);
                hipLaunchKernelGGL(k_amg_gather_gid, dim3(grid_for(L.n_loc)), dim3(kBlock), 0, s->stream, L.n_loc, static_cast<const double *>(xg),
                                   static_cast<const int32_t *>(L.gid.p), L.x, ctl);
            } else if (amg_smooth(s, M, L, b, true, nl == 1 ? M.cheb_degree : M.coarsest_sweeps, ctl, false, overlap) != PFEM_OK) {
                return nullptr;
            }
            break;
        }
        AmgLevel &C = *M.lev[static_cast<size_t>(l) + 1];
        if (amg_smooth(s, M, L, b, true, deg_of(l), ctl, false, overlap) != PFEM_OK) return nullptr;
        amg_spmv(s, M, L, L.x, L.t.p);                   // this rank's share, not summed
        if (L.rbm)
            amg_rbm_restrict_launch(s, L, C, C.n_loc / C.bs, L.n_loc / L.bs, b, static_cast<const double *>(L.t.p), M.eig_ratio, nullptr, nullptr, ctl, L.n_nodes);
        {
            const PlanRef PC = amg_plan(s, C);
            const bool cf = M.coupled_fused && PC.row_sh != nullptr && !L.rbm;
            const ShareSum SC = cf ? ShareSum{PC.row_sh, PC.sh_ptr, PC.sh_src, s->d_recv.p} : ShareSum{nullptr, nullptr, nullptr, nullptr};
            if (!L.rbm)
            hipLaunchKernelGGL(k_amg_restrict, dim3(grid_for(C.n_loc)), dim3(kBlock), 0, s->stream, C.n_loc, static_cast<const int32_t *>(L.mem_ptr.p),
                           static_cast<const int32_t *>(L.mem_idx.p), b, static_cast<const double *>(L.t.p), C.b.p, static_cast<const double *>(C.dinv.p),
                           static_cast<const double *>(C.lam.p), M.eig_ratio, static_cast<double *>(nullptr), static_cast<double *>(nullptr), ctl,
                           static_cast<int32_t>(L.n), SC, s->d_send.p);
            if (cf) {       // the restriction packed the shared coarse dofs itself; the sum is written back: three kernels read the right-hand side
                if (exchange_only(s, PC, overlap) != PFEM_OK) return nullptr;
                if (PC.n_sh > 0)
                    hipLaunchKernelGGL(k_unpack_sum, dim3(grid_for(PC.n_sh)), dim3(kBlock), 0, s->stream, C.b.p, PC.sh_lidx, PC.sh_ptr, PC.sh_src, PC.n_sh,
                                       static_cast<const double *>(s->d_recv.p), ctl);
            } else if (exchange_sum(s, PC, C.b.p, overlap, ctl) != PFEM_OK) {
                return nullptr;
            }
        }
    }
    for (int l = nl - 2; l >= 0; --l) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        AmgLevel &C = *M.lev[static_cast<size_t>(l) + 1];
        const double *b = l == 0 ? r : L.b.p;
        s->xprof_level = l;
        if (L.rbm) {
            PFEM_RBM_DISPATCH(L.bs, L.dim, hipLaunchKernelGGL((k_rbm_prolong<FB, DIM>), dim3(vec_grid(L.n_loc / L.bs)), dim3(kBlock), 0, s->stream, L.n_loc / L.bs,
                static_cast<const int32_t *>(L.node_agg.p), static_cast<const double *>(L.roff.p), L.n_loc / L.bs, static_cast<const double *>(C.x),
                M.coarse_scale, L.x, ctl));
        } else
        hipLaunchKernelGGL(k_amg_prolong, dim3(vec_grid(L.n_loc)), dim3(kBlock), 0, s->stream, L.n_loc, static_cast<const int32_t *>(L.agg.p),
                           static_cast<const double *>(C.x), M.coarse_scale, L.x, ctl);
        if (amg_smooth(s, M, L, b, false, deg_of(l), ctl, false, overlap) != PFEM_OK) return nullptr;
    }
    return M.lev[0]->x;
}

// z = M^-1 r: one V(1,1) cycle -- or W(1,1): M.cycle_gamma --; returns the vector that holds z (level 0's x; its t after kLast0Epilogue).
// Three ways through a level, all the same arithmetic (PFEM_AMG_FUSED=0 takes the first everywhere; tested bit for bit):
//   * level 0 and any level whose Chebyshev degree is not 2: SpMV launches + vector kernels (amg_smooth).  Level 0's two ends
//     ride on the CG's own kernels during the iterations: step 0 of the pre-smoothing on k_pc_update, and -- fine degree 1 --
//     the post-smoothing step either on the dots kernel (k_pc_post_dots, t = A x stored) or, on one rank with a 4-row
//     relative-group SpMV form, on the product itself: z and the CG's (r,z), (z,z) are its epilogue (Level0Ep), t is never stored;
//   * levels 1 .. tail_from-1: the SpMV with the vector step as its epilogue (k_amg_spmv_ep), step 0 of the pre-smoothing
//     done by the restriction kernel of the level above: 6 launches per level instead of 10;
//   * levels tail_from .. last (at most kAmgTailRows rows each): one workgroup walks them all in one launch (k_amg_tail).
// join_ev (the first cycle behind a numeric phase that forked its side chain, never a captured cycle): the stream waits for it
// once, in front of the first kernel that reads or writes anything of a level >= join_level.
double *amg_apply(pfem_solver *s, Amg &M, const double *r, const CgCtl *ctl, bool first0_done, int last0, int join_level, hipEvent_t join_ev)
{
    const int nl = static_cast<int>(M.lev.size());
    bool joined = join_ev == nullptr;
    // called in front of every kernel that touches level l (and, the tail: the last level)
    auto touches = [&](int l) {
        if (joined || l < join_level) return;
        joined = true;
        if (hipStreamWaitEvent(s->stream, join_ev, 0) == hipSuccess) M.side_pending = false;
    };
    // several ranks: the ghost part of z holds the owners' values after the exchange of the previous cycle; as an SpMV
    // input of THIS rank's block it has to be zero again
    if (M.lev[0]->fine && s->n_ghost > 0) (void)hipMemsetAsync(M.lev[0]->x + s->n_owned, 0, sizeof(double) * static_cast<size_t>(s->n_ghost), s->stream);
    const bool fuse = M.fused && M.cheb_degree == 2;
    const int tail = (M.fused && M.tail_from > 0) ? M.tail_from : nl;         // levels [tail, nl) in one launch
    auto deg_of = [&](int l) { return (l == 0 && M.fine_degree > 0) ? M.fine_degree : M.cheb_degree; };
    auto fused_level = [&](int l) { return fuse && l >= 1 && l < tail && l < nl - 1; };
    auto ep = [&](int mode, AmgLevel &L, const double *xin, const double *r_in, int step, int add_dd0, double *r_out, double *dd_out, double *x) {
        const SellDev A = amg_sell(s, L);
        const dim3 grid(spmv_grid(A.n_slices)), block(kBlock);
        const double *dinv = L.dinv.p, *lam = L.lam.p;
        const hipStream_t st = s->stream;
        with_ep_mode(mode, [&](auto mode_c) {
            constexpr int MODE = decltype(mode_c)::value;
            if (L.gptr.p && (L.bs == 6 || L.bs == 3)) {          // a level below a rigid-body transfer: node-block form of the same product
                const int64_t *gp = L.gptr.p;
                const int32_t *gc = L.gcol.p;
                if (L.bs == 6) hipLaunchKernelGGL((k_rbm_spmv_ep<MODE, 6>), grid, block, 0, st, A, gp, gc, xin, r_in, dinv, lam, M.eig_ratio, step, add_dd0, r_out, dd_out, x, ctl);
                else hipLaunchKernelGGL((k_rbm_spmv_ep<MODE, 3>), grid, block, 0, st, A, gp, gc, xin, r_in, dinv, lam, M.eig_ratio, step, add_dd0, r_out, dd_out, x, ctl);
            } else if (L.vd.ok && L.vcodes.p) {          // the level's values as dictionary codes (amg_value_codes)
                const uint16_t *q = L.vcodes.p;
                const double *d = L.vd.dict.p;
                const size_t lds = sizeof(double) * static_cast<size_t>(L.vd.n);
                if (amg_level_col_codes(M, L)) {          // ... and its columns as one-byte codes (amg_column_codes_enqueue): 1 + 2 B a slot
                    const uint32_t *cw = L.ccodes.p;
                    const int32_t *cdl = L.cdelta.p;
                    const size_t lds_cc = lds + sizeof(int32_t) * static_cast<size_t>(L.cd_n);
                    hipLaunchKernelGGL((k_amg_spmv_ep_vd<MODE, true>), grid, block, lds_cc, st, A, q, d, L.vd.n, xin, r_in, dinv, lam, M.eig_ratio, step, add_dd0, r_out, dd_out, x, ctl, cw, cdl, L.cd_n);
                } else {
                    hipLaunchKernelGGL((k_amg_spmv_ep_vd<MODE, false>), grid, block, lds, st, A, q, d, L.vd.n, xin, r_in, dinv, lam, M.eig_ratio, step, add_dd0, r_out, dd_out, x, ctl, nullptr, nullptr, 0);
                }
            } else {
                hipLaunchKernelGGL(k_amg_spmv_ep<MODE>, grid, block, 0, st, A, xin, r_in, dinv, lam, M.eig_ratio, step, add_dd0, r_out, dd_out, x, ctl);
            }
        });
    };
    // the levels [tail, nl) in one launch
    auto run_tail = [&]() {
        AmgTail T{};
        T.nlev = nl - tail;
        T.deg = M.cheb_degree;
        T.coarsest_deg = M.coarsest_sweeps;
        T.dense_n = M.dense ? static_cast<int>(M.lev.back()->n) : 0;
        T.dense_inv = M.dense_inv.p;
        T.ratio = M.eig_ratio;
        T.scale = M.coarse_scale;
        amg_tail_shape(M, tail, T);
        for (int q = 0; q < T.nlev; ++q) {
            AmgLevel &L = *M.lev[static_cast<size_t>(tail + q)];
            AmgTailLevel &t = T.lev[q];
            t.A = amg_sell(s, L);
            t.dinv = L.dinv.p; t.lam = L.lam.p;
            t.x = L.x; t.dd = L.dd; t.t = L.t.p; t.r = L.r.p; t.b = L.b.p;
            t.agg = L.agg.p; t.mem_ptr = L.mem_ptr.p; t.mem_idx = L.mem_idx.p;
            t.n = L.n; t.nc = L.nc; t.stored = L.stored;
            t.rbm_dim = L.rbm ? L.dim : 0; t.fb = L.bs; t.nn = L.n_nodes; t.node_agg = L.node_agg.p; t.roff = L.roff.p;
        }
        // the levels' vectors in LDS (6 a level; config 3: 343 + 64 rows = 19.5 KB) with the plain transfers' index lists (3.4 KB) and,
        // beside them, the first level's matrix when all of it fits 156 KB (config 3: 10 368 slots = 124 KB)
        const TailLds W = tail_lds_bytes(T);
        const size_t lds = W.vec_b + W.mat_b;
        const bool use_lds = W.vecs_b <= 65536 && (W.vec_b <= 65536 || W.vec_b <= M.tail_vec_allowed || lds <= M.tail_lds_allowed);
        const bool mat_ok = use_lds && W.mat_b > 0 && lds <= kAmgTailLdsMax && (lds <= 65536 || lds <= M.tail_lds_allowed);
        const bool vec_ok = use_lds && (W.vec_b <= 65536 || W.vec_b <= M.tail_vec_allowed);
        M.tail_build = mat_ok ? 3 : vec_ok ? 2 : 1;          // (reported by pfem_solver_amg_tail_from)
        if (mat_ok) hipLaunchKernelGGL((k_amg_tail<true, true>), dim3(1), dim3(1024), lds, s->stream, T, ctl, T.lev[0].stored);
        else if (vec_ok) hipLaunchKernelGGL((k_amg_tail<true, false>), dim3(1), dim3(1024), W.vec_b, s->stream, T, ctl, static_cast<int64_t>(0));
        else hipLaunchKernelGGL((k_amg_tail<false, false>), dim3(1), dim3(1024), 0, s->stream, T, ctl, static_cast<int64_t>(0));
    };
    // one visit of level l: its problem  A_l x = b_l  (b_0 = r) answered in L.x -- pre-smoothing, the coarse problem (twice in a
    // W-cycle: the second time on what the first left), correction, post-smoothing
    std::function<void(int)> visit = [&](int l) {
        AmgLevel &L = *M.lev[static_cast<size_t>(l)];
        const double *b = l == 0 ? r : L.b.p;
        if (l == tail) { touches(nl - 1); run_tail(); return; }
        touches(l);
        if (l == nl - 1) {                      // the last level, outside a tail
            if (M.dense) {
                hipLaunchKernelGGL(k_amg_dense_apply, dim3(1), dim3(kAmgDense), 0, s->stream, static_cast<int>(L.n),
                                   static_cast<const double *>(M.dense_inv.p), b, L.x, ctl);
            } else {
                (void)amg_smooth(s, M, L, b, true, nl == 1 ? M.cheb_degree : M.coarsest_sweeps, ctl);
            }
            return;
        }
        // ---- down
        AmgLevel &C = *M.lev[static_cast<size_t>(l) + 1];
        const double *res = nullptr, *res_t = nullptr;           // the restriction reads res - res_t (or res alone)
        if (fused_level(l)) {
            // step 0 (x = dd = c D^-1 b) came with the restriction above; step 1 and the residual ride on their SpMVs
            ep(kEpNextLast, L, L.dd, b, 1, 0, nullptr, nullptr, L.x);
            ep(kEpResid, L, L.x, b, 0, 0, L.r.p, nullptr, nullptr);
            res = L.r.p;
        } else {
            (void)amg_smooth(s, M, L, b, true, deg_of(l), ctl, l == 0 && first0_done);
            amg_spmv(s, M, L, L.x, L.t.p);
            res = b;
            res_t = L.t.p;
        }
        const bool first_below = fused_level(l + 1);              // the next level wants its step 0 from this launch
        touches(l + 1);                                           // (the restriction writes the next level's right-hand side and reads its dinv and lam)
        if (L.rbm) {
            amg_rbm_restrict_launch(s, L, C, C.n_nodes, L.n_nodes, res, res_t, M.eig_ratio, first_below ? C.dd : static_cast<double *>(nullptr),
                                    first_below ? C.x : static_cast<double *>(nullptr), ctl, L.n_nodes);
        } else
        hipLaunchKernelGGL(k_amg_restrict, dim3(grid_for(C.n)), dim3(kBlock), 0, s->stream, C.n, static_cast<const int32_t *>(L.mem_ptr.p),
                           static_cast<const int32_t *>(L.mem_idx.p), res, res_t, C.b.p, static_cast<const double *>(C.dinv.p),
                           static_cast<const double *>(C.lam.p), M.eig_ratio, first_below ? C.dd : static_cast<double *>(nullptr),
                           first_below ? C.x : static_cast<double *>(nullptr), ctl);
        // ---- the coarse problem
        visit(l + 1);
        if (M.cycle_gamma > 1 && l + 1 <= M.w_to && l + 1 < nl - 1 && C.x1.p) {
            amg_spmv(s, M, C, C.x, C.t.p);
            hipLaunchKernelGGL(k_amg_w_between, dim3(vec_grid(C.n)), dim3(kBlock), 0, s->stream, C.n, C.b.p, static_cast<const double *>(C.t.p), C.x, C.x1.p,
                               static_cast<const double *>(C.dinv.p), static_cast<const double *>(C.lam.p), M.eig_ratio,
                               first_below ? C.dd : static_cast<double *>(nullptr), ctl);
            visit(l + 1);
            hipLaunchKernelGGL(k_amg_w_add, dim3(vec_grid(C.n)), dim3(kBlock), 0, s->stream, C.n, C.x, static_cast<const double *>(C.x1.p), ctl);
        }
        // ---- up
        if (L.rbm) {
            PFEM_RBM_DISPATCH(L.bs, L.dim, hipLaunchKernelGGL((k_rbm_prolong<FB, DIM>), dim3(vec_grid(L.n_nodes)), dim3(kBlock), 0, s->stream, L.n_nodes,
                static_cast<const int32_t *>(L.node_agg.p), static_cast<const double *>(L.roff.p), L.n_nodes, static_cast<const double *>(C.x),
                M.coarse_scale, L.x, ctl));
        } else
        hipLaunchKernelGGL(k_amg_prolong, dim3(vec_grid(L.n)), dim3(kBlock), 0, s->stream, L.n, static_cast<const int32_t *>(L.agg.p),
                           static_cast<const double *>(C.x), M.coarse_scale, L.x, ctl);
        if (fused_level(l)) {
            ep(kEpFirstRes, L, L.x, b, 0, 0, L.r.p, L.dd, nullptr);
            ep(kEpNextLast, L, L.dd, L.r.p, 1, 1, nullptr, nullptr, L.x);
        } else if (l == 0 && last0 == kLast0Epilogue) {
            // degree 1, a 4-row form on one rank: the step and the CG's (r,z), (z,z) are the product's epilogue; z goes to L.t
            // (other waves still gather L.x), one pair of partials per block, folded to kFoldBlocks here
            const unsigned gs = spmv_blocks(s);
            double *prz = s->d_part_ep.p, *pzz = prz + gs, *frz = pzz + gs, *fzz = frz + kFoldBlocks;
            launch_spmv<false, true>(s, L.x, nullptr, 0, nullptr, ctl, nullptr, nullptr, SliceSel{nullptr, 0}, Level0Ep{b, L.dinv.p, L.lam.p, M.eig_ratio, L.t.p, prz, pzz});
            hipLaunchKernelGGL(k_fold_partials2, dim3(kFoldBlocks, 2), dim3(kBlock), 0, s->stream, static_cast<const double *>(prz),
                               static_cast<const double *>(pzz), static_cast<int>(gs), frz, fzz, ctl);
        } else if (l == 0 && last0 == kLast0Product) {
            amg_spmv(s, M, L, L.x, L.t.p);          // degree 1: the step itself rides on the CG's dots kernel (k_pc_post_dots)
        } else {
            (void)amg_smooth(s, M, L, b, false, deg_of(l), ctl);
        }
    };
    visit(0);
    return last0 == kLast0Epilogue ? M.lev[0]->t.p : M.lev[0]->x;
}

// ---- the CG solve with z = M^-1 r from the V-cycle (KSPSolve, solverpetsc.F:476; -pc_type gamg) -----------------------
// Several ranks, default: ONE hierarchy across the ranks (amg_apply_coupled; what PCGAMG is under MPI) -- z comes out the
// same on every holder, no further exchange.  On request (PFEM_AMG_COUPLED=0): block Jacobi over the ranks with one
// hierarchy per rank on its owned diagonal block (PETSc: -pc_type bjacobi -sub_pc_type gamg; the reference's own parallel
// preconditioner is PCBJACOBI with ILU(0) blocks, solverpetsc.F:206).  A rank's block is built from its own elements only -- the interface rows lack the neighbour's
// share, which keeps it symmetric positive definite and needs no exchange of matrix entries.  Per iteration: the SpMV with
// its neighbour exchange and the all-reduce of (p,Ap) as in the Jacobi loop; the local V-cycles; one more neighbour
// exchange that hands the owners' z to the ranks that hold those dofs as ghosts (the ghosts send zeros, so the rank-ordered
// sum IS the owner's value, bit for bit); the all-reduce of (r,z), (z,z).
// V or W (-pc_mg_cycle_type; pfem_solver_set_amg_cycle, PFEM_AMG_CYCLE=v|w).  V unless asked otherwise.  What W buys was measured
// on the meshes whose aggregates come from matching (nodes moved off the lattice by 0.2 h, profiles/r05/wcycle_*.txt): the beam
// 67 -> 30 iterations, 200^3 18 -> 11 -- and 113 -> 234 ms, 33 -> 78 ms per step: level l is visited 2^l times, and from level 3
// on a visit is a handful of launches (or the single-workgroup tail) that cost their latency, not their flops: 32 visits of
// the tail alone outweigh the iterations saved.  Second visits on the first levels only (where a visit is bandwidth) make the
// preconditioner INDEFINITE on those meshes (the over-corrected V-cycle below has eigenvalues beyond 2, so 2B - BAB changes
// sign; CG stops with KSP_DIVERGED_INDEFINITE_PC): the W goes down to the tail or not at all.  On the lattice's bricks:
// 12 -> 8 and 18 -> 11 iterations, 18.6 -> 32.0 and 28.8 -> 49.0 ms.
// One hierarchy across several ranks keeps the V-cycle (a second visit would double the exchanges of every coarse level).
int amg_cycle_shape(pfem_solver *s, Amg &M)
{
    if (const char *e = std::getenv("PFEM_AMG_CYCLE")) M.cycle_gamma = (e[0] == 'w' || e[0] == 'W' || e[0] == '2') ? 2 : 1;
    else if (!M.cycle_given) M.cycle_gamma = 1;
    if (M.coupled) M.cycle_gamma = 1;
    if (M.cycle_gamma > 1)
        for (int l = 1; l <= M.w_to && l + 1 < static_cast<int>(M.lev.size()); ++l) {
            AmgLevel &L = *M.lev[static_cast<size_t>(l)];
            if (L.x1.n < static_cast<size_t>(std::max<int64_t>(L.n_loc, 1))) PFEM_TRY(L.x1.alloc(static_cast<size_t>(std::max<int64_t>(L.n_loc, 1))));
        }
    return PFEM_OK;
}

int run_pcg_amg(pfem_solver *s)
{
    const int64_t n = s->n_loc;
    const bool multi = cg_multi(s);
    mark_group_vals(s);
    PFEM_TRY(refresh_group_vals(s));
    bool overlap = false;
    PFEM_TRY(agree_overlap(s, multi, &overlap));
    PFEM_TRY(cg_require_comm(s, multi));
    if (multi && !s->rhs_summed) {
        PFEM_TRY(exchange_sum(s, s->d_rhs.p, overlap));
        s->rhs_summed = true;
    }
    bool did_symbolic = false;
    if (!s->amg || !s->amg->symbolic_ok) {
        did_symbolic = true;
        int rc = amg_symbolic(s, multi, overlap);
        if (rc == kAmgRetryBlock) {           // (all ranks get this verdict together) one hierarchy per rank instead
            s->amg->coupled_refused = true;
            rc = amg_symbolic(s, multi, overlap);
        }
        PFEM_TRY(rc);
        // a new hierarchy: no level's bound or codes come from a product of the old one, nor level 0's bound from an assembly for it
        s->asm_bound_fresh = false;
        for (auto &L : s->amg->lev) L->bound_fresh = L->bound_done = L->vd_direct = false;
    }
    Amg &M = *s->amg;
    amg_knobs(M);
    PFEM_TRY(amg_cycle_shape(s, M));
    M.coupled_fused = [] { const char *e = std::getenv("PFEM_AMG_COUPLED_FUSED"); return e ? std::atoi(e) != 0 : true; }();
    M.col_codes = [] { const char *e = std::getenv("PFEM_AMG_COL_CODES"); return e ? std::atoi(e) != 0 : true; }();      // (read at every solve)
    M.side_on = [] { const char *e = std::getenv("PFEM_AMG_SIDE_STREAM"); return e ? std::atoi(e) != 0 : true; }();      // (likewise)
    M.side_used = false;
    M.side_first = 0;
    M.side_ms = 0.0;
    if (M.coupled && M.coupled_fused && !s->d_row_sh.p && s->n_loc > 0) {        // level 0's dof -> shared index table (the coarse levels got theirs with their plans)
        PFEM_TRY(s->d_row_sh.alloc(static_cast<size_t>(s->n_loc)));
        PFEM_HIP(hipMemsetAsync(s->d_row_sh.p, 0xff, sizeof(int32_t) * static_cast<size_t>(s->n_loc), s->stream));
        if (s->n_sh > 0)
            hipLaunchKernelGGL(k_amg_fill_row_sh, dim3(grid_for(s->n_sh)), dim3(kBlock), 0, s->stream, s->n_sh, static_cast<const int32_t *>(s->d_sh_lidx.p), s->d_row_sh.p);
        PFEM_TRY(check_kernel("k_amg_fill_row_sh (level 0)"));
    }
    if (!M.ev_num0) PFEM_HIP(hipEventCreate(&M.ev_num0));
    if (!M.ev_num1) PFEM_HIP(hipEventCreate(&M.ev_num1));
    hipEvent_t ea = M.ev_num0, eb = M.ev_num1;
    PFEM_HIP(hipEventRecord(ea, s->stream));
    M.galerkin_fresh = did_symbolic;              // (only the phase that ran a moment ago, in THIS call, vouches for the coarse operators)
    if (M.rep) M.rep->galerkin_fresh = did_symbolic;
    // Between the fork of the numeric phase's side chain (amg_numeric) and the first cycle's wait for it (amg_apply) no way out of this
    // function may leave the chain running beside what the caller enqueues next: the solver's stream follows the side stream first.
    struct SideJoin {
        pfem_solver *s;
        Amg &M;
        ~SideJoin()
        {
            if (!M.side_pending || !M.side_stream || !M.ev_fork) return;
            if (hipEventRecord(M.ev_fork, M.side_stream) != hipSuccess || hipStreamWaitEvent(s->stream, M.ev_fork, 0) != hipSuccess)
                (void)hipStreamSynchronize(M.side_stream);
            M.side_pending = false;
        }
    } side_join{s, M};
    PFEM_TRY(amg_numeric(s, M, overlap));
    M.numeric_epoch = s->values_epoch;
    PFEM_HIP(hipEventRecord(eb, s->stream));          // (the solver's stream: the side chain has its own pair, ev_side0 .. ev_side1)
    M.cc_used.clear();              // (pfem_solver_amg_column_codes: what this solve's cycles run)
    for (size_t l = 1; l + 1 < M.lev.size(); ++l)
        if (amg_level_col_codes(M, *M.lev[l])) M.cc_used.push_back(static_cast<int>(l));
    const unsigned gv = vec_grid(n), gs = spmv_blocks(s);
    const dim3 block(kBlock);
    if (s->d_part_pw.n < gs + 2) PFEM_TRY(s->d_part_pw.alloc(gs + 2));
    double *part_pw = s->d_part_pw.p, *part_rz = s->d_part.p, *part_zz = s->d_part.p + kMaxGrid, *scal_pw = s->d_part.p + 2 * kMaxGrid;
    double *sbuf = s->d_sbuf.p;
    CgCtl *ctl = s->d_ctl.p;
    PFEM_TRY(cg_reset_control(s, ctl));
    double host_comm_s = 0.0;
    // Two fusions of the cycle's ends with the CG's own vector kernels (iterations only; same arithmetic, same bits):
    // step 0 of the pre-smoothing on the assembled matrix rides on k_pc_update, and -- when the fine degree is 1 -- the one
    // step of the post-smoothing rides on the dots kernel (or, `ep0` below, on the product in front of it).  Both need at least two levels.
    const int deg0 = M.fine_degree > 0 ? M.fine_degree : M.cheb_degree;
    const bool fuse_first0 = M.fused && M.lev.size() > 1 && !M.coupled;
    const bool fuse_last0 = M.fused && M.lev.size() > 1 && deg0 == 1 && !M.coupled;
    // One rank, level 0 in a relative-group form with 16-bit gaps: the iteration's (r,z), (z,z) are summed per block of the product
    // (1024 consecutive rows, 4 to the thread) and folded to kFoldBlocks -- by the epilogue of the cycle's last product (Level0Ep)
    // where the step rides on it, by k_pc_dots_rows4 behind every other cycle: the layout belongs to the form, not to the fusion.
    const bool rows4 = !multi && spmv_form(s).has_level0_epilogue();
    const bool ep0 = rows4 && fuse_last0;
    const int last0 = ep0 ? kLast0Epilogue : (fuse_last0 ? kLast0Product : kLast0Smooth);
    M.level0_ep = ep0;
    if (rows4 && s->d_part_ep.n < 2 * static_cast<size_t>(gs) + 2 * kFoldBlocks) PFEM_TRY(s->d_part_ep.alloc(2 * static_cast<size_t>(gs) + 2 * kFoldBlocks));
    double *ep_rz = s->d_part_ep.p, *ep_zz = ep_rz ? ep_rz + gs : nullptr, *fold_rz = ep_rz ? ep_zz + gs : nullptr, *fold_zz = ep_rz ? fold_rz + kFoldBlocks : nullptr;
    // One rank: the cycle of the iterations (the one that takes the control block) is replayed from a hipGraph -- a
    // dependent tiny kernel costs ~3.4 us on a stream and ~1.75 us in a graph (tools/lab/graph_gap.hip), and six of the
    // eight levels of the 200^3 hierarchy are too small to fill the chip.  PFEM_CG_GRAPH=0 turns it off.
    bool use_vgraph = false;
    {
        const int graph_env = cg_graph_env();
        // (several ranks: stream launches.  The coupled cycle with its RCCL calls as one captured graph was tried this round -- it
        // would take the ~80 launches of an iteration off the host, which runs ahead of the device anyway -- and the replay never
        // returned in the self-peer probe (tools/probe_coupled.py); dropped)
        // (round 5: a transport whose calls are plain kernel launches with constant arguments -- peer memory, message counters on
        // the device -- lets the cycle ACROSS ranks be captured too: ~65 of an iteration's ~80 launches leave the host)
        const bool coupled_capturable = multi && M.coupled && !overlap && s->comm && s->comm->capturable() && s->comm->p2p_capturable() &&
                                        (!M.rep || M.n_last_global <= s->comm->allreduce_capture_limit());
        if ((!multi || coupled_capturable) && graph_env && s->stream != nullptr) {
            std::vector<uint64_t> key = {reinterpret_cast<uint64_t>(s->d_r.p), reinterpret_cast<uint64_t>(ctl), reinterpret_cast<uint64_t>(s->stream),
                                         reinterpret_cast<uint64_t>(s->d_vals.p), reinterpret_cast<uint64_t>(s->d_cols.p), reinterpret_cast<uint64_t>(s->d_rvals.p),
                                         reinterpret_cast<uint64_t>(s->d_gvals.p), reinterpret_cast<uint64_t>(s->d_dwords.p), spmv_key(s),
                                         static_cast<uint64_t>(M.cheb_degree), static_cast<uint64_t>(M.fine_degree), static_cast<uint64_t>(M.dense),
                                         static_cast<uint64_t>(M.eig_ratio * 1e6), static_cast<uint64_t>(M.coarse_scale * 1e6), static_cast<uint64_t>(M.lev.size()),
                                         static_cast<uint64_t>(M.fused), static_cast<uint64_t>(M.tail_from + 1), static_cast<uint64_t>(M.coupled),
                                         static_cast<uint64_t>(M.cycle_gamma), static_cast<uint64_t>(M.w_to + 1),
                                         static_cast<uint64_t>(M.coupled_fused), reinterpret_cast<uint64_t>(s->d_send.p), reinterpret_cast<uint64_t>(s->d_recv.p),
                                         reinterpret_cast<uint64_t>(s->comm), reinterpret_cast<uint64_t>(M.rep.get()), reinterpret_cast<uint64_t>(M.bx_glob.p),
                                         static_cast<uint64_t>(last0), ep0 ? reinterpret_cast<uint64_t>(s->d_part_ep.p) : 0, ep0 ? static_cast<uint64_t>(gs) : 0,
                                         reinterpret_cast<uint64_t>(M.lev[0]->t.p), reinterpret_cast<uint64_t>(M.lev[0]->dinv.p)};
            auto level_key = [&](const std::unique_ptr<AmgLevel> &L) {
                key.push_back(reinterpret_cast<uint64_t>(L->x)); key.push_back(reinterpret_cast<uint64_t>(L->vals.p)); key.push_back(static_cast<uint64_t>(L->n));
                key.push_back(L->vd.ok ? static_cast<uint64_t>(L->vd.n + 1) : 0); key.push_back(reinterpret_cast<uint64_t>(L->vcodes.p));
                // (the column codes: whether the level's products read them, and from where)
                const bool cc = amg_level_col_codes(M, *L);
                key.push_back(cc ? static_cast<uint64_t>(L->cd_n + 1) : 0); key.push_back(cc ? reinterpret_cast<uint64_t>(L->ccodes.p) : 0);
                key.push_back(cc ? reinterpret_cast<uint64_t>(L->cdelta.p) : 0);
            };
            for (auto &L : M.lev) level_key(L);
            if (M.rep) for (auto &L : M.rep->lev) level_key(L);
            PFEM_TRY(M.graph.ensure(s->stream, std::move(key), {s->stream}, [&](int) {
                if (M.coupled) return amg_apply_coupled(s, M, s->d_r.p, ctl, overlap) != nullptr;
                (void)amg_apply(s, M, s->d_r.p, ctl, fuse_first0, last0);
                return true;
            }, &use_vgraph));
        }
    }
    // z = M^-1 r on every local dof: the V-cycle on the owned block, then (several ranks) the owners' values to the ghosts
    auto precondition = [&](const CgCtl *c) -> double * {
        if (use_vgraph && c == ctl) {
            if (hipGraphLaunch(M.graph.exec[0], s->stream) != hipSuccess) return nullptr;
            return ep0 ? M.lev[0]->t.p : M.lev[0]->x;
        }
        if (M.coupled) return amg_apply_coupled(s, M, s->d_r.p, c, overlap);      // z is the same on every holder already
        // (the first cycle, c == nullptr, is the one that joins the numeric phase's side chain)
        const bool join = c == nullptr && M.side_pending;
        double *z = amg_apply(s, M, s->d_r.p, c, c == ctl && fuse_first0, c == ctl ? last0 : kLast0Smooth, join ? M.side_first : 0, join ? M.ev_side1 : nullptr);
        if (c == ctl && fuse_last0) return z;            // the exchange follows the fused last step (dots lambda)
        if (multi && exchange_sum(s, z, overlap) != PFEM_OK) return nullptr;
        return z;
    };
    // (r,z), (z,z) over the owned rows; several ranks: summed into sbuf[2..3]
    auto dots = [&](double *z, const CgCtl *c, hipEvent_t *cev) -> int {
        if (c == ctl && ep0) return PFEM_OK;             // (the cycle's last product left the folded sums)
        if (c == ctl && rows4) {
            hipLaunchKernelGGL(k_pc_dots_rows4, dim3(gs), block, 0, s->stream, c, s->n_owned, static_cast<const double *>(s->d_r.p),
                               static_cast<const double *>(z), ep_rz, ep_zz);
            hipLaunchKernelGGL(k_fold_partials2, dim3(kFoldBlocks, 2), block, 0, s->stream, static_cast<const double *>(ep_rz),
                               static_cast<const double *>(ep_zz), static_cast<int>(gs), fold_rz, fold_zz, c);
            return PFEM_OK;
        }
        if (c == ctl && fuse_last0) {
            AmgLevel &L0 = *M.lev[0];
            hipLaunchKernelGGL(k_pc_post_dots, dim3(gv), block, 0, s->stream, c, n, s->n_owned, static_cast<const double *>(s->d_r.p),
                               static_cast<const double *>(L0.t.p), static_cast<const double *>(L0.dinv.p), static_cast<const double *>(L0.lam.p),
                               M.eig_ratio, z, part_rz, part_zz);
            if (multi) PFEM_TRY(exchange_sum(s, z, overlap));          // the owners' z to the ghost holders (precondition left it to us)
        } else {
            hipLaunchKernelGGL(k_pc_dots, dim3(gv), block, 0, s->stream, c, n, s->n_owned, static_cast<const double *>(s->d_r.p),
                               static_cast<const double *>(z), part_rz, part_zz);
        }
        if (multi) {
            hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, s->stream, static_cast<const double *>(part_rz),
                               static_cast<const double *>(part_zz), static_cast<int>(gv), sbuf + 2, c);
            if (cev) PFEM_HIP(hipEventRecord(cev[4], s->stream));
            PFEM_TRY(s->comm->allreduce(sbuf + 2, 2, s->stream));
            if (cev) PFEM_HIP(hipEventRecord(cev[5], s->stream));
        }
        return PFEM_OK;
    };
    // Single-reduction form (pfem_solver_set_cg_single_reduction / -ksp_cg_single_reduction) for the hierarchy across the ranks:
    // s = A z instead of w = A p, (p,Ap) by recurrence, so (z,s), (r,z), (z,z) travel in ONE all-reduce -- with the cycle's own
    // (the replicated level's right-hand side) two per iteration instead of three.  One rank keeps the two-reduction loop (its
    // fused ends: the single-reduction form streams two more vectors).
    if (multi && M.coupled && want_single_reduction(s)) {
        bool grown = false;
        PFEM_TRY(ensure_guarded(s->d_zg, n, &grown));
        PFEM_HIP(hipMemsetAsync(s->d_zg.store.p, 0, (static_cast<size_t>(n) + 2 * kVecGuard) * sizeof(double), s->stream));
        if (s->d_sv.n < static_cast<size_t>(std::max<int64_t>(n, 1))) PFEM_TRY(s->d_sv.alloc(static_cast<size_t>(std::max<int64_t>(n, 1))));
        double *zg = s->d_zg.p, *sv = s->d_sv.p;
        hipLaunchKernelGGL(k_pc_init, dim3(gv), block, 0, s->stream, n, static_cast<const double *>(s->d_rhs.p), s->d_x.p, s->d_r.p);
        auto step1 = [&](int it, int, int *) -> int {
            double *zc = amg_apply_coupled(s, M, s->d_r.p, ctl, overlap);          // (every kernel leaves at once when the solve has finished)
            if (!zc) return PFEM_ERR_COMM;
            hipLaunchKernelGGL(k_pc_dots, dim3(gv), block, 0, s->stream, static_cast<const CgCtl *>(ctl), n, s->n_owned, static_cast<const double *>(s->d_r.p),
                               static_cast<const double *>(zc), part_rz, part_zz);
            hipLaunchKernelGGL(k_pc_copy, dim3(gv), block, 0, s->stream, n, static_cast<const double *>(zc), zg);       // into the guarded SpMV input
            PFEM_TRY(spmv_exchange(s, zg, sv, part_pw, gs, overlap, ctl, nullptr, nullptr, nullptr, nullptr, nullptr, &host_comm_s, [&](int nblocks) -> int {
                hipLaunchKernelGGL(k_reduce_partials3, dim3(1), dim3(1024), 0, s->stream, static_cast<const double *>(part_pw), nblocks,
                                   static_cast<const double *>(part_rz), static_cast<const double *>(part_zz), static_cast<int>(gv), sbuf,
                                   static_cast<const CgCtl *>(ctl));
                return 3;
            }));
            hipLaunchKernelGGL(k_pcg1_step, dim3(gv), block, 0, s->stream, ctl, it, n, static_cast<const double *>(sbuf), static_cast<const double *>(nullptr), 0,
                               static_cast<const double *>(nullptr), static_cast<const double *>(nullptr), 0, static_cast<const double *>(zg),
                               static_cast<const double *>(sv), s->d_p.p, s->d_w.p, s->d_x.p, s->d_r.p, s->rtol, s->abstol, s->dtol, s->d_hist.p,
                               s->hist_cap, s->maxits);
            return PFEM_OK;
        };
        // a fixed batch of 4 (step maxits only judges)
        PFEM_TRY(cg_iterate(s, ctl, std::max(s->maxits, 0) + 1, host_comm_s, [](const CgCtl &) { return 4; }, step1,
                            "gamg single-reduction pcg iteration"));
        PFEM_TRY(CgSampler(s, multi).tally(overlap, s->last_its + 1, false));      // nothing sampled: zeroes the figures
        float fs = 0.f;
        PFEM_HIP(hipEventElapsedTime(&fs, ea, eb));
        M.numeric_ms = fs;
        return PFEM_OK;
    }
    const double *red2 = multi ? sbuf + 2 : nullptr;
    hipLaunchKernelGGL(k_pc_init, dim3(gv), block, 0, s->stream, n, static_cast<const double *>(s->d_rhs.p), s->d_x.p, s->d_r.p);
    double *z = precondition(nullptr);
    if (!z) return PFEM_ERR_COMM;
    PFEM_TRY(dots(z, nullptr, nullptr));
    hipLaunchKernelGGL(k_cg_start, dim3(1), block, 0, s->stream, ctl, static_cast<const double *>(part_rz), static_cast<const double *>(part_zz),
                       static_cast<int>(gv), red2, s->rtol, s->abstol, s->dtol, s->d_hist.p);
    hipLaunchKernelGGL(k_pc_copy, dim3(gv), block, 0, s->stream, n, static_cast<const double *>(z), s->d_p.p);
    PFEM_TRY(check_kernel("gamg pcg start"));

    // Iterations enqueued between two reads of the control block.  An iteration enqueued after the verdict still costs its
    // ~40 launches (each leaves at once, ~0.1 ms together), a read costs a round trip: one rank sizes the next batch from
    // the contraction seen so far -- the multigrid cycle contracts at a steady rate -- instead of a fixed 4; several ranks
    // keep the fixed size (every rank must enqueue the same calls, and nothing may depend on a host's libm for that).
    const int chunk_env = cg_chunk_env();
    const int chunk = chunk_env > 0 ? chunk_env : 4;
    auto batch = [&](const CgCtl &h) -> int {
        if (!multi && chunk_env == 0 && h.its >= chunk && h.rn > 0.0 && h.rn < h.rn0 && h.ttol > 0.0 && h.rn > h.ttol) {
            const double rate = std::pow(h.rn / h.rn0, 1.0 / h.its);         // mean contraction per iteration so far
            const double need = std::log(h.ttol / h.rn) / std::log(rate);
            // (three quarters of the estimate, at most 16: a CG that stalls and then drops -- the beam -- makes the estimate
            // overshoot near the end, and 60 iterations enqueued for nothing cost 7 ms there)
            return need >= 1.0 ? std::min(16, std::max(1, static_cast<int>(std::ceil(0.75 * need)))) : 1;
        }
        return chunk;
    };
    CgSampler sampler(s, multi);
    auto step = [&](int it, int, int *) -> int {
        hipEvent_t e[4] = {}, *cev = nullptr;
        if (sampler.due(it)) {
            PFEM_TRY(sampler.spmv(e));
            PFEM_TRY(sampler.comm(&cev));        // the sampled iterations also time the exchange and the all-reduces
        }
        const double *pw_parts = part_pw, *red_pw = nullptr;
        int pw_n = static_cast<int>(gs);
        if (multi) {
            PFEM_TRY(spmv_exchange(s, s->d_p.p, s->d_w.p, part_pw, gs, overlap, ctl, e[0], e[1], e[2], e[3], cev, &host_comm_s, [&](int nblocks) -> int {
                hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, s->stream, static_cast<const double *>(part_pw),
                                   static_cast<const double *>(nullptr), nblocks, sbuf, static_cast<const CgCtl *>(ctl));
                return 1;
            }));
            red_pw = sbuf;
            pw_n = 0;
        } else {
            launch_spmv<true>(s, s->d_p.p, s->d_w.p, n, part_pw, ctl, e[0], e[1]);
            cg_fold(s, part_pw, gs, scal_pw, ctl, &pw_parts, &pw_n);
        }
        {
            AmgLevel &L0 = *M.lev[0];
            hipLaunchKernelGGL(k_pc_update, dim3(gv), block, 0, s->stream, ctl, it, n, pw_parts, pw_n, red_pw,
                               static_cast<const double *>(s->d_w.p), s->d_r.p, L0.n, static_cast<const double *>(L0.dinv.p),
                               static_cast<const double *>(L0.lam.p), M.eig_ratio, fuse_first0 ? L0.x : static_cast<double *>(nullptr),
                               (fuse_first0 && deg0 > 1) ? L0.dd : static_cast<double *>(nullptr));
        }
        z = precondition(ctl);
        if (!z) return PFEM_ERR_COMM;
        PFEM_TRY(dots(z, ctl, cev));
        hipLaunchKernelGGL(k_pc_direction, dim3(gv), block, 0, s->stream, ctl, it, n, static_cast<const double *>(rows4 ? fold_rz : part_rz),
                           static_cast<const double *>(rows4 ? fold_zz : part_zz), rows4 ? kFoldBlocks : static_cast<int>(gv), red2, static_cast<const double *>(z), s->d_p.p, s->d_x.p,
                           s->d_hist.p, s->hist_cap, s->maxits);
        return PFEM_OK;
    };
    PFEM_TRY(cg_iterate(s, ctl, s->maxits, host_comm_s, batch, step, "gamg pcg iteration"));
    PFEM_TRY(sampler.tally(overlap, s->last_its, true));
    float f = 0.f;
    PFEM_HIP(hipEventElapsedTime(&f, ea, eb));
    M.numeric_ms = f;
    if (M.side_used) {
        PFEM_HIP(hipEventElapsedTime(&f, M.ev_side0, M.ev_side1));
        M.side_ms = f;
    }
    return PFEM_OK;
}

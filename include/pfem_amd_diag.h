/* pfem_amd_diag.h -- introspection, measurement and lab knobs of libpfem_amd.so.
 *
 * NOT part of the drop-in boundary: nothing here replaces an interface of the reference (chennachaos/PFEMFort).  include/pfem_amd.h
 * is what a maintainer binds (INTEGRATION.md section 1 maps each of its entry points to the reference interface it replaces); this
 * header is what the build's own tests, bench.py and lab probes use to look inside the solver: which SpMV form and assembly
 * formulation a pattern got, the multigrid hierarchy of the last solve (levels, aggregates, transfer, layout across ranks, one
 * instrumented cycle), device-evaluated element matrices for the parity tests, event timings, and the transport's self-test and
 * latency probes.  Same conventions: extern "C", plain pointers and sizes, int return codes.                                      */
#ifndef PFEM_AMD_DIAG_H
#define PFEM_AMD_DIAG_H

#include "pfem_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Numeric-assembly formulation used by pfem_assemble:
 *   GATHER  (default) one thread per node walks its incident elements in ascending element
 *           order and owns its matrix rows: no atomics, K and F bit-identical to the serial
 *           reference loop, run-to-run deterministic;
 *   SCATTER one thread per element, hardware f64 atomicAdd into the matrix (sum order varies). */
#define PFEM_ASSEMBLY_GATHER 0
#define PFEM_ASSEMBLY_SCATTER 1
int pfem_solver_set_assembly_mode(pfem_solver *s, int mode);
/* what pfem_assemble does with the current pattern: gather form in effect (1/0); nodes whose rows are too long for the
 * gather records (> 255 entries: "hubs" -- their rows alone are assembled by a scatter pass with atomics, every other
 * row keeps one writer); threads and LDS bytes per block of the row-accumulating gather kernels                      */
int pfem_solver_assembly_info(pfem_solver *s, int *gather_form, int *hub_nodes, int *block_threads, int64_t *lds_bytes);
/* kernel time (HIP events around the kernels; host copies excluded) of the last pfem_post_elements / pfem_post_nodal_forces call */
int pfem_post_timings(pfem_solver *s, double *elements_ms, double *nodal_forces_ms);
/* the same for the last pfem_post_nodal_recovery / pfem_post_error_indicator call (the indicator's time includes its recovery) */
int pfem_post_recovery_timings(pfem_solver *s, double *recovery_ms, double *indicator_ms);
/* Matrix encoding streamed by the SpMV.  AUTO uses 16-bit gaps between the ascending columns of a
 * row (4 + 2 B per entry instead of 4 B) whenever every gap of the pattern fits, and on top of that
 * serves consecutive rows with identical column sets (the dof rows of a node) from one lane with a
 * shared column stream when the pattern has, on average, at least 2.75 such rows per group of 3;
 * or (scalar problems) serves 4 consecutive rows from one lane with the union of their columns
 * relative to the row -- both only when the system is large enough to keep the chip full with
 * 3-4x fewer waves (>= 327 680 groups); GROUPED takes the group forms at any size, GAPS16 forces
 * the plain row form with 16-bit gaps, INT32 plain int32 columns.  Every row sums the same
 * products in the same order: y is bit-identical in all of them. */
#define PFEM_SPMV_AUTO 0
#define PFEM_SPMV_INT32 1
#define PFEM_SPMV_GAPS16 2
#define PFEM_SPMV_GROUPED 3   /* the row-group forms whenever the pattern has them, however small the system */
int pfem_solver_set_spmv_format(pfem_solver *s, int format);
/* 16 if the SpMV currently streams 16-bit column gaps, 32 for int32 columns */
int pfem_solver_get_spmv_format(pfem_solver *s, int *bits_per_column);
/* rows served by one lane of the current SpMV: 3 in the row-grouped form, else 1 */
int pfem_solver_get_spmv_row_group(pfem_solver *s, int *rows_per_lane);
/* Relative row groups whose pattern has gaps beyond 65535 (planes of more than 65 535 nodes): number of entries of the
 * table of distinct large gaps when the 16-bit DICTIONARY form is in use (codes >= 0x8000 index the table; at most
 * 256 distinct gaps of 32768 and more), 0 otherwise (literal 16-bit gaps, 32-bit gaps, or another form).            */
int pfem_solver_get_spmv_gap_table(pfem_solver *s, int *entries);
/* Value dictionary of the SpMV's group forms (pfem_valdict.hpp): when the assembled matrix holds at most 4096 distinct values
 * (structured meshes: element matrices repeat) the SpMV streams 16-bit codes into a dictionary held in LDS instead of the
 * doubles -- the same doubles, the same products, the same bits, 2 B a slot instead of 8.  *entries = the dictionary's size
 * after the last solve / product, 0 when the fp64 copy is streamed (PFEM_SPMV_VALDICT=0 turns the form off).               */
int pfem_solver_get_spmv_value_dictionary(pfem_solver *s, int *entries);
/* ... and per level of the last gamg hierarchy (scalar coarse levels of >= 2^20 slots on one rank take the form too: the Galerkin
 * sums over the bricks of a lattice repeat like the element matrices do): entries[l] = the level's dictionary size, 0 = fp64 values */
int pfem_solver_amg_value_dictionaries(pfem_solver *s, int max_levels, int *n_levels, int *entries);
/* 1 when the row form streams 16-bit gaps WITH ESCAPES (k_spmv16e: the code 0xffff sends a column to the matrix's int32 column
 * array -- numberings whose far neighbours are too many and too irregular for the table: partition-renumbered and
 * curve-ordered meshes; taken when at most a quarter of the entries escape), else 0.  Same bits as every other form.     */
int pfem_solver_get_spmv_gap_escapes(pfem_solver *s, int *in_use);
/* bytes one launch of the selected SpMV form moves at best: its own storage (values, gap words / columns, offsets)
 * + x + y, each touched once.  (The judged figure 12 nnz + 20 N of SURVEY 8d is the plain int32-CSR equivalent.)   */
int pfem_solver_spmv_bytes(pfem_solver *s, int64_t *format_bytes);

/* GAMG hierarchy of the last solve: number of levels, rows / nonzeros / eigenvalue bound of each (arrays of max_levels),
 * time of the symbolic phase (once per pattern) and of the numeric phase of the last solve (inside its timer), the knobs */
int pfem_solver_amg_info(pfem_solver *s, int max_levels, int *n_levels, int64_t *rows, int64_t *nnz, double *lambda_max,
                         double *symbolic_ms, double *numeric_ms, int *cheb_degree, int *fine_degree, double *eig_ratio, double *coarse_scale);
/* coarse dof of every dof of `level` (0 = the assembled matrix); what the oracle's restatement of the cycle is given */
int pfem_solver_amg_aggregates(pfem_solver *s, int level, int32_t *agg);
/* Displacement problems (as many dofs per node as space dimensions: the tetra / tria elasticity kinds), mesh on the
 * device: the coarse space carries the RIGID-BODY MODES of every aggregate (PETSc: MatSetNearNullSpace / PCSetCoordinates
 * ahead of PCGAMG; tetraelasticityparallelimpl1.F:894-902, 993) -- dim translations and 3 (plane: 1) rotations about the
 * aggregate's centroid, so a coarse node has 6 (3) dofs; the beam of BASELINE config 4 needs 18 iterations instead of 169.
 * What the transfer from `level` to the next one looks like (one rank, and the hierarchy across several): *rbm = 1 when it
 * carries rotations, dofs per node on this level and the next, the space dimension, and (optional, [3 x n_nodes] as x | y | z) the coordinates of this level's
 * nodes (level 0: the mesh nodes in dof order; below: the centroids of the aggregates).  With *rbm = 1
 * pfem_solver_amg_aggregates reports the TRANSLATION part: dof c of node i belongs to coarse dof coarse_bs * aggregate(i) + c. */
int pfem_solver_amg_transfer(pfem_solver *s, int level, int *rbm, int *fine_bs, int *coarse_bs, int *dim, int64_t *n_nodes, double *node_xyz);
/* several ranks: is the hierarchy of the last solve one across the ranks (1) or one per rank (0); how many of its levels
 * are distributed over the ranks (the levels after them -- at most PFEM_AMG_REPLICATE_ROWS rows over all ranks, default
 * 150000 -- are assembled on every rank, which carries the rest of the cycle alone); per level (arrays of max_levels) the
 * global number of this rank's first dof and its local rows (owned + ghosts; replicated levels: 0 and all rows).  With a
 * coupled hierarchy pfem_solver_amg_aggregates hands out GLOBAL coarse numbers and pfem_solver_amg_info's rows are the
 * owned ones on the distributed levels, all rows on the replicated ones.                                                */
int pfem_solver_amg_layout(pfem_solver *s, int max_levels, int *coupled, int *distributed_levels, int64_t *first_dof, int64_t *local_rows);
/* the gather form's incidence lists as translated copies of patterns (lists equal up to a shift of the node numbers, as a mesh
 * numbered along lines has them): number of patterns in use (0: every node reads its own records) and the longest list      */
int pfem_solver_incidence_patterns(pfem_solver *s, int *count, int *longest);
/* how the aggregates of every level of the last gamg hierarchy were formed (kind[l], l < *n_levels; the last level: 0):
 * 1 bricks of the lattice in one step, 2 node bricks in one step (rigid-body transfer), 3 bricks split between their owners
 * (several ranks whose dofs do not fill boxes), 4 pairing passes along the axes of the lattice, 5 matching on the strength
 * graph.                                                                                                                  */
int pfem_solver_amg_aggregation(pfem_solver *s, int max_levels, int *n_levels, int *kind);
/* several ranks: neighbour exchanges and all-reduces ONE V-cycle of the last solve enqueued (next to the CG's own exchange
 * and two all-reduces per iteration); 0 / 0 on one rank                                                                */
int pfem_solver_amg_comm_counts(pfem_solver *s, int *exchanges_per_cycle, int *allreduces_per_cycle);
/* One instrumented V-cycle of the hierarchy across the ranks (collective, after a -pc_type gamg solve of a multi-rank run):
 * per level l < *n_levels the neighbour exchanges the cycle enqueues there, their summed time (event pairs on the stream that
 * carries them) and doubles sent; the cycle's all-reduces (the replicated level's right-hand side / the dense bottom) likewise;
 * the whole cycle's time.  PFEM_ERR_STATE without such a hierarchy.  Diagnostic (bench.py's N > 1 line). */
int pfem_solver_amg_cycle_profile(pfem_solver *s, int max_levels, int *n_levels, int *exchanges, double *exchange_ms,
                                  int64_t *exchange_doubles, int *allreduces, double *allreduce_ms, int64_t *allreduce_doubles,
                                  double *cycle_ms);
/* how many levels of the last hierarchy were coarsened by pairing on the mesh's lattice (the others: by matching on the
 * strength graph); 0 when the mesh has no lattice or came without coordinates                                          */
int pfem_solver_amg_pairing(pfem_solver *s, int *lattice_levels);
/* the cycle the last gamg solve ran: 1 = V, 2 = W, and the last level whose problem got two visits (0 with V)          */
int pfem_solver_amg_cycle(pfem_solver *s, int *cycle, int *last_level_visited_twice);
/* 1 when the iterations of the last gamg solve ran the cycle's last product on the assembled matrix with the final smoothing
 * step and the CG's (r,z), (z,z) as its epilogue (one rank, a 4-row relative-group SpMV form with 16-bit gaps, fine degree 1,
 * PFEM_AMG_FUSED not 0); 0 when they took the stand-alone kernels                                                          */
int pfem_solver_amg_level0_epilogue(pfem_solver *s, int *taken);
/* the first level of the cycle's single-launch tail (k_amg_tail walks it and every level below it in one workgroup), or -1
 * when the cycle goes level by level all the way down (PFEM_AMG_FUSED=0, several ranks, no level small enough);
 * *tail_build: which build of the tail the last cycle launched -- 0 none, 1 everything in memory, 2 vectors and index lists in
 * LDS, 3 the first tail level's matrix in LDS as well; *bounds_by_products: coarse levels whose eigenvalue bound the last
 * numeric phase took from the Galerkin product that formed them instead of k_amg_max_rows / k_amg_max (0 in a pattern's first
 * solve, whose products run in the symbolic phase)                                                                       */
int pfem_solver_amg_tail_from(pfem_solver *s, int *tail_from, int *tail_build, int *bounds_by_products);
/* the side chain of the last gamg solve's numeric phase: *used = 1 when the products that form the levels from *first_level on and
 * the dense inverse ran on a stream of their own beside the first cycle's upper levels (one rank, plain transfers, fused kernels, a
 * warm step of at least two levels one of which lies below every level that takes the value dictionary; PFEM_AMG_SIDE_STREAM not 0),
 * and *ms = that chain's span on its stream (pfem_solver_amg_info's numeric_ms then covers the solver's own stream only); 0, 0, 0
 * when everything ran on the solver's stream (always so in a pattern's first solve).  Same bits either way.                    */
int pfem_solver_amg_side_stream(pfem_solver *s, int *used, int *first_level, double *ms);
/* 1 when the numeric phase of the last gamg solve formed level 1 from the SpMV's 16-bit value codes (one rank, a scalar brick
 * level 0 whose 4-row relative-group form streams codes that hold the current values; PFEM_AMG_GALERKIN_CODES not 0); 0 when it
 * read the fp64 row form (the first step of a pattern forms the level in the symbolic phase: 0 as well).  Same bits either way. */
int pfem_solver_amg_galerkin_from_codes(pfem_solver *s, int *taken);
/* the stored values of coarse level `level` (>= 1) of the last hierarchy in slot order, padding included: *stored of them, the
 * first min(max_values, *stored) copied to vals (max_values = 0: the count alone)                                             */
int pfem_solver_amg_level_values(pfem_solver *s, int level, int64_t max_values, double *vals, int64_t *stored);
/* the levels whose fused products of the last gamg solve read one-byte column codes instead of int32 columns (the levels that
 * take the value dictionary, on one rank, once their codes have been built and compared with the columns on the device;
 * PFEM_AMG_COL_CODES not 0), ascending: *n_levels of them, at most max_levels written; *builds: how many times this hierarchy has
 * built a level's codes (a refused level is counted once and never built again)                                              */
int pfem_solver_amg_column_codes(pfem_solver *s, int max_levels, int *n_levels, int *levels, int *builds);
/* the columns of coarse level `level` (>= 1) of the last hierarchy in slot order, padding included: *stored of them, the first
 * min(max_cols, *stored) copied to cols.  decoded = 0: the level's int32 columns; decoded = 1: decoded on the device from the
 * level's column codes and offset table (PFEM_ERR_STATE when it has none).  The two agree on every slot of every row < n; the
 * lanes past n of the last slice read 0 either way                                                                          */
int pfem_solver_amg_level_columns(pfem_solver *s, int level, int decoded, int64_t max_cols, int32_t *cols, int64_t *stored);
/* coarse level `level` (>= 1) of the last hierarchy as plain CSR with the padding slots dropped and the columns of a row ascending,
 * as pfem_get_csr hands out the matrix itself: rowptr [*n + 1], cols and vals [*nnz].  A slot belongs to its row iff its index
 * within the row is below the row's stored length, whatever it holds.  rowptr = cols = vals = NULL: the sizes alone (call twice).
 * One rank after a gamg solve; PFEM_ERR_STATE without a hierarchy or with one across the ranks.  Built on the host from the
 * level's arrays copied back: what the tests compare with an independently formed P^T A P.                                    */
int pfem_solver_amg_level_csr(pfem_solver *s, int level, int64_t *rowptr, int32_t *cols, double *vals, int64_t *n, int64_t *nnz);
/* z = M^-1 r: ONE application of the multigrid cycle of the last gamg solve, with the numeric set-up (coarse operators, inverse
 * diagonals, bounds, dense bottom) that solve left -- the call its CG makes for z_0.  r and z: host arrays of n_local doubles in
 * the caller's dof order (the internal renumbering does not show).  Synchronises the stream.  Leaves the cycle's graph and every
 * state the next solve reads as they are: solve, apply, solve gives the bits of solve, solve.  One rank after a gamg solve;
 * PFEM_ERR_STATE without a hierarchy or with one across the ranks.  What the tests compare, vector by vector, with the oracle's
 * cycle evaluated in extended precision.                                                                                       */
int pfem_solver_amg_apply(pfem_solver *s, const double *r, double *z);

/* Per-element Ke/Fe of the uploaded mesh as computed by the DEVICE kernel (parity
 * inspection): K_out[e*nsize*nsize + i + nsize*j], F_out[e*nsize + i].           */
int pfem_eval_elems(pfem_solver *s, const double *elemData, const double *timeData,
                    double *K_out, double *F_out);

/* local matrix dimensions: n_local = owned + ghost rows, nnz of the pattern      */
int pfem_matrix_info(pfem_solver *s, int64_t *n_owned, int64_t *n_local, int64_t *nnz,
                     int64_t *stored_entries);

/* An arbitrary CSR matrix (n = size_global rows, one rank) through the MatSetValues compat path, for tests that need a pattern
 * or values no mesh produces: a host loop over the public calls and nothing else -- pfem_mat_set_values(INSERT_VALUES) once per
 * row for the pattern, pfem_solver_set_zero, pfem_mat_set_values(INSERT_VALUES) once per row for the values (not ADD_VALUES: a
 * sum with the +0.0 of set_zero loses the sign of -0.0 and the payload bit of a signalling NaN, and every bit pattern has to
 * arrive as given).  values_only != 0: set_zero and the value loop alone, on the standing pattern.  The values are staged on
 * the host; the next solve pushes them to the device, as for the compat calls.                                              */
int pfem_load_csr(pfem_solver *s, int64_t n, const int64_t *rowptr, const int32_t *cols, const double *vals, int values_only);
/* y = A_local x (both length n_local, host arrays): one launch of the CG SpMV kernel */
int pfem_spmv(pfem_solver *s, const double *x, double *y);
/* time `reps` back-to-back SpMV launches with HIP events on the solver's stream */
int pfem_bench_spmv(pfem_solver *s, int reps, double *ms_per_launch);
/* time of one explicit step (pfem_dynamics_run's two launches) in microseconds, inside `graphs` back-to-back replays of the
 * captured step graph between two HIP events, after a run that aligns the step counter, captures and warms up; undamped, no
 * history.  The state advances by the steps taken.  PFEM_ERR_STATE where the stream cannot be captured.                     */
int pfem_dynamics_bench(pfem_solver *s, double dt, int graphs, double *us_per_step, int *steps_per_graph);
/* time of one iteration of pfem_dynamics_run_implicit's shifted CG loop (three launches) in microseconds: `iterations`
 * iterations of the first step from the state at hand between two HIP events, with no convergence exit (rtol = 0), after one
 * graph unit to warm up.  The state does not advance.  PFEM_ERR_STATE when the loop ended early (zero load and state).      */
int pfem_dynamics_bench_implicit(pfem_solver *s, int scheme, double dt, double p0, double p1, int iterations, double *us_per_iteration);
/* Y = K X by the block product of pfem_modal_solve (k_spmm<mb> on the row form; mb = 4, 8 or 16): x and y are host blocks of
 * n_local x mb doubles, row-major (the mb values of a dof contiguous), in the caller's dof order.  One rank, an assembled
 * matrix (PFEM_ERR_STATE); writes no state of the handle.                                                                     */
int pfem_modal_spmm(pfem_solver *s, int mb, const double *x, double *y);
/* One launch of a kernel of pfem_modal_solve on blocks of the caller's, through the grid function and the launch code of the
 * solve itself: what the tests compare with an exact or extended-precision evaluation at row counts beyond one pass of the
 * capped grids.  Every block is a host array of n x mb doubles, row-major, in plain row order (rows of a block, not dofs: no
 * renumbering applies); m and dinv hold n doubles; n >= 1, mb = 4, 8 or 16 (PFEM_ERR_ARG).  An initialised handle is all they
 * need -- no mesh, pattern or mass -- and they write no state of it.  On the device every block is followed by one tile of rows
 * of quiet NaNs: a read behind row n poisons the sums, and a write there is found after the launch -- PFEM_ERR_HIP, with the
 * block's name in pfem_last_error_string.
 *   gram:     k_modal_gram<mb> on its grid for n rows, then k_modal_sum; out: the 2 NS NS doubles (NS = 3 mb) of S^T K S and
 *             S^T (m o S), S = [X W P], as the solve's Rayleigh-Ritz step reads them (upper block triangles, zeros below).
 *   residual: k_modal_residual<mb> on its grid for n mb entries, then k_modal_sum; W_out = dinv o (KX - (m o X) diag(theta))
 *             (dinv == NULL: without dinv), norms_out: the 3 mb sums ||R_j||^2, ||KX_j||^2, ||m o X_j||^2.  theta: mb doubles.
 *   update:   k_modal_update<mb> on its grid for n rows with coef = C (3 mb x mb, row-major: rows of X, of W, of P); X, P, KX
 *             and KP come back updated, W and KW as they stood on the device after the launch.                              */
int pfem_modal_probe_gram(pfem_solver *s, int mb, int64_t n, const double *X, const double *W, const double *P, const double *KX,
                          const double *KW, const double *KP, const double *m, double *out);
int pfem_modal_probe_residual(pfem_solver *s, int mb, int64_t n, const double *KX, const double *X, const double *m, const double *dinv,
                              const double *theta, double *W_out, double *norms_out);
int pfem_modal_probe_update(pfem_solver *s, int mb, int64_t n, const double *coef, double *X, double *W, double *P, double *KX,
                            double *KW, double *KP);
/* One launch of a kernel of the steppers (pfem_dynamics_run_implicit, pfem_dynamics_run) on vectors of the caller's, through the
 * grid function, the parameter block and the launch code of the run itself: what the tests compare with an exact or an
 * extended-precision evaluation at row counts beyond one trip of the capped grid (2 048 blocks of 1 024 rows).  Every vector is
 * a host array of n >= 1 doubles in plain row order.  An initialised handle is all they need, and they read and write no state
 * of it.  On the device every vector is an allocation of its own with 8 quiet NaNs in front and 1 024 behind; outputs start as
 * quiet NaNs throughout.  After the launch the guards must hold their bits and so must every vector the kernel takes as const:
 * else PFEM_ERR_HIP with the vector's name in pfem_last_error_string.  scheme, dt, p0, p1, alpha: as pfem_dynamics_run_implicit
 * takes them (PFEM_ERR_ARG likewise); the curve as pfem_dynamics_set_load_curve (n_curve = 0: none).  Partial arrays that come
 * back hold 2 048 doubles, those behind the launch's gv (or nb) blocks still NaN; partial arrays that go in hold exactly
 * gv = min(2 048, ceil(n / 1 024)) doubles (PFEM_ERR_ARG otherwise).
 *   predict:   k_imp_predict: ut, vt from u, v, a.
 *   rhs:       k_imp_rhs with the times and weights of step `step` from t_base, then k_cg_start with rtol, abstol, dtol: d, r,
 *              p, the partials of (r,z), (z,z), sigma m p^2, their count *gv and the control block.  vt: Newmark only.
 *   update:    k_imp_update on the control block *ctl (in and out) with it_arg >= 0 or -1 (the graph's form: ctl->its), the
 *              n_pw partials of (p,Kp) and the n_mp = gv of sigma m p^2: r in place, the partials of (r,z) and (z,z).
 *   direction: k_imp_direction on *ctl (in and out; it_arg = -1: ctl->its_dir) and the n_parts = gv partials of (r,z), (z,z):
 *              p and d in place, the partials of sigma m p^2.
 *   correct:   k_imp_correct: Newmark u, v, a from ut, vt, d; theta-method u in place and v from d (a stays NaN; ut, vt unused).
 *   energy:    k_imp_energy, then k_imp_row at time t: row = [t, T, S, W, u at the probes, v at the probes] (4 + 2 n_probe
 *              doubles; probe: rows in [0, n)), part = the [3][gv] partials (3 x 2 048 doubles of room).
 *   step:      k_dyn_step for step -> step + 1 of a run that began at state run_start <= step, the step index as an argument
 *              (use_ctl = 0) or from the control block (ctl_step[step & 1]); then, after a sampled step, k_dyn_flush.
 *              ctl_step[2] goes in and comes back; un; *have_row and row (4 + 2 n_probe doubles) of a sampled step; part: the
 *              [3][*nb] partials of parity step & 1 (room for 3 ceil(n / 1 024)), NaN after a step that is not sampled.       */
typedef struct pfem_cg_ctl {
    double beta[2], rn0, ttol, rn, dtol, alpha;
    int flag, its, its_dir;
} pfem_cg_ctl;
int pfem_imp_probe_predict(pfem_solver *s, int64_t n, double dt, double beta, double gamma, const double *u, const double *v, const double *a,
                           double *ut, double *vt);
int pfem_imp_probe_rhs(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, int n_curve, const double *ct,
                       const double *cl, double t_base, int64_t step, double rtol, double abstol, double dtol, const double *f, const double *m,
                       const double *vt, const double *w, const double *dinv, double *d, double *r, double *p, double *part_rz, double *part_zz,
                       double *part_mp, int *gv, pfem_cg_ctl *ctl);
int pfem_imp_probe_update(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, pfem_cg_ctl *ctl, int it_arg,
                          int n_pw, const double *part_pw, int n_mp, const double *part_mp, const double *p, const double *w, const double *m,
                          const double *dinv, double *r, double *part_rz, double *part_zz);
int pfem_imp_probe_direction(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, pfem_cg_ctl *ctl, int it_arg,
                             int n_parts, const double *part_rz, const double *part_zz, const double *r, const double *dinv, const double *m,
                             double *p, double *d, int maxits, double *part_mp);
int pfem_imp_probe_correct(pfem_solver *s, int scheme, int64_t n, double dt, double p0, double p1, double alpha, const double *ut, const double *vt,
                           const double *d, double *u, double *v, double *a);
int pfem_imp_probe_energy(pfem_solver *s, int scheme, int64_t n, const double *f, const double *m, const double *u, const double *v, const double *w,
                          int n_probe, const int32_t *probe, double t, double *row, double *part, int *gv);
int pfem_dyn_probe_step(pfem_solver *s, int64_t n, double dt, double alpha, double t0, int n_curve, const double *ct, const double *cl,
                        int64_t step, int64_t run_start, int64_t sample_every, int n_probe, const int32_t *probe, int use_ctl,
                        const double *f, const double *m, const double *minv, const double *w, const double *u, const double *up, double *un,
                        double *row, int *have_row, double *part, int *nb, int64_t *ctl_step);
/* *in_effect = 1 when the mesh on the device is held under the internal renumbering (a numbering without locality from 4 096
 * owned dofs, or PFEM_REORDER=1 at the upload), else 0: the tests of the translations assert it.                            */
int pfem_solver_reordered(pfem_solver *s, int *in_effect);
/* the preconditioner T the last pfem_modal_solve on this handle ran with: PFEM_PC_JACOBI or PFEM_PC_GAMG.  PFEM_ERR_STATE before
 * the first run on the current pattern.                                                                                        */
int pfem_modal_last_pc(pfem_solver *s, int *pc);
/* microseconds of one k_spmm<mb> launch and of mb launches of the SpMV form in effect (what the block product replaces): `reps`
 * of each between two HIP events, each series after one warm-up launch, on the same handle.  Like pfem_bench_spmv it uses the
 * solve's SpMV input and output vectors.                                                                                      */
int pfem_modal_bench_spmm(pfem_solver *s, int mb, int reps, double *us_spmm, double *us_mb_spmv);
/* One launch of a kernel of pfem_buckling_solve on blocks of the caller's, through the grid functions and the launch code of the
 * solve itself; blocks, n, mb, the NaN guards and the errors as the pfem_modal_probe_* above.  GX, GW, GP are the K_g-products.
 *   gram:     k_buck_gram<mb>, then k_modal_sum; out: the 2 NS NS doubles (NS = 3 mb) of S^T (K_g S) and S^T (K S), S = [X W P]
 *             (upper block triangles, zeros below).
 *   residual: k_buck_residual<mb>, then k_modal_sum; W_out = dinv o (GX - KX diag(theta)) (dinv == NULL: without dinv),
 *             norms_out: the 3 mb sums ||R_j||^2, ||GX_j||^2, ||KX_j||^2.  theta: mb doubles.
 *   update:   k_buck_update<mb> with coef = C (3 mb x mb, row-major: rows of X, of W, of P); X, P, KX, KP, GX and GP come back
 *             updated, W, KW and GW as they stood on the device after the launch.                                            */
int pfem_buck_probe_gram(pfem_solver *s, int mb, int64_t n, const double *X, const double *W, const double *P, const double *KX,
                         const double *KW, const double *KP, const double *GX, const double *GW, const double *GP, double *out);
int pfem_buck_probe_residual(pfem_solver *s, int mb, int64_t n, const double *GX, const double *KX, const double *dinv, const double *theta,
                             double *W_out, double *norms_out);
int pfem_buck_probe_update(pfem_solver *s, int mb, int64_t n, const double *coef, double *X, double *W, double *P, double *KX, double *KW,
                           double *KP, double *GX, double *GW, double *GP);
/* the preconditioner T the last pfem_buckling_solve on this handle ran with: PFEM_PC_JACOBI or PFEM_PC_GAMG.  PFEM_ERR_STATE
 * before the first run on the current set-up.                                                                                */
int pfem_buckling_last_pc(pfem_solver *s, int *pc);
/* microseconds of one launch of k_buck_gram<mb> (+ k_modal_sum), k_buck_update<mb>, k_modal_gram<mb> (+ k_modal_sum) and
 * k_modal_update<mb> on blocks of n rows of the call's own (hashed values), `reps` of each between two HIP events after one
 * warm-up launch: us[4] in that order.  An initialised handle is all it needs.  (tools/lab/buckling_measure.py)              */
int pfem_buckling_bench_kernels(pfem_solver *s, int mb, int64_t n, int reps, double *us);
/* kernel time [ms] of the last pfem_buckling_setup (HIP events around the stress pass, the zeroing and k_geo_assemble)       */
int pfem_buckling_setup_ms(pfem_solver *s, double *ms);
/* One launch of a kernel of pfem_solver_solve_multi on panels of the caller's, through the grid functions and the launch code of
 * the solve itself.  An initialised handle is all they need.  Panels are host arrays of n x mb doubles in
 * plain row order, mb = 4 or 8; dinv: n doubles, or NULL for the form the solve launches under gamg.  Every device block has NaN
 * guard tiles (see the pfem_modal_probe_* above); a block a kernel takes as const is compared with what went up.  pfem_mcg_ctl is
 * the device's control block as a plain struct: per column (8 places, mb of them used) beta[2], rn0, ttol, rn, alpha, bb, flag,
 * its and the verdict of the current step (0 idle, 1 goes on, 2 last step, 3 breakdown); the running count; the step counter.
 * Partials of the vector kernels: part[block][2][mb] -- (r,z), then (z,z) -- for *gv blocks (room for 1 024 x 2 mb doubles).
 *   init:      k_mcg_init<mb>: X = 0, R = B, and with dinv P = dinv o R and the partials (without: P and part come back NaN).
 *   start:     k_mcg_start (one block) on nparts rows of partials: *ctl is written throughout.
 *   fold:      k_mcg_fold<mb>: nb rows of mb product partials to fold_out[32][mb].
 *   update:    k_mcg_update<mb> on *ctl (in and out) and the folded product partials fold_pw[32][mb]: R in place, the partials
 *              (dinv == NULL: none, part_out comes back NaN).
 *   dots:      k_mcg_dots<mb>: the partials from R and Z; ctl == NULL: every column; fold_pw == NULL: no breakdown marker.
 *   verdict:   k_mcg_verdict (one block) on *ctl (in and out) and nparts rows of partials.
 *   direction: k_mcg_direction<mb> on *ctl: P and X in place; Z (dinv == NULL) is the stored T R.
 * pfem_multi_spmm_dot: k_spmm_dot<mb>, then k_mcg_fold, on the handle's assembled matrix like pfem_modal_spmm: W = K P in the
 * caller's dof order and pw_out[mb] = the folded (p, Kp) summed in index order, as k_mcg_update reads them.                   */
typedef struct pfem_mcg_ctl {
    double beta[8][2], rn0[8], ttol[8], rn[8], alpha[8], bb[8];
    int flag[8], its[8], verdict[8], running, step;
} pfem_mcg_ctl;
int pfem_multi_probe_init(pfem_solver *s, int mb, int64_t n, const double *B, const double *dinv, double *X_out, double *R_out, double *P_out,
                          double *part_out, int *gv);
int pfem_multi_probe_start(pfem_solver *s, int mb, int nparts, const double *part, double rtol, double abstol, pfem_mcg_ctl *ctl);
int pfem_multi_probe_fold(pfem_solver *s, int mb, int nb, const double *part_pw, double *fold_out);
int pfem_multi_probe_update(pfem_solver *s, int mb, int64_t n, pfem_mcg_ctl *ctl, const double *fold_pw, const double *W, const double *dinv,
                            double *R, double *part_out, int *gv);
int pfem_multi_probe_dots(pfem_solver *s, int mb, int64_t n, const pfem_mcg_ctl *ctl, const double *fold_pw, const double *R, const double *Z,
                          double *part_out, int *gv);
int pfem_multi_probe_verdict(pfem_solver *s, int mb, pfem_mcg_ctl *ctl, int nparts, const double *part, double dtol, int maxits);
int pfem_multi_probe_direction(pfem_solver *s, int mb, int64_t n, pfem_mcg_ctl *ctl, const double *R, const double *dinv, const double *Z,
                               double *P, double *X);
int pfem_multi_spmm_dot(pfem_solver *s, int mb, const double *P, double *W_out, double *pw_out);
/* the preconditioner T the last pfem_solver_solve_multi on this handle ran with: PFEM_PC_JACOBI or PFEM_PC_GAMG.  PFEM_ERR_STATE
 * before the first call on the current pattern.                                                                               */
int pfem_multi_last_pc(pfem_solver *s, int *pc);
/* device time [ms] of `reps` multi solves of the assembled right-hand side scaled by j + 1 (column j), between two HIP events per
 * panel -- after the panel's upload, after the last copy of its control block -- summed over the panels: ms[reps]; its[nrhs] of
 * the last one.  Arguments and preconditions as pfem_solver_solve_multi.  (tools/lab/multirhs_measure.py)                   */
int pfem_multi_bench(pfem_solver *s, int nrhs, int reps, int pc, double *ms, int *its);

/* Timings of the last calls, measured with HIP events on the solver's stream [ms]. */
typedef struct pfem_timings {
    double pattern_ms;      /* pfem_pattern_build                                  */
    double assemble_ms;     /* pfem_assemble (reference timer :826 -> :893)        */
    double solve_ms;        /* pfem_solver_solve (reference timer :898 -> :902)    */
    double spmv_ms_total;   /* sum of the SpMV launches inside the last solve      */
    int64_t spmv_launches;  /* number of SpMV launches inside the last solve       */
    double upload_ms;       /* pfem_mesh_upload (PCIe, host wall clock)            */
    double event_overhead_ms; /* what a start/stop event pair reports for an EMPTY kernel (marker-to-
                               * dispatch gap of the measurement itself, calibrated at solve start);
                               * kernel time per SpMV = spmv_ms_total/spmv_launches - event_overhead_ms */
    double iface_ms_total;  /* multi-rank, sampled with the SpMV: pack + neighbour exchange, time on the comm stream ... */
    double scalar_ms_total; /* ... and the two scalar all-reduces of the iteration, time on the comm stream           */
    int64_t comm_samples;   /* number of iterations both were sampled in                                             */
    double exposed_ms_total;/* of those: time the compute stream spent WAITING for the comm stream (not hidden by the
                             * interior SpMV), per sampled iteration                                                 */
    int64_t graph_iterations; /* iterations of the last solve that were replayed from a hipGraph                       */
    double host_enqueue_ms;   /* host time spent enqueueing the iterations of the last solve (without the per-chunk     */
    int64_t host_enqueued_iterations; /* wait for the control block) and the number of iterations enqueued;            */
    double host_comm_ms;      /* of it: time inside the communication backend's calls (RCCL launch cost)              */
} pfem_timings;
int pfem_get_timings(pfem_solver *s, pfem_timings *t);
/* record an event pair around every SpMV launch of the next solves (bench.py) */
int pfem_solver_profile_spmv(pfem_solver *s, int enable);   /* 0 off, 1 every launch, k > 1 every k-th launch */

/* Transport self-test (collective, no mesh needed): stamped buffers of `count` doubles to every other rank (to itself
 * when there is one rank) through the backend's exchange, then an all-reduce of a known vector; *bad = wrong entries. */
int pfem_solver_comm_selftest(pfem_solver *s, int64_t count, int64_t *bad);
/* Transport timing (collective, no mesh needed): `reps` back-to-back exchanges of `count` doubles with every other rank (with
 * itself when there is one rank), then `reps` all-reduces of 4 doubles, each series between two events on the solver's stream
 * (for the host backend the time includes its staging); milliseconds per call.                                           */
int pfem_solver_comm_bench(pfem_solver *s, int64_t count, int reps, double *ms_per_exchange, double *ms_per_allreduce);
/* The same with the sizes of a run in hand: exchanges of `count` doubles (62 KB = 7 803: a face of config 4; 1.29 MB = 160 801:
 * a face of config 5) with every other rank, or (slab_neighbours != 0) with rank - 1 and rank + 1 only, what a slab partition
 * exchanges; all-reduces of `allreduce_count` doubles (3: the CG's scalars; 125 000: the right-hand side of a replicated
 * multigrid level).  bench.py prints these for N > 1 so that the one 8-GPU run shows what the links cost. */
int pfem_solver_comm_bench_sizes(pfem_solver *s, int64_t count, int64_t allreduce_count, int reps, int slab_neighbours,
                                 double *ms_per_exchange, double *ms_per_allreduce);
/* what the last solve exchanged per iteration: number of neighbours, doubles sent to all of them together, and
 * how many of the SpMV's slices hold shared rows (they run first) out of how many                                  */
int pfem_solver_comm_info(pfem_solver *s, int *n_peers, int64_t *doubles_per_exchange, int64_t *boundary_slices,
                          int64_t *total_slices);
/* What carries the multi-rank solve, as the transport reports it (replaces what `-log_view` / MPI_Comm_size would tell a
 * PETSc user, solverpetsc.F:447-476): backend name ("rccl", "host", "peer-ipc", "none"), ncclCommCount / ncclCommCuDevice /
 * ncclGetVersion of the bound communicators (-1 for host hooks), the device the solver runs on, and the form of the
 * multi-rank SpMV all ranks agreed on for the current plan (0 in order, 1 overlapped, -1 before the first solve).     */
int pfem_solver_comm_describe(pfem_solver *s, char *backend, int backend_len, int *backend_ranks, int *backend_device,
                              int *backend_version, int *solver_device, int *overlapped_form);

#ifdef __cplusplus
}
#endif
#endif /* PFEM_AMD_DIAG_H */

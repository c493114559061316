/*
 * pfem_amd.h -- C ABI of the MI355X-native implicit-FEM hot path that replaces, for
 * PFEMFort's drivers, the per-element stiffness routines, the PETSc Mat/Vec assembly
 * calls and Module_SolverPetsc's KSP solve.
 *
 * Every entry point is extern "C", takes plain pointers and sizes, returns an int
 * error code (PFEM_OK == 0) and never throws, exits or STOPs: the Fortran wrappers
 *  print and STOP on a nonzero code exactly where the reference
 * STOPs / CHKERRQs.  The caller owns all host arrays; the library owns all device
 * memory behind the opaque pfem_solver handle.  A handle is not thread-safe; use
 * one handle per process (= per GPU), as the reference uses one PetscSolver per rank.
 *
 * Citations are file:line of the reference (chennachaos/PFEMFort) interface that
 * each entry point replaces.
 *
 * Array conventions are those of the Fortran drivers (column-major == SoA):
 *   coords(nNode,ndim)         -> xyz  [d*nNode + n]
 *   elemNodeConn(nElem,npElem) -> conn [i*nElem + e]   0-based node ids
 *   ElemDofArray(nElem,nsize)  -> edof [i*nElem + e]   0-based GLOBAL dof ids, -1 = Dirichlet
 *   Klocal(nsize,nsize)        -> K[i + nsize*j]       column-major
 */
#ifndef PFEM_AMD_H
#define PFEM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFEM_VERSION 100

/* ---- error codes -------------------------------------------------------- */
#define PFEM_OK 0
#define PFEM_ERR_ARG 1        /* bad argument                                        */
#define PFEM_ERR_STATE 2      /* call out of order (currentStatus, solverpetsc.F:415,441) */
#define PFEM_ERR_NEG_JAC 3    /* STOP " Negative Jacobian ..." elementutilitiespoisson.F:157 */
#define PFEM_ERR_HIP 4        /* a HIP runtime call failed (pfem_last_error_string)  */
#define PFEM_ERR_NOGPU 5      /* no gfx950 device visible: the product has no CPU path */
#define PFEM_ERR_NOMEM 6
#define PFEM_ERR_DIVERGED 7   /* KSPConvergedReason < 0 (solverpetsc.F:481-483)      */
#define PFEM_ERR_PATTERN 8    /* ADD_VALUES into a slot outside the inserted pattern  */
#define PFEM_ERR_COMM 9       /* the communication backend (RCCL / host hooks) failed */

/* ---- element kinds ------------------------------------------------------ */
#define PFEM_POISSON_TRIA 1        /* StiffnessResidualPoissonLinearTria  elementutilitiespoisson.F:23   */
#define PFEM_POISSON_TET 2         /* StiffnessResidualPoissonLinearTetra elementutilitiespoisson.F:107  */
#define PFEM_ELAST_TET 3           /* StiffnessResidualElasticityLinearTetra elementutilitieselasticity3D.F:248 */
#define PFEM_POISSON_TRIA_INLINE 4 /* inline area*B*B^T of triapoissonserialimpl1.F:573-594             */
#define PFEM_ELAST_TRIA 5          /* StiffnessResidualElasticityLinearTria elementutilitieselasticity2D.F:23 (next row 8f.1) */

/* ---- solver status (solverpetsc.F:64-68) -------------------------------- */
#define PFEM_SOLVER_EMPTY 1
#define PFEM_PATTERN_OK 2
#define PFEM_INIT_OK 3
#define PFEM_ASSEMBLY_OK 4
#define PFEM_FACTORISE_OK 5

/* ---- InsertMode (PETSc INSERT_VALUES / ADD_VALUES) ---------------------- */
#define PFEM_INSERT_VALUES 1
#define PFEM_ADD_VALUES 2

typedef struct pfem_solver pfem_solver;

/* ========================================================================= */
/* 0. library / device                                                        */
/* ========================================================================= */
int pfem_version(void);
const char *pfem_strerror(int code);
const char *pfem_last_error_string(void);
/* number of visible HIP devices (0 without a GPU; never an error) */
int pfem_device_count(int *n);
int pfem_device_info(int device, char *name, int name_len, int *compute_units,
                     int64_t *hbm_bytes, int *clock_khz);
/* free / total device memory right now (hipMemGetInfo): what a mesh of a given size leaves of the 288 GB             */
int pfem_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);

/* ========================================================================= */
/* 1. per-element routines, host, one element per call.                       */
/*    This is the call surface of MODULE ElementUtilitiesPoisson /            */
/*    ElementUtilitiesElasticity3D: the unchanged drivers call them once per  */
/*    element and read Klocal back on the host for the Dirichlet lifting      */
/*    (tetrapoissonparallelimpl1.F:841-870), so by construction they are host */
/*    functions.  They share one source (csrc/pfem_elem.hpp) with the device  */
/*    kernels used by pfem_assemble().                                        */
/* ========================================================================= */
/* elementutilitiespoisson.F:23-101 */
int pfem_poisson_tria_ke(const double xNode[3], const double yNode[3],
                         const double *elemData /*kx,ky*/, const double *timeData /*(2)=af*/,
                         const double valC[3], double K[9], double F[3]);
/* elementutilitiespoisson.F:107-193 */
int pfem_poisson_tet_ke(const double xNode[4], const double yNode[4], const double zNode[4],
                        const double *elemData /*kx,ky,kz*/, const double *timeData,
                        const double valC[4], double K[16], double F[4]);
/* elementutilitieselasticity3D.F:248-393 (intended semantics, DESIGN.md "deviations") */
int pfem_elast_tet_ke(const double xNode[4], const double yNode[4], const double zNode[4],
                      const double *elemData /*E,nu,thick,bx,by,bz*/, const double *timeData,
                      const double valC[12], double K[144], double F[12]);

/* elementutilitieselasticity2D.F:23-153: plane stress, D(3,3) = b1(1-nu) as in the reference */
int pfem_elast_tria_ke(const double xNode[3], const double yNode[3],
                       const double *elemData /*E,nu,thick,bx,by*/, const double *timeData,
                       const double valC[6], double K[36], double F[6]);

/* Post-processing of one element from its nodal values valC[nsize] -- the grad u -> strain -> stress -> B^T sigma chain of
 * ResidualElasticityLinearTetra (elementutilitieselasticity3D.F:575-723) and the residual halves of the StiffnessResidual...
 * routines, consistent with the Klocal of the routines above (DESIGN.md "Post-processing"):
 *   grad[ng]   Poisson: grad u (ng = 2 tria, 3 tet).  Elasticity: strain, Voigt order of the B matrix with ENGINEERING shear:
 *              [xx,yy,zz,gxy,gyz,gzx] (ng = 6) for the tet, [xx,yy,gxy] (ng = 3) for the triangle
 *   flux[ng]   Poisson: q = -(kx,ky,kz) o grad u (PFEM_POISSON_TRIA_INLINE: k = 1).  Elasticity: sigma = D strain with the D of
 *              the stiffness routine; the plane-stress D(3,3) = b1(1-nu) of the reference is kept, so the 2-D
 *              shear stress carries the reference's factor
 *   scalar     Poisson: |q|_2.  Elasticity: von Mises (plane stress: sqrt(sxx^2 - sxx syy + syy^2 + 3 txy^2))
 *   fint[nsize] dvol B^T sigma (Poisson: dvol grad N . (k o grad u)) = Klocal valC to rounding, Klocal at af = 1
 * kind = PFEM_POISSON_TRIA ... PFEM_ELAST_TRIA, elemData as for the kind's stiffness routine (not read for the inline
 * triangle); zNode may be NULL in 2-D; any output may be NULL.  PFEM_ERR_NEG_JAC for an inverted element.                 */
int pfem_elem_post(int kind, const double *xNode, const double *yNode, const double *zNode /* NULL in 2-D */,
                   const double *elemData, const double *valC, double *grad, double *flux, double *scalar, double *fint);
/* The scalar of pfem_elem_post evaluated on ANY flux / stress vector flux[ng] of the kind, in its stored Voigt order (the
 * recovered nodal values of pfem_post_nodal_recovery): |q|_2, von Mises, the plane-stress form above.                        */
int pfem_post_scalar(int kind, const double *flux, double *scalar);
/* One element's share of the Zienkiewicz-Zhu indicator.  nodal_flux[a*ng + c]: recovered values at the element's nodes; with
 * f = flux and V = dvol of pfem_elem_post (volume; area; area x thickness for PFEM_ELAST_TRIA), d_ac = nodal_flux[a*ng+c] - f_c
 * and d the space dimension
 *   eta2       = V / ((d+1)(d+2)) sum_c [ sum_a d_ac^2 + (sum_a d_ac)^2 ]   -- the exact integral of |sigma* - sigma_h|^2 over the
 *                simplex, sigma* interpolated linearly from the nodes (P1 mass matrix V (1 + delta_ab) / ((d+1)(d+2)))
 *   flux_norm2 = V sum_c f_c^2
 * plain Euclidean sums over the ng stored components.  Either output may be NULL.  PFEM_ERR_NEG_JAC for an inverted element.  */
int pfem_elem_recovery_error(int kind, const double *xNode, const double *yNode, const double *zNode, const double *elemData,
                             const double *valC, const double *nodal_flux, double *eta2, double *flux_norm2);

/* ---- loads on a side of an element -------------------------------------- */
/* Side f of an element is the face (tets, f = 0..3) or edge (triangles, f = 0..2) OPPOSITE local node f; its nodes are the
 * element's other local nodes in ascending local order.  The reference has nothing of the kind: its surface loads arrive
 * integrated by hand as nodal forces (cookmembranetria32-ForceBC.dat is a traction of 6.25 on the edge x = 48).
 *   PFEM_LOAD_FLUX      the Poisson kinds, 1 component: g = (k grad u).n, the normal flux INTO the body (= -q.n with the q of
 *                       pfem_elem_post); adds the integral of N_a g to the row of node a
 *   PFEM_LOAD_TRACTION  the elasticity kinds, ndof components: force per unit area (per unit length and thickness in 2-D)
 *   PFEM_LOAD_PRESSURE  the elasticity kinds, 1 component: the traction -p n, n the outward unit normal                       */
#define PFEM_LOAD_FLUX 1
#define PFEM_LOAD_TRACTION 2
#define PFEM_LOAD_PRESSURE 3
/* One side of one element: measure (area of the face / length of the edge), unit normal[ndim] pointing away from local node
 * `side` -- decided from that node's position, never from the order of the nodes -- and the consistent nodal load F[nsize] of
 * values[a*ncomp + c], a over the side's nodes in ascending local order, taken as linear on the side:
 *   3-D  F_a = A/12 (2 g_a + g_b + g_c)        2-D  F_a = L thick/6 (2 g_a + g_b)
 * zeros at the dofs of the opposite node.  thick = elemData[2] for PFEM_ELAST_TRIA, 1 otherwise (elemData may then be NULL).
 * Any output may be NULL; with F == NULL load and values are not read.  PFEM_ERR_ARG: side out of range, a load that does not
 * fit the kind.  PFEM_ERR_NEG_JAC: a side of zero measure (or an element so flat that no side of it has an outside).
 * Shares its source (csrc/pfem_elem.hpp) with the kernels of pfem_surface_geometry / pfem_rhs_add_surface_load: same bits.  */
int pfem_face_load(int kind, const double *xNode, const double *yNode, const double *zNode /* NULL in 2-D */,
                   int side, int load, const double *values /* [(npe-1)*ncomp], per side node */,
                   const double *elemData /* thickness, PFEM_ELAST_TRIA only; else may be NULL */,
                   double *F /* [nsize], zero off the side */, double *measure, double *normal /* [ndim] */);

/* ---- thermal strains of one element --------------------------------------- */
/* PFEM_ELAST_TET and PFEM_ELAST_TRIA only (PFEM_ERR_ARG for a Poisson kind).  theta[a] = T_a - T_ref at the element's nodes; the
 * thermal strain is constant over the constant-strain element: e_th = alpha * sum_a N_a theta[a], N the Gauss-point shape values
 * of the kind's stiffness routine, summed over a ascending.  eps_th = e_th [1,1,1,0,0,0] (tet), e_th [1,1,0] (plane stress):
 *   F[nsize]      dvol B^T D eps_th with the D and dvol of the stiffness routine (thickness in the triangle's dvol): with one
 *                 normal stress s = (d11 e_th + d12 e_th) + d12 e_th (tet), d11 e_th + d12 e_th (triangle),
 *                 F[ndof*a + d] = dvol * (dN_a/dx_d * s)
 *   sigma_th[ng]  D eps_th, each row of D in the order pfem_elem_post_thermal evaluates it (rows xx and yy are s; the tet's row
 *                 zz is (d12 e_th + d12 e_th) + d11 e_th), zeros at the shear components: the stress of a fully restrained
 *                 element (valC = 0) is -sigma_th bit for bit
 * Any output may be NULL.  PFEM_ERR_NEG_JAC for an inverted element.  Shares its source (csrc/pfem_elem.hpp) with the kernels
 * of pfem_rhs_add_thermal_load: same bits.                                                                                  */
int pfem_elem_thermal_load(int kind, const double *xNode, const double *yNode, const double *zNode /* NULL in 2-D */,
                           const double *elemData, double alpha, const double *theta /* [npe] */, double *F, double *sigma_th);
/* pfem_elem_post under a thermal state: the normal strains enter D less e_th (flux = D (strain - eps_th)), scalar and fint are
 * formed from that stress (fint = Klocal valC - F of pfem_elem_thermal_load, to rounding), grad stays the total strain B valC.
 * With alpha = 0 or theta = 0 the outputs are pfem_elem_post's bits.  The same kinds and error codes as above.              */
int pfem_elem_post_thermal(int kind, const double *xNode, const double *yNode, const double *zNode /* NULL in 2-D */,
                           const double *elemData, const double *valC, double alpha, const double *theta /* [npe] */,
                           double *grad, double *flux, double *scalar, double *fint);

/* ========================================================================= */
/* 2. driver bookkeeping, host, integer-exact (tetrapoissonparallelimpl1.F)   */
/* ========================================================================= */
/* genTetra.cpp:152-216,247-323,348-525 -- structured box, 6 tets per hex.
 * kz0/kz1 select the hex layers [kz0,kz1) to emit elements for (0,nEz = all);
 * nodes are always the full grid.  bc_mode 0: u=x^2+y^2+z^2 on all six faces
 * (float coordinates, %.8f text round trip); bc_mode 1: clamp the plane y=y0
 * (all ndof dofs, value 0).  Pass NULL output arrays to query *nDBC only.      */
int pfem_gen_box_tets(double x0, double x1, int nEx, double y0, double y1, int nEy,
                      double z0, double z1, int nEz, int kz0, int kz1, int bc_mode,
                      int ndof, double *xyz, int32_t *conn, int64_t *nDBC,
                      int32_t *bc_node, int32_t *bc_dof, double *bc_val);

/* :316-367 + :393-679.  0-based everywhere.  nParts==1 -> identity maps.
 * node_start/node_end/row_start/row_end have nParts entries, ends exclusive.   */
int pfem_dof_numbering(int64_t nNode, int ndof, int64_t nDBC, const int32_t *dbc_node,
                       const int32_t *dbc_dof, const double *dbc_val, int nParts,
                       const int32_t *node_proc_id, int32_t *node_map_get_old,
                       int32_t *node_map_get_new, int32_t *NodeDofArrayNew,
                       double *solnApplied, int64_t *node_start, int64_t *node_end,
                       int64_t *row_start, int64_t *row_end, int64_t *size_global);
/* The renumbering gathers of the driver: elemNodeConn(e,a) = node_map_get_new(elemNodeConn(e,a)) (:659-664)
 * and the coordinate gather through node_map_get_old (:832-838).  conn arrays are SoA [npElem][nElem],
 * xyz arrays SoA [ndim][nNode]; all ids 0-based.  Threaded (the outputs are first touched in parallel). */
int pfem_renumber_mesh(int64_t nNode, int ndim, int64_t nElem, int npElem, const int32_t *conn_old,
                       const double *xyz_old, const int32_t *node_map_get_new,
                       const int32_t *node_map_get_old, int32_t *conn_new, double *xyz_new);
/* :698-713 */
int pfem_elem_dof_array(int64_t nElem, int npElem, int ndof, const int32_t *conn_new,
                        const int32_t *NodeDofArrayNew, int32_t *edof);
/* :722-734 */
int pfem_assy_for_soln(int64_t nNode, int ndof, const int32_t *NodeDofArrayNew,
                       int32_t *assyForSoln);
/* Stand-in for METIS_PartMeshNodal (:464; METIS is a third-party dependency that is
 * not part of the reference tree): deterministic partition of a pfem_gen_box_tets
 * mesh into nParts slabs of hex layers along z; a node belongs to the lowest part
 * among the elements that touch it.  Any other partitioner's
 * (elem_proc_id,node_proc_id) can be fed to pfem_dof_numbering instead.        */
int pfem_partition_box_slabs(int nEx, int nEy, int nEz, int nParts,
                             int32_t *elem_proc_id, int32_t *node_proc_id);
/* the same along any axis (0 x, 1 y, 2 z; -1: the axis with the most hex layers, ties to z) */
int pfem_partition_box_slabs_axis(int nEx, int nEy, int nEz, int axis, int nParts,
                                  int32_t *elem_proc_id, int32_t *node_proc_id);
/* Recursive coordinate bisection of the element centroids (median splits along the longest axis, any nParts): a
 * geometric stand-in for METIS_PartMeshNodal on meshes WITH coordinates; a node goes to the lowest part among the
 * elements touching it.  conn SoA npElem x nElem, 0-based; xyz SoA ndim x nNode.  (A real METIS partition is taken
 * through its files: PFEM_METIS_PREFIX / read_metis_partition.)                                                     */
int pfem_partition_rcb(int64_t nNode, int ndim, const double *xyz, int64_t nElem, int npElem, const int32_t *conn,
                       int nParts, int32_t *elem_proc_id, int32_t *node_proc_id);

/* Mesh ingest, the step before the path: the three/four `.dat` files are whitespace-
 * separated ASCII tables, one record per line (tetrapoissonparallelimpl1.F:216-355).  `shape` counts
 * the non-empty records and the tokens of the first one; `parse` fills out[c*rows + r] (column-major,
 * like the Fortran arrays), OpenMP over records.  Extra tokens on a line are ignored, as a
 * list-directed READ does.                                                                     */
int pfem_text_table_shape(const char *buf, int64_t len, int64_t *rows, int *cols);
int pfem_text_table_parse(const char *buf, int64_t len, int64_t rows, int cols, double *out);

/* Output step after the path: legacy ASCII VTK exactly as MODULE WriterVTK writes it
 * (writervtk.F:33-201: F12.6 reals, I10 ids, CELL_TYPES 5/10, `procid` cell scalars, scalar or vector
 * `solution` point data).  conn is 0-based SoA, soln is [node*ndof+d] by node id.                  */
int pfem_write_vtk(const char *path, int ndim, int64_t nElem, int64_t nNode, int npElem, int ndof,
                   const double *coords, const int32_t *conn, const int32_t *elem_procid,
                   const double *soln);
/* pfem_write_vtk's file with further arrays: n_cell cell arrays after `procid` inside CELL_DATA, n_point point arrays after
 * `solution` inside POINT_DATA.  Array k has *_ncomp[k] components per item, laid out data[i*ncomp + c]:
 *   1: "SCALARS name float 1" + "LOOKUP_TABLE default";  3: "VECTORS name float";  9: "TENSORS name float", three rows of three
 *   per item and a blank line;  any other count: PFEM_ERR_ARG.  Names may not be empty or contain whitespace (PFEM_ERR_ARG).
 * The new arrays are written as %16.8E, one item per line (F12.6 would print a strain of 1e-7 as zero); coords, procid and
 * solution keep the reference's formats.  With n_cell = n_point = 0 the file is pfem_write_vtk's, byte for byte.           */
int pfem_write_vtk_fields(const char *path, int ndim, int64_t nElem, int64_t nNode, int npElem, int ndof,
                          const double *coords, const int32_t *conn, const int32_t *elem_procid, const double *soln,
                          int n_cell, const char *const *cell_name, const int *cell_ncomp, const double *const *cell_data,
                          int n_point, const char *const *point_name, const int *point_ncomp, const double *const *point_data);
/* temp.dat of the drivers: one record per free dof, " ii ind value" (tetrapoissonparallelimpl1.F:935-942) or, with
 * ii = ind = NULL, the value alone (tetraelasticityparallelimpl1.F:1031-1046); values as %.16E.  Formatted on all host
 * threads like pfem_write_vtk.                                                                                      */
int pfem_write_temp_dat(const char *path, int64_t n, const int64_t *ii, const int64_t *ind, const double *val);

/* ========================================================================= */
/* 3. the solver object == TYPE PetscSolver (solverpetsc.F:72-105)            */
/* ========================================================================= */
/* initialise(size_local,size_global,diag_nnz,offdiag_nnz) solverpetsc.F:116-214.
 * row_start = first global row owned by this rank (PETSc derives it from the
 * size_local of the lower ranks; pass 0 on one rank).  diag_nnz/offdiag_nnz are
 * accepted for call compatibility and ignored: the pattern is computed exactly.
 * device < 0 -> current HIP device.  Fails with PFEM_ERR_NOGPU without a GPU.   */
int pfem_solver_create(pfem_solver **s, int64_t size_local, int64_t size_global,
                       int64_t row_start, const int *diag_nnz, const int *offdiag_nnz,
                       int device);
/* free  solverpetsc.F:254-278 */
int pfem_solver_destroy(pfem_solver *s);
/* launch everything on the caller's hipStream_t (e.g. torch's current stream) instead of the
 * solver's own non-blocking stream; a null handle means the legacy default stream */
int pfem_solver_set_stream(pfem_solver *s, void *hip_stream);
/* KSPSetFromOptions / petsc_options.dat stand-in (tetrapoissonparallelimpl1.F:168,
 * solverpetsc.F:198): PETSc defaults are rtol 1e-5, abstol 1e-50, dtol 1e5, maxits 1e4 */
int pfem_solver_set_tolerances(pfem_solver *s, double rtol, double abstol, double dtol, int maxits);
int pfem_solver_status(pfem_solver *s, int *currentStatus);
/* setZero  solverpetsc.F:222-246: finalises the inserted pattern, zeroes values + rhs */
int pfem_solver_set_zero(pfem_solver *s);
/* printInfo solverpetsc.F:286-320 (writes nRow, nnz, storage to stdout) */
int pfem_solver_print_info(pfem_solver *s);

/* MatSetValues(mtx,m,idxm,n,idxn,v,mode) as called at tetrapoissonparallelimpl1.F:798,851:
 * global 0-based indices, negative rows/cols ignored, v read ROW-major (PETSc).
 * INSERT before set_zero records the pattern; ADD after it accumulates on the host
 * staging copy, uploaded by solve (compat path for the unchanged drivers).       */
int pfem_mat_set_values(pfem_solver *s, int m, const int *idxm, int n, const int *idxn,
                        const double *v, int mode);
/* VecSetValues(rhsVec,n,idx,v,mode) :880; negative indices ignored (solverpetsc.F:142) */
int pfem_vec_set_values(pfem_solver *s, int n, const int *idx, const double *v, int mode);
/* assembleMatrix / assembleVector / assembleMatrixAndVector solverpetsc.F:328-401 */
int pfem_solver_assemble_matrix_and_vector(pfem_solver *s, int n, const int *rows,
                                           const int *cols, const double *K /*col-major*/,
                                           const double *F);

/* factorise solverpetsc.F:409-423 (status check only, as in the reference) */
int pfem_solver_factorise(pfem_solver *s);
/* solve solverpetsc.F:431-490: final assembly, zero initial guess, Jacobi-PCG on the GPU.
 * reason follows KSPConvergedReason (2 rtol, 3 atol, -3 its, -4 dtol, -10 indefinite matrix, -8 indefinite PC).
 * Returns PFEM_OK also when reason < 0 ("Divergence." is printed by the caller).   */
int pfem_solver_solve(pfem_solver *s, int *its, int *reason, double *rnorm);
/* factoriseAndSolve solverpetsc.F:498-509 */
int pfem_solver_factorise_and_solve(pfem_solver *s, int *its, int *reason, double *rnorm);
/* VecGetArray on solnVec: the size_local owned entries, device -> host */
int pfem_solver_get_solution(pfem_solver *s, double *x_owned);
/* residual-norm history ||M^-1 r_k||, k = 0..its (up to n entries) */
int pfem_solver_get_history(pfem_solver *s, double *hist, int n, int *n_written);

/* ========================================================================= */
/* 4. batched device path: the element loop of the drivers as ONE call        */
/*    (tetrapoissonparallelimpl1.F:786-884, tetraelasticityparallelimpl1.F:   */
/*    906-965, triapoissonserialimpl1.F:559-650)                              */
/* ========================================================================= */
/* Upload this rank's elements (those with elem_proc_id == rank): connectivity in the
 * NEW numbering, coordinates of all nodes in NEW order, ElemDofArray rows (GLOBAL
 * dof ids; ids outside [row_start,row_start+size_local) become ghost columns/rows
 * of the sub-assembled local matrix), solnApplied by NEW node*ndof+d.            */
int pfem_mesh_upload(pfem_solver *s, int kind, int64_t nElem, const int32_t *conn,
                     int64_t nNode, const double *xyz, const int32_t *edof,
                     const double *solnApplied);
/* Pattern-initialisation loop :786-802 on the device (symbolic phase). */
/* Synthetic configurations without a host mesh (BASELINE configs 2-5): genTetra.cpp's structured box -- node order,
 * "%.8f" coordinates, the 6-tet split of :263-322, Dirichlet data of :505-525 (bc_mode 0: u = x^2+y^2+z^2 on all six
 * faces; 1: the plane y = y0 clamped) -- and the driver's bookkeeping for it (free-dof numbering
 * tetrapoissonparallelimpl1.F:357-367, ElemDofArray :698-713; for nparts > 1 the z-slab partition of
 * pfem_partition_box_slabs, whose renumbering :541-612 is the identity) evaluated ON THE DEVICE for slab `part`.
 * pfem_box_slab_sizes (host, closed forms) gives the sizes to create the solver with; a rank holds the node planes of
 * its own hex layers only.  Replaces pfem_gen_box_tets + pfem_dof_numbering + pfem_renumber_mesh +
 * pfem_elem_dof_array + pfem_mesh_upload for these meshes (bit-identical arrays: tests/test_gpu_parity.py).      */
int pfem_box_slab_sizes(int nEx, int nEy, int nEz, int bc_mode, int ndof, int nparts, int part,
                        int64_t *size_global, int64_t *row_start, int64_t *size_local,
                        int64_t *nNode_local, int64_t *nElem_local);
int pfem_mesh_generate_box(pfem_solver *s, int kind, double x0, double x1, int nEx, double y0, double y1, int nEy,
                           double z0, double z1, int nEz, int bc_mode, int nparts, int part);
/* The same for slabs of hex layers along ANY axis (0 x, 1 y, 2 z; -1: the axis with the most hex layers, ties to z) --
 * what a graph partitioner (METIS_PartMeshNodal, tetraelasticityparallelimpl1.F:522-529) does with a slender body:
 * BASELINE config 4's 50x300x50 beam is cut across its length (37-38 layers per rank on 8 ranks, faces of 51x51 nodes).
 * The reference's renumbering (:541-612: ranks concatenated, ascending old id inside a rank) is no longer the identity
 * for x- or y-slabs; the device evaluates it in closed form, bit-identical to pfem_partition_box_slabs_axis +
 * pfem_dof_numbering + pfem_renumber_mesh + pfem_elem_dof_array on the host (tests/test_gpu_parity.py).
 * axis_used / layer0 / layer1 (may be NULL): the axis taken and the slab's hex layers [layer0, layer1).           */
int pfem_box_slab_sizes_axis(int nEx, int nEy, int nEz, int bc_mode, int ndof, int axis, int nparts, int part,
                             int64_t *size_global, int64_t *row_start, int64_t *size_local,
                             int64_t *nNode_local, int64_t *nElem_local, int *axis_used, int *layer0, int *layer1);
int pfem_mesh_generate_box_axis(pfem_solver *s, int kind, double x0, double x1, int nEx, double y0, double y1, int nEy,
                                double z0, double z1, int nEz, int bc_mode, int axis, int nparts, int part);
/* the mesh as the device holds it; edof in LOCAL numbering (owned rows first, ghosts after); any pointer may be NULL */
int pfem_mesh_download(pfem_solver *s, int32_t *conn, double *xyz, int32_t *edof_local, double *solnApplied);
/* Several materials.  elem_mat[e] in 0 .. n_mat-1 (1 <= n_mat <= 256: one byte per element on the device) names the material
 * of element e, in the order of the conn given to pfem_mesh_upload, or of pfem_gen_box_tets for pfem_mesh_generate_box*.  While
 * a map is set, the elemData argument of pfem_assemble, pfem_eval_elems and the pfem_post_* calls is a TABLE
 * elemData[m * stride + k] and element e takes row elem_mat[e]; stride >= the kind's count of elemData entries (Poisson tet 3,
 * Poisson triangle 2, elastic tet 6, elastic triangle 5).  timeData stays global.  The table is an argument of every call and
 * may change from call to call; the map may not: it is legal after a mesh upload / generate and before pfem_pattern_build
 * (PFEM_ERR_STATE afterwards, and on a handle without a mesh).  elem_mat == NULL or n_mat == 0 clears the map, and so does a
 * new mesh.  PFEM_ERR_ARG: nElem is not the mesh's, an id out of range, n_mat > 256, stride too small, or
 * PFEM_POISSON_TRIA_INLINE (which has no material).  One rank only: pfem_assemble with a map and a communication backend of
 * more than one rank is PFEM_ERR_STATE.  pfem_mesh_get_materials: n_mat = 0 without a map; elem_mat may be NULL. */
int pfem_mesh_set_materials(pfem_solver *s, int64_t nElem, const int32_t *elem_mat, int n_mat, int stride);
int pfem_mesh_get_materials(pfem_solver *s, int *n_mat, int *stride, int32_t *elem_mat);
int pfem_pattern_build(pfem_solver *s);
/* setZero + element loop :817-884 on the device: Ke/Fe, Dirichlet lifting,
 * atomic scatter into the device matrix and rhs.                                */
int pfem_assemble(pfem_solver *s, const double *elemData, const double *timeData);
/* Preconditioner of the CG (PCSetType, solverpetsc.F:206).  JACOBI (default) is the diagonal scaling
 * BASELINE's north_star names.  NODE_BLOCK_JACOBI (PETSc: -pc_type pbjacobi) inverts the
 * diagonal block of every row group of the SpMV (the 1..3 dof rows of a node); it takes effect when the
 * pattern has such groups (3-dof problems) and, on several ranks, when all ranks hold the same groups for
 * the dofs they share (voted at the start of a solve; blocks of shared nodes are summed over the ranks),
 * otherwise JACOBI stays in effect -- pfem_solver_get_preconditioner reports which one the last solve
 * used / the next one will try. */
#define PFEM_PC_JACOBI 0
#define PFEM_PC_NODE_BLOCK_JACOBI 1
/* GAMG (PETSc: -pc_type gamg, reachable from the reference through KSPSetFromOptions / petsc_options.dat,
 * solverpetsc.F:191-206): aggregation algebraic multigrid, one V(1,1) cycle per CG iteration -- aggregates of up to 8 nodes
 * (on a lattice with strong couplings along its axes: bricks of node positions formed in one step; else three passes of
 * pairing along the lattice's axes, or pairwise matching on the strength graph), Galerkin coarse operators re-summed in
 * every solve, Chebyshev smoothing on D^-1 A with a Gershgorin bound (degree 1 on the assembled matrix, 2 below), dense
 * inverse at the coarsest level.  Coarse space: one vector per dof component (piecewise constant) for scalar problems; the
 * rigid-body modes of every aggregate for displacement problems (pfem_solver_amg_transfer).  The reference's own
 * PCBJACOBI/ILU(0) needs 110 / 1 122 iterations on BASELINE configs 3 / 4 and point Jacobi 370 / 5 207; this needs 12 / 18.
 * Aggregates are formed from the values of the first solve after a pattern build and reused while the pattern lives
 * (-pc_gamg_reuse_interpolation true).  Several ranks: ONE hierarchy across the ranks (what PCGAMG does under MPI) --
 * aggregates stay inside a rank's owned dofs, coarse operators are the global Galerkin products held sub-assembled like the
 * matrix, every level has its own neighbour plan, levels small enough are replicated; with PFEM_AMG_COUPLED=0 (or beyond
 * 52 ranks) block Jacobi over the ranks with one hierarchy per rank on its owned diagonal block as assembled from its own
 * elements (PETSc: -pc_type bjacobi -sub_pc_type gamg).                                                                   */
#define PFEM_PC_GAMG 2
int pfem_solver_set_preconditioner(pfem_solver *s, int pc);
int pfem_solver_get_preconditioner(pfem_solver *s, int *pc_in_effect);
/* -pc_gamg knobs: Chebyshev degree on the coarse levels (1..6, default 2) and on the assembled matrix itself (0 = the same;
 * default 1: there an SpMV is dearest), lmax/lmin of the smoothing interval (until set: 16, and 8 for 3-dof nodes WITHOUT rigid-body modes), scaling of the coarse-grid
 * correction (the over-correction a piecewise-constant coarse space wants; until set: 1.5, and 1.8 for 3-dof nodes without rigid-body modes)   */
int pfem_solver_set_amg_options(pfem_solver *s, int cheb_degree, int fine_degree, double eig_ratio, double coarse_scale);
/* (eig_ratio <= 0 / coarse_scale <= 0: that knob is automatic -- picked per kind of problem at the symbolic phase, and taken from
 * the next solve on also where it was given a value before) */
/* -pc_mg_cycle_type v|w (PETSc's PCMGSetCycleType behind PCGAMG): 1 = V(1,1), 2 = W(1,1) -- every coarse problem above the
 * single-launch tail of the cycle is visited twice, the second time on the residual of the first --, 0 = the default again
 * (V, as in PETSc).  W roughly halves the iterations on aggregates matched on the strength graph and costs more than it saves
 * on this hardware (DESIGN.md has the numbers).  One hierarchy across several ranks always runs the V-cycle.              */
int pfem_solver_set_amg_cycle(pfem_solver *s, int cycle);
/* KSPCGUseSingleReduction / -ksp_cg_single_reduction (PETSc option of the KSPCG the reference creates, solverpetsc.F:187;
 * off by default there and here): the Chronopoulos-Gear form of the same iteration -- s = A z instead of w = A p,
 * (p,Ap) by recurrence -- so that (z,r), (z,s), (z,z) are reduced together: ONE all-reduce per iteration on several
 * ranks instead of two, at the price of two more vectors of traffic per iteration and one more SpMV per solve.  Point
 * Jacobi, and -pc_type gamg with ONE hierarchy across several ranks (two all-reduces per iteration instead of three: the
 * cycle keeps its own); node-block Jacobi and gamg on one rank keep the two-reduction loop.  on = 1 / 0, or -1: the environment variable
 * PFEM_CG_SINGLE_REDUCTION decides (default off).  Same stopping rule and reasons; iterates agree with the default
 * loop to rounding.                                                                                                    */
int pfem_solver_set_cg_single_reduction(pfem_solver *s, int on);
/* Specified nodal forces after the element loop (VecSetValue(rhsVec,row,fact,ADD_VALUES),
 * tetraelasticityparallelimpl1.F:971-982) for the batched path: GLOBAL free-dof ids (i.e.
 * NodeDofArrayNew(n,d)-1; the reference's own row formula ignores constrained dofs);
 * ids this rank does not own and negative ids are skipped.                                      */
int pfem_rhs_add_values(pfem_solver *s, int64_t n, const int64_t *global_dof, const double *values);

/* ---- surface loads -------------------------------------------------------- */
/* Elements are never reordered on the device, so (element, side) -- element in the order of the conn given to pfem_mesh_upload,
 * or of pfem_gen_box_tets for pfem_mesh_generate_box*; side as for pfem_face_load -- names a face for the mesh's whole life.
 * One rank only (PFEM_ERR_STATE with a communication backend of more than one rank: a cut between ranks would look like a
 * boundary) and the batched path only (PFEM_ERR_STATE on a handle without a mesh).
 *
 * pfem_mesh_boundary_faces: the sides that belong to exactly one element, sorted by (element, side).  Two-call: with NULL arrays
 * only *nFace is set.  Needs the mesh only; the same output before and after pfem_pattern_build.  Found on the device: a
 * radix sort of one 64-bit key per side and one thread per side that scans its run of equal keys;
 * temporary device memory (32 npe + 4) nElem bytes plus the sort's own.  The result is kept on the handle until the next mesh.
 * PFEM_ERR_ARG: 2^29 elements or more (element * 4 + side is carried in 32 bits).                                         */
int pfem_mesh_boundary_faces(pfem_solver *s, int64_t *nFace, int32_t *face_elem, int32_t *face_side);
/* measure[i], normal[c*nFace + i] and face_nodes[a*nFace + i] (the side's nodes in ascending local order, in the caller's node
 * numbering) of any sides, boundary or not; one thread per side, pfem_face_load's arithmetic.  Any output may be NULL.
 * PFEM_ERR_ARG: an element or side out of range.  PFEM_ERR_NEG_JAC: a side of zero measure among them.                        */
int pfem_surface_geometry(pfem_solver *s, int64_t nFace, const int32_t *face_elem, const int32_t *face_side,
                          double *measure, double *normal /* [c*nFace + i] */, int32_t *face_nodes /* [a*nFace + i] */);
#define PFEM_LOAD_UNIFORM 0        /* values[ncomp]                                   */
#define PFEM_LOAD_PER_FACE 1       /* values[i*ncomp + c]                              */
#define PFEM_LOAD_PER_FACE_NODE 2  /* values[(i*(npe-1) + a)*ncomp + c]: linear on the side (hydrostatic pressure) */
/* rhs += the consistent nodal loads (pfem_face_load) of the nFace sides, one thread per side, f64 atomics into the rows of the
 * sides' free dofs; constrained dofs are skipped, as the reference skips negative indices.  Semantics of pfem_rhs_add_values:
 * needs the pattern, is called after pfem_assemble (which zeroes the rhs) and before the solve, and again after every later
 * pfem_assemble.  Interior sides are accepted (the normal is the named element's outward one) and a side given twice adds
 * twice.  elemData is read for PFEM_ELAST_TRIA only (the thickness): the vector, or the table while a material map is set,
 * exactly as pfem_assemble takes it.  PFEM_ERR_ARG: an element or side out of range, a load that does not fit the mesh's kind,
 * a bad layout.  PFEM_ERR_STATE: no pattern, more than one rank.  PFEM_ERR_NEG_JAC: a side of zero measure among them (the
 * other sides are added).  Robin terms (they would add to K) and follower loads are not covered.                           */
int pfem_rhs_add_surface_load(pfem_solver *s, int64_t nFace, const int32_t *face_elem, const int32_t *face_side,
                              int load, int layout, const double *values, const double *elemData);

/* ---- post-processing of a solution on the device ------------------------- */
/* u_nodal: host array [node*ndof + d] in the CALLER's node numbering (the one pfem_mesh_upload received, or the generator's own
 * for pfem_mesh_generate_box*), or NULL = the field of the last solve (x at the free dofs, solnApplied at the constrained ones;
 * PFEM_ERR_STATE before a solve).  The internal renumbering never shows.  One rank and the batched path only: PFEM_ERR_STATE
 * on a handle without a mesh (MatSetValues path) and with a communication backend of more than one rank.
 *
 * pfem_post_elements: pfem_elem_post for every element, one thread per element; outputs SoA grad[c*nElem + e],
 * flux[c*nElem + e], scalar[e], any of them NULL.  Needs the mesh only.                                                    */
int pfem_post_elements(pfem_solver *s, const double *elemData, const double *u_nodal,
                       double *grad, double *flux, double *scalar);
/* R[node*ndof + d] = sum over the elements of (K_e u_e - F_e) at EVERY node dof, K_e / F_e exactly those pfem_assemble computes
 * for elemData / timeData: at a free dof of a converged solution the nodal force applied through pfem_rhs_add_values (zero
 * where none was), at a constrained dof the reaction; the sum of R_d over all nodes is -sum F_e whatever u is.  With the gather
 * form of the assembly in effect one thread per node sums its incident elements in ascending element order (no atomics, the
 * same bits in every run; hub nodes by a restricted atomic pass); otherwise one thread per element with f64 atomics.
 * Needs the pattern.                                                                                                       */
int pfem_post_nodal_forces(pfem_solver *s, const double *elemData, const double *timeData,
                           const double *u_nodal, double *R);
#define PFEM_POST_FLUX 0
#define PFEM_POST_GRAD 1
/* Recovery of a nodal field from the piecewise-constant element field by volume-weighted averaging:
 *   nodal[node*ng + c] = sum_e w_e f_c(e) / sum_e w_e over the elements at the node, w_e = dvol of pfem_elem_post (volume; area;
 *   area x thickness for PFEM_ELAST_TRIA), f = flux (field == PFEM_POST_FLUX) or grad (PFEM_POST_GRAD) of pfem_elem_post;
 *   nodal_scalar[node] = pfem_post_scalar of the recovered flux (PFEM_POST_FLUX only, else it must be NULL: PFEM_ERR_ARG);
 *   weight[node] = sum_e w_e.
 * A node without elements gets zeros.  Any output may be NULL.  With the gather form of the assembly in effect one thread per
 * node walks its incident elements in ascending element order (no atomics, the same bits in every run; hub nodes by a
 * restricted atomic pass and a division); otherwise one thread per element with f64 atomics, then the division.  Needs the
 * pattern (the incidence lists).                                                                                           */
int pfem_post_nodal_recovery(pfem_solver *s, const double *elemData, const double *u_nodal, int field,
                             double *nodal, double *nodal_scalar, double *weight);
/* Zienkiewicz-Zhu error indicator: eta2[e] = pfem_elem_recovery_error of every element against the recovered nodal flux (the
 * recovery above runs on the device and its result stays there), and the sums of eta2 and flux_norm2 over all elements
 * (per-block partials in fixed order: reproducible where the recovery is).  Any output may be NULL.                        */
int pfem_post_error_indicator(pfem_solver *s, const double *elemData, const double *u_nodal,
                              double *eta2, double *eta2_total, double *flux_norm2_total);
/* KSPBuildResidual / -ksp_monitor_true_residual: |b - K x|_2 and |b|_2 over the owned rows for the x of the last solve, K x by
 * the SpMV form in effect (pfem_solver_solve's rnorm is |M^-1 r| of the CG recurrence).  PFEM_ERR_STATE before a solve.     */
int pfem_solver_true_residual(pfem_solver *s, double *rnorm2, double *bnorm2);

/* ---- thermal strains: a temperature field that loads an elastic body ------- */
/* PFEM_ELAST_TET and PFEM_ELAST_TRIA (PFEM_ERR_ARG on a handle of a Poisson kind), one rank and the batched path only, like the
 * surface loads.  The state on the handle is theta = T - T_ref per node and the expansion coefficient alpha per material row; it
 * lives until pfem_thermal_clear, the next mesh or the next pfem_pattern_build.  While it is set
 *   pfem_post_elements        returns the stress D (strain - eps_th) and its von Mises (grad stays the total strain),
 *   pfem_post_nodal_forces    returns sum_e (K_e u_e - F_e - F_th,e): the true reactions of a thermally loaded solution,
 *   pfem_post_nodal_recovery (PFEM_POST_FLUX) and pfem_post_error_indicator work on that stress,
 * with u_nodal given or NULL (pfem_elem_post_thermal per element, the element's own alpha row: same bits).  Assembly, the solve,
 * the steppers and the modal solve do not read the state: they see the load below in the assembled right-hand side.
 *
 * pfem_thermal_set: theta_nodal[nNode] in the CALLER's node numbering (kept on the device in the device's node order);
 * alpha[n_alpha], n_alpha = 1 without a material map and n_mat with one (anything else: PFEM_ERR_ARG).  Needs the pattern
 * (PFEM_ERR_STATE before it).  Replaces a state already set.                                                                */
int pfem_thermal_set(pfem_solver *s, int n_alpha, const double *alpha, const double *theta_nodal);
/* The same with theta = (the nodal field of src's last solve) - T_ref, which never visits the host: src is a handle of a one-dof
 * kind with the same nNode (else PFEM_ERR_ARG) on the same device and a solve of its pattern (else PFEM_ERR_STATE); its field is x
 * at the free dofs and solnApplied at the constrained ones, what the post-processing calls take for u_nodal = NULL.  One kernel,
 * one thread per node, carries it from src's device order to dst's through an index map composed on the host; dst's stream
 * waits on an event of src's.  BOTH handles must have been given the same node numbering by the caller: only nNode is checked. */
int pfem_thermal_set_from_solver(pfem_solver *dst, int n_alpha, const double *alpha, pfem_solver *src, double T_ref);
/* n_alpha, alpha[n_alpha] and theta_nodal[nNode] in the caller's numbering; any output may be NULL.  PFEM_ERR_STATE: no state.  */
int pfem_thermal_get(pfem_solver *s, int *n_alpha, double *alpha, double *theta_nodal);
int pfem_thermal_clear(pfem_solver *s);
/* rhs += sum_e F_th,e (pfem_elem_thermal_load) at the free dofs; constrained dofs are skipped.  Semantics of
 * pfem_rhs_add_surface_load: after pfem_assemble (which zeroes the rhs) and before the solve, and again after every later
 * pfem_assemble; elemData is the vector, or the table while a material map is set, exactly as pfem_assemble takes it.  With the
 * gather form of the assembly in effect one thread per node sums its incident elements in ascending element order (no atomics,
 * the same bits in every run) and a pass adds the node sums to the rows of the free dofs; hub nodes, and the scatter form, by an
 * element pass with f64 atomics.  PFEM_ERR_STATE: no pattern, no thermal state, more than one rank.  PFEM_ERR_NEG_JAC: an
 * inverted element among them (the others are added).                                                                      */
int pfem_rhs_add_thermal_load(pfem_solver *s, const double *elemData);

/* ---- explicit dynamics: lumped mass and central-difference steps ----------- */
/* M u'' + alpha M u' + K u = lambda(t) f on the assembled system: K by the SpMV form in effect, f the assembled right-hand side
 * (body force, nodal forces, surface loads and the Dirichlet lift, all scaled together by lambda), M the lumped mass below.  The
 * reference's explicit drivers (tetraelasticityexplicit.F, triaelasticityexplicit.F) are this loop on the host; their Residual*
 * routines differ from their own stiffness routines and are not reproduced: the internal force here is K u.
 * One rank and the batched path only (PFEM_ERR_STATE otherwise).  Vectors per owned dof are in pfem_solver_get_solution's order.
 *
 * pfem_elem_lumped_mass: MassMatrixLinearTria / MassMatrixLinearTetra (elementutilitieselasticity2D.F:283, 3D.F:401) for any
 * kind -- the row sums of the consistent mass at the kind's one Gauss point, ((density * dvol) * N_i) * N_j summed over j
 * ascending, Mlocal[npe * ndof] (a scalar kind gives the wave equation's mass).  dvol and N are the stiffness routine's;
 * density is an argument of its own (the reference reads elemData(3), which is the thickness here); elemData is read for the
 * thickness of PFEM_ELAST_TRIA only and may be NULL otherwise.  PFEM_ERR_ARG: density not positive.                         */
int pfem_elem_lumped_mass(int kind, const double *xNode, const double *yNode, const double *zNode /* NULL in 2-D */,
                          const double *elemData, double density, double *Mlocal);
/* The mass vector on the device.  density[m]: one entry per material row while a map is set, else one entry; elemData as
 * pfem_assemble takes it (read for the thickness of PFEM_ELAST_TRIA; may be NULL for the other kinds without a map).  A node's
 * mass is the sum of its shares of its elements' pfem_elem_lumped_mass in ascending element order (gather form: one thread per
 * node, the same bits in every run; hub nodes and the scatter form: f64 atomics).  total_mass (may be NULL): the sum over ALL
 * nodes.  Needs the pattern and an assembled matrix (PFEM_ERR_STATE); lives until the next pattern build; the state is set to
 * rest at t = 0, lambda = 1, no probes.                                                                                      */
int pfem_dynamics_setup(pfem_solver *s, const double *elemData, const double *density, double *total_mass);
int pfem_dynamics_get_mass(pfem_solver *s, double *mass_owned);
/* dt = 2 / sqrt(max_i sum_j |K_ij| / m_i): a Gershgorin bound on omega_max, so never above the critical step 2 / omega_max   */
int pfem_dynamics_stable_dt(pfem_solver *s, double *dt);
/* u(t0) = u0, u'(t0) = v0 (NULL: zeros).  The start is the standard one, a0 = (lambda(t0) f - K u0) / m and
 * u_{-1} = u0 - dt v0 + dt^2/2 a0, formed at the next pfem_dynamics_run, where dt is known.                                 */
int pfem_dynamics_set_state(pfem_solver *s, double t0, const double *u0, const double *v0);
/* lambda(t): piecewise linear through (t[k], lambda[k]), t strictly ascending, constant outside the table; n = 0: lambda = 1.
 * It scales the assembled right-hand side AS A WHOLE: a nonzero Dirichlet value enters through the lift in that vector and is
 * scaled with the loads.                                                                                                    */
int pfem_dynamics_set_load_curve(pfem_solver *s, int n, const double *t, const double *lambda);
/* dofs whose u and v go into the history rows: GLOBAL free-dof ids as for pfem_rhs_add_values (PFEM_ERR_ARG: not an owned row) */
int pfem_dynamics_set_probes(pfem_solver *s, int n, const int64_t *global_dof);
/* n_steps steps   (1/dt^2 + alpha/2dt) m u_{n+1} = lambda(t_n) f - K u_n + m/dt^2 (2 u_n - u_{n-1}) + alpha m/(2dt) u_{n-1}:
 * two launches a step (the product, the update), replayed from a captured graph of 48 steps with the step counter, t_n,
 * lambda(t_n) and the sampling on the device; nothing waits for the device before the last step.  Every sample_every-th step of
 * THIS run (0: none) writes a row  [t_{n+1}, T, S, W, u_{n+1} at the probes, v_{n+1/2} at the probes]  with
 *   T = 1/2 sum m v_{n+1/2}^2,  S = 1/2 u_{n+1} . K u_n,  W = f . u_{n+1}      (v_{n+1/2} = (u_{n+1} - u_n) / dt)
 * -- T + S is the exact invariant of the undamped, unloaded scheme -- summed in a fixed order (the same bits in every run);
 * history[rows * (4 + 2 n_probe)] is copied back once, after the run; *rows = n_steps / sample_every (history may be NULL when
 * that is 0).  A second run with the same dt continues exactly; another dt needs a new pfem_dynamics_set_state (PFEM_ERR_STATE). */
int pfem_dynamics_run(pfem_solver *s, double dt, int64_t n_steps, double alpha, int64_t sample_every, double *history, int64_t *rows);
/* t_n, n, u_n and v_{n-1/2} (before the first run: u0 and v0 as set; after pfem_dynamics_run_implicit: v_n, at the integer
 * step); any output may be NULL                                                                                            */
int pfem_dynamics_get_state(pfem_solver *s, double *t, int64_t *step, double *u, double *v);

/* ---- implicit time stepping on the lumped mass: Newmark and the theta-method ---- */
/* Unconditionally stable steps on the same K, f, m, load curve, probes and state as above.  With a lumped
 * mass every step is ONE solve with a shifted operator,  (K + sigma diag(m)) d = b,  sigma > 0 a scalar of the step size; nothing
 * is assembled and no matrix value is rewritten.  t_n = t0 + n dt is formed from n.  A row without mass stays put (d = 0).
 *
 * PFEM_SCHEME_NEWMARK (p0 = beta > 0, p1 = gamma >= 1/2; M u'' + alpha M u' + K u = lambda f), in increment form:
 *     ut = u_n + dt v_n + dt^2 (1/2 - beta) a_n,   vt = v_n + dt (1 - gamma) a_n,   sigma = (1 + gamma dt alpha) / (beta dt^2),
 *     b = lambda(t_{n+1}) f - alpha m vt - K ut,   u_{n+1} = ut + d,   a_{n+1} = d / (beta dt^2),   v_{n+1} = vt + gamma dt a_{n+1},
 *   started from a_0 = (lambda(t0) f - alpha m v0 - K u0) / m.
 * PFEM_SCHEME_THETA (p0 = theta in (0, 1], p1 unused; M u' + K u = lambda f; alpha must be 0, the state's v0 is ignored):
 *     sigma = 1 / (theta dt),   b = [theta lambda(t_{n+1}) + (1 - theta) lambda(t_n)] f - K u_n,   u_{n+1} = u_n + d / theta,
 *   and the reported v is (u_{n+1} - u_n) / dt.  For a scalar kind the `density` of pfem_dynamics_setup is then rho c.
 *
 * The solve: the two-reduction KSPCG iteration of pfem_solver_solve from d = 0 with the solver's rtol, abstol, dtol and maxits
 * (||z|| relative to ||z_0||).  Its preconditioner is ALWAYS the point Jacobi of the shifted operator, 1 / (K_ii + sigma m_i),
 * also when the solver's preconditioner is gamg or node-block Jacobi: neither is used or touched.  ||z_0|| <= abstol: zero
 * iterations, d = 0.  A solve that ends with a negative reason stops the run with PFEM_ERR_DIVERGED: the state stays at the last
 * completed step, *steps_done (may be NULL) says how many there were, and their rows and iteration counts are returned.
 * iterations[n_steps] (may be NULL): the CG iterations of every step.
 *
 * Rows as pfem_dynamics_run's, [t_{n+1}, T, S, W, u_{n+1} at the probes, v_{n+1} at the probes], with  S = 1/2 u_{n+1} . K u_{n+1},
 * W = f . u_{n+1}  and  T = 1/2 sum m v_{n+1}^2  (theta-method: 1/2 sum m u_{n+1}^2), summed in a fixed order; a sampled step
 * costs one product more.  *rows (may be NULL): the rows written.
 *
 * The run leaves the solve alone: the solution vector, the solver's inverse diagonal, control block, residual history, last
 * iteration count / reason / norm, timings and CG graphs are not written; its own vectors are allocated at the first call.
 * Afterwards pfem_dynamics_get_state returns (t_n, u_n, v_n) -- v AT the step, not the explicit scheme's v_{n-1/2}.  Implicit runs
 * of one scheme continue from one another, also with another dt or other parameters.  After an explicit run an implicit one
 * needs a new pfem_dynamics_set_state, and the other way round, and so does a Newmark run after a theta run (PFEM_ERR_STATE).
 * Preconditions as pfem_dynamics_run: one rank, the batched path, pfem_dynamics_setup after the pattern build (PFEM_ERR_STATE).
 * PFEM_ERR_ARG, before the device is touched: dt <= 0 or not finite, n_steps < 0, an unknown scheme, parameters out of range.
 * PFEM_ERR_NOGPU without a device.                                                                                           */
#define PFEM_SCHEME_NEWMARK 1      /* p0 = beta, p1 = gamma */
#define PFEM_SCHEME_THETA   2      /* p0 = theta, p1 unused (0) */
int pfem_dynamics_run_implicit(pfem_solver *s, int scheme, double dt, int64_t n_steps, double p0, double p1, double alpha,
                               int64_t sample_every, double *history, int64_t *rows,
                               int32_t *iterations /* n_steps, or NULL */, int64_t *steps_done);

/* ---- modal analysis: the lowest modes of (K, lumped M) --------------------- */
/* The lowest n_modes pairs of  K phi = omega^2 M phi,  M = diag(m) the lumped mass of pfem_dynamics_setup, by LOBPCG (no soft
 * locking) on a block X of MB columns, n x MB row-major on the device:  n_modes <= 2: MB = 4,  <= 6: 8,  <= 12: 16;  `block`
 * (0: that choice) may force a larger one of the three.  tests/modal_reference.py is the scheme in numpy:
 *   start   X0 = x0, or entry (i, j) = (splitmix64(i MB + j) >> 11) 2^-52 - 1 with i the GLOBAL free dof: no generator state,
 *           the same block in every run.  K X0, then one Rayleigh-Ritz on X0 alone.
 *   then    R = K X - (m o X) diag(theta);  res_j = ||R_j|| / (||K X_j|| + |theta_j| ||m o X_j||);  stop when res_j <= tol for
 *           all j < n_modes.  W = T R;  K W in one pass over the matrix for all MB columns;  S = [X W P];  the upper triangles of
 *           S^T K S and S^T (m o S), summed in a fixed order, go to the host;  pfem_dense_sym_geneig gives the lowest MB pairs and
 *           the coefficients C, which come back;  P' = W C_W + P C_P,  X' = X C_X + P',  and the same on K X, K W, K P.
 *           When the Gram matrix of the masses is singular to working precision P is dropped for that iteration (a restart,
 *           counted in *restarts); when it is without P as well, the run ends with reason -2.  Every 10th iteration K X is
 *           formed by a product instead of the recurrence.
 *   T       pc = -1: the solver's preconditioner -- when that is gamg (one rank's own hierarchy) and its numeric set-up is
 *           current, i.e. a gamg solve has run since the last assemble, W's columns are the multigrid cycle of that solve
 *           applied to R's columns one at a time (the cycle and its set-up are used as they stand and left as they are);
 *           otherwise the point Jacobi 1 / K_ii, in the run's own buffer.  pc = PFEM_PC_JACOBI / PFEM_PC_NODE_BLOCK_JACOBI: the
 *           point Jacobi.  pc = PFEM_PC_GAMG: the cycle, or PFEM_ERR_STATE where it is not current.
 *   end     pairs in ascending theta;  phi^T M phi = 1;  the entry of largest magnitude positive (the lowest index on ties);
 *           residuals from an explicit K X.
 * omega2[n_modes];  modes[n_modes x n_owned], mode-major, in pfem_solver_get_solution's order (may be NULL);  residuals[n_modes];
 * *reason: 1 converged, -1 max_iterations, -2 breakdown -- a negative reason still returns the current pairs with PFEM_OK.
 * x0: n_owned x MB row-major in the caller's dof order, or NULL.
 * The run leaves the solve and the steppers alone: it reads the matrix in its row form, m and the diagonal, and writes only its
 * own buffers (under gamg also the cycle's work vectors, which every solve fills before it reads them, and the SpMV's copies of
 * the values, as every product outside a solve) -- not the solution, the right-hand side, the last iteration count / reason /
 * norm, the residual history, the timings, the CG graphs or the state of pfem_dynamics_run / pfem_dynamics_run_implicit.  One
 * stream, no graph; per iteration one device -> host copy (Gram matrices and norms) and one host -> device copy (C, theta), both
 * through pinned buffers.
 * Preconditions as pfem_dynamics_run: one rank, the batched path, pfem_dynamics_setup after the pattern build, an assembled
 * matrix; and every m_i > 0 (PFEM_ERR_STATE).  PFEM_ERR_ARG, before the device is touched: n_modes < 1 or > 12, a block that is
 * not 0 / 4 / 8 / 16 or too small for n_modes, tol <= 0 or not finite, max_iterations < 1, an unknown pc; and MB > n_owned.
 * PFEM_ERR_NOGPU without a device.                                                                                            */
#define PFEM_MODAL_MAX_MODES 12
int pfem_modal_solve(pfem_solver *s, int n_modes, int block /*0: auto*/, double tol, int max_iterations, int pc /*-1: the solver's*/,
                     const double *x0 /* n_owned x MB row-major, or NULL */, double *omega2 /* n_modes */,
                     double *modes /* n_modes x n_owned, mode-major; may be NULL */, double *residuals, int *iterations,
                     int *restarts, int *reason /* 1 converged, -1 max_iterations, -2 breakdown */);
/* Host only, no device, no allocation: A c = w B c for symmetric A, B of order n <= PFEM_GENEIG_MAX (row-major, the upper
 * triangles are read) by scaling with diag(B)^-1/2, a Cholesky factor of the scaled B and cyclic Jacobi rotations on the
 * standard problem.  w[n] ascending, C[i * n + k] = entry i of vector k, C^T B C = I.  *status: 0, or 1 = singular (a diagonal
 * entry of B or a pivot not positive, or a squared pivot of the scaled factor below `floor`): w and C are then not written.
 * PFEM_ERR_ARG: n < 1 or > PFEM_GENEIG_MAX, a NULL pointer, floor negative or not finite.                                      */
#define PFEM_GENEIG_MAX 48
int pfem_dense_sym_geneig(int n, const double *A, const double *B, double floor, double *w, double *C, int *status);

/* ---- linear buckling: geometric stiffness and critical load factors -------- */
/* (K + lambda K_g(sigma_0)) phi = 0 on the free dofs for a reference state with the stress sigma_0 per element (DESIGN.md section
 * 15).  PFEM_ELAST_TET and PFEM_ELAST_TRIA, one rank and the batched path only.  K is SPD, so the problem is posed as
 * K_g phi = theta K phi and the LOWEST theta are sought: lambda = -1 / theta for theta < 0 -- the most negative theta is the
 * smallest positive load factor --, and a pair with theta >= 0 does not buckle in the load's direction: lambda = +infinity.
 *
 * pfem_elem_geometric: the geometric stiffness of one linear simplex couples equal displacement components only,
 *     K_g[(a,i),(b,j)] = delta_ij g_ab,      g_ab = dvol (grad N_a . sigma grad N_b),      Kg[a + npe * b] = g_ab,
 * with dvol and grad N of the kind's stiffness routine (the triangle's thickness elemData[2] in dvol; the tet reads no elemData,
 * which may be NULL there).  sigma in the order pfem_post_elements stores `flux`: [xx,yy,zz,xy,yz,zx] for the tet, [xx,yy,xy] for
 * the triangle -- and for the triangle it is that flux as returned, the reference's plane-stress shear factor included: K_g is
 * built from the stress the library reports.  The triangle's K_g describes in-plane instability only.  The order of operations
 * is fixed (pfem_elem.hpp: elem_geometric) and the device kernel gives the same bits.  PFEM_ERR_ARG: another kind, a NULL
 * pointer.  PFEM_ERR_NEG_JAC: an inverted element.                                                                            */
int pfem_elem_geometric(int kind, const double *xNode, const double *yNode, const double *zNode /* NULL in 2-D */,
                        const double *elemData, const double *sigma, double *Kg /* npe * npe, g[a + npe * b] */);
/* K_g on the device: a second fp64 value array on the pattern and the wave-sliced row form of K.  elem_stress: SoA
 * [c * nElem + e] in the caller's element order, or NULL: the stresses pfem_post_elements would return for u_nodal (NULL: the
 * last solve; a thermal state is honoured, so thermal buckling takes the thermal stress), which never leave the device.
 * elemData is the vector, or the material table while a map is set, exactly as pfem_assemble takes it.  One thread per element
 * adds g_ab with f64 atomics at (row = dof(b,i), col = dof(a,i)) for every component i whose two dofs are free; constrained dofs
 * are dropped (an eigenproblem has no lifting).  The order of the sums therefore varies from run to run.  A new set-up replaces
 * the old one; a re-assemble of K keeps K_g; the next mesh and the next pfem_pattern_build drop it.  PFEM_ERR_ARG: a handle of a
 * Poisson kind, elemData NULL.  PFEM_ERR_STATE: no pattern, no assembled matrix, more than one rank (and, with neither
 * elem_stress nor u_nodal, no solve).  PFEM_ERR_NEG_JAC: an inverted element.                                                */
int pfem_buckling_setup(pfem_solver *s, const double *elemData, const double *u_nodal, const double *elem_stress);
/* K_g's values in pfem_get_csr's layout and order (the same rowptr and cols).  PFEM_ERR_STATE without a set-up.             */
int pfem_buckling_get_geometric(pfem_solver *s, double *vals);
/* The lowest n_modes pairs of K_g phi = theta K phi by the LOBPCG of pfem_modal_solve with m o S replaced by K S and A = K_g:
 * block choice, hashed start block, Rayleigh-Ritz on X0, dropping P when the K-Gram matrix is singular, reasons 1 / -1 / -2, the
 * refresh of the recurrences (K X and K_g X) every 10th iteration, argument errors and PFEM_ERR_NOGPU are that routine's.
 *     R = K_g X - (K X) diag(theta),     res_j = ||R_j|| / (||K_g X_j|| + |theta_j| ||K X_j||).
 * T follows pfem_modal_solve's rule: the cycle of the last gamg solve where that is current, else the point Jacobi of K;
 * pc = PFEM_PC_GAMG without a current set-up: PFEM_ERR_STATE.  (T is an approximate inverse of K: the natural one here.)
 * theta[n_modes] ascending; factor[j] = -1 / theta_j for theta_j < 0, else INFINITY; modes mode-major in
 * pfem_solver_get_solution's order (may be NULL), phi^T K phi = 1 by the final explicit K X, the entry of largest magnitude
 * positive.  Preconditions: pfem_buckling_setup on the current pattern, an assembled matrix, one rank, the batched path.  It reads
 * K's row form, K_g and the diagonal and writes only its own buffers (under gamg also the cycle's work vectors and the SpMV's
 * value copies, as the modal solve): nothing of the solve, the steppers, the modal or the thermal state changes.             */
int pfem_buckling_solve(pfem_solver *s, int n_modes, int block /*0: auto*/, double tol, int max_iterations, int pc /*-1: the solver's*/,
                        const double *x0 /* n_owned x MB row-major, or NULL */, double *theta /* n_modes */, double *factor /* n_modes */,
                        double *modes /* n_modes x n_owned, mode-major; may be NULL */, double *residuals, int *iterations,
                        int *restarts, int *reason /* 1 converged, -1 max_iterations, -2 breakdown */);

/* ---- several load cases in one solve: batched PCG on the block product ----- */
/* K x_j = B_j for nrhs right-hand sides on the assembled K.  Column j is exactly the solve
 * pfem_solver_solve would do with B_j as right-hand side: the two-reduction KSPCG recurrences from x = 0, the norm ||z|| against
 * ttol = max(rtol ||z0||, abstol), the solver's rtol / abstol / dtol / maxits, the reasons 2, 3, -3, -4, -8 and -10 with that
 * routine's meaning and its `its` convention.  A negative reason in some column is not an error of the call (PFEM_OK, as
 * pfem_solver_solve).  A zero column returns reason 3, its = 0 and x = 0 exactly.
 *
 * The columns are independent CG iterations that share one pass over the matrix per iteration (the block product of
 * pfem_modal_solve with the (p, Kp) sums as its epilogue) and nothing else: per-column step lengths, verdicts and iteration
 * counts; no coupled steps, no rank questions -- this is not O'Leary's block CG.  When a column finishes, its x, r and p are
 * never written again; the others go on.  Columns are processed in panels of 4 or 8: nrhs <= 4 takes one panel of 4, otherwise
 * panels of 8 and a last panel of 4 where at most 4 columns remain; the panels run one after the other, padding columns are
 * zero and finish at the start.  A column's bits depend on n and on its panel's width only -- not on its place in the panel or on
 * what the other columns hold -- and every run gives the same bits.
 *
 * B and X are case-major (column j at B + j * n_owned) in pfem_solver_get_solution's order, which is pfem_get_rhs's on one rank:
 * the caller's; the internal renumbering never shows.  A Dirichlet lift is part of a right-hand side: take each B_j from
 * pfem_get_rhs after that case's assemble and loads.
 *
 * T follows pfem_modal_solve's rule.  pc = -1 takes the solver's.  Point Jacobi is 1 / K_ii extracted from the row form into the
 * run's own buffer; PFEM_PC_NODE_BLOCK_JACOBI gets it too.  Where gamg is in effect and its numeric set-up is current -- a gamg
 * solve has run since the last assemble -- T is the cycle of that solve, applied to the columns still running one at a time;
 * pc = PFEM_PC_GAMG without a current set-up: PFEM_ERR_STATE.  Under gamg the cycles run one after the other: the gain is the
 * assembly and the set-up not repeated per case.
 *
 * Preconditions: one rank; a pattern and an assembled matrix whose fp64 row form is current: on the batched path any time after
 * pfem_assemble, on the MatSetValues path only after a solve has uploaded the staged values (PFEM_ERR_STATE before, with a message
 * that says so).  PFEM_ERR_ARG before the device is touched: a NULL pointer, nrhs < 1 or > PFEM_MULTI_MAX_RHS, an unknown pc.  A
 * non-finite entry of B is not checked.  PFEM_ERR_NOGPU without a device.
 *
 * It leaves the solve alone: the solution vector, the right-hand side, last_its / last_reason / last_rnorm, the residual
 * history, the timings, the CG graphs, the status and the states of the steppers, the modal, buckling and thermal paths are not
 * written.  Under gamg it writes what the modal solve writes: the cycle's work vectors and the SpMV's value copies.  Its own
 * state (five panels of n x MB doubles, six under gamg: 320 B a row for a panel of 8) is allocated at the first call, again
 * when n or the panel width changes, and dropped with the pattern.
 *
 * When it pays (measured on one MI355X, DESIGN.md section 16, 30 iterations under the point Jacobi): from 4 columns on the
 * batched solve is ahead of as many single solves -- per column-iteration 0.89 of their time on the 200^3 Poisson box (0.96 for
 * one panel of 4), 0.63 on the 50 x 300 x 50 beam, 0.45 on a jittered box without a value dictionary, 0.27 on a 20^3 box.  For ONE
 * column it loses: the column travels in a panel of 4 and costs what 4 cost, 1.7 to 3.9 x pfem_solver_solve, which is the call
 * for a single right-hand side.                                                                                              */
#define PFEM_MULTI_MAX_RHS 64
int pfem_solver_solve_multi(pfem_solver *s, int nrhs, const double *B /* nrhs x n_owned, case-major */,
                            int pc /* -1: the solver's */, double *X /* nrhs x n_owned, case-major */,
                            int *its /* nrhs */, int *reason /* nrhs */, double *rnorm /* nrhs */);

/* ---- inspection / export (device -> host) -------------------------------- */
/* global dof id of every local row (owned first, then ghosts ascending) */
int pfem_get_local_to_global(pfem_solver *s, int64_t *gid);
/* CSR of the LOCAL (sub-assembled) matrix, local column ids, columns ascending */
int pfem_get_csr(pfem_solver *s, int64_t *rowptr, int32_t *cols, double *vals);
int pfem_get_rhs(pfem_solver *s, double *rhs_local);

/* ========================================================================= */
/* 5. multi-GPU: one process per GPU, sub-assembled interface rows            */
/*    (replaces MatAssembly stash + VecScatter + VecDot MPI_Allreduce inside   */
/*    KSPSolve, solverpetsc.F:447-476)                                        */
/* ========================================================================= */
/* Every rank assembles only its own elements (elem_proc_id == rank, tetrapoissonparallelimpl1.F:829) into a local
 * matrix over owned + ghost rows; rows of dofs that another rank also touches hold partial sums.  Per CG iteration:
 *   1. w = A_loc p on the slices that hold shared rows, then  pack -> NEIGHBOUR exchange  on a second stream while
 *      the interior slices run; every rank adds the partials of a shared dof in ascending rank order (same bits on
 *      all ranks, so the replicated ghost entries of the vectors never drift);
 *   2. two scalar all-reduces: (p, A p) and [(r,z), (z,z)].
 * Who shares which dofs with whom is the NEIGHBOUR PLAN (pure integer host logic):                                */

/* Neighbour plan of `rank`: dof g is shared with rank q when both have it in their local numbering (owned block or
 * ghost list).  Inputs: every rank's owned block [row_start[r], row_end[r]) and ghost list (ascending global ids,
 * concatenated; ghost_off[r]..ghost_off[r+1]).  Two-call: with peers == NULL only *n_peers and *n_total are set.
 * Outputs: peers[] ascending, peer_off[n_peers+1], shared_gid[] = for each peer the ascending global ids shared with
 * it (both sides of a pair compute the same list).  Host only, no GPU needed.                                      */
int pfem_neighbour_plan(int nranks, int rank, const int64_t *row_start, const int64_t *row_end,
                        const int64_t *ghost_off, const int64_t *ghost_gid, int *n_peers, int64_t *n_total,
                        int *peers, int64_t *peer_off, int64_t *shared_gid);
/* install the plan (after pfem_mesh_upload, or after the first setZero of the compat path: the local numbering
 * must exist; and after the communication backend, which tells the solver its rank).  n_peers == 0 is legal (a rank that shares nothing still takes part in the scalar all-reduces).   */
int pfem_solver_set_neighbours(pfem_solver *s, int n_peers, const int *peers, const int64_t *peer_off,
                               const int64_t *shared_gid);
/* Communication backend 1 -- RCCL over xGMI, bound inside the library (librccl is loaded at run time; nothing else
 * needs it): rank 0 creates the unique ids (256 bytes), the host program broadcasts them by whatever means it has
 * (torch.distributed store, MPI_Bcast, a file) and every rank calls pfem_solver_set_comm_rccl.  The exchange is one
 * grouped ncclSend/ncclRecv per neighbour on the solver's communication stream (under the interior SpMV); the
 * reductions are ncclAllReduce on a second communicator, in order on the compute stream.                          */
#define PFEM_RCCL_ID_BYTES 256     /* two ncclUniqueIds: one communicator for the exchange, one for the all-reduces */
int pfem_rccl_unique_id(void *id_out);
int pfem_solver_set_comm_rccl(pfem_solver *s, int rank, int nranks, const void *id);
/* Communication backend 2 -- host hooks, for hosts whose transport works on HOST memory (MPI: the reference's own
 * transport, pfemfort_amd/fortran/pfem_mpi.cpp; gloo in the tests where several ranks share one GPU).  The library
 * stages the packed buffers through pinned host memory and calls:
 *   allreduce(ctx, buf, count)         in-place SUM of `count` doubles; EVERY rank must receive the same bits
 *   exchange(ctx, n_peers, peers, off, send, recv)   send[off[k]..off[k+1]) goes to peers[k], the same range of
 *                                      recv is filled with what peers[k] sent (symmetric counts)
 * Return 0 on success.                                                                                             */
typedef int (*pfem_host_allreduce_fn)(void *ctx, double *buf, int64_t count);
typedef int (*pfem_host_exchange_fn)(void *ctx, int n_peers, const int *peers, const int64_t *off,
                                     const double *send, double *recv);
int pfem_solver_set_comm_host(pfem_solver *s, int rank, int nranks, pfem_host_allreduce_fn allreduce,
                              pfem_host_exchange_fn exchange, void *ctx);
/* Peer memory: the ranks map each other's receive boxes (hipIpcGetMemHandle / hipIpcOpenMemHandle) and their kernels write a
 * neighbour's segment straight into its box, one release / acquire flag per (rank, neighbour) pair; small all-reduces the same
 * way (every rank sums the boxes in rank order: identical bits).  Replaces the VecScatter / MPI_Allreduce inside KSPSolve
 * (solverpetsc.F:476) without a collective library and without the host in the data path.  Works between processes that SHARE
 * one device -- where RCCL refuses a second rank -- and is what the ranks-on-one-GPU tests run the device path with; between
 * devices it needs peer-mapped memory the runtime keeps coherent (not available to the builder: RCCL stays the default for
 * one rank per GPU).  The host hooks carry the bring-up (memory handles through `allreduce`), the teardown barrier and
 * all-reduces of more than 65536 doubles (symbolic phases); `exchange` is unused and may be NULL.  At most 16 ranks;
 * a neighbour's segment may hold PFEM_PEER_CAP_DOUBLES doubles (default 2^20).  Waits are bounded (10 s): a lost rank
 * surfaces as PFEM_ERR_COMM after the solve instead of a hung device.                                                    */
int pfem_solver_set_comm_peer(pfem_solver *s, int rank, int nranks, pfem_host_allreduce_fn allreduce,
                              pfem_host_exchange_fn exchange, void *ctx);
/* Collective teardown step of the communication backend, for all ranks while they can still reach each other (the host mirror's
 * free() calls it): the peer-memory transport waits here until no rank may still write into another's region.  Destroying a
 * solver without it is safe but not synchronised (the destructor is deliberately NOT collective).  Idempotent; PFEM_OK without a
 * backend.  Reference: MPI_Finalize-time destruction of the VecScatter inside KSPDestroy (solverpetsc.F:254-320). */
int pfem_solver_comm_shutdown(pfem_solver *s);
/* host-only helper (no GPU needed): ascending unique global dof ids in edof[0..count) that
 * lie outside the owned block [row_start,row_start+n_owned); two-call (NULL -> count).  */
int pfem_find_ghosts(int64_t count, const int32_t *edof, int64_t row_start, int64_t n_owned,
                     int64_t *n_ghost, int64_t *ghost_gid);
/* ghost dof ids (ascending) of the uploaded mesh: two-call (ghost_gid NULL -> count) */
int pfem_get_ghosts(pfem_solver *s, int64_t *n_ghost, int64_t *ghost_gid);

#ifdef __cplusplus
}
#endif
#endif /* PFEM_AMD_H */

// pfem_elem.hpp -- element arithmetic shared by the device kernels and the host
// per-element C-ABI entry points.
//
// One source for both sides so the per-element compat surface (host) and the batched
// assembly kernels (gfx950) produce the same bits.  Evaluation ORDER follows the
// reference statement by statement and the translation unit is compiled with
// -ffp-contract=off, because the reference is built without FMA contraction; with
// IEEE division on both sides the element matrices are bit-identical to the
// reference's (tests/test_elements_*).
//
// Reference: elementutilitiesbasisfuncs.F:16-52,165-234 (tria), :242-289,430-538 (tet);
//            elementutilitiespoisson.F:23-101,107-193;
//            elementutilitieselasticity3D.F:248-393;
//            triapoissonserialimpl1.F:573-594.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PFEM_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define PFEM_HD inline
#endif

namespace pfem {

// REAL(4) literals widened to double (the reference is compiled without
// -fdefault-real-8): 1.0/6.0 -> 0.16666667163372040, 1.0/3.0 -> 0.3333333432674408
constexpr double kGaussWtTet = static_cast<double>(1.0f / 6.0f);
constexpr double kGaussPtTria = static_cast<double>(1.0f / 3.0f);

// ---------------------------------------------------------------------------
// P1 tetrahedron: physical gradients and Jacobian at the single Gauss point.
// Local node order (a,b,c,d); parametric gradients g_a=(1,0,0), g_b=(0,1,0),
// g_c=(-1,-1,-1), g_d=(0,0,1)   [elementutilitiesbasisfuncs.F:268-281].
// The mapping matrix rows are a-c, b-c, d-c [:493-509]: the reference
// accumulates 0 + x_a*1 + x_b*0 + x_c*(-1) + x_d*0, which equals x_a - x_c
// exactly in IEEE arithmetic for finite inputs.
// ---------------------------------------------------------------------------
struct TetGeom {
    double gx[4], gy[4], gz[4];  // dN_a/dx, dN_a/dy, dN_a/dz
    double jac;
};

PFEM_HD void tet_geometry(const double x[4], const double y[4], const double z[4], TetGeom &g)
{
    // zero-initialised accumulation reproduced literally for the signed-zero cases
    const double b11 = ((0.0 + x[0]) + x[1] * 0.0) + (x[2] * -1.0) + x[3] * 0.0;
    const double b21 = ((0.0 + x[0] * 0.0) + x[1]) + (x[2] * -1.0) + x[3] * 0.0;
    const double b31 = ((0.0 + x[0] * 0.0) + x[1] * 0.0) + (x[2] * -1.0) + x[3];
    const double b12 = ((0.0 + y[0]) + y[1] * 0.0) + (y[2] * -1.0) + y[3] * 0.0;
    const double b22 = ((0.0 + y[0] * 0.0) + y[1]) + (y[2] * -1.0) + y[3] * 0.0;
    const double b32 = ((0.0 + y[0] * 0.0) + y[1] * 0.0) + (y[2] * -1.0) + y[3];
    const double b13 = ((0.0 + z[0]) + z[1] * 0.0) + (z[2] * -1.0) + z[3] * 0.0;
    const double b23 = ((0.0 + z[0] * 0.0) + z[1]) + (z[2] * -1.0) + z[3] * 0.0;
    const double b33 = ((0.0 + z[0] * 0.0) + z[1] * 0.0) + (z[2] * -1.0) + z[3];

    // determinant, three-term cofactor expansion in the reference's order [:512-514]
    double jac = b11 * (b22 * b33 - b23 * b32);
    jac = jac + b12 * (b23 * b31 - b21 * b33);
    jac = jac + b13 * (b21 * b32 - b22 * b31);
    const double di = 1.0 / jac;  // [:517]

    // adjugate inverse [:520-528]; i(r,c) == Binv(r,c)
    const double i11 = +di * (b22 * b33 - b23 * b32);
    const double i21 = -di * (b21 * b33 - b23 * b31);
    const double i31 = +di * (b21 * b32 - b22 * b31);
    const double i12 = -di * (b12 * b33 - b13 * b32);
    const double i22 = +di * (b11 * b33 - b13 * b31);
    const double i32 = -di * (b11 * b32 - b12 * b31);
    const double i13 = +di * (b12 * b23 - b13 * b22);
    const double i23 = -di * (b11 * b23 - b13 * b21);
    const double i33 = +di * (b11 * b22 - b12 * b21);

    // dN/dx = g.(Binv row 1) etc. [:532-536], with the literal 1/0/-1 products kept
    const double u1[4] = {1.0, 0.0, -1.0, 0.0};
    const double u2[4] = {0.0, 1.0, -1.0, 0.0};
    const double u3[4] = {0.0, 0.0, -1.0, 1.0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        g.gx[a] = u1[a] * i11 + u2[a] * i12 + u3[a] * i13;
        g.gy[a] = u1[a] * i21 + u2[a] * i22 + u3[a] * i23;
        g.gz[a] = u1[a] * i31 + u2[a] * i32 + u3[a] * i33;
    }
    g.jac = jac;
}

// The same geometry without the reference's literal products by 0.0 / 1.0 / -1.0 and its zero-initialised sums (117 of
// the 168 operations above).  For finite coordinates every NONZERO result has the same bits: x + (+-0) = x, x * -1.0 = -x,
// and the remaining additions are the same additions in the same order ((-x2) + x3 = x3 - x2 exactly).  What may differ is
// the SIGN OF A ZERO entry (the literal form turns -0 into +0 at its first `0.0 +`).  A signed zero can only travel on as
// a signed zero (no division by it short of a degenerate element, which the reference cannot assemble either), and every
// value the gather kernels build from these is ADDED to an accumulator that starts at +0.0, where +-0 changes nothing:
// assembled K and F have the same bits either way.  Used by the gather kernels only; the per-element entry points and
// pfem_eval_elems keep the literal form above.  (tests/native: lean == literal up to the sign of zeros, -0.0 coordinates
// included; tests/test_gpu_*: assembled K, F bit-exact against the oracle's literal serial loop.)
PFEM_HD void tet_geometry_lean(const double x[4], const double y[4], const double z[4], TetGeom &g)
{
    const double b11 = x[0] - x[2], b21 = x[1] - x[2], b31 = x[3] - x[2];
    const double b12 = y[0] - y[2], b22 = y[1] - y[2], b32 = y[3] - y[2];
    const double b13 = z[0] - z[2], b23 = z[1] - z[2], b33 = z[3] - z[2];
    double jac = b11 * (b22 * b33 - b23 * b32);
    jac = jac + b12 * (b23 * b31 - b21 * b33);
    jac = jac + b13 * (b21 * b32 - b22 * b31);
    const double di = 1.0 / jac;
    const double i11 = +di * (b22 * b33 - b23 * b32);
    const double i21 = -di * (b21 * b33 - b23 * b31);
    const double i31 = +di * (b21 * b32 - b22 * b31);
    const double i12 = -di * (b12 * b33 - b13 * b32);
    const double i22 = +di * (b11 * b33 - b13 * b31);
    const double i32 = -di * (b11 * b32 - b12 * b31);
    const double i13 = +di * (b12 * b23 - b13 * b22);
    const double i23 = -di * (b11 * b23 - b13 * b21);
    const double i33 = +di * (b11 * b22 - b12 * b21);
    g.gx[0] = i11;  g.gx[1] = i12;  g.gx[2] = (-i11 - i12) - i13;  g.gx[3] = i13;
    g.gy[0] = i21;  g.gy[1] = i22;  g.gy[2] = (-i21 - i22) - i23;  g.gy[3] = i23;
    g.gz[0] = i31;  g.gz[1] = i32;  g.gz[2] = (-i31 - i32) - i33;  g.gz[3] = i33;
    g.jac = jac;
}

// Poisson on a P1 tet, one Gauss point (1/4,1/4,1/4), source term -6
// [elementutilitiespoisson.F:107-193].  K column-major 4x4.  Returns false when the
// reference would STOP on a negative Jacobian [:157].
PFEM_HD bool poisson_tet(const double x[4], const double y[4], const double z[4], double kx,
                         double ky, double kz, double af, const double valC[4], double K[16],
                         double F[4])
{
    TetGeom g;
    tet_geometry(x, y, z, g);
    if (g.jac < 0.0) return false;
    const double dvol = kGaussWtTet * g.jac;                 // [:161]
    const double N[4] = {0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25};
    double du0 = 0.0, du1 = 0.0, du2 = 0.0;                  // [:165-170]
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        du0 = du0 + valC[a] * g.gx[a];
        du1 = du1 + valC[a] * g.gy[a];
        du2 = du2 + valC[a] * g.gz[a];
    }
    const double force = -6.0;                               // [:172]
#pragma unroll
    for (int i = 0; i < 4; ++i) {                            // [:174-188]
        const double b1 = g.gx[i] * dvol;
        const double b2 = g.gy[i] * dvol;
        const double b3 = g.gz[i] * dvol;
        const double b4 = N[i] * dvol;
        double f = 0.0 + b4 * force;
        f = f - b1 * du0 - b2 * du1 - b3 * du2;
        F[i] = f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            K[i + 4 * j] = 0.0 + af * (b1 * (kx * g.gx[j]) + b2 * (ky * g.gy[j]) + b3 * (kz * g.gz[j]));
    }
    return true;
}

// The part of poisson_tet() one NODE of the element needs (gather assembly): column a and, when
// `need_row`, row a of Klocal plus Flocal(a) -- the same expressions in the same order, entry by
// entry, so the bits equal those of the full routine (a is a run-time index: selects, no branches).
PFEM_HD bool poisson_tet_node(const double x[4], const double y[4], const double z[4], double kx,
                              double ky, double kz, double af, const double valC[4], int a, bool need_row,
                              double Kcol[4], double Krow[4], double &Fa)
{
    TetGeom g;
    tet_geometry(x, y, z, g);
    if (g.jac < 0.0) return false;
    const double dvol = kGaussWtTet * g.jac;
    const double N[4] = {0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25};
    double du0 = 0.0, du1 = 0.0, du2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        du0 = du0 + valC[i] * g.gx[i];
        du1 = du1 + valC[i] * g.gy[i];
        du2 = du2 + valC[i] * g.gz[i];
    }
    double gxa = g.gx[0], gya = g.gy[0], gza = g.gz[0], Na = N[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (i == a) { gxa = g.gx[i]; gya = g.gy[i]; gza = g.gz[i]; Na = N[i]; }
    const double force = -6.0;
    const double b1a = gxa * dvol, b2a = gya * dvol, b3a = gza * dvol, b4a = Na * dvol;
    double f = 0.0 + b4a * force;
    f = f - b1a * du0 - b2a * du1 - b3a * du2;
    Fa = f;
    const double cx = kx * gxa, cy = ky * gya, cz = kz * gza;
#pragma unroll
    for (int j = 0; j < 4; ++j) {          // Klocal(j,a): b's of row j, gradient of column a
        const double b1 = g.gx[j] * dvol, b2 = g.gy[j] * dvol, b3 = g.gz[j] * dvol;
        Kcol[j] = 0.0 + af * (b1 * cx + b2 * cy + b3 * cz);
    }
    if (need_row) {
#pragma unroll
        for (int j = 0; j < 4; ++j)        // Klocal(a,j)
            Krow[j] = 0.0 + af * (b1a * (kx * g.gx[j]) + b2a * (ky * g.gy[j]) + b3a * (kz * g.gz[j]));
    }
    return true;
}

// poisson_tet_node() on the lean geometry for valC = 0 (what the drivers pass, and all the gather kernel ever sees): the
// du terms vanish (b * (+0) = +-0, f - (+-0) = f) and the `0.0 +` of the literal form only turns a -0 into +0 -- again the
// same bits for every nonzero result (see tet_geometry_lean).
PFEM_HD bool poisson_tet_node_lean(const double x[4], const double y[4], const double z[4], double kx, double ky, double kz,
                                   double af, int a, bool need_row, double Kcol[4], double Krow[4], double &Fa)
{
    TetGeom g;
    tet_geometry_lean(x, y, z, g);
    if (g.jac < 0.0) return false;
    const double dvol = kGaussWtTet * g.jac;
    double gxa = g.gx[0], gya = g.gy[0], gza = g.gz[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (i == a) { gxa = g.gx[i]; gya = g.gy[i]; gza = g.gz[i]; }
    const double Na = a == 2 ? 1.0 - 0.25 - 0.25 - 0.25 : 0.25;
    const double b1a = gxa * dvol, b2a = gya * dvol, b3a = gza * dvol;
    Fa = (Na * dvol) * -6.0;
    const double cx = kx * gxa, cy = ky * gya, cz = kz * gza;
#pragma unroll
    for (int j = 0; j < 4; ++j) {          // Klocal(j,a)
        const double b1 = g.gx[j] * dvol, b2 = g.gy[j] * dvol, b3 = g.gz[j] * dvol;
        Kcol[j] = af * (b1 * cx + b2 * cy + b3 * cz);
    }
    if (need_row) {
#pragma unroll
        for (int j = 0; j < 4; ++j)        // Klocal(a,j)
            Krow[j] = af * (b1a * (kx * g.gx[j]) + b2a * (ky * g.gy[j]) + b3a * (kz * g.gz[j]));
    }
    return true;
}

// ---------------------------------------------------------------------------
// P1 triangle [elementutilitiesbasisfuncs.F:16-52,165-234]: N=(xi3,xi1,xi2),
// parametric gradients (-1,-1),(1,0),(0,1); mapping rows n2-n1, n3-n1.
// ---------------------------------------------------------------------------
PFEM_HD bool poisson_tria(const double x[3], const double y[3], double kx, double ky, double af,
                          const double valC[3], double K[9], double F[3])
{
    const double u1[3] = {-1.0, 1.0, 0.0};
    const double u2[3] = {-1.0, 0.0, 1.0};
    double b11 = 0.0, b21 = 0.0, b12 = 0.0, b22 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {                            // [:207-215]
        b11 = b11 + (x[a] * u1[a]);
        b21 = b21 + (x[a] * u2[a]);
        b12 = b12 + (y[a] * u1[a]);
        b22 = b22 + (y[a] * u2[a]);
    }
    const double jac = b11 * b22 - b12 * b21;                // [:217]
    const double di = 1.0 / jac;
    const double i11 = b22 * di, i12 = -b12 * di, i21 = -b21 * di, i22 = b11 * di;  // [:221-224]
    double gx[3], gy[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        gx[a] = u1[a] * i11 + u2[a] * i12;
        gy[a] = u1[a] * i21 + u2[a] * i22;
    }
    if (jac < 0.0) return false;                             // elementutilitiespoisson.F:72
    const double xi1 = kGaussPtTria, xi2 = kGaussPtTria;     // [:57]
    const double N[3] = {1.0 - xi1 - xi2, xi1, xi2};
    const double dvol = 0.5 * jac;                           // [:58,76]
    double du0 = 0.0, du1 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        du0 = du0 + valC[a] * gx[a];
        du1 = du1 + valC[a] * gy[a];
    }
    const double force = 0.0;                                // [:84]
#pragma unroll
    for (int i = 0; i < 3; ++i) {                            // [:86-97]
        const double b1 = gx[i] * dvol, b2 = gy[i] * dvol, b4 = N[i] * dvol;
        F[i] = 0.0 + b4 * force - b1 * du0 - b2 * du1;
#pragma unroll
        for (int j = 0; j < 3; ++j) K[i + 3 * j] = 0.0 + af * (b1 * (kx * gx[j]) + b2 * (ky * gy[j]));
    }
    return true;
}

// Inline element of the serial driver: Ke = area * (B B^T), B = [y_jk, x_kj]/(2 area),
// no load vector [triapoissonserialimpl1.F:573-594].
PFEM_HD bool poisson_tria_inline(const double x[3], const double y[3], double K[9], double F[3])
{
    const double area =
        0.5 * (x[1] * y[2] - x[2] * y[1] + x[2] * y[0] - x[0] * y[2] + x[0] * y[1] - x[1] * y[0]);
    const double two_a = 2.0 * area;
    const double bm[3][2] = {{(y[1] - y[2]) / two_a, (x[2] - x[1]) / two_a},
                             {(y[2] - y[0]) / two_a, (x[0] - x[2]) / two_a},
                             {(y[0] - y[1]) / two_a, (x[1] - x[0]) / two_a}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            K[i + 3 * j] = area * ((0.0 + bm[i][0] * bm[j][0]) + bm[i][1] * bm[j][1]);
    F[0] = F[1] = F[2] = 0.0;
    return true;
}

// ---------------------------------------------------------------------------
// Plane-stress elasticity on a P1 triangle [elementutilitieselasticity2D.F:23-153], the 2-D sibling
// (SURVEY 8f.1).  D = b1*[[1,nu,0],[nu,1,0],[0,0,(1-nu)]] with b1 = E/(1-nu^2) -- the reference's
// D(3,3) = b1*(1-nu), i.e. 2G with engineering shear, is reproduced as is.
// B (3x6) has columns (gx,0,gy) / (0,gy,gx); with the structural zeros dropped the reference's two
// MATMULs collapse, in the same summation order, to two products per entry:
//   K(2a+0,2b+0) = dvol*(ax*(D11 bx) + ay*(D33 by))   K(2a+0,2b+1) = dvol*(ax*(D12 by) + ay*(D33 bx))
//   K(2a+1,2b+0) = dvol*(ay*(D21 bx) + ax*(D33 by))   K(2a+1,2b+1) = dvol*(ay*(D22 by) + ax*(D33 bx))
// ---------------------------------------------------------------------------
struct TriaGeom {
    double gx[3], gy[3], jac;
};

PFEM_HD void tria_geometry(const double x[3], const double y[3], TriaGeom &g)
{
    const double u1[3] = {-1.0, 1.0, 0.0};
    const double u2[3] = {-1.0, 0.0, 1.0};
    double b11 = 0.0, b21 = 0.0, b12 = 0.0, b22 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {                            // elementutilitiesbasisfuncs.F:207-215
        b11 = b11 + (x[a] * u1[a]);
        b21 = b21 + (x[a] * u2[a]);
        b12 = b12 + (y[a] * u1[a]);
        b22 = b22 + (y[a] * u2[a]);
    }
    g.jac = b11 * b22 - b12 * b21;
    const double di = 1.0 / g.jac;
    const double i11 = b22 * di, i12 = -b12 * di, i21 = -b21 * di, i22 = b11 * di;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.gx[a] = u1[a] * i11 + u2[a] * i12;
        g.gy[a] = u1[a] * i21 + u2[a] * i22;
    }
}

struct Elast2dMat {
    double d11, d12, d33;
};

PFEM_HD Elast2dMat elast2d_material(double E, double nu)
{
    const double b1 = E / (1.0 - nu * nu);                   // [:60]
    Elast2dMat m;
    m.d11 = b1;
    m.d12 = b1 * nu;
    m.d33 = b1 * (1.0 - nu);
    return m;
}

// 2x2 block K(2a+p, 2b+q) from grad N_a = (ax,ay), grad N_b = (bx,by)
PFEM_HD void elast2d_block_v(double ax, double ay, double bx, double by, const Elast2dMat &m, double dvol,
                             double blk[2][2])
{
    blk[0][0] = dvol * (ax * (m.d11 * bx) + ay * (m.d33 * by));
    blk[0][1] = dvol * (ax * (m.d12 * by) + ay * (m.d33 * bx));
    blk[1][0] = dvol * (ay * (m.d12 * bx) + ax * (m.d33 * by));
    blk[1][1] = dvol * (ay * (m.d11 * by) + ax * (m.d33 * bx));
}

// shape functions at the Gauss point (1/3,1/3) given as REAL(4) literals [:73]: N = (xi3, xi1, xi2)
PFEM_HD void tria_shape_gp(double N[3])
{
    const double xi1 = kGaussPtTria, xi2 = kGaussPtTria;
    N[0] = 1.0 - xi1 - xi2;
    N[1] = xi1;
    N[2] = xi2;
}

// Full 6x6 (column-major) + load vector; elemData = (E, nu, thick, bx, by)
PFEM_HD bool elast_tria(const double x[3], const double y[3], double E, double nu, double thick,
                        const double bforce[2], double K[36], double F[6])
{
    TriaGeom g;
    tria_geometry(x, y, g);
    if (g.jac < 0.0) return false;                           // [:88]
    const double dvol = 0.5 * (g.jac * thick);               // [:92]
    const Elast2dMat m = elast2d_material(E, nu);
    double blk[2][2], N[3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            elast2d_block_v(g.gx[a], g.gy[a], g.gx[b], g.gy[b], m, dvol, blk);
            K[(2 * a) + 6 * (2 * b)] = blk[0][0];
            K[(2 * a) + 6 * (2 * b + 1)] = blk[0][1];
            K[(2 * a + 1) + 6 * (2 * b)] = blk[1][0];
            K[(2 * a + 1) + 6 * (2 * b + 1)] = blk[1][1];
        }
    tria_shape_gp(N);
#pragma unroll
    for (int a = 0; a < 3; ++a) {                            // [:140-148]
        const double b4 = dvol * N[a];
        F[2 * a] = 0.0 + b4 * bforce[0];
        F[2 * a + 1] = 0.0 + b4 * bforce[1];
    }
    return true;
}

// ---------------------------------------------------------------------------
// Linear elasticity on a P1 tet [elementutilitieselasticity3D.F:248-393], intended
// semantics (one Gauss point, Ke = dvol * B^T (D B); DESIGN.md "deviations").
//
// B is 6x12 with Voigt rows [xx,yy,zz,xy,yz,zx] [:359-371] and D is the isotropic
// matrix of [:287-296].  The reference forms DB = MATMUL(D,B) and K = MATMUL(B^T,DB),
// both summed over the inner index ascending from zero.  Because B and D are sparse
// with structural zeros, and x + 0*y == x, 0 + x == x in IEEE arithmetic (finite y),
// the sums collapse to the few terms below IN THE SAME ORDER, i.e. the same bits --
// without ever materialising the 6x12 / 12x12 dense operands.
//   DB(:, 3a+0) = [D11 gx, D21 gx, D31 gx, G gy, 0, G gz]
//   DB(:, 3a+1) = [D12 gy, D22 gy, D32 gy, G gx, G gz, 0]
//   DB(:, 3a+2) = [D13 gz, D23 gz, D33 gz, 0, G gy, G gx]
// K(3a+p, 3b+q) = dvol * sum_k B(k,3a+p) DB(k,3b+q), k ascending over the nonzero rows
// of column 3a+p: p=0 -> k={0,3,5}, p=1 -> k={1,3,4}, p=2 -> k={2,4,5}.
// The callback form lets the device kernel stream 3x3 node blocks straight to the
// scatter without holding the 12x12 matrix in registers.
// ---------------------------------------------------------------------------
struct ElastMat {
    double d11, d12, gsh;  // b1(1-nu), b1 nu, b1 b2
};

PFEM_HD ElastMat elast_material(double E, double nu)
{
    const double b1 = E / ((1.0 + nu) * (1.0 - 2.0 * nu));  // [:284]
    const double b2 = (1.0 - 2.0 * nu) / 2.0;               // [:285]
    ElastMat m;
    m.d11 = b1 * (1.0 - nu);
    m.d12 = b1 * nu;
    m.gsh = b1 * b2;
    return m;
}

// 3x3 block K(3a+p,3b+q), p,q=0..2, into blk[p][q].
// Value form: (ax,ay,az) = grad N_a, (bx,by,bz) = grad N_b.
PFEM_HD void elast_block_v(double ax, double ay, double az, double bx, double by, double bz,
                           const ElastMat &m, double dvol, double blk[3][3]);

PFEM_HD void elast_block(const TetGeom &g, const ElastMat &m, double dvol, int a, int b,
                         double blk[3][3])
{
    elast_block_v(g.gx[a], g.gy[a], g.gz[a], g.gx[b], g.gy[b], g.gz[b], m, dvol, blk);
}

PFEM_HD void elast_block_v(double ax, double ay, double az, double bx, double by, double bz,
                           const ElastMat &m, double dvol, double blk[3][3])
{
    // DB columns of node b (rows 0..5); structural zeros omitted
    const double c0_0 = m.d11 * bx, c0_1 = m.d12 * bx, c0_2 = m.d12 * bx, c0_3 = m.gsh * by, c0_5 = m.gsh * bz;
    const double c1_0 = m.d12 * by, c1_1 = m.d11 * by, c1_2 = m.d12 * by, c1_3 = m.gsh * bx, c1_4 = m.gsh * bz;
    const double c2_0 = m.d12 * bz, c2_1 = m.d12 * bz, c2_2 = m.d11 * bz, c2_4 = m.gsh * by, c2_5 = m.gsh * bx;
    // row p=0 of node a: B rows {0:ax, 3:ay, 5:az}
    blk[0][0] = dvol * ((ax * c0_0 + ay * c0_3) + az * c0_5);
    blk[0][1] = dvol * (ax * c1_0 + ay * c1_3);
    blk[0][2] = dvol * (ax * c2_0 + az * c2_5);
    // row p=1: B rows {1:ay, 3:ax, 4:az}
    blk[1][0] = dvol * (ay * c0_1 + ax * c0_3);
    blk[1][1] = dvol * ((ay * c1_1 + ax * c1_3) + az * c1_4);
    blk[1][2] = dvol * (ay * c2_1 + az * c2_4);
    // row p=2: B rows {2:az, 4:ay, 5:ax}
    blk[2][0] = dvol * (az * c0_2 + ax * c0_5);
    blk[2][1] = dvol * (az * c1_2 + ay * c1_4);
    blk[2][2] = dvol * ((az * c2_2 + ay * c2_4) + ax * c2_5);
}

// Full 12x12 (column-major) + load vector; used by the host per-element entry point
// and by pfem_eval_elems.
PFEM_HD bool elast_tet(const double x[4], const double y[4], const double z[4], double E, double nu,
                       const double bforce[3], double K[144], double F[12])
{
    TetGeom g;
    tet_geometry(x, y, z, g);
    if (g.jac < 0.0) return false;                           // [:320]
    const double dvol = kGaussWtTet * g.jac;                 // [:305,324]
    const ElastMat m = elast_material(E, nu);
    double blk[3][3];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            elast_block(g, m, dvol, a, b, blk);
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) K[(3 * a + p) + 12 * (3 * b + q)] = blk[p][q];
        }
    const double N[4] = {0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25};
#pragma unroll
    for (int a = 0; a < 4; ++a) {                            // [:380-390]
        const double b4 = dvol * N[a];
        F[3 * a + 0] = 0.0 + b4 * bforce[0];
        F[3 * a + 1] = 0.0 + b4 * bforce[1];
        F[3 * a + 2] = 0.0 + b4 * bforce[2];
    }
    return true;
}

// ---------------------------------------------------------------------------
// Post-processing of a solution, element by element (pfem_elem_post / pfem_post_elements / pfem_post_nodal_forces): from the
// nodal values valC of one element
//   grad   Poisson: grad u.  Elasticity: the strain B valC in the B matrix's own Voigt order with ENGINEERING shear --
//          [xx,yy,zz,gxy,gyz,gzx] for the tet [elementutilitieselasticity3D.F:359-371], [xx,yy,gxy] for the triangle.
//   flux   Poisson: q = -(kx,ky,kz) o grad u.  Elasticity: sigma = D strain with the very D the stiffness routine beside it
//          uses (elast_material / elast2d_material).  The plane-stress D(3,3) is the reference's b1(1-nu) = 2G:
//          the 2-D shear stress therefore carries the reference's factor, twice the textbook G gxy.
//   scalar Poisson: |q|_2.  Elasticity: von Mises -- the 6-component form in 3-D, sqrt(sxx^2 - sxx syy + syy^2 + 3 txy^2)
//          for plane stress.
//   fint   dvol B^T sigma (Poisson: dvol grad N . (k o grad u)): the element's internal nodal forces.  fint = Klocal valC to
//          rounding, with Klocal of the stiffness routine at af = 1 (tests/test_post_host.py).
// Geometry, material and dvol are those of the stiffness routines.  Two things of the reference are NOT followed, because
// they disagree with the K they sit beside (DESIGN.md "deviations"): its explicit residual routine multiplies HALF shear
// strains by G [elementutilitieselasticity3D.F:676-683], and the residual half of the Poisson routines (poisson_tet above,
// `f - b1*du0 ...`) leaves the conductivity out.  dvol is handed back for the load vector of the nodal forces.
// ---------------------------------------------------------------------------
PFEM_HD bool poisson_tet_post(const double x[4], const double y[4], const double z[4], double kx, double ky, double kz,
                              const double valC[4], double grad[3], double flux[3], double &scalar, double fint[4], double &dvol)
{
    TetGeom g;
    tet_geometry(x, y, z, g);
    if (g.jac < 0.0) return false;
    dvol = kGaussWtTet * g.jac;
    double du0 = 0.0, du1 = 0.0, du2 = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        du0 = du0 + valC[a] * g.gx[a];
        du1 = du1 + valC[a] * g.gy[a];
        du2 = du2 + valC[a] * g.gz[a];
    }
    const double q0 = kx * du0, q1 = ky * du1, q2 = kz * du2;      // k o grad u
    grad[0] = du0;  grad[1] = du1;  grad[2] = du2;
    flux[0] = -q0;  flux[1] = -q1;  flux[2] = -q2;
    scalar = sqrt((q0 * q0 + q1 * q1) + q2 * q2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double b1 = g.gx[i] * dvol, b2 = g.gy[i] * dvol, b3 = g.gz[i] * dvol;
        fint[i] = (b1 * q0 + b2 * q1) + b3 * q2;
    }
    return true;
}

// `oriented` = false: the inline element of the serial driver (poisson_tria_inline), which has no orientation test -- k = 1 and
// the gradients of tria_geometry (differences of coordinates; the inline routine's own area formula, products of absolute
// coordinates, loses digits that a gradient of the solution should not lose: its fint agrees with poisson_tria_inline's
// K valC to the rounding of THAT formula)
PFEM_HD bool poisson_tria_post(const double x[3], const double y[3], double kx, double ky, const double valC[3], double grad[2],
                               double flux[2], double &scalar, double fint[3], double &dvol, bool oriented = true)
{
    TriaGeom g;
    tria_geometry(x, y, g);
    if (oriented && g.jac < 0.0) return false;
    dvol = 0.5 * g.jac;
    double du0 = 0.0, du1 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        du0 = du0 + valC[a] * g.gx[a];
        du1 = du1 + valC[a] * g.gy[a];
    }
    const double q0 = kx * du0, q1 = ky * du1;
    grad[0] = du0;  grad[1] = du1;
    flux[0] = -q0;  flux[1] = -q1;
    scalar = sqrt(q0 * q0 + q1 * q1);
#pragma unroll
    for (int i = 0; i < 3; ++i) fint[i] = (g.gx[i] * dvol) * q0 + (g.gy[i] * dvol) * q1;
    return true;
}

// TH: a thermal state is given -- the normal strains enter D less the thermal strain eth (thermal_strain below), `grad` stays
// the total strain B valC, scalar and fint are formed from that stress.  TH = false is the routine as it always was.
template <bool TH>
PFEM_HD bool elast_tet_post_t(const double x[4], const double y[4], const double z[4], double E, double nu, const double valC[12],
                              double eth, double grad[6], double flux[6], double &scalar, double fint[12], double &dvol)
{
    TetGeom g;
    tet_geometry(x, y, z, g);
    if (g.jac < 0.0) return false;
    dvol = kGaussWtTet * g.jac;
    const ElastMat m = elast_material(E, nu);
    // strain = B valC, B rows [xx,yy,zz,xy,yz,zx]: column 3a+0 = (gx,0,0,gy,0,gz), 3a+1 = (0,gy,0,gx,gz,0), 3a+2 = (0,0,gz,0,gy,gx)
    double exx = 0.0, eyy = 0.0, ezz = 0.0, gxy = 0.0, gyz = 0.0, gzx = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double u = valC[3 * a], v = valC[3 * a + 1], w = valC[3 * a + 2];
        exx = exx + g.gx[a] * u;
        eyy = eyy + g.gy[a] * v;
        ezz = ezz + g.gz[a] * w;
        gxy = (gxy + g.gy[a] * u) + g.gx[a] * v;
        gyz = (gyz + g.gz[a] * v) + g.gy[a] * w;
        gzx = (gzx + g.gz[a] * u) + g.gx[a] * w;
    }
    const double mxx = TH ? exx - eth : exx, myy = TH ? eyy - eth : eyy, mzz = TH ? ezz - eth : ezz;   // mechanical normal strains
    const double sxx = (m.d11 * mxx + m.d12 * myy) + m.d12 * mzz;
    const double syy = (m.d12 * mxx + m.d11 * myy) + m.d12 * mzz;
    const double szz = (m.d12 * mxx + m.d12 * myy) + m.d11 * mzz;
    const double txy = m.gsh * gxy, tyz = m.gsh * gyz, tzx = m.gsh * gzx;
    grad[0] = exx;  grad[1] = eyy;  grad[2] = ezz;  grad[3] = gxy;  grad[4] = gyz;  grad[5] = gzx;
    flux[0] = sxx;  flux[1] = syy;  flux[2] = szz;  flux[3] = txy;  flux[4] = tyz;  flux[5] = tzx;
    const double d0 = sxx - syy, d1 = syy - szz, d2 = szz - sxx;
    scalar = sqrt(0.5 * ((d0 * d0 + d1 * d1) + d2 * d2) + 3.0 * ((txy * txy + tyz * tyz) + tzx * tzx));
#pragma unroll
    for (int a = 0; a < 4; ++a) {                            // B^T sigma: the rows of elast_block_v
        const double ax = g.gx[a], ay = g.gy[a], az = g.gz[a];
        fint[3 * a + 0] = dvol * ((ax * sxx + ay * txy) + az * tzx);
        fint[3 * a + 1] = dvol * ((ay * syy + ax * txy) + az * tyz);
        fint[3 * a + 2] = dvol * ((az * szz + ay * tyz) + ax * tzx);
    }
    return true;
}

PFEM_HD bool elast_tet_post(const double x[4], const double y[4], const double z[4], double E, double nu, const double valC[12],
                            double grad[6], double flux[6], double &scalar, double fint[12], double &dvol)
{
    return elast_tet_post_t<false>(x, y, z, E, nu, valC, 0.0, grad, flux, scalar, fint, dvol);
}

template <bool TH>
PFEM_HD bool elast_tria_post_t(const double x[3], const double y[3], double E, double nu, double thick, const double valC[6],
                               double eth, double grad[3], double flux[3], double &scalar, double fint[6], double &dvol)
{
    TriaGeom g;
    tria_geometry(x, y, g);
    if (g.jac < 0.0) return false;
    dvol = 0.5 * (g.jac * thick);
    const Elast2dMat m = elast2d_material(E, nu);
    double exx = 0.0, eyy = 0.0, gxy = 0.0;                  // B columns (gx,0,gy) / (0,gy,gx)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        exx = exx + g.gx[a] * valC[2 * a];
        eyy = eyy + g.gy[a] * valC[2 * a + 1];
        gxy = (gxy + g.gy[a] * valC[2 * a]) + g.gx[a] * valC[2 * a + 1];
    }
    const double mxx = TH ? exx - eth : exx, myy = TH ? eyy - eth : eyy;       // no thermal shear: D(3,3) sees gxy as it is
    const double sxx = m.d11 * mxx + m.d12 * myy, syy = m.d12 * mxx + m.d11 * myy, txy = m.d33 * gxy;
    grad[0] = exx;  grad[1] = eyy;  grad[2] = gxy;
    flux[0] = sxx;  flux[1] = syy;  flux[2] = txy;
    scalar = sqrt(((sxx * sxx - sxx * syy) + syy * syy) + 3.0 * (txy * txy));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        fint[2 * a] = dvol * (g.gx[a] * sxx + g.gy[a] * txy);
        fint[2 * a + 1] = dvol * (g.gy[a] * syy + g.gx[a] * txy);
    }
    return true;
}

PFEM_HD bool elast_tria_post(const double x[3], const double y[3], double E, double nu, double thick, const double valC[6],
                             double grad[3], double flux[3], double &scalar, double fint[6], double &dvol)
{
    return elast_tria_post_t<false>(x, y, E, nu, thick, valC, 0.0, grad, flux, scalar, fint, dvol);
}

// components of grad / flux per kind (kinds as in include/pfem_amd.h: 1 Poisson tria, 2 Poisson tet, 3 elasticity tet,
// 4 inline Poisson tria, 5 elasticity tria)
PFEM_HD int post_components(int kind) { return kind == 3 ? 6 : ((kind == 2 || kind == 5) ? 3 : 2); }

// One element of any kind; z is not read in 2-D.  ed = elemData of the kind's stiffness routine.
PFEM_HD bool elem_post(int kind, const double *x, const double *y, const double *z, const double *ed, const double *valC,
                       double *grad, double *flux, double &scalar, double *fint, double &dvol)
{
    switch (kind) {
    case 1: return poisson_tria_post(x, y, ed[0], ed[1], valC, grad, flux, scalar, fint, dvol);
    case 2: return poisson_tet_post(x, y, z, ed[0], ed[1], ed[2], valC, grad, flux, scalar, fint, dvol);
    case 3: return elast_tet_post(x, y, z, ed[0], ed[1], valC, grad, flux, scalar, fint, dvol);
    case 4: return poisson_tria_post(x, y, 1.0, 1.0, valC, grad, flux, scalar, fint, dvol, false);
    default: return elast_tria_post(x, y, ed[0], ed[1], ed[2], valC, grad, flux, scalar, fint, dvol);
    }
}

// ---------------------------------------------------------------------------
// Thermal strains of the elasticity kinds (pfem_elem_thermal_load / pfem_thermal_* / pfem_rhs_add_thermal_load; DESIGN.md
// section 14).  theta[a] = T_a - T_ref at the element's nodes.  The thermal strain is constant over a constant-strain element:
//     thetabar = sum over a ascending of N(a) * theta[a], from 0.0, N the Gauss-point shape values of the kind's stiffness
//                routine (the tet's literal quarters, tria_shape_gp);        e_th = alpha * thetabar
// eps_th = e_th [1,1,1,0,0,0] (tet), e_th [1,1,0] (plane stress): no thermal shear.
// ---------------------------------------------------------------------------
PFEM_HD double thermal_strain(int kind, double alpha, const double *theta)
{
    double tb = 0.0;
    if (kind == 3) {
        const double N[4] = {0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25};
#pragma unroll
        for (int a = 0; a < 4; ++a) tb = tb + N[a] * theta[a];
    } else {
        double N[3];
        tria_shape_gp(N);
#pragma unroll
        for (int a = 0; a < 3; ++a) tb = tb + N[a] * theta[a];
    }
    return alpha * tb;
}

// elem_post under a thermal state: the stress is D (eps - eps_th) for the elasticity kinds; the Poisson kinds have no such state
PFEM_HD bool elem_post_th(int kind, const double *x, const double *y, const double *z, const double *ed, const double *valC, double eth,
                          double *grad, double *flux, double &scalar, double *fint, double &dvol)
{
    switch (kind) {
    case 3: return elast_tet_post_t<true>(x, y, z, ed[0], ed[1], valC, eth, grad, flux, scalar, fint, dvol);
    case 5: return elast_tria_post_t<true>(x, y, ed[0], ed[1], ed[2], valC, eth, grad, flux, scalar, fint, dvol);
    default: return elem_post(kind, x, y, z, ed, valC, grad, flux, scalar, fint, dvol);
    }
}

// The thermal load F = dvol B^T D eps_th of one element and sig[ng] = D eps_th, geometry, D and dvol those of the stiffness
// routine (thickness in the triangle's dvol).  The load takes ONE normal stress
//     tet       s = (d11 * e_th + d12 * e_th) + d12 * e_th          F[3a + d] = dvol * (g_d[a] * s)
//     triangle  s = d11 * e_th + d12 * e_th                         F[2a] = dvol * (gx[a] * s),  F[2a + 1] = dvol * (gy[a] * s)
// sig[c] is row c of D on eps_th in that row's own order of elem_post_th, so that with valC = 0 the stress of elem_post_th is
// -sig bit for bit: rows xx and yy give s (an addition commutes), the tet's row zz is (d12 * e_th + d12 * e_th) + d11 * e_th;
// zeros at the shear components.  F and sig may be null.  false: a negative Jacobian.  Kinds 3 and 5 only (the caller checks).
PFEM_HD bool elem_thermal_load(int kind, const double *x, const double *y, const double *z, const double *ed, double eth, double *F,
                               double *sig)
{
    if (kind == 3) {
        TetGeom g;
        tet_geometry(x, y, z, g);
        if (g.jac < 0.0) return false;
        const double dvol = kGaussWtTet * g.jac;
        const ElastMat m = elast_material(ed[0], ed[1]);
        const double s = (m.d11 * eth + m.d12 * eth) + m.d12 * eth;
        if (F) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                F[3 * a + 0] = dvol * (g.gx[a] * s);
                F[3 * a + 1] = dvol * (g.gy[a] * s);
                F[3 * a + 2] = dvol * (g.gz[a] * s);
            }
        }
        if (sig) {
            sig[0] = s;
            sig[1] = (m.d12 * eth + m.d11 * eth) + m.d12 * eth;
            sig[2] = (m.d12 * eth + m.d12 * eth) + m.d11 * eth;
            sig[3] = sig[4] = sig[5] = 0.0;
        }
        return true;
    }
    TriaGeom g;
    tria_geometry(x, y, g);
    if (g.jac < 0.0) return false;
    const double dvol = 0.5 * (g.jac * ed[2]);
    const Elast2dMat m = elast2d_material(ed[0], ed[1]);
    const double s = m.d11 * eth + m.d12 * eth;
    if (F) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            F[2 * a] = dvol * (g.gx[a] * s);
            F[2 * a + 1] = dvol * (g.gy[a] * s);
        }
    }
    if (sig) {
        sig[0] = s;
        sig[1] = m.d12 * eth + m.d11 * eth;
        sig[2] = 0.0;
    }
    return true;
}

// r = Klocal valC - Flocal for the Klocal, Flocal the assembly takes from the stiffness routine with valC = 0 (af scales the
// Poisson matrices only; source term -6 of the Poisson tet, body force of the elasticity kinds): the element's share of the
// nodal forces R of pfem_post_nodal_forces.
// TH: under a thermal state (elem_post_th) -- fint is then dvol B^T D (eps - eps_th) = Klocal valC - F_th, so r is the element's
// share of sum (K_e u_e - F_e - F_th,e).
template <bool TH>
PFEM_HD bool elem_nodal_forces_t(int kind, const double *x, const double *y, const double *z, const double *ed, double af,
                                 const double *valC, double eth, double *r)
{
    double grad[6], flux[6], scalar, dvol;
    if (TH) {
        if (!elem_post_th(kind, x, y, z, ed, valC, eth, grad, flux, scalar, r, dvol)) return false;
    } else {
        if (!elem_post(kind, x, y, z, ed, valC, grad, flux, scalar, r, dvol)) return false;
    }
    if (kind == 2) {
        const double N[4] = {0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25};
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = af * r[i] - (N[i] * dvol) * -6.0;
    } else if (kind == 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = af * r[i];
    } else if (kind == 3) {
        const double N[4] = {0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double b4 = dvol * N[a];
#pragma unroll
            for (int d = 0; d < 3; ++d) r[3 * a + d] = r[3 * a + d] - b4 * ed[3 + d];
        }
    } else if (kind == 5) {
        double N[3];
        tria_shape_gp(N);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double b4 = dvol * N[a];
            r[2 * a] = r[2 * a] - b4 * ed[3];
            r[2 * a + 1] = r[2 * a + 1] - b4 * ed[4];
        }
    }
    return true;
}

PFEM_HD bool elem_nodal_forces(int kind, const double *x, const double *y, const double *z, const double *ed, double af,
                               const double *valC, double *r)
{
    return elem_nodal_forces_t<false>(kind, x, y, z, ed, af, valC, 0.0, r);
}

// ---------------------------------------------------------------------------
// Nodal recovery and the Zienkiewicz-Zhu indicator (pfem_post_nodal_recovery / pfem_post_error_indicator)
// ---------------------------------------------------------------------------
// The scalar of elem_post, evaluated on ANY flux / stress vector in the kind's stored Voigt order (the recovered nodal values):
// |q|_2, von Mises, the plane-stress form.  The expressions are elem_post's, term for term (|q| of -q is |q|'s own bits).
PFEM_HD double post_scalar(int kind, const double *f)
{
    switch (kind) {
    case 2: return sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
    case 3: {
        const double d0 = f[0] - f[1], d1 = f[1] - f[2], d2 = f[2] - f[0];
        return sqrt(0.5 * ((d0 * d0 + d1 * d1) + d2 * d2) + 3.0 * ((f[3] * f[3] + f[4] * f[4]) + f[5] * f[5]));
    }
    case 5: return sqrt(((f[0] * f[0] - f[0] * f[1]) + f[1] * f[1]) + 3.0 * (f[2] * f[2]));
    default: return sqrt(f[0] * f[0] + f[1] * f[1]);
    }
}

// One element's share of the ZZ indicator.  sigma* is interpolated linearly from nodal[a * ng + c], sigma_h = flux of elem_post is
// constant, so with d_ac = nodal[a * ng + c] - f_c and the P1 mass matrix V (1 + delta_ab) / ((d+1)(d+2)) of a simplex in d
// dimensions the integral of |sigma* - sigma_h|^2 is exactly
//     eta2 = V / ((d+1)(d+2)) sum_c [ sum_a d_ac^2 + (sum_a d_ac)^2 ],        fnorm2 = V sum_c f_c^2,
// a plain Euclidean sum over the ng stored Voigt components (no D^-1 weighting; shear components count once, as stored).  V is
// elem_post's dvol (area x thickness for the plane-stress triangle).  nodal == flux at every node gives eta2 = 0.0 exactly.
// TH: sigma_h is the stress of elem_post_th.
template <bool TH>
PFEM_HD bool elem_recovery_error_t(int kind, const double *x, const double *y, const double *z, const double *ed, const double *valC,
                                   double eth, const double *nodal, double &eta2, double &fnorm2)
{
    double grad[6], flux[6], fint[12], scalar, dvol;
    if (TH) {
        if (!elem_post_th(kind, x, y, z, ed, valC, eth, grad, flux, scalar, fint, dvol)) return false;
    } else {
        if (!elem_post(kind, x, y, z, ed, valC, grad, flux, scalar, fint, dvol)) return false;
    }
    const int ng = post_components(kind), npe = (kind == 2 || kind == 3) ? 4 : 3;
    double e2 = 0.0, f2 = 0.0;
    for (int c = 0; c < ng; ++c) {
        double sq = 0.0, sm = 0.0;
        for (int a = 0; a < npe; ++a) {
            const double d = nodal[a * ng + c] - flux[c];
            sq = sq + d * d;
            sm = sm + d;
        }
        e2 = e2 + (sq + sm * sm);
        f2 = f2 + flux[c] * flux[c];
    }
    eta2 = dvol / static_cast<double>(npe * (npe + 1)) * e2;
    fnorm2 = dvol * f2;
    return true;
}

PFEM_HD bool elem_recovery_error(int kind, const double *x, const double *y, const double *z, const double *ed, const double *valC,
                                 const double *nodal, double &eta2, double &fnorm2)
{
    return elem_recovery_error_t<false>(kind, x, y, z, ed, valC, 0.0, nodal, eta2, fnorm2);
}

// ---------------------------------------------------------------------------
// Lumped mass (pfem_elem_lumped_mass / pfem_dynamics_setup): MassMatrixLinearTria / MassMatrixLinearTetra
// [elementutilitieselasticity2D.F:283-362, elementutilitieselasticity3D.F:401-482] -- the row sums of the consistent mass
// at the one Gauss point, Mn[a] for local node a (the same for each of the node's dofs):
//     b4 = (dens * dvol) * N(a);   Mn[a] = sum over j ascending of b4 * N(j),  from 0.0
// the reference's loop with the structural zeros of its (nsize x nsize) Klocal left out (x + 0.0 == x).  dvol and N are those of
// the kind's stiffness routine: the tet's N = 1/4 each, the triangle's REAL(4) Gauss point (tria_shape_gp), thickness in the
// triangle's dvol.  Density is an argument: the reference reads elemData(3), which is `thick` in the stiffness routines.
// The tet routine's nGP = 8 over one initialised point is the stiffness routine's defect (DESIGN.md "deviations"): one point.
// false: a negative Jacobian (not tested for the inline triangle, which has no orientation test).
// ---------------------------------------------------------------------------
PFEM_HD bool elem_lumped_mass(int kind, const double *x, const double *y, const double *z, const double *ed, double dens, double *Mn)
{
    if (kind == 2 || kind == 3) {
        TetGeom g;
        tet_geometry(x, y, z, g);
        if (g.jac < 0.0) return false;
        const double dvol = kGaussWtTet * g.jac;
        const double N[4] = {0.25, 0.25, 1.0 - 0.25 - 0.25 - 0.25, 0.25};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double b4 = (dens * dvol) * N[a];
            double fact = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) fact = fact + b4 * N[j];
            Mn[a] = fact;
        }
        return true;
    }
    TriaGeom g;
    tria_geometry(x, y, g);
    if (kind != 4 && g.jac < 0.0) return false;
    const double dvol = kind == 5 ? 0.5 * (g.jac * ed[2]) : 0.5 * g.jac;
    double N[3];
    tria_shape_gp(N);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double b4 = (dens * dvol) * N[a];
        double fact = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) fact = fact + b4 * N[j];
        Mn[a] = fact;
    }
    return true;
}

// ---------------------------------------------------------------------------
// Geometric stiffness of the elasticity kinds (pfem_elem_geometric / pfem_buckling_setup).  With a stress
// sig that is constant over the constant-strain element, K_g couples equal displacement components only:
//     K_g[(a,i),(b,j)] = delta_ij g_ab,      g_ab = dvol * (grad N_a . (sig grad N_b))
// Written-down order, host and device the same bits (no contraction):
//   tet       sig = [xx,yy,zz,xy,yz,zx];  t = sig grad N_b:  tx = (sxx bx + sxy by) + szx bz,  ty = (sxy bx + syy by) + syz bz,
//             tz = (szx bx + syz by) + szz bz;      g_ab = dvol * ((ax tx + ay ty) + az tz)
//   triangle  sig = [xx,yy,xy];  tx = sxx bx + sxy by,  ty = sxy bx + syy by;      g_ab = dvol * (ax tx + ay ty)
// sig is in the order elem_post stores `flux`, and for the triangle it IS that flux: the plane-stress shear stress as the
// library reports it, with the reference's D(3,3) = b1 (1 - nu) (elast_tria_post_t above).  The triangle's K_g describes
// in-plane instability only: a plane-stress element has no out-of-plane displacement to buckle into.  dvol and grad N are those
// of the kind's stiffness routine (thickness ed[2] in the triangle's dvol).  g[a + npe * b].  Kinds 3 and 5 only (the caller
// checks).  false: a negative Jacobian.
// ---------------------------------------------------------------------------
PFEM_HD bool elem_geometric(int kind, const double *x, const double *y, const double *z, const double *ed, const double *sig, double *g)
{
    if (kind == 3) {
        TetGeom q;
        tet_geometry(x, y, z, q);
        if (q.jac < 0.0) return false;
        const double dvol = kGaussWtTet * q.jac;
        const double sxx = sig[0], syy = sig[1], szz = sig[2], sxy = sig[3], syz = sig[4], szx = sig[5];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double bx = q.gx[b], by = q.gy[b], bz = q.gz[b];
            const double tx = (sxx * bx + sxy * by) + szx * bz;
            const double ty = (sxy * bx + syy * by) + syz * bz;
            const double tz = (szx * bx + syz * by) + szz * bz;
#pragma unroll
            for (int a = 0; a < 4; ++a) g[a + 4 * b] = dvol * ((q.gx[a] * tx + q.gy[a] * ty) + q.gz[a] * tz);
        }
        return true;
    }
    TriaGeom q;
    tria_geometry(x, y, q);
    if (q.jac < 0.0) return false;
    const double dvol = 0.5 * (q.jac * ed[2]);
    const double sxx = sig[0], syy = sig[1], sxy = sig[2];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double bx = q.gx[b], by = q.gy[b];
        const double tx = sxx * bx + sxy * by;
        const double ty = sxy * bx + syy * by;
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a + 3 * b] = dvol * (q.gx[a] * tx + q.gy[a] * ty);
    }
    return true;
}

// ---------------------------------------------------------------------------
// Sides of an element and the loads on them (pfem_face_load / pfem_surface_geometry / pfem_rhs_add_surface_load)
// ---------------------------------------------------------------------------
// Side f of an element is the face (tet) or edge (triangle) OPPOSITE local node f; its nodes are the element's other local
// nodes in ascending local order: s[0] < s[1] (< s[2]).  Written-down order of operations, host and device the same bits:
//   tet       e1 = P_s1 - P_s0, e2 = P_s2 - P_s0, c = e1 x e2 with c_x = e1y e2z - e1z e2y (and cyclic), len = sqrt((c_x^2 +
//             c_y^2) + c_z^2), measure = 0.5 len, d = ((P_f - P_s0)_x c_x + (..)_y c_y) + (..)_z c_z
//   triangle  t = P_s1 - P_s0, c = (t_y, -t_x), len = sqrt(t_x^2 + t_y^2), measure = len, d = (P_f - P_s0)_x c_x + (..)_y c_y
//   normal    n = c / len when d < 0 (c already points away from node f), (-c) / len when d > 0
// The orientation comes from the opposite node alone -- never from the order of the nodes, so an inverted element has
// outward normals too.  false: a side of zero measure, or an element so flat (d == 0) that "outward" has no meaning.
// The routines take the side's points in that order (xs[a], a < npe - 1) and the opposite node's point apart, so that no array
// is ever indexed by the run-time side number (registers, not scratch, on the device).
PFEM_HD void side_nodes(int npe, int f, int s[3])
{
    s[0] = f == 0 ? 1 : 0;
    s[1] = f <= 1 ? 2 : 1;
    s[2] = npe == 4 ? (f <= 2 ? 3 : 2) : 0;
}

PFEM_HD bool side_geometry(int npe, const double xs[3], const double ys[3], const double zs[3], double xo, double yo, double zo,
                           double &measure, double nrm[3])
{
    double cx, cy, cz, len, d;
    if (npe == 4) {
        const double e1x = xs[1] - xs[0], e1y = ys[1] - ys[0], e1z = zs[1] - zs[0];
        const double e2x = xs[2] - xs[0], e2y = ys[2] - ys[0], e2z = zs[2] - zs[0];
        cx = e1y * e2z - e1z * e2y;
        cy = e1z * e2x - e1x * e2z;
        cz = e1x * e2y - e1y * e2x;
        len = sqrt((cx * cx + cy * cy) + cz * cz);
        measure = 0.5 * len;
        d = ((xo - xs[0]) * cx + (yo - ys[0]) * cy) + (zo - zs[0]) * cz;
    } else {
        const double tx = xs[1] - xs[0], ty = ys[1] - ys[0];
        cx = ty;
        cy = -tx;
        cz = 0.0;
        len = sqrt(tx * tx + ty * ty);
        measure = len;
        d = (xo - xs[0]) * cx + (yo - ys[0]) * cy;
    }
    if (!(len > 0.0) || !(d > 0.0 || d < 0.0)) return false;
    if (d > 0.0) { cx = -cx; cy = -cy; cz = -cz; }
    nrm[0] = cx / len;
    nrm[1] = cy / len;
    nrm[2] = cz / len;
    return true;
}

// load kinds and components of a side's nodal values (kinds of include/pfem_amd.h: PFEM_LOAD_FLUX 1, _TRACTION 2, _PRESSURE 3);
// 0: the load does not fit the element kind
PFEM_HD int side_load_components(int kind, int load)
{
    const bool elast = kind == 3 || kind == 5;
    if (load == 1) return elast ? 0 : 1;
    if (load == 2) return elast ? (kind == 3 ? 3 : 2) : 0;
    if (load == 3) return elast ? 1 : 0;
    return 0;
}

// Consistent nodal load of a P1 side from its nodal values vals[a * ncomp + c], a over the side's nodes in ascending local order:
// the exact integral of N_a g for g linear on the side,
//   tet       F_a = A / 12 (2 g_a + g_b + g_c)      evaluated as  (A * ((2 g_a + g_b) + g_c)) / 12
//   triangle  F_a = L thick / 6 (2 g_a + g_b)       evaluated as  ((L * thick) * (2 g_a + g_b)) / 6
// with b, c the side's other nodes in ascending local order.  The division comes LAST: where measure times the bracket is exact
// and the quotient representable (the reference's Cook's-membrane forces 3.125 and 1.5625), the result is the exact one.
// A pressure p is the traction -p n: g_a,c = -(p_a n_c), then the same expression.  A flux has one component and lands on the
// node's single dof.  Fs[a * ndof + c]: the side's nodes only (the opposite node gets nothing).  thick: 1 except for the
// plane-stress triangle.  measure and nrm must be side_geometry's.
PFEM_HD void side_load(int kind, int load, double measure, const double nrm[3], const double *vals, double thick, double Fs[9])
{
    const int npe = (kind == 2 || kind == 3) ? 4 : 3;
    const int ndof = kind == 3 ? 3 : (kind == 5 ? 2 : 1);
    const int ncomp = load == 2 ? ndof : 1;
    const double m = npe == 4 ? measure : measure * thick;
    if (npe == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= ndof) break;
            const double g0 = load == 3 ? -(vals[0] * nrm[c]) : vals[c];
            const double g1 = load == 3 ? -(vals[1] * nrm[c]) : vals[ncomp + c];
            const double g2 = load == 3 ? -(vals[2] * nrm[c]) : vals[2 * ncomp + c];
            Fs[c] = (m * ((2.0 * g0 + g1) + g2)) / 12.0;
            Fs[ndof + c] = (m * ((2.0 * g1 + g0) + g2)) / 12.0;
            Fs[2 * ndof + c] = (m * ((2.0 * g2 + g0) + g1)) / 12.0;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c >= ndof) break;
            const double g0 = load == 3 ? -(vals[0] * nrm[c]) : vals[c];
            const double g1 = load == 3 ? -(vals[1] * nrm[c]) : vals[ncomp + c];
            Fs[c] = (m * (2.0 * g0 + g1)) / 6.0;
            Fs[ndof + c] = (m * (2.0 * g1 + g0)) / 6.0;
        }
    }
}

}  // namespace pfem

// Stand-alone walk of pfem_elem_lumped_mass (pfem_host.cpp + pfem_elem.hpp's elem_lumped_mass) for AddressSanitizer / UBSan:
// every kind on exact-size buffers (a write past Mlocal[npe * ndof], a read past the coordinates or past elemData[3] is a heap
// overflow here), the sum of the node shares against density x measure, and the error returns.  Prints "dynamics_sanitize: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/pfem_amd.h"

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

int main()
{
    const int kinds[5] = {PFEM_POISSON_TRIA, PFEM_POISSON_TET, PFEM_ELAST_TET, PFEM_POISSON_TRIA_INLINE, PFEM_ELAST_TRIA};
    const double X[4] = {0.1, 1.3, 0.2, 0.4}, Y[4] = {0.0, 0.2, 1.1, 0.3}, Z[4] = {0.05, -0.1, 0.2, 1.2};
    const double area = 0.5 * ((1.3 - 0.1) * (1.1 - 0.0) - (0.2 - 0.0) * (0.2 - 0.1));
    for (int kind : kinds) {
        const bool tet = kind == PFEM_POISSON_TET || kind == PFEM_ELAST_TET;
        const int npe = tet ? 4 : 3;
        const int ndof = kind == PFEM_ELAST_TET ? 3 : (kind == PFEM_ELAST_TRIA ? 2 : 1);
        std::vector<double> x(X, X + npe), y(Y, Y + npe), z(Z, Z + npe);
        std::vector<double> ed = {10.0, 0.25, 0.5};                     // E, nu, thick: exactly the three entries read
        const double *edp = kind == PFEM_ELAST_TRIA ? ed.data() : nullptr;
        std::vector<double> M(static_cast<size_t>(npe * ndof), -7.0);
        CHECK(pfem_elem_lumped_mass(kind, x.data(), y.data(), tet ? z.data() : nullptr, edp, 2.5, M.data()) == PFEM_OK);
        double sum = 0.0;
        for (int a = 0; a < npe; ++a) {
            sum += M[static_cast<size_t>(a * ndof)];
            CHECK(M[static_cast<size_t>(a * ndof)] > 0.0);
            for (int d = 1; d < ndof; ++d) CHECK(M[static_cast<size_t>(a * ndof + d)] == M[static_cast<size_t>(a * ndof)]);
        }
        // density x measure, to the accuracy of the reference's REAL(4) Gauss data
        const double measure = tet ? 1.495 / 6.0 : area * (kind == PFEM_ELAST_TRIA ? 0.5 : 1.0);
        CHECK(std::fabs(sum - 2.5 * measure) < 1e-6 * 2.5 * measure);
        // errors
        CHECK(pfem_elem_lumped_mass(kind, nullptr, y.data(), tet ? z.data() : nullptr, edp, 2.5, M.data()) == PFEM_ERR_ARG);
        CHECK(pfem_elem_lumped_mass(kind, x.data(), nullptr, tet ? z.data() : nullptr, edp, 2.5, M.data()) == PFEM_ERR_ARG);
        CHECK(pfem_elem_lumped_mass(kind, x.data(), y.data(), tet ? z.data() : nullptr, edp, 2.5, nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_elem_lumped_mass(kind, x.data(), y.data(), tet ? z.data() : nullptr, edp, 0.0, M.data()) == PFEM_ERR_ARG);
        CHECK(pfem_elem_lumped_mass(kind, x.data(), y.data(), tet ? z.data() : nullptr, edp, -1.0, M.data()) == PFEM_ERR_ARG);
        CHECK(pfem_elem_lumped_mass(kind, x.data(), y.data(), tet ? z.data() : nullptr, edp, std::nan(""), M.data()) == PFEM_ERR_ARG);
        if (tet) CHECK(pfem_elem_lumped_mass(kind, x.data(), y.data(), nullptr, edp, 2.5, M.data()) == PFEM_ERR_ARG);
        if (kind == PFEM_ELAST_TRIA) CHECK(pfem_elem_lumped_mass(kind, x.data(), y.data(), nullptr, nullptr, 2.5, M.data()) == PFEM_ERR_ARG);
        // an inverted element: two nodes swapped (the inline triangle has no orientation test)
        std::vector<double> xs = x, ys = y, zs = z;
        std::swap(xs[0], xs[1]); std::swap(ys[0], ys[1]); std::swap(zs[0], zs[1]);
        CHECK(pfem_elem_lumped_mass(kind, xs.data(), ys.data(), tet ? zs.data() : nullptr, edp, 2.5, M.data()) ==
              (kind == PFEM_POISSON_TRIA_INLINE ? PFEM_OK : PFEM_ERR_NEG_JAC));
    }
    double M[12];
    CHECK(pfem_elem_lumped_mass(0, X, Y, Z, nullptr, 1.0, M) == PFEM_ERR_ARG);
    CHECK(pfem_elem_lumped_mass(6, X, Y, Z, nullptr, 1.0, M) == PFEM_ERR_ARG);
    if (fails) return 1;
    std::printf("dynamics_sanitize: ok\n");
    return 0;
}

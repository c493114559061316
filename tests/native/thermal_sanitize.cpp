// Stand-alone walk of pfem_elem_thermal_load and pfem_elem_post_thermal (pfem_host.cpp + pfem_elem.hpp's thermal arithmetic) for
// AddressSanitizer / UBSan: both elasticity kinds in both orientations, exact-size buffers (a write past F[nsize], sigma_th[ng] or a
// read past theta[npe], elemData[2 or 3] is a heap overflow here), NULL outputs, and the error returns.
// Prints "thermal_sanitize: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../include/pfem_amd.h"

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

int main()
{
    const double X[4] = {0.1, 1.3, 0.2, 0.4}, Y[4] = {0.0, 0.2, 1.1, 0.3}, Z[4] = {0.05, -0.1, 0.2, 1.2};
    for (int kind : {PFEM_ELAST_TET, PFEM_ELAST_TRIA}) {
        const bool tet = kind == PFEM_ELAST_TET;
        const int npe = tet ? 4 : 3, ndof = tet ? 3 : 2, ng = tet ? 6 : 3, nsize = npe * ndof;
        std::vector<double> x(X, X + npe), y(Y, Y + npe), z(Z, Z + npe);
        std::vector<double> ed = {10.0, 0.25};                          // E, nu: the entries the tet reads
        if (!tet) ed.push_back(0.5);                                    // ... and the triangle's thickness
        std::vector<double> theta(static_cast<size_t>(npe)), valC(static_cast<size_t>(nsize));
        for (int a = 0; a < npe; ++a) theta[static_cast<size_t>(a)] = 10.0 + 3.0 * a;
        for (int i = 0; i < nsize; ++i) valC[static_cast<size_t>(i)] = 0.01 * (i + 1);
        const double alpha = 1.0e-3;
        int ok = 0, inverted = 0;
        for (int flip = 0; flip < 2; ++flip) {
            if (flip) { std::swap(x[0], x[1]); std::swap(y[0], y[1]); std::swap(z[0], z[1]); }
            std::vector<double> F(static_cast<size_t>(nsize), -7.0), sg(static_cast<size_t>(ng), -7.0);
            const int rc = pfem_elem_thermal_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), alpha, theta.data(), F.data(), sg.data());
            CHECK(rc == PFEM_OK || rc == PFEM_ERR_NEG_JAC);
            std::vector<double> g(static_cast<size_t>(ng)), f(static_cast<size_t>(ng)), fi(static_cast<size_t>(nsize));
            double sc = -1.0;
            const int rp = pfem_elem_post_thermal(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), valC.data(), alpha, theta.data(), g.data(),
                                                  f.data(), &sc, fi.data());
            CHECK(rp == rc);
            if (rc == PFEM_ERR_NEG_JAC) { ++inverted; continue; }
            ++ok;
            // the load is self-equilibrated, the stress has no shear, sigma_th's normals agree to rounding
            for (int d = 0; d < ndof; ++d) {
                double sum = 0.0, mag = 0.0;
                for (int a = 0; a < npe; ++a) { sum += F[static_cast<size_t>(a * ndof + d)]; mag += std::fabs(F[static_cast<size_t>(a * ndof + d)]); }
                CHECK(std::fabs(sum) <= 1e-14 * mag);
            }
            CHECK(sg[0] > 0.0 && sg[0] == sg[1]);
            for (int c = ndof; c < ng; ++c) CHECK(sg[static_cast<size_t>(c)] == 0.0);
            CHECK(sc >= 0.0);
            // every output on its own, the others NULL
            CHECK(pfem_elem_thermal_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), alpha, theta.data(), F.data(), nullptr) == PFEM_OK);
            CHECK(pfem_elem_thermal_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), alpha, theta.data(), nullptr, sg.data()) == PFEM_OK);
            CHECK(pfem_elem_thermal_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), alpha, theta.data(), nullptr, nullptr) == PFEM_OK);
            CHECK(pfem_elem_post_thermal(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), valC.data(), alpha, theta.data(), nullptr, f.data(),
                                         nullptr, nullptr) == PFEM_OK);
            CHECK(pfem_elem_post_thermal(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), valC.data(), alpha, theta.data(), nullptr, nullptr,
                                         nullptr, nullptr) == PFEM_OK);
            // alpha = 0: the plain routine's bits
            std::vector<double> f0(static_cast<size_t>(ng));
            CHECK(pfem_elem_post(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), valC.data(), nullptr, f0.data(), nullptr, nullptr) == PFEM_OK);
            CHECK(pfem_elem_post_thermal(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), valC.data(), 0.0, theta.data(), nullptr, f.data(),
                                         nullptr, nullptr) == PFEM_OK);
            for (int c = 0; c < ng; ++c) CHECK(f[static_cast<size_t>(c)] == f0[static_cast<size_t>(c)]);
        }
        CHECK(ok == 1 && inverted == 1);
        // errors
        std::vector<double> F(static_cast<size_t>(nsize));
        CHECK(pfem_elem_thermal_load(kind, nullptr, y.data(), z.data(), ed.data(), alpha, theta.data(), F.data(), nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_elem_thermal_load(kind, x.data(), y.data(), z.data(), nullptr, alpha, theta.data(), F.data(), nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_elem_thermal_load(kind, x.data(), y.data(), z.data(), ed.data(), alpha, nullptr, F.data(), nullptr) == PFEM_ERR_ARG);
        if (tet) CHECK(pfem_elem_thermal_load(kind, x.data(), y.data(), nullptr, ed.data(), alpha, theta.data(), F.data(), nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_elem_post_thermal(kind, x.data(), y.data(), z.data(), ed.data(), nullptr, alpha, theta.data(), nullptr, nullptr, nullptr, nullptr) == PFEM_ERR_ARG);
    }
    for (int kind : {0, PFEM_POISSON_TRIA, PFEM_POISSON_TET, PFEM_POISSON_TRIA_INLINE, 6}) {
        double F[12], th[4] = {1, 2, 3, 4}, ed[3] = {1, 1, 1}, v[4] = {0, 0, 0, 0};
        CHECK(pfem_elem_thermal_load(kind, X, Y, Z, ed, 1e-3, th, F, nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_elem_post_thermal(kind, X, Y, Z, ed, v, 1e-3, th, nullptr, F, nullptr, nullptr) == PFEM_ERR_ARG);
    }
    if (fails) return 1;
    std::printf("thermal_sanitize: ok\n");
    return 0;
}

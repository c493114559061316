// Stand-alone walk of pfem_elem_geometric (pfem_host.cpp + pfem_elem.hpp's elem_geometric) for AddressSanitizer / UBSan: both
// elasticity kinds in both orientations on exact-size buffers (a write past Kg[npe * npe] or a read past sigma[ng], the
// coordinates or elemData[3] is a heap overflow here), the tet without elemData, and the error returns.
// Prints "buckling_sanitize: ok".
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
    const double S[6] = {-3.0, 0.7, 1.1, 0.4, -0.2, 0.9};
    for (int kind : {PFEM_ELAST_TET, PFEM_ELAST_TRIA}) {
        const bool tet = kind == PFEM_ELAST_TET;
        const int npe = tet ? 4 : 3, ng = tet ? 6 : 3;
        std::vector<double> x(X, X + npe), y(Y, Y + npe), z(Z, Z + npe), sg(S, S + ng);
        std::vector<double> ed = {10.0, 0.25, 0.5};                     // E, nu, thickness: what the triangle reads
        int ok = 0, inverted = 0;
        for (int flip = 0; flip < 2; ++flip) {
            if (flip) { std::swap(x[0], x[1]); std::swap(y[0], y[1]); std::swap(z[0], z[1]); }
            std::vector<double> g(static_cast<size_t>(npe * npe), -7.0);
            const int rc = pfem_elem_geometric(kind, x.data(), y.data(), tet ? z.data() : nullptr, ed.data(), sg.data(), g.data());
            CHECK(rc == PFEM_OK || rc == PFEM_ERR_NEG_JAC);
            if (rc == PFEM_ERR_NEG_JAC) {
                ++inverted;
                for (double v : g) CHECK(v == -7.0);                  // nothing written
                continue;
            }
            ++ok;
            double big = 0.0;
            for (double v : g) big = std::fmax(big, std::fabs(v));
            CHECK(big > 0.0);
            for (int a = 0; a < npe; ++a) {
                double row = 0.0, col = 0.0;
                for (int b = 0; b < npe; ++b) {
                    row += g[static_cast<size_t>(a + npe * b)];
                    col += g[static_cast<size_t>(b + npe * a)];
                    CHECK(std::fabs(g[static_cast<size_t>(a + npe * b)] - g[static_cast<size_t>(b + npe * a)]) <= 1e-13 * big);
                }
                CHECK(std::fabs(row) <= 1e-13 * big && std::fabs(col) <= 1e-13 * big);       // rigid translations
            }
            // the stress scales it; the tet reads no elemData
            std::vector<double> s2(sg), g2(g.size());
            for (double &v : s2) v *= 2.0;
            CHECK(pfem_elem_geometric(kind, x.data(), y.data(), tet ? z.data() : nullptr, tet ? nullptr : ed.data(), s2.data(), g2.data()) == PFEM_OK);
            for (size_t i = 0; i < g.size(); ++i) CHECK(g2[i] == 2.0 * g[i]);
        }
        CHECK(ok == 1 && inverted == 1);
        std::vector<double> g(static_cast<size_t>(npe * npe));
        CHECK(pfem_elem_geometric(kind, nullptr, y.data(), z.data(), ed.data(), sg.data(), g.data()) == PFEM_ERR_ARG);
        CHECK(pfem_elem_geometric(kind, x.data(), nullptr, z.data(), ed.data(), sg.data(), g.data()) == PFEM_ERR_ARG);
        CHECK(pfem_elem_geometric(kind, x.data(), y.data(), z.data(), ed.data(), nullptr, g.data()) == PFEM_ERR_ARG);
        CHECK(pfem_elem_geometric(kind, x.data(), y.data(), z.data(), ed.data(), sg.data(), nullptr) == PFEM_ERR_ARG);
        if (tet) CHECK(pfem_elem_geometric(kind, x.data(), y.data(), nullptr, ed.data(), sg.data(), g.data()) == PFEM_ERR_ARG);
        else CHECK(pfem_elem_geometric(kind, x.data(), y.data(), nullptr, nullptr, sg.data(), g.data()) == PFEM_ERR_ARG);
    }
    for (int kind : {0, PFEM_POISSON_TRIA, PFEM_POISSON_TET, PFEM_POISSON_TRIA_INLINE, 6}) {
        double g[16], ed[3] = {1, 1, 1};
        CHECK(pfem_elem_geometric(kind, X, Y, Z, ed, S, g) == PFEM_ERR_ARG);
    }
    if (fails) return 1;
    std::printf("buckling_sanitize: ok\n");
    return 0;
}

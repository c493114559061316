// Stand-alone walk of pfem_face_load (pfem_host.cpp + pfem_elem.hpp's side arithmetic) for AddressSanitizer / UBSan: every
// kind, side and load, exact-size buffers (a write past F[nsize], values[(npe-1)*ncomp] or normal[ndim] is a heap overflow
// here), NULL outputs, and the error returns.  Prints "surface_sanitize: ok".
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
    for (int kind : kinds) {
        const bool tet = kind == PFEM_POISSON_TET || kind == PFEM_ELAST_TET;
        const int npe = tet ? 4 : 3, ndim = tet ? 3 : 2;
        const int ndof = kind == PFEM_ELAST_TET ? 3 : (kind == PFEM_ELAST_TRIA ? 2 : 1);
        const bool elast = ndof > 1;
        std::vector<double> x(X, X + npe), y(Y, Y + npe), z(Z, Z + npe);
        std::vector<double> ed = {10.0, 0.25, 0.5};                     // E, nu, thick: exactly the three entries read
        for (int side = 0; side < npe; ++side) {
            for (int load = PFEM_LOAD_FLUX; load <= PFEM_LOAD_PRESSURE; ++load) {
                const bool fits = elast ? load != PFEM_LOAD_FLUX : load == PFEM_LOAD_FLUX;
                const int ncomp = load == PFEM_LOAD_TRACTION ? ndof : 1;
                std::vector<double> vals(static_cast<size_t>((npe - 1) * ncomp)), F(static_cast<size_t>(npe * ndof), -7.0), nrm(static_cast<size_t>(ndim));
                for (size_t i = 0; i < vals.size(); ++i) vals[i] = 1.0 + 0.5 * static_cast<double>(i);
                double meas = -1.0;
                const int rc = pfem_face_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, side, load, vals.data(),
                                              kind == PFEM_ELAST_TRIA ? ed.data() : nullptr, F.data(), &meas, nrm.data());
                CHECK(rc == (fits ? PFEM_OK : PFEM_ERR_ARG));
                if (!fits) continue;
                CHECK(meas > 0.0);
                double n2 = 0.0;
                for (int c = 0; c < ndim; ++c) n2 += nrm[static_cast<size_t>(c)] * nrm[static_cast<size_t>(c)];
                CHECK(std::fabs(n2 - 1.0) < 1e-14);
                for (int d = 0; d < ndof; ++d) CHECK(F[static_cast<size_t>(side * ndof + d)] == 0.0);
                // every output on its own, the others NULL
                CHECK(pfem_face_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, side, load, vals.data(),
                                     kind == PFEM_ELAST_TRIA ? ed.data() : nullptr, F.data(), nullptr, nullptr) == PFEM_OK);
                CHECK(pfem_face_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, side, 0, nullptr, nullptr, nullptr, &meas, nullptr) == PFEM_OK);
                CHECK(pfem_face_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, side, 0, nullptr, nullptr, nullptr, nullptr, nrm.data()) == PFEM_OK);
            }
        }
        // errors
        double meas = 0.0;
        CHECK(pfem_face_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, -1, 0, nullptr, nullptr, nullptr, &meas, nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_face_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, npe, 0, nullptr, nullptr, nullptr, &meas, nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_face_load(kind, nullptr, y.data(), tet ? z.data() : nullptr, 0, 0, nullptr, nullptr, nullptr, &meas, nullptr) == PFEM_ERR_ARG);
        if (tet) CHECK(pfem_face_load(kind, x.data(), y.data(), nullptr, 0, 0, nullptr, nullptr, nullptr, &meas, nullptr) == PFEM_ERR_ARG);
        std::vector<double> F(static_cast<size_t>(npe * ndof));
        CHECK(pfem_face_load(kind, x.data(), y.data(), tet ? z.data() : nullptr, 0, elast ? PFEM_LOAD_PRESSURE : PFEM_LOAD_FLUX, nullptr,
                             ed.data(), F.data(), nullptr, nullptr) == PFEM_ERR_ARG);        // a load without values
        if (kind == PFEM_ELAST_TRIA) {
            const double p[2] = {1.0, 2.0};
            CHECK(pfem_face_load(kind, x.data(), y.data(), nullptr, 0, PFEM_LOAD_PRESSURE, p, nullptr, F.data(), nullptr, nullptr) == PFEM_ERR_ARG);
        }
        // a side of zero measure: two of its nodes in one place
        std::vector<double> xd = x, yd = y, zd = z;
        xd[1] = xd[2]; yd[1] = yd[2]; zd[1] = zd[2];
        CHECK(pfem_face_load(kind, xd.data(), yd.data(), tet ? zd.data() : nullptr, 0, 0, nullptr, nullptr, nullptr, &meas, nullptr) == PFEM_ERR_NEG_JAC);
    }
    CHECK(pfem_face_load(0, X, Y, Z, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == PFEM_ERR_ARG);
    CHECK(pfem_face_load(6, X, Y, Z, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == PFEM_ERR_ARG);
    if (fails) return 1;
    std::printf("surface_sanitize: ok\n");
    return 0;
}

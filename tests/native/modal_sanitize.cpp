// Stand-alone walk of pfem_dense_sym_geneig (pfem_host.cpp) for AddressSanitizer / UBSan: orders 1, 47 and 48 on exact-size heap
// buffers (a read past A[n * n] or a write past w[n] / C[n * n] is a heap overflow here), the residual A C - B C diag(w) and
// C^T B C = I of what comes back, the "singular" status on a duplicated column, and the argument errors.  Prints
// "modal_sanitize: ok".
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

static double rnd(unsigned long long &st)
{
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(st >> 11) * 0x1.0p-53 - 0.5;
}

// G^T G / n + shift I for a random G: symmetric positive definite, full storage
static std::vector<double> spd(int n, double shift, unsigned long long &st)
{
    std::vector<double> G(static_cast<size_t>(n) * n), M(static_cast<size_t>(n) * n);
    for (double &g : G) g = rnd(st);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double a = 0.0;
            for (int k = 0; k < n; ++k) a += G[static_cast<size_t>(k) * n + i] * G[static_cast<size_t>(k) * n + j];
            M[static_cast<size_t>(i) * n + j] = a / n + (i == j ? shift : 0.0);
        }
    return M;
}

int main()
{
    unsigned long long st = 12345;
    for (int n : {1, 47, 48}) {
        const size_t nn = static_cast<size_t>(n) * n;
        std::vector<double> A = spd(n, 0.5, st), B = spd(n, 1.0, st), w(static_cast<size_t>(n), -7.0), C(nn, -7.0);
        int status = -1;
        CHECK(pfem_dense_sym_geneig(n, A.data(), B.data(), 1e-12, w.data(), C.data(), &status) == PFEM_OK);
        CHECK(status == 0);
        double worst_r = 0.0, worst_o = 0.0;
        for (int k = 0; k < n; ++k) {
            CHECK(w[static_cast<size_t>(k)] > 0.0);
            if (k > 0) CHECK(w[static_cast<size_t>(k)] >= w[static_cast<size_t>(k) - 1]);
            for (int i = 0; i < n; ++i) {
                double ac = 0.0, bc = 0.0;
                for (int j = 0; j < n; ++j) {
                    ac += A[static_cast<size_t>(i) * n + j] * C[static_cast<size_t>(j) * n + k];
                    bc += B[static_cast<size_t>(i) * n + j] * C[static_cast<size_t>(j) * n + k];
                }
                worst_r = std::fmax(worst_r, std::fabs(ac - w[static_cast<size_t>(k)] * bc));
            }
            for (int l = 0; l < n; ++l) {
                double o = 0.0;
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j) o += C[static_cast<size_t>(i) * n + k] * B[static_cast<size_t>(i) * n + j] * C[static_cast<size_t>(j) * n + l];
                worst_o = std::fmax(worst_o, std::fabs(o - (k == l ? 1.0 : 0.0)));
            }
        }
        CHECK(worst_r < 1e-11);
        CHECK(worst_o < 1e-11);
        // errors: nothing may be read or written
        CHECK(pfem_dense_sym_geneig(n, nullptr, B.data(), 1e-12, w.data(), C.data(), &status) == PFEM_ERR_ARG);
        CHECK(pfem_dense_sym_geneig(n, A.data(), nullptr, 1e-12, w.data(), C.data(), &status) == PFEM_ERR_ARG);
        CHECK(pfem_dense_sym_geneig(n, A.data(), B.data(), 1e-12, nullptr, C.data(), &status) == PFEM_ERR_ARG);
        CHECK(pfem_dense_sym_geneig(n, A.data(), B.data(), 1e-12, w.data(), nullptr, &status) == PFEM_ERR_ARG);
        CHECK(pfem_dense_sym_geneig(n, A.data(), B.data(), 1e-12, w.data(), C.data(), nullptr) == PFEM_ERR_ARG);
        CHECK(pfem_dense_sym_geneig(n, A.data(), B.data(), -1.0, w.data(), C.data(), &status) == PFEM_ERR_ARG);
        CHECK(pfem_dense_sym_geneig(n, A.data(), B.data(), std::nan(""), w.data(), C.data(), &status) == PFEM_ERR_ARG);
        if (n > 1) {                       // column and row n - 1 of B made equal to column and row 0: singular, outputs untouched
            std::vector<double> Bs = B, w2(static_cast<size_t>(n), -7.0), C2(nn, -7.0);
            for (int i = 0; i < n; ++i) Bs[static_cast<size_t>(i) * n + n - 1] = Bs[static_cast<size_t>(n - 1) * n + i] = B[static_cast<size_t>(i) * n];
            Bs[nn - 1] = B[0];
            status = -1;
            CHECK(pfem_dense_sym_geneig(n, A.data(), Bs.data(), 1e-12, w2.data(), C2.data(), &status) == PFEM_OK);
            CHECK(status == 1);
            for (double v : w2) CHECK(v == -7.0);
            for (double v : C2) CHECK(v == -7.0);
        }
    }
    double one = 1.0, w = 0.0, c = 0.0;
    int status = -1;
    CHECK(pfem_dense_sym_geneig(0, &one, &one, 0.0, &w, &c, &status) == PFEM_ERR_ARG);
    CHECK(pfem_dense_sym_geneig(-3, &one, &one, 0.0, &w, &c, &status) == PFEM_ERR_ARG);
    CHECK(pfem_dense_sym_geneig(PFEM_GENEIG_MAX + 1, &one, &one, 0.0, &w, &c, &status) == PFEM_ERR_ARG);
    const double zero = 0.0;
    CHECK(pfem_dense_sym_geneig(1, &one, &zero, 0.0, &w, &c, &status) == PFEM_OK && status == 1);
    if (fails) return 1;
    std::printf("modal_sanitize: ok\n");
    return 0;
}

// pfem_buckling_kernels.hpp -- gfx950 kernels of the linear buckling analysis (pfem_buckling_setup / pfem_buckling_solve;
// DESIGN.md section 15): the scatter assembly of the geometric stiffness K_g on K's pattern, and the block kernels of LOBPCG on
// the pencil (K_g, K), whose second matrix is a sparse matrix and not a diagonal -- so that S = [X W P] travels with TWO product
// families, K S and K_g S.  Block layout (n x MB doubles, row-major), tile sizes and grid caps are those of the modal kernels
// (pfem_modal_kernels.hpp); the products themselves are k_spmm<MB> of that header, once with K's values and once with K_g's.
// Every sum of the block kernels is taken in a fixed order -- per thread, then over the threads of a block by index, then over
// the blocks by index (k_modal_sum) -- without atomics: the same bits in every run.  k_geo_assemble is the scatter form: f64
// atomics, the order of the sums varies from run to run.
#pragma once

#include "pfem_modal_kernels.hpp"

namespace pfem {

// doubles of k_buck_gram's LDS buffer: three row tiles (S, K S, K_g S) of kModalGramTile x (3 MB + 1) at MB = 16, which also
// covers the 256 threads' 3 x 3 tiles of both matrices at the end (256 x 18)
constexpr int kBuckGramLds = 3 * kModalGramTile * (3 * 16 + 1);
static_assert(kBuckGramLds >= 256 * 18, "the partial tiles of the row groups fit the buffer");

// K_g of one element into the value array A.vals on K's row form (zeroed before the launch).  One thread per element: the
// element's npe^2 scalars g_ab from its stress stress[c * nElem + e] (pfem_elem.hpp: elem_geometric, the host's bits), and for
// every component i the entry (row = dof(b,i), col = dof(a,i)) += g_ab when both dofs are free.  A constrained dof has no row
// and no column: there is no lifting in an eigenproblem.  PRM gives the element's elemData (the triangle's thickness).
template <int KIND, class PRM>
__global__ void __launch_bounds__(kBlock) k_geo_assemble(MeshDev m, SellDev A, PRM prm, const double *__restrict__ stress, int *err)
{
    using P = PostKind<KIND>;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= m.nElem) return;
    int nd[4] = {0, 0, 0, 0}, dof[P::NPE * P::NDOF];
    double x[4], y[4], z[4], sig[6], g[16];
#pragma unroll
    for (int a = 0; a < P::NPE; ++a) {
        nd[a] = m.conn[a * m.nElem + e];
        x[a] = m.xyz[nd[a]];
        y[a] = m.xyz[m.nNode + nd[a]];
        z[a] = P::NDIM == 3 ? m.xyz[2 * m.nNode + nd[a]] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < P::NPE * P::NDOF; ++i) dof[i] = m.edof[i * m.nElem + e];
#pragma unroll
    for (int c = 0; c < P::NG; ++c) sig[c] = stress[c * m.nElem + e];
    if (!elem_geometric(KIND, x, y, z, prm_at(prm, AtElem{e}), sig, g)) { atomicMax(err, PFEM_ERR_NEG_JAC); return; }
#pragma unroll
    for (int b = 0; b < P::NPE; ++b)
#pragma unroll
        for (int a = 0; a < P::NPE; ++a)
#pragma unroll
            for (int i = 0; i < P::NDOF; ++i) {
                const int row = dof[P::NDOF * b + i], col = dof[P::NDOF * a + i];
                if (row < 0 || col < 0) continue;
                const int64_t sl = find_slot(A, row, col);
                if (sl < 0) { atomicMax(err, PFEM_ERR_PATTERN); continue; }
                add_f64(&A.vals[sl], g[a + P::NPE * b]);
            }
}

// R = K_g X - (K X) diag(theta), W = dinv o R (dinv == nullptr: W = R, for a T applied afterwards), and per block the partial
// sums of ||R_j||^2, ||K_g X_j||^2 and ||K X_j||^2: part[block][3][MB].  Thread t owns column t % MB throughout.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_buck_residual(int64_t n, const double *__restrict__ GX, const double *__restrict__ KX, const double *__restrict__ dinv,
                                                          const double *__restrict__ theta, double *__restrict__ W, double *__restrict__ part)
{
    __shared__ double sm[3][kBlock];
    const int j = threadIdx.x % MB;
    const double th = theta[j];
    double a_r = 0.0, a_g = 0.0, a_k = 0.0;
    const int64_t total = n * MB;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock) {
        const double gx = GX[e], kx = KX[e];
        const double r = gx - kx * th;
        W[e] = dinv ? dinv[e / MB] * r : r;
        a_r = fma(r, r, a_r);
        a_g = fma(gx, gx, a_g);
        a_k = fma(kx, kx, a_k);
    }
    sm[0][threadIdx.x] = a_r;
    sm[1][threadIdx.x] = a_g;
    sm[2][threadIdx.x] = a_k;
    __syncthreads();
    if (threadIdx.x < 3 * MB) {
        const int q = threadIdx.x / MB, c = threadIdx.x % MB;
        double a = 0.0;
        for (int k = 0; k < kBlock / MB; ++k) a += sm[q][c + k * MB];
        part[static_cast<int64_t>(blockIdx.x) * (3 * MB) + threadIdx.x] = a;
    }
}

// The upper block triangles of G_A = S^T (K_g S) and G_B = S^T (K S), S = [X W P], as per-block partials part[block][2][NS][NS]
// (G_A first: the layout k_modal_gram gives S^T K S and S^T (m o S), so that k_modal_sum and the host's Rayleigh-Ritz serve
// both).  One pass: a tile of kModalGramTile rows of the nine blocks goes through LDS as three row tiles of NS + 1 doubles a row
// (the odd stride keeps the 3 x 3 reads of a row off one bank); thread ownership, row groups and the order of the sums are
// k_modal_gram's.  Tiles below the diagonal are not computed: their threads write zeros.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_buck_gram(int64_t n, const double *__restrict__ X, const double *__restrict__ W, const double *__restrict__ P,
                                                      const double *__restrict__ KX, const double *__restrict__ KW, const double *__restrict__ KP,
                                                      const double *__restrict__ GX, const double *__restrict__ GW, const double *__restrict__ GP,
                                                      double *__restrict__ part)
{
    constexpr int NS = 3 * MB, LD = NS + 1, TR = kModalGramTile;
    constexpr int G = MB * MB, NG = kBlock / G;          // threads of one row group, row groups
    static_assert(3 * TR * LD <= kBuckGramLds, "the row tiles fit the buffer");
    __shared__ double buf[kBuckGramLds];
    double *sS = buf, *sK = buf + TR * LD, *sG = buf + 2 * TR * LD;
    const int t = threadIdx.x, g = t / G, tt = t % G, a0 = 3 * (tt / MB), b0 = 3 * (tt % MB);
    const bool active = a0 <= b0;
    double ga[3][3], gb[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) ga[a][b] = gb[a][b] = 0.0;
    const int64_t n_tiles = (n + TR - 1) / TR;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r0 = tile * TR;
        __syncthreads();                   // (the tile before has been read)
        for (int idx = t; idx < TR * MB; idx += kBlock) {
            const int row = idx / MB, col = idx % MB;
            const int64_t gi = r0 + row;
            const bool in = gi < n;
            const int64_t e = gi * MB + col;
            sS[row * LD + col] = in ? X[e] : 0.0;
            sS[row * LD + MB + col] = in ? W[e] : 0.0;
            sS[row * LD + 2 * MB + col] = in ? P[e] : 0.0;
            sK[row * LD + col] = in ? KX[e] : 0.0;
            sK[row * LD + MB + col] = in ? KW[e] : 0.0;
            sK[row * LD + 2 * MB + col] = in ? KP[e] : 0.0;
            sG[row * LD + col] = in ? GX[e] : 0.0;
            sG[row * LD + MB + col] = in ? GW[e] : 0.0;
            sG[row * LD + 2 * MB + col] = in ? GP[e] : 0.0;
        }
        __syncthreads();
        if (active) {
            for (int row = g; row < TR; row += NG) {
                double sa[3], kb[3], qb[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sa[c] = sS[row * LD + a0 + c];
                    kb[c] = sK[row * LD + b0 + c];
                    qb[c] = sG[row * LD + b0 + c];
                }
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        ga[a][b] = fma(sa[a], qb[b], ga[a][b]);
                        gb[a][b] = fma(sa[a], kb[b], gb[a][b]);
                    }
            }
        }
    }
    if (NG > 1) {                          // the row groups' sums, in group order
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                buf[(0 * 9 + a * 3 + b) * kBlock + t] = ga[a][b];
                buf[(1 * 9 + a * 3 + b) * kBlock + t] = gb[a][b];
            }
        __syncthreads();
        if (g == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    double k = 0.0, q = 0.0;
                    for (int h = 0; h < NG; ++h) {
                        k += buf[(0 * 9 + a * 3 + b) * kBlock + h * G + tt];
                        q += buf[(1 * 9 + a * 3 + b) * kBlock + h * G + tt];
                    }
                    ga[a][b] = k;
                    gb[a][b] = q;
                }
        }
    }
    if (g == 0) {
        double *out = part + static_cast<int64_t>(blockIdx.x) * (2 * NS * NS);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                out[(a0 + a) * NS + b0 + b] = ga[a][b];
                out[NS * NS + (a0 + a) * NS + b0 + b] = gb[a][b];
            }
    }
}

// P' = W C_W + P C_P,  X' = X C_X + P'  and the same coefficients on both product families (K X, K W, K P) and (K_g X, K_g W,
// K_g P), in place, in one pass.  coef, thread ownership and the LDS tile of 256 / MB rows are k_modal_update's; the tile is
// filled and consumed once per family.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_buck_update(int64_t n, const double *__restrict__ coef, double *__restrict__ X, const double *__restrict__ W,
                                                        double *__restrict__ P, double *__restrict__ KX, const double *__restrict__ KW, double *__restrict__ KP,
                                                        double *__restrict__ GX, const double *__restrict__ GW, double *__restrict__ GP)
{
    constexpr int NS = 3 * MB, LD = NS + 1, TR = kBlock / MB;
    __shared__ double sS[TR * LD];
    const int t = threadIdx.x, j = t % MB, row = t / MB;
    double c[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) c[k] = coef[k * MB + j];
    const int64_t n_tiles = (n + TR - 1) / TR;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t gi = tile * TR + row;
        const bool in = gi < n;
        const int64_t e = gi * MB + j;
#pragma unroll
        for (int fam = 0; fam < 3; ++fam) {
            double *__restrict__ bx = fam == 0 ? X : (fam == 1 ? KX : GX);
            const double *__restrict__ bw = fam == 0 ? W : (fam == 1 ? KW : GW);
            double *__restrict__ bp = fam == 0 ? P : (fam == 1 ? KP : GP);
            __syncthreads();               // (the tile before has been read)
            sS[row * LD + j] = in ? bx[e] : 0.0;
            sS[row * LD + MB + j] = in ? bw[e] : 0.0;
            sS[row * LD + 2 * MB + j] = in ? bp[e] : 0.0;
            __syncthreads();
            double p = 0.0, x = 0.0;
#pragma unroll
            for (int k = MB; k < NS; ++k) p = fma(sS[row * LD + k], c[k], p);
#pragma unroll
            for (int k = 0; k < MB; ++k) x = fma(sS[row * LD + k], c[k], x);
            if (in) {
                bx[e] = x + p;
                bp[e] = p;
            }
        }
    }
}

}  // namespace pfem

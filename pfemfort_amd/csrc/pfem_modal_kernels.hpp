// pfem_modal_kernels.hpp -- gfx950 kernels of the modal analysis (pfem_modal_solve): LOBPCG on blocks of
// MB = 4 / 8 / 16 vectors.  A block is n x MB doubles, row-major: the MB values of a row are contiguous (32 / 64 / 128 bytes, so
// a row of MB = 16 is one cache line).  Every sum below is taken in a fixed order -- per thread, then over the threads of a
// block by index, then over the blocks by index -- without atomics: the same bits in every run.
#pragma once

#include "pfem_kernels.hpp"

namespace pfem {

constexpr int kModalGramTile = 32;         // rows of one LDS tile of k_modal_gram
constexpr int kModalGramBlocks = 256;      // most blocks of k_modal_gram (one per CU): the capacity of its partials
constexpr int kModalVecBlocks = 1024;      // most blocks of the grid-stride vector kernels (k_modal_residual, k_modal_update)
constexpr int kModalGramLds = 256 * 18;    // doubles: the 256 threads' 3 x 3 tiles of both matrices; the row tiles alias it

// out doubles of one Gram pass: S^T K S and S^T (m o S), NS x NS row-major each (NS = 3 MB), then the 3 MB column norms^2
__host__ __device__ constexpr int modal_gram_len(int mb) { return 2 * (3 * mb) * (3 * mb); }
__host__ __device__ constexpr int modal_out_len(int mb) { return modal_gram_len(mb) + 3 * mb; }
// doubles of the coefficient block the host sends back: C (NS x MB, rows of X, W, P), then theta (MB)
__host__ __device__ constexpr int modal_coef_len(int mb) { return 3 * mb * mb + mb; }

__host__ __device__ inline uint64_t modal_splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// entry (i, j) of the start block, i the GLOBAL free dof: the hash's top 53 bits x 2^-52 - 1, in [-1, 1)
__host__ __device__ inline double modal_start_value(uint64_t i, int mb, int j)
{
    return static_cast<double>(modal_splitmix64(i * static_cast<uint64_t>(mb) + static_cast<uint64_t>(j)) >> 11) * 0x1.0p-52 - 1.0;
}

// X0 by the hash.  One thread per entry of the caller's numbering; perm (may be nullptr): caller's row -> the device's.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_modal_init(int64_t n, int64_t row_start, const int32_t *__restrict__ perm, double *__restrict__ X)
{
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= n * MB) return;
    const int64_t l = e / MB;
    const int j = static_cast<int>(e % MB);
    const int64_t r = perm ? perm[l] : l;
    X[r * MB + j] = modal_start_value(static_cast<uint64_t>(row_start + l), MB, j);
}

// d -> 1 / d in place (the diagonal k_extract_diag wrote); a row without a diagonal entry counts as 1
__global__ void __launch_bounds__(kBlock) k_modal_invert(int64_t n, double *__restrict__ d)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) d[i] = d[i] != 0.0 ? 1.0 / d[i] : 1.0;
}

// Y = K X on the row form (wave-sliced, int32 columns, fp64 values; entry k of row r at slice_off[r >> 6] + (r & 63) + 64 k).
// Lane = row: a column index and a value are read once -- coalesced over the 64 lanes of the slice -- and serve MB vectors; the
// gathered row of X is MB contiguous doubles, read as 16-byte loads, and so is the row of Y the lane writes.  A lane runs to its
// own row's length, so no padding slot is read; lanes at and beyond n_rows read and write nothing; no column reaches n_rows, so
// nothing beyond n_rows x MB doubles of X is read.  At MB = 16 the lane holds 16 accumulators and one gathered row (64 VGPRs of
// doubles): no reason to split a row over lanes, which would have every lane of the row fetch the same column and value.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_spmm(SellDev A, const double *__restrict__ X, double *__restrict__ Y)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (r >= A.n_rows) return;
    const int64_t base = A.slice_off[r >> 6] + (r & 63);
    const int len = A.rowlen[r];
    double acc[MB];
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[j] = 0.0;
    const int32_t *__restrict__ cols = A.cols + base;
    const double *__restrict__ vals = A.vals + base;
#pragma unroll 2
    for (int k = 0; k < len; ++k) {
        const int32_t c = cols[64LL * k];
        const double v = vals[64LL * k];
        const double2 *__restrict__ x = reinterpret_cast<const double2 *>(X + static_cast<int64_t>(c) * MB);
#pragma unroll
        for (int j = 0; j < MB / 2; ++j) {
            const double2 q = x[j];
            acc[2 * j] = fma(v, q.x, acc[2 * j]);
            acc[2 * j + 1] = fma(v, q.y, acc[2 * j + 1]);
        }
    }
    double2 *__restrict__ y = reinterpret_cast<double2 *>(Y + r * MB);
#pragma unroll
    for (int j = 0; j < MB / 2; ++j) y[j] = make_double2(acc[2 * j], acc[2 * j + 1]);
}

// R = K X - (m o X) diag(theta), W = dinv o R (R itself is not kept; dinv == nullptr: W = R, for a T applied afterwards), and per
// block the partial sums of ||R_j||^2, ||K X_j||^2 and ||m o X_j||^2: part[block][3][MB].  Thread t owns column t % MB throughout
// (the stride is a multiple of MB).
template <int MB>
__global__ void __launch_bounds__(kBlock) k_modal_residual(int64_t n, const double *__restrict__ KX, const double *__restrict__ X, const double *__restrict__ m,
                                                           const double *__restrict__ dinv, const double *__restrict__ theta, double *__restrict__ W,
                                                           double *__restrict__ part)
{
    __shared__ double sm[3][kBlock];
    const int j = threadIdx.x % MB;
    const double th = theta[j];
    double a_r = 0.0, a_k = 0.0, a_m = 0.0;
    const int64_t total = n * MB;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t i = e / MB;
        const double kx = KX[e], mx = m[i] * X[e];
        const double r = kx - mx * th;
        W[e] = dinv ? dinv[i] * r : r;
        a_r = fma(r, r, a_r);
        a_k = fma(kx, kx, a_k);
        a_m = fma(mx, mx, a_m);
    }
    sm[0][threadIdx.x] = a_r;
    sm[1][threadIdx.x] = a_k;
    sm[2][threadIdx.x] = a_m;
    __syncthreads();
    if (threadIdx.x < 3 * MB) {
        const int q = threadIdx.x / MB, c = threadIdx.x % MB;
        double a = 0.0;
        for (int k = 0; k < kBlock / MB; ++k) a += sm[q][c + k * MB];
        part[static_cast<int64_t>(blockIdx.x) * (3 * MB) + threadIdx.x] = a;
    }
}

// The upper block triangles of G_K = S^T (K S) and G_M = S^T (m o S), S = [X W P], as per-block partials part[block][2][NS][NS].
// A tile of kModalGramTile rows of the six blocks and of m goes through LDS; a thread owns a 3 x 3 tile of both matrices
// (NS / 3 = MB tiles a side, MB^2 threads for all of them), and the 256 / MB^2 groups of such threads take the tile's rows in
// turn; their sums are added in group order at the end.  Tiles below the diagonal are not computed: their threads write zeros.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_modal_gram(int64_t n, const double *__restrict__ X, const double *__restrict__ W, const double *__restrict__ P,
                                                       const double *__restrict__ KX, const double *__restrict__ KW, const double *__restrict__ KP,
                                                       const double *__restrict__ m, double *__restrict__ part)
{
    constexpr int NS = 3 * MB, LD = NS + 1, TR = kModalGramTile;
    constexpr int G = MB * MB, NG = kBlock / G;          // threads of one row group, row groups
    static_assert(2 * TR * LD + TR <= kModalGramLds, "the row tiles fit the buffer");
    __shared__ double buf[kModalGramLds];
    double *sS = buf, *sK = buf + TR * LD, *sM = buf + 2 * TR * LD;
    const int t = threadIdx.x, g = t / G, tt = t % G, a0 = 3 * (tt / MB), b0 = 3 * (tt % MB);
    const bool active = a0 <= b0;
    double gk[3][3], gm[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) gk[a][b] = gm[a][b] = 0.0;
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
        }
        if (t < TR) sM[t] = r0 + t < n ? m[r0 + t] : 0.0;
        __syncthreads();
        if (active) {
            for (int row = g; row < TR; row += NG) {
                const double mi = sM[row];
                double sa[3], kb[3], sb[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sa[c] = sS[row * LD + a0 + c];
                    kb[c] = sK[row * LD + b0 + c];
                    sb[c] = mi * sS[row * LD + b0 + c];
                }
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        gk[a][b] = fma(sa[a], kb[b], gk[a][b]);
                        gm[a][b] = fma(sa[a], sb[b], gm[a][b]);
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
                buf[(0 * 9 + a * 3 + b) * kBlock + t] = gk[a][b];
                buf[(1 * 9 + a * 3 + b) * kBlock + t] = gm[a][b];
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
                    gk[a][b] = k;
                    gm[a][b] = q;
                }
        }
    }
    if (g == 0) {
        double *out = part + static_cast<int64_t>(blockIdx.x) * (2 * NS * NS);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                out[(a0 + a) * NS + b0 + b] = gk[a][b];
                out[NS * NS + (a0 + a) * NS + b0 + b] = gm[a][b];
            }
    }
}

// Column j of a block <-> a contiguous vector: how a preconditioner written for one vector (gamg's cycle) sees W a column at a time
template <int MB>
__global__ void __launch_bounds__(kBlock) k_modal_pack(int64_t n, const double *__restrict__ B, int j, double *__restrict__ v)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) v[i] = B[i * MB + j];
}
template <int MB>
__global__ void __launch_bounds__(kBlock) k_modal_unpack(int64_t n, const double *__restrict__ v, int j, double *__restrict__ B)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) B[i * MB + j] = v[i];
}

// out[e] = the sum over the blocks, in block order, of the Gram partials (e < n_gram) and of the residual kernel's norm partials
// (the n_res entries after them).  nb_gram = 0 / nb_res = 0: that part of `out` is left as it is.
__global__ void __launch_bounds__(kBlock) k_modal_sum(int n_gram, int nb_gram, const double *__restrict__ part_gram, int n_res, int nb_res,
                                                      const double *__restrict__ part_res, double *__restrict__ out)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < n_gram) {
        if (nb_gram == 0) return;
        double a = 0.0;
        for (int b = 0; b < nb_gram; ++b) a += part_gram[static_cast<int64_t>(b) * n_gram + e];
        out[e] = a;
    } else if (e < n_gram + n_res) {
        if (nb_res == 0) return;
        const int q = e - n_gram;
        double a = 0.0;
        for (int b = 0; b < nb_res; ++b) a += part_res[static_cast<int64_t>(b) * n_res + q];
        out[e] = a;
    }
}

// P' = W C_W + P C_P,  X' = X C_X + P'  and the same coefficients on K X, K W, K P, in place.  coef: C as NS x MB row-major (rows
// of X, of W, of P).  A thread owns column t % MB -- that column of C stays in its registers -- and row t / MB of a tile of
// 256 / MB rows, which goes through LDS so that every block is read once, coalesced, before any of it is overwritten.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_modal_update(int64_t n, const double *__restrict__ coef, double *__restrict__ X, const double *__restrict__ W,
                                                         double *__restrict__ P, double *__restrict__ KX, const double *__restrict__ KW, double *__restrict__ KP)
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
        for (int half = 0; half < 2; ++half) {
            double *__restrict__ bx = half ? KX : X;
            const double *__restrict__ bw = half ? KW : W;
            double *__restrict__ bp = half ? KP : P;
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

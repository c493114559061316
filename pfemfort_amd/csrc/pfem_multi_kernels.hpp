// pfem_multi_kernels.hpp -- gfx950 kernels of the solve for several right-hand sides (pfem_solver_solve_multi; DESIGN.md section
// 16): MB = 4 / 8 independent Jacobi- or gamg-preconditioned CG iterations that share one pass over the matrix per iteration.  A
// panel is n x MB doubles, row-major, as the modal blocks.  In the vector kernels thread t owns column t % MB throughout (the
// stride is a multiple of MB): coalesced, the column's scalars in registers.  Every sum is taken in a fixed order -- per thread,
// then over the threads of a block by index, then over the blocks by index -- without atomics: the same bits in every run, and a
// column's bits depend on n and MB only, not on its place in the panel or on what the other columns hold.
//
// The control rule: no kernel reads a word of McgCtl that a block of the SAME launch writes.  The verdicts are formed by
// one-block kernels (k_mcg_start, k_mcg_verdict) between the vector kernels; a vector kernel reads only what an earlier launch
// wrote, and returns at once when no column is running.  k_mcg_update's block 0 writes alpha, which nobody in that launch reads.
#pragma once

#include "pfem_modal_kernels.hpp"

namespace pfem {

constexpr int kMcgMaxMB = 8;               // the widest panel (k_spmm<16> does not pay)
constexpr int kMcgVecBlocks = 1024;        // most blocks of the grid-stride vector kernels: the capacity of their partials

// What a step's verdict says about a column (McgCtl::verdict): what k_mcg_direction does with it
enum { kMcgIdle = 0,      // was not running when the step began: nothing is read or written
       kMcgGoesOn = 1,    // still running: x += alpha p, p = z + bb p
       kMcgLastStep = 2,  // finished in this step: x += alpha p (as in KSPCG the test follows the update)
       kMcgBroke = 3 };   // (p, Kp) <= 0 in this step: x is not advanced

struct McgCtl {                            // device-resident control block of one panel
    double beta[kMcgMaxMB][2];             // (r,z) ping-pong by step parity
    double rn0[kMcgMaxMB], ttol[kMcgMaxMB];   // ||z0||, max(rtol rn0, abstol)
    double rn[kMcgMaxMB];                  // last preconditioned residual norm
    double alpha[kMcgMaxMB];               // step length of the current step (k_mcg_update -> k_mcg_direction)
    double bb[kMcgMaxMB];                  // (r,z)_new / (r,z)_old of the current step (k_mcg_verdict -> k_mcg_direction)
    int flag[kMcgMaxMB];                   // 0 = running, else KSPConvergedReason
    int its[kMcgMaxMB];                    // iterations completed
    int verdict[kMcgMaxMB];                // kMcg* of the current step
    int running;                           // columns with flag == 0
    int step;                              // steps completed by the panel: the `it` of the columns still running
};

// W = K P as k_spmm<MB> -- the same fma chain per row, so the same bits -- and the block's partial of sum_i p_ij w_ij per column:
// part_pw[block][MB].  One thread per row; lanes at and beyond n_rows add zeros and read nothing of P.  The products go through
// LDS (rows of kBlock + 1 doubles: the MB columns of a lane group fall on different banks): group g of kBlock / MB adds the MB
// values of threads g MB .. g MB + MB - 1 in thread order, then thread j < MB adds the groups' sums of column j in group order.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_spmm_dot(const McgCtl *ctl, SellDev A, const double *__restrict__ P, double *__restrict__ W,
                                                     double *__restrict__ part_pw)
{
    constexpr int LD = kBlock + 1, NG = kBlock / MB;
    __shared__ double sm[MB * LD];
    __shared__ double sg[MB * (NG + 1)];
    if (ctl && ctl->running == 0) return;
    const int t = threadIdx.x;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + t;
    double acc[MB];
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[j] = 0.0;
    if (r < A.n_rows) {
        const int64_t base = A.slice_off[r >> 6] + (r & 63);
        const int len = A.rowlen[r];
        const int32_t *__restrict__ cols = A.cols + base;
        const double *__restrict__ vals = A.vals + base;
#pragma unroll 2
        for (int k = 0; k < len; ++k) {
            const int32_t c = cols[64LL * k];
            const double v = vals[64LL * k];
            const double2 *__restrict__ x = reinterpret_cast<const double2 *>(P + static_cast<int64_t>(c) * MB);
#pragma unroll
            for (int j = 0; j < MB / 2; ++j) {
                const double2 q = x[j];
                acc[2 * j] = fma(v, q.x, acc[2 * j]);
                acc[2 * j + 1] = fma(v, q.y, acc[2 * j + 1]);
            }
        }
        double2 *__restrict__ y = reinterpret_cast<double2 *>(W + r * MB);
        const double2 *__restrict__ p = reinterpret_cast<const double2 *>(P + r * MB);
#pragma unroll
        for (int j = 0; j < MB / 2; ++j) {
            y[j] = make_double2(acc[2 * j], acc[2 * j + 1]);
            const double2 q = p[j];
            sm[(2 * j) * LD + t] = q.x * acc[2 * j];
            sm[(2 * j + 1) * LD + t] = q.y * acc[2 * j + 1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < MB; ++j) sm[j * LD + t] = 0.0;
    }
    __syncthreads();
    {
        const int j = t % MB, g = t / MB;
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < MB; ++k) a += sm[j * LD + g * MB + k];
        sg[j * (NG + 1) + g] = a;
    }
    __syncthreads();
    if (t < MB) {
        double a = 0.0;
        for (int g = 0; g < NG; ++g) a += sg[t * (NG + 1) + g];
        part_pw[static_cast<int64_t>(blockIdx.x) * MB + t] = a;
    }
}

// The sum over the 256 threads of a block of `nq` quantities per column, thread t owning column t % MB: sm holds nq * kBlock
// doubles; thread q MB + j (q < nq) adds column j of quantity q in thread order and returns it, the others return 0.
template <int MB>
__device__ __forceinline__ double mcg_block_sums(int nq, const double *v, double *sm)
{
    for (int q = 0; q < nq; ++q) sm[q * kBlock + threadIdx.x] = v[q];
    __syncthreads();
    double a = 0.0;
    if (static_cast<int>(threadIdx.x) < nq * MB) {
        const int q = threadIdx.x / MB, c = threadIdx.x % MB;
        for (int k = 0; k < kBlock / MB; ++k) a += sm[q * kBlock + c + k * MB];
    }
    return a;
}

// First stage of the fold of the product's partials (one row of MB per block of k_spmm_dot): block b of kFoldBlocks sums the b-th
// contiguous chunk of rows into out[b][MB]; k_mcg_update re-sums those kFoldBlocks rows.  The shape of k_fold_partials.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_mcg_fold(const McgCtl *ctl, const double *__restrict__ part, int n, double *__restrict__ out)
{
    __shared__ double sm[kBlock];
    if (ctl && ctl->running == 0) return;
    const int chunk = (n + kFoldBlocks - 1) / kFoldBlocks;
    const int lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
    const int j = threadIdx.x % MB;
    double a = 0.0;
    for (int i = lo + threadIdx.x / MB; i < hi; i += kBlock / MB) a += part[static_cast<int64_t>(i) * MB + j];
    const double t = mcg_block_sums<MB>(1, &a, sm);
    if (threadIdx.x < MB) out[blockIdx.x * MB + threadIdx.x] = t;
}

// the kFoldBlocks folded partials of column j, in index order: every thread of every block gets the same bits
template <int MB>
__device__ __forceinline__ double mcg_folded(const double *__restrict__ fold, int j)
{
    double a = 0.0;
    for (int b = 0; b < kFoldBlocks; ++b) a += fold[b * MB + j];
    return a;
}

// X = 0, R = B, and with dinv (point Jacobi): P = Z = dinv o R and the partials of (r,z) and (z,z) per column,
// part[block][2][MB].  dinv == nullptr (gamg): P and the partials are left to the cycles and k_mcg_dots.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_mcg_init(int64_t n, const double *__restrict__ B, const double *__restrict__ dinv, double *__restrict__ X,
                                                     double *__restrict__ R, double *__restrict__ P, double *__restrict__ part)
{
    __shared__ double sm[2 * kBlock];
    double a[2] = {0.0, 0.0};
    const int64_t total = n * MB;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock) {
        const double ri = B[e];
        X[e] = 0.0;
        R[e] = ri;
        if (dinv) {
            const double zi = ri * dinv[e / MB];
            P[e] = zi;
            a[0] = __builtin_fma(ri, zi, a[0]);
            a[1] = __builtin_fma(zi, zi, a[1]);
        }
    }
    if (!dinv) return;
    const double t = mcg_block_sums<MB>(2, a, sm);
    if (threadIdx.x < 2 * MB) part[static_cast<int64_t>(blockIdx.x) * (2 * MB) + threadIdx.x] = t;
}

// The sums over the blocks, in block order, of the partials part[block][2][MB]: sm holds kBlock doubles; thread c < 2 MB returns
// the sum of entry c ((r,z) of column c, or (z,z) of column c - MB), the others 0.  One block.
__device__ __forceinline__ double mcg_finish(int mb, const double *__restrict__ part, int nparts, double *sm)
{
    const int w = 2 * mb, c = threadIdx.x % w, g = threadIdx.x / w, ng = kBlock / w;
    double a = 0.0;
    for (int b = g; b < nparts; b += ng) a += part[static_cast<int64_t>(b) * w + c];
    sm[threadIdx.x] = a;
    __syncthreads();
    double t = 0.0;
    if (static_cast<int>(threadIdx.x) < w)
        for (int k = 0; k < ng; ++k) t += sm[c + k * w];
    __syncthreads();
    return t;
}

// One block: finish the initial sums and set the tolerances (KSPConvergedDefault, as k_cg_start): beta[0], rn0, ttol; flag = 3
// where rn0 <= abstol (a zero column), -8 where (r,z) < 0; the running count.
__global__ void __launch_bounds__(kBlock) k_mcg_start(McgCtl *ctl, int mb, const double *__restrict__ part, int nparts, double rtol, double abstol)
{
    __shared__ double sm[kBlock];
    __shared__ double tot[2 * kMcgMaxMB];
    const double t = mcg_finish(mb, part, nparts, sm);
    if (static_cast<int>(threadIdx.x) < 2 * mb) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        int running = 0;
        for (int j = 0; j < kMcgMaxMB; ++j) {
            const bool in = j < mb;
            const double rz = in ? tot[j] : 0.0, zz = in ? tot[mb + j] : 0.0;
            const double rn0 = sqrt(zz);
            ctl->beta[j][0] = rz;
            ctl->beta[j][1] = 0.0;
            ctl->rn0[j] = rn0;
            ctl->rn[j] = rn0;
            ctl->ttol[j] = fmax(rtol * rn0, abstol);
            ctl->alpha[j] = 0.0;
            ctl->bb[j] = 0.0;
            ctl->its[j] = 0;
            ctl->verdict[j] = kMcgIdle;
            const int flag = !in ? 3 : ((rn0 <= abstol) ? 3 : ((rz < 0.0) ? -8 : 0));
            ctl->flag[j] = flag;
            running += flag == 0;
        }
        ctl->running = running;
        ctl->step = 0;
    }
}

// alpha_j = beta_j / (p,w)_j from the folded product partials, which every thread re-sums for its column; R -= alpha W; with dinv
// (point Jacobi) also z = dinv o r and the partials of (r,z) and (z,z), part[block][2][MB].  A column whose (p,w) is not positive
// leaves R alone and marks its (z,z) partial -1, as k_cg_update does.  A column that is not running is skipped: no load of W, no
// store.  dinv == nullptr (gamg): no partials; k_mcg_dots forms them, and the marker, after the cycles.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_mcg_update(McgCtl *ctl, int64_t n, const double *__restrict__ fold_pw, const double *__restrict__ W,
                                                       const double *__restrict__ dinv, double *__restrict__ R, double *__restrict__ part)
{
    __shared__ double sm[2 * kBlock];
    if (ctl->running == 0) return;
    const int j = threadIdx.x % MB;
    const bool on = ctl->flag[j] == 0;
    double a[2] = {0.0, 0.0};
    if (on) {
        const double pw = mcg_folded<MB>(fold_pw, j);
        if (!(pw > 0.0)) {                 // KSP_DIVERGED_INDEFINITE_MAT
            a[1] = threadIdx.x < MB ? -1.0 : 0.0;
        } else {
            const double alpha = ctl->beta[j][ctl->step & 1] / pw;
            if (blockIdx.x == 0 && threadIdx.x < MB) ctl->alpha[j] = alpha;      // nobody in this launch reads it
            const int64_t total = n * MB;
            for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock) {
                const double ri = __builtin_fma(-alpha, W[e], R[e]);
                R[e] = ri;
                if (dinv) {
                    const double zi = ri * dinv[e / MB];
                    a[0] = __builtin_fma(ri, zi, a[0]);
                    a[1] = __builtin_fma(zi, zi, a[1]);
                }
            }
        }
    }
    if (!dinv) return;
    const double t = mcg_block_sums<MB>(2, a, sm);
    if (threadIdx.x < 2 * MB) part[static_cast<int64_t>(blockIdx.x) * (2 * MB) + threadIdx.x] = t;
}

// gamg: the partials of (r,z) and (z,z) per column from the Z the cycles left, part[block][2][MB]; a running column whose (p,w)
// was not positive (fold_pw re-summed as k_mcg_update did; nullptr at the start) gets the -1 marker instead.  ctl == nullptr (the
// start, before k_mcg_start): every column.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_mcg_dots(const McgCtl *ctl, int64_t n, const double *__restrict__ fold_pw, const double *__restrict__ R,
                                                     const double *__restrict__ Z, double *__restrict__ part)
{
    __shared__ double sm[2 * kBlock];
    if (ctl && ctl->running == 0) return;
    const int j = threadIdx.x % MB;
    const bool on = !ctl || ctl->flag[j] == 0;
    double a[2] = {0.0, 0.0};
    if (on) {
        if (fold_pw && !(mcg_folded<MB>(fold_pw, j) > 0.0)) {
            a[1] = threadIdx.x < MB ? -1.0 : 0.0;
        } else {
            const int64_t total = n * MB;
            for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock) {
                const double ri = R[e], zi = Z[e];
                a[0] = __builtin_fma(ri, zi, a[0]);
                a[1] = __builtin_fma(zi, zi, a[1]);
            }
        }
    }
    const double t = mcg_block_sums<MB>(2, a, sm);
    if (threadIdx.x < 2 * MB) part[static_cast<int64_t>(blockIdx.x) * (2 * MB) + threadIdx.x] = t;
}

// One block: finish (r,z) and ||z|| and, per running column, apply the tests of k_cg_direction in their order: -10 from the
// marker, then 2, -4, -8, -3.  Writes beta[(it + 1) & 1], rn, bb = rz / beta_old, its = it + 1 and the step's verdict (idle for a
// column that was not running), then the running count and the step counter.
__global__ void __launch_bounds__(kBlock) k_mcg_verdict(McgCtl *ctl, int mb, const double *__restrict__ part, int nparts, double dtol, int maxits)
{
    __shared__ double sm[kBlock];
    __shared__ double tot[2 * kMcgMaxMB];
    if (ctl->running == 0) {               // a launch after the last verdict: k_mcg_direction must not repeat that step
        if (static_cast<int>(threadIdx.x) < mb) ctl->verdict[threadIdx.x] = kMcgIdle;
        return;
    }
    const double t = mcg_finish(mb, part, nparts, sm);
    if (static_cast<int>(threadIdx.x) < 2 * mb) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int it = ctl->step;
        int running = 0;
        for (int j = 0; j < mb; ++j) {
            if (ctl->flag[j] != 0) { ctl->verdict[j] = kMcgIdle; continue; }
            const double rz = tot[j], zz = tot[mb + j];
            ctl->its[j] = it + 1;
            if (zz < 0.0) {                // breakdown flagged by k_mcg_update / k_mcg_dots: KSP_DIVERGED_INDEFINITE_MAT
                ctl->flag[j] = -10;
                ctl->verdict[j] = kMcgBroke;
                continue;
            }
            const double rn = sqrt(zz);
            const double beta_old = ctl->beta[j][it & 1];
            int flag = 0;
            if (rn <= ctl->ttol[j]) flag = 2;            // KSP_CONVERGED_RTOL (or ATOL, resolved on the host)
            else if (rn >= dtol * ctl->rn0[j]) flag = -4;
            else if (rz < 0.0) flag = -8;                // KSP_DIVERGED_INDEFINITE_PC
            else if (it + 1 >= maxits) flag = -3;
            ctl->beta[j][(it + 1) & 1] = rz;
            ctl->rn[j] = rn;
            ctl->bb[j] = rz / beta_old;
            ctl->flag[j] = flag;
            ctl->verdict[j] = flag != 0 ? kMcgLastStep : kMcgGoesOn;
            running += flag == 0;
        }
        ctl->running = running;
        ctl->step = it + 1;
    }
}

// For the columns that entered this step running: X += alpha P, also when the step turned out to be the last, not on a
// breakdown.  For the columns still running: P = Z + bb P, Z = dinv o R recomputed (point Jacobi) or the stored Z (gamg: dinv ==
// nullptr).  Reads the verdicts k_mcg_verdict left; writes no control word.
template <int MB>
__global__ void __launch_bounds__(kBlock) k_mcg_direction(const McgCtl *ctl, int64_t n, const double *__restrict__ R, const double *__restrict__ dinv,
                                                          const double *__restrict__ Z, double *__restrict__ P, double *__restrict__ X)
{
    const int j = threadIdx.x % MB;
    const int v = ctl->verdict[j];
    if (v != kMcgGoesOn && v != kMcgLastStep) return;
    const double alpha = ctl->alpha[j], bb = ctl->bb[j];
    const int64_t total = n * MB;
    if (v == kMcgLastStep) {
        for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock)
            X[e] = __builtin_fma(alpha, P[e], X[e]);
        return;
    }
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock) {
        const double pi = P[e];
        X[e] = __builtin_fma(alpha, pi, X[e]);
        const double zi = dinv ? R[e] * dinv[e / MB] : Z[e];
        P[e] = __builtin_fma(bb, pi, zi);
    }
}

}  // namespace pfem

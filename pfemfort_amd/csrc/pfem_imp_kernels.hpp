// pfem_imp_kernels.hpp -- gfx950 kernels of the implicit time stepping (pfem_dynamics_run_implicit):
// Newmark (beta, gamma) and the theta-method on the lumped mass.  Every step is one solve (K + sigma diag(m)) d = b by the
// two-reduction Jacobi-PCG of k_cg_update / k_cg_direction with the diagonal sigma m added to the operator: the product K p is
// the SpMV's, unchanged; the direction kernel also leaves the partials of sum sigma m p^2, so that (p, Ap) = (p, Kp) + that sum
// is known in the update kernel without another pass.  Three launches an iteration.  Every cross-block sum crosses a launch
// boundary (per-block partials, re-summed by every consumer block in index order): no atomics, no fences, the same bits in
// every run.  Included once by pfem_device.hip after pfem_dyn_kernels.hpp.  The vector kernels take four consecutive rows per
// thread with 16-byte loads (k_dyn_step's shape) in a grid-stride loop over at most kMaxGrid blocks.
// Outside the CG recurrence (which uses fma like the solver's) every value is a written-down sequence of IEEE operations
// that tests/implicit_reference.py repeats.
#pragma once

#include "pfem_dyn_kernels.hpp"

namespace pfem {

constexpr int kImpNewmark = 1, kImpTheta = 2;          // PFEM_SCHEME_*

// what stays the same for every step of a run
struct ImpPar {
    int64_t n;                   // rows
    int scheme;
    double dt, sigma;            // the shift: (1 + gamma dt alpha) / (beta dt^2), or 1 / (theta dt)
    double alpha;                // damping C = alpha M (Newmark)
    double cu, cv;               // Newmark predictor: dt^2 (1/2 - beta), dt (1 - gamma)
    double bdt2, gdt;            // Newmark corrector: beta dt^2, gamma dt
    double theta;
};

__device__ __forceinline__ void imp_st4(double *__restrict__ p, int64_t r0, int64_t n, const double v[4])
{
    if (r0 + kDynRows <= n) {
        *reinterpret_cast<double2 *>(p + r0) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2 *>(p + r0 + 2) = make_double2(v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kDynRows; ++k)
            if (r0 + k < n) p[r0 + k] = v[k];
    }
}

// first row of the thread's chunk `c` of a grid-stride loop over chunks of four rows
#define PFEM_IMP_CHUNKS(r0, n)                                                                                              \
    for (int64_t r0 = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kDynRows; r0 < (n);                          \
         r0 += static_cast<int64_t>(gridDim.x) * kDynBlockRows)

// dinv = 1 / (K_ii + sigma m_i), in place on the diagonal k_extract_diag wrote; a row without mass counts as 1
__global__ void __launch_bounds__(kBlock) k_imp_dinv(int64_t n, double sigma, const double *__restrict__ m, double *__restrict__ diag)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    diag[i] = m[i] > 0.0 ? 1.0 / (diag[i] + sigma * m[i]) : 1.0;
}

// a_0 = (lambda(t0) f - alpha m v0 - K u0) / m, w = K u0; a row without mass: 0
__global__ void __launch_bounds__(kBlock) k_imp_accel0(ImpPar P, DynPar C, double t0, const double *__restrict__ f, const double *__restrict__ m,
                                                        const double *__restrict__ v, const double *__restrict__ w, double *__restrict__ a)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const double lam = dyn_lambda(C, t0);
    a[i] = m[i] > 0.0 ? ((lam * f[i] - P.alpha * (m[i] * v[i])) - w[i]) / m[i] : 0.0;
}

// Newmark predictor: ut = (u + dt v) + cu a,  vt = v + cv a
__global__ void __launch_bounds__(kBlock) k_imp_predict(ImpPar P, const double *__restrict__ u, const double *__restrict__ v,
                                                         const double *__restrict__ a, double *__restrict__ ut, double *__restrict__ vt)
{
    PFEM_IMP_CHUNKS(r0, P.n) {
        double ui[4], vi[4], ai[4], x[4], y[4];
        dyn_ld4(u, r0, P.n, ui);
        dyn_ld4(v, r0, P.n, vi);
        dyn_ld4(a, r0, P.n, ai);
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) {
            x[k] = (ui[k] + P.dt * vi[k]) + P.cu * ai[k];
            y[k] = vi[k] + P.cv * ai[k];
        }
        imp_st4(ut, r0, P.n, x);
        imp_st4(vt, r0, P.n, y);
    }
}

// b = lam f - alpha m vt - w (w = K ut; theta-method: vt == nullptr, w = K u_n), lam = ln1 lambda(tn1) + ln0 lambda(tn0);
// a row without mass has b = 0.  d = 0, r = b, p = z = r dinv; the block's partials of (r, z), (z, z) and sum sigma m p^2.
__global__ void __launch_bounds__(kBlock) k_imp_rhs(ImpPar P, DynPar C, double tn0, double ln0, double tn1, double ln1, const double *__restrict__ f,
                                                     const double *__restrict__ m, const double *__restrict__ vt, const double *__restrict__ w,
                                                     const double *__restrict__ dinv, double *__restrict__ d, double *__restrict__ r,
                                                     double *__restrict__ p, double *part_rz, double *part_zz, double *part_mp)
{
    __shared__ double sm[4];
    __shared__ double s_lam;
    if (threadIdx.x == 0) s_lam = ln0 != 0.0 ? ln1 * dyn_lambda(C, tn1) + ln0 * dyn_lambda(C, tn0) : ln1 * dyn_lambda(C, tn1);
    __syncthreads();
    const double lam = s_lam;
    double rz = 0.0, zz = 0.0, mp = 0.0;
    PFEM_IMP_CHUNKS(r0, P.n) {
        double fi[4], mi[4], vi[4] = {0.0, 0.0, 0.0, 0.0}, wi[4], qi[4], b[4], z[4], zero[4] = {0.0, 0.0, 0.0, 0.0};
        dyn_ld4(f, r0, P.n, fi);
        dyn_ld4(m, r0, P.n, mi);
        if (vt) dyn_ld4(vt, r0, P.n, vi);
        dyn_ld4(w, r0, P.n, wi);
        dyn_ld4(dinv, r0, P.n, qi);
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) {                          // (rows past the end read zeros and add zeros)
            const double load = vt ? lam * fi[k] - P.alpha * (mi[k] * vi[k]) : lam * fi[k];
            b[k] = mi[k] > 0.0 ? load - wi[k] : 0.0;
            z[k] = b[k] * qi[k];
            rz = __builtin_fma(b[k], z[k], rz);
            zz = __builtin_fma(z[k], z[k], zz);
            mp = __builtin_fma((P.sigma * mi[k]) * z[k], z[k], mp);
        }
        imp_st4(d, r0, P.n, zero);
        imp_st4(r, r0, P.n, b);
        imp_st4(p, r0, P.n, z);
    }
    const double t0 = block_sum(rz, sm), t1 = block_sum(zz, sm), t2 = block_sum(mp, sm);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = t0; part_zz[blockIdx.x] = t1; part_mp[blockIdx.x] = t2; }
}

// k_cg_update of the shifted operator: (p, Ap) = (p, Kp) [the SpMV's partials] + sum sigma m p^2 [the direction kernel's];
// alpha = beta / (p, Ap); r -= alpha (w + sigma m p); partials of (r, z), (z, z) with z = r dinv.
// `it_arg` < 0 (launches replayed from a hipGraph): the iteration index is taken from the control block.
__global__ void __launch_bounds__(kBlock) k_imp_update(CgCtl *ctl, int it_arg, ImpPar P, const double *part_pw, int n_pw, const double *part_mp,
                                                        int nparts, const double *__restrict__ p, const double *__restrict__ w,
                                                        const double *__restrict__ m, const double *__restrict__ dinv, double *__restrict__ r,
                                                        double *part_rz, double *part_zz)
{
    __shared__ double sm[4];
    if (ctl->flag != 0) {                   // finished in an earlier iteration (this kernel never writes flag)
        if (blockIdx.x == 0 && threadIdx.x == 0) ctl->its_dir = -2;
        return;
    }
    const int it = it_arg >= 0 ? it_arg : ctl->its;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->its_dir = it;      // nobody in this launch reads it
    const double pkp = sum_partials(part_pw, n_pw, sm);
    const double pmp = sum_partials(part_mp, nparts, sm);
    const double pw = pkp + pmp;
    if (!(pw > 0.0)) {                      // KSP_DIVERGED_INDEFINITE_MAT
        part_rz[blockIdx.x] = 0.0; part_zz[blockIdx.x] = -1.0;       // signals breakdown to k_imp_direction
        return;
    }
    const double alpha = ctl->beta[it & 1] / pw;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->alpha = alpha;
    double rz = 0.0, zz = 0.0;
    PFEM_IMP_CHUNKS(r0, P.n) {
        double pi[4], wi[4], mi[4], qi[4], ri[4];
        dyn_ld4(p, r0, P.n, pi);
        dyn_ld4(w, r0, P.n, wi);
        dyn_ld4(m, r0, P.n, mi);
        dyn_ld4(dinv, r0, P.n, qi);
        dyn_ld4(r, r0, P.n, ri);
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) {
            ri[k] = __builtin_fma(-alpha, __builtin_fma(P.sigma * mi[k], pi[k], wi[k]), ri[k]);
            const double zi = ri[k] * qi[k];
            rz = __builtin_fma(ri[k], zi, rz);
            zz = __builtin_fma(zi, zi, zz);
        }
        imp_st4(r, r0, P.n, ri);
    }
    const double t0 = block_sum(rz, sm), t1 = block_sum(zz, sm);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = t0; part_zz[blockIdx.x] = t1; }
}

// k_cg_direction of the shifted operator: finish (r, z), ||z||; d += alpha p (also when this iteration is the last; not on a
// breakdown); convergence test; p = z + (beta_new / beta) p and the block's partial of sum sigma m p^2 for the next update.
__global__ void __launch_bounds__(kBlock) k_imp_direction(CgCtl *ctl, int it_arg, ImpPar P, const double *part_rz, const double *part_zz, int nparts,
                                                           const double *__restrict__ r, const double *__restrict__ dinv,
                                                           const double *__restrict__ m, double *__restrict__ p, double *__restrict__ d,
                                                           int maxits, double *part_mp)
{
    __shared__ double sm[4];
    const int it = it_arg >= 0 ? it_arg : ctl->its_dir;              // ctl->its is written by this launch: not read here
    if (ctl_finished_before(ctl, it)) return;
    const double rz = sum_partials(part_rz, nparts, sm), zz = sum_partials(part_zz, nparts, sm);
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (zz < 0.0) {                          // breakdown flagged by k_imp_update: KSP_DIVERGED_INDEFINITE_MAT
        if (lead) ctl_publish(ctl, -10, it + 1);
        return;
    }
    const double rn = sqrt(zz);
    const double beta_old = ctl->beta[it & 1];
    int flag = 0;
    if (rn <= ctl->ttol) flag = 2;           // KSP_CONVERGED_RTOL (or ATOL, resolved on the host)
    else if (rn >= ctl->dtol * ctl->rn0) flag = -4;
    else if (rz < 0.0) flag = -8;            // KSP_DIVERGED_INDEFINITE_PC
    else if (it + 1 >= maxits) flag = -3;
    if (lead) {
        // other blocks of THIS launch read only beta[it&1]/ttol/dtol/rn0/alpha and test the verdict word against `it`
        ctl->beta[(it + 1) & 1] = rz;
        ctl->rn = rn;
        ctl_publish(ctl, flag, it + 1);
    }
    const double alpha = ctl->alpha;
    const double bb = rz / beta_old;
    double mp = 0.0;
    PFEM_IMP_CHUNKS(r0, P.n) {
        double pi[4], di[4];
        dyn_ld4(p, r0, P.n, pi);
        dyn_ld4(d, r0, P.n, di);
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) di[k] = __builtin_fma(alpha, pi[k], di[k]);
        imp_st4(d, r0, P.n, di);
        if (flag != 0) continue;             // (uniform over the grid)
        double ri[4], qi[4], mi[4];
        dyn_ld4(r, r0, P.n, ri);
        dyn_ld4(dinv, r0, P.n, qi);
        dyn_ld4(m, r0, P.n, mi);
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) {
            pi[k] = __builtin_fma(bb, pi[k], ri[k] * qi[k]);
            mp = __builtin_fma((P.sigma * mi[k]) * pi[k], pi[k], mp);
        }
        imp_st4(p, r0, P.n, pi);
    }
    if (flag != 0) return;
    const double t = block_sum(mp, sm);
    if (threadIdx.x == 0) part_mp[blockIdx.x] = t;
}

// corrector.  Newmark: u = ut + d, a = d / (beta dt^2), v = vt + (gamma dt) a.  theta: u' = u + d / theta, v = (u' - u) / dt.
__global__ void __launch_bounds__(kBlock) k_imp_correct(ImpPar P, const double *__restrict__ ut, const double *__restrict__ vt,
                                                         const double *__restrict__ d, double *__restrict__ u, double *__restrict__ v,
                                                         double *__restrict__ a)
{
    PFEM_IMP_CHUNKS(r0, P.n) {
        double di[4], x[4], y[4], z[4];
        dyn_ld4(d, r0, P.n, di);
        if (P.scheme == kImpNewmark) {
            double ui[4], vi[4];
            dyn_ld4(ut, r0, P.n, ui);
            dyn_ld4(vt, r0, P.n, vi);
#pragma unroll
            for (int k = 0; k < kDynRows; ++k) {
                x[k] = ui[k] + di[k];
                z[k] = di[k] / P.bdt2;
                y[k] = vi[k] + P.gdt * z[k];
            }
            imp_st4(a, r0, P.n, z);
        } else {
            double ui[4];
            dyn_ld4(u, r0, P.n, ui);
#pragma unroll
            for (int k = 0; k < kDynRows; ++k) {
                x[k] = ui[k] + di[k] / P.theta;
                y[k] = (x[k] - ui[k]) / P.dt;
            }
        }
        imp_st4(u, r0, P.n, x);
        imp_st4(v, r0, P.n, y);
    }
}

// the block's partials of a sampled step: sum m v^2 (theta-method: m u^2), u . w with w = K u, f . u; part = [3][nparts]
__global__ void __launch_bounds__(kBlock) k_imp_energy(ImpPar P, const double *__restrict__ f, const double *__restrict__ m,
                                                        const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                                                        double *part)
{
    __shared__ double sm[4];
    double T = 0.0, S = 0.0, W = 0.0;
    PFEM_IMP_CHUNKS(r0, P.n) {
        double fi[4], mi[4], ui[4], vi[4], wi[4];
        dyn_ld4(f, r0, P.n, fi);
        dyn_ld4(m, r0, P.n, mi);
        dyn_ld4(u, r0, P.n, ui);
        dyn_ld4(P.scheme == kImpNewmark ? v : u, r0, P.n, vi);
        dyn_ld4(w, r0, P.n, wi);
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) {
            T = T + mi[k] * (vi[k] * vi[k]);
            S = S + ui[k] * wi[k];
            W = W + fi[k] * ui[k];
        }
    }
    const double a = block_sum(T, sm), b = block_sum(S, sm), c = block_sum(W, sm);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a;
        part[gridDim.x + blockIdx.x] = b;
        part[2 * gridDim.x + blockIdx.x] = c;
    }
}

// ONE block: the history row [t, T, S, W, u at the probes, v at the probes] from the partials of k_imp_energy, in index order
__global__ void __launch_bounds__(kBlock) k_imp_row(double t, const double *part, int nparts, int n_probe, const int32_t *__restrict__ probe,
                                                     const double *__restrict__ u, const double *__restrict__ v, double *row)
{
    __shared__ double sm[4];
    const double T = sum_partials(part, nparts, sm);
    const double S = sum_partials(part + nparts, nparts, sm);
    const double W = sum_partials(part + 2 * nparts, nparts, sm);
    if (threadIdx.x == 0) {
        row[0] = t;
        row[1] = 0.5 * T;
        row[2] = 0.5 * S;
        row[3] = W;
    }
    for (int k = threadIdx.x; k < n_probe; k += kBlock) {
        row[4 + k] = u[probe[k]];
        row[4 + n_probe + k] = v[probe[k]];
    }
}

#undef PFEM_IMP_CHUNKS

}  // namespace pfem

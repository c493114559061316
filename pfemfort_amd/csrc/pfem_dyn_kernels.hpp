// pfem_dyn_kernels.hpp -- gfx950 kernels of the explicit dynamics (pfem_dynamics_*): the lumped mass
// per node, the Gershgorin bound of the stable step, the start and the central-difference step.  Included once by
// pfem_device.hip after pfem_kernels.hpp.  The translation unit is compiled with -ffp-contract=off and nothing here asks for
// an fma: apart from the product w = K u (the SpMV's own order) every value is a written-down sequence of IEEE operations
// that tests/dynamics_reference.py repeats.
#pragma once

#include "pfem_kernels.hpp"

namespace pfem {

// ---------------------------------------------------------------------------
// lumped mass per node, in the device's node order
// ---------------------------------------------------------------------------
// density at an element or a visit (AtElem / AtVisit): one value, or one per material row
struct DynDens {
    const double *tab;          // [n_mat] on the device, nullptr: `one`
    double one;
};
template <class AT> __device__ __forceinline__ double dens_at(const ElemPrm &, const DynDens &d, AT) { return d.one; }
template <class AT> __device__ __forceinline__ double dens_at(const ElemPrmTab &p, const DynDens &d, AT at) { return d.tab[prm_mat(p, at)]; }

template <int KIND>
__device__ __forceinline__ void dyn_load_xyz(const MeshDev &m, const int nd[4], double x[4], double y[4], double z[4])
{
    using P = PostKind<KIND>;
#pragma unroll
    for (int a = 0; a < P::NPE; ++a) {
        x[a] = m.xyz[nd[a]];
        y[a] = m.xyz[m.nNode + nd[a]];
        z[a] = P::NDIM == 3 ? m.xyz[2 * m.nNode + nd[a]] : 0.0;
    }
}

// Gather form: k_post_recovery_gather's walk over the node's own incidence records (ascending element id); the node's share
// elem_lumped_mass()[a] of every incident element is added in that order -- one writer per node, no atomics, the same bits in
// every run.  Hub nodes have no records: zero here, summed by k_dyn_mass_scatter restricted to them.
template <int KIND, class PRM = ElemPrm>
__global__ void __launch_bounds__(kBlock) k_dyn_mass_gather(MeshDev m, PRM prm, DynDens dens, const int64_t *__restrict__ inc_ptr,
                                                             const int32_t *__restrict__ inc_cnt, const int4 *__restrict__ inc_rec,
                                                             const uint8_t *__restrict__ node_hub, double *__restrict__ mnode, int *err)
{
    using P = PostKind<KIND>;
    const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (n >= m.nNode) return;
    double acc = 0.0;
    const int cnt = (node_hub && node_hub[n]) ? 0 : inc_cnt[n];
    const int64_t beg = inc_ptr[n >> 6] + (n & 63), end = beg + 64LL * cnt;
    for (int64_t t = beg; t < end; t += 64) {
        const int4 rc = inc_rec[t];
        const int a = static_cast<int>((static_cast<uint32_t>(rc.x) >> 31) | ((static_cast<uint32_t>(rc.y) >> 31) << 1));
        const int o[3] = {rc.x & 0x7fffffff, rc.y & 0x7fffffff, rc.z};
        int nd[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < P::NPE; ++i) {
            const int q = i < a ? i : (i > 0 ? i - 1 : 0);
            nd[i] = (i == a) ? static_cast<int>(n) : o[q];
        }
        double x[4], y[4], z[4], Mn[4];
        dyn_load_xyz<KIND>(m, nd, x, y, z);
        if (!elem_lumped_mass(KIND, x, y, z, prm_at(prm, AtVisit{t}), dens_at(prm, dens, AtVisit{t}), Mn)) { atomicMax(err, PFEM_ERR_NEG_JAC); continue; }
#pragma unroll
        for (int i = 0; i < P::NPE; ++i)
            if (i == a) acc += Mn[i];
    }
    mnode[n] = acc;
}

// Scatter form: one thread per element, f64 atomics into mnode (zeroed by the caller, or -- only_nodes != nullptr, the hub pass
// of the gather form -- by k_dyn_mass_gather at the flagged nodes, which alone are added to).
template <int KIND, class PRM = ElemPrm>
__global__ void __launch_bounds__(kBlock) k_dyn_mass_scatter(MeshDev m, PRM prm, DynDens dens, const uint8_t *__restrict__ only_nodes,
                                                              double *mnode, int *err)
{
    using P = PostKind<KIND>;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= m.nElem) return;
    int nd[4] = {0, 0, 0, 0};
    bool any = only_nodes == nullptr;
#pragma unroll
    for (int a = 0; a < P::NPE; ++a) {
        nd[a] = m.conn[a * m.nElem + e];
        if (only_nodes && only_nodes[nd[a]]) any = true;
    }
    if (!any) return;
    double x[4], y[4], z[4], Mn[4];
    dyn_load_xyz<KIND>(m, nd, x, y, z);
    if (!elem_lumped_mass(KIND, x, y, z, prm_at(prm, AtElem{e}), dens_at(prm, dens, AtElem{e}), Mn)) { atomicMax(err, PFEM_ERR_NEG_JAC); return; }
#pragma unroll
    for (int a = 0; a < P::NPE; ++a) {
        if (only_nodes && !only_nodes[nd[a]]) continue;
        add_f64(&mnode[nd[a]], Mn[a]);
    }
}

// m and 1 / m of every matrix row from its node: every element dof with a row stores its node's mass there (all elements of a
// node store the same value).  A row no element touches keeps the zeros the caller wrote: it has no matrix entries either, and
// 1 / m = 0 leaves its dof where it is.
__global__ void __launch_bounds__(kBlock) k_dyn_mass_rows(MeshDev m, const double *__restrict__ mnode, double *mrow, double *minv)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= m.nElem * m.nsize) return;
    const int64_t e = t % m.nElem;
    const int i = static_cast<int>(t / m.nElem);
    const int r = m.edof[t];
    if (r < 0) return;
    const double v = mnode[m.conn[(i / m.ndof) * m.nElem + e]];
    mrow[r] = v;
    minv[r] = v > 0.0 ? 1.0 / v : 0.0;
}

// per-block partial sums of the nodal masses (the total mass), block_sum's fixed order
__global__ void __launch_bounds__(kBlock) k_dyn_mass_total(int64_t nNode, const double *__restrict__ mnode, double *part)
{
    __shared__ double sm[4];
    double a = 0.0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < nNode; i += static_cast<int64_t>(gridDim.x) * kBlock) a += mnode[i];
    const double b = block_sum(a, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = b;
}

// ---------------------------------------------------------------------------
// stable step: max over the rows of (sum_j |K_ij|) / m_i, one thread per row of the assembled (row-form) matrix, the entries of
// a row in their stored (ascending column) order; per-block maxima (a maximum does not depend on the order)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_dyn_gershgorin(SellDev A, int64_t n_rows, const double *__restrict__ minv, double *part)
{
    __shared__ double sm[4];
    double best = 0.0;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < n_rows; r += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t base = A.slice_off[r >> 6] + (r & 63);
        const int len = A.rowlen[r];
        double a = 0.0;
        for (int k = 0; k < len; ++k) a = a + fabs(A.vals[base + 64LL * k]);
        best = fmax(best, a * minv[r]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_down(best, o, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

// ---------------------------------------------------------------------------
// the step
// ---------------------------------------------------------------------------
constexpr int kDynRows = 4;                          // consecutive rows per thread
constexpr int kDynBlockRows = kBlock * kDynRows;     // 1024 rows per block, the SpMV's rows per block on the 4-row forms

// Device control block.  step[] holds n, the index of the state u_n, twice: a launch with parity argument p reads step[p] and
// its first thread stores n + 1 into step[p ^ 1], which nobody in that launch reads; the next launch has the other parity.  So
// the counter advances on the device with no atomics and no fences, and a captured graph of an even number of steps can be
// replayed any number of times.  run_start is written by the host at the start of a run and only read here.
struct DynCtl {
    long long step[2];
    long long run_start;
};

// what stays the same for every step of a run (all of it is part of the graph key)
struct DynPar {
    int64_t n;                   // rows
    double t0, dt;               // t_n = t0 + n dt
    double c0, c1, a;            // 1 / dt^2, alpha / (2 dt), c0 + c1
    long long sample_every;
    int n_curve;                 // load curve: lambda(t) piecewise linear through (ct[k], cl[k]), constant outside; 0: lambda = 1
    const double *ct, *cl;
    int n_probe;
    const int32_t *probe;        // matrix rows of the probes
    double *hist;                // rows of ncol = 4 + 2 n_probe doubles
    int nb;                      // blocks of a step launch = partial sums per quantity
    double *part;                // [2][3][nb]: T, S, W partials of a sampled step n at parity n & 1
};

__device__ __forceinline__ double dyn_lambda(const DynPar &P, double t)
{
    if (P.n_curve <= 0) return 1.0;
    if (t <= P.ct[0]) return P.cl[0];
    if (t >= P.ct[P.n_curve - 1]) return P.cl[P.n_curve - 1];
    int lo = 0, hi = P.n_curve - 1;              // ct[lo] <= t < ct[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.ct[mid] <= t) lo = mid; else hi = mid;
    }
    return P.cl[lo] + (P.cl[hi] - P.cl[lo]) * ((t - P.ct[lo]) / (P.ct[hi] - P.ct[lo]));
}

// History row of the sampled step that led to state `step` (step - run_start a positive multiple of sample_every), written by
// ONE block after the launch boundary that made the step's partials and its u visible: [t, T, S, W, u at the probes, v at the
// probes] with u = u_step, up = u_{step-1}.  The partials are added in index order by sum_partials: the same bits in every run.
__device__ __forceinline__ void dyn_emit_row(const DynPar &P, long long step, long long run_start, const double *u, const double *up, double *sm)
{
    const long long done = step - run_start;
    if (done <= 0 || done % P.sample_every != 0) return;            // (uniform over the block)
    const double *part = P.part + static_cast<int64_t>((step - 1) & 1) * 3 * P.nb;
    const double T = sum_partials(part, P.nb, sm);
    const double S = sum_partials(part + P.nb, P.nb, sm);
    const double W = sum_partials(part + 2 * P.nb, P.nb, sm);
    const int ncol = 4 + 2 * P.n_probe;
    double *row = P.hist + (done / P.sample_every - 1) * ncol;
    if (threadIdx.x == 0) {
        row[0] = P.t0 + static_cast<double>(step) * P.dt;
        row[1] = 0.5 * T;
        row[2] = 0.5 * S;
        row[3] = W;
    }
    for (int k = threadIdx.x; k < P.n_probe; k += kBlock) {
        const int r = P.probe[k];
        row[4 + k] = u[r];
        row[4 + P.n_probe + k] = (u[r] - up[r]) / P.dt;
    }
}

// rows r0 .. r0 + 3 of a vector of n rows whose base is 16-byte aligned (r0 a multiple of 4): two 16-byte loads, zeros past the end
__device__ __forceinline__ void dyn_ld4(const double *__restrict__ p, int64_t r0, int64_t n, double v[4])
{
    if (r0 + kDynRows <= n) {
        const double2 a = *reinterpret_cast<const double2 *>(p + r0), b = *reinterpret_cast<const double2 *>(p + r0 + 2);
        v[0] = a.x;  v[1] = a.y;  v[2] = b.x;  v[3] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) v[k] = r0 + k < n ? p[r0 + k] : 0.0;
    }
}

// u_{-1} = u0 - dt v0 + dt^2 / 2 a0 with a0 = (lambda(t0) f - K u0) / m; w = K u0 by the SpMV before it
__global__ void __launch_bounds__(kBlock) k_dyn_start(DynPar P, const double *__restrict__ f, const double *__restrict__ minv,
                                                       const double *__restrict__ w, const double *__restrict__ u0,
                                                       const double *__restrict__ v0, double *__restrict__ um1)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const double lam = dyn_lambda(P, P.t0);
    const double a0 = (lam * f[i] - w[i]) * minv[i];
    um1[i] = (u0[i] - P.dt * v0[i]) + (0.5 * (P.dt * P.dt)) * a0;
}

// One central-difference step with mass-proportional damping C = alpha M, divided through by m:
//     u_{n+1} = [ c0 (2 u_n - u_{n-1}) + c1 u_{n-1} + (lambda(t_n) f - w) / m ] / (c0 + c1),      w = K u_n
// and, on a sampled step, the block's partial sums of   m v^2 (v = (u_{n+1} - u_n) / dt),   u_{n+1} w,   f u_{n+1}.
// Block b owns rows 1024 b .. 1024 b + 1023, thread t four consecutive ones; a thread adds its rows in ascending order, the
// block by block_sum.  `par` = n & 1 (see DynCtl); step_arg >= 0: n itself, for launches outside a graph.
// Block 0 first writes the history row of the step before, if that was a sampled one (dyn_emit_row).
__global__ void __launch_bounds__(kBlock) k_dyn_step(DynPar P, DynCtl *ctl, int par, long long step_arg, const double *__restrict__ f,
                                                      const double *__restrict__ m, const double *__restrict__ minv,
                                                      const double *__restrict__ w, const double *__restrict__ u,
                                                      const double *__restrict__ up, double *__restrict__ un)
{
    __shared__ double sm[4];
    __shared__ double s_lam;
    __shared__ long long s_step[2];
    __shared__ int s_sample;
    if (threadIdx.x == 0) {
        const long long n = step_arg >= 0 ? step_arg : ctl->step[par];
        s_step[0] = n;
        s_step[1] = ctl->run_start;
        s_sample = (n + 1 - s_step[1]) % P.sample_every == 0;
        s_lam = dyn_lambda(P, P.t0 + static_cast<double>(n) * P.dt);
        if (blockIdx.x == 0) ctl->step[par ^ 1] = n + 1;
    }
    __syncthreads();
    const long long step = s_step[0];
    const double lam = s_lam;
    const bool sample = s_sample != 0;
    if (blockIdx.x == 0) dyn_emit_row(P, step, s_step[1], u, up, sm);

    const int64_t r0 = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kDynRows;
    double T = 0.0, S = 0.0, W = 0.0;
    if (r0 < P.n) {
        double ui[4], pi[4], wi[4], fi[4], mi[4], qi[4], x[4];
        dyn_ld4(u, r0, P.n, ui);
        dyn_ld4(up, r0, P.n, pi);
        dyn_ld4(w, r0, P.n, wi);
        dyn_ld4(f, r0, P.n, fi);
        dyn_ld4(m, r0, P.n, mi);
        dyn_ld4(minv, r0, P.n, qi);
#pragma unroll
        for (int k = 0; k < kDynRows; ++k) {                          // (rows past the end read zeros and add zeros)
            x[k] = (((2.0 * ui[k] - pi[k]) * P.c0 + P.c1 * pi[k]) + (lam * fi[k] - wi[k]) * qi[k]) / P.a;
            const double v = (x[k] - ui[k]) / P.dt;
            T = T + mi[k] * (v * v);
            S = S + x[k] * wi[k];
            W = W + fi[k] * x[k];
        }
        if (r0 + kDynRows <= P.n) {
            *reinterpret_cast<double2 *>(un + r0) = make_double2(x[0], x[1]);
            *reinterpret_cast<double2 *>(un + r0 + 2) = make_double2(x[2], x[3]);
        } else {
#pragma unroll
            for (int k = 0; k < kDynRows; ++k)
                if (r0 + k < P.n) un[r0 + k] = x[k];
        }
    }
    if (sample) {                                                     // (uniform over the grid)
        double *part = P.part + static_cast<int64_t>(step & 1) * 3 * P.nb;
        const double a = block_sum(T, sm), b = block_sum(S, sm), c = block_sum(W, sm);
        if (threadIdx.x == 0) {
            part[blockIdx.x] = a;
            part[P.nb + blockIdx.x] = b;
            part[2 * P.nb + blockIdx.x] = c;
        }
    }
}

// the history row of a run's last step, when that was a sampled one: u = u_n, up = u_{n-1} of the final state n = `step`
__global__ void __launch_bounds__(kBlock) k_dyn_flush(DynPar P, long long step, long long run_start, const double *__restrict__ u,
                                                       const double *__restrict__ up)
{
    __shared__ double sm[4];
    dyn_emit_row(P, step, run_start, u, up, sm);
}

// v_{n-1/2} = (u_n - u_{n-1}) / dt (pfem_dynamics_get_state)
__global__ void __launch_bounds__(kBlock) k_dyn_velocity(int64_t n, double dt, const double *__restrict__ u, const double *__restrict__ up,
                                                          double *__restrict__ v)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) v[i] = (u[i] - up[i]) / dt;
}

}  // namespace pfem

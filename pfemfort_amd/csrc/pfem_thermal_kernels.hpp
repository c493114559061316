// pfem_thermal_kernels.hpp -- gfx950 kernels of the thermal strains (pfem_thermal_* / pfem_rhs_add_thermal_load; DESIGN.md
// section 14): the handover of a temperature field from one handle to another and the thermal load of the elasticity kinds.
// Included once by pfem_device.hip after pfem_kernels.hpp.  The stresses under a thermal state are the post-processing kernels
// of pfem_kernels.hpp instantiated with ElemPrmTh<.>.  The translation unit is compiled with -ffp-contract=off: every value is
// the written-down sequence of IEEE operations of pfem_elem.hpp (thermal_strain, elem_thermal_load) that
// tests/thermal_reference.py repeats.
#pragma once

#include "pfem_kernels.hpp"

namespace pfem {

// theta[i] = field[map[i]] - t_ref, one thread per node of the receiving handle: `field` is the giving handle's nodal field in ITS
// device order, map[i] the giving handle's device node of the receiving handle's device node i (nullptr: the same order).
__global__ void __launch_bounds__(kBlock) k_thermal_carry(int64_t nNode, const int32_t *__restrict__ map, const double *__restrict__ field,
                                                           double t_ref, double *__restrict__ theta)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= nNode) return;
    theta[i] = field[map ? static_cast<int64_t>(map[i]) : i] - t_ref;
}

// Thermal load per node, gather form: k_post_forces_gather's walk over the node's own incidence records (ascending element id);
// the node's rows of elem_thermal_load of every incident element are added in that order -- one writer per entry, no atomics, the
// same bits in every run.  Fn[node * NDOF + d], in the device's node order; k_thermal_load_rows adds it to the right-hand side.
// Hub nodes have no records: zeros here, and k_thermal_load_scatter restricted to them adds straight to their rows.
// Traffic per record: 16 B of record, (NPE - 1) (NDIM + 1) doubles of the other nodes through L2.
template <int KIND, class PRM>
__global__ void __launch_bounds__(kBlock) k_thermal_load_gather(MeshDev m, PRM prm, const int64_t *__restrict__ inc_ptr,
                                                                 const int32_t *__restrict__ inc_cnt, const int4 *__restrict__ inc_rec,
                                                                 const uint8_t *__restrict__ node_hub, double *__restrict__ Fn, int *err)
{
    using P = PostKind<KIND>;
    const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (n >= m.nNode) return;
    double acc[P::NDOF];
#pragma unroll
    for (int d = 0; d < P::NDOF; ++d) acc[d] = 0.0;
    const int cnt = (node_hub && node_hub[n]) ? 0 : inc_cnt[n];
    const int64_t beg = inc_ptr[n >> 6] + (n & 63), end = beg + 64LL * cnt;
    for (int64_t t = beg; t < end; t += 64) {
        int nd[4] = {0, 0, 0, 0};
        const int a = inc_rec_nodes<P::NPE>(inc_rec[t], n, nd);
        double x[4], y[4], z[4], F[12];
#pragma unroll
        for (int i = 0; i < P::NPE; ++i) {
            x[i] = m.xyz[nd[i]];
            y[i] = m.xyz[m.nNode + nd[i]];
            z[i] = P::NDIM == 3 ? m.xyz[2 * m.nNode + nd[i]] : 0.0;
        }
        const double eth = prm_thermal_strain<KIND>(prm, AtVisit{t}, nd);
        if (!elem_thermal_load(KIND, x, y, z, prm_at(prm, AtVisit{t}), eth, F, nullptr)) { atomicMax(err, PFEM_ERR_NEG_JAC); continue; }
#pragma unroll
        for (int i = 0; i < P::NPE; ++i)
            if (i == a) {
#pragma unroll
                for (int d = 0; d < P::NDOF; ++d) acc[d] += F[P::NDOF * i + d];
            }
    }
#pragma unroll
    for (int d = 0; d < P::NDOF; ++d) Fn[n * P::NDOF + d] = acc[d];
}

// rhs[row] += Fn[i] for every node dof i with a matrix row (node_row[i] >= 0: the free dofs); one writer per row, no atomics
__global__ void __launch_bounds__(kBlock) k_thermal_load_rows(int64_t n, const int32_t *__restrict__ node_row, const double *__restrict__ Fn,
                                                               double *__restrict__ rhs)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const int r = node_row[i];
    if (r >= 0) rhs[r] = rhs[r] + Fn[i];
}

// The same load, scatter form: one thread per element, f64 atomics straight into the rows of the element's free dofs (m.edof, as
// k_surface_load).  only_nodes != nullptr: the hub pass of the gather form -- only the dofs of flagged nodes are added.
template <int KIND, class PRM>
__global__ void __launch_bounds__(kBlock) k_thermal_load_scatter(MeshDev m, PRM prm, const uint8_t *__restrict__ only_nodes, double *rhs, int *err)
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
    double x[4], y[4], z[4], F[12];
#pragma unroll
    for (int a = 0; a < P::NPE; ++a) {
        x[a] = m.xyz[nd[a]];
        y[a] = m.xyz[m.nNode + nd[a]];
        z[a] = P::NDIM == 3 ? m.xyz[2 * m.nNode + nd[a]] : 0.0;
    }
    const double eth = prm_thermal_strain<KIND>(prm, AtElem{e}, nd);
    if (!elem_thermal_load(KIND, x, y, z, prm_at(prm, AtElem{e}), eth, F, nullptr)) { atomicMax(err, PFEM_ERR_NEG_JAC); return; }
#pragma unroll
    for (int a = 0; a < P::NPE; ++a) {
        if (only_nodes && !only_nodes[nd[a]]) continue;
#pragma unroll
        for (int d = 0; d < P::NDOF; ++d) {
            const int r = m.edof[(a * P::NDOF + d) * m.nElem + e];
            if (r >= 0) add_f64(&rhs[r], F[P::NDOF * a + d]);
        }
    }
}

}  // namespace pfem

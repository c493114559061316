"""The reference of the per-element-material tests checks itself first: the numpy mirror of the oracle's assembly loop
(tests/materials_reference.py) reproduces oracle.assemble bit for bit, and with two materials it reproduces a closed form."""
import numpy as np
import pytest

import materials_reference as MR
from oracle import pfem_oracle as O
from pfemfort_amd import host as H


def _omesh(m):
    return O.Mesh(m.xyz, m.conn, m.bc_node, m.bc_dof, m.bc_val)


def _mesh(name, golden_dir):
    if name == "tet10":
        return O.POISSON_TET, np.array([1.3, 0.7, 2.1]), H.read_mesh(f"{golden_dir}/input/tet10")
    if name == "beam":
        return O.ELAST_TET, H.ELAST_ELEMDATA, H.gen_box_tets(-0.5, 0.5, 3, 0.0, 6.0, 12, -0.5, 0.5, 3, bc_mode=1, ndof=3)
    if name == "tria20":
        return O.POISSON_TRIA, np.array([1.5, 0.5]), H.read_mesh(f"{golden_dir}/input/tria20x20")
    return O.ELAST_TRIA, np.array([H.ELAST_ELEMDATA[0], H.ELAST_ELEMDATA[1], 0.5, 0.05, -0.02]), \
        H.read_mesh(f"{golden_dir}/input/cookmembranetria32")


@pytest.mark.parametrize("name", ["tet10", "beam", "tria20", "cook"])
def test_mirror_with_one_material_is_the_oracle_bit_for_bit(name, golden_dir):
    kind, ed, mesh = _mesh(name, golden_dir)
    if name == "beam":                     # nonzero Dirichlet values at partially constrained nodes: the lifting does something
        rng = np.random.default_rng(2)
        keep = rng.random(len(mesh.bc_node)) < 0.6
        extra = np.arange(40, 60, dtype=np.int32)
        mesh = H.Mesh(mesh.xyz, mesh.conn, np.concatenate([mesh.bc_node[keep], extra]),
                      np.concatenate([mesh.bc_dof[keep], extra % 3]).astype(np.int32),
                      np.concatenate([rng.standard_normal(keep.sum()) * 0.01, rng.standard_normal(20) * 0.01]))
    prob = O.setup_problem(kind, _omesh(mesh), elemData=ed)
    got = MR.setup_problem(kind, mesh, ed[None, :], np.zeros(mesh.nElem, np.int32))
    assert np.array_equal(got.rowptr, prob.rowptr) and np.array_equal(got.cols, prob.cols)
    assert np.abs(prob.vals).max() > 0 and np.abs(prob.rhs).max() > 0
    assert np.array_equal(got.vals, prob.vals)
    assert np.array_equal(got.rhs, prob.rhs)
    # ... and split over three identical rows by a random map it still is
    ids = np.random.default_rng(5).integers(0, 3, mesh.nElem).astype(np.int32)
    got3 = MR.setup_problem(kind, mesh, np.tile(ed, (3, 1)), ids)
    assert np.array_equal(got3.vals, prob.vals) and np.array_equal(got3.rhs, prob.rhs)


def test_two_material_bar_in_closed_form():
    """sigma = delta / (1/E1 + 1/E2), u_x piecewise linear, u_y = u_z = 0: mirror matrix + direct solve to 1e-12 (delta = 1)."""
    mesh, table, elem_mat, sigma, ux = MR.bar(H, delta=1.0)
    assert sigma == 1.0 / (1.0 / 100.0 + 1.0 / 400.0)
    assert 0 < elem_mat.sum() < mesh.nElem and elem_mat.sum() * 2 == mesh.nElem
    p = MR.setup_problem(O.ELAST_TET, mesh, table, elem_mat)
    u = MR.full_field(p, MR.direct_solve(p))
    exact = np.zeros_like(u)
    exact[:, 0] = ux(p.xyz_new[0])
    err = np.abs(u - exact).max()
    print(f"two-E bar: max |u - exact| = {err:.3e}")
    assert err <= 1e-12
    # a uniform bar of either material gives another answer: the map is what the closed form sees
    for m in (0, 1):
        q = MR.setup_problem(O.ELAST_TET, mesh, table, np.full(mesh.nElem, m, np.int32))
        assert np.abs(MR.full_field(q, MR.direct_solve(q)) - exact).max() > 1e-3

"""Nodal recovery and the Zienkiewicz-Zhu indicator on the host: the per-element routines (pfem_post_scalar,
pfem_elem_recovery_error) against the numpy reference, the VTK writer with further arrays (pfem_write_vtk_fields), and the
reference itself on a solution whose exact flux is known."""
import os

import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import host as H
import post_reference as R
from test_post_host import _cases, _post

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "elements.npz"))


@pytest.fixture(scope="module")
def cook(golden_dir):
    return H.read_mesh(os.path.join(golden_dir, "input", "cookmembranetria32"))


def _thick(kind, ed):
    return float(ed[2]) if kind == L.ELAST_TRIA else 1.0


def _recovery_error(kind, xyz, nd, ed, valC, nodal):
    z = xyz[2, nd] if xyz.shape[0] == 3 else None
    return H.ElementRecoveryError(kind, xyz[0, nd], xyz[1, nd], z, ed, valC, nodal)


def test_recovery_error_equals_the_closed_form(gold, cook):
    """All five kinds, random elements and random nodal values: eta2 and flux_norm2 within 1e-13 relative of numpy's closed form
    (flux from pfem_elem_post, volume from the coordinates); nodal == flux at every node gives 0.0 exactly."""
    rng = np.random.default_rng(20261019)
    for name, kind, xyz, conn, ed, _ in _cases(gold, cook):
        npe, ng, ns = L.NPELEM[kind], L.NG[kind], L.NPELEM[kind] * L.NDOF[kind]
        w = R.element_weights(xyz, conn, _thick(kind, ed))
        worst = 0.0
        for e in range(conn.shape[1]):
            nd = conn[:, e]
            valC = rng.standard_normal(ns)
            flux = _post(kind, xyz, nd, ed, valC)[1]
            nodal = flux + np.abs(flux).max() * rng.standard_normal((npe, ng))
            eta2, fn2 = _recovery_error(kind, xyz, nd, ed, valC, nodal)
            loc = np.arange(npe)[:, None]                    # the reference on a one-element mesh
            want_e, want_f = R.indicator(loc, w[e:e + 1], flux[:, None], nodal)
            worst = max(worst, abs(eta2 - want_e[0]) / want_e[0], abs(fn2 - want_f[0]) / want_f[0])
            assert abs(eta2 - want_e[0]) <= 1e-13 * want_e[0], (name, e, eta2, want_e)
            assert abs(fn2 - want_f[0]) <= 1e-13 * want_f[0], (name, e, fn2, want_f)
            zero, fn2b = _recovery_error(kind, xyz, nd, ed, valC, np.tile(flux, (npe, 1)))
            assert zero == 0.0 and fn2b == fn2, (name, e, zero)
        print(f"{name}: worst relative deviation from the closed form = {worst:.3e}")


def test_post_scalar_is_the_scalar_of_elem_post(gold, cook):
    rng = np.random.default_rng(5)
    for name, kind, xyz, conn, ed, _ in _cases(gold, cook):
        ns = L.NPELEM[kind] * L.NDOF[kind]
        for e in range(conn.shape[1]):
            _, flux, sc, _ = _post(kind, xyz, conn[:, e], ed, rng.standard_normal(ns))
            got = H.PostScalar(kind, flux)
            assert abs(got - sc) <= 4 * EPS * sc, (name, e, got, sc)
    assert np.array_equal(H.PostScalar(L.POISSON_TET, np.array([[3.0, 4.0, 12.0], [0.0, 0.0, 0.0]])), [13.0, 0.0])
    assert H.PostScalar(L.ELAST_TET, np.array([2.0, 2.0, 2.0, 0.0, 0.0, 0.0])) == 0.0          # hydrostatic


def test_error_codes(gold):
    xyz, nd = gold["rt_xyz"], gold["rt_conn"][[1, 0, 2, 3], 0]
    with pytest.raises(pf.PfemError) as ei:
        _recovery_error(L.ELAST_TET, xyz, nd, gold["rt_elast_data"], np.zeros(12), np.zeros((4, 6)))
    assert ei.value.code == L.ERR_NEG_JAC
    xy, n3 = gold["rtri_xy"], gold["rtri_conn"][[1, 0, 2], 0]
    with pytest.raises(pf.PfemError) as ei:
        _recovery_error(L.POISSON_TRIA, xy, n3, gold["rtri_data"], np.zeros(3), np.zeros((3, 2)))
    assert ei.value.code == L.ERR_NEG_JAC
    for kind in (0, 6, -1):
        assert L.lib().pfem_elem_recovery_error(kind, None, None, None, None, None, None, None, None) == L.ERR_ARG
        assert L.lib().pfem_post_scalar(kind, None, None) == L.ERR_ARG


# ---- the writer -----------------------------------------------------------------------------------------------------
def parse_vtk_array(text, section, name, n):
    """(keyword, values (n, ncomp)) of array `name` inside CELL_DATA / POINT_DATA of a legacy ASCII file."""
    lines = text.split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(section))
    k = next(i for i in range(start, len(lines)) if lines[i].split()[:2] in (["SCALARS", name], ["VECTORS", name], ["TENSORS", name]))
    key = lines[k].split()[0]
    if key == "SCALARS":
        assert lines[k] == f"SCALARS {name} float 1" and lines[k + 1] == "LOOKUP_TABLE default"
        return key, np.array([float(v) for v in lines[k + 2:k + 2 + n]]).reshape(n, 1)
    assert lines[k] == f"{key} {name} float"
    if key == "VECTORS":
        return key, np.array([[float(v) for v in ln.split()] for ln in lines[k + 1:k + 1 + n]]).reshape(n, 3)
    body = lines[k + 1:k + 1 + 4 * n]
    assert all(body[4 * i + 3] == "" for i in range(n))          # a blank line after each tensor
    return key, np.array([[float(v) for r in range(3) for v in body[4 * i + r].split()] for i in range(n)]).reshape(n, 9)


def _writer_cases(golden_dir):
    tet = H.read_mesh(os.path.join(golden_dir, "input", "tet10"))
    tri = H.read_mesh(os.path.join(golden_dir, "input", "tria20x20"))
    rng = np.random.default_rng(1)
    return [("tet10 scalar", 3, tet, rng.standard_normal((tet.nNode, 1))),
            ("tet10 vector", 3, tet, rng.standard_normal((tet.nNode, 3))),
            ("tria20x20", 2, tri, rng.standard_normal((tri.nNode, 1)))]


def test_writer_without_arrays_writes_the_plain_file(golden_dir, tmp_path):
    for name, ndim, m, soln in _writer_cases(golden_dir):
        pid = (np.arange(m.nElem) % 3).astype(np.int32)
        a, b = tmp_path / "plain.vtk", tmp_path / "fields.vtk"
        H.writeoutputvtk(ndim, m.xyz, m.conn, pid, soln, a, ndof=soln.shape[1])
        H.writeoutputvtk_fields(ndim, m.xyz, m.conn, pid, soln, b, ndof=soln.shape[1])
        assert a.read_bytes() == b.read_bytes(), name


def test_writer_arrays_parse_back(golden_dir, tmp_path):
    rng = np.random.default_rng(2)
    for name, ndim, m, soln in _writer_cases(golden_dir):
        pid = (np.arange(m.nElem) % 3).astype(np.int32)
        scale = lambda n, k: rng.standard_normal((n, k)) * 10.0 ** rng.integers(-9, 9, (n, 1))      # noqa: E731
        cell = {"eta": scale(m.nElem, 1)[:, 0], "flux": scale(m.nElem, 3), "stress": scale(m.nElem, 9)}
        point = {"q": scale(m.nNode, 3), "vm": scale(m.nNode, 1)[:, 0], "sigma": scale(m.nNode, 9)}
        a, b = tmp_path / "plain.vtk", tmp_path / "fields.vtk"
        H.writeoutputvtk(ndim, m.xyz, m.conn, pid, soln, a, ndof=soln.shape[1])
        H.writeoutputvtk_fields(ndim, m.xyz, m.conn, pid, soln, b, ndof=soln.shape[1], cell_fields=cell, point_fields=point)
        plain, got = a.read_bytes(), b.read_bytes()
        cut = plain.index(b"POINT_DATA")
        assert got.startswith(plain[:cut]), name                     # everything up to the end of the procid block
        at = got.index(b"POINT_DATA")
        assert got[at:at + len(plain) - cut] == plain[cut:], name     # the solution block
        assert got.count(b"CELL_DATA") == 1 and got.count(b"POINT_DATA") == 1
        text = got.decode()
        # the new blocks come in the order given: cell arrays between procid and POINT_DATA, point arrays after the solution
        order = [ln.split()[1] for ln in text.split("\n") if ln.split()[:1] and ln.split()[0] in ("SCALARS", "VECTORS", "TENSORS")]
        assert order == ["procid", "eta", "flux", "stress", "solution", "q", "vm", "sigma"], (name, order)
        for section, fields, n in (("CELL_DATA", cell, m.nElem), ("POINT_DATA", point, m.nNode)):
            for fname, want in fields.items():
                want = want.reshape(n, -1)
                key, vals = parse_vtk_array(text, section, fname, n)
                assert key == {1: "SCALARS", 3: "VECTORS", 9: "TENSORS"}[want.shape[1]]
                assert np.all(np.abs(vals - want) <= 5e-9 * np.abs(want)), (name, fname)
        # one item per line, %16.8E per value
        k = text.split("\n").index("VECTORS q float")
        assert len(text.split("\n")[k + 1]) == 48


def test_writer_expands_voigt_and_pads_two_vectors(golden_dir, tmp_path):
    m = H.read_mesh(os.path.join(golden_dir, "input", "tria20x20"))
    pid = np.zeros(m.nElem, np.int32)
    rng = np.random.default_rng(3)
    v6, v3, v2 = rng.standard_normal((m.nElem, 6)), rng.standard_normal((m.nNode, 3)), rng.standard_normal((m.nElem, 2))
    out = tmp_path / "f.vtk"
    H.writeoutputvtk_fields(2, m.xyz, m.conn, pid, np.zeros(m.nNode), out, cell_fields={"s6": v6, "q2": v2},
                            point_fields={"s3": v3}, voigt=("s3",))
    text = out.read_text()
    key, t = parse_vtk_array(text, "CELL_DATA", "s6", m.nElem)
    xx, yy, zz, xy, yz, zx = v6.T
    want = np.stack([xx, xy, zx, xy, yy, yz, zx, yz, zz], axis=1)
    assert key == "TENSORS" and np.all(np.abs(t - want) <= 5e-9 * np.abs(want))
    key, t = parse_vtk_array(text, "POINT_DATA", "s3", m.nNode)
    z = np.zeros(m.nNode)
    want = np.stack([v3[:, 0], v3[:, 2], z, v3[:, 2], v3[:, 1], z, z, z, z], axis=1)
    assert key == "TENSORS" and np.all(np.abs(t - want) <= 5e-9 * np.abs(want))
    key, t = parse_vtk_array(text, "CELL_DATA", "q2", m.nElem)
    assert key == "VECTORS" and np.all(np.abs(t[:, :2] - v2) <= 5e-9 * np.abs(v2)) and np.all(t[:, 2] == 0.0)


def test_writer_rejects_bad_arrays(golden_dir, tmp_path):
    m = H.read_mesh(os.path.join(golden_dir, "input", "tet10"))
    pid = np.zeros(m.nElem, np.int32)
    soln = np.zeros(m.nNode)
    bad = [dict(cell_fields={"four": np.zeros((m.nElem, 4))}), dict(point_fields={"five": np.zeros((m.nNode, 5))}),
           dict(cell_fields={"two words": np.zeros(m.nElem)}), dict(point_fields={"": np.zeros(m.nNode)}),
           dict(point_fields={"tab\tbed": np.zeros(m.nNode)})]
    for kw in bad:
        with pytest.raises(pf.PfemError) as ei:
            H.writeoutputvtk_fields(3, m.xyz, m.conn, pid, soln, tmp_path / "bad.vtk", **kw)
        assert ei.value.code == L.ERR_ARG, kw


# ---- the reference on an exact solution -------------------------------------------------------------------------------
def test_indicator_on_an_exact_solution():
    """u = x^2+y^2+z^2 on the box [-1,1]^3, unit conductivity, q = -2x: the indicator against the error measured with the exact
    flux at the nodes through the same closed form.  Pins the reference itself: effectivity near 1, first order in h."""
    r4, r8 = R.exact_box(4), R.exact_box(8)
    for n, r in ((4, r4), (8, r8)):
        print(f"n = {n}: eta = {r['eta']:.5f}, true error = {r['true']:.5f}, effectivity = {r['eta'] / r['true']:.4f}")
        assert 0.95 <= r["eta"] / r["true"] <= 1.05
    assert 1.9 <= r4["eta"] / r8["eta"] <= 2.1

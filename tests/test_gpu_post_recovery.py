"""Nodal recovery, the Zienkiewicz-Zhu indicator and the VTK file with fields on the device (pfem_post_nodal_recovery,
pfem_post_error_indicator, Result.write_outputs(fields=True)) against the numpy reference of post_reference.py, the host's
per-element routine and closed forms, on the meshes of test_gpu_post.py."""
import ctypes as C

import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import _lib as L
from pfemfort_amd import drivers as D
from pfemfort_amd import host as H
import post_reference as R
from test_gpu_parity import _shuffled
from test_gpu_post import NAMES, Case, _mesh, case  # noqa: F401  (`case` is the fixture: one Case per mesh for the whole run)
from test_post_host import linear_field_expectation
from test_post_recovery_host import parse_vtk_array

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
_REF = {}


def _thick(c):
    return float(c.ed[2]) if c.kind == pf.ELAST_TRIA else 1.0


def _reference(c, u, field, key=None):
    """(nodal, weight, B, cnt) of the numpy reference for the element field the device computes from u (bit for bit the host
    routine's: test_gpu_post.py) and the weights from the coordinates -- computed once per (mesh, field) for the case's own u."""
    if key is not None and (key, field) in _REF:
        return _REF[(key, field)]
    grad, flux, _ = c.s.elementFields(c.ed, u)
    w = R.element_weights(c.xyz, c.conn, _thick(c))
    out = R.recover(c.conn, w, flux if field == "flux" else grad, c.nNode) + (w, flux)
    if key is not None:
        _REF[(key, field)] = out
    return out


def _within_bound(got, ref, B, cnt, what):
    """|got - ref| <= (2 cnt + 8) eps B per entry: two sums of cnt terms and a division, on both sides."""
    bound = (2 * cnt + 8).reshape((-1,) + (1,) * (got.ndim - 1)) * EPS * B
    dev = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, dev / bound, np.where(dev > 0, np.inf, 0.0)))
    print(f"{what}: worst |got - ref| / bound = {worst:.3e}")
    assert np.all(dev <= bound), what


@pytest.mark.parametrize("field", ["flux", "grad"])
@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_recovery_equals_the_reference(case, mode, field):
    c = case
    nodal_ref, w_ref, B, cnt, _, _ = _reference(c, c.u, field, c.name)
    if c.name.startswith("hub"):
        assert c.s.assemblyInfo()["hub_nodes"] >= 1              # the restricted atomic pass is on the gather form's path
    c.s.setAssemblyMode(mode)
    try:
        nodal, sc, w = c.s.nodalRecovery(c.ed, c.u, field)
        again = c.s.nodalRecovery(c.ed, c.u, field)
    finally:
        c.s.setAssemblyMode("gather")
    assert nodal.shape == (c.nNode, L.NG[c.kind]) and w.shape == (c.nNode,)
    _within_bound(nodal, nodal_ref, B, cnt, f"{c.name}/{mode}/{field} nodal")
    _within_bound(w, w_ref, w_ref, cnt, f"{c.name}/{mode}/{field} weight")
    if field == "flux":
        want = H.PostScalar(c.kind, nodal)
        assert sc.shape == (c.nNode,) and np.all(np.abs(sc - want) <= 4 * EPS * want)
    else:
        assert sc is None
    if mode == "gather" and c.s.assemblyInfo()["hub_nodes"] == 0:
        for a, b in zip((nodal, sc, w), again):
            assert (a is None and b is None) or np.array_equal(a, b)
    else:
        _within_bound(again[0], nodal_ref, B, cnt, f"{c.name}/{mode}/{field} nodal, second call")


def test_scalar_of_the_gradient_is_refused(golden_dir):
    c = Case(*_mesh("tet10", golden_dir))
    ed, u = np.ascontiguousarray(c.ed, dtype=np.float64), np.ascontiguousarray(c.u)
    nodal, sc = np.empty((c.nNode, 3)), np.empty(c.nNode)
    rc = L.lib().pfem_post_nodal_recovery(c.s._h, ed.ctypes.data, u.ctypes.data, 1, nodal.ctypes.data, sc.ctypes.data, None)
    assert rc == L.ERR_ARG
    assert L.lib().pfem_post_nodal_recovery(c.s._h, ed.ctypes.data, u.ctypes.data, 2, nodal.ctypes.data, None, None) == L.ERR_ARG
    # any output may be NULL
    w = np.empty(c.nNode)
    L.check(L.lib().pfem_post_nodal_recovery(c.s._h, ed.ctypes.data, u.ctypes.data, 0, None, None, w.ctypes.data), "recovery")
    assert np.array_equal(w, c.s.nodalRecovery(c.ed, c.u)[2])
    tot = C.c_double(0)
    L.check(L.lib().pfem_post_error_indicator(c.s._h, ed.ctypes.data, u.ctypes.data, None, C.byref(tot), None), "indicator")
    assert tot.value == c.s.errorIndicator(c.ed, c.u)[1]


@pytest.mark.parametrize("case", ["tet10", "beam", "tria20", "tria20inline", "cook"], indirect=True)
def test_linear_field_is_recovered(case):
    """u = a + G x, all five kinds: every element has the same flux, so the recovered value equals every incident element's within
    64 cnt eps |f|, and the indicator vanishes: eta2_total <= (1e-12)^2 flux_norm2_total (the numpy reference: 2.5e-16 relative)."""
    c = case
    rng = np.random.default_rng(3)
    ndim = c.xyz.shape[0]
    G = np.zeros((3, ndim))
    G[:c.ndof] = rng.standard_normal((c.ndof, ndim))
    a0 = rng.standard_normal(3)
    u = (a0[:c.ndof, None] + G[:c.ndof] @ c.xyz).T
    _, flux, _ = c.s.elementFields(c.ed, u)
    nodal, sc, _ = c.s.nodalRecovery(c.ed, u)
    cnt = np.bincount(c.conn.ravel(), minlength=c.nNode)
    fmag = np.abs(flux).max(0)                                           # |f| of each element
    worst = 0.0
    for a in range(c.npe):
        nd = c.conn[a]
        dev = np.abs(nodal[nd] - flux.T)
        bound = (64 * cnt[nd] * EPS * fmag)[:, None]
        worst = max(worst, (dev / bound).max())
        assert np.all(dev <= bound), (c.name, a)
    _, f_exact, sc_exact, _ = linear_field_expectation(c.kind, c.ed, G)
    eta2, tot, fn = c.s.errorIndicator(c.ed, u)
    print(f"{c.name}: worst |nodal - f_e| / bound = {worst:.3e}, eta2_total / flux_norm2_total = {tot / fn:.3e}")
    assert tot <= 1e-24 * fn
    used = cnt > 0
    assert np.all(np.abs(nodal[used] - f_exact) <= 1e-10 * np.abs(f_exact).max())
    assert np.all(np.abs(sc[used] - sc_exact) <= 1e-10 * sc_exact)


def _host_indicator(c, u, nodal):
    eta2 = np.empty(c.nElem); fn2 = np.empty(c.nElem)
    for e in range(c.nElem):
        nd = c.conn[:, e]
        z = c.xyz[2, nd] if c.xyz.shape[0] == 3 else None
        eta2[e], fn2[e] = H.ElementRecoveryError(c.kind, c.xyz[0, nd], c.xyz[1, nd], z, c.ed, u[nd].ravel(), nodal[nd])
    return eta2, fn2


def _check_indicator(c, u, what):
    """eta2[e] against the host's routine fed with the device's own recovered values: the same source, another order of the
    gathers -- to rounding; the totals against the sum of the entries."""
    nodal = c.s.nodalRecovery(c.ed, u)[0]
    eta2, tot, fn = c.s.errorIndicator(c.ed, u)
    want, fn2 = _host_indicator(c, u, nodal)
    bound = 1e-13 * (want + EPS * fn2)
    print(f"{what}: worst |eta2 - host| / bound = {(np.abs(eta2 - want) / bound).max():.3e}, "
          f"totals off by {abs(tot - eta2.sum()) / eta2.sum():.3e}, {abs(fn - fn2.sum()) / fn2.sum():.3e}")
    assert eta2.shape == (c.nElem,) and np.all(np.abs(eta2 - want) <= bound), what
    assert abs(tot - eta2.sum()) <= 1e-12 * eta2.sum() and abs(fn - fn2.sum()) <= 1e-12 * fn2.sum(), what
    return nodal, eta2, tot, fn


@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_indicator_equals_the_host_routine(case):
    c = case
    _, eta2, tot, fn = _check_indicator(c, c.u, c.name)
    if c.s.assemblyInfo()["hub_nodes"] == 0:                          # gather form: reproducible entries and totals
        again = c.s.errorIndicator(c.ed, c.u)
        assert np.array_equal(eta2, again[0]) and (tot, fn) == again[1:]
    # ... and against the reference end to end: a relative rounding error of cnt eps in the nodal values (cnt <= 300 here) moves
    # eta2 by about cnt eps |f| / |d| relative, and |d| is of the size of |f| for a random u -- orders below 1e-10
    nodal_ref, _, B, cnt, w, flux = _reference(c, c.u, "flux", c.name)
    ref, _ = R.indicator(c.conn, w, flux, nodal_ref)
    assert abs(tot - ref.sum()) <= 1e-10 * ref.sum()


def test_the_generated_box(golden_dir):
    """generateBoxMesh 8^3 with u = x^2+y^2+z^2: effectivity and totals of the CPU test's reference run, and the uploaded box's
    results."""
    r = R.exact_box(8)
    sz = H.box_slab_sizes(8, 8, 8, 0, 1)
    g = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    g.generateBoxMesh(pf.POISSON_TET, -1, 1, 8, -1, 1, 8, -1, 1, 8)
    g.buildPattern()
    ed = H.POISSON_ELEMDATA
    eta2, tot, fn = g.errorIndicator(ed, r["u"])
    nodal, _, w = g.nodalRecovery(ed, r["u"])
    eff, eff_ref = np.sqrt(tot) / r["true"], r["eta"] / r["true"]
    print(f"eta = {np.sqrt(tot):.5f}, effectivity = {eff:.4f} (reference {eff_ref:.4f})")
    assert abs(eff - eff_ref) <= 1e-10 * eff_ref and 0.95 <= eff <= 1.05
    assert abs(tot - r["eta2_total"]) <= 1e-10 * r["eta2_total"] and abs(fn - r["fnorm2_total"]) <= 1e-10 * r["fnorm2_total"]
    c = Case(pf.POISSON_TET, ed, r["mesh"])
    _, _, B, cnt = R.recover(c.conn, R.element_weights(c.xyz, c.conn), r["flux"], c.nNode)
    _within_bound(nodal, r["nodal"], B, cnt, "generated box nodal")
    _within_bound(w, r["weight"], r["weight"], cnt, "generated box weight")
    up_nodal, _, up_w = c.s.nodalRecovery(ed, r["u"])
    _within_bound(up_nodal, nodal, B, cnt, "uploaded box nodal")
    _within_bound(up_w, w, w, cnt, "uploaded box weight")
    up = c.s.errorIndicator(ed, r["u"])
    assert np.all(np.abs(up[0] - eta2) <= 1e-10 * eta2.max()) and abs(up[1] - tot) <= 1e-10 * tot


def test_internal_renumbering_does_not_show(case_tet10, golden_dir, monkeypatch):
    """tet10 under a random node permutation with the library's internal renumbering forced: the nodal results come back in the
    caller's numbering -- unscrambled, the unpermuted mesh's within the recovery's bound --, eta2 by element as before."""
    c = case_tet10
    nodal_ref, w_ref, B, cnt, _, _ = _reference(c, c.u, "flux", c.name)
    perm = np.random.default_rng(7).permutation(c.mesh.nNode).astype(np.int32)         # old id -> new id, as _shuffled draws it
    monkeypatch.setenv("PFEM_REORDER", "1")
    p = Case(c.kind, c.ed, _shuffled(c.mesh, seed=7))
    assert np.array_equal(p.conn, perm[c.conn])
    u = np.empty_like(c.u)
    u[perm] = c.u
    for mode in ("gather", "scatter"):
        p.s.setAssemblyMode(mode)
        nodal, sc, w = p.s.nodalRecovery(c.ed, u)
        _within_bound(nodal[perm], nodal_ref, B, cnt, f"shuffled/{mode} nodal")
        _within_bound(w[perm], w_ref, w_ref, cnt, f"shuffled/{mode} weight")
        assert np.all(np.abs(sc - H.PostScalar(c.kind, nodal)) <= 4 * EPS * sc)
        _check_indicator(p, u, f"shuffled/{mode}")
    p.s.setAssemblyMode("gather")
    eta2 = p.s.errorIndicator(c.ed, u)[0]
    ref = c.s.errorIndicator(c.ed, c.u)
    assert np.all(np.abs(eta2 - ref[0]) <= 1e-10 * ref[0].max())


@pytest.fixture
def case_tet10(golden_dir):
    from test_gpu_post import _CASES
    if "tet10" not in _CASES:
        _CASES["tet10"] = Case(*_mesh("tet10", golden_dir))
        _CASES["tet10"].name = "tet10"
    return _CASES["tet10"]


@pytest.mark.parametrize("name", ["beam", "tet10"])
def test_after_a_solve(name, golden_dir):
    """u = None: the field of the last solve -- the same bits as the call with the nodal field the solution assembles to."""
    kind, ed, mesh = _mesh(name, golden_dir)
    if name == "tet10":
        ed = H.POISSON_ELEMDATA
    c = Case(kind, ed, mesh)
    s, nda = c.s, c.dm.NodeDofArrayNew
    s.assemble(ed, H.TIMEDATA)
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-10, maxits=20000)
    assert s.factoriseAndSolve()[1] > 0
    x = s.getSolution()
    free = nda >= 0
    full = c.dm.solnApplied.reshape(-1, c.ndof).copy()
    full[free] = x[nda[free]]
    assert s.assemblyInfo()["hub_nodes"] == 0
    for a, b in zip(s.nodalRecovery(ed) + s.nodalRecovery(ed, field="grad"), s.nodalRecovery(ed, full) + s.nodalRecovery(ed, full, "grad")):
        assert (a is None and b is None) or np.array_equal(a, b)
    a, b = s.errorIndicator(ed), s.errorIndicator(ed, full)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[1] > 0
    t = s.recoveryTimings()
    assert t["recovery_ms"] > 0 and t["indicator_ms"] > 0


def test_driver_writes_the_fields(tmp_path):
    """tetrapoissonparallelimpl1(8^3 box).write_outputs(fields=True): the file parses, its nodal flux is nodalRecovery's by OLD
    node id, the cell arrays are the element fields, and the plain file beside it is the one written without fields."""
    mesh = H.gen_box_tets(-1, 1, 8, -1, 1, 8, -1, 1, 8)
    res = pf.tetrapoissonparallelimpl1(mesh, rtol=1e-10)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    plain = res.write_outputs(a)
    with_fields = res.write_outputs(b, fields=True)
    assert open(plain, "rb").read() == open(with_fields, "rb").read()
    assert sorted(p.name for p in a.iterdir()) == ["Poisson-soln.vtk", "temp.dat"]
    assert sorted(p.name for p in b.iterdir()) == ["Poisson-soln-fields.vtk", "Poisson-soln.vtk", "temp.dat"]
    text = (b / "Poisson-soln-fields.vtk").read_text()
    ed, old = H.POISSON_ELEMDATA, res.dm.node_map_get_old
    nodal, sc, _ = res.solver.nodalRecovery(ed)
    _, flux, mag = res.solver.elementFields(ed)
    eta = np.sqrt(res.solver.errorIndicator(ed)[0])
    close = lambda got, want: np.all(np.abs(got - want) <= 5e-9 * np.abs(want))      # noqa: E731
    key, got = parse_vtk_array(text, "POINT_DATA", "flux_recovered", mesh.nNode)
    assert key == "VECTORS" and close(got[old], nodal)
    key, got = parse_vtk_array(text, "POINT_DATA", "flux_magnitude_recovered", mesh.nNode)
    assert key == "SCALARS" and close(got[old, 0], sc)
    for name, want, kw in (("flux", flux.T, "VECTORS"), ("flux_magnitude", mag[:, None], "SCALARS"), ("eta", eta[:, None], "SCALARS")):
        key, got = parse_vtk_array(text, "CELL_DATA", name, mesh.nElem)
        assert key == kw and close(got, want), name
    # the compat path has no mesh on the device: the library's PFEM_ERR_STATE
    compat = pf.tetrapoissonparallelimpl1(H.gen_box_tets(-1, 1, 2, -1, 1, 2, -1, 1, 2), rtol=1e-10, mode="compat")
    with pytest.raises(pf.PfemError) as ei:
        compat.write_outputs(b, fields=True)
    assert ei.value.code == L.ERR_STATE


def test_states(golden_dir):
    kind, ed, mesh = _mesh("tet10", golden_dir)
    c = Case(kind, ed, mesh)
    for call in (lambda: c.s.nodalRecovery(ed), lambda: c.s.errorIndicator(ed)):
        with pytest.raises(pf.PfemError) as ei:
            call()                                                        # u = None before any solve
        assert ei.value.code == L.ERR_STATE
    # the MatSetValues path has no mesh on the device
    compat = pf.tetrapoissonparallelimpl1(mesh, rtol=1e-10, mode="compat").solver
    for call in (lambda: compat.nodalRecovery(ed), lambda: compat.errorIndicator(ed)):
        with pytest.raises(pf.PfemError) as ei:
            call()
        assert ei.value.code == L.ERR_STATE and "no mesh" in str(ei.value)
    # a mesh without its pattern
    dm, conn, xyz, edof = D._setup(kind, mesh)
    s = pf.PetscSolver().initialise(dm.size_global, dm.size_global)
    s.uploadMesh(kind, conn, xyz, edof, dm.solnApplied)
    with pytest.raises(pf.PfemError) as ei:
        s.nodalRecovery(ed, c.u)
    assert ei.value.code == L.ERR_STATE and "pattern" in str(ei.value)
    # an inverted element
    bad = H.Mesh(mesh.xyz, mesh.conn.copy(), mesh.bc_node, mesh.bc_dof, mesh.bc_val)
    bad.conn[[0, 1], 5] = bad.conn[[1, 0], 5]
    b = Case(kind, ed, bad)
    for mode in ("gather", "scatter"):
        b.s.setAssemblyMode(mode)
        for call in (lambda: b.s.nodalRecovery(ed, b.u), lambda: b.s.errorIndicator(ed, b.u)):
            with pytest.raises(pf.PfemError) as ei:
                call()
            assert ei.value.code == L.ERR_NEG_JAC

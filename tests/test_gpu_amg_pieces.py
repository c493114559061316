"""The pieces of -pc_type gamg, each against an independent reference (tests/amg_reference.py, itself checked on the CPU by
test_amg_reference.py): every coarse operator against P^T A P formed by scipy, every eigenvalue bound against the Gershgorin
bound of the level the device holds, and ONE application z = M^-1 r against the oracle's cycle evaluated in extended precision on
the device's own levels -- so that a wrong entry, bound or cycle step is named by the test that fails, instead of costing an
iteration in a solve-level comparison.  Every other gamg test compares two device variants bit for bit or a whole PCG solve.

Every case asserts the hierarchy it means to run (no passing by taking another path), is solved once per module (the pattern's
FIRST solve: operators formed in the symbolic phase, stand-alone bounds) and stepped once (assemble, solve: the WARM step runs
the numeric set-up, where the bounds come from the products and level 0's product reads value codes where that applies); both
states are exported and every test looks at both.

Rigid-body levels: the oracle's own prolongator (oracle.rbm_prolongator) from the node aggregates and the level's node
coordinates as the device reports them (all levels report them), which agree with the oracle's chained centroids to 1e-12.

The last level above the dense limit (eight Chebyshev sweeps at the bottom) is not reached by any case: amg_build_levels stops
at the first level of at most 128 rows, after 14 levels, or when a level would keep more than 8/10 of its rows; on a connected
mesh matching and pairing shrink a level by 4 to 8, so the coarsening never stalls above 128 rows, and 14 levels are out of reach
of a small mesh.  cycle_ld's Chebyshev bottom is exercised on the CPU (test_amg_reference.py) only.

The tolerance of one application is not a constant: 32 x e64(case), at least 64 eps, where e64 is the distance of the ORACLE's fp64
cycle from the extended evaluation over this case's own vectors (amg_reference.e64).  Measured figures: profiles/gamg_pieces/.
"""
import contextlib
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as R
import pfemfort_amd as pf
from oracle import pfem_oracle as O
from pfemfort_amd import host as H
from test_gpu_amg_tail import _cube, _no_lattice
from test_gpu_parity import _device_problem, _moved

pytestmark = pytest.mark.gpu

EPS = R.EPS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWITCHES = ("PFEM_AMG_LATTICE_BY_NUMBERING", "PFEM_CG_GRAPH", "PFEM_AMG_FUSED", "PFEM_AMG_COL_CODES", "PFEM_SPMV_VALDICT", "PFEM_AMG_CYCLE")


def _beam():
    return H.gen_box_tets(-0.5, 0.5, 6, 0.0, 6.0, 36, -0.5, 0.5, 6, bc_mode=1, ndof=3)


# case -> kind, mesh, element data, grouped SpMV form, W-cycle, environment; `expect`: the hierarchy the case is there for
CASES = {
    "cube28": dict(kind=pf.POISSON_TET, mesh=lambda: _cube((28, 28, 28)), ed=H.POISSON_ELEMDATA, grouped=True,
                   expect=dict(rows=[19683, 2744, 343, 64], tail=(2, "lds+matrix"), kinds={"bricks"})),
    "ragged": dict(kind=pf.POISSON_TET, mesh=lambda: _cube((40, 38, 36)), ed=H.POISSON_ELEMDATA, grouped=True,
                   expect=dict(rows=[50505, 6840, 900, 125], tail=(2, "lds"), kinds={"bricks"})),
    "aniso": dict(kind=pf.POISSON_TET, mesh=lambda: _cube((20, 20, 20)), ed=np.array([1.0, 1.0, 100.0]),
                  expect=dict(has_kind="lattice-passes")),
    "matched": dict(kind=pf.POISSON_TET, mesh=lambda: _no_lattice((14, 13, 13)), ed=H.POISSON_ELEMDATA,
                    expect=dict(rows=[1872, 275, 42], tail=(1, "lds+matrix"), kinds={"matching"})),
    "matched20": dict(kind=pf.POISSON_TET, mesh=lambda: _no_lattice((20, 20, 20)), ed=H.POISSON_ELEMDATA,
                      expect=dict(rows=[6859, 1013, 152, 25], tail=(1, "lds"), kinds={"matching"})),
    "beam": dict(kind=pf.ELAST_TET, mesh=_beam, ed=H.ELAST_ELEMDATA, grouped=True,
                 expect=dict(rows=[5292, 216, 24], tail=(1, "lds"), rbm=True, kinds={"node-bricks"})),
    "beam_moved": dict(kind=pf.ELAST_TET, mesh=lambda: _moved(_beam(), 1.0 / 6), ed=H.ELAST_ELEMDATA, grouped=True,
                       env={"PFEM_AMG_LATTICE_BY_NUMBERING": "0"}, expect=dict(rbm=True, kinds={"lattice-passes", "matching"})),
    "cook": dict(kind=pf.ELAST_TRIA, mesh=lambda: H.read_mesh(f"{GOLDEN}/input/cookmembranetria32"), ed=H.ELAST2D_ELEMDATA, forces=True,
                 expect=dict(rbm=True, coarse_bs=3)),
    "coded": dict(kind=pf.POISSON_TET, mesh=lambda: _cube((84, 82, 80)), ed=H.POISSON_ELEMDATA,
                  expect=dict(rows2=[83 * 81 * 79, 42 * 41 * 40], column_codes=[1])),
    "cube28_w": dict(kind=pf.POISSON_TET, mesh=lambda: _cube((28, 28, 28)), ed=H.POISSON_ELEMDATA, grouped=True, w=True,
                     expect=dict(rows=[19683, 2744, 343, 64], tail=(2, "lds+matrix"), w_to=2)),
    "matched_w": dict(kind=pf.POISSON_TET, mesh=lambda: _no_lattice((14, 13, 13)), ed=H.POISSON_ELEMDATA, w=True,
                      expect=dict(rows=[1872, 275, 42], tail=(1, "lds+matrix"))),
}
ALL = sorted(CASES)
OPERATOR_CASES = ALL


@contextlib.contextmanager
def _env(**kw):
    """The switches that choose a path, as given, every other one unset; restored afterwards."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(kw)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _new_solver(case):
    c = CASES[case]
    mesh = c["mesh"]()
    s, dm = _device_problem(c["kind"], mesh, c["ed"])
    if c.get("grouped"):
        s.setSpmvFormat("grouped")
        s.buildPattern()
        s.assemble(c["ed"], H.TIMEDATA)
    load = None
    if c.get("forces") and mesh.force_node is not None:
        load = (dm.NodeDofArrayNew[dm.node_map_get_new[mesh.force_node], mesh.force_dof], mesh.force_val)
        s.addNodalForces(*load)
    if c.get("w"):
        s.setAmgCycle("w")
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-10, maxits=5000)
    return s, load


def _assemble(s, case, load):
    s.assemble(CASES[case]["ed"], H.TIMEDATA)
    if load is not None:
        s.addNodalForces(*load)


def _solve(s):
    its, reason, _ = s.factoriseAndSolve()
    assert reason == 2
    return its, s.getHistory(), s.getSolution()


def _csr(t):
    rowptr, cols, vals = t
    return sp.csr_matrix((vals, cols, rowptr), shape=(len(rowptr) - 1, len(rowptr) - 1))


def _transfers(s, info):
    """Per transfer: the aggregates, or (rigid-body levels) the oracle's prolongator from the device's node aggregates and the
    device's reported node coordinates of that level -- with (P, node aggregates, coordinates) kept for the tolerance."""
    out, rbm, cen = [], [], None
    for l in range(info["levels"] - 1):
        a = s.amgAggregates(l, info["rows"][l])
        tr = s.amgTransfer(l)
        if not tr["rbm"]:
            out.append(a)
            rbm.append(None)
            cen = None
            continue
        fb, cb, dim = tr["fine_bs"], tr["coarse_bs"], tr["dim"]
        assert cb == dim + (3 if dim == 3 else 1) and fb in (dim, cb) and info["rows"][l] == fb * tr["n_nodes"]
        a2 = a.reshape(-1, fb)
        assert not (a2[:, 0] % cb).any() and all(np.array_equal(a2[:, c], a2[:, 0] + c) for c in range(fb))     # translation part of P
        dev_xyz = s.amgTransfer(l, xyz=True)["xyz"]          # (every level of a rigid-body hierarchy reports its nodes)
        if cen is not None:          # the oracle's chained centroids agree with what the device reports
            assert np.abs(cen - dev_xyz).max() <= 1e-12 * max(1.0, np.abs(dev_xyz).max())
        node_agg = a2[:, 0] // cb
        P, cen = O.rbm_prolongator(node_agg, dev_xyz, dim, fb)
        out.append(P)
        rbm.append(dict(node_agg=node_agg, xyz=dev_xyz, dim=dim, fb=fb, cb=cb))
    return out, rbm


def _export(s, info):
    """What one state of the solver holds: the matrix, every coarse level, the bounds."""
    return dict(A0=_csr(s.getCSR()), levels=[_csr(s.amgLevelCSR(l)) for l in range(1, info["levels"])], lam=list(info["lambda_max"]),
                by_products=s.amgBoundsByProducts(), from_codes=info["galerkin_from_codes"])


def _same_levels(a, b):
    return all(np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices) and np.array_equal(x.data, y.data)
               for x, y in zip([a["A0"]] + a["levels"], [b["A0"]] + b["levels"])) and a["lam"] == b["lam"]


def _check_hierarchy(case, s, info, cyc):
    e = CASES[case]["expect"]
    kinds = s.amgAggregation()
    rbm = [s.amgTransfer(l)["rbm"] for l in range(info["levels"] - 1)]
    print(case, "rows", info["rows"], "kinds", kinds, "cycle", cyc, "rbm", rbm)
    assert info["levels"] >= 3 and info["rows"][-1] <= 128
    if "rows" in e:
        assert info["rows"] == e["rows"]
    if "rows2" in e:
        assert info["rows"][:2] == e["rows2"]
    if "tail" in e:
        assert (cyc["tail_from"], cyc["tail_build"]) == e["tail"]
    if "kinds" in e:
        assert set(kinds) <= e["kinds"], kinds
    if "has_kind" in e:
        assert e["has_kind"] in kinds and s.amgLayout()["lattice_levels"] >= 2
    assert all(rbm) if e.get("rbm") else not any(rbm)
    if "coarse_bs" in e:
        assert s.amgTransfer(0)["coarse_bs"] == e["coarse_bs"] and s.amgTransfer(0)["dim"] == 2
    if "column_codes" in e:
        assert cyc["column_codes"] == e["column_codes"]
    assert cyc["cycle"] == ("w" if CASES[case].get("w") else "v")
    if CASES[case].get("w"):
        assert 1 <= cyc["last_level_visited_twice"] <= info["levels"] - 2
    if "w_to" in e:
        assert cyc["last_level_visited_twice"] == e["w_to"]


def _vectors(n, rhs, agg0):
    """The right-hand side, a seeded standard normal, all ones, unit vectors at the first dof, the last dof and a dof of the
    smallest aggregate (the thinnest brick) of level 0.  (test_amg_reference.py's sensitivity test needed no further vector.)"""
    cnt = np.bincount(agg0)
    small = int(np.nonzero(agg0 == int(np.argmin(cnt)))[0][-1])
    v = {"rhs": np.asarray(rhs, dtype=np.float64), "normal": np.random.default_rng(11).standard_normal(n), "ones": np.ones(n)}
    for name, i in (("unit_first", 0), ("unit_last", n - 1), ("unit_smallest_aggregate", small)):
        e = np.zeros(n)
        e[i] = 1.0
        v[name] = e
    return v


def _pairs(n):
    rng = np.random.default_rng(23)
    return [(rng.standard_normal(n), rng.standard_normal(n)) for _ in range(2)]


@functools.lru_cache(maxsize=None)
def _state(case):
    """One solver per case: the first solve and a warm step, and after each the exported levels and the device's z for every
    test vector and symmetry pair."""
    with _env(**CASES[case].get("env", {})):
        s, load = _new_solver(case)
        try:
            out = {"case": case}
            for step in ("first", "warm"):
                if step == "warm":
                    _assemble(s, case, load)
                _solve(s)
                info, cyc = s.amgInfo(), s.amgCycle()
                if step == "first":
                    _check_hierarchy(case, s, info, cyc)
                    out["info"], out["cyc"] = info, cyc
                    out["transfers"], out["rbm"] = _transfers(s, info)
                    out["kinds"] = s.amgAggregation()
                    agg0 = s.amgAggregates(0, info["rows"][0])
                    if out["rbm"][0]:
                        agg0 = agg0 // out["rbm"][0]["cb"]
                    out["vectors"] = _vectors(info["rows"][0], s.getRHS(), agg0)
                    out["pairs"] = _pairs(info["rows"][0])
                    assert s.amgBoundsByProducts() == 0
                else:
                    assert info["rows"] == out["info"]["rows"] and s.amgCycle()["cycle"] == out["cyc"]["cycle"]
                    for key in ("cheb_degree", "fine_degree", "eig_ratio", "coarse_scale"):
                        assert info[key] == out["info"][key]
                st = _export(s, info)
                st["z"] = {name: s.amgApply(v) for name, v in out["vectors"].items()}
                st["z_pairs"] = [(s.amgApply(u), s.amgApply(v)) for u, v in out["pairs"]]
                out[step] = st
                print(case, step, "bounds by products", st["by_products"], "level 1 from codes", st["from_codes"])
        finally:
            s.free()
    i, c = out["info"], out["cyc"]
    out["knobs"] = dict(cheb_degree=i["cheb_degree"], fine_degree=i["fine_degree"], eig_ratio=i["eig_ratio"], coarse_scale=i["coarse_scale"],
                        gamma=2 if c["cycle"] == "w" else 1, gamma_to=c["last_level_visited_twice"] if c["cycle"] == "w" else 99)
    return out


@functools.lru_cache(maxsize=None)
def _tolerance(case):
    """(e64, tol) of the case from the oracle alone: its fp64 cycle against the extended one, over the case's own vectors."""
    st = _state(case)
    vec = list(st["vectors"].values()) + [w for p in st["pairs"] for w in p]
    e = R.e64((st["first"]["A0"], st["transfers"], st["knobs"]), vec)
    return e, R.apply_tolerance(e)


@functools.lru_cache(maxsize=None)
def _reference_cycle(case, step):
    """cycle_ld on the DEVICE's exported levels and bounds of that state (the warm step's are the first solve's, bit for bit, on
    every case whose values did not change: one reference serves both)."""
    st = _state(case)
    if step == "warm" and _same_levels(st["warm"], st["first"]):
        return _reference_cycle(case, "first")
    x = st[step]
    M = R.cycle_ld(x["A0"], x["levels"], st["transfers"], x["lam"], st["knobs"])
    return {"z": {name: M(v) for name, v in st["vectors"].items()}, "z_pairs": [(M(u), M(v)) for u, v in st["pairs"]]}


# ---- test 1: the coarse operators ---------------------------------------------------------------------------------------------
def _on(M, keys, ncols):
    """(values, stored?) of M at the sorted positions ``keys`` (row * ncols + col); every stored entry of M must be one of them."""
    M = M.tocoo()
    k = M.row.astype(np.int64) * ncols + M.col
    pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
    assert (keys[pos] == k).all(), "an entry outside the product's pattern"
    vals, stored = np.zeros(len(keys)), np.zeros(len(keys), bool)
    vals[pos] = M.data
    stored[pos] = True
    return vals, stored


def _rbm_rounding(A, P, r):
    """|P^T| |A| E + E^T |A| |P|: the rounding of the centroids -- the device and numpy each average up to m coordinates -- sits in
    the offset-dependent entries of P (translation rows, rotation columns): E holds 2 (m + 1) eps max|xyz| there."""
    m = int(np.bincount(r["node_agg"]).max())
    Pc = P.tocoo()
    on = (Pc.row % r["fb"] < r["dim"]) & (Pc.col % r["cb"] >= r["dim"])
    E = sp.csr_matrix((np.full(int(on.sum()), 2.0 * (m + 1) * EPS * float(np.abs(r["xyz"]).max())), (Pc.row[on], Pc.col[on])), shape=P.shape)
    X = (abs(P).T @ abs(A) @ E).tocsr()
    return (X + X.T).tocsr()


@pytest.mark.parametrize("case", OPERATOR_CASES)
def test_coarse_operators_equal_the_galerkin_products(case):
    """Every level l >= 1 against P^T A P of the level above AS THE DEVICE HOLDS IT (level 1: the assembled matrix), entry by
    entry within a derived tolerance T.  Scalar levels: T = 2 (K + 2) eps |P^T| |A| |P| -- both sides sum K terms in fp64, in
    different orders.  Rigid-body levels: T = 2 (K + 16) eps |P^T| |A| |P| + _rbm_rounding -- sixteen more steps for the small-block
    arithmetic of P_i^T F_ij P_j.
    Patterns.  scipy's product keeps no sum that is exactly zero, the DEVICE stores such entries, so "the reference's pattern" is
    taken in two parts.  Structure: no stored entry lies outside the product of the 0/1 patterns, every entry of the reference
    is stored, and scalar levels whose aggregates come from pairing passes or matching store that product exactly (their slot
    lists ARE it).  Values: on scalar levels of bricks and of matched aggregates the nonzero entries are the reference's, exactly
    (the issue's "after dropping explicit zeros").  Where sums cancel -- rigid-body levels, the anisotropic problem's paired
    levels -- a sum comes out as an exact zero in one order of summation and as a residue of a few ulps in another (measured: the
    beam's level 1 stores 39 zeros, one of them at an entry the reference holds; Cook's membrane stores one residue where scipy
    dropped an exact zero; the anisotropic cube's level 2 likewise), so "the same entries after dropping zeros" is no property
    of the operator there; asserted instead: where the reference has no entry the device's is zero to within T, and T is 0
    wherever |P^T| |A| |P| is."""
    st = _state(case)
    for step in ("first", "warm"):
        x = st[step]
        fine = x["A0"]
        for l, (dev, t, r, kind) in enumerate(zip(x["levels"], st["transfers"], st["rbm"], st["kinds"]), start=1):
            ref, Aabs, K = R.galerkin_reference(fine, t)
            assert dev.shape == ref.shape and dev.has_sorted_indices
            Kc = K.tocoo()
            ncols = K.shape[1]
            keys = Kc.row.astype(np.int64) * ncols + Kc.col
            order = np.argsort(keys)
            keys, terms = keys[order], Kc.data[order]
            dv, dstored = _on(dev, keys, ncols)
            rv, rstored = _on(ref, keys, ncols)
            T = 2.0 * (terms + (16.0 if r else 2.0)) * EPS * _on(Aabs, keys, ncols)[0]
            if r:
                T = T + _on(_rbm_rounding(fine, t, r), keys, ncols)[0]
            err = np.abs(dv - rv)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err > 0, err / T, 0.0)
            print(f"{case} {step} level {l} ({kind}): rows {dev.shape[0]} stored {int(dstored.sum())} of them zeros {int((dstored & (dv == 0)).sum())}"
                  f" reference entries {int(rstored.sum())} product of the patterns {len(keys)} max |dev - ref| {err.max():.3e} largest |dev - ref| / T {ratio.max():.3f}")
            assert not (rstored & ~dstored).any(), (step, l, "a reference entry the device does not store")
            if not r and kind != "bricks":
                assert dstored.all(), (step, l, "the device does not store the product of the 0/1 patterns")
            if not r and kind in ("bricks", "matching"):
                assert np.array_equal(dv != 0, rv != 0), (step, l, "patterns differ after dropping zeros")
            assert (err <= T).all(), (step, l, int((err > T).sum()), float(ratio.max()))          # (where the reference has nothing: |dev| <= T)
            fine = dev


# ---- test 2: the bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OPERATOR_CASES)
def test_bounds_equal_the_gershgorin_bounds_of_the_devices_levels(case):
    """lambda of every level against max_i sum_j |a_ij| / a_ii of the level the device itself holds (with rigid-body modes: the
    smaller of it and the bound on D^-1/2 A D^-1/2, as oracle.amg_cycle takes it), within 2 (longest row + 4) eps: a row's sum in
    another order, the division, and -- second bound -- two roots and two products.  After the first solve (stand-alone maxima)
    and after the warm step (bounds left by the products)."""
    st = _state(case)
    rbm = any(r is not None for r in st["rbm"])
    for step in ("first", "warm"):
        x = st[step]
        for l, (M, lam_dev) in enumerate(zip([x["A0"]] + x["levels"], x["lam"])):
            lam_ref = R.gershgorin(M, rbm)
            longest = int(np.diff(M.indptr).max())
            tol = 2.0 * (longest + 4) * EPS * lam_ref
            print(f"{case} {step} level {l}: lambda {lam_dev!r} reference {lam_ref!r} difference {abs(lam_dev - lam_ref):.3e} tolerance {tol:.3e}")
            assert abs(lam_dev - lam_ref) <= tol, (step, l, lam_dev, lam_ref)
    if case in ("cube28", "ragged", "cube28_w"):          # (the warm step took bounds from the products: what the second pass above looked at)
        assert st["warm"]["by_products"] >= 1


# ---- test 3: the inverse diagonal has no getter; test 4 reads it through every smoothing step ------------------------------------

# ---- test 4: one application ----------------------------------------------------------------------------------------------------
_ERRORS = {}


def _dump_errors():
    path = os.environ.get("PFEM_GAMG_PIECES_ERRORS")          # (the lab's record: profiles/gamg_pieces/errors.json is a run of this)
    if path:
        with open(path, "w") as f:
            json.dump(_ERRORS, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("case", ALL)
def test_one_application_equals_the_extended_cycle(case):
    """z = amgApply(v) against cycle_ld(v) built from the device's exported levels, its bounds and knobs, and the transfers:
    |z_dev - z_ref|_inf <= tol |z_ref|_inf with tol = 32 x e64(case), at least 64 eps -- both are fp64 roundings of one operator, so
    2 is the least factor; 32 leaves room for other summation orders.  Tests 1 and 2 localise a wrong level or bound; this one
    checks the cycle alone: the smoother's coefficients and inverse diagonal, the restriction, the second visit, the dense bottom."""
    st = _state(case)
    e, tol = _tolerance(case)
    rec = _ERRORS.setdefault(case, {"e64": e, "tol": tol, "rows": st["info"]["rows"], "first": {}, "warm": {}})
    bad = []
    for step in ("first", "warm"):
        ref = _reference_cycle(case, step)
        for name, z in st[step]["z"].items():
            zr = ref["z"][name]
            err = R._rel_inf(z.astype(np.longdouble), zr)
            rec[step][name] = err
            print(f"{case} {step} {name}: e64 {e:.3e} tol {tol:.3e} device {err:.3e}")
            if not err <= tol:
                bad.append((step, name, err))
    _dump_errors()
    assert not bad, (bad, tol)


# ---- test 5: the probe is invisible, and the operator is what CG needs --------------------------------------------------------
def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("case", ["cube28", "beam"])
def test_the_probe_is_invisible(case, graph):
    """solve, amgApply, solve gives the iteration count, history and solution of solve, solve, bit for bit, with the cycle replayed
    from a graph and launched plainly; amgApply twice gives the same bits."""
    v = _state(case)["vectors"]["normal"]
    with _env(PFEM_CG_GRAPH=graph, **CASES[case].get("env", {})):
        runs = {}
        for probe in (False, True):
            s, _ = _new_solver(case)
            try:
                first = _solve(s)
                if probe:
                    z1, z2 = s.amgApply(v), s.amgApply(v)
                    assert np.array_equal(z1, z2) and np.isfinite(z1).all()
                    assert np.array_equal(z1, _state(case)["first"]["z"]["normal"])          # ... and the bits of the shared solver's
                    cyc = s.amgCycle()
                second = _solve(s)
                if probe:
                    assert s.amgCycle() == cyc
                    assert np.array_equal(s.amgApply(v), z1)
                runs[probe] = (first, second, s.amgInfo()["lambda_max"], s.timings()["graph_iterations"] > 0)
            finally:
                s.free()
    for k in (0, 1):
        assert _same(runs[False][k], runs[True][k]), (case, graph, k)
    assert runs[False][2] == runs[True][2] and runs[False][3] == runs[True][3]


@pytest.mark.parametrize("case", ALL)
def test_the_operator_is_symmetric_and_positive(case):
    """|(u, M^-1 v) - (v, M^-1 u)| <= 2 tol |u| |M^-1 v| for two seeded pairs, and (v, M^-1 v) > 0 for every test vector: what CG asks
    of a preconditioner, which no comparison of solutions can see."""
    st = _state(case)
    _, tol = _tolerance(case)
    for step in ("first", "warm"):
        for (u, v), (zu, zv) in zip(st["pairs"], st[step]["z_pairs"]):
            a, b = float(u @ zv), float(v @ zu)
            bound = 2.0 * tol * float(np.linalg.norm(u) * np.linalg.norm(zv))
            print(f"{case} {step}: (u, M^-1 v) {a!r} (v, M^-1 u) {b!r} difference {abs(a - b):.3e} bound {bound:.3e}")
            assert abs(a - b) <= bound
            assert float(u @ zu) > 0.0 and float(v @ zv) > 0.0
        for name, v in st["vectors"].items():
            assert float(v @ st[step]["z"][name]) > 0.0, (step, name)


def test_the_probes_refuse_a_solver_without_a_hierarchy():
    """PFEM_ERR_STATE before any gamg solve and for a level the hierarchy does not have, PFEM_ERR_ARG for level 0 (the assembled
    matrix comes from getCSR); after the solve both answer.  (A hierarchy across ranks is refused the same way; it takes several
    ranks to make one: not run here.)"""
    from pfemfort_amd import _lib as L
    s, _ = _new_solver("matched")
    try:
        n = s.matrixInfo()["n_local"]
        for call in (lambda: s.amgApply(np.ones(n)), lambda: s.amgLevelCSR(1)):
            with pytest.raises(pf.PfemError) as ei:
                call()
            assert ei.value.code == L.ERR_STATE
        s.setPreconditioner("jacobi")
        _solve(s)
        with pytest.raises(pf.PfemError) as ei:
            s.amgApply(np.ones(n))
        assert ei.value.code == L.ERR_STATE
        s.setPreconditioner("gamg")
        _solve(s)
        levels = s.amgInfo()["levels"]
        assert s.amgApply(np.ones(n)).shape == (n,) and len(s.amgLevelCSR(levels - 1)[0]) == s.amgInfo()["rows"][-1] + 1
        with pytest.raises(pf.PfemError) as ei:
            s.amgLevelCSR(levels)
        assert ei.value.code == L.ERR_STATE
        with pytest.raises(pf.PfemError) as ei:
            s.amgLevelCSR(0)
        assert ei.value.code == L.ERR_ARG
    finally:
        s.free()

"""The synthetic SpMV matrices (tests/spmv_synthetic.py) have the shapes they are meant to have, and the chain reference
(orc_spmv_chain) is what it says: checked on the CPU, so that a device test that asserts a form cannot rest on a pattern that
quietly stopped reaching it."""
from fractions import Fraction

import numpy as np
import pytest

import spmv_synthetic as S
from oracle import pfem_oracle as O


def _rows(rowptr, cols):
    return [cols[rowptr[r]:rowptr[r + 1]] for r in range(len(rowptr) - 1)]


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_hard_rules_of_every_pattern(name):
    """ascending columns inside [0, n), a stored diagonal in every row, n no multiple of 4 or 256, a size a test can afford"""
    rowptr, cols = S.pattern(name)
    n = len(rowptr) - 1
    assert n % 4 and n % 256 and n <= 140003 and rowptr[-1] == len(cols) and S.model(name)["stored"] < 600000
    assert cols.min() >= 0 and cols.max() < n
    inner = np.ones(len(cols), bool); inner[rowptr[:-1]] = False
    assert (np.diff(rowptr) >= 1).all() and (np.diff(cols.astype(np.int64))[inner[1:]] > 0).all()
    assert np.array_equal(np.bincount(np.repeat(np.arange(n), np.diff(rowptr))[S.diag_mask(rowptr, cols)], minlength=n), np.ones(n))


@pytest.mark.parametrize("name, wmax", [("stencil", 12), ("stencil24", 24)])
def test_stencil_widths_groups_and_byte_ratios(name, wmax):
    rowptr, cols = S.pattern(name)
    m = S.model(name)
    n = m["n"]
    # every width 1 .. wmax among the slices of the row form and of the relative groups: every class mod 4 and mod 8, widths 1 and 2
    assert m["widths"] == list(range(1, wmax + 1)) and m["rwidths"] == list(range(1, wmax + 1))
    # lanes of unequal length inside a slice, rows that lack an offset of their group's union, a short last group, a partly empty last slice
    rl = np.diff(rowptr)
    assert any(len(set(rl[s:s + 64].tolist())) > 1 for s in range(0, n, 64))
    assert 4 * m["union"] > m["nnz"] and n % 4 == 3 and ((n + 3) // 4) % 64 != 0
    lacking = 0
    for g in range(n // 4):
        offs = [set((c.astype(np.int64) - r).tolist()) for r, c in zip(range(4 * g, 4 * g + 4), _rows(rowptr[4 * g:4 * g + 5], cols))]
        lacking += sum(o != set.union(*offs) for o in offs)
    assert lacking >= 0.02 * n
    # the union form pays: the library keeps it up to 0.95 of the row form's bytes
    assert m["ratio16"] <= 0.90 and m["ratio32"] <= 0.90
    assert (m["row"], m["rel"], m["group3"]) == ("lit16", "lit16", False)


def test_blocks3_with_a_far_neighbour():
    m = S.model("blocks3_table")
    assert m["group3"] and m["row"] == "table" and m["rel"] is None and m["row_large"] == [67998, 67999, 68000]
    assert min(m["group_rows"]) >= 1000 and m["stored"] < 600000


def test_blocks3_groups():
    rowptr, cols, d = S.blocks3(6403, seed=2)
    assert np.array_equal(rowptr, S.pattern("blocks3")[0]) and np.array_equal(cols, S.pattern("blocks3")[1])
    m = S.model("blocks3")
    assert m["groups"] == 6403 and m["group_rows"] == np.bincount(d, minlength=4)[1:4].tolist() and min(m["group_rows"]) >= 200
    assert 11 * m["groups"] <= 4 * m["n"] and m["group3"] and m["rel"] is None and m["row"] == "lit16"
    assert {w % 8 for w in m["gwidths"]} == set(range(8))                  # every trip structure of k_spmvg
    assert 3 * m["gstored"] > m["nnz"]                                     # slots without an entry: +0.0 is in the dictionary
    assert any(w % 3 for w in np.diff(rowptr).tolist())                    # widths that are no multiple of 3
    rl = np.diff(rowptr)
    first = np.r_[0, np.cumsum(d)][:-1]
    assert any(len(set(rl[first[s:s + 64]].tolist())) > 1 for s in range(0, 6403, 64))       # zero padding inside a group-slice


LARGE = {  # name -> (distinct large gaps of the rows = of the unions, row form, relative groups)
    "gaps256": (256, "table", "table"),
    "gaps257": (257, "escape", "gap32"),
    "gap32767": (1, "table", "table"),
    "gap32768": (2, "table", "table"),
    "gap65534": (1, "lit16", "lit16"),
    "gap65535": (1, "lit16", "lit16"),
    "gap65536": (1, "table", "table"),
    "gap65534e": (2, "table", "table"),
    "gap65535e": (2, "table", "table"),
    "escapes_heavy": (257, "int32", "gap32"),
}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_large_gap_cases_are_what_their_names_say(name):
    m = S.model(name)
    count, row, rel = LARGE[name]
    assert len(m["row_large"]) == count and m["row_large"] == m["rel_large"]
    assert (m["row"], m["rel"], m["group3"]) == (row, rel, False)
    assert m["rel_bytes_ratio"] <= 0.91                                    # (the relative groups are kept: the library's limit is 0.95)
    if name[3:8].isdigit():
        g, two = int(name[3:8]), name in ("gap32767", "gap32768", "gap65534e", "gap65535e")
        assert m["row_large"] == sorted({g, 70000} if two else {g})[g == 32767:]
        rowptr, cols = S.pattern(name)
        gaps = np.diff(cols.astype(np.int64))
        assert (gaps == g).sum() >= 1000                                   # (the boundary gap is there, in many rows)
        if name.endswith("e"):          # without the table: the escape form, where only gaps from 65 535 on escape
            assert m["esc"] == (gaps >= 65535).sum() == (gaps == 70000).sum() + (g == 65535) * (gaps == g).sum()
            assert 0 < 4 * m["esc"] <= m["stored"]
    if name == "gaps257":
        assert m["esc"] > 0 and 4 * m["esc"] / m["stored"] <= 0.8
    if name == "escapes_heavy":
        assert 4 * m["esc"] / m["stored"] >= 1.2


def test_value_streams():
    rowptr, cols = S.pattern("stencil")
    n = len(rowptr) - 1
    d = S.diag_mask(rowptr, cols)
    v = S.values_int(rowptr, cols)
    x = S.x_int(n)
    assert (v != 0).all() and (np.abs(v) <= 1024).all() and (v == np.rint(v)).all() and (v[d] > 0).all()
    assert (x != 0).all() and (np.abs(x) <= 1024).all() and (x == np.rint(x)).all()
    assert 24 * 1024 * 1024 < 2 ** 53                                      # every partial sum of a row is an exact integer
    for K in (1, 2, 600, 4094, 4095, 4096, 5000):
        p = S.pool(K)
        v = S.values_pool(rowptr, cols, p)
        assert len(np.unique(p.view(np.uint64))) == K and not (p == 0.0).any() and np.isfinite(p).all()
        assert np.array_equal(np.unique(v.view(np.uint64)), np.unique(p.view(np.uint64))) and (v[d] > 0).all()      # each one occurs
        w = S.values_pool(rowptr, cols, p, shift=7)
        assert np.array_equal(np.unique(w.view(np.uint64)), np.unique(p.view(np.uint64))) and (K == 1 or not np.array_equal(v, w))
    p = S.pool(600, extra=S.HOSTILE + (S.VD_EMPTY, S.pattern_of(-0.0), S.pattern_of(5e-324)))
    v = S.values_pool(rowptr, cols, p)
    assert len(np.unique(v.view(np.uint64))) == 600 and np.isfinite(v[d]).all() and (v[d] > 0).all()
    assert {S.VD_EMPTY, S.NAN_A, S.NAN_B, S.pattern_of(-0.0), 1} <= set(v.view(np.uint64).tolist())
    v = S.values_normal(rowptr, cols)
    assert len(np.unique(v.view(np.uint64))) > S.VD_MAX and (v[d] > 0).all() and np.isfinite(v).all()
    assert np.isfinite(S.x_normal(n)).all() and (S.x_normal(n) != 0).all()
    v = S.values_dominant(rowptr, cols)
    # 2 a_ii > sum_j |a_ij| + sum_j |a_ji| >= sum_j |a_ij + a_ji|: the symmetric part is strictly diagonally dominant
    row_abs, col_abs = np.zeros(n), np.zeros(n)
    for r in range(n):
        for k in range(rowptr[r], rowptr[r + 1]):
            if cols[k] != r:
                row_abs[r] += abs(v[k]); col_abs[cols[k]] += abs(v[k])
    assert np.array_equal(v[d], row_abs + col_abs + 1.0) and (v[~d] == np.rint(v[~d])).all() and (v[~d] != 0).all()


def test_chain_reference_against_exact_rationals():
    """orc_spmv_chain on 200 rows = the same chain in fractions.Fraction rounded once per step, bit for bit: the first product
    rounded, every further product added exactly and rounded once (an fma)"""
    rowptr, cols = S.stencil(200, wfix=13, seed=11, drop=0.3)             # rows of up to 13 entries
    assert len(rowptr) == 201 and set(np.diff(rowptr).tolist()) >= {12, 13} and rowptr[-1] > 2000
    rng = np.random.default_rng(12)
    v = rng.standard_normal(len(cols)) * 2.0 ** rng.integers(-3, 4, len(cols))
    x = rng.standard_normal(200) * 2.0 ** rng.integers(-3, 4, 200)
    y = O.spmv_chain(rowptr, cols, v, x)
    want = np.empty(200)
    for r in range(200):
        k0, k1 = rowptr[r], rowptr[r + 1]
        acc = float(Fraction(float(v[k0])) * Fraction(float(x[cols[k0]])))
        for k in range(k0 + 1, k1):
            acc = float(Fraction(float(v[k])) * Fraction(float(x[cols[k]])) + Fraction(acc))
        want[r] = acc
    assert np.array_equal(y.view(np.int64), want.view(np.int64))
    # ... and it is not the plain two-rounding sum: the check above can tell them apart
    two = np.empty(200)
    for r in range(200):
        acc = 0.0
        for k in range(rowptr[r], rowptr[r + 1]):
            acc = acc + v[k] * x[cols[k]]
        two[r] = acc
    assert not np.array_equal(two, want)
    # the longdouble row sums agree with it within the bound the device tests use
    yl, al = O.spmv_longdouble(rowptr, cols, v, x)
    assert (np.abs(y - yl) <= np.diff(rowptr) * 2.0 ** -53 * al).all()

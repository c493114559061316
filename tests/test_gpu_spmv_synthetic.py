"""Every SpMV form and the value dictionary on synthetic matrices (tests/spmv_synthetic.py; their shapes are asserted on the CPU by
tests/test_spmv_synthetic_host.py).

The finite-element meshes of the other tests have one stencil length each, a handful of large gaps and a few thousand values: the
trip structure of the kernels (trips of four entries and a remainder of 0-3; W = 8, 4, 2 words and an odd tail), groups of 1 and 2
rows, lanes of unequal length, rows that lack an offset of their group, the boundaries of the three gap encodings and the
dictionary at its capacity are paths they visit by accident or not at all.  Here every case

* asserts the form FIRST, through the getters -- no case passes by falling back to another kernel;
* compares the product bit for bit: exact integers with the int64 product; rounding data with the chain the kernels themselves
  state (orc_spmv_chain: first product rounded, then one correctly rounded fma per entry in ascending column order), with the
  int32 form's product, and with a longdouble row sum under the bound len(row) 2^-53 sum |v| |x|.

Bit patterns are compared with -0.0 taken for +0.0 (spmv_synthetic.bits says why).
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import pfemfort_amd as pf
import spmv_synthetic as S
from oracle import pfem_oracle as O

pytestmark = pytest.mark.gpu

_SWITCHES = ("PFEM_SPMV_VALDICT", "PFEM_DEBUG_REL_GAP32", "PFEM_DEBUG_NO_ROW_GAP_TABLE")


@contextlib.contextmanager
def _env(**kw):
    """the library's switches as given and none of the others (the library reads them per call / per pattern build)"""
    old = {k: os.environ.get(k) for k in _SWITCHES}
    try:
        for k in _SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in kw.items() if v is not None})
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _flush(s):
    """the staged values reach the device with the next solve: zero right-hand side, no iteration"""
    s.setTolerances(maxits=0)
    its, _, _ = s.factoriseAndSolve()
    assert its == 0


def _load(name, vals, debug=None):
    rowptr, cols = S.pattern(name)
    n = len(rowptr) - 1
    with _env(**({debug: "1"} if debug else {})):          # (the debug switches are read when the pattern is built)
        s = pf.PetscSolver().initialise(n, n)
        s.loadCSR(rowptr, cols, vals)
        _flush(s)
    return s


def _push(s, name, vals):
    rowptr, cols = S.pattern(name)
    s.loadCSR(rowptr, cols, vals, values_only=True)
    _flush(s)


def _form(s):
    return (s.spmvRowGroup(), s.spmvColumnBits(), s.spmvGapTable(), s.spmvGapEscapes())


def _kernel(form, codes):
    rows, bits, table, esc = form
    t = "<table>" if table else "<literal>"
    if rows == 1:
        return "k_spmv" if bits == 32 else ("k_spmv16e" if esc else "k_spmv16" + t)
    if rows == 3:
        return ("k_spmvg_vd" if codes else "k_spmvg") + t
    if bits == 32:
        return "k_spmvr32"
    return ("k_spmvr_vd" if codes else "k_spmvr") + t


ALL_KERNELS = {"k_spmv", "k_spmv16<literal>", "k_spmv16<table>", "k_spmv16e", "k_spmvg<literal>", "k_spmvg<table>",
               "k_spmvg_vd<literal>", "k_spmvg_vd<table>", "k_spmvr<literal>", "k_spmvr<table>", "k_spmvr_vd<literal>",
               "k_spmvr_vd<table>", "k_spmvr32"}


def _has_codes(form):
    return form[0] == 3 or (form[0] == 4 and form[1] == 16)


def _same_class(y, ref):
    """finite rows bit for bit; the others NaN at the same places, +inf and -inf at the same places"""
    fin = np.isfinite(ref)
    return (np.array_equal(np.isfinite(y), fin) and np.array_equal(S.bits(y[fin]), S.bits(ref[fin]))
            and np.array_equal(np.isnan(y), np.isnan(ref)) and np.array_equal(y[np.isinf(ref)], ref[np.isinf(ref)]))


def _check_rounded(y, name, vals, x):
    """the three comparisons of a product of rounding data, but the one with the int32 form; '' or what failed"""
    rowptr, cols = S.pattern(name)
    chain = O.spmv_chain(rowptr, cols, vals, x)
    if not np.array_equal(S.bits(y), S.bits(chain)):
        bad = np.flatnonzero(S.bits(y) != S.bits(chain))
        return f"{len(bad)} rows differ from the chain, first {bad[0]} (length {rowptr[bad[0] + 1] - rowptr[bad[0]]}): {y[bad[0]]!r} != {chain[bad[0]]!r}"
    yl, al = O.spmv_longdouble(rowptr, cols, vals, x)
    if not (np.abs(y - yl) <= np.diff(rowptr) * 2.0 ** -53 * al).all():
        return "a row leaves the longdouble bound"
    return ""


# ---------------------------------------------------------------------------------------------------------------------------------
# forms and products
# ---------------------------------------------------------------------------------------------------------------------------------
# matrix -> debug switch of the pattern build -> format -> (rows per lane, column bits, entries of the gap table, escapes)
PLAN = {
    "stencil": {None: {"int32": (1, 32, 0, False), "gaps16": (1, 16, 0, False), "grouped": (4, 16, 0, False), "auto": (1, 16, 0, False)}},
    "stencil24": {None: {"int32": (1, 32, 0, False), "gaps16": (1, 16, 0, False), "grouped": (4, 16, 0, False)}},
    "blocks3": {None: {"int32": (1, 32, 0, False), "gaps16": (1, 16, 0, False), "grouped": (3, 16, 0, False)}},
    "blocks3_table": {None: {"gaps16": (1, 16, 3, False), "grouped": (3, 16, 3, False)}},
    "gaps256": {None: {"int32": (1, 32, 0, False), "gaps16": (1, 16, 256, False), "grouped": (4, 16, 256, False)},
                "PFEM_DEBUG_REL_GAP32": {"grouped": (4, 32, 0, False)}},
    "gaps257": {None: {"gaps16": (1, 16, 0, True), "grouped": (4, 32, 0, False)}},
    "gap32767": {None: {"gaps16": (1, 16, 1, False), "grouped": (4, 16, 1, False)}},
    "gap32768": {None: {"gaps16": (1, 16, 2, False), "grouped": (4, 16, 2, False)}},
    "gap65534": {None: {"gaps16": (1, 16, 0, False), "grouped": (4, 16, 0, False)}},
    "gap65535": {None: {"gaps16": (1, 16, 0, False), "grouped": (4, 16, 0, False)}},          # fits plain 16 bits
    "gap65536": {None: {"gaps16": (1, 16, 1, False), "grouped": (4, 16, 1, False)}},          # does not
    "gap65534e": {"PFEM_DEBUG_NO_ROW_GAP_TABLE": {"gaps16": (1, 16, 0, True)}},
    "gap65535e": {"PFEM_DEBUG_NO_ROW_GAP_TABLE": {"gaps16": (1, 16, 0, True)}},
    "escapes_heavy": {None: {"gaps16": (1, 32, 0, False), "grouped": (4, 32, 0, False)}},     # more than a quarter would escape
}
POOL = 600
STREAMS = ("int", "pool", "normal")          # in this order: the normal values make the library refuse the dictionary for good
CASES = [(m, d, f, vd) for m, by_debug in PLAN.items() for d, forms in by_debug.items() for f in forms for vd in ("0", "1")]


def _stream(name, stream):
    rowptr, cols = S.pattern(name)
    n = len(rowptr) - 1
    if stream == "int":
        return S.values_int(rowptr, cols), S.x_int(n)
    if stream == "pool":
        return S.values_pool(rowptr, cols, S.pool(POOL)), S.x_normal(n)
    return S.values_normal(rowptr, cols), S.x_normal(n)


@functools.lru_cache(maxsize=None)
def _observe(name, debug):
    """One handle for the matrix: per value stream one push, then every format of the plan with PFEM_SPMV_VALDICT 0 and 1.
    (format, valdict, stream) -> (form, dictionary entries, what failed in the product or '')."""
    rowptr, cols = S.pattern(name)
    out = {}
    s = None
    for stream in STREAMS:
        vals, x = _stream(name, stream)
        if s is None:
            s = _load(name, vals, debug)
        else:
            _push(s, name, vals)
        with _env(PFEM_SPMV_VALDICT="1"):
            s.setSpmvFormat("int32")
            y32 = s.spmv(x)
            int32_says = _form(s) + (s.spmvValueDictionary(),)
        if stream == "int":
            p = vals.astype(np.int64) * x.astype(np.int64)[cols]
            exact = np.add.reduceat(p, rowptr[:-1]).astype(np.float64)          # (every row stores its diagonal: no empty segment)
            ref_fail = "" if np.array_equal(y32, exact) else "the int32 form differs from the int64 product"
        else:
            ref_fail = _check_rounded(y32, name, vals, x)
        if int32_says != (1, 32, 0, False, 0):
            ref_fail = f"the int32 form reports {int32_says}; " + ref_fail
        for fmt in PLAN[name][debug]:
            for vd in ("0", "1"):
                with _env(PFEM_SPMV_VALDICT=vd):
                    s.setSpmvFormat(fmt)
                    y = s.spmv(x)
                    form, entries = _form(s), s.spmvValueDictionary()
                fail = ref_fail
                if stream == "int" and not np.array_equal(y, exact):
                    fail += "differs from the int64 product; "
                if stream != "int" and not fail:
                    fail = _check_rounded(y, name, vals, x)
                if not np.array_equal(S.bits(y), S.bits(y32)):
                    fail += "differs from the int32 form; "
                out[fmt, vd, stream] = (form, entries, fail)
    s.free()
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(p) for p in c if p))
def test_form_in_effect_and_product(case):
    name, debug, fmt, vd = case
    want = PLAN[name][debug][fmt]
    rowptr, cols = S.pattern(name)
    for stream in STREAMS:
        form, entries, fail = _observe(name, debug)[fmt, vd, stream]
        vals, _ = _stream(name, stream)
        distinct = len(np.unique(vals.view(np.uint64))) + 1          # + the zero of the padding and of the offsets a row lacks
        codes = vd == "1" and _has_codes(want) and distinct <= S.VD_MAX
        print(f"{name} {debug or ''} {fmt} valdict={vd} {stream}: {_kernel(form, entries > 0)} {form} dictionary {entries}: {fail or 'same bits'}")
        assert form == want, stream                                    # the form first: nothing passes by falling back
        assert entries == (distinct if codes else 0), stream           # codes exactly where the form has them and the values fit
        assert not fail, stream


def test_every_spmv_kernel_was_asserted_in_effect():
    """the thirteen kernels, each at least once -- those with codes with either value stream, which are two kernels each"""
    seen = set()
    for name, debug, fmt, vd in CASES:
        for stream in STREAMS:
            form, entries, fail = _observe(name, debug)[fmt, vd, stream]
            if form == PLAN[name][debug][fmt] and not fail:
                seen.add(_kernel(form, entries > 0))
    print(sorted(seen))
    assert seen == ALL_KERNELS


# ---------------------------------------------------------------------------------------------------------------------------------
# the value dictionary at its limits
# ---------------------------------------------------------------------------------------------------------------------------------
def _grouped_product(s, name, vals, seed=0):
    """(dictionary entries, '' or what failed) of one product in the group form with codes switched on"""
    rowptr, cols = S.pattern(name)
    x = S.x_normal(len(rowptr) - 1, seed)
    with _env(PFEM_SPMV_VALDICT="1"):
        s.setSpmvFormat("grouped")
        y = s.spmv(x)
        form, entries = _form(s), s.spmvValueDictionary()
    assert form == PLAN[name][None]["grouped"]
    ref = O.spmv_chain(rowptr, cols, vals, x)
    if np.isfinite(ref).all():
        return entries, y, _check_rounded(y, name, vals, x)
    return entries, y, "" if _same_class(y, ref) else "differs from the chain in a finite row or in the class of another"


@pytest.mark.parametrize("name", ["stencil", "blocks3"])
@pytest.mark.parametrize("K", [1, 2, 600, 4094, 4095, 4096, 5000])
def test_dictionary_capacity(name, K):
    """K nonzero values and the +0.0 of the explicit zeros: 4096 entries are accepted, 4097 are refused"""
    rowptr, cols = S.pattern(name)
    vals = S.values_pool(rowptr, cols, S.pool(K))
    assert len(np.unique(vals.view(np.uint64))) == K
    s = _load(name, vals)
    entries, _, fail = _grouped_product(s, name, vals)
    s.free()
    print(f"{name} K={K}: dictionary {entries}")
    assert entries == (K + 1 if K + 1 <= S.VD_MAX else 0) and not fail


@pytest.mark.parametrize("name", ["stencil", "blocks3"])
def test_dictionary_keeps_both_zeros_and_the_smallest_denormal(name):
    rowptr, cols = S.pattern(name)
    vals = S.values_pool(rowptr, cols, S.pool(POOL, extra=(S.pattern_of(-0.0), S.pattern_of(5e-324))))
    assert len(np.unique(vals.view(np.uint64))) == POOL and (vals.view(np.uint64) == S.pattern_of(-0.0)).any() and (vals == 5e-324).any()
    s = _load(name, vals)
    entries, _, fail = _grouped_product(s, name, vals)
    s.free()
    assert entries == POOL + 1 and not fail          # -0.0 and 5e-324 among the 600, +0.0 the one more


@pytest.mark.parametrize("name", ["stencil", "blocks3"])
def test_dictionary_life_cycle(name):
    """one handle, new values on the standing pattern: the steady state encodes against the standing dictionary, a new value
    misses and is collected, too many values are refused -- and stay refused until the pattern changes, as documented"""
    rowptr, cols = S.pattern(name)
    p = S.pool(POOL)
    first = S.values_pool(rowptr, cols, p)
    one_new = first.copy()
    one_new[np.flatnonzero(~S.diag_mask(rowptr, cols))[17]] = 3.25
    assert 3.25 not in p
    steps = [("600 values", first, POOL + 1), ("the same again", first, POOL + 1),
             ("the same pool dealt differently", S.values_pool(rowptr, cols, p, shift=7), POOL + 1), ("one new value", one_new, POOL + 2),
             ("5000 values", S.values_pool(rowptr, cols, S.pool(5000, seed=1)), 0), ("600 values again", first, 0)]
    s, seen, ys = None, [], []
    for what, vals, want in steps:
        if s is None:
            s = _load(name, vals)
        else:
            _push(s, name, vals)
        entries, y, fail = _grouped_product(s, name, vals)
        seen.append((what, entries, fail)); ys.append(y)
    s.free()
    print(seen)
    assert seen == [(what, want, "") for what, _, want in steps]
    assert np.array_equal(ys[0].view(np.int64), ys[1].view(np.int64)) and np.array_equal(ys[0].view(np.int64), ys[5].view(np.int64))


@pytest.mark.parametrize("name", ["stencil", "blocks3"])
def test_hostile_bit_patterns(name):
    """+-inf, DBL_MAX and two NaNs off the diagonal: the product is the chain's, by bits where it is finite and by class elsewhere.
    The all-ones pattern that marks a free slot of the dictionary's table fails the form, not the table: 0 entries, the right
    product from the fp64 copy, and 0 entries for clean values afterwards."""
    rowptr, cols = S.pattern(name)
    vals = S.values_pool(rowptr, cols, S.pool(POOL, extra=S.HOSTILE))
    assert len(np.unique(vals.view(np.uint64))) == POOL and np.isnan(vals).sum() >= 2 and np.isinf(vals).sum() >= 2
    s = _load(name, vals)
    entries, y, fail = _grouped_product(s, name, vals)
    assert not fail and not np.isfinite(y).all() and np.isfinite(y).any()
    assert entries in (0, POOL + 1)          # (these are values like any other: nothing says they must be refused)
    s.free()
    vals = S.values_pool(rowptr, cols, S.pool(POOL, extra=(S.VD_EMPTY,)))
    assert (vals.view(np.uint64) == S.VD_EMPTY).any()
    s = _load(name, vals)
    entries, _, fail = _grouped_product(s, name, vals)
    assert entries == 0 and not fail
    clean = S.values_pool(rowptr, cols, S.pool(POOL))
    _push(s, name, clean)
    entries, _, fail = _grouped_product(s, name, clean)
    s.free()
    assert entries == 0 and not fail


# ---------------------------------------------------------------------------------------------------------------------------------
# the WITH_DOT instantiations: five iterations of the Jacobi-PCG
# ---------------------------------------------------------------------------------------------------------------------------------
ITS = 5


def _pcg_longdouble_dots(rowptr, cols, vals, b):
    """orc_pcg_jacobi's loop for ITS iterations with the products of the device (the chain) and every dot in longdouble"""
    def dot(a, c):
        return float(np.dot(a.astype(np.longdouble), c.astype(np.longdouble)))
    dinv = 1.0 / vals[S.diag_mask(rowptr, cols)]
    x, r = np.zeros_like(b), b.copy()
    z = r * dinv
    p = z.copy()
    beta = dot(r, z)
    hist = [np.sqrt(dot(z, z))]
    for _ in range(ITS):
        w = O.spmv_chain(rowptr, cols, vals, p)
        alpha = beta / dot(p, w)
        x = x + alpha * p
        r = r - alpha * w
        z = r * dinv
        betan = dot(r, z)
        hist.append(np.sqrt(dot(z, z)))
        p = z + (betan / beta) * p
        beta = betan
    return np.array(hist), x


def _deviation(hist, x, ref):
    return max(np.abs(hist - ref[0]).max() / np.abs(ref[0]).max(), np.abs(x - ref[1]).max() / np.abs(ref[1]).max())


@functools.lru_cache(maxsize=None)
def _dot_problem(name):
    rowptr, cols = S.pattern(name)
    vals = S.values_dominant(rowptr, cols)
    b = np.random.default_rng(21).standard_normal(len(rowptr) - 1)
    ref = _pcg_longdouble_dots(rowptr, cols, vals, b)
    xo, its, _, _, ho = O.pcg_jacobi(rowptr, cols, vals, b, rtol=1e-300, maxits=ITS, hist_len=ITS + 1)
    assert its == ITS and len(ho) == ITS + 1
    return vals, b, ref, _deviation(ho, xo, ref)


def _five_iterations(name, debug, fmt, vd, want):
    rowptr, cols = S.pattern(name)
    vals, b, _, _ = _dot_problem(name)
    s = _load(name, vals, debug)
    with _env(PFEM_SPMV_VALDICT=vd):
        s.setSpmvFormat(fmt)
        s.VecSetValues(np.arange(len(b), dtype=np.int32), b, pf.solver.INSERT_VALUES)
        s.setTolerances(rtol=1e-300, maxits=ITS)
        its, reason, _ = s.factoriseAndSolve()
        form, entries = _form(s), s.spmvValueDictionary()
        hist, x = s.getHistory(), s.getSolution()
    s.free()
    assert its == ITS and reason == -3 and len(hist) == ITS + 1
    assert form == want and (entries > 0) == (vd == "1" and _has_codes(want))
    return hist, x


# matrix -> the layouts in (debug switch, format, form) whose blocks and partials are the same: bit-identical runs.  (A pattern's
# relative groups have literal gaps or the table, never both; PFEM_DEBUG_REL_GAP32 turns a table into 32-bit gaps: those two share
# a matrix, the literal mode stands next to them on the matrices without a large gap.)
DOT_CASES = {
    "stencil": [[(None, "int32", (1, 32, 0, False))], [(None, "gaps16", (1, 16, 0, False))], [(None, "grouped", (4, 16, 0, False))]],
    "blocks3": [[(None, "int32", (1, 32, 0, False))], [(None, "gaps16", (1, 16, 0, False))], [(None, "grouped", (3, 16, 0, False))]],
    "gap65536": [[(None, "gaps16", (1, 16, 1, False))],
                 [(None, "grouped", (4, 16, 1, False)), ("PFEM_DEBUG_REL_GAP32", "grouped", (4, 32, 0, False))]],
    "gaps257": [[(None, "gaps16", (1, 16, 0, True))], [(None, "grouped", (4, 32, 0, False))]],
    "blocks3_table": [[(None, "gaps16", (1, 16, 3, False))], [(None, "grouped", (3, 16, 3, False))]],
}


@pytest.mark.parametrize("name", sorted(DOT_CASES))
def test_five_pcg_iterations_on_every_layout(name):
    """(p, Ap) from the SpMV's epilogue: history and iterate bit-identical between the two value streams and between the gap modes
    of the relative groups; across layouts (other blocks, other partial sums) within 8 x the deviation the serial plain-double
    oracle has from the same loop with longdouble dots"""
    _, _, ref, oracle_dev = _dot_problem(name)
    for same in DOT_CASES[name]:
        runs = {}
        for debug, fmt, want in same:
            for vd in ("0", "1") if _has_codes(want) else ("1",):
                runs[debug, fmt, vd] = _five_iterations(name, debug, fmt, vd, want)
        first = next(iter(runs.values()))
        for key, (hist, x) in runs.items():
            dev = _deviation(hist, x, ref)
            print(f"{name} {key}: deviation {dev:.3e} from the longdouble-dot loop, the oracle's {oracle_dev:.3e}")
            assert np.array_equal(hist.view(np.int64), first[0].view(np.int64)) and np.array_equal(x.view(np.int64), first[1].view(np.int64)), key
            assert dev <= 8 * oracle_dev, key

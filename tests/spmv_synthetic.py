"""Synthetic CSR matrices that reach every SpMV form and every path inside it (tests/test_gpu_spmv_synthetic.py runs them on the
device, tests/test_spmv_synthetic_host.py checks on the CPU that each one has the shape it is meant to have).

The finite-element generators give one stencil length per mesh, a handful of large gaps and a few thousand values.  The SpMV forms
are chosen from the pattern alone, so a pattern made here reaches each of them through PetscSolver.loadCSR:

* ``stencil``: scalar rows in groups of four that share a set of relative offsets -- the shape the 4-row relative groups (k_spmvr)
  are kept for.  The width changes every 256 rows, so every class of ``width mod 4`` / ``mod 8`` occurs; one group in four is
  shorter than its slice (lanes of unequal length), 3 % of the rows lack one offset of their group (explicit zeros), the first
  and last rows lose the columns outside the matrix (reads into the guard band of x), and n is no multiple of 4 or 256 (a last
  group of fewer than four rows, a last slice that is partly empty).
* its large-gap variants: the groups of width >= 3 end in the offsets +41 and ``bigs[g mod K]``, so the last gap of their rows and
  of their unions is ``bigs[..] - 41`` exactly.
* ``blocks3``: the node graph of ``stencil`` with 3, 2 or 1 dofs a node -- the 3-row groups (k_spmvg) with groups of 1 and 2 rows
  among them and widths that are no multiple of 3.

Rules every matrix keeps (they keep the flush solve at zero iterations and every run harmless): every row stores a finite,
positive diagonal entry; hostile values go off the diagonal only; every x is finite and has no zeros.

``model`` restates on the host what build_cols16 / build_groups / build_rel_groups (pfem_device.hip) decide from a pattern.
"""
import functools

import numpy as np

K_GAP_TABLE = 256          # kGapTable
VD_MAX = 4096              # kVdMax
SMALL = np.r_[-40:0, 1:41]


# ---------------------------------------------------------------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------------------------------------------------------------
def _csr(n, rows, cols):
    rows = np.concatenate(rows); cols = np.concatenate(cols)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols.astype(np.int32)


def stencil(n, wmax=12, wfix=None, bigs=(), sym=False, seed=0, drop=0.03):
    """(rowptr, cols): group g = rows 4g .. 4g+3 shares an offset set that holds 0; group-slice S = g // 64 has width
    ``wfix or 1 + S mod wmax``; group g with g mod 4 == S mod 4 draws a shorter width.  ``bigs``: groups of width >= 3 end in
    +41 and bigs[g mod len(bigs)] (``sym``: start at -bigs[..] and end at +bigs[..] instead); neither is ever dropped."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for g in range((n + 3) // 4):
        S = g // 64
        w = wfix or 1 + S % wmax
        if not wfix and w > 1 and g % 4 == S % 4:
            w = int(rng.integers(1, w + 1))
        isbig = bool(len(bigs)) and w >= 3
        ns = w - 3 if isbig else w - 1                      # small offsets next to 0
        off = np.r_[0, rng.choice(SMALL, size=ns, replace=False)] if ns > 0 else np.zeros(1, np.int64)
        if isbig:
            b = int(bigs[g % len(bigs)])
            off = np.r_[off, -b, b] if sym else np.r_[off, 41, b]
        for r in range(4 * g, min(4 * g + 4, n)):
            c = r + off
            keep = (c >= 0) & (c < n)
            if drop and ns > 0 and rng.random() < drop:
                keep[1 + int(rng.integers(ns))] = False
            rows.append(np.full(int(keep.sum()), r, np.int64)); cols.append(c[keep])
    return _csr(n, rows, cols)


def node_dofs(n_nodes):
    """3 dofs a node; one node in 12 has 2, one in 24 has 1"""
    i = np.arange(n_nodes)
    return np.where(i % 24 == 11, 1, np.where(i % 12 == 5, 2, 3))


def blocks3(n_nodes, **kw):
    """(rowptr, cols, dofs per node): ``stencil(n_nodes, ...)`` as a node graph, every node pair a full block of its dofs"""
    nrp, ncols = stencil(n_nodes, **kw)
    d = node_dofs(n_nodes)
    first = np.r_[0, np.cumsum(d)]
    rows, cols = [], []
    for i in range(n_nodes):
        nb = ncols[nrp[i]:nrp[i + 1]]
        c = np.concatenate([np.arange(first[j], first[j + 1]) for j in nb])
        for r in range(first[i], first[i + 1]):
            rows.append(np.full(len(c), r, np.int64)); cols.append(c)
    rowptr, cols = _csr(int(first[-1]), rows, cols)
    return rowptr, cols, d


# name -> the pattern; every large-gap case says in its name what it is for (the host tests assert that it is so)
B = 65536
CASES = {
    "stencil": lambda: stencil(6403),                                                  # 25 group-slices, every width 1 .. 12
    "stencil24": lambda: stencil(6403, wmax=24, seed=1),                               # widths up to 24: the W = 8 trips of the row forms
    "blocks3": lambda: blocks3(6403, seed=2)[:2],
    "gaps256": lambda: stencil(74003, bigs=[B + 17 * k for k in range(256)], seed=3),  # the gap table exactly full
    "gaps257": lambda: stencil(74003, bigs=[B + 17 * k for k in range(257)], seed=4),  # one more: escapes / 32-bit gaps; few escapes
    "gap32767": lambda: stencil(74003, bigs=[32767 + 41, 70000 + 41], seed=5),         # literal in the table form the other gap forces
    "gap32768": lambda: stencil(74003, bigs=[32768 + 41, 70000 + 41], seed=6),         # a table code
    "gap65534": lambda: stencil(74003, bigs=[65534 + 41], seed=7),
    "gap65535": lambda: stencil(74003, bigs=[65535 + 41], seed=8),                     # the last gap that fits plain 16 bits
    "gap65536": lambda: stencil(74003, bigs=[65536 + 41], seed=9),                     # the first that does not
    # with the row form's table switched off (PFEM_DEBUG_NO_ROW_GAP_TABLE) the other gap forces the escape form: 65 534 is its last
    # literal gap, 65 535 is its escape code
    "gap65534e": lambda: stencil(74003, bigs=[65534 + 41, 70000 + 41], seed=14),
    "gap65535e": lambda: stencil(74003, bigs=[65535 + 41, 70000 + 41], seed=15),
    # three dofs a node and a far neighbour 24 000 nodes = about 68 000 dofs on: the 3-row groups with the gap table
    "blocks3_table": lambda: blocks3(27003, wfix=3, bigs=[24000 + 41], seed=13)[:2],
    # rows -b' 0 +b' with 257 values of b': most rows keep a large gap, more than a quarter of the stored entries escape
    "escapes_heavy": lambda: stencil(140003, wfix=3, bigs=[B + 17 * k for k in range(257)], sym=True, seed=10, drop=0.0),
}


@functools.lru_cache(maxsize=None)
def pattern(name):
    rowptr, cols = CASES[name]()
    rowptr.setflags(write=False); cols.setflags(write=False)
    return rowptr, cols


# ---------------------------------------------------------------------------------------------------------------------------------
# what the library decides from a pattern, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def _slice_max(a, per):
    pad = (-len(a)) % per
    return np.r_[a, np.zeros(pad, a.dtype)].reshape(-1, per).max(axis=1)


@functools.lru_cache(maxsize=None)
def model(name):
    """Counts of the pattern and the forms build_cols16 / build_groups / build_rel_groups keep for it:
    ``row`` / ``rel`` in {"lit16", "table", "escape", "int32", "gap32", None}, ``group3`` (bool)."""
    rowptr, cols = pattern(name)
    n = len(rowptr) - 1
    rl = np.diff(rowptr)
    row_of = np.repeat(np.arange(n), rl)
    m = dict(n=n, nnz=int(rowptr[-1]), widths=sorted(set(_slice_max(rl, 64).tolist())))
    m["stored"] = stored = int(64 * _slice_max(rl, 64).sum())
    inner = np.ones(len(cols), bool); inner[rowptr[:-1][rl > 0]] = False          # entries after the first of their row
    gaps = (cols.astype(np.int64) - np.r_[0, cols[:-1]])[inner]
    m["row_large"] = sorted(set(gaps[gaps >= 0x8000].tolist()))                   # what k_row_gap_table collects
    m["row_max_gap"] = int(gaps.max()) if len(gaps) else 0
    m["esc"] = esc = int((gaps >= 0xffff).sum())                                  # what k_cols16_fill_escape counts
    if m["row_max_gap"] <= 65535:
        m["row"] = "lit16"
    elif len(m["row_large"]) <= K_GAP_TABLE:
        m["row"] = "table"
    else:
        m["row"] = "escape" if 4 * esc <= stored else "int32"
    # 3-row groups: runs of consecutive rows with identical columns, cut every 3 rows
    same = np.zeros(n, bool)
    for r in range(1, n):
        same[r] = rl[r] > 0 and rl[r] == rl[r - 1] and np.array_equal(cols[rowptr[r]:rowptr[r + 1]], cols[rowptr[r - 1]:rowptr[r]])
    run_start = np.maximum.accumulate(np.where(same, 0, np.arange(n)))
    head = (np.arange(n) - run_start) % 3 == 0
    m["groups"] = ng = int(head.sum())
    m["group3"] = m["row"] in ("lit16", "table") and n >= 2 and 11 * ng <= 4 * n
    grow0 = np.flatnonzero(head)
    m["group_rows"] = np.bincount(np.diff(np.r_[grow0, n]), minlength=4)[1:4].tolist()     # groups of 1, 2, 3 rows
    m["gwidths"] = sorted(set(_slice_max(rl[grow0], 64).tolist()))
    m["gstored"] = int(64 * _slice_max(rl[grow0], 64).sum())                       # lane entries of the 3-row form, 3 slots each
    # relative groups: the union of (column - row) over 4 consecutive rows
    key = np.unique((row_of // 4).astype(np.int64) * (1 << 34) + (cols.astype(np.int64) - row_of + (1 << 33)))
    grp, off = key >> 34, (key & ((1 << 34) - 1)) - (1 << 33)
    u = np.bincount(grp, minlength=(n + 3) // 4)
    m["union"] = union = int(64 * _slice_max(u, 64).sum())
    m["rwidths"] = sorted(set(_slice_max(u, 64).tolist()))
    first = np.r_[True, grp[1:] != grp[:-1]]
    ugaps = (off - np.r_[0, off[:-1]])[~first]
    m["rel_large"] = sorted(set(ugaps[ugaps >= 0x8000].tolist()))
    wide = len(ugaps) > 0 and ugaps.max() > 65535
    rel = "lit16" if not wide else ("table" if len(m["rel_large"]) <= K_GAP_TABLE else "gap32")
    m["rel_bytes_ratio"] = union * (32.0 + (4.0 if rel == "gap32" else 2.0)) / (stored * (12.0 if m["row"] == "int32" else 10.0))
    m["rel"] = rel if (not m["group3"] and n >= 4 and m["rel_bytes_ratio"] <= 0.95) else None
    m["ratio16"] = 34.0 * union / (10.0 * stored)            # union form with 16-bit gaps against the 16-bit row form
    m["ratio32"] = 36.0 * union / (12.0 * stored)            # ... with 32-bit gaps against int32 rows
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# values and vectors
# ---------------------------------------------------------------------------------------------------------------------------------
def diag_mask(rowptr, cols):
    n = len(rowptr) - 1
    return cols == np.repeat(np.arange(n), np.diff(rowptr))


def values_int(rowptr, cols, seed=0):
    """nonzero integers, |v| <= 1024, the diagonal positive: with x_int every row sum is exact"""
    rng = np.random.default_rng(100 + seed)
    v = rng.integers(1, 1025, size=len(cols)) * rng.choice([-1, 1], size=len(cols))
    d = diag_mask(rowptr, cols)
    v[d] = np.abs(v[d])
    return v.astype(np.float64)


def x_int(n, seed=0):
    rng = np.random.default_rng(200 + seed)
    return (rng.integers(1, 1025, size=n) * rng.choice([-1, 1], size=n)).astype(np.float64)


def x_normal(n, seed=0):
    x = np.random.default_rng(300 + seed).standard_normal(n)
    x[x == 0.0] = 1.0
    return x


def pool(K, seed=0, extra=()):
    """K distinct doubles, none a zero, the even-numbered ones positive (the diagonal draws from those); ``extra``: 64-bit
    patterns that replace the last odd-numbered members (hostile or special values: they go off the diagonal only)"""
    rng = np.random.default_rng(400 + seed)
    while True:
        p = rng.uniform(0.5, 2.0, size=K)
        if len(np.unique(p)) == K:
            break
    p[1::2] *= -1.0
    odd = np.arange(1, K, 2)[::-1]
    assert len(extra) <= len(odd)
    for i, e in zip(odd, extra):
        p.view(np.uint64)[i] = np.uint64(e)
    return p


def pattern_of(value):
    """the 64-bit pattern of a double, for ``pool(extra=...)``"""
    return int(np.array([value], dtype=np.float64).view(np.uint64)[0])


VD_EMPTY = 0xFFFFFFFFFFFFFFFF                    # kVdEmpty: the all-ones NaN that marks a free slot of the dictionary's table
NAN_A, NAN_B = 0x7FF8000000000001, 0xFFF0000000BEEF01      # two NaNs with different payloads (a quiet and a signalling one)
HOSTILE = (pattern_of(np.inf), pattern_of(-np.inf), pattern_of(np.finfo(np.float64).max), NAN_A, NAN_B)


def values_pool(rowptr, cols, p, shift=0):
    """the pool dealt round-robin: all of it over the off-diagonal entries, its even-numbered members over the diagonal"""
    d = diag_mask(rowptr, cols)
    v = np.empty(len(cols))
    nd, no = int(d.sum()), int((~d).sum())
    pos = p[0::2]
    v[d] = pos[(np.arange(nd) + shift) % len(pos)]
    v[~d] = p[(np.arange(no) + shift) % len(p)]
    return v


def values_normal(rowptr, cols, seed=0):
    v = np.random.default_rng(500 + seed).standard_normal(len(cols))
    v[v == 0.0] = 1.0
    d = diag_mask(rowptr, cols)
    v[d] = np.abs(v[d])
    return v


def values_dominant(rowptr, cols, seed=0, vmax=4):
    """integer off-diagonals and diag = sum |row| + sum |column| + 1: the symmetric part is diagonally dominant, (p, A p) > 0.
    |v| <= vmax off the diagonal keeps the diagonal sums few enough for the value dictionary."""
    rng = np.random.default_rng(600 + seed)
    v = (rng.integers(1, vmax + 1, size=len(cols)) * rng.choice([-1, 1], size=len(cols))).astype(np.float64)
    d = diag_mask(rowptr, cols)
    n = len(rowptr) - 1
    a = np.where(d, 0.0, np.abs(v))
    row_of = np.repeat(np.arange(n), np.diff(rowptr))
    v[d] = np.bincount(row_of, weights=a, minlength=n) + np.bincount(cols, weights=a, minlength=n) + 1.0
    return v


def bits(y):
    """the bit patterns of y with -0.0 taken for +0.0: k_spmv starts a row from fma(v, x, 0.0) where the other forms start from
    v * x, and a row that lacks the first offset of its group starts from 0 * x -- sums that differ in the sign of a zero only"""
    return (np.asarray(y, dtype=np.float64) + 0.0).view(np.int64)

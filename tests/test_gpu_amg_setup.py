"""The hierarchy that the symbolic phase of -pc_type gamg builds (amg_symbolic, pfem_amg.inc), level by level, as integers.

The table below is not derived here: it is what the library built before the set-up's shared steps were written once (commit
42c1877, recorded twice in separate processes with every field equal; profiles/LAB_NOTES.md), so that a change to the member
lists, the sorted route to a coarse pattern, the counted route, the matching's tail or the order of the steps shows up as a
changed row.  Per case, after the pattern's first solve: the iteration count, and per level rows and nonzeros, how its aggregates
were formed, the integers of its transfer, the number of aggregates and a short sha256 of the aggregate of every dof; from level
1 on a short sha256 of the level's row pointers and of its columns.  Integers only: the VALUES of every level are checked
against scipy's P^T A P by test_gpu_amg_pieces.py, whose meshes these are.

cube28: bricks, maps by walks.  ragged: bricks on an uneven box (50 505 rows).  aniso: lattice passes.  matched: matching, scalar.
beam: node bricks, maps by codes.  beam_moved: rigid-body levels through the sorted maps.  cook: 2-D, coarse block 3.
pinned: three dofs to the node WITHOUT the rigid-body transfer (the node_of / comp_of branch of k_amg_emit_node_keys,
k_amg_mark_cdofs and k_amg_coarse_nodes, which no mesh of test_gpu_amg_pieces.py reaches).
"""
import dataclasses
import functools
import hashlib

import numpy as np
import pytest

import pfemfort_amd as pf
from pfemfort_amd import host as H
from test_gpu_amg_pieces import CASES, _env, _new_solver
from test_gpu_parity import _device_problem

pytestmark = pytest.mark.gpu

SETUP_CASES = ("cube28", "ragged", "aniso", "matched", "beam", "beam_moved", "cook", "pinned")
PINNED_CELLS = (4, 24, 4)


def _pinned(cells=PINNED_CELLS):
    """A clamped beam with ONE dof of one free node fixed as well: its nodes are no longer whole, the rigid-body transfer is
    refused, and the levels keep three dofs to the node with one coarse dof per aggregate and component."""
    m = H.gen_box_tets(-0.5, 0.5, cells[0], 0.0, 6.0, cells[1], -0.5, 0.5, cells[2], bc_mode=1, ndof=3)
    free = np.setdiff1d(np.arange(m.xyz.shape[1]), np.unique(m.bc_node))
    return dataclasses.replace(m, bc_node=np.append(m.bc_node, free[len(free) // 2]).astype(m.bc_node.dtype),
                               bc_dof=np.append(m.bc_dof, 0).astype(m.bc_dof.dtype), bc_val=np.append(m.bc_val, 0.0))


def _solver(case):
    if case in CASES:
        return _new_solver(case)[0]
    s, _ = _device_problem(pf.ELAST_TET, _pinned(), H.ELAST_ELEMDATA)
    s.setPreconditioner("gamg")
    s.setTolerances(rtol=1e-10, maxits=5000)
    return s


def _sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()[:16]


def observe(case):
    """The record of one case: a fresh solver, the pattern's first solve, what the getters say about every level."""
    with _env(**CASES.get(case, {}).get("env", {})):
        s = _solver(case)
        try:
            its, reason, _ = s.factoriseAndSolve()
            assert reason == 2
            info, kinds = s.amgInfo(), s.amgAggregation()
            levels = []
            for l in range(info["levels"]):
                rec = {"rows": int(info["rows"][l]), "nnz": int(info["nnz"][l])}
                if l + 1 < info["levels"]:
                    t = s.amgTransfer(l)
                    a = s.amgAggregates(l, info["rows"][l])
                    rec.update(kind=kinds[l], transfer=[int(t["rbm"]), t["fine_bs"], t["coarse_bs"], t["dim"], t["n_nodes"]],
                               aggregates=int(len(np.unique(a))), agg_sha=_sha(a, np.int32))
                if l >= 1:
                    rowptr, cols, _ = s.amgLevelCSR(l)
                    rec.update(rowptr_sha=_sha(rowptr, np.int64), cols_sha=_sha(cols, np.int32))
                levels.append(rec)
        finally:
            s.free()
    return {"its": int(its), "levels": levels}


EXPECTED = {
    "cube28": {"its": 19, "levels": [
        {"rows": 19683, "nnz": 278071, "kind": "bricks", "transfer": [0, 1, 1, 0, 19683], "aggregates": 2744, "agg_sha": "f20448fe463607cd"},
        {"rows": 2744, "nnz": 41016, "kind": "bricks", "transfer": [0, 1, 1, 0, 2744], "aggregates": 343, "agg_sha": "f2226cf1e9223821", "rowptr_sha": "0bcc816b9f298b58", "cols_sha": "06114ebd84f5a2c0"},
        {"rows": 343, "nnz": 4555, "kind": "bricks", "transfer": [0, 1, 1, 0, 343], "aggregates": 64, "agg_sha": "eb7375cc84f1fa6f", "rowptr_sha": "119eaaac208d5777", "cols_sha": "6542af50ea685d42"},
        {"rows": 64, "nnz": 694, "rowptr_sha": "e9fac0a128fcdc3b", "cols_sha": "0dbf45402d6d09e6"},
    ]},
    "ragged": {"its": 20, "levels": [
        {"rows": 50505, "nnz": 725193, "kind": "bricks", "transfer": [0, 1, 1, 0, 50505], "aggregates": 6840, "agg_sha": "f6c239a5e40978c0"},
        {"rows": 6840, "nnz": 105798, "kind": "bricks", "transfer": [0, 1, 1, 0, 6840], "aggregates": 900, "agg_sha": "ff28323ea5a57145", "rowptr_sha": "a0433dc28b6d88df", "cols_sha": "9342cc73707981e7"},
        {"rows": 900, "nnz": 12832, "kind": "bricks", "transfer": [0, 1, 1, 0, 900], "aggregates": 125, "agg_sha": "2b7441688c03d264", "rowptr_sha": "d734bd79640c7e85", "cols_sha": "3483359d9138a3c5"},
        {"rows": 125, "nnz": 1493, "rowptr_sha": "d86f8e993654a3dc", "cols_sha": "06f1c4314f1dfeab"},
    ]},
    "aniso": {"its": 65, "levels": [
        {"rows": 6859, "nnz": 94447, "kind": "bricks", "transfer": [0, 1, 1, 0, 6859], "aggregates": 1000, "agg_sha": "295dbea4abb8f8fe"},
        {"rows": 1000, "nnz": 14176, "kind": "lattice-passes", "transfer": [0, 1, 1, 0, 1000], "aggregates": 217, "agg_sha": "a234da8bd4f4c582", "rowptr_sha": "0006a0b005c2bf24", "cols_sha": "d9053b6d6524f2e8"},
        {"rows": 217, "nnz": 2523, "kind": "matching", "transfer": [0, 1, 1, 0, 217], "aggregates": 67, "agg_sha": "4cf6b0ecdfd7e1cf", "rowptr_sha": "9a34c7ee620be69d", "cols_sha": "df089ee7b4cfb057"},
        {"rows": 67, "nnz": 609, "rowptr_sha": "5d8c405794509e5e", "cols_sha": "74cc35938acca20d"},
    ]},
    "matched": {"its": 21, "levels": [
        {"rows": 1872, "nnz": 24578, "kind": "matching", "transfer": [0, 1, 1, 0, 1872], "aggregates": 275, "agg_sha": "1f008a3da53f9537"},
        {"rows": 275, "nnz": 3555, "kind": "matching", "transfer": [0, 1, 1, 0, 275], "aggregates": 42, "agg_sha": "86ad52df5908d2a1", "rowptr_sha": "458a53f2800e1ab0", "cols_sha": "abc5f648fcdefad4"},
        {"rows": 42, "nnz": 444, "rowptr_sha": "3469cd962d410991", "cols_sha": "52b2e07aa1ea55a7"},
    ]},
    "beam": {"its": 57, "levels": [
        {"rows": 5292, "nnz": 200106, "kind": "node-bricks", "transfer": [1, 3, 6, 3, 1764], "aggregates": 108, "agg_sha": "da1f063fd0dd7d27"},
        {"rows": 216, "nnz": 10872, "kind": "node-bricks", "transfer": [1, 6, 6, 3, 36], "aggregates": 24, "agg_sha": "d4b75b78a8c9f58c", "rowptr_sha": "0214b00243c92fae", "cols_sha": "b156bdd80449bc88"},
        {"rows": 24, "nnz": 360, "rowptr_sha": "a48c65fad01f8b60", "cols_sha": "2b23adbf7e0aa8eb"},
    ]},
    "beam_moved": {"its": 63, "levels": [
        {"rows": 5292, "nnz": 200106, "kind": "matching", "transfer": [1, 3, 6, 3, 1764], "aggregates": 219, "agg_sha": "4a7f9d06a3581748"},
        {"rows": 438, "nnz": 25164, "kind": "matching", "transfer": [1, 6, 6, 3, 73], "aggregates": 66, "agg_sha": "e3a734f316272a77", "rowptr_sha": "a20d7e506fecf38b", "cols_sha": "6c8e2568b66a282b"},
        {"rows": 66, "nnz": 1908, "rowptr_sha": "5f44a975b9e33d67", "cols_sha": "f7aa45ea0e834d18"},
    ]},
    "cook": {"its": 86, "levels": [
        {"rows": 2112, "nnz": 28536, "kind": "matching", "transfer": [1, 2, 3, 2, 1056], "aggregates": 94, "agg_sha": "2a9f695b7a7d196d"},
        {"rows": 141, "nnz": 2457, "kind": "matching", "transfer": [1, 3, 3, 2, 47], "aggregates": 21, "agg_sha": "eb1fe6a87a8c2941", "rowptr_sha": "aecca8c20b6bd054", "cols_sha": "f31dd642764fd84b"},
        {"rows": 21, "nnz": 261, "rowptr_sha": "6e73903d5e3e5862", "cols_sha": "6c204809ecd1602b"},
    ]},
    "pinned": {"its": 154, "levels": [
        {"rows": 1799, "nnz": 63061, "kind": "lattice-passes", "transfer": [0, 3, 3, 0, 600], "aggregates": 132, "agg_sha": "712cd3f4b068a382"},
        {"rows": 132, "nnz": 3366, "kind": "lattice-passes", "transfer": [0, 3, 3, 0, 44], "aggregates": 15, "agg_sha": "e03a988dafe91ac0", "rowptr_sha": "302b5c60e0ed7efb", "cols_sha": "559214bb2c481272"},
        {"rows": 15, "nnz": 117, "rowptr_sha": "7c90935ace3e1c7a", "cols_sha": "2a20cf555c1660d0"},
    ]},
}


@functools.lru_cache(maxsize=None)
def _observed(case):
    return observe(case)


@pytest.mark.parametrize("case", SETUP_CASES)
def test_the_hierarchy_is_the_recorded_one(case):
    got, want = _observed(case), EXPECTED[case]
    assert got["its"] == want["its"]
    assert len(got["levels"]) == len(want["levels"])
    for l, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        for key in sorted(set(g) | set(w)):
            assert g.get(key) == w.get(key), (case, l, key, g.get(key), w.get(key))

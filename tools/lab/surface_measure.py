"""What the surface loads cost at BASELINE configs 3 and 4 (the 200^3 Poisson box, the 50 x 300 x 50 elastic beam): the
extraction of the boundary sides (pfem_mesh_boundary_faces: key kernel, radix sort, match, selection, the ids back to the host)
beside the pattern build of the same run -- the symbolic phase it sits next to --, and pfem_rhs_add_surface_load on one face of
the box (upload of the sides and values included: it is what a load step pays).

Host clock around calls that end in a device synchronise.  The extraction is kept on the handle, so every repetition runs on a
freshly generated mesh; the first one also pays hipcub's code objects and the pool's first allocations, and is reported apart.
`python tools/lab/surface_measure.py [out.json]`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402

REPS = 4
out = {}
for name, kind, box, bc, ndof, ed, load, value in (
        ("config3_poisson_200", pf.POISSON_TET, (-1, 1, 200, -1, 1, 200, -1, 1, 200), 0, 1, H.POISSON_ELEMDATA, "flux", [1.0]),
        ("config4_beam_50x300x50", pf.ELAST_TET, (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50), 1, 3, H.ELAST_ELEMDATA, "pressure", [1.0])):
    nE = (box[2], box[5], box[8])
    sz = H.box_slab_sizes(*nE, bc, ndof)
    nElem = 6 * nE[0] * nE[1] * nE[2]
    s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    extract, pattern = [], []
    for rep in range(REPS):
        s.generateBoxMesh(kind, *box, bc_mode=bc)                 # a new mesh drops the sides kept on the handle
        t0 = time.perf_counter()
        fe, fs = s.boundaryFaces()
        extract.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        s.buildPattern()
        pattern.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    s.boundaryFaces()
    cached = (time.perf_counter() - t0) * 1e3
    want = 4 * (nE[0] * nE[1] + nE[1] * nE[2] + nE[0] * nE[2])
    assert len(fe) == want, (len(fe), want)
    t0 = time.perf_counter()
    meas, nrm, nodes = s.surfaceGeometry(fe, fs)
    geometry = (time.perf_counter() - t0) * 1e3
    face = nrm[1] == 1.0                                          # the face y = y1: the beam's end face, one side of the cube
    assert face.sum() == 2 * nE[0] * nE[2]
    area = (box[1] - box[0]) * (box[7] - box[6])
    assert abs(meas[face].sum() - area) < 1e-9 * area
    s.assemble(ed, H.TIMEDATA)
    r0 = s.getRHS()
    add = []
    for rep in range(REPS):
        t0 = time.perf_counter()
        s.addSurfaceLoad(fe[face], fs[face], load, value, layout="uniform")
        add.append((time.perf_counter() - t0) * 1e3)
    gained = (s.getRHS() - r0).sum()
    res = {"elements": nElem, "sides": 4 * nElem, "boundary_sides": int(len(fe)), "loaded_sides": int(face.sum()),
           "boundary_faces_ms": extract, "boundary_faces_ms_first": extract[0], "boundary_faces_ms_min_warm": min(extract[1:]),
           "pattern_build_ms": pattern, "pattern_build_ms_min_warm": min(pattern[1:]), "pattern_build_kernel_ms": s.timings()["pattern_ms"],
           "boundary_faces_over_pattern_build": min(extract[1:]) / min(pattern[1:]),
           "boundary_faces_cached_ms": cached, "surface_geometry_all_boundary_ms": geometry,
           "add_surface_load_ms": add, "add_surface_load_ms_min_warm": min(add[1:]),
           "temporary_bytes_formula": 132 * nElem, "rhs_gained_sum": float(gained), "repetitions": REPS}
    print(name, json.dumps(res), flush=True)
    out[name] = res
    s.free()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)

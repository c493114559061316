"""Kernel time of the post-processing passes (pfem_post_elements, pfem_post_nodal_forces) on BASELINE configs 3 and 4 beside the
assembly kernel of the same run, with the compulsory bytes of each pass.  `python tools/lab/post_measure.py [out.json]`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402

out = {}
for name, kind, box, bc, ndof, ed in (("config3_poisson_200", pf.POISSON_TET, (-1, 1, 200, -1, 1, 200, -1, 1, 200), 0, 1, H.POISSON_ELEMDATA),
                                      ("config4_beam_50x300x50", pf.ELAST_TET, (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50), 1, 3, H.ELAST_ELEMDATA)):
    nE = (box[2], box[5], box[8])
    sz = H.box_slab_sizes(*nE, bc, ndof)
    s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    s.generateBoxMesh(kind, *box, bc_mode=bc)
    s.buildPattern()
    asm = []
    for _ in range(4):
        s.assemble(ed, H.TIMEDATA)
        asm.append(s.timings()["assemble_ms"])
    u = np.random.default_rng(1).standard_normal((s.nNode, ndof))
    el, nf, nfs, wall = [], [], [], []
    for _ in range(4):
        t0 = time.perf_counter()
        s.elementFields(ed, u)
        wall.append(time.perf_counter() - t0)
        el.append(s.postTimings()["elements_ms"])
        s.nodalForces(ed, H.TIMEDATA, u)
        nf.append(s.postTimings()["nodal_forces_ms"])
    s.setAssemblyMode("scatter")
    for _ in range(3):
        s.nodalForces(ed, H.TIMEDATA, u)
        nfs.append(s.postTimings()["nodal_forces_ms"])
    s.setAssemblyMode("gather")
    ng = {pf.POISSON_TET: 3, pf.ELAST_TET: 6}[kind]
    nElem, nNode = s.nElem, s.nNode
    info = s.assemblyInfo()
    inc = 4 * nElem
    # compulsory bytes: every array read or written once
    b_el = nElem * 16 + nNode * (3 + ndof) * 8 + nElem * (2 * ng + 1) * 8
    b_nf = inc * 16 + (nNode // 64 + 1) * 8 + nNode * 4 + nNode * (3 + ndof) * 8 + nNode * ndof * 8
    r = {"nElem": nElem, "nNode": nNode, "assembly": info, "patterns": s.incidencePatterns(),
         "assemble_ms": asm, "post_elements_ms": el, "post_nodal_forces_gather_ms": nf, "post_nodal_forces_scatter_ms": nfs,
         "elementFields_wall_s": wall,
         "post_elements_compulsory_bytes": b_el, "post_nodal_forces_gather_compulsory_bytes": b_nf,
         "post_elements_TBps": b_el / (min(el[1:]) * 1e-3) / 1e12, "post_nodal_forces_gather_TBps": b_nf / (min(nf[1:]) * 1e-3) / 1e12}
    out[name] = r
    print(name, json.dumps(r), flush=True)
    s.free()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)

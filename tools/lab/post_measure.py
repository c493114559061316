"""Kernel time of the post-processing passes (pfem_post_elements, pfem_post_nodal_forces, pfem_post_nodal_recovery,
pfem_post_error_indicator) on BASELINE configs 3 and 4 beside the assembly kernel of the same run, with the compulsory bytes of
each pass.  `python tools/lab/post_measure.py [out.json]`."""
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
    rec, ind, recs = [], [], []
    for _ in range(4):                     # the recovery and the indicator (its time includes its own recovery), same run
        s.nodalRecovery(ed, u)
        rec.append(s.recoveryTimings()["recovery_ms"])
        s.errorIndicator(ed, u)
        ind.append(s.recoveryTimings()["indicator_ms"])
    s.setAssemblyMode("scatter")
    for _ in range(3):
        s.nodalForces(ed, H.TIMEDATA, u)
        nfs.append(s.postTimings()["nodal_forces_ms"])
        s.nodalRecovery(ed, u)
        recs.append(s.recoveryTimings()["recovery_ms"])
    s.setAssemblyMode("gather")
    ng = {pf.POISSON_TET: 3, pf.ELAST_TET: 6}[kind]
    nElem, nNode = s.nElem, s.nNode
    info = s.assemblyInfo()
    inc = 4 * nElem
    # compulsory bytes: every array read or written once
    b_el = nElem * 16 + nNode * (3 + ndof) * 8 + nElem * (2 * ng + 1) * 8
    b_nf = inc * 16 + (nNode // 64 + 1) * 8 + nNode * 4 + nNode * (3 + ndof) * 8 + nNode * ndof * 8
    b_rec = inc * 16 + (nNode // 64 + 1) * 8 + nNode * 4 + nNode * (3 + ndof) * 8 + nNode * (ng + 2) * 8
    b_ind = nElem * 16 + nNode * (3 + ndof) * 8 + nNode * ng * 8 + nElem * 8          # the element pass alone
    r = {"nElem": nElem, "nNode": nNode, "assembly": info, "patterns": s.incidencePatterns(),
         "assemble_ms": asm, "post_elements_ms": el, "post_nodal_forces_gather_ms": nf, "post_nodal_forces_scatter_ms": nfs,
         "elementFields_wall_s": wall,
         "post_recovery_gather_ms": rec, "post_recovery_scatter_ms": recs, "post_indicator_with_recovery_ms": ind,
         "post_recovery_gather_compulsory_bytes": b_rec, "post_indicator_pass_compulsory_bytes": b_ind,
         "post_recovery_gather_TBps": b_rec / (min(rec[1:]) * 1e-3) / 1e12,
         "post_recovery_gather_over_forces_gather": min(rec[1:]) / min(nf[1:]),
         "post_indicator_pass_ms": min(ind[1:]) - min(rec[1:]),
         "post_elements_compulsory_bytes": b_el, "post_nodal_forces_gather_compulsory_bytes": b_nf,
         "post_elements_TBps": b_el / (min(el[1:]) * 1e-3) / 1e12, "post_nodal_forces_gather_TBps": b_nf / (min(nf[1:]) * 1e-3) / 1e12}
    out[name] = r
    print(name, json.dumps(r), flush=True)
    s.free()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)

"""What a material map costs (pfem_mesh_set_materials): the assembly kernel's time on BASELINE configs 3 and 4 without a map, with
two layers and with eight materials drawn per element, the step time with -pc_type gamg beside it, and what became of the
SpMV's value dictionary.  Minimum of three warm steps, as post_measure.py takes it.
`python tools/lab/materials_measure.py [out.json]`."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402


def table(kind, n_mat, seed):
    rng = np.random.default_rng(seed)
    if kind == pf.POISSON_TET:
        return rng.uniform(1.0, 10.0, (n_mat, 3))
    return np.column_stack([rng.uniform(100.0, 1000.0, n_mat), rng.uniform(0.15, 0.4, n_mat), np.ones(n_mat),
                            rng.uniform(-0.2, 0.2, (n_mat, 3))])


out = {}
for name, kind, box, bc, ndof, ed, axis in (
        ("config3_poisson_200", pf.POISSON_TET, (-1, 1, 200, -1, 1, 200, -1, 1, 200), 0, 1, H.POISSON_ELEMDATA, 2),
        ("config4_beam_50x300x50", pf.ELAST_TET, (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50), 1, 3, H.ELAST_ELEMDATA, 1)):
    nE = (box[2], box[5], box[8])
    sz = H.box_slab_sizes(*nE, bc, ndof)
    nElem = 6 * nE[0] * nE[1] * nE[2]
    hexa = np.arange(nElem, dtype=np.int64) // 6                  # element 6 h + t of hex h = i + nEx (j + nEy k): pfem_gen_box_tets
    ijk = (hexa % nE[0], (hexa // nE[0]) % nE[1], hexa // (nE[0] * nE[1]))
    res = {}
    for config in ("no_map", "two_layers", "eight_random"):
        s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
        s.generateBoxMesh(kind, *box, bc_mode=bc)
        if config == "no_map":
            tab = ed
        elif config == "two_layers":
            tab = table(kind, 2, 1)
            s.setMaterials((ijk[axis] >= nE[axis] // 2).astype(np.int32), n_mat=2)
        else:
            tab = table(kind, 8, 2)
            s.setMaterials(np.random.default_rng(3).integers(0, 8, nElem).astype(np.int32), n_mat=8)
        s.buildPattern()
        s.setPreconditioner("gamg")
        asm, step, its, reasons, dic = [], [], [], [], []
        for _ in range(4):
            t0 = time.perf_counter()
            s.assemble(tab, H.TIMEDATA)
            a = s.timings()["assemble_ms"]
            i, r, _ = s.factoriseAndSolve()
            step.append((time.perf_counter() - t0) * 1e3)
            asm.append(a); its.append(i); reasons.append(r); dic.append(s.spmvValueDictionary())
        res[config] = {"assemble_ms": asm, "assemble_ms_min_warm": min(asm[1:]), "step_ms": step, "step_ms_min_warm": min(step[1:]),
                       "its": its, "reason": reasons, "value_dictionary_entries": dic, "patterns": s.incidencePatterns(),
                       "assembly": s.assemblyInfo(), "amg_levels": s.amgInfo()["levels"], "amg_aggregation": s.amgAggregation()}
        print(name, config, json.dumps(res[config]), flush=True)
        s.free()
    base = res["no_map"]["assemble_ms_min_warm"]
    for config in ("two_layers", "eight_random"):
        res[config]["assemble_over_no_map"] = res[config]["assemble_ms_min_warm"] / base
        res[config]["step_over_no_map"] = res[config]["step_ms_min_warm"] / res["no_map"]["step_ms_min_warm"]
    out[name] = res
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps({k: {c: {q: v[c][q] for q in v[c] if q.endswith("no_map") or q.endswith("min_warm")} for c in v} for k, v in out.items()}))

"""What an explicit step costs (pfem_dynamics_run): the time of one central-difference step -- the product K u by the SpMV form
in effect plus k_dyn_step -- inside replays of the captured step graph (64 replays of 48 steps = 3072 steps between two HIP
events), on BASELINE config 4 (the 50 x 300 x 50 beam, 2.34 M dof) and the 200^3 Poisson box, beside benchSpmv of the same
handle (code older than the dynamics: a floor that does not depend on it).  One warm-up box, then five boxes each; median and
spread.  `python tools/lab/dynamics_measure.py [out.json]`."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402

BOXES, GRAPHS, SPMV_REPS = 5, 64, 400


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "boxes": v}


out = {}
for name, kind, box, bc, ndof, ed in (
        ("config4_beam_50x300x50", pf.ELAST_TET, (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50), 1, 3, H.ELAST_ELEMDATA),
        ("config3_poisson_200", pf.POISSON_TET, (-1, 1, 200, -1, 1, 200, -1, 1, 200), 0, 1, H.POISSON_ELEMDATA)):
    sz = H.box_slab_sizes(box[2], box[5], box[8], bc, ndof)
    s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    s.generateBoxMesh(kind, *box, bc_mode=bc)
    s.buildPattern()
    s.assemble(ed, H.TIMEDATA)
    total = s.dynamicsSetup(ed, 7.8)
    stable = s.stableDt()
    dt = 0.5 * stable
    s.benchDynamics(dt, GRAPHS)                                   # warm-up box
    s.benchSpmv(SPMV_REPS)
    step = [s.benchDynamics(dt, GRAPHS) for _ in range(BOXES)]
    spmv = [1e3 * s.benchSpmv(SPMV_REPS) for _ in range(BOXES)]
    t, u, v = s.dynamicsState()
    res = {"dof": sz["size_global"], "total_mass": total, "stable_dt": stable, "steps_taken": round(t / dt),
           "max_abs_u": float(abs(u).max()), "step_us": summary(step), "spmv_us": summary(spmv),
           "step_over_spmv": statistics.median(step) / statistics.median(spmv),
           "spmv_form": {"column_bits": s.spmvColumnBits(), "rows_per_lane": s.spmvRowGroup(), "value_dictionary": s.spmvValueDictionary(),
                         "format_bytes": s.spmvFormatBytes()}}
    out[name] = res
    print(name, json.dumps(res), flush=True)
    s.free()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)

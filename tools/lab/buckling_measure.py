"""What the linear buckling analysis costs (pfem_buckling_setup / pfem_buckling_solve), on one MI355X, on
BASELINE config 4 -- the 50 x 300 x 50 beam, 2.34 M dof -- under a unit end compression, n_modes = 6 (MB = 8); events, a
warm-up, five repetitions, median and range (the method of modal_measure.py):

  * the kernel time of pfem_buckling_setup (stress pass, zeroing, k_geo_assemble);
  * microseconds of one launch of k_buck_gram (with k_modal_sum) and k_buck_update against the bytes they move (9 and 9 + 6
    blocks of 8 n MB bytes), and of k_modal_gram / k_modal_update (6 and 6 + 4 blocks) in the same run;
  * wall time per LOBPCG iteration under the point Jacobi of K over a fixed number of iterations and the residual reached, and
    under the cycle of a gamg solve with the iterations to tol 1e-6.

`python tools/lab/buckling_measure.py [out.json] [--small]` (--small: a mesh of a few thousand dofs, to try the script);
the JSON is kept under profiles/buckling/."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402

BOXES, REPS, CAP, MB = 5, 20, 100, 8
small = "--small" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "boxes": list(v)}


name, box = ("small_beam_5x30x5", (-0.5, 0.5, 5, 0.0, 6.0, 30, -0.5, 0.5, 5)) if small else ("config4_beam_50x300x50", (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50))
ed = np.array([H.ELAST_ELEMDATA[0], H.ELAST_ELEMDATA[1], 1.0, 0.0, 0.0, 0.0])
sz = H.box_slab_sizes(box[2], box[5], box[8], 1, 3)
s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
s.generateBoxMesh(pf.ELAST_TET, *box, bc_mode=1)
s.buildPattern()
s.assemble(ed, H.TIMEDATA)
conn, xyz, edof, _ = s.downloadMesh()
top = np.unique(np.concatenate([edof[3 * a + 1][xyz[1][conn[a]] == xyz[1].max()] for a in range(4)]))     # the y dofs of the free end's nodes
top = top[top >= 0].astype(np.int64)
s.addNodalForces(top, np.full(len(top), -1.0 / len(top)))
s.setPreconditioner("gamg")
s.setTolerances(rtol=1e-8, maxits=20000)
its_solve = s.factoriseAndSolve()[0]
n = s.matrixInfo()["n_owned"]
res = {"dof": n, "gamg_solve_iterations": its_solve, "block_bytes": 8 * n * MB}
s.bucklingSetup(ed)
setups = []
for _ in range(BOXES):
    s.bucklingSetup(ed)
    setups.append(s.bucklingSetupMs())
res["setup_kernel_ms"] = summary(setups)
s.benchBucklingKernels(MB, n, REPS)
boxes = [s.benchBucklingKernels(MB, n, REPS) for _ in range(BOXES)]
for key, blocks in (("buck_gram", 9), ("buck_update", 15), ("modal_gram", 6), ("modal_update", 10)):
    us = summary([b[key] for b in boxes])
    res[key] = {"us": us, "bytes": blocks * 8 * n * MB, "TB_per_s": blocks * 8 * n * MB / (us["median"] * 1e-6) / 1e12}
for pc, cap in (("jacobi", CAP), ("gamg", 4 * CAP)):
    s.bucklingSolve(6, tol=1e-6, max_iterations=2, pc=pc, modes=False)           # buffers, warm-up
    walls = []
    for _ in range(3 if pc == "gamg" else BOXES):
        t0 = time.perf_counter()
        r = s.bucklingSolve(6, tol=1e-6, max_iterations=cap, pc=pc, modes=False)
        walls.append(time.perf_counter() - t0)
    res[f"lobpcg_n_modes6_{pc}"] = {"pc": r.pc, "iterations": r.iterations, "reason": r.reason, "restarts": r.restarts,
                                    "largest_residual": float(r.residuals.max()), "theta": r.theta.tolist(), "factors": r.factors.tolist(),
                                    "wall_s": summary(walls), "ms_per_iteration": 1e3 * statistics.median(walls) / max(r.iterations, 1)}
print(name, json.dumps(res), flush=True)
if args:
    json.dump({name: res}, open(args[0], "w"), indent=1)
s.free()

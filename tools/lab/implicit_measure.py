"""What an implicit step costs (pfem_dynamics_run_implicit), on one MI355X; events, one warm-up box, five boxes, median and spread
(the method of dynamics_measure.py):

  * microseconds per iteration of the shifted CG loop (benchImplicit: 200 iterations between two events, no convergence exit)
    on BASELINE config 4 (the 50 x 300 x 50 beam, 2.34 M dof) and on the 200^3 Poisson box, beside -- same handle, same session --
    the solver's own Jacobi loop (solve_ms / iterations of a point-Jacobi solve, which is how bench.py's `jacobi_step` forms its
    ms_per_iteration) and benchSpmv;
  * CG iterations per Newmark step on the beam at dt = 1, 10, 100 and 1000 x the stable step (rtol 1e-5, five steps under the
    constant load from rest);
  * wall time to carry the beam to the same physical time, 1000 x the stable step, explicitly (at 0.9 x the stable step) and by
    Newmark steps of 10, 100 and 1000 x the stable step.

`python tools/lab/implicit_measure.py [out.json] [--small]` (--small: meshes of a few thousand dofs, to try the script)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pfemfort_amd as pf  # noqa: E402
from pfemfort_amd import host as H  # noqa: E402

BOXES, ITERS, SPMV_REPS = 5, 200, 400
small = "--small" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "boxes": v}


def spread(d):
    return (d["max"] - d["min"]) / d["median"]


out = {}
cases = (("config4_beam_50x300x50", pf.ELAST_TET, (-0.5, 0.5, 50, 0.0, 6.0, 300, -0.5, 0.5, 50), 1, 3, H.ELAST_ELEMDATA),
         ("config3_poisson_200", pf.POISSON_TET, (-1, 1, 200, -1, 1, 200, -1, 1, 200), 0, 1, H.POISSON_ELEMDATA))
if small:
    cases = (("small_beam_5x30x5", pf.ELAST_TET, (-0.5, 0.5, 5, 0.0, 6.0, 30, -0.5, 0.5, 5), 1, 3, H.ELAST_ELEMDATA),
             ("small_poisson_20", pf.POISSON_TET, (-1, 1, 20, -1, 1, 20, -1, 1, 20), 0, 1, H.POISSON_ELEMDATA))
for name, kind, box, bc, ndof, ed in cases:
    sz = H.box_slab_sizes(box[2], box[5], box[8], bc, ndof)
    s = pf.PetscSolver().initialise(sz["size_local"], sz["size_global"])
    s.generateBoxMesh(kind, *box, bc_mode=bc)
    s.buildPattern()
    s.assemble(ed, H.TIMEDATA)
    s.dynamicsSetup(ed, 7.8)
    stable = s.stableDt()
    res = {"dof": sz["size_global"], "stable_dt": stable}
    # ---- time per iteration: the shifted loop, the solver's Jacobi loop, the product alone
    dt = 100.0 * stable
    s.benchImplicit(dt, ITERS)                                   # warm-up box
    s.benchSpmv(SPMV_REPS)
    imp = [s.benchImplicit(dt, ITERS) for _ in range(BOXES)]
    spmv = [1e3 * s.benchSpmv(SPMV_REPS) for _ in range(BOXES)]
    s.setPreconditioner("jacobi")
    jac = []
    for k in range(BOXES + 1):                                   # (the first solve warms up)
        its = s.factoriseAndSolve()[0]
        if k:
            jac.append(1e3 * s.timings()["solve_ms"] / max(its, 1))
    res.update({"implicit_iteration_us": summary(imp), "jacobi_iteration_us": summary(jac), "spmv_us": summary(spmv),
                "jacobi_iterations_timed": its})
    res["implicit_over_jacobi"] = res["implicit_iteration_us"]["median"] / res["jacobi_iteration_us"]["median"]
    res["spread"] = {"implicit": spread(res["implicit_iteration_us"]), "jacobi": spread(res["jacobi_iteration_us"])}
    # bytes a row per iteration besides the matrix: the Jacobi loop moves 10 vectors, the shifted loop 13
    # (m twice, p once more in the update)
    fmt = s.spmvFormatBytes()
    n = sz["size_global"]
    res["byte_ratio_expected"] = (fmt - 16 * n + 13 * 8 * n) / (fmt - 16 * n + 10 * 8 * n)
    if kind == pf.ELAST_TET:
        # ---- iterations per step and wall time to a fixed physical time (the beam under its own load, from rest)
        per = {}
        for f in (1, 10, 100, 1000):
            s.setDynamicsState(0.0)
            try:
                _, its = s.implicitRun(f * stable, 5)
                per[str(f)] = its.tolist()
            except pf.PfemError as e:                            # (maxits: say so, go on)
                per[str(f)] = str(e)
        res["iterations_per_step_rtol_1e-5"] = per
        t_end = 1000.0 * stable
        wall = {}
        n_exp = int(round(t_end / (0.9 * stable)))
        s.setDynamicsState(0.0)
        s.dynamicsRun(0.9 * stable, 96)                          # capture, warm up
        s.setDynamicsState(0.0)
        t0 = time.perf_counter()
        s.dynamicsRun(0.9 * stable, n_exp)
        wall["explicit_0.9"] = {"steps": n_exp, "seconds": time.perf_counter() - t0}
        for f in (10, 100, 1000):
            if isinstance(per[str(f)], str):
                continue
            s.setDynamicsState(0.0)
            s.implicitRun(f * stable, 1)                         # capture, warm up
            s.setDynamicsState(0.0)
            t0 = time.perf_counter()
            _, its = s.implicitRun(f * stable, 1000 // f)
            wall[f"newmark_{f}"] = {"steps": 1000 // f, "seconds": time.perf_counter() - t0, "iterations": int(its.sum())}
        res["wall_to_1000_stable_steps"] = wall
    out[name] = res
    print(name, json.dumps(res), flush=True)
    s.free()
if args:
    json.dump(out, open(args[0], "w"), indent=1)

#!/usr/bin/env python3
"""bench.py -- DOF/s (assembly + CG-to-tolerance) of the implicit-FEM hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over the resident mesh: setZero + element loop
(Ke/Fe, Dirichlet lifting, scatter; the reference's timer tetrapoissonparallelimpl1.F:826->893)
+ factoriseAndSolve (Jacobi-PCG to the PETSc default rtol 1e-5; timer :898->902).
Inputs (mesh, maps, pattern) are resident in HBM before the timed region, as in the reference
where mesh read / numbering / pattern precede the timers.  The synthetic mesh and its numbering are
generated ON THE DEVICE (pfem_mesh_generate_box_axis: genTetra.cpp's box + the driver's bookkeeping,
bit-identical to the host path); a rank holds the node planes of its own hex layers only.

N = 1 : BASELINE.json configs[2]: synthetic [-1,1]^3, 200x200x200x6 P1 tets (genTetra logic).
N > 1 : one process per GPU.  Started either by a launcher (python -m torch.distributed.run --nproc-per-node N bench.py
        --gpus N ..., RANK / LOCAL_RANK / WORLD_SIZE in the environment) or plainly as `python bench.py --gpus N`: the
        parent then starts the N ranks itself, before it has touched the GPU, relays their one JSON line and returns
        their exit code.  Weak scaling, per-GPU element count fixed: the [-1,1]^3 cube with round(200 N^(1/3)) cells per
        side (N = 8: BASELINE configs[4], 400x400x400x6), cut into N slabs of hex layers along its longest axis (cubes:
        z; the beam of --workload beam: across its length, y).  Per CG iteration: SpMV, the neighbour exchange of the
        partial sums (RCCL grouped send/recv, bound in C++, in order on the compute stream; exchanges of 4 MiB and more
        run the slices with shared rows first and put the exchange on a second stream under the interior slices -- the
        form is voted by all ranks) and two scalar all-reduces.  The Jacobi-PCG iteration count about doubles from N=1
        to N=8 (a property of the preconditioner), which caps weak DOF/s scaling at ~0.5 N independently of the
        hardware, so the line also carries (a) `per_iteration_efficiency`: rows per GPU and per millisecond of CG
        iteration against the committed N=1 figure, and (b) `strong_cfg5`: BASELINE config 5 (400^3 x 6 tets, which fits
        one MI355X: 2.02 s per step, profiles/r02/bench_cfg5_400cube_single_gpu.json) solved by the same N ranks, with
        its speed-up over that single-GPU step -- the >= 6x-at-8-GPUs evidence.  `comm` says what carried the run:
        transport, ncclCommCount, every rank's device, the fallback reason if gloo host hooks had to be taken.
        --strong keeps the whole problem at --cells per side instead; --stack grows the box along z.

Prints ONE JSON line on rank 0 (contract in the task description).  A plain run sets up, warms up, times the --steps
steps and prints the headline (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, iterations, setup).
--full adds everything that takes measurements or runs of its own: `roofline` for the CG SpMV kernel (raw HIP event
pairs around sampled SpMV launches of the timed solves, HBM traffic from two child runs under rocprofv3 --pmc),
`cpu_baseline` (the C oracle on the host cores, timed at the reference's three timer points on the SAME configuration),
the point-Jacobi companion, the step at the parity tolerance, the check of the answer, and for N > 1 the strong-scaling
companion, the link latencies and the peer-transport A/B.
--dump-outputs DIR writes what the last timed step computed (one GPU) as DIR/<name>.npy, float64.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def pmc_traffic(nnz, value_dict=False):
    """HBM bytes per launch of the CG SpMV from the committed rocprofv3 PMC passes
    (profiles/spmv_pmc_traffic.json, written by tools/r05/collect_final.py from the passes of tools/r05/final.sh on the SAME workload in a
    builder lease, not in this run): (2*FETCH_SIZE + WRITE_SIZE)*1024, FETCH_SIZE doubled per
    MI355X_MICROARCH.md section HBM.  Returns (bytes, source) or (None, None)."""
    path = os.path.join(ROOT, "profiles", "spmv_pmc_traffic.json")
    try:
        doc = json.load(open(path))
        for d in doc.get("entries", [doc]):          # one entry per workload (keyed by the matrix's nnz)
            if d.get("nnz") == nnz and bool(d.get("value_dictionary", False)) == bool(value_dict):      # (the dictionary form is another kernel)
                return (2.0 * d["FETCH_SIZE_KB"] + d["WRITE_SIZE_KB"]) * 1024.0, \
                    "profiles/spmv_pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, " \
                    f"{d.get('source', 'builder lease')}); replayed, NOT measured in this run"
    except (OSError, ValueError, KeyError):
        pass
    return None, None


def kernel_trace_figures(nnz, value_dict=False):
    """rocprofv3 --kernel-trace averages of the CG SpMV committed next to the PMC figures (same file, same caveat: a
    builder lease, replayed here for comparison with this run's event pairs), or None."""
    try:
        doc = json.load(open(os.path.join(ROOT, "profiles", "spmv_pmc_traffic.json")))
        for d in doc.get("entries", [doc]):
            if d.get("nnz") == nnz and bool(d.get("value_dictionary", False)) == bool(value_dict):
                return d.get("kernel_trace_avg_us")
    except (OSError, ValueError, KeyError):
        pass
    return None


def pmc_traffic_live(argv, timeout_s=240.0):
    """HBM traffic of the CG SpMV measured IN THIS RUN: before this process touches the GPU, two child runs of the same command
    (one step, no companions) under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` -- separate passes, the counters do not fit
    one (MI355X_MICROARCH.md, rocprofv3 PMC slots) --, kernel filter on the SpMV family.  Returns a dict
    {kernel name: {"FETCH_SIZE_KB", "WRITE_SIZE_KB", "dispatches"}} for the kernels of the WITH_DOT = true family (the CG's own
    product), or a string saying why not.  The program after `--` is python3 itself (never a shell or env hop)."""
    import csv
    import glob
    import shutil
    import signal
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not exe:
        return "rocprofv3 is not on this box"
    if any(k.startswith("ROCPROF") or k.startswith("ROCP_") for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return "this process runs under a profiler already"
    child = drop_option(argv, "--dump-outputs") + ["--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-parity-step", "--no-jacobi-step", "--no-pmc"]
    out = {}
    env = dict(os.environ, TMPDIR="/tmp")
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="pfem_pmc_", dir="/tmp")
        cmd = [exe, "--pmc", counter, "--kernel-include-regex", "k_spmv", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__)] + child
        try:
            pr = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = pr.wait(timeout=timeout_s / 2)
            except subprocess.TimeoutExpired:
                os.killpg(pr.pid, signal.SIGKILL)
                pr.wait()
                shutil.rmtree(d, ignore_errors=True)
                return f"the {counter} pass did not finish in {timeout_s / 2:g} s"
            if rc != 0:
                shutil.rmtree(d, ignore_errors=True)
                return f"the {counter} pass ended with code {rc}"
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r.get("Counter_Name") != counter or "<true" not in r.get("Kernel_Name", ""):
                        continue
                    e = out.setdefault(r["Kernel_Name"].replace("void ", "").split("(")[0], {})
                    e[counter + "_sum"] = e.get(counter + "_sum", 0.0) + float(r["Counter_Value"])
                    e[counter + "_n"] = e.get(counter + "_n", 0) + 1
        except (OSError, ValueError, KeyError) as e:
            shutil.rmtree(d, ignore_errors=True)
            return f"{type(e).__name__}: {e}"
        shutil.rmtree(d, ignore_errors=True)
    res = {}
    for k, e in out.items():
        if e.get("FETCH_SIZE_n") and e.get("WRITE_SIZE_n"):
            res[k] = {"FETCH_SIZE_KB": e["FETCH_SIZE_sum"] / e["FETCH_SIZE_n"], "WRITE_SIZE_KB": e["WRITE_SIZE_sum"] / e["WRITE_SIZE_n"],
                      "dispatches": e["FETCH_SIZE_n"]}
    return res or "the passes recorded no dispatch of a k_spmv*<true, ...> kernel"


def cpu_baseline(n, rtol, extra_sample=True):
    """The oracle (C restatement of the reference path) on the host cores, on the SAME configuration as the GPU
    number (n^3 x 6 tets, same rtol), timed at the reference's three timer points (tetrapoissonparallelimpl1.F:826,
    893, 898-902): assembly, solve, total.  Threads: OpenMP over the element loop (atomic ADD_VALUES) and over
    SpMV / dots / axpys -- the shared-memory stand-in for the reference's `mpirun -np P` (PETSc is not installable
    here: "reference-equivalent CPU path, not PETSc").  The 1-thread figures come from the 100^3 sample (configs[1])
    so that the whole leg stays bounded."""
    from oracle import pfem_oracle as O
    cores = max(1, min(os.cpu_count() or 1, 64, cpu_quota() or 1 << 30))

    def problem(m):
        mesh = O.gen_box_tets(-1, 1, m, -1, 1, m, -1, 1, m)
        dm = O.dof_numbering(mesh.nNode, 1, mesh.bc_node, mesh.bc_dof, mesh.bc_val)
        edof = O.elem_dof_array(mesh.conn, dm.NodeDofArrayNew)
        O.set_threads(cores)
        rowptr, cols = O.csr_pattern(edof, dm.size_global)          # pattern precedes the timers (:786-802)
        return mesh, dm, edof, rowptr, cols

    def run(prob, threads):
        mesh, dm, edof, rowptr, cols = prob
        O.set_threads(threads)
        t0 = time.perf_counter()
        asm = O.assemble if threads == 1 else O.assemble_mt
        vals, rhs = asm(O.POISSON_TET, mesh.xyz, mesh.conn, edof, dm.solnApplied, O.POISSON_ELEMDATA, dm.size_global, rowptr, cols)
        t1 = time.perf_counter()
        x, its, reason, rn, _ = O.pcg_jacobi(rowptr, cols, vals, rhs, rtol=rtol)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, its

    t_setup = time.perf_counter()
    prob = problem(n)
    t_setup = time.perf_counter() - t_setup
    N = prob[1].size_global
    nb = 12 * len(prob[4]) + 20 * N
    run(prob, cores)                                             # first touch / thread pool warm-up
    am, sm, its = run(prob, cores)
    O.set_threads(cores)
    triad = O.stream_triad_gbps()
    out = {"value": N / (am + sm), "unit": "DOF/s", "cores": cores, "kind": "port",
           "preconditioner": "point Jacobi (the GPU's jacobi_step is the like-for-like figure; `value` runs -pc_type gamg)",
           "host_stream_triad_gbps": triad,
           "sample": f"{n}^3x6 tet Poisson (the GPU number's own configuration), N={N}: {cores} OpenMP threads: assembly "
                     f"{am:.2f}s + Jacobi-PCG rtol {rtol:g} {its} its {sm:.2f}s = {am + sm:.2f}s "
                     f"({nb * its / sm / 1e9:.0f} GB/s SpMV-equivalent; the host's STREAM triad with the same threads: {triad:.0f} GB/s); "
                     "reference-equivalent CPU path (C restatement), not PETSc",
           "assembly_s": am, "solve_s": sm, "total_s": am + sm, "its": its, "setup_s_untimed": t_setup}
    del prob
    mpi = cpu_baseline_mpi(n, rtol)
    if mpi:
        # "MPI, one rank per core, if MPI exists on the box" -- the reference's own way of using a node.  The
        # OpenMP figure above stays in the line; `value` is the better of the two.
        out["mpi_one_rank_per_core"] = mpi
        out["openmp_port"] = {k: out[k] for k in ("value", "cores", "assembly_s", "solve_s", "total_s", "its")}
        if mpi["value"] > out["value"]:
            out.update(value=mpi["value"], cores=mpi["ranks"], assembly_s=mpi["assembly_s"], solve_s=mpi["solve_s"], total_s=mpi["total_s"], its=mpi["iterations"],
                       sample=f"{n}^3x6 tet Poisson (the GPU number's own configuration), N={N}: mpiexec -n {mpi['ranks']} oracle/pfem_oracle_mpi (one rank per "
                              f"core, slabs of node planes, the oracle's element routine, distributed CSR Jacobi-PCG rtol {rtol:g}): assembly {mpi['assembly_s']:.2f}s + "
                              f"{mpi['iterations']} its {mpi['solve_s']:.2f}s = {mpi['total_s']:.2f}s ({nb * mpi['iterations'] / mpi['solve_s'] / 1e9:.0f} GB/s "
                              f"SpMV-equivalent; the host's STREAM triad: {triad:.0f} GB/s); {cores} OpenMP threads on the same configuration: "
                              f"{am + sm:.2f}s; reference-equivalent CPU path (C restatement), not PETSc")
    if extra_sample:
        p1 = problem(100)
        a1, s1, i1 = run(p1, 1)
        run(p1, cores)
        ac, sc, ic = run(p1, cores)
        N1 = p1[1].size_global
        out["extra"] = {"sample": "100^3x6 tet Poisson (BASELINE configs[1])", "free_dofs": N1,
                        "single_core": {"assembly_s": a1, "solve_s": s1, "its": i1, "value": N1 / (a1 + s1)},
                        f"{cores}_threads": {"assembly_s": ac, "solve_s": sc, "its": ic, "value": N1 / (ac + sc)}}
    return out


def cpu_quota():
    """CPUs' worth of time the container may use (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited / unreadable:
    a GPU box of this pool shows 256 hardware threads and grants 16 -- more runnable threads than that are throttled."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            return max(1, int(float(q) / float(per)))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return max(1, q // per)
    except (OSError, ValueError):
        pass
    return None


def physical_cores():
    """Distinct (socket, core) pairs of /proc/cpuinfo (hardware threads do not count); half of os.cpu_count() if unreadable."""
    try:
        pairs, phys = set(), None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                phys = ln.split(":")[1].strip()
            elif ln.startswith("core id"):
                pairs.add((phys, ln.split(":")[1].strip()))
        if pairs:
            return len(pairs)
    except OSError:
        pass
    return max(1, (os.cpu_count() or 2) // 2)


def cpu_baseline_mpi(n, rtol):
    """The reference's `mpirun -np P` restated (oracle/pfem_oracle_mpi.c), one rank per physical core, on the GPU number's own
    configuration; None where no MPI is installed or the program was not built (`make -C oracle mpi`)."""
    import shutil
    import subprocess
    exe = os.path.join(ROOT, "oracle", "pfem_oracle_mpi")
    launcher = next((c for c in ("/opt/conda/bin/mpiexec", shutil.which("mpiexec")) if c and os.path.exists(c)), None)
    if not launcher or not os.path.exists(exe):
        return None
    ranks = max(1, min(physical_cores(), n - 1, len(os.sched_getaffinity(0)), cpu_quota() or 1 << 30))
    env = dict(os.environ, OMP_NUM_THREADS="1")
    # (measured on a GPU box of this pool, 16 ranks = its CPU quota, 200^3: -bind-to numa 1.9 s solve, unbound 2.5 s,
    # -bind-to core -- which packs the ranks onto neighbouring cores of one socket -- 5.6 s)
    for bind in (["-bind-to", "numa"], []):
        try:
            r = subprocess.run([launcher, "-n", str(ranks)] + bind + [exe, str(n), repr(rtol), "10000", "2"], capture_output=True, text=True, timeout=600, env=env)
        except (OSError, subprocess.TimeoutExpired):
            return None
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode == 0 and lines:
            d = json.loads(lines[-1])
            d.update(value=d["free_dofs"] / d["total_s"], unit="DOF/s", binding=" ".join(bind) or "none",
                     what="mpiexec -n %d oracle/pfem_oracle_mpi %d: second of two repeats, maximum over the ranks" % (ranks, n))
            return d
    return None


def self_launch(args):
    """Parent of an N > 1 run started as `python bench.py --gpus N ...` (the form the driver uses for N = 1): starts
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py <same
    arguments>` as a CHILD process (never an exec: this process stays a plain waiter and never touches the GPU), passes
    the children's stdout and stderr through, and returns their exit code.  A watchdog kills the whole process group if
    the ranks' own faulthandler timeout did not end them.  If the RCCL attempt ends without a result line (a rank died or
    timed out in the bring-up), the job is started ONCE more, in fresh processes, over gloo host hooks -- slow, but a
    number, and the line says why (`comm.fallback_reason`)."""
    import signal
    import socket
    import subprocess
    import threading
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: what RCCL needs on this host driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))

    def attempt(extra):
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:] + extra
        proc = subprocess.Popen(cmd, env=env, cwd=ROOT, start_new_session=True, stdout=subprocess.PIPE, text=True)
        got_line = []

        def relay():
            for ln in proc.stdout:
                if ln.lstrip().startswith("{"):
                    got_line.append(True)
                sys.stdout.write(ln)
                sys.stdout.flush()
        th = threading.Thread(target=relay, daemon=True)
        th.start()
        try:
            rc = proc.wait(timeout=args.rank_timeout + 120.0)
        except subprocess.TimeoutExpired:
            print(f"bench.py: the {args.gpus} ranks did not finish within {args.rank_timeout + 120:.0f} s: killing them", file=sys.stderr)
            rc = 124
        except KeyboardInterrupt:
            rc = 130
        if proc.poll() is None:
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
            proc.wait()
        th.join(timeout=10.0)
        return rc, bool(got_line)

    rc, ok = attempt([])
    if rc not in (0, 130) and not ok and args.backend == "nccl" and not args.no_relaunch:
        print(f"bench.py: the RCCL attempt ended with exit code {rc} and no result line; starting the ranks once more over "
              "gloo host hooks", file=sys.stderr)
        rc, ok = attempt(["--backend", "gloo", "--fallback-note", f"a first attempt over RCCL ended with exit code {rc} and no result"])
    return rc


def transport_ab_child(args):
    """The peer-transport companion of an N > 1 line as a fresh job: `python -m torch.distributed.run ... bench.py <same arguments>
    --ab-child` started as a CHILD of rank 0 (which has finished its own work and left its process group), in its own session.
    Returns the child's brief line, or {"skipped": why}.  A child that does not come back within --transport-ab-timeout is
    killed by process group; the caller is never inside a hung kernel itself."""
    import signal
    import socket
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "GROUP_WORLD_SIZE", "ROLE_RANK", "ROLE_WORLD_SIZE",
                        "ROLE_NAME", "MASTER_ADDR", "MASTER_PORT") and not k.startswith("TORCHELASTIC_")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:] + ["--ab-child", "--no-transport-ab"]
    try:
        proc = subprocess.Popen(cmd, env=env, cwd=ROOT, start_new_session=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    except OSError as e:
        return {"skipped": f"the companion job could not be started: {e}"}
    try:
        so, _ = proc.communicate(timeout=args.transport_ab_timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        proc.wait()
        return {"skipped": f"the companion job did not come back within {args.transport_ab_timeout:g} s (its process group was killed)"}
    lines = [ln for ln in (so or "").splitlines() if ln.lstrip().startswith("{")]
    if proc.returncode != 0 or not lines:
        return {"skipped": f"the companion job ended with exit code {proc.returncode} and {'no' if not lines else 'a'} result line"}
    try:
        return json.loads(lines[-1])
    except ValueError as e:
        return {"skipped": f"unreadable result line of the companion job: {e}"}


def drop_option(argv, name):
    """argv without `name VALUE` / `name=VALUE`."""
    out, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a == name:
            skip = True
        elif not a.startswith(name + "="):
            out.append(a)
    return out


def dump_outputs(solver, its, reason, rnorm, out_dir):
    """--dump-outputs: what the last timed step handed its caller -- the solution, the assembled right-hand side and
    matrix values, and the solve's (iterations, converged reason, residual norm) -- as float64 .npy files.  An array longer
    than its cap is replaced by its entries at indices drawn from a fixed seed (the same for every build), so that two
    builds compare entry for entry; the caps keep the files under 56 MB in all."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)

    def put(name, a, cap):
        a = np.asarray(a, dtype=np.float64)
        if a.size > cap:
            a = a[np.sort(np.random.default_rng(20240611).integers(0, a.size, cap))]
        np.save(os.path.join(out_dir, name + ".npy"), a)
    put("solution", solver.getSolution(), 4_000_000)
    put("rhs", solver.getRHS(), 1_000_000)
    put("matrix_values", solver.getCSR()[2], 2_000_000)
    put("solve", [its, reason, rnorm], 3)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5, help="timed steps")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps before them")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: roofline (with the PMC child runs), CPU baseline, point-Jacobi companion, parity-"
                         "tolerance step, check of the answer; N>1: strong-scaling companion, link latencies, peer-transport A/B")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="one GPU: write what the last timed step computed as DIR/<name>.npy (float64; long arrays as a fixed, seeded sample)")
    ap.add_argument("--cells", dest="n", type=int, default=200, help="cells per side of one rank's block")
    ap.add_argument("--rtol", type=float, default=1e-5, help="PETSc default (the reference sets none)")
    ap.add_argument("--workload", choices=["poisson", "beam"], default="poisson",
                    help="poisson: BASELINE configs[2] (the headline metric); beam: configs[3], the 50x300x50x6-tet "
                         "linear-elasticity cantilever (fixed size: strong scaling for N>1, cut across its length)")
    ap.add_argument("--beam-scale", type=int, default=1,
                    help="beam workload: cells per direction multiplied by this (2: 100x600x100, 36.4 M dofs -- beyond literal 16-bit column gaps)")
    ap.add_argument("--axis", type=int, default=-1, choices=[-1, 0, 1, 2],
                    help="N>1: axis the box is cut along (0 x, 1 y, 2 z; -1: the one with the most hex layers, ties to z -- the "
                         "beam is cut across y, cubes across z)")
    ap.add_argument("--strong", action="store_true",
                    help="N>1: keep the WHOLE problem at --cells per side (strong scaling; e.g. --cells 400 = BASELINE config 5 on N ranks)")
    ap.add_argument("--stack", action="store_true", help="N>1: z-extended box n x n x (n N) instead of the cube of n N^(1/3) cells per side")
    ap.add_argument("--no-strong-block", action="store_true",
                    help="N>1 weak runs: skip the extra strong-scaling measurement (the cube of 2 x --cells per side -- BASELINE "
                         "config 5 at the default 200 -- on the same N ranks) reported as `strong_cfg5`")
    ap.add_argument("--numbering", choices=["lattice", "rcb8", "shuffle"], default="lattice",
                    help="N=1: node numbering of the SAME mesh.  lattice: genTetra's own (line by line; the generator runs on the "
                         "device); rcb8: the reference's renumbering for 8 ranks (tetrapoissonparallelimpl1.F:500-679: parts "
                         "concatenated) of a recursive-coordinate-bisection partition, solved on one rank; shuffle: a random "
                         "permutation of the node ids -- the worst case of an unstructured mesh file.  Mesh built on the host and "
                         "uploaded (untimed)")
    ap.add_argument("--mode", choices=["batched", "compat"], default="batched",
                    help="compat: the UNCHANGED driver's own path instead of the batched one -- a Fortran host program (tests/native/"
                         "boundary_check.F90, the build's counterpart of tetrapoissonparallelimpl1.F:786-905) loops over the elements "
                         "on the host: element routine, MatSetValues(INSERT_VALUES) pass, setZero, MatSetValues / VecSetValues(ADD_VALUES), "
                         "then the GPU solves.  One process, one GPU; prints its own JSON line (not the driver's contract line)")
    ap.add_argument("--jitter", type=float, default=0.0,
                    help="move every node that carries no Dirichlet value by up to this fraction of the cell size (host-generated mesh, "
                         "uploaded): the coordinates no longer form a lattice, so -pc_type gamg takes the path any unstructured file "
                         "mesh takes -- matching on the strength graph along a Morton curve instead of bricks.  One rank")
    ap.add_argument("--no-transport-ab", action="store_true", help="N>1: skip the companion run over the peer-memory transport")
    ap.add_argument("--transport-ab-timeout", type=float, default=240.0,
                    help="N>1: seconds the peer-transport companion may take before the line is printed without it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true",
                    help="N=1: do not measure the SpMV's HBM traffic in this run (two short child runs under rocprofv3 --pmc before this "
                         "process touches the GPU); `roofline.traffic` then comes from the committed passes of the same workload")
    ap.add_argument("--no-parity-step", action="store_true", help="skip the extra (untimed) step at rtol 1e-10")
    ap.add_argument("--cycle", choices=["auto", "v", "w"], default="auto", help="-pc_mg_cycle_type of the gamg cycle (auto = the library's default: v)")
    ap.add_argument("--pc", choices=["jacobi", "pbjacobi", "gamg"], default="gamg",
                    help="preconditioner of the CG (PCSetType, solverpetsc.F:206; the reference: PCBJACOBI/ILU(0)).  gamg (default): "
                         "plain-aggregation multigrid V-cycle, on several ranks ONE hierarchy across the ranks ("
                         "PFEM_AMG_COUPLED=0: block Jacobi over the ranks with one hierarchy per rank); jacobi: the diagonal (north_star's baseline preconditioner; always measured too and reported as "
                         "`jacobi_step`); pbjacobi: node-block Jacobi")
    ap.add_argument("--no-jacobi-step", action="store_true", help="skip the extra point-Jacobi measurement reported as `jacobi_step`")
    ap.add_argument("--single-reduction", action="store_true",
                    help="KSPCGUseSingleReduction: one all-reduce per CG iteration instead of two (PETSc's opt-in form; off by default)")
    ap.add_argument("--backend", default="nccl", help="nccl: RCCL bound inside the library; gloo: host hooks (development)")
    ap.add_argument("--simulate-rccl-failure", action="store_true", help="development: exercise the fallback to gloo host hooks")
    ap.add_argument("--same-device", action="store_true",
                    help="development: put every rank on cuda:0 (with --backend gloo) to exercise the N>1 path on a 1-GPU box")
    ap.add_argument("--no-relaunch", action="store_true", help="self-launched N>1 runs: do not retry over gloo when the RCCL attempt dies")
    ap.add_argument("--fallback-note", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)       # this job is the peer-transport companion of another job's line
    ap.add_argument("--debug-die-rank", type=int, default=-1, help=argparse.SUPPRESS)     # tests: this rank exits(3) after the rendezvous
    ap.add_argument("--bringup-timeout", type=float, default=420.0,
                    help="seconds the communicator bring-up + transport self-test of an N>1 run may take before the rank gives up")
    ap.add_argument("--rank-timeout", type=float, default=1500.0,
                    help="seconds after which a rank that is still running dumps every thread's traceback and exits non-zero "
                         "(a hung collective must not hang the job)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.gpus != 1 or args.mode != "batched"):
        ap.error("--dump-outputs needs --gpus 1 and --mode batched")
    return args


def single_gpu_reference():
    """Committed single-GPU figures the N > 1 line is read against (profiles/single_gpu_reference.json: which driver /
    builder record each one comes from is named there)."""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "single_gpu_reference.json")))
    except (OSError, ValueError):
        return {}


class Job:
    """What every case of this process shares: the rank's place in the job, the modules, and the transport verdict."""

    def __init__(self, args):
        self.args = args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.device_index = self.local_rank if (self.world > 1 and not args.same_device) else 0
        self.dist = self.torch = None
        self.gloo_group = None          # host-hook group once RCCL was found unusable (or the default group is gloo)
        self.fallback_reason = args.fallback_note
        self.rccl_dead = False


def run_case(J, beam, nE, ext, steps, warmup, rtol, profile=True, parity_step=False, pc=None, transport=None, probe_comm=False,
             dump_dir=None):
    """One configuration through the whole hot path on this job's ranks: device-generated slab, transport, pattern,
    `warmup` + `steps` steps (assembly + solve) bracketed by barriers; returns everything the JSON line needs.  The
    second pattern build and the check of the answer are made under --full only."""
    import faulthandler

    import numpy as np
    import pfemfort_amd as pf
    from pfemfort_amd import host as H
    args, world, rank, dist, torch = J.args, J.world, J.rank, J.dist, J.torch
    kind = pf.ELAST_TET if beam else pf.POISSON_TET
    ndof = 3 if beam else 1
    bc_mode = 1 if beam else 0
    elem_data = H.ELAST_ELEMDATA if beam else H.POISSON_ELEMDATA
    nEx, nEy, nEz = nE
    box = (ext[0], ext[1], nEx, ext[2], ext[3], nEy, ext[4], ext[5], nEz)
    R = {"nE": nE, "ext": ext, "beam": beam, "steps": steps, "warmup": warmup, "rtol": rtol}

    t_setup = time.perf_counter()
    sz = H.box_slab_sizes(nEx, nEy, nEz, bc_mode, ndof, world, rank, axis=args.axis)
    axis = sz["axis"]
    N, row_start, size_local = sz["size_global"], sz["row_start"], sz["size_local"]
    solver = pf.PetscSolver().initialise(size_local, N, row_start=row_start, device=J.device_index)
    solver.setTolerances(rtol=rtol, maxits=100000 if beam else 10000)
    pc = pc or args.pc
    solver.setPreconditioner(pc)
    if args.cycle != "auto":
        solver.setAmgCycle(args.cycle)
    if args.single_reduction:
        solver.setSingleReduction(True)
    dm_host = mesh_host = None
    if (args.numbering == "lattice" and args.jitter <= 0.0) or world > 1:
        solver.generateBoxMesh(kind, *box, bc_mode=bc_mode, nparts=world, part=rank, axis=axis)
    else:
        # the same mesh under another node numbering: host generator, renumbering, upload (all untimed setup)
        mesh_host = H.gen_box_tets(*box, bc_mode=bc_mode, ndof=ndof)
        if args.jitter > 0.0:
            # nodes without a Dirichlet value move inside a ball of radius jitter * (smallest cell edge): Kuhn's tetrahedra keep
            # their orientation up to 0.28 (half their smallest altitude h / sqrt 3), the boundary values stay those of the lattice
            hmin = min((ext[1] - ext[0]) / nEx, (ext[3] - ext[2]) / nEy, (ext[5] - ext[4]) / nEz)
            rng = np.random.default_rng(7)
            d = rng.uniform(-1.0, 1.0, size=mesh_host.xyz.shape) * (args.jitter * hmin / np.sqrt(3.0))
            d[:, np.unique(mesh_host.bc_node)] = 0.0
            mesh_host = H.Mesh(mesh_host.xyz + d, mesh_host.conn, mesh_host.bc_node, mesh_host.bc_dof, mesh_host.bc_val, box=mesh_host.box)
        if args.numbering == "lattice":
            dm_host = H.dof_numbering(mesh_host.nNode, ndof, mesh_host.bc_node, mesh_host.bc_dof, mesh_host.bc_val)
        elif args.numbering == "shuffle":
            perm = np.random.default_rng(2024).permutation(mesh_host.nNode).astype(np.int32)      # old id -> shuffled id
            xyz = np.empty_like(mesh_host.xyz)
            xyz[:, perm] = mesh_host.xyz
            mesh_host = H.Mesh(xyz, perm[mesh_host.conn], perm[mesh_host.bc_node], mesh_host.bc_dof, mesh_host.bc_val, box=mesh_host.box)
            dm_host = H.dof_numbering(mesh_host.nNode, ndof, mesh_host.bc_node, mesh_host.bc_dof, mesh_host.bc_val)
        else:
            _, npid = H.partition_rcb(mesh_host, 8)
            dm_host = H.dof_numbering(mesh_host.nNode, ndof, mesh_host.bc_node, mesh_host.bc_dof, mesh_host.bc_val, 8, npid)
        conn_new, xyz_new = H.renumber_mesh(mesh_host, dm_host)
        edof = H.elem_dof_array(conn_new, dm_host.NodeDofArrayNew)
        solver.uploadMesh(kind, conn_new, xyz_new, edof, dm_host.solnApplied)
        R["xyz_free"] = xyz_new[:, H.assy_for_soln(dm_host.NodeDofArrayNew) // ndof]
        del conn_new, edof
    R["t_generate"] = time.perf_counter() - t_setup
    hooks = None
    if world > 1:
        from pfemfort_amd import distributed as PD
        # RCCL inside the library unless the group is gloo.  If RCCL cannot be brought up or fails the transport self-test
        # on ANY rank, all ranks fall back together to host hooks over a gloo subgroup: slow, but a result.
        why = None
        if transport == "peer":
            # the A/B companion of an N > 1 line: the same steps over the peer-memory transport (device-side boxes + flags mapped
            # through hipIpc*, bring-up over gloo hooks).  Any rank's failure -- bring-up or self-test -- is everybody's: the case
            # is skipped with the reason, together
            if J.gloo_group is None and args.backend != "gloo":
                J.gloo_group = dist.new_group(backend="gloo")
            try:
                hooks = PD.attach(solver, dist, torch, staged=True, group=J.gloo_group, peer=True)
                bad = solver.commSelftest(4096)
                why = f"self-test: {bad} wrong entries" if bad else None
            except pf.PfemError as e:
                why = str(e)
            votes = [None] * world
            dist.all_gather_object(votes, why)
            why = next((v for v in votes if v), None)
            if why:
                solver.free(collective=False)
                return {"skipped": f"peer-memory transport not usable here: {why}"}
        elif (args.backend != "gloo" and not J.rccl_dead) or (args.simulate_rccl_failure and not J.rccl_dead):
            try:
                if args.simulate_rccl_failure:
                    raise pf.PfemError(9, "simulated", "--simulate-rccl-failure")
                hooks = PD.attach(solver, dist, torch, staged=False)
                bad = solver.commSelftest(4096)
                why = f"self-test: {bad} wrong entries" if bad else None
            except pf.PfemError as e:
                why = str(e)
            votes = [None] * world
            dist.all_gather_object(votes, why)
            why = next((v for v in votes if v), None)
            if why:
                J.rccl_dead = True
                J.fallback_reason = f"RCCL was not usable: {why}"
        if transport != "peer" and (args.backend == "gloo" or J.rccl_dead):
            if J.gloo_group is None and args.backend != "gloo":
                J.gloo_group = dist.new_group(backend="gloo")
            hooks = PD.attach(solver, dist, torch, staged=True, group=J.gloo_group)
            bad = solver.commSelftest(4096)
            if bad:
                raise SystemExit(f"rank {rank}: communication self-test failed ({bad} wrong entries)")
        faulthandler.dump_traceback_later(args.rank_timeout, exit=True)        # bring-up done: the full leash
        # what is carrying the run, from the transport itself (ncclCommCount etc.), one entry per rank
        me = solver.commDescribe()
        try:
            pr = torch.cuda.get_device_properties(J.device_index)
            me["device_name"] = pr.name
            me["device_uuid"] = str(getattr(pr, "uuid", "")) or None
            me["pci_bus_id"] = getattr(pr, "pci_bus_id", None)
        except Exception:           # noqa: BLE001 -- reporting only
            pass
        me.update(rank=rank, local_rank=J.local_rank, device_index=J.device_index, pid=os.getpid(),
                  layers=[sz["layer0"], sz["layer1"]], size_local=size_local)
        R["ranks_report"] = [None] * world
        dist.all_gather_object(R["ranks_report"], me)
    t1 = time.perf_counter()
    solver.buildPattern()
    R["t_pattern"] = time.perf_counter() - t1
    info = solver.matrixInfo()
    R["t_setup"] = time.perf_counter() - t_setup
    # the first build also pays for the first multi-GB device allocations of the process (0.05 - 1 s from box to box);
    # a second build of the same pattern shows the symbolic phase itself
    R["t_pattern2"] = None
    if args.full:
        t1 = time.perf_counter()
        solver.buildPattern()
        R["t_pattern2"] = time.perf_counter() - t1
    if profile:      # event pair around every 8th (gamg: every 2nd) SpMV launch of the CG loop of the timed solves (a pair costs ~2 us)
        solver.profileSpmv(2 if pc == "gamg" else 8)

    def step():
        solver.assemble(elem_data, H.TIMEDATA)
        return solver.factoriseAndSolve()

    def sync():
        if world > 1:
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()

    R["first_step_ms"] = None
    for k in range(warmup):
        t1 = time.perf_counter()
        step()
        if k == 0:        # the first step after a pattern build also pays for the preconditioner's symbolic set-up (gamg: aggregates,
            R["first_step_ms"] = (time.perf_counter() - t1) * 1e3      # coarse patterns, Galerkin maps) and for first-touch allocations
    sync()
    acc = dict(spmv_ms=0.0, spmv_n=0, asm_ms=0.0, sol_ms=0.0, if_ms=0.0, sc_ms=0.0, ex_ms=0.0, comm_n=0, enq_ms=0.0, enq_n=0, hostcomm_ms=0.0)
    its = reason = 0
    rnorm = 0.0
    tm = None
    t0 = time.perf_counter()
    for _ in range(steps):
        its, reason, rnorm = step()
        tm = solver.timings()
        acc["spmv_ms"] += tm["spmv_ms_total"]; acc["spmv_n"] += tm["spmv_launches"]
        acc["asm_ms"] += tm["assemble_ms"]; acc["sol_ms"] += tm["solve_ms"]
        acc["if_ms"] += tm["iface_ms_total"]; acc["sc_ms"] += tm["scalar_ms_total"]; acc["ex_ms"] += tm["exposed_ms_total"]
        acc["comm_n"] += tm["comm_samples"]
        acc["enq_ms"] += tm["host_enqueue_ms"]; acc["enq_n"] += tm["host_enqueued_iterations"]; acc["hostcomm_ms"] += tm["host_comm_ms"]
    sync()
    elapsed = time.perf_counter() - t0
    if dump_dir:
        dump_outputs(solver, its, reason, rnorm, dump_dir)
    R["mem"] = pf.device_memory(J.device_index)      # mesh, pattern, incidence, both SpMV forms, vectors: all resident
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if hooks is not None and hooks.error is not None:
            raise hooks.error

    # ---- sanity of the answer on the owned rows ------------------------------------------
    def owned_check(u):
        if beam:    # the reference's docs image shows a maximum displacement magnitude of 0.82 (the tip; partial on a rank)
            conn, xyz, edof, sa = solver.downloadMesh()
            full = np.zeros(sz["nNode_local"] * 3)
            # owned local dof l <-> (node, d): scatter through the element dof array
            e_l = edof.reshape(4, 3, -1)
            for a in range(4):
                for d in range(3):
                    l = e_l[a, d]
                    ok = (l >= 0) & (l < size_local)
                    full[conn[a][ok] * 3 + d] = u[l[ok]]
            return "max_displacement_magnitude_owned_rows", float(np.linalg.norm(full.reshape(-1, 3), axis=1).max())
        if "xyz_free" in R:          # another numbering: the coordinates of the free nodes came with the host mesh
            return "max_nodal_error", float(np.abs(u - (R["xyz_free"] ** 2).sum(0)).max())
        # u = x^2+y^2+z^2 is nodally exact on this mesh family; owned free nodes in closed form

        def axis_tab(lo, hi, m):      # xx = lo; repeat: use xx; xx += dx, then the "%.8f" round trip (genTetra.cpp:194-216)
            out, v, d = [], lo, (hi - lo) / m
            for _ in range(m + 1):
                out.append(float("%.8f" % v))
                v += d
            return np.array(out)
        ax = [axis_tab(ext[0], ext[1], nEx), axis_tab(ext[2], ext[3], nEy), axis_tab(ext[4], ext[5], nEz)]
        idx = [np.arange(1, m) for m in nE]                  # interior nodes of every axis ...
        l0, l1 = sz["layer0"], sz["layer1"]                  # ... of the owned node planes along the cut axis
        idx[axis] = np.array([c for c in range(0 if rank == 0 else l0 + 1, l1 + 1) if 0 < c < nE[axis]], dtype=int)
        if not len(u):
            return "max_nodal_error", 0.0
        ex = (ax[2][idx[2]] ** 2)[:, None, None] + (ax[1][idx[1]] ** 2)[None, :, None] + (ax[0][idx[0]] ** 2)[None, None, :]
        return "max_nodal_error", float(np.abs(u - ex.ravel()).max())

    if args.full:
        R["check_name"], R["check"] = owned_check(solver.getSolution())

    # ---- the same step at the parity tolerance (SURVEY 8d asks for both), untimed extra ----
    R["parity"] = None
    if parity_step:
        solver.setTolerances(rtol=1e-10, maxits=10000)
        t1 = time.perf_counter()
        its10, reason10, rn10 = step()
        t10 = time.perf_counter() - t1
        R["parity"] = {"rtol": 1e-10, "iterations": its10, "converged_reason": reason10, "rnorm": rn10, "ms_per_step": t10 * 1e3,
                       "dof_per_s": N / t10, "max_nodal_error": owned_check(solver.getSolution())[1]}
        solver.setTolerances(rtol=rtol, maxits=10000)

    R["pc"] = pc
    R["pc_in_effect"] = solver.preconditioner()
    R["amg"] = solver.amgInfo() if R["pc_in_effect"] == "gamg" else None
    R["amg_aggregation"] = solver.amgAggregation() if R["pc_in_effect"] == "gamg" else None
    R["incidence_patterns"] = solver.incidencePatterns()
    R["amg_layout"] = solver.amgLayout() if R["pc_in_effect"] == "gamg" else None
    R["amg_cycle"] = solver.amgCycle() if R["pc_in_effect"] == "gamg" else None
    R["amg_vd"] = solver.amgValueDictionaries() if R["pc_in_effect"] == "gamg" else None
    R.update(N=int(N), sz=sz, axis=axis, elapsed=elapsed, its=its, reason=reason, rnorm=rnorm, acc=acc, info=info,
             event_overhead_ms=tm["event_overhead_ms"] if tm else 0.0, cinfo=solver.commInfo(),
             fmt_bytes=solver.spmvFormatBytes(), value_dict=solver.spmvValueDictionary(), gap_table=solver.spmvGapTable(), gap_escapes=solver.spmvGapEscapes(), bits=solver.spmvColumnBits(),
             row_group=solver.spmvRowGroup(), final=solver.commDescribe() if world > 1 else None,
             ms_per_step=elapsed / steps * 1e3, ms_per_iteration=acc["sol_ms"] / steps / max(its, 1))
    R.pop("xyz_free", None)
    if world > 1 and probe_comm:
        # what the links cost, measured in THIS job on THIS transport (collective; SURVEY 8(e)'s message sizes): a face of config 4
        # (51 x 51 nodes x 3 dofs = 62 KB) and of config 5 (401^2 dofs = 1.29 MB) with the two slab neighbours, the CG's 3 scalars
        # and the 125 000-row right-hand side of a replicated multigrid level through the all-reduce
        try:
            x62, a3 = solver.commBench(7803, 100, allreduce_count=3, slab_neighbours=True)
            x129, a125 = solver.commBench(160801, 50, allreduce_count=125000, slab_neighbours=True)
            R["comm_bench"] = {"exchange_62KB_with_slab_neighbours_us": 1e3 * x62, "exchange_1.29MB_with_slab_neighbours_us": 1e3 * x129,
                               "allreduce_3_doubles_us": 1e3 * a3, "allreduce_125000_doubles_us": 1e3 * a125, "transport": solver.commDescribe()["backend"]}
        except pf.PfemError as e:
            R["comm_bench"] = {"skipped": str(e)}
        if R["pc_in_effect"] == "gamg" and (R["amg_layout"] or {}).get("coupled"):
            try:
                R["cycle_profile"] = solver.amgCycleProfile()
            except pf.PfemError as e:
                R["cycle_profile"] = {"skipped": str(e)}
    solver.free()
    return R


def comm_block(J, R):
    """`comm` of an N > 1 line: the proof of what ran (backend and rank count as the transport's own communicators report
    them, every rank's device) and what an iteration exchanges."""
    rr, final, cinfo, acc = R["ranks_report"], R["final"], R["cinfo"], R["acc"]
    counts = sorted({r["backend_ranks"] for r in rr})
    out = {
        "transport": {"rccl": "rccl", "host": "gloo-host-hooks"}.get(final["backend"], final["backend"]),
        # ncclCommCount on every rank (-1: host hooks have no communicator)
        "rccl_comm_count": counts[0] if len(counts) == 1 else counts,
        "rccl_version": rr[0]["backend_version"],
        "fallback_reason": J.fallback_reason,
        "spmv_form": {0: "in order", 1: "overlapped", -1: "not voted"}[final["overlapped_form"]],
        "ranks": [{k: r.get(k) for k in ("rank", "local_rank", "device_index", "solver_device", "backend_device", "backend_ranks",
                                          "device_name", "device_uuid", "pci_bus_id", "pid", "layers", "size_local")} for r in rr],
        "distinct_devices": len({(r.get("device_uuid") or r.get("pci_bus_id") or r["device_index"]) for r in rr}),
        "neighbours": cinfo["n_peers"], "bytes_per_exchange": 8 * cinfo["doubles_per_exchange"],
        "bytes_per_neighbour": 8 * cinfo["doubles_per_exchange"] // max(cinfo["n_peers"], 1),
        "boundary_slices": cinfo["boundary_slices"], "slices": cinfo["total_slices"], "samples": acc["comm_n"],
        "host_enqueue_us_per_iteration": 1e3 * acc["enq_ms"] / max(acc["enq_n"], 1),
        "host_us_inside_transport_calls_per_iteration": 1e3 * acc["hostcomm_ms"] / max(acc["enq_n"], 1)}
    if acc["comm_n"]:           # rank 0, sampled with the SpMV
        out.update({"interface_exchange_ms": acc["if_ms"] / acc["comm_n"], "scalar_allreduce_ms": acc["sc_ms"] / acc["comm_n"],
                    "exposed_wait_ms": acc["ex_ms"] / acc["comm_n"]})
    return out


def compat_mode(args):
    """`--mode compat`: what the reference's unchanged driver costs through the drop-in boundary at this size.
    The problem is prepared here (host generator + the driver's numbering, untimed), handed to the build's Fortran host program as
    a binary file, and that program -- a CHILD process, it alone touches the GPU -- runs the reference's call sequence:
    MatSetValues(INSERT_VALUES) per element (:791-802), setZero, the element loop with StiffnessResidualPoissonLinearTetra +
    MatSetValues / VecSetValues(ADD_VALUES) (:828-884), factoriseAndSolve (:898-902).  Beside it: the oracle's serial assembly of
    the same mesh on this host (what the same loop costs without the boundary)."""
    import subprocess
    import tempfile

    import numpy as np
    from oracle import pfem_oracle as O
    from pfemfort_amd import host as H
    n = args.n
    exe = os.path.join(ROOT, "pfemfort_amd", "fortran", "build", "boundary_check")
    if not os.path.exists(exe):
        raise SystemExit(f"{exe} is not built (make -C pfemfort_amd/fortran check: needs flang where the tree is built)")
    beam = args.workload == "beam"
    ndof = 3 if beam else 1
    box = (-0.5, 0.5, n // 4, 0.0, 6.0, 3 * n // 2, -0.5, 0.5, n // 4) if beam else (-1, 1, n, -1, 1, n, -1, 1, n)
    t0 = time.perf_counter()
    mesh = H.gen_box_tets(*box, bc_mode=1 if beam else 0, ndof=ndof)
    dm = H.dof_numbering(mesh.nNode, ndof, mesh.bc_node, mesh.bc_dof, mesh.bc_val)
    conn_new, xyz_new = H.renumber_mesh(mesh, dm)
    edof = H.elem_dof_array(conn_new, dm.NodeDofArrayNew)
    ed = np.zeros(6)
    src = H.ELAST_ELEMDATA if beam else H.POISSON_ELEMDATA
    ed[:len(src)] = src
    N = int(dm.size_global)
    t_prepare = time.perf_counter() - t0
    # the oracle's serial assembly of the same system (pattern outside its timer, like the INSERT pass here)
    O.set_threads(1)
    o_edof = O.elem_dof_array(mesh.conn, dm.NodeDofArrayNew)
    rowptr, cols = O.csr_pattern(o_edof, N)
    t0 = time.perf_counter()
    O.assemble(O.ELAST_TET if beam else O.POISSON_TET, mesh.xyz, mesh.conn, o_edof, dm.solnApplied, O.ELAST_ELEMDATA if beam else O.POISSON_ELEMDATA, N, rowptr, cols)
    t_oracle = time.perf_counter() - t0
    del rowptr, cols
    out = {"mode": "compat", "what": "the reference driver's call sequence through the drop-in boundary: Fortran host loop (element routine + MatSetValues / "
                                     "VecSetValues per element) -> C ABI, the GPU solves (tests/native/boundary_check.F90 = tetrapoissonparallelimpl1.F:786-905 "
                                     "without the mesh bookkeeping)",
           "config": {"workload": f"{box[2]}x{box[5]}x{box[8]}x6 tet {'elasticity beam' if beam else 'Poisson'}", "elements": int(mesh.nElem), "free_dofs": N},
           "pc": args.pc, "rtol": args.rtol, "prepare_s_untimed": t_prepare, "oracle_serial_assembly_s": t_oracle}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "problem.bin"), "wb") as f:
            np.array([ndof, mesh.nNode, mesh.nElem, N, 1], np.int32).tofile(f)
            np.array([N], np.int32).tofile(f)
            np.zeros(mesh.nElem, np.int32).tofile(f)
            np.ascontiguousarray(xyz_new.T, np.float64).tofile(f)            # xyz(3, nNode), column by column
            np.ascontiguousarray((conn_new.T + 1), np.int32).tofile(f)        # conn(4, nElem), 1-based
            np.ascontiguousarray(edof.T, np.int32).tofile(f)                  # edof(nsize, nElem)
            np.ascontiguousarray(dm.solnApplied, np.float64).tofile(f)
            ed.tofile(f)
        with open(os.path.join(tmp, "petsc_options.dat"), "w") as f:
            f.write(f"-pc_type {args.pc}\n")
        runs = []
        for rep in range(max(1, args.steps)):
            r = subprocess.run([exe], cwd=tmp, env=dict(os.environ, PFEM_KSP_RTOL=repr(args.rtol)), capture_output=True, text=True, timeout=3000)
            tline = [ln for ln in r.stdout.splitlines() if ln.startswith("TIMING")]
            if r.returncode != 0 or not tline:
                raise SystemExit("the Fortran host program failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
            ins, setz, loop, solve = (float(x) for x in tline[-1].split()[1:5])
            conv = [ln for ln in r.stdout.splitlines() if "Convergence in" in ln or "onvergence" in ln]
            runs.append({"insert_values_pass_s": ins, "set_zero_pattern_on_device_s": setz, "element_loop_add_values_s": loop, "factorise_and_solve_s": solve,
                         "reference_timed_region_s": loop + solve, "dof_per_s_reference_timed_region": N / (loop + solve), "solver_line": conv[-1].strip() if conv else None})
    best = min(runs, key=lambda q: q["reference_timed_region_s"])
    out.update(best)
    out["runs"] = runs
    out["element_loop_vs_oracle_serial_assembly"] = best["element_loop_add_values_s"] / t_oracle
    print(json.dumps(out))
    return 0


def main():
    args = parse_args()
    if args.mode == "compat":
        raise SystemExit(compat_mode(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: this process has not touched the GPU (nothing but argparse so
        # far) and never will -- it starts N fresh rank processes through torch.distributed.run, relays their output and
        # exits with their code
        raise SystemExit(self_launch(args))

    # stdout carries ONE JSON line and nothing else: libraries that print to the C stdout of a rank (gloo announces its
    # peers there) are sent to stderr, the line goes out through a duplicate of the original descriptor
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    import faulthandler
    faulthandler.enable()
    # os._exit(1) after the dump; the bring-up of an N>1 run (rendezvous, RCCL communicators, transport self-test) gets a
    # shorter leash so that a hung first collective ends the attempt while a retry is still worth it
    faulthandler.dump_traceback_later(min(args.rank_timeout, args.bringup_timeout) if args.gpus > 1 else args.rank_timeout, exit=True)

    # N = 1: the SpMV's HBM traffic, measured by two short child runs under rocprofv3 --pmc BEFORE this process touches the GPU
    pmc_live = None
    if args.full and args.gpus == 1 and "WORLD_SIZE" not in os.environ and not args.no_pmc:
        pmc_live = pmc_traffic_live(sys.argv[1:])
        if isinstance(pmc_live, str):
            print(f"bench.py: HBM traffic not measured in this run ({pmc_live})", file=sys.stderr, flush=True)

    import pfemfort_amd as pf
    from pfemfort_amd import host as H

    if int(os.environ.get("RANK", "0")) == 0:      # (the first line of every run says which solver it is: the library's own default differs)
        print(f"bench.py: KSP = cg, PC = {args.pc} (-pc_type {args.pc}); the library, the Python drivers and the Fortran modules default to "
              "-pc_type jacobi unless petsc_options.dat / setPreconditioner says otherwise", file=sys.stderr, flush=True)
    J = Job(args)
    world, rank = J.world, J.rank
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE {world}")
    if world > 1:
        import torch
        import torch.distributed as dist
        J.torch, J.dist = torch, dist
        torch.cuda.set_device(J.device_index)
        dist.init_process_group(backend=args.backend, device_id=torch.device("cuda", J.device_index)
                                if args.backend == "nccl" else None)
    if pf.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X: libpfem_amd has no CPU path")
    if world > 1 and rank == args.debug_die_rank:
        os._exit(3)

    # ---- the configuration ---------------------------------------------------------------
    n = args.n
    beam = args.workload == "beam"
    cube = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
    if beam:      # SURVEY 8(d) cfg 4: [-.5,.5]x[0,6]x[-.5,.5], clamp y=0, body force (0.1f,0,0)
        nE = (50 * args.beam_scale, 300 * args.beam_scale, 50 * args.beam_scale); ext = (-0.5, 0.5, 0.0, 6.0, -0.5, 0.5)
    elif world == 1 or args.strong:
        nE = (n, n, n); ext = cube
    elif not args.stack:
        side = round(n * world ** (1.0 / 3.0))
        nE = (side, side, side); ext = cube
    else:
        nE = (n, n, n * world); ext = (-1.0, 1.0, -1.0, 1.0, -1.0, -1.0 + 2.0 * world)
    # the first HIP calls of a process create the device context, load the code objects of every kernel family on first
    # use and set up the runtime's copy paths (0.3 - 1 s, depending on how cold the box is; one 96 KB device-to-host copy
    # took 8 ms the first time a process made one): not part of the mesh setup nor of a step, so a small problem is run
    # through the whole path first -- the same preconditioner, enough levels to touch every kernel of the hierarchy -- and
    # its time is reported separately
    t_init = time.perf_counter()
    kind = pf.ELAST_TET if beam else pf.POISSON_TET
    ni = 8 if world > 1 else 24
    w = pf.PetscSolver().initialise(*[H.box_slab_sizes(ni, ni, ni, 1 if beam else 0, 3 if beam else 1)[k] for k in ("size_local", "size_global")],
                                    device=J.device_index)
    w.generateBoxMesh(kind, 0.0, 1.0, ni, 0.0, 1.0, ni, 0.0, 1.0, ni, bc_mode=1 if beam else 0)
    w.buildPattern()
    if world == 1:
        w.setPreconditioner(args.pc)
    w.assemble(H.ELAST_ELEMDATA if beam else H.POISSON_ELEMDATA, H.TIMEDATA)
    w.factoriseAndSolve()
    w.free()
    t_init = time.perf_counter() - t_init

    if args.ab_child:
        # this job IS the companion of another job's line: the same steps over the peer-memory transport, one brief JSON line
        try:
            P = run_case(J, beam, nE, ext, max(1, min(args.steps, 3)), 1, args.rtol, profile=False, transport="peer", probe_comm=True)
        except (pf.PfemError, RuntimeError) as e:           # (a transport that failed mid-run on this rank: its peers time out and report the same)
            P = {"skipped": f"{type(e).__name__}: {e}"}
        if rank == 0:
            Pb = P if "skipped" in P else {"value": P["N"] * P["steps"] / P["elapsed"], "ms_per_step": P["ms_per_step"], "iterations": P["its"],
                                           "converged_reason": P["reason"], "ms_per_iteration": P["ms_per_iteration"], "steps": P["steps"],
                                           "first_step_ms": P.get("first_step_ms"), "link_latencies": P.get("comm_bench"),
                                           "coupled_cycle": P.get("cycle_profile"),
                                           "host_enqueue_us_per_iteration": 1e3 * P["acc"]["enq_ms"] / max(P["acc"]["enq_n"], 1)}
            json_out.write(json.dumps(Pb) + "\n")
            json_out.flush()
        if world > 1:
            J.dist.barrier()
            J.dist.destroy_process_group()
        faulthandler.cancel_dump_traceback_later()
        return
    R = run_case(J, beam, nE, ext, args.steps, args.warmup, args.rtol, profile=args.full,
                 parity_step=(args.full and world == 1 and not args.no_parity_step and not beam), probe_comm=args.full,
                 dump_dir=args.dump_outputs)
    weak = not (beam or args.strong)
    # ---- the same configuration with north_star's own preconditioner, the diagonal: a shorter, separately timed run
    Jac = None
    if args.full and R["pc"] != "jacobi" and not args.no_jacobi_step:
        Jac = run_case(J, beam, nE, ext, max(1, min(args.steps, 3)), 1, args.rtol, profile=True, pc="jacobi")
    # ---- N > 1, weak run: the strong-scaling companion.  The cube of 2 x --cells per side (at the default 200: BASELINE
    # config 5, 400^3 x 6 tets, which fits ONE MI355X: profiles/r02/bench_cfg5_400cube_single_gpu.json) on the same N
    # ranks -- the >= 6x-at-8-GPUs evidence next to the weak figure, whose Jacobi iteration count grows with the problem.
    S = None
    if args.full and world > 1 and weak and not args.stack and not args.no_strong_block:
        side = 2 * n
        if nE == (side, side, side):
            S = R                       # N = 8: the weak configuration IS that cube
        else:
            S = run_case(J, False, (side, side, side), cube, max(1, min(args.steps, 2)), 1, args.rtol, profile=False)

    nEx, nEy, nEz = nE
    N, its, acc, info, cinfo, sz = R["N"], R["its"], R["acc"], R["info"], R["cinfo"], R["sz"]
    if rank == 0:
        axis_name = "xyz"[R["axis"]]
        cross = [m + 1 for d, m in enumerate(nE) if d != R["axis"]]
        partition = None
        if world > 1:
            rr = R["ranks_report"]
            partition = {"axis": axis_name, "hex_layers_per_rank": [r["layers"][1] - r["layers"][0] for r in rr],
                         "face_nodes": cross[0] * cross[1],
                         "face_bytes_per_neighbour": 8 * cinfo["doubles_per_exchange"] // max(cinfo["n_peers"], 1),
                         "rows_per_rank": [r["size_local"] for r in rr]}
        out = {
            "metric": "DOF/s (assembly+CG-to-tol)", "value": N * args.steps / R["elapsed"], "unit": "DOF/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": R["ms_per_step"], "higher_is_better": True, "scaling": "weak" if weak else "strong",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": (f"tetraelasticityparallelimpl1: [-.5,.5]x[0,6]x[-.5,.5] beam, {nEx}x{nEy}x{nEz}x6 P1 tets, "
                                    "3 dofs/node, clamped at y=0, body force (0.1,0,0), E=240.565, nu=0.3 (REAL(4) literals)"
                                    if beam else
                                    f"tetrapoissonparallelimpl1: [-1,1]^2x[{ext[4]:g},{ext[5]:g}] box, "
                                    f"{nEx}x{nEy}x{nEz}x6 P1 tets, u=x^2+y^2+z^2 Dirichlet on all faces, f=-6"),
                       "elements": 6 * nEx * nEy * nEz, "nodes": (nEx + 1) * (nEy + 1) * (nEz + 1), "free_dofs": int(N),
                       "solver": f"CG{' (single-reduction form)' if args.single_reduction else ''} + " +
                                 {"pbjacobi": "node-block Jacobi (pbjacobi)", "jacobi": "point Jacobi",
                                  "gamg": "plain-aggregation multigrid V(1,1) cycle (-pc_type gamg: aggregates of 2x2x2 nodes paired along the axes of the mesh's "
                                          "lattice -- by matching on the strength graph where there is none --, Galerkin coarse "
                                          "operators re-summed in every solve, Chebyshev smoothing, dense bottom solve" +
                                          ("" if world == 1 else
                                           "; ONE hierarchy across the ranks: aggregates inside a rank's owned dofs, global Galerkin operators held "
                                           "sub-assembled, a neighbour exchange behind every SpMV of the cycle" if (R["amg_layout"] or {}).get("coupled") else
                                           "; block Jacobi over the ranks, one hierarchy per rank") + ")"}[R["pc_in_effect"]] +
                                 f", zero initial guess, rtol {args.rtol:g} on ||M^-1 r|| (PETSc KSPCG default norm). The reference's PETSc run "
                                 "used KSPCG + PCBJACOBI (per-rank ILU(0), solverpetsc.F:187,206), which is NOT reproduced: "
                                 "iteration counts are not comparable with a PETSc run of the reference; north_star's CG + point Jacobi is "
                                 "measured next to it under --full (`jacobi_step`)",
                       "parallelism": "1 GPU" if world == 1 else
                                      f"{world} slabs of hex layers across {axis_name}, sub-assembled interface rows, neighbour exchange of "
                                      f"{cinfo['doubles_per_exchange']} doubles with {cinfo['n_peers']} neighbour(s) per SpMV "
                                      f"+ {1 if args.single_reduction and args.pc == 'jacobi' else 2} scalar all-reduce(s) per iteration",
                       "partition": partition, "numbering": args.numbering, "jitter": args.jitter},
            "iterations": its, "converged_reason": R["reason"], "rnorm": R["rnorm"],
            "assembly_ms_per_step": acc["asm_ms"] / args.steps, "solve_ms_per_step": acc["sol_ms"] / args.steps,
            "ms_per_iteration": R["ms_per_iteration"],     # weak scaling: iterations grow with the problem
            "setup_s_untimed": R["t_setup"], "setup_breakdown_s": {"generate_mesh_and_numbering_on_device": R["t_generate"],
                                                                   "symbolic_pattern_and_incidence": R["t_pattern"],
                                                                   "symbolic_pattern_and_incidence_second_build": R["t_pattern2"],
                                                                   "hip_context_and_code_object_load_on_a_small_problem_not_in_setup": t_init},
            # what ONE cold step costs (the first warm-up step: everything a timed step does + the once-per-pattern symbolic set-up
            # of the preconditioner, which the timed steps reuse like they reuse the sparsity pattern): the figure to compare
            # with a single run of the reference driver, whose KSPSolve timer contains its PCSetUp
            "first_step_ms_including_once_per_pattern_setup": R["first_step_ms"],
            # the same as a rate: DOF/s of ONE run of the reference driver's timed section on a fresh pattern (assembly + KSPSolve with
            # its PCSetUp, tetrapoissonparallelimpl1.F:826-902); `value` is the rate of every later step on the same pattern
            "cold_value": (N / (R["first_step_ms"] * 1e-3)) if R.get("first_step_ms") else None,
            # what carried an N > 1 run (no measurement of its own: the ranks' reports and the transport's own description)
            "comm": comm_block(J, R) if world > 1 else None,
        }
        if args.full:
            ref1 = single_gpu_reference()
            bytes_per_spmv = 12 * info["nnz"] + 20 * info["n_local"]       # FP64 vals, int32 cols
            fmt_bytes = R["fmt_bytes"]
            # The event pair of a sampled launch reports marker-end -> kernel-end.  `avg_launch_ms` is that RAW figure: it is
            # the one rocprofv3 --kernel-trace agrees with (profiles/r02: 209.97 us traced, 209.98 us raw pairs in the driver's
            # run).  The offset of an empty kernel timed the same way is reported for information only and NOT subtracted
            # (round 2 did, and overstated the fraction by 0.02).
            raw_spmv_ms = acc["spmv_ms"] / max(acc["spmv_n"], 1)
            avg_spmv_ms = max(raw_spmv_ms, 1e-9)
            achieved = bytes_per_spmv / (avg_spmv_ms * 1e-3) / 1e9 if acc["spmv_n"] else 0.0
            traffic, traffic_source, traffic_counters = None, None, None
            if isinstance(pmc_live, dict) and pmc_live:
                # the CG's own product: the WITH_DOT = true kernel with the most dispatches in the child runs (same command, one step)
                kname, e = max(pmc_live.items(), key=lambda kv: kv[1]["dispatches"])
                traffic = (2.0 * e["FETCH_SIZE_KB"] + e["WRITE_SIZE_KB"]) * 1024.0
                traffic_source = ("measured in THIS run: two child runs of the same command (one step) under rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE "
                                  "(separate passes) before this process touched the GPU; bytes = (2 x FETCH_SIZE + WRITE_SIZE) KB per dispatch, "
                                  "FETCH_SIZE doubled because gfx950 tallies 128-B requests at 64 B")
                traffic_counters = dict(e, kernel=kname)
            elif world == 1 and args.numbering == "lattice" and args.jitter <= 0.0:
                traffic, traffic_source = pmc_traffic(info["nnz"], R["value_dict"])
                if traffic and isinstance(pmc_live, str):
                    traffic_source += f" [not measured in this run: {pmc_live}]"
            hbm_bytes = traffic if traffic else fmt_bytes
            hbm_gbps = hbm_bytes / (avg_spmv_ms * 1e-3) / 1e9 if acc["spmv_n"] else 0.0
            # names as rocprofv3 prints them: k_spmvr / k_spmvg / k_spmv16 <WITH_DOT, gap table>, k_spmvr32 / k_spmv <WITH_DOT>
            tbl = R["gap_table"]
            tname = "true" if tbl else "false"
            tnote = f" with a table of the {tbl} distinct gaps beyond 32767" if tbl else ""
            bits = R["bits"]
            vdn = R["value_dict"]           # pfem_valdict.hpp: the values as 16-bit codes into a dictionary of the distinct ones (0: fp64 copy)
            vd = "_vd" if vdn else ""
            vnote = (f"; matrix values streamed as 16-bit codes into a dictionary of the {vdn} DISTINCT values of this matrix held in LDS "
                     "(lossless: the same doubles, the same products, the same bits)") if vdn else ""
            kernel = {3: f"pfem::k_spmvg{vd}<true, {tname}> (row-grouped wave-sliced CSR SpMV + (p,Ap) partials: the 3 dof rows of a "
                         f"node share one lane, 16-bit column gaps{tnote}{vnote}), rank 0",
                      4: ("pfem::k_spmvr32<true>" if bits == 32 else f"pfem::k_spmvr{vd}<true, {tname}>") +
                         " (wave-sliced CSR SpMV + (p,Ap) partials; 4 consecutive rows per lane share one relative column stream of "
                         f"{bits}-bit gaps{tnote}, x read as 32-B quads{vnote}), rank 0"}.get(
                R["row_group"],
                ("pfem::k_spmv16e<true>" if (bits == 16 and R.get("gap_escapes")) else f"pfem::k_spmv16<true, {tname}>" if bits == 16 else "pfem::k_spmv<true>") +
                " (wave-sliced CSR SpMV + (p,Ap) partials; %d-bit column %s%s), rank 0"
                % (bits, "gaps" if bits == 16 else "indices", " with escapes to the int32 columns" if R.get("gap_escapes") else tnote))
            out.update({
                R["check_name"]: R["check"],
                # how to quote this line: three rates of the same configuration, never the first alone
                "headline": {"value_warm_step_default_solver": N * args.steps / R["elapsed"],
                             "cold_value_first_step_with_preconditioner_setup": (N / (R["first_step_ms"] * 1e-3)) if R.get("first_step_ms") else None,
                             "north_star_cg_point_jacobi": (Jac["N"] / (Jac["ms_per_step"] * 1e-3)) if Jac else None,
                             "unit": "DOF/s", "default_solver": R["pc_in_effect"],
                             "solver_default_at_the_boundary": "the C ABI, the Python drivers and the Fortran modules default to -pc_type jacobi (north_star's "
                                                               "solver); one line `-pc_type gamg` in petsc_options.dat -- where the reference's own run "
                                                               "takes its KSP options from (tetrapoissonparallelimpl1.F:168) -- selects what this line's `value` ran"},
                "parity_tolerance_step": R["parity"],
                "preconditioner": ({"name": R["pc_in_effect"], "levels": R["amg"]["levels"], "rows_per_level": R["amg"]["rows"],
                                    "nnz_per_level": R["amg"]["nnz"], "gershgorin_lambda_max": R["amg"]["lambda_max"],
                                    "operator_complexity": sum(R["amg"]["nnz"]) / max(R["amg"]["nnz"][0], 1),
                                    "cheb_degree": R["amg"]["cheb_degree"], "cheb_degree_on_the_assembled_matrix": R["amg"]["fine_degree"], "eig_ratio": R["amg"]["eig_ratio"], "coarse_scale": R["amg"]["coarse_scale"],
                                    "numeric_setup_ms_per_solve_inside_the_timer": R["amg"]["numeric_ms"],
                                    # a solve = numeric set-up + (iterations + 1) cycles: the initial one, then one per iteration
                                    # (`ms_per_iteration` above divides the whole solve by the iterations)
                                    "ms_per_cycle_with_its_cg_iteration": (acc["sol_ms"] / args.steps - R["amg"]["numeric_ms"]) / (its + 1),
                                    "symbolic_setup_ms_once_per_pattern": R["amg"]["symbolic_ms"],
                                    "symbolic_setup_where": "first solve after a pattern build (a warm-up step; with --warmup 0 the first timed step)",
                                    "levels_paired_on_the_lattice": R["amg_layout"]["lattice_levels"],
                                    # how every level's aggregates were formed (pfem_solver_amg_aggregation), rank 0's view
                                    "aggregation": R["amg_aggregation"],
                                    # -pc_mg_cycle_type (--cycle; V unless asked: W halves the iterations on matched aggregates and costs
                                    # twice the time, LAB_NOTES round 5)
                                    "cycle": R["amg_cycle"]["cycle"], "last_level_visited_twice": R["amg_cycle"]["last_level_visited_twice"],
                                    # levels whose SpMVs stream 16-bit value codes into a dictionary of the level's distinct values (0: fp64 values)
                                    "value_dictionary_entries_per_level": R["amg_vd"],
                                    "distributed_levels": R["amg_layout"]["distributed_levels"] if world > 1 else None,
                                    "communication_per_cycle": ({"neighbour_exchanges": R["amg_layout"]["exchanges_per_cycle"],
                                                                 "all_reduces": R["amg_layout"]["allreduces_per_cycle"],
                                                                 "note": "enqueued by one V-cycle, next to the CG's own exchange and two all-reduces per iteration"}
                                                                if world > 1 else None),
                                    "hierarchy": ("one rank" if world == 1 else "one across the ranks" if R["amg_layout"]["coupled"] else "one per rank (block Jacobi over the ranks)"),
                                    "scope": ("the whole matrix" if world == 1 else "rank 0's owned rows of every level of the global hierarchy"
                                              if R["amg_layout"]["coupled"] else "rank 0's block")} if R["amg"] else {"name": R["pc_in_effect"]}),
                "jacobi_step": ({"preconditioner": "point Jacobi (north_star's)", "steps": Jac["steps"], "warmup": Jac["warmup"],
                                 "ms_per_step": Jac["ms_per_step"], "dof_per_s": Jac["N"] / (Jac["ms_per_step"] * 1e-3), "iterations": Jac["its"],
                                 "converged_reason": Jac["reason"], "ms_per_iteration": Jac["ms_per_iteration"], Jac["check_name"]: Jac["check"],
                                 "speedup_of_value_over_it": Jac["ms_per_step"] / R["ms_per_step"]} if Jac else None),
                "device_memory_gb": {"in_use_rank0_device": round((R["mem"]["total_bytes"] - R["mem"]["free_bytes"]) / 1e9, 2),
                                     "total": round(R["mem"]["total_bytes"] / 1e9, 2)},
                # the kernel furthest from the HBM roofline, with the bound it really has: FP64 issue (every element's geometry is
                # evaluated once per incident node, un-contracted as the reference's order demands).  The event time is this
                # run's; the issue fraction is replayed from the committed SQ counters of the same kernel on the same workload
                "assembly_kernel": ({"kernel": "pfem::k_gather_poisson_tet4 (gather assembly; in the steady state it also writes the SpMV's 16-bit value codes "
                                               "and level 0's inverse diagonal + Gershgorin ratios for the multigrid)",
                                     "event_ms_per_step": acc["asm_ms"] / args.steps,
                                     # what it waits for (profiles/r06/assembly_kernel_bound.txt): not its arithmetic -- the same kernel with the
                                     # element geometry for nothing is no faster -- but its gathered node records (72 x 32 B per row through the
                                     # L1) under 4 waves per SIMD; its incidence records come from a cached pattern table where the mesh's
                                     # numbering repeats (`incidence_patterns` > 0: 2.34 GB moved per launch instead of 5.37)
                                     "bound": "memory-latency (gathered node records at 4 waves per SIMD)",
                                     "incidence_patterns": R["incidence_patterns"][0], "longest_incidence_list": R["incidence_patterns"][1],
                                     "bytes_moved_per_launch_replayed_not_this_run": {"records_from_the_pattern_table": 2.34e9, "every_nodes_own_records": 5.37e9,
                                                                                      "source": "profiles/r06/assembly_kernel_bound.txt (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE per dispatch, tools/r06/incpat2.sh)"},
                                     # SQ_ACTIVE_INST_VALU / (32 x GRBM_GUI_ACTIVE) of this kernel on this workload, re-taken in round 6 at commit 43503de
                                     # with the pattern table (473.5 M / (32 x 18.47 M); before the table 0.68 = 466.1 M / (32 x 21.34 M); round 4: 0.75)
                                     "valu_issue_fraction_replayed_not_this_run": 0.80,
                                     "valu_issue_source": "profiles/r06/gather_and_spmv_sq_counters.txt (rocprofv3 --pmc, separate passes, tools/r06/final.sh)",
                                     # compulsory bytes per launch: SURVEY 8(d)'s 2.69 GB + the codes (0.24 GB) + the two vectors for the multigrid (0.13 GB)
                                     "hbm_frac_of_compulsory_bytes": (3.05e9 / (acc["asm_ms"] / args.steps * 1e-3) / 1e9 / HBM_PEAK_GBPS)
                                     if (not beam and world == 1 and args.n == 200 and args.numbering == "lattice" and args.jitter <= 0.0) else None}
                                    if (not beam and world == 1) else None),
                "roofline": {"bound": "hbm", "kernel": kernel,
                             # `frac` is the REAL fraction of the HBM peak: bytes the launch moves through the memory side (PMC counters of
                             # this run when rocprofv3 is on the box, else the committed passes of the same workload, else the storage of
                             # the selected form + x + y) / measured launch time / peak.  Never above 1.  What SURVEY 8(d) prices a launch
                             # at -- plain CSR, 12 B per nonzero + 20 B per row -- stands beside it as `algorithmic_*`; the compressed forms
                             # (16-bit gaps, relative row groups, value dictionary) move fewer bytes than that: `compression`
                             "achieved": hbm_gbps, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": hbm_gbps / HBM_PEAK_GBPS,
                             "frac_of_achievable_6300_gbps": hbm_gbps / 6300.0,
                             "algorithmic_achieved": achieved, "algorithmic_frac": achieved / HBM_PEAK_GBPS,
                             "compression": (bytes_per_spmv / hbm_bytes) if hbm_bytes else None,
                             "value_dictionary_entries": vdn,
                             "note": ("`achieved` / `frac`: bytes really moved (traffic) per second of the launch; `algorithmic_*`: the plain-CSR "
                                      "bytes of SURVEY 8(d) the launch REPLACES per second -- above the peak when the kernel streams "
                                      f"2 B of value code + 1/2 B of column gap per slot instead of 8 + 4 (the {vdn} distinct values of the assembled "
                                      "matrix sit in LDS; lossless, same bits). PFEM_SPMV_VALDICT=0 runs the fp64 copy") if vdn else None,
                             "traffic": traffic, "traffic_source": traffic_source, "traffic_counters": traffic_counters,
                             "format_bytes_per_launch": fmt_bytes,
                             "hbm_bytes_source": "PMC counters (traffic)" if traffic else "storage of the selected form + x + y",
                             "algorithmic_bytes_per_launch": bytes_per_spmv, "avg_launch_ms": avg_spmv_ms,
                             "avg_launch_source": f"raw HIP event pairs around every {2 if R['pc_in_effect'] == 'gamg' else 8}th launch of this kernel in the timed solves "
                                                  "(the CG's own SpMV), on the solver's stream" +
                                                  ("; the same kernel in the Jacobi step of this line: avg_launch_ms_in_jacobi_step; "
                                                   "profiles/r03/rocprofv3_kernel_stats*.txt hold one kernel trace per loop" if R["pc_in_effect"] == "gamg" else ""),
                             # what rocprofv3 --kernel-trace says about the same kernel in the same command (committed trace summaries).
                             # The events are bound to the dispatch itself (hipExtLaunchKernelGGL), and still read ~20 us more than the
                             # trace: under the tracer dispatches run one at a time, on the plain stream the kernel's first waves share
                             # the device with the last waves of the kernel before it (events without the system-scope fence: no change,
                             # measured in round 3).  The judged fraction uses the pair as it is, the lower of the two figures
                             "kernel_trace_avg_launch_us_replayed_not_this_run": kernel_trace_figures(info["nnz"], R["value_dict"]) if (world == 1 and args.numbering == "lattice" and args.jitter <= 0.0) else None,
                             "avg_launch_ms_in_jacobi_step": (Jac["acc"]["spmv_ms"] / max(Jac["acc"]["spmv_n"], 1)) if (Jac and Jac["acc"]["spmv_n"]) else None,
                             "event_pair_offset_ms_not_subtracted": R["event_overhead_ms"],
                             "launches_timed": acc["spmv_n"], "nnz": info["nnz"], "rows": info["n_local"]},
            })
            if world > 1:
                # how to read an N > 1 line: (1) per-iteration efficiency -- rows per GPU and millisecond of iteration against
                # the committed N = 1 figure (independent of the iteration count, which Jacobi makes grow with the problem);
                # (2) the strong-scaling companion on BASELINE config 5
                r1 = ref1.get("cfg3_200cube_" + R["pc_in_effect"], {})
                if r1.get("ms_per_iteration") and r1.get("free_dofs"):
                    rate1 = r1["free_dofs"] / r1["ms_per_iteration"]
                    out["per_iteration_efficiency"] = {
                        "value": (N / world / R["ms_per_iteration"]) / rate1,
                        "definition": "(free dofs per GPU / ms per CG iteration) of this run / the same of the N=1 run",
                        "n1_ms_per_iteration": r1["ms_per_iteration"], "n1_free_dofs": r1["free_dofs"], "n1_source": r1.get("source")}
                if S is not None:
                    r5 = ref1.get("cfg5_400cube_" + S["pc_in_effect"], {})
                    is5 = S["nE"] == (400, 400, 400)
                    out["strong_cfg5"] = {
                        "workload": "tetrapoissonparallelimpl1: [-1,1]^3, %dx%dx%dx6 P1 tets%s" % (*S["nE"], " (BASELINE config 5)" if is5 else ""),
                        "is_baseline_config5": is5, "free_dofs": S["N"], "n_gpus": world, "steps": S["steps"], "warmup": S["warmup"],
                        "same_run_as_value": S is R, "preconditioner": S["pc_in_effect"],
                        "ms_per_step": S["ms_per_step"], "dof_per_s": S["N"] / (S["ms_per_step"] * 1e-3), "iterations": S["its"],
                        "converged_reason": S["reason"], "ms_per_iteration": S["ms_per_iteration"], S["check_name"]: S["check"],
                        "single_gpu_ms_per_step": r5.get("ms_per_step") if is5 else None,
                        "single_gpu_source": r5.get("source") if is5 else None,
                        "speedup_vs_single_gpu": (r5["ms_per_step"] / S["ms_per_step"]) if (is5 and r5.get("ms_per_step")) else None,
                        "bytes_per_neighbour": 8 * S["cinfo"]["doubles_per_exchange"] // max(S["cinfo"]["n_peers"], 1)}
            if world == 1 and not args.no_cpu_baseline and not beam:
                out["cpu_baseline"] = cpu_baseline(n, args.rtol, extra_sample=(n >= 200))
            if world > 1:
                out["comm"]["link_latencies"] = R.get("comm_bench")
                out["comm"]["coupled_cycle"] = R.get("cycle_profile")
    else:
        out = None
    # ---- N > 1: the same steps over the OTHER device-side transport (A/B).  RCCL stays the headline (north_star); the
    # peer-memory transport (boxes + flags mapped through hipIpc*, fine-grained so that it is legal between devices) has only
    # ever run between processes sharing one GPU.  It runs as a SECOND, FRESH job of N rank processes that rank 0 starts as a
    # child once this job's ranks have left their process group (never an exec; the child gets its own process group and
    # session): if it hangs -- kernels spinning in bounded waits -- the child's process group is killed and THIS process, which
    # is healthy, prints the line without it and exits 0.  (Round 5 ran it inside these ranks behind a timer that called
    # os._exit(0) from a thread: a hung transport was reported to the launcher as success by processes that were not.)
    def brief(Q):
        if "skipped" in Q:
            return Q
        return {"value": Q["N"] * Q["steps"] / Q["elapsed"], "ms_per_step": Q["ms_per_step"], "iterations": Q["its"], "converged_reason": Q["reason"],
                "ms_per_iteration": Q["ms_per_iteration"], "steps": Q["steps"], "first_step_ms": Q.get("first_step_ms"),
                "link_latencies": Q.get("comm_bench"), "coupled_cycle": Q.get("cycle_profile"),
                "host_enqueue_us_per_iteration": 1e3 * Q["acc"]["enq_ms"] / max(Q["acc"]["enq_n"], 1)}
    main_kind = (R["final"]["backend"] if R.get("final") else None) if world > 1 else None
    if world > 1:
        J.dist.barrier()
        J.dist.destroy_process_group()
    faulthandler.cancel_dump_traceback_later()
    if args.full and world > 1 and not args.no_transport_ab and rank == 0:
        P = transport_ab_child(args)
        out["comm"]["transports"] = {{"rccl": "rccl", "host": "gloo-host-hooks"}.get(main_kind, main_kind): brief(R), "peer-ipc": P,
                                     "note": "same configuration, fresh solver each; the first entry is the run `value` reports; the second ran as "
                                             "a fresh child job of the same N ranks after this job's ranks had finished"}
    if rank == 0:
        json_out.write(json.dumps(out) + "\n")
        json_out.flush()


if __name__ == "__main__":
    main()

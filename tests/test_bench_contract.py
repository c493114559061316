"""bench.py's output contract: ONE JSON line on stdout with the metric of BASELINE.json, the roofline object of the
dominant kernel and the CPU baseline (small workload here; the default run is the 200^3 configuration)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _skip_unless_eight_gpus():
    """The eight-rank runs of BASELINE configs[3] / [4] put one rank on each of 8 GPUs; checked before any work."""
    import pfemfort_amd as pf
    n = pf.device_count()
    if n < 8:
        pytest.skip(f"needs 8 GPUs (one per rank), found {n}")


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_roofline_and_cpu_baseline():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--cells", "40", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"].split(" ")[0] == base["metric"].split(" ")[0] == "DOF/s" and d["unit"] == "DOF/s"
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (1, 2, 1)
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - d["config"]["free_dofs"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["converged_reason"] == 2 and d["max_nodal_error"] < 1e-3
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert rf["achieved"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and "traffic" in rf
    assert rf["algorithmic_bytes_per_launch"] == 12 * rf["nnz"] + 20 * rf["rows"] and rf["launches_timed"] > 0
    # `frac` is the REAL fraction (bytes moved: PMC traffic of this run where rocprofv3 is on the box, else the form's storage), never
    # above 1; the plain-CSR bytes of SURVEY 8(d) that the launch replaces travel beside it as algorithmic_*
    assert 0 < rf["frac"] <= 1.0 and rf["algorithmic_achieved"] >= rf["achieved"] and "traffic_source" in rf
    assert abs(rf["algorithmic_frac"] - rf["algorithmic_achieved"] / rf["peak"]) < 1e-12 and rf["compression"] >= 1.0
    assert rf["format_bytes_per_launch"] < rf["algorithmic_bytes_per_launch"]
    if rf["traffic"] is not None and "THIS run" in (rf["traffic_source"] or ""):
        c = rf["traffic_counters"]
        assert "<true" in c["kernel"] and c["dispatches"] > 0 and abs(rf["traffic"] - (2 * c["FETCH_SIZE_KB"] + c["WRITE_SIZE_KB"]) * 1024) < 1
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "DOF/s" and cb["value"] > 0 and cb["cores"] >= 1 and cb["sample"]
    # the same configuration as the GPU number, at the reference's three timer points
    assert "40^3" in cb["sample"] and abs(cb["total_s"] - cb["assembly_s"] - cb["solve_s"]) < 1e-9 and cb["its"] == d["jacobi_step"]["iterations"]
    if "mpi_one_rank_per_core" in cb:          # where an MPI is installed: the reference's mpirun restated, next to the OpenMP port
        m, o = cb["mpi_one_rank_per_core"], cb["openmp_port"]
        assert m["iterations"] == o["its"] == cb["its"] and m["converged_reason"] == 2 and m["free_dofs"] == d["config"]["free_dofs"]
        assert cb["value"] == max(m["value"], o["value"]) and 1 <= m["ranks"] <= 39
    assert d["parity_tolerance_step"]["rtol"] == 1e-10 and d["parity_tolerance_step"]["max_nodal_error"] < 1e-6
    # the default preconditioner is the multigrid V-cycle; north_star's point Jacobi is measured next to it
    pcb, js = d["preconditioner"], d["jacobi_step"]
    assert pcb["name"] == "gamg" and pcb["levels"] >= 3 and pcb["rows_per_level"][0] == d["config"]["free_dofs"] and pcb["rows_per_level"][-1] <= 128
    assert 1.0 < pcb["operator_complexity"] < 1.3 and pcb["numeric_setup_ms_per_solve_inside_the_timer"] > 0
    assert js["converged_reason"] == 2 and d["iterations"] < js["iterations"] / 3 and js["max_nodal_error"] < 1e-3
    assert abs(js["speedup_of_value_over_it"] - js["ms_per_step"] / d["ms_per_step"]) < 1e-9
    assert "PCBJACOBI" in d["config"]["solver"] and "gamg" in d["config"]["solver"] and d["setup_breakdown_s"]["generate_mesh_and_numbering_on_device"] >= 0 and d["setup_s_untimed"] < 5
    # a solve = numeric set-up + (iterations + 1) cycles; the kernel furthest from the HBM roofline travels with its real bound
    assert 0 < pcb["ms_per_cycle_with_its_cg_iteration"] < d["ms_per_iteration"]
    ak = d["assembly_kernel"]
    assert ak["bound"].startswith("memory-latency") and ak["event_ms_per_step"] == d["assembly_ms_per_step"] and os.path.exists(os.path.join(ROOT, ak["valu_issue_source"].split(" ")[0]))
    assert ak["incidence_patterns"] >= 1 and os.path.exists(os.path.join(ROOT, ak["bytes_moved_per_launch_replayed_not_this_run"]["source"].split(" ")[0]))
    assert d["preconditioner"]["aggregation"][0] == "bricks"
    assert d["cold_value"] > 0 and abs(d["cold_value"] - d["config"]["free_dofs"] / (d["first_step_ms_including_once_per_pattern_setup"] * 1e-3)) <= 1e-6 * d["cold_value"]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full: the headline only (no companion runs, no CPU baseline), exactly --steps timed steps, and with
    --dump-outputs what the last timed step computed, as float64 arrays of at most 64 MB in all."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--cells", "40",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "DOF/s (assembly+CG-to-tol)" and d["unit"] == "DOF/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (1, 3, 1) and d["converged_reason"] == 2
    assert d["value"] > 0 and abs(d["value"] - d["config"]["free_dofs"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not {"roofline", "cpu_baseline", "jacobi_step", "parity_tolerance_step", "max_nodal_error"} & set(d)
    files = {f: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(files) == {"solution.npy", "rhs.npy", "matrix_values.npy", "solve.npy"}
    assert all(a.dtype == np.float64 for a in files.values()) and sum(os.path.getsize(tmp_path / f) for f in files) <= 64e6
    assert files["solution.npy"].size == files["rhs.npy"].size == d["config"]["free_dofs"] == 39 ** 3
    assert list(files["solve.npy"][:2]) == [d["iterations"], d["converged_reason"]] and files["solve.npy"][2] == d["rnorm"]
    # u = x^2+y^2+z^2 is nodally exact on this mesh: the dumped solution is the converged answer
    x = np.linspace(-1, 1, 41)[1:-1]
    exact = (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2).ravel()
    assert np.abs(files["solution.npy"] - exact).max() < 1e-3


def test_bench_rejects_what_it_cannot_time_or_dump():
    """--steps sets the number of timed steps, so it must be at least 1; --dump-outputs writes one GPU's arrays."""
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "out"], ["--mode", "compat", "--dump-outputs", "out"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 2 and "error" in r.stderr and not r.stdout.strip(), (bad, r.stderr[-500:])


@pytest.mark.gpu
def test_bench_two_ranks_sharing_the_device():
    """The N > 1 code path of bench.py (per-rank device-generated slab, neighbour plan, exchange, comm report) with two
    ranks on cuda:0 over gloo host hooks -- the launch line is the driver's, only backend and placement differ."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--cells", "40", "--backend", "gloo", "--same-device", "--simulate-rccl-failure", "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["converged_reason"] == 2 and d["max_nodal_error"] < 1e-3 and d["scaling"] == "weak"
    # (the run also went through bench.py's safety net: a rank reported RCCL unusable, all ranks fell back together to host
    # hooks over a gloo subgroup)
    c = d["comm"]
    assert c["transport"] == "gloo-host-hooks" and "RCCL was not usable" in c["fallback_reason"] and c["rccl_comm_count"] == -1
    side = round(40 * 2 ** (1 / 3))
    assert d["config"]["free_dofs"] == (side - 1) ** 3
    assert d["config"]["partition"]["axis"] == "z" and sum(d["config"]["partition"]["hex_layers_per_rank"]) == side
    assert c["neighbours"] == 1 and c["bytes_per_neighbour"] == 8 * (side - 1) ** 2 and c["samples"] > 0
    assert 0 < c["boundary_slices"] < c["slices"] and c["interface_exchange_ms"] > 0 and c["scalar_allreduce_ms"] > 0
    # what the ONE 8-GPU run of the driver has to answer, filled here with two ranks sharing the device:
    # all three headline rates, the links' latencies at the message sizes of configs 4 / 5, the coupled cycle's exchanges per
    # level with their times, the multigrid's phase times, and the same steps over the other device-side transport
    assert d["value"] > 0 and d["cold_value"] > 0 and d["jacobi_step"]["ms_per_step"] > d["ms_per_step"]
    ll = c["link_latencies"]
    assert ll["transport"] == "host" and all(ll[k] > 0 for k in ("exchange_62KB_with_slab_neighbours_us", "exchange_1.29MB_with_slab_neighbours_us",
                                                                 "allreduce_3_doubles_us", "allreduce_125000_doubles_us"))
    cc = c["coupled_cycle"]
    nl = d["preconditioner"]["levels"]
    assert cc["cycle_ms"] > 0 and len(cc["exchanges_per_level"]) >= 2 and sum(cc["exchanges_per_level"]) == d["preconditioner"].get("exchanges_per_cycle", sum(cc["exchanges_per_level"]))
    assert all((n == 0) == (t == 0.0) for n, t in zip(cc["exchanges_per_level"], cc["exchange_ms_per_level"])) and nl >= 2
    assert d["preconditioner"]["symbolic_setup_ms_once_per_pattern"] > 0 and d["preconditioner"]["numeric_setup_ms_per_solve_inside_the_timer"] > 0
    tr = c["transports"]
    assert set(tr) == {"gloo-host-hooks", "peer-ipc", "note"}
    pe = tr["peer-ipc"]
    assert "skipped" not in pe, pe
    assert pe["converged_reason"] == 2 and abs(pe["iterations"] - d["iterations"]) <= 1 and pe["link_latencies"]["transport"] == "peer-ipc"
    assert pe["coupled_cycle"]["exchanges_per_level"] == cc["exchanges_per_level"]
    assert pe["host_enqueue_us_per_iteration"] < 0.5 * c["host_enqueue_us_per_iteration"]       # its cycle replays from a hipGraph


@pytest.mark.gpu
def test_config5_at_full_size_with_eight_ranks_sharing_the_device():
    """BASELINE configs[4] -- the 400x400x400x6 cube (384 M tets, 63.5 M free dofs) on 8 ranks -- functionally and at full
    size: eight processes, one per GPU, exchange through gloo host hooks, and solve the whole problem.  Not a performance
    figure; it pins the per-rank device generator, the neighbour plan (one or two faces of 399^2 dofs), the relative-row-group
    SpMV with a table of the large gaps that slabs of this size need, and the multi-rank loop at the size the scaling run uses."""
    import socket
    _skip_unless_eight_gpus()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--no-transport-ab", "--steps", "1", "--warmup", "0",
                        "--backend", "gloo", "--pc", "jacobi", "--full"], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert d["config"]["free_dofs"] == 63521199 and d["config"]["elements"] == 384000000 and d["n_gpus"] == 8
    assert d["converged_reason"] == 2 and abs(d["iterations"] - 720) <= 5 and d["max_nodal_error"] < 3e-4
    sc = d["strong_cfg5"]               # N = 8: the weak configuration IS config 5 -- the same run, read against one GPU
    assert sc["is_baseline_config5"] and sc["same_run_as_value"] and sc["single_gpu_ms_per_step"] > 1000 and sc["preconditioner"] == "jacobi"
    assert abs(sc["speedup_vs_single_gpu"] - sc["single_gpu_ms_per_step"] / d["ms_per_step"]) < 1e-9
    c = d["comm"]
    assert len(c["ranks"]) == 8 and c["distinct_devices"] == 8 and [r["layers"] for r in c["ranks"]] == [[50 * r, 50 * r + 50] for r in range(8)]
    assert c["bytes_per_neighbour"] == 8 * 399 ** 2 and c["neighbours"] == 1            # rank 0: one face
    # dictionary form of the column gaps -- and of the VALUES: a slab of the structured box repeats its element matrices
    assert "k_spmvr_vd<true, true>" in d["roofline"]["kernel"] and "table of the" in d["roofline"]["kernel"]
    assert 0 < d["roofline"]["value_dictionary_entries"] <= 4096


@pytest.mark.gpu
def test_config5_at_full_size_alone_on_one_device():
    """BASELINE configs[4] solved by ONE rank on one MI355X (288 GB): 63.5 M free dofs, 949 M nonzeros, 6.1e9
    element-matrix entries -- more than one sort call indexes, so the pattern comes from element ranges.  Same problem
    as the eight-rank test above: the same answer (nodal error of the %.8f boundary data), the same iteration count to
    a few (one rank sums in a different order than eight), and the strong-scaling baseline of SURVEY 8(e)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cells", "400", "--steps", "1", "--warmup", "0",
                        "--no-cpu-baseline", "--pc", "jacobi", "--full"], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert d["config"]["free_dofs"] == 63521199 and d["config"]["elements"] == 384000000 and d["n_gpus"] == 1
    assert d["converged_reason"] == 2 and abs(d["iterations"] - 720) <= 2 and d["max_nodal_error"] < 3e-4
    # the parity setting at full size: rtol 1e-10 leaves only the error of the "%.8f" boundary data
    pt = d["parity_tolerance_step"]
    assert pt["converged_reason"] == 2 and pt["max_nodal_error"] < 2e-7 and 1250 < pt["iterations"] < 1400
    assert d["roofline"]["nnz"] == 949001947 and "table of the" in d["roofline"]["kernel"]


@pytest.mark.gpu
def test_config5_with_the_default_solver():
    """BASELINE configs[4] with the solver `bench.py` runs by default (-pc_type gamg), alone on one device: 13 iterations
    (720 with point Jacobi), the converged answer at rtol 1e-10 within the error of the "%.8f" boundary data."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cells", "400", "--steps", "1", "--warmup", "1",
                        "--no-cpu-baseline", "--no-jacobi-step", "--full"], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert d["config"]["free_dofs"] == 63521199 and d["preconditioner"]["name"] == "gamg" and d["converged_reason"] == 2
    assert d["iterations"] <= 15 and d["max_nodal_error"] < 1e-3
    assert d["preconditioner"]["rows_per_level"][:3] == [399 ** 3, 200 ** 3, 100 ** 3]
    pt = d["parity_tolerance_step"]
    assert pt["converged_reason"] == 2 and pt["max_nodal_error"] < 2e-7 and pt["iterations"] <= 40


@pytest.mark.gpu
def test_config5_with_the_default_solver_on_eight_gpus():
    """BASELINE configs[4] with the default solver on 8 ranks, one per GPU: 15 iterations across the eight ranks (one
    hierarchy across them), against 13 alone (test_config5_with_the_default_solver)."""
    _skip_unless_eight_gpus()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--no-transport-ab", "--backend", "gloo", "--steps", "1",
                        "--warmup", "0", "--no-jacobi-step", "--no-parity-step", "--full"], capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d8 = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert d8["config"]["free_dofs"] == 63521199 and d8["n_gpus"] == 8 and d8["converged_reason"] == 2
    assert d8["preconditioner"]["hierarchy"] == "one across the ranks" and d8["iterations"] <= 17 and d8["max_nodal_error"] < 1e-3


@pytest.mark.gpu
def test_strong_scaling_flag_keeps_the_problem():
    """`--strong`: N ranks solve the problem one rank solves (here 60^3 on 1 and on 2 ranks sharing the device): same
    free dofs, the same answer, "scaling": "strong"; and the line reports the device memory in use."""
    import socket
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cells", "60", "--steps", "1", "--warmup", "0",
                          "--no-cpu-baseline", "--no-parity-step", "--pc", "jacobi", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-3000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.strip().startswith("{")][-1])
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-transport-ab", "--cells", "60", "--strong",
                          "--steps", "1", "--warmup", "0", "--backend", "gloo", "--same-device", "--no-cpu-baseline", "--no-parity-step", "--pc", "jacobi",
                          "--full"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-3000:]
    d2 = json.loads([ln for ln in two.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert d1["config"]["free_dofs"] == d2["config"]["free_dofs"] == 59 ** 3
    assert (d1["scaling"], d2["scaling"], d2["n_gpus"]) == ("weak", "strong", 2)
    assert d1["converged_reason"] == d2["converged_reason"] == 2 and abs(d1["iterations"] - d2["iterations"]) <= 2
    assert abs(d1["max_nodal_error"] - d2["max_nodal_error"]) < 1e-6
    m = d1["device_memory_gb"]
    assert 0 < m["in_use_rank0_device"] < m["total"] and m["total"] > 200


@pytest.mark.gpu
def test_plain_invocation_with_two_gpus_launches_its_own_ranks():
    """`python bench.py --gpus 2 ...` with no launcher and no WORLD_SIZE -- the form the driver uses for N = 1 -- must
    work for N > 1: the parent starts the ranks itself (before touching the GPU), relays their ONE JSON line and returns
    their exit code.  The line says what carried the run and how to read it: transport and rank count, every rank's
    device, per-iteration efficiency, and the strong-scaling companion block."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-transport-ab", "--same-device", "--backend", "gloo", "--cells", "40",
                        "--full"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["converged_reason"] == 2 and d["scaling"] == "weak" and d["steps"] == 5 and d["warmup"] == 3
    c = d["comm"]
    assert c["transport"] == "gloo-host-hooks" and c["fallback_reason"] is None and c["spmv_form"] == "in order"
    assert [(x["rank"], x["device_index"], x["solver_device"]) for x in c["ranks"]] == [(0, 0, 0), (1, 0, 0)]
    assert len({x["pid"] for x in c["ranks"]}) == 2 and c["distinct_devices"] == 1
    assert d["preconditioner"]["name"] == "gamg" and d["preconditioner"]["hierarchy"] == "one across the ranks" and d["jacobi_step"]["iterations"] > 2 * d["iterations"]
    e = d["per_iteration_efficiency"]
    assert e["value"] > 0 and e["n1_free_dofs"] == 7880599 and "profiles/r0" in e["n1_source"]
    sc = d["strong_cfg5"]
    assert sc["free_dofs"] == 79 ** 3 and not sc["is_baseline_config5"] and sc["speedup_vs_single_gpu"] is None
    assert sc["converged_reason"] == 2 and sc["n_gpus"] == 2 and sc["max_nodal_error"] < 1e-3 and not sc["same_run_as_value"]


@pytest.mark.gpu
def test_plain_invocation_reports_a_dead_rank_with_its_exit_code():
    """A rank that dies must end the job with a non-zero exit code and no result line -- promptly, not after a hung
    collective times out (rank 1 exits right after the rendezvous; the launcher tears the other rank down)."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-transport-ab", "--same-device", "--backend", "gloo", "--cells", "20",
                        "--steps", "1", "--warmup", "0", "--debug-die-rank", "1", "--bringup-timeout", "60"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode != 0 and not [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert time.time() - t0 < 300


@pytest.mark.gpu
def test_beam_on_eight_ranks_is_cut_across_its_length():
    """BASELINE configs[3] on 8 ranks (one per GPU, gloo host hooks): the 50x300x50 beam is cut
    across y -- 37/38 hex layers per rank, faces of 51x51 nodes = 62 KB per neighbour -- not into 6-7
    z-layers with 368 KB faces; the default solve (one multigrid hierarchy across the eight ranks) converges to the same tip
    displacement in about the iterations the one-GPU hierarchy needs (18), a small fraction of point Jacobi's 5 207."""
    _skip_unless_eight_gpus()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--no-transport-ab", "--backend", "gloo",
                        "--workload", "beam", "--steps", "1", "--warmup", "0", "--no-jacobi-step", "--no-parity-step", "--full"],
                       capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    pt = d["config"]["partition"]
    assert pt["axis"] == "y" and sorted(set(pt["hex_layers_per_rank"])) == [37, 38] and sum(pt["hex_layers_per_rank"]) == 300
    assert pt["face_nodes"] == 51 * 51 and pt["face_bytes_per_neighbour"] == 51 * 51 * 3 * 8 == 62424
    assert d["config"]["free_dofs"] == 2340900 and d["scaling"] == "strong" and d["converged_reason"] == 2
    # (23 iterations when measured, with the rigid-body modes of every aggregate in the coarse space -- 18 on one GPU; 181 with
    # translations only in round 3; block Jacobi over the eight slabs, one hierarchy per slab, needed 763)
    assert d["preconditioner"]["name"] == "gamg" and d["preconditioner"]["hierarchy"] == "one across the ranks" and d["iterations"] <= 30
    # rank 0 holds the clamped end: its owned rows move little; the line reports the owned maximum
    assert 0 < d["max_displacement_magnitude_owned_rows"] < 0.83

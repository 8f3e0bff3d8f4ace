#!/usr/bin/env python3
"""Benchmark of the hot path: full forward-difference Jacobian sweeps of the NLP callbacks.

    python bench.py --gpus N --steps K --warmup W

N > 1 runs one process per GPU over RCCL: under a launcher (``python -m torch.distributed.run --nproc-per-node N
bench.py --gpus N ...``: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment) or, when WORLD_SIZE is
not set, by launching itself that way (``--standalone --local-addr 127.0.0.1``).  ``--single-process`` instead
drives the N devices from ONE process (``og_comm_init`` + ``og_multi_fd_sweep_enqueue``: ncclCommInitAll and a
grouped all-gather; no launcher at all).  ``OG_BENCH_SAME_DEVICE=1`` puts every rank / sub-handle on device 0 (a
dry run of the N > 1 plumbing on a one-GPU box: the exchange then goes through host staging / peer copies and
the line says so).

One *step* = one SLSQP major iteration's worth of callback work at a fixed point x0 that is
already resident in HBM: F(x0) plus the n forward-difference columns of
[cost | c_eq | c_ineq], left in HBM as the transposed Jacobian (n x m, float64).  The
reference spends 3n+2 Python callback evaluations on this, so
``value`` = (3n+2) * K / elapsed  [NLP-callback evals/s], BASELINE.json's metric, and ``ms_per_step`` =
elapsed / K.  The timed region is exactly K steps (barrier + synchronize on both sides, MAX over ranks); with
``--reps R`` it is repeated R times and the median repetition is reported, with min and max next to it.

A plain run does only what that line needs: set-up, W warm-up steps, the K timed steps and the line.
``--dump-outputs DIR`` also writes what the last timed step computed (``DIR/F.npy``: F(x0), ``DIR/JT.npy``: the
transposed Jacobian, float64; a seeded sample of its rows above 64 MB) - the inputs are the same from run to run,
so two builds can be compared output for output.  ``--full`` adds everything else described below (and makes
``--reps`` 25 unless it is given).

Workload: BASELINE.json's target configuration, the 2-phase / 6-state / 3-control /
80-node-per-phase polar ascent (``polar_tsto``, C3, n = 1442).  Output goes to registered persistent-zero
buffers (``og_jt_register_dev``) used in rotation (> 256 MB together, so the Infinity Cache does not serve one
step what the previous one left).  With N > 1 ranks the columns are split in contiguous blocks (strong scaling -
total work is fixed) and every rank's replica is completed by ONE RCCL all-gather of the packed non-zeros per
step (``opengoddard_amd/sharding.py``).

Extra objects on the JSON line of a ``--full`` run: ``roofline`` (the one launch that does evaluation + sweep, ``ogk_fused``,
against the HBM roofline: algorithmic bytes 8*[(n+1)n + m n + sum N_i^2] per launch, duration from HIP events on
the launch stream, also as a fraction of a fill peak measured in this run); ``cpu_baseline`` (the NumPy
restatement of the reference path, serial, 1 core), ``cpu_baseline_all_cores`` (its column loop over every host
core) and ``cpu_baseline_batch_last`` (one vectorised NumPy evaluation of all columns) - ``oracle/cpu_baselines.py``,
rank 0, N = 1 only; ``self_check`` (the buffers equal a literal dense sweep bit for bit); ``dense_sweep_ms``;
``host_api_ms_per_sweep`` (the PCIe-inclusive host-pointer path ``Problem.solve`` uses).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
DEPENDENT_CHAIN_US = 3.6       # ogk_fused at C3: first request -> last store issued, from the in-kernel stamps of every
                               # wavefront (tools/trace_fused.py, profiles/r02_trace_fused_polar_tsto.txt)


def cpu_baseline(name, mode, seconds=10.0, nodes=None):
    """One CPU baseline (oracle/cpu_baselines.py: ``serial`` = the reference's own way, ``all_cores`` = its
    column loop dealt to every host core, ``batch_last`` = one vectorised NumPy evaluation of all columns),
    in a process of its own: never the measured product, and no HIP state is forked into the workers."""
    import subprocess
    cmd = [sys.executable, "-m", "oracle.cpu_baselines", "--workload", name, "--mode", mode, "--seconds", str(seconds)]
    if nodes:
        cmd += ["--nodes", nodes]
    try:
        proc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              timeout=60 + 8 * seconds)
        return json.loads(proc.stdout.strip().splitlines()[-1])
    except Exception as exc:                                   # a missing baseline must not lose the GPU line
        return {"value": None, "unit": "callback evals/s", "cores": None, "kind": "port", "sample": "failed: %r" % (exc,)}


def compiled_loop_context(name, nodes=None):
    """Context only: the same dense column loop as compiled C++ (oracle/twin.cpp, one core) - how much of the
    GPU/NumPy ratio is Python interpreter overhead rather than arithmetic."""
    try:
        import numpy as np
        from opengoddard_amd import _native, problems
        from oracle import np_path, twin
        prob, obj = problems.build(name, **({"nodes": [int(v) for v in nodes.split(",")]} if nodes else {}))
        lb, ub = np_path.bounds_arrays(prob)
        x0 = np.clip(prob.p, lb, ub)
        tw = twin.Twin(prob, obj)
        h = _native.fd_step(x0, lb, ub)
        cols = np.arange(min(x0.size, 256))
        tw.sweep(x0, h, cols[:8])
        t0 = time.perf_counter()
        tw.sweep(x0, h, cols)
        return 3 * (cols.size + 1) / (time.perf_counter() - t0)
    except Exception:
        return None


def measured_traffic(workload, kernel, custom_size):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes of THIS
    workload at its registered size (profiles/rNN_traffic.json, made by tools/summarize_profiles.py; FETCH_SIZE
    doubled as MI355X_MICROARCH.md prescribes for gfx950).  None when the workload was not profiled, or when the
    run uses another size (--nodes) than the profile."""
    import glob
    if custom_size:
        return None
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json"))):
        try:
            with open(path) as fh:
                entry = json.load(fh).get(workload, {}).get(kernel)
        except (OSError, ValueError):
            continue
        if entry and entry.get("hbm_bytes_per_launch"):
            best = {"bytes": entry["hbm_bytes_per_launch"], "source": os.path.basename(path),
                    "mfma": {k: entry[k] for k in ("mfma_f64_instructions_per_launch", "mfma_busy_cycles_per_launch",
                                                   "mfma_util_pct") if k in entry}}
    return best


def committed_rocprof_average(workload, kernel, custom_size):
    """Average duration (us) of the dominant kernel in the newest committed ``rocprofv3 --kernel-trace --stats`` summary
    of THIS workload (profiles/rNN_kernel_stats_<workload>.csv): the figure the live HIP-event mean has to agree with."""
    import csv
    import glob
    if custom_size:
        return None
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_stats_%s.csv" % workload))):
        try:
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    if kernel + "(" in row.get("Name", ""):
                        best = {"average_us": float(row["AverageNs"]) * 1e-3, "calls": int(row["Calls"]),
                                "source": os.path.basename(path)}
        except (OSError, ValueError, KeyError):
            continue
    return best


def measured_chain(name, nodes=None):
    """The dependent chain INSIDE one launch of this workload's ``ogk_fused``, measured in this run (not a
    constant of C3): the kernel module is rebuilt with in-kernel ``s_memrealtime`` stamps (-DOGK_TRACE=1, a module of its
    own next to the product's), 30 launches are stamped, and the figure is `the fastest complete workgroup of the slowest
    kind` - per kind of workgroup (evaluation, light, heavy part, MFMA tile) the smallest (last stamp - first start) over
    its workgroups, i.e. the least contended instance of that chain, then the largest over the kinds: no launch of this
    dependency structure ends sooner.  In a process of its own (tools/trace_fused.py --json)."""
    import subprocess
    env = dict(os.environ, OG_MODULE_HIPFLAGS="-DOGK_TRACE=1", OGPSX_TRACE="1", OGPSX_SWEEP="fused")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "trace_fused.py"), name, "--json"] + (["--nodes", nodes] if nodes else [])
    try:
        proc = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        return json.loads(proc.stdout.strip().splitlines()[-1])
    except Exception as exc:
        return {"chain_us": None, "error": repr(exc)}


def cold_start(name, nodes=None):
    """What a NEW problem shape pays before its first sweep (the reference starts iterating at once,
    ``optimize.py:649-755``): trace the callbacks, generate the device header, compile the kernel module with hipcc
    (forced: the cached module of this workload is ignored), load it and create the handle.  In a process of its
    own, so that nothing of this run's state helps."""
    import subprocess
    code = ("import json, sys, time; t0 = time.perf_counter(); "
            "from opengoddard_amd import build, codegen, problems; from opengoddard_amd.engine import HipEngine; "
            "kw = {'nodes': [int(v) for v in sys.argv[2].split(',')]} if sys.argv[2] else {}; "
            "prob, obj = problems.build(sys.argv[1], **kw); t1 = time.perf_counter(); "
            "P = codegen.trace_problem(prob, obj); hdr = codegen.emit_header(P); t2 = time.perf_counter(); "
            "build.build_module(hdr, force=True, out_suffix='.cold'); t3 = time.perf_counter(); "
            "eng = HipEngine(prob, obj, program=P); t4 = time.perf_counter(); "
            "import numpy as np; from opengoddard_amd import _native; "
            "lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float); "
            "ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float); x = np.clip(prob.p, lb, ub); "
            "F, JT = eng.sweep_stacked(x, _native.fd_step(x, lb, ub)); t5 = time.perf_counter(); "
            "print(json.dumps({'import_and_problem_s': t1 - t0, 'trace_and_codegen_s': t2 - t1, 'hipcc_s': t3 - t2, "
            "'load_and_create_s': t4 - t3, 'first_sweep_s': t5 - t4, 'total_s': t5 - t0}))")
    try:
        proc = subprocess.run([sys.executable, "-c", code, name, nodes or ""], cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, timeout=600)
        return json.loads(proc.stdout.strip().splitlines()[-1])
    except Exception as exc:
        return {"total_s": None, "error": repr(exc)}


def fill_and_copy_peaks(torch, dev):
    """What this very GPU sustains on a long stream, measured in this run: a 1 GiB fill (write only) and a
    1 GiB device-to-device copy (read + write), GB/s."""
    size = 1 << 27                                             # doubles: 1 GiB
    a = torch.empty(size, dtype=torch.float64, device=dev)
    b = torch.empty(size, dtype=torch.float64, device=dev)
    out = {}
    for label, op, nbytes in (("fill", lambda: a.zero_(), 8 * size), ("copy", lambda: b.copy_(a), 16 * size)):
        for _ in range(2):
            op()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            op()
        e1.record()
        torch.cuda.synchronize()
        out[label] = 5 * nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9
    del a, b
    return out


DUMP_LIMIT_BYTES = 64 * 2 ** 20


def write_outputs(folder, F, JT):
    """``--dump-outputs``: F(x0) (m) and the transposed Jacobian (n x m) of the last timed step as float64 ``.npy``
    files, so that two builds can be compared output for output.  Above 64 MB together, JT.npy holds a fixed sample of
    its rows (seeded; it depends on n and m only) in ascending order, and sample_rows.npy their indices."""
    import numpy as np
    import torch
    os.makedirs(folder, exist_ok=True)
    n, m = int(JT.shape[0]), int(JT.shape[1])
    rows = None
    if 8 * (n * m + m) > DUMP_LIMIT_BYTES:
        keep = max(1, (DUMP_LIMIT_BYTES - 8 * m) // (8 * (m + 1)))
        rows = np.sort(np.random.default_rng(20261016).choice(n, size=min(n, keep), replace=False))
        JT = JT.index_select(0, torch.as_tensor(rows, device=JT.device)) if torch.is_tensor(JT) else JT[rows]
    out = {"F": F, "JT": JT}
    for name, value in out.items():
        value = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
        np.save(os.path.join(folder, name + ".npy"), np.ascontiguousarray(value, dtype=np.float64))
    if rows is not None:
        np.save(os.path.join(folder, "sample_rows.npy"), rows.astype(np.float64))
    return sorted(out) + (["sample_rows"] if rows is not None else [])


def sqp_first_qp_parity(eng, prob, lb, ub):
    """The first QP subproblem of the SQP leg (B = I, the Jacobian the sweep kernel leaves in HBM) solved by the HIP
    core and by the CPU restatement (oracle/slsqp_np.py, LAPACK LQ) - the checker, not the thing measured.  An
    inconsistent linearisation (mode 4: C3 starts with one) is compared on the relaxed problem, as the driver
    solves it.  Returns what was compared; ``parity_checked`` is True only if everything asserted here held."""
    import numpy as np
    from opengoddard_amd import _native, _sqp_native
    from oracle import slsqp_np
    x = np.clip(prob.p, lb, ub)
    F0, JT = eng.sweep_stacked(x, _native.fd_step(x, lb, ub))
    n, meq = eng.n, eng.m_eq
    g, A, c = JT[:, 0].copy(), JT[:, 1:].T.copy(), F0[1:]
    t0 = time.perf_counter()
    ref = slsqp_np.qp_solve(np.eye(n), g, A[:meq], c[:meq], A[meq:], c[meq:], lb - x, ub - x, lq="lapack")
    core = _sqp_native.QpCore(n, meq, eng.m_ineq, device=eng.device)
    d, mult, bm, status, iters = core.solve(A, g, c, lb - x, ub - x)
    relaxed = False
    assert status == ref[3], "first QP: exit mode %d, restatement %d" % (status, ref[3])
    if status == 4:
        relaxed = True
        Za = np.eye(n + 1)
        Za[n, n] = 1.0 / 100.0
        extra = np.concatenate([-c[:meq], np.maximum(-c[meq:], 0.0)])
        Aa = np.hstack([A, extra[:, None]])
        lo, hi = np.append(lb - x, 0.0), np.append(ub - x, 1.0)
        ref = slsqp_np.qp_solve(Za, np.append(g, 0.0), Aa[:meq], c[:meq], Aa[meq:], c[meq:], lo, hi, lq="lapack")
        core.set_active()
        d, mult, bm, status, iters = core.solve(A, g, c, lo, hi, True, 100.0)
        assert status == ref[3] == 1, "relaxed first QP: exit mode %d, restatement %d" % (status, ref[3])
    hip_active = sorted(int(v) for v in core.get_active())
    core.close()
    # the referee (oracle/qp_referee.py): the exact step of THIS subproblem on the reported active set, by iterative
    # refinement with np.longdouble residuals - how far each of the two solvers is from it
    from oracle import qp_referee
    mg = A.shape[0] - meq
    ref_active = sorted(j if kind == "g" else mg + 2 * j + (1 if kind == "u" else 0) for kind, j in ref[5]["active"])
    if relaxed:
        Zr, gr, Ar, lor, hir = Za, np.append(g, 0.0), Aa, lo, hi
    else:
        Zr, gr, Ar, lor, hir = np.eye(n), g, A, lb - x, ub - x
    dist, _, rinfo = qp_referee.distances(Zr, gr, Ar, c, lor, hir, meq, ref_active, {"hip": d, "restatement": ref[0]})
    scale = max(1.0, float(np.abs(ref[0]).max()))
    step_err = float(np.max(np.abs(d - ref[0])) / scale)
    # vertex solutions at these sizes are ill-conditioned (tests/test_slsqp_core.py measures the amplification):
    # two exact solvers agree to ~1e-7 of the step, not to 1e-11
    assert step_err <= 1e-6, "first QP: step differs from the restatement by %.3g of its size" % step_err
    assert abs(iters - ref[5]["ldp_iterations"]) <= max(2, ref[5]["ldp_iterations"] // 100)
    return {"parity_checked": True, "first_qp_relaxed": relaxed, "first_qp_exit_mode": int(status),
            "first_qp_step_error_rel": step_err, "first_qp_active_set_changes": int(iters),
            "first_qp_active_set_changes_restatement": int(ref[5]["ldp_iterations"]),
            "first_qp_same_active_set": hip_active == ref_active,
            "first_qp_distance_to_refined_solution": {"hip": dist["hip"], "restatement": dist["restatement"],
                                                      "active_rows": rinfo["active_rows"],
                                                      "referee_converged_to": max(rinfo["step_moved"][-3:]),
                                                      "referee": "oracle/qp_referee.py (np.longdouble residuals)"},
            "checker": "oracle/slsqp_np.py qp_solve (LAPACK LQ), %.1f s of CPU" % (time.perf_counter() - t0)}


def sqp_leg(eng, prob, iterations, reference_iterations=0, check_first_qp=True):
    """Second BASELINE metric, "wall-clock to SLSQP convergence", on a bounded sample: the first
    ``iterations`` major iterations of ``Problem.solve`` with the QP subproblems on the GPU
    (``sqp_core="hip"``), split into callbacks / QP / BFGS.  The same iterations with SciPy's Fortran
    core take 8 s each at n = 1442 (profiles/r01_solve_timing.jsonl), which is why they are not
    re-timed in every bench run."""
    import numpy as np
    from opengoddard_amd import sqp
    lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
    ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
    t0 = time.perf_counter()
    res = sqp.minimize_slsqp_hip(eng, prob.p.copy(), lb, ub, ftol=1e-6, maxiter=iterations + 1)
    wall = time.perf_counter() - t0
    t = res.timing
    out = _sqp_result(res, wall, t, iterations)
    if check_first_qp:
        try:
            out.update(sqp_first_qp_parity(eng, prob, lb, ub))
        except AssertionError as exc:
            out.update({"parity_checked": False, "parity_failure": str(exc)})
    else:
        out.update({"parity_checked": None, "parity_note": "the CPU checker of the first subproblem takes minutes at this size: "
                    "tests/test_slsqp_core.py::test_gpu_first_subproblem_of_the_baseline_configurations runs it"})
    out["recoveries"] = int(t.get("recoveries", 0))
    if reference_iterations > 0:
        out["scipy_core"] = scipy_core_sample(eng, prob, lb, ub, reference_iterations)
        out["speedup_per_major_iteration"] = (out["scipy_core"]["ms_per_major_iteration"] /
                                              out["ms_per_major_iteration"])
    return out


def scipy_core_sample(eng, prob, lb, ub, iterations):
    """The same solve with SciPy's Fortran SLSQP core (GPU callbacks and Jacobians, as
    Problem.solve(sqp_core="scipy") runs it), for ``iterations`` major iterations: the measured
    baseline of the SQP leg on this machine."""
    import numpy as np
    from scipy import optimize
    import warnings

    def fun(which):
        return lambda p: eng.values(p)[which]

    def jac(which):
        return lambda p: eng.jacobians(p, lb, ub)[0][which]

    cons = ({"type": "eq", "fun": fun(1), "jac": jac(1)}, {"type": "ineq", "fun": fun(2), "jac": jac(2)})
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = optimize.minimize(fun(0), prob.p.copy(), jac=jac(0), bounds=list(zip(lb, ub)), constraints=cons,
                                method="SLSQP", options={"maxiter": iterations + 1, "ftol": 1e-6})
    wall = time.perf_counter() - t0
    done = max(1, int(res.nit) - 1)
    return {"core": "scipy %s _slsqp (Fortran)" % __import__("scipy").__version__, "major_iterations": done,
            "wall_s": wall, "ms_per_major_iteration": 1e3 * wall / done}


# what the `solve` leg runs (the reference's loop, ``optimize.py:738-755``: restarts of ``maxiter`` major iterations
# until SLSQP reports exit mode 0): C3 with 400 iterations per restart (the reference's default of 25 resets the
# quasi-Newton matrix too often for this size to converge inside maxIterator restarts); C4 likewise since round 6 - with
# 25 iterations per restart its ten restarts end by SLSQP's cost test or by their limit depending on rounding (3 of 5
# neighbouring starts, and the problem's own start after the LQ panel's sums changed order), with 400 it needs ~130
# major iterations and no restart
SOLVE_OPTIONS = {"polar_tsto": {"maxiter": 400}, "low_thrust": {"maxiter": 400}, "launch4": {"maxiter": 3000},
                 "goddard": {"ftol": 1e-10}}


def solve_leg(name, options=None, check=True, perturb_seed=None, start=None, max_restarts=None):
    """Second half of BASELINE.json's metric, measured whole: ``Problem.solve`` (this package's, default SQP core = the
    HIP one at these sizes) from the problem's own initial guess to SLSQP's exit mode 0 - wall-clock of the call, split
    into callbacks (values + Jacobians), QP subproblems and BFGS updates - and, NOT timed, the independent check of
    what it returned: the KKT residuals of the reference's NLP at the returned point, every number of which comes from
    the NumPy restatement of the reference path (oracle/kkt.py; the checker, never the thing measured)."""
    import contextlib
    import io
    from opengoddard_amd import problems
    import numpy as np
    options = dict(SOLVE_OPTIONS.get(name, {}) if options is None else options)
    prob, obj = problems.build(name)
    if start is not None:                                     # (a stored iterate instead of the problem's own guess)
        prob.p = np.array(start, dtype=float)
    if perturb_seed is not None:
        # a neighbouring start: x0 + 1e-6 N(0, 1), clipped to the bounds - the path to SLSQP's exit depends on rounding
        # (one wall-clock per configuration is not a reproducible measurement), so the leg is run from
        # several seeded starts and reported as median and range
        lo = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
        hi = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
        prob.p = np.clip(prob.p + 1e-6 * np.random.default_rng(perturb_seed).standard_normal(prob.p.size), lo, hi)
    if max_restarts is not None:
        prob.maxIterator = int(max_restarts)
    buf = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        prob.solve(obj, sqp_core="hip", **options)
    wall = time.perf_counter() - t0
    text = buf.getvalue()
    tm = prob.sqp_timings
    res = prob.last_result
    parts = {k: sum(t[k] for t in tm) for k in ("callbacks", "qp", "bfgs")}
    out = {"workload": name, "n": int(prob.number_of_variables), "options": dict(options, sqp_core="hip"),
           "exit_mode": int(res.status), "converged": bool(res.status == 0), "wall_s": wall,
           "callbacks_s": parts["callbacks"], "qp_s": parts["qp"], "bfgs_s": parts["bfgs"],
           "driver_and_python_s": wall - sum(parts.values()),
           "restarts": text.count("---- iteration"), "major_iterations_of_last_restart": int(res.nit),
           "qp_solves": int(sum(t["qp_solves"] for t in tm)),
           "active_set_changes": int(sum(t["qp_iterations"] for t in tm)),
           "recoveries": int(sum(t.get("recoveries", 0) for t in tm)), "cost": float(res.fun),
           "start": ("a stored iterate" if start is not None else "the problem's initial guess") +
                    ("" if perturb_seed is None else " + 1e-6 N(0, 1), seed %d, clipped to the bounds" % perturb_seed),
           "what": "Problem.solve(obj, **options); wall_s is the whole call (tracing, module load and handle creation "
                   "included)"}
    if tm and "resident_launches" in tm[-1]:
        out["resident_active_set"] = {"launches": int(tm[-1]["resident_launches"]), "changes": int(tm[-1]["resident_changes"]),
                                      "note": "subproblems whose active-set loop ran as ONE launch (k_rows_resident) and the "
                                              "changes those launches made, totals of the QP handle"}
    out["m_eq"] = int(prob._engine.m_eq)
    if start is not None:
        out["_x"] = np.array(res.x, dtype=float)              # (bounded_c5_leg hands it to the oracle and drops it)
    if check:
        from oracle import kkt
        t0 = time.perf_counter()
        k = kkt.residuals(prob, obj, res.x, prob._engine.m_eq)
        k["checker"] = "oracle/kkt.py on oracle/np_path.py (NumPy restatement of the reference path), %.1f s of CPU" % (
            time.perf_counter() - t0)
        out["kkt"] = k
        out["cost_by_the_oracle"] = k["cost"]
    prob._engine.close()
    return out


def solve_starts(name, starts=5, options=None, first=None):
    """The solve leg from ``starts`` neighbouring starts (the problem's own guess first, then x0 + 1e-6 N(0, 1) with seeds
    1 .. starts - 1): time to SLSQP's exit mode 0 as median and range, every start's cost and its gap to the best cost any
    of them reached.  ``first``: an already measured run from the unperturbed guess (with its KKT check)."""
    import statistics
    runs = [first if first is not None else solve_leg(name, options, check=False)]
    for seed in range(1, int(starts)):
        try:
            runs.append(solve_leg(name, options, check=False, perturb_seed=seed))
        except Exception as exc:                               # a failed start is reported, not hidden
            runs.append({"error": repr(exc), "start": "seed %d" % seed})
    done = [r for r in runs if "wall_s" in r]
    walls = sorted(r["wall_s"] for r in done)
    best = min(r["cost"] for r in done)
    return {"workload": name, "starts": len(runs), "exit_mode_0": sum(1 for r in done if r.get("exit_mode") == 0),
            "wall_s_median": statistics.median(walls), "wall_s_min": walls[0], "wall_s_max": walls[-1],
            "qp_solves_median": statistics.median(r["qp_solves"] for r in done),
            "best_cost": best,
            "per_start": [{"start": r.get("start"), "wall_s": r.get("wall_s"), "exit_mode": r.get("exit_mode"),
                           "qp_solves": r.get("qp_solves"), "active_set_changes": r.get("active_set_changes"),
                           "cost": r.get("cost"), "cost_gap_to_best": (r["cost"] - best) if "cost" in r else None,
                           "error": r.get("error")} for r in runs],
            "note": "minimisation: cost_gap_to_best >= 0; SLSQP's ftol test stops where the cost changes by less than ftol "
                    "between major iterations, which in a flat valley is path dependent (DESIGN.md section 9)"}


def bounded_c5_leg(seconds=90.0):
    """C5 (launch4, n = 6148) needs minutes from its own guess to SLSQP's exit; the line carries a bounded piece: 120 major
    iterations from a late iterate of such a solve (tests/golden/start_launch4.npz - an input made by this package's own
    solver, tools/make_start_launch4.py), and what the oracle says about the iterate SLSQP holds afterwards."""
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "start_launch4.npz")
    G = np.load(path)
    t0 = time.perf_counter()
    out = solve_leg("launch4", {"maxiter": 120}, check=False, start=G["x"], max_restarts=1)
    out["start_cost"] = float(G["cost_there"])
    out["bounded"] = "one restart of 120 major iterations from tests/golden/start_launch4.npz"
    left = seconds - (time.perf_counter() - t0)
    if left > 45.0:
        try:
            from oracle import kkt
            from opengoddard_amd import problems
            prob, obj = problems.build("launch4")
            tk = time.perf_counter()
            k = kkt.residuals(prob, obj, out.pop("_x"), out["m_eq"], max_rounds=1)
            k["checker"] = "oracle/kkt.py (max_rounds=1), %.1f s of CPU" % (time.perf_counter() - tk)
            out["kkt"] = k
        except Exception as exc:
            out["kkt"] = {"error": repr(exc)}
    out.pop("_x", None)
    return out


def _sqp_result(res, wall, t, iterations):
    return {"core": "hip (include/ogsqp.h)", "major_iterations": int(res.nit - 1 if res.status == 9 else res.nit),
            "exit_mode": int(res.status), "wall_s": wall, "callbacks_s": t["callbacks"], "qp_s": t["qp"],
            "bfgs_s": t["bfgs"], "qp_solves": t["qp_solves"], "active_set_iterations": t["qp_iterations"],
            "ms_per_major_iteration": 1e3 * wall / max(1, res.nit - 1),
            # (the first call of an engine also builds the QP work space - two n x n factors, the LQ buffers, the mailbox: a
            # cost per ENGINE, not per iteration, that a ten-iteration sample carries in full)
            "setup_s": t.get("setup"),
            "ms_per_major_iteration_without_setup": 1e3 * (wall - (t.get("setup") or 0.0)) / max(1, res.nit - 1)}


def launch_ranks(n_gpus):
    """``python bench.py --gpus N`` without a launcher: start N ranks of this script under torch.distributed.run
    (one node, rendezvous on 127.0.0.1) and hand its exit code on; rank 0 of the children prints the JSON line."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1",
           "--nproc-per-node", str(int(n_gpus)), "--local-addr", "127.0.0.1", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def single_process_bench(a):
    """N devices from one process: every step is one ``og_multi_fd_sweep_enqueue`` (x, h uploaded to every device,
    one launch per device that sweeps its column block and packs its non-zeros, ONE grouped ncclAllGather - or peer
    copies -, one scatter per device), K steps between two ``og_multi_synchronize``.  Afterwards the matrix of
    device 0 is compared bit for bit with a one-device sweep."""
    import ctypes as C
    import numpy as np
    import torch                                              # noqa: F401  (one HIP runtime in the process)
    from opengoddard_amd import _native, problems
    from opengoddard_amd.engine import HipEngine
    G = int(a.gpus)
    same = bool(os.environ.get("OG_BENCH_SAME_DEVICE"))
    if same:
        os.environ["OGPSX_GATHER"] = "peer"                   # one device listed G times: peer copies only
    devices = [0] * G if same else list(range(G))
    if not same and _native.device_count() < G:
        raise SystemExit("bench.py --single-process: %d devices wanted, %d visible" % (G, _native.device_count()))
    build_kw = {"nodes": [int(v) for v in a.nodes.split(",")]} if a.nodes else {}
    prob, obj = problems.build(a.workload, **build_kw)
    single = HipEngine(prob, obj, device=devices[0])
    multi = HipEngine(prob, obj, devices=devices) if G > 1 else single
    n, m = single.n, single.m
    lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds])
    ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds])
    x0 = np.clip(prob.p, lb, ub)
    h = _native.fd_step(x0, lb, ub)
    lib = single._lib
    if G > 1:
        xp, hp = _native.dptr(x0), _native.dptr(h)

        def run(k):
            for _ in range(k):
                _native.check(lib.og_multi_fd_sweep_enqueue(multi._multi, xp, hp), "og_multi_fd_sweep_enqueue")
            _native.check(lib.og_multi_synchronize(multi._multi), "og_multi_synchronize")
    else:
        last = [None]

        def run(k):
            for _ in range(k):
                last[0] = single.sweep_persistent(x0, h)
    run(a.warmup)
    times = []
    for _ in range(max(1, a.reps)):
        t0 = time.perf_counter()
        run(a.steps)
        times.append(time.perf_counter() - t0)
    times = np.sort(np.array(times))
    elapsed = float(np.median(times))
    if a.dump_outputs:
        # (G > 1: the grouped step leaves its result on the devices; one more step of the same path hands it to the host)
        F_out, JT_out = multi.sweep_persistent(x0, h) if G > 1 or last[0] is None else last[0]
        write_outputs(a.dump_outputs, F_out, JT_out)
    result = {
        "metric": "NLP-callback evals/sec (cost+constr+FD-Jacobian)", "value": (3 * n + 2) * a.steps / elapsed,
        "unit": "callback evals/s", "n_gpus": G, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "timed_region": {"repetitions": int(times.size), "steps_each": a.steps, "reported": "median",
                         "ms_per_step_min": float(times[0]) / a.steps * 1e3,
                         "ms_per_step_max": float(times[-1]) / a.steps * 1e3},
        "config": {"workload": "%s: %d phases, %s states, %s controls, %s LGL nodes" % (
            a.workload, len(prob.nodes), prob.number_of_states, prob.number_of_controls, prob.nodes),
            "n": n, "m_eq": single.m_eq, "m_ineq": single.m_ineq, "evals_per_step": 3 * n + 2,
            "parallelism": "fd-columns x%d from ONE process (og_multi_fd_sweep_enqueue; x and h uploaded per step; %s)" % (
                G, "devices %r" % devices + (", " + ("ncclAllGather" if lib.og_comm_uses_rccl() else "peer copies") if G > 1 else ""))},
    }
    if a.full:
        F1, J1 = single.sweep_stacked(x0, h)
        FG, JG = (multi.sweep_persistent(x0, h) if G > 1 else (F1, J1))
        equal = bool(np.array_equal(J1, JG) and np.array_equal(F1, FG))
        result["self_check"] = {"multi_device_matrix_equals_single_device_bitwise": equal}
        assert equal, "the column-sharded matrix differs from the single-device one"
    if a.full and a.sqp_iterations > 0 and n <= 3000:
        # the SQP leg on the sharded sweep: the QP core reads device d0's replica in place (sqp.DeviceJacobian) - and
        # walks the same iterates as on one device, bit for bit (the sharded matrix IS the single-device matrix)
        from opengoddard_amd import sqp
        runs = {}
        for tag, eng_ in ((("sharded", multi), ("one_device", single)) if G > 1 else (("sharded", single),)):
            t0 = time.perf_counter()
            res = sqp.minimize_slsqp_hip(eng_, prob.p.copy(), lb, ub, ftol=1e-6, maxiter=a.sqp_iterations + 1)
            runs[tag] = (res, time.perf_counter() - t0)
        res, wall = runs["sharded"]
        leg = _sqp_result(res, wall, res.timing, a.sqp_iterations)
        leg["fd_columns_sharded_over"] = int(multi._sqp_cache[0].sharded_over)
        if G > 1:
            leg["one_device_ms_per_major_iteration"] = runs["one_device"][1] / max(1, a.sqp_iterations) * 1e3
            leg["same_iterates_as_one_device"] = bool(np.array_equal(res.x, runs["one_device"][0].x))
            assert leg["same_iterates_as_one_device"], "the SQP leg on the sharded sweep left the single-device path"
        result["sqp"] = leg
    if G > 1:
        multi.close()
    single.close()
    print(json.dumps(result), flush=True)
    return 0


def physical_device_id(torch, dev):
    """What tells one GPU from another on a node: host name + the device's uuid (or its PCI address) - never the
    ordinal a process happens to see it under, and never the pid (VERDICT r5 / ADVICE r5: N ranks on one GPU must
    count as ONE device)."""
    import socket
    props = torch.cuda.get_device_properties(dev)
    parts = []
    uuid = getattr(props, "uuid", None)
    if uuid is not None and not set(str(uuid).replace("-", "")) <= {"0"} and str(uuid) not in ("", "None"):
        parts.append("uuid:" + str(uuid))
    pci = [getattr(props, f, None) for f in ("pci_domain_id", "pci_bus_id", "pci_device_id")]
    if all(v is not None for v in pci):
        parts.append("pci:%04x:%02x:%02x" % tuple(int(v) for v in pci))
    ident = "|".join(parts) or "ordinal:%d" % (dev.index if getattr(dev, "index", None) is not None else int(dev))
    return socket.gethostname() + "/" + ident


def device_census(ranks_report):
    """-> distinct_devices (physical), ranks_per_device {device: [ranks]} from the all-gathered per-rank records."""
    per = {}
    for r_ in ranks_report:
        per.setdefault(str(r_.get("physical_device", r_.get("device"))), []).append(int(r_["rank"]))
    return {"distinct_devices": len(per), "ranks_per_device": per}


def multi_gpu_verdict(result, world, same_device):
    """None when an N > 1 line may stand; otherwise why it may not (the process exits non-zero with it): every rank
    on its own physical GPU AND the exchange RCCL's own N-rank communicator - anything else measures something other
    than what the line says (OG_BENCH_SAME_DEVICE=1 is the declared dry run of the plumbing and is labelled as such)."""
    if world <= 1 or same_device:
        return None
    problems_ = []
    if result.get("distinct_devices") != world:
        problems_.append("%d ranks on %s physical device(s): %s" % (world, result.get("distinct_devices"),
                                                                     result.get("ranks_per_device")))
    if result.get("rccl_ranks") != world:
        problems_.append("the exchange is not an RCCL communicator of %d ranks (ncclCommCount reports %s)"
                         % (world, result.get("rccl_ranks")))
    return "; ".join(problems_) or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=None,
                    help="the timed region of --steps steps is repeated this often; the median repetition is reported "
                         "(default 1: exactly --steps timed steps; 25 with --full)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: roofline and kernel timings, self-checks, host API, hipGraph "
                         "replay, CPU baselines, exact Jacobian, cold start, SQP and solve legs, the BASELINE "
                         "configurations of N = 4 / 8 (the --quick / --no-* options below select among these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (F(x0): F.npy, the transposed "
                         "Jacobian: JT.npy, float64; rows of a seeded sample when above 64 MB) into DIR")
    ap.add_argument("--workload", default="polar_tsto")
    ap.add_argument("--nodes", default=None,
                    help="comma-separated LGL node counts per phase (size studies; default: the "
                         "workload's own)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--sqp-iterations", type=int, default=10,
                    help="major iterations of the SQP leg (0 = skip)")
    ap.add_argument("--sqp-reference-iterations", type=int, default=2,
                    help="major iterations of the same solve with SciPy's Fortran core, timed next to the SQP "
                         "leg (0 = skip; about 8 s each at n = 1442); skipped above n = 1600")
    ap.add_argument("--cpu-seconds", type=float, default=8.0)
    ap.add_argument("--force-collective", action="store_true",
                    help="initialise RCCL and run the all-gather even with one rank (plumbing test)")
    ap.add_argument("--quick", action="store_true",
                    help="with --full: only the timed region and the roofline (profiling runs)")
    ap.add_argument("--no-cold-start", action="store_true", help="skip the forced rebuild of the workload's kernel module")
    ap.add_argument("--no-solve", action="store_true",
                    help="skip the solve leg (Problem.solve to exit mode 0 at C3 and C4 + the oracle's KKT check: ~45 s)")
    ap.add_argument("--solve-starts", type=int, default=5,
                    help="the solve leg is run from this many neighbouring starts (x0 + 1e-6 N(0,1), seeded) and reported as "
                         "median and range (about 17 s each at C3)")
    ap.add_argument("--no-c5", action="store_true", help="skip the bounded C5 piece of the solve leg (~60 s)")
    ap.add_argument("--single-process", action="store_true",
                    help="N > 1 from ONE process: og_comm_init + og_multi_fd_sweep_enqueue over the N devices (no launcher)")
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 25 if a.full else 1
    if a.single_process:
        return single_process_bench(a)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(a.gpus)

    import numpy as np
    import torch
    from opengoddard_amd import _native, problems, sharding
    from opengoddard_amd.engine import HipEngine

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no GPU visible - the engine has no CPU path to measure")
    same_device = bool(os.environ.get("OG_BENCH_SAME_DEVICE")) and world > 1
    if same_device:
        local_rank = 0                  # dry run of the N > 1 plumbing on a one-GPU box
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    collective = world > 1 or (a.force_collective and "MASTER_ADDR" in os.environ)
    if collective:
        import torch.distributed as dist
        if same_device:
            dist.init_process_group("gloo")             # RCCL refuses two ranks on one device
        else:
            dist.init_process_group("nccl", device_id=dev)
    pg_dev = "cpu" if same_device else dev

    build_kw = {"nodes": [int(v) for v in a.nodes.split(",")]} if a.nodes else {}
    prob, obj = problems.build(a.workload, **build_kw)
    eng = HipEngine(prob, obj, device=local_rank)
    n, m = eng.n, eng.m
    lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds])
    ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds])
    x0 = np.clip(prob.p, lb, ub)
    h = _native.fd_step(x0, lb, ub)
    backend = sharding.HipBackend(eng, dev)
    if same_device:
        backend.host_staged = True
        backend.direct_note = "gloo through host staging (dry run: every rank on device 0)"
    elif collective and not os.environ.get("OG_BENCH_TORCH_ALLGATHER"):
        backend.init_direct_rccl(rank, world)       # ncclCommInitRank in libogpsx.so; falls back by itself
    d_x, d_h = backend.upload(x0), backend.upload(h)
    stream = backend.stream
    # Output buffers: every rank keeps full n x m replicas of J_T that were zeroed once; its own block of rows is
    # a registered persistent-zero buffer (og_jt_register_dev), so a step writes - and the ranks exchange - the
    # non-zeros only.  Several replicas are used in rotation so that together they exceed the 256 MB Infinity
    # Cache: consecutive steps do not hit lines the previous step left there.
    replica_bytes = 8 * n * m
    nbuf = int(min(48, max(2, -(-300 * 2 ** 20 // replica_bytes))))
    sweeps = [sharding.ShardedSweep(backend, n, m, rank, world, exchange_alone=a.force_collective) for _ in range(nbuf)]
    lo, hi = sweeps[0].lo, sweeps[0].hi
    counter = [0]

    # one pass of the hot path: F(x0) and this rank's FD columns (og_fd_sweep_dev: ONE launch, ogk_fused), then - with
    # more than one rank - pack, all-gather of the packed non-zeros (RCCL), scatter.  The calls are bound once per output
    # buffer (sharding.ShardedSweep.bound_step): a step costs the host one ctypes call (A/B against the per-step Python
    # path, OG_BENCH_UNBOUND=1, in one lease: no difference - profiles/r05_host_ab.txt; the loop is GPU-bound either way)
    bound = {flag: [sh.bound_step(d_x, d_h, gather=flag and collective) for sh in sweeps] for flag in (True, False)}
    if os.environ.get("OG_BENCH_UNBOUND"):                 # A/B: rounds 1-4's per-step Python path (slice, data_ptr, three frames)
        bound = {flag: [(lambda sh=sh, flag=flag: sh.backend.sweep(d_x, d_h, sh.lo, sh.hi, sh.replica, sh.F0)
                         if not (flag and collective) else sh.step(d_x, d_h, gather=True)) for sh in sweeps]
                 for flag in (True, False)}

    def step(gather=True):
        counter[0] += 1
        bound[gather][counter[0] % nbuf]()

    def fence():
        if collective:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_region(gather=True):
        """EXACTLY --steps steps between barrier + synchronize, --reps times; per repetition the MAX over ranks."""
        times = []
        for _ in range(max(1, a.reps)):
            fence()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(gather)
            fence()
            times.append(time.perf_counter() - t0)
        t = torch.tensor(times, dtype=torch.float64, device=pg_dev if collective else dev)
        if collective:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return np.sort(t.cpu().numpy())

    for _ in range(a.warmup):
        step()
    times = timed_region()
    elapsed = float(np.median(times))
    if a.dump_outputs and rank == 0:
        last = sweeps[counter[0] % nbuf]                # the buffer the last timed step wrote (see step())
        write_outputs(a.dump_outputs, last.F0, last.replica)
    result = {
        "metric": "NLP-callback evals/sec (cost+constr+FD-Jacobian)",
        "value": (3 * n + 2) * a.steps / elapsed,
        "unit": "callback evals/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": elapsed / a.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "timed_region": {"repetitions": int(times.size), "steps_each": a.steps, "reported": "median",
                         "ms_per_step_min": float(times[0]) / a.steps * 1e3,
                         "ms_per_step_median": elapsed / a.steps * 1e3,
                         "ms_per_step_max": float(times[-1]) / a.steps * 1e3},
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "%s: %d phases, %s states, %s controls, %s LGL nodes" % (
            a.workload, len(prob.nodes), prob.number_of_states, prob.number_of_controls, prob.nodes),
            "n": n, "m_eq": eng.m_eq, "m_ineq": eng.m_ineq,
            "evals_per_step": 3 * n + 2,
            "output_buffers": "%d registered persistent-zero replicas of %.1f MB in rotation" % (nbuf, replica_bytes / 1e6),
            "parallelism": "fd-columns x%d%s" % (world, " + RCCL all-gather of the packed non-zeros (%d bytes per rank; %s)"
                                                  % (sweeps[0].message_bytes, backend.direct_note) if collective else "")},
    }

    # ---- who took part (VERDICT r4 #8e): every rank's device as torch sees it and - when the exchange is the direct
    # ncclAllGather of libogpsx.so - what RCCL itself reports about the communicator (ncclCommCount / UserRank / CuDevice)
    ranks_report = None
    if collective:
        import ctypes as C
        mine = {"rank": rank, "local_rank": local_rank, "pid": os.getpid(), "device": int(torch.cuda.current_device()),
                "device_name": torch.cuda.get_device_name(dev), "physical_device": physical_device_id(torch, dev),
                "message_bytes": int(sweeps[0].message_bytes)}
        if getattr(backend, "direct", False):
            v = (C.c_int32 * 3)()
            if eng._lib.og_shard_comm_info(eng._handle, C.byref(v, 0), C.byref(v, 4), C.byref(v, 8)) == 0:
                mine.update({"rccl_comm_ranks": int(v[0]), "rccl_comm_rank": int(v[1]), "rccl_comm_device": int(v[2]),
                             "rccl_comm_source": "ncclCommCount of the communicator inside libogpsx.so"})
        elif not same_device and dist.get_backend() == "nccl":
            # the exchange fell back to torch.distributed's all_gather_into_tensor: its "nccl" backend IS RCCL on ROCm, and
            # the process group the ranks rendezvoused in is the communicator
            mine.update({"rccl_comm_ranks": int(dist.get_world_size()), "rccl_comm_rank": int(dist.get_rank()),
                         "rccl_comm_device": int(torch.cuda.current_device()),
                         "rccl_comm_source": "torch.distributed process group (backend nccl = RCCL)"})
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        ranks_report = everyone

    def finish(result):
        """Who took part, the validity of an N > 1 line, the JSON line; then the process group is taken down."""
        if ranks_report is not None:
            result["ranks"] = ranks_report
            counts = {r_.get("rccl_comm_ranks") for r_ in ranks_report}
            result["rccl_ranks"] = counts.pop() if len(counts) == 1 else None
            # PHYSICAL devices (host + uuid / PCI address), not (ordinal, pid) pairs: N ranks piled onto one GPU count as one
            result.update(device_census(ranks_report))
            result["message_bytes_per_rank"] = [r_.get("message_bytes") for r_ in ranks_report]
        eng.close()
        # The JSON line is the LAST thing on stdout.  RCCL prints its banner through C stdio, which a pipe buffers
        # until exit: every rank flushes that first, then all ranks meet, then rank 0 prints.
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        if collective:
            dist.barrier()
        verdict = multi_gpu_verdict(result, world, same_device) if rank == 0 else None
        if rank == 0:
            if same_device:
                result["dry_run"] = "OG_BENCH_SAME_DEVICE=1: every rank on device 0, gloo through host staging - plumbing only, measures nothing"
            if verdict:
                result["invalid"] = verdict
            print(json.dumps(result), flush=True)
        if collective:
            dist.destroy_process_group()
        if verdict:
            sys.stderr.write("bench.py: this --gpus %d line is INVALID: %s\n" % (world, verdict))
            return 3

    # a plain run ends here: set-up, warm-up, the timed steps, their outputs and the line.  Everything below is --full.
    if not a.full:
        return finish(result)

    # the same steps without the exchange: how the column-sharded kernels alone scale
    times_local = timed_region(gather=False) if collective else times
    elapsed_local = float(np.median(times_local))

    # ---- BASELINE.json quotes C4 on 4 GPUs and C5 on 8: with the driver's command (`--gpus N`, default workload) those
    # configurations get their own measurement beside the headline's - same step, same fences, fewer repetitions
    def sharded_rate(name, reps, steps, warmup):
        prob2, obj2 = problems.build(name)
        eng2 = HipEngine(prob2, obj2, device=local_rank)
        lb2 = np.array([-np.inf if b[0] is None else b[0] for b in prob2.bounds])
        ub2 = np.array([np.inf if b[1] is None else b[1] for b in prob2.bounds])
        x2 = np.clip(prob2.p, lb2, ub2)
        h2 = _native.fd_step(x2, lb2, ub2)
        be2 = sharding.HipBackend(eng2, dev)
        if same_device:
            be2.host_staged = True
        elif collective and not os.environ.get("OG_BENCH_TORCH_ALLGATHER"):
            be2.init_direct_rccl(rank, world)
        dx2, dh2 = be2.upload(x2), be2.upload(h2)
        sw2 = [sharding.ShardedSweep(be2, eng2.n, eng2.m, rank, world) for _ in range(2)]
        count = [0]

        def one():
            sw2[count[0] % 2].step(dx2, dh2, gather=collective)
            count[0] += 1
        for _ in range(warmup):
            one()
        samples = []
        for _ in range(reps):
            fence()
            t0 = time.perf_counter()
            for _ in range(steps):
                one()
            fence()
            samples.append(time.perf_counter() - t0)
        t = torch.tensor(samples, dtype=torch.float64, device=pg_dev if collective else dev)
        if collective:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        med = float(np.median(t.cpu().numpy()))
        sums = torch.stack([sh.replica.sum(dtype=torch.float64) for sh in sw2]).to(pg_dev if collective else dev)
        same = True
        if collective:
            got = [torch.empty_like(sums) for _ in range(world)]
            dist.all_gather(got, sums)
            same = all(torch.equal(g_, got[0]) for g_ in got)
        out = {"workload": "%s: %d phases, %s states, %s controls, %s LGL nodes" % (
                   name, len(prob2.nodes), prob2.number_of_states, prob2.number_of_controls, prob2.nodes),
               "n": eng2.n, "m_eq": eng2.m_eq, "m_ineq": eng2.m_ineq, "value": (3 * eng2.n + 2) * steps / med,
               "unit": "callback evals/s", "ms_per_step": med / steps * 1e3, "steps": steps, "repetitions": reps,
               "message_bytes_per_rank": int(sw2[0].message_bytes), "exchange": be2.direct_note if collective else None,
               "replicas_equal_across_ranks": bool(same)}
        del sw2
        eng2.close()
        return out

    baseline_at = {4: "low_thrust", 8: "launch4"}
    baseline_config = None
    if world in baseline_at and a.workload == "polar_tsto" and not a.nodes:
        baseline_config = sharded_rate(baseline_at[world], max(3, a.reps // 5), a.steps, max(3, a.warmup // 4))

    # duration of the dominant kernel from HIP events on the launch stream.  A single
    # event-to-event interval around one launch carries ~2 us of event overhead (an empty kernel
    # reads 6 us that way, tools/gpu_probe.hip), so the kernel is also timed in back-to-back
    # batches of 10 between two events; the batch figure is the one used for the roofline and is
    # the one that agrees with rocprofv3 --kernel-trace (profiles/).
    def timed(launch, reps, batch):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                 for _ in range(reps)]
        for _ in range(batch):                     # one untimed batch: the first launches after another phase
            launch()                               # (a collective, a different kernel) are not representative
        torch.cuda.synchronize()
        for e0, e1 in pairs:
            e0.record()
            for _ in range(batch):
                launch()
            e1.record()
        torch.cuda.synchronize()
        return np.array([e0.elapsed_time(e1) / batch for e0, e1 in pairs])

    d_F0 = sweeps[0].F0

    # (every address resolved once per buffer instead of a tensor slice and four data_ptr() per launch)
    block_ptrs = [sh.replica[lo:hi].data_ptr() if hi > lo else sh.replica.data_ptr() for sh in sweeps]
    x_ptr, h_ptr, f0_ptr = d_x.data_ptr(), d_h.data_ptr(), d_F0.data_ptr()

    def block_ptr():
        counter[0] += 1
        return block_ptrs[counter[0] % nbuf]

    def launch_sweep():
        eng.sweep_dev(x_ptr, h_ptr, lo, hi, block_ptr(), f0_ptr, stream)

    def launch_columns():
        eng.columns_dev(x_ptr, h_ptr, lo, hi, block_ptr(), f0_ptr, stream)

    def launch_eval():
        eng.eval_dev(x_ptr, f0_ptr, stream)

    fused = eng.sweep_mode == "fused"
    kernel = "ogk_fused" if fused else "ogk_sweep"
    launch_eval()
    nb = max(a.steps // 10, 25)
    single = timed(launch_sweep if fused else launch_columns, max(a.steps, 25), 1)
    batched = timed(launch_sweep if fused else launch_columns, nb, 10)
    # the two kernels of the two-launch form, for reference (ogk_eval, then ogk_sweep reading its results)
    eval_ms_mean = float(np.mean(timed(launch_eval, nb, 10)))
    columns_ms_mean = float(np.mean(timed(launch_columns, nb, 10)))
    kern_ms = float(np.median(batched))
    kern_ms_mean = float(np.mean(batched))
    kern_ms_single = float(np.mean(single))

    # launch floor of this box: a kernel that does nothing, one workgroup per CU of 512 threads (the sweep's
    # geometry class), back to back on the same stream between two events - what ANY one-launch step costs
    def launch_probe():
        _native.check(eng._lib.og_probe_launch(256, 512, 1, stream), "og_probe_launch")

    floor_ms = float(np.median(timed(launch_probe, nb, 10)))
    ncols = hi - lo
    sumN2 = sum(int(v) ** 2 for v in prob.nodes)
    alg_bytes = 8.0 * ((ncols + 1) * n + m * ncols + sumN2)
    # average duration of a launch: every sample is the mean over a back-to-back batch of 10 launches between two
    # events; the MEDIAN of those batch means is used (one batch that catches a clock transition or another process's
    # copy would otherwise move the figure by 60 % - both are reported)
    # (round 5, VERDICT r4 #8c: `achieved` and `frac` use the MEAN, which is what rocprofv3's average duration measures;
    #  the median of the batches stays on the line as kernel_ms_median)
    achieved = alg_bytes / (kern_ms_mean * 1e-3) / 1e9
    indptr = backend.pattern_indptr()
    nnz_block = int(indptr[hi] - indptr[lo])
    peaks = fill_and_copy_peaks(torch, dev) if rank == 0 else None

    traffic = measured_traffic(a.workload, kernel, bool(a.nodes)) if world == 1 else None
    rocprof = committed_rocprof_average(a.workload, kernel, bool(a.nodes)) if world == 1 else None
    chain = (measured_chain(a.workload, a.nodes) if (world == 1 and rank == 0 and fused and not a.quick)
             else {"chain_us": None})
    chain_us = chain.get("chain_us") or DEPENDENT_CHAIN_US
    # VERDICT r5 #8a: `frac` (and `achieved`) on the line are the ones that FOLLOW FROM profiles/ - the committed rocprofv3
    # average duration of this workload's kernel (a dispatch's own begin -> end, 5-10 % longer than the back-to-back
    # period the HIP-event batches measure, because consecutive launches overlap their ramp-up and drain) - whenever such a
    # profile of the workload at this size exists; the live HIP-event batch mean stands beside it, and alone otherwise.
    achieved_events = achieved
    if rocprof and world == 1:
        achieved = alg_bytes / (rocprof["average_us"] * 1e-6) / 1e9
    result.update({
        "value_without_collective": (3 * n + 2) * a.steps / elapsed_local,
        "ms_per_step_without_collective": elapsed_local / a.steps * 1e3,
        "roofline": {"bound": "hbm", "kernel": kernel, "achieved": achieved,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     # (above 1 the convention prices traffic this kernel does not have: no fraction is reported)
                     "frac": achieved / HBM_PEAK_GBS if achieved <= HBM_PEAK_GBS else None,
                     "traffic": traffic["bytes"] if traffic else None,
                     "traffic_source": traffic["source"] if traffic else None,
                     # the honest bandwidth statement: bytes the PMC counters saw per launch over the launch's duration,
                     # against the peak - small, because the launch is a latency chain that moves only the non-zeros
                     "hbm_frac_on_measured_traffic": (traffic["bytes"] / (kern_ms_mean * 1e-3) / 1e9 / HBM_PEAK_GBS
                                                      if traffic else None),
                     # the D.X path on the matrix cores (rocprofv3 --pmc SQ_INSTS_VALU_MFMA_F64 SQ_VALU_MFMA_BUSY_CYCLES,
                     # same committed pass): v_mfma_f64_16x16x4_f64 per launch and busy cycles / (GRBM_GUI_ACTIVE x 1024 SIMDs)
                     "mfma": (traffic or {}).get("mfma") or None,
                     "algorithmic_bytes_per_launch": alg_bytes,
                     # what a launch really stores: the structural non-zeros of its block, F(x0) and the sweep scratch
                     "bytes_actually_written_per_launch": 8.0 * (nnz_block + 4 * m),
                     "structural_nonzeros_of_the_block": nnz_block,
                     "convention": "reference-formulation bytes (SURVEY.md 8(d)) over the launch's duration; the launch "
                                   "itself is a latency chain that moves only the non-zeros - see latency_floor_us",
                     # the budget that discriminates now: an empty 256 x 512-thread launch back to back on this box
                     # (launch floor) plus the dependent chain of one step (request -> barrier -> MFMA/dynamics chain ->
                     # stores: 3.6 us of in-kernel s_memrealtime stamps at C3)
                     # (the two overlap: a launch's ramp-up and drain hide under its neighbours' when launches follow each
                     # other, the chain does not - the floor of the back-to-back period is the larger of the two)
                     "latency_floor_us": max(floor_ms * 1e3, chain_us),
                     "latency_floor_parts_us": {"empty_launch_back_to_back": floor_ms * 1e3,
                                                "dependent_chain_in_kernel": chain_us,
                                                "dependent_chain_source": (
                                                    "measured in this run (tools/trace_fused.py --json: in-kernel stamps, the "
                                                    "fastest complete workgroup of the slowest kind)" if chain.get("chain_us")
                                                    else "constant of C3 (profiles/r02_trace_fused_polar_tsto.txt): %s" % (
                                                        chain.get("error") or "not measured in a --quick / multi-rank run")),
                                                "dependent_chain_by_kind_us": chain.get("by_kind_us")},
                     "frac_of_latency_floor": max(floor_ms * 1e3, chain_us) / (kern_ms_mean * 1e3),
                     "frac_source": ("committed rocprofv3 average of this workload (%s)" % rocprof["source"]
                                     if rocprof and world == 1 else "HIP-event batch mean of this run (no committed profile of "
                                                                    "this workload / size, or a multi-rank run)"),
                     "achieved_hip_events_batch_mean": achieved_events,
                     "frac_hip_events_batch_mean": achieved_events / HBM_PEAK_GBS if achieved_events <= HBM_PEAK_GBS else None,
                     "rocprofv3_average_us": rocprof["average_us"] if rocprof else None,
                     "rocprofv3_source": rocprof["source"] if rocprof else None,
                     "frac_from_rocprofv3_average": (alg_bytes / (rocprof["average_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
                                                     if rocprof and alg_bytes / (rocprof["average_us"] * 1e-6) / 1e9 <= HBM_PEAK_GBS
                                                     else None),
                     "kernel_ms_mean": kern_ms_mean, "kernel_ms_median": kern_ms,
                     "kernel_ms_single_launch_events": kern_ms_single,
                     "measured_fill_peak_GBs": peaks["fill"] if peaks else None,
                     "measured_copy_peak_GBs": peaks["copy"] if peaks else None,
                     "kernel_ms_used": "kernel_ms_mean (mean over batches of 10 back-to-back launches between two HIP "
                                       "events on the launch stream: what rocprofv3's average duration measures)",
                     "frac_of_measured_fill_peak": achieved / peaks["fill"] if peaks else None,
                     "frac_of_measured_copy_peak": achieved / peaks["copy"] if peaks else None,
                     # the two-launch form of the same step (OGPSX_SWEEP=split, or an unregistered buffer), timed
                     # in this run: the FD sweep kernel on its own, and evaluation + sweep as a step
                     "split_eval_kernel_ms_mean": eval_ms_mean,
                     "split_sweep_kernel_ms_mean": columns_ms_mean,
                     "split_sweep_kernel_frac": alg_bytes / (columns_ms_mean * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "split_step_frac": alg_bytes / ((columns_ms_mean + eval_ms_mean) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "frac_of_whole_step": alg_bytes / (elapsed / a.steps) / 1e9 / HBM_PEAK_GBS,
                     "note": ("achieved = SURVEY.md section 8(d)'s ALGORITHMIC bytes (the stack of n+1 perturbed vectors read "
                              "once + the dense m x n Jacobian written once + D) over the duration of the one launch that "
                              "produces F(x0) and the whole Jacobian.  The implementation never materialises the stack and, "
                              "with a persistent-zero output buffer, stores only the structural non-zeros "
                              "(bytes_actually_written_per_launch): the kernel is a latency chain, not a stream, so the "
                              "fraction can exceed 1 at C5's size - it prices the reference formulation's traffic, not this "
                              "kernel's; measured HBM traffic is `traffic`.")},
    })
    if world == 1 and rank == 0 and not a.quick:
        # self-check after the timed loop: every rotated buffer holds exactly what a literal dense sweep
        # (every row re-evaluated for every column, OGPSX_SWEEP=dense) produces, bit for bit
        os.environ["OGPSX_SWEEP"] = "dense"
        dense = HipEngine(prob, obj, device=local_rank)
        del os.environ["OGPSX_SWEEP"]
        d_ref = torch.empty((n, m), dtype=torch.float64, device=dev)
        d_Fr = torch.empty(m, dtype=torch.float64, device=dev)

        def launch_dense():
            dense.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), 0, n, d_ref.data_ptr(), d_Fr.data_ptr(), stream)

        launch_dense()
        dense_ms = float(np.median(timed(launch_dense, 5, 1 if n > 3000 else 3)))
        torch.cuda.synchronize()
        same = all(torch.equal(sh.replica, d_ref) for sh in sweeps) and torch.equal(d_F0, d_Fr)
        result["self_check"] = {"equals_dense_sweep_bitwise": bool(same), "buffers_checked": nbuf}
        result["dense_sweep_ms"] = dense_ms
        result["dense_sweep_evals_per_s"] = (3 * n + 2) / (dense_ms * 1e-3)
        dense.close()
        del d_ref
        assert same, "the structured sweep into the registered buffers differs from the dense sweep"
        # the host-pointer API as Problem.solve's callbacks use it (PCIe inclusive): x, h up, packed non-zeros + F
        # down into ONE persistent host matrix (og_jt_register_host); and the dense transfer into a fresh array
        for _ in range(10):                                   # (the first calls page-lock and map the matrix, fault its pages in)
            eng.sweep_persistent(x0, h)
        reps = 100
        calls = np.empty(reps)
        if os.environ.get("OG_BENCH_NOGC"):                   # diagnostics: is the one slow call a full Python garbage collection?
            import gc
            gc.disable()
        for i in range(reps):
            t0 = time.perf_counter()
            eng.sweep_persistent(x0, h)
            calls[i] = time.perf_counter() - t0
        # (per call: one stall of tens of milliseconds among a hundred calls - seen on some leases - would otherwise pass for
        # the cost of a call; mean, median and the slowest call are all on the line)
        result["host_api_ms_per_sweep"] = float(np.median(calls)) * 1e3
        result["host_api_ms_per_sweep_mean"] = float(np.mean(calls)) * 1e3
        result["host_api_ms_per_sweep_max"] = float(np.max(calls)) * 1e3
        result["host_api_slow_calls"] = [(int(i), float(calls[i]) * 1e3) for i in np.argsort(calls)[-3:][::-1]]
        if os.environ.get("OG_BENCH_PROFILE_HOSTAPI"):        # diagnostics: where a call's time goes on the Python side
            import cProfile
            import pstats
            pr = cProfile.Profile()
            pr.enable()
            for _ in range(reps):
                eng.sweep_persistent(x0, h)
            pr.disable()
            pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(6)
        result["host_api_path"] = eng.host_path               # "mapped" or "staged": whichever the first six sweeps found faster
        reps = 5 if n > 3000 else 10
        eng.sweep_stacked(x0, h)
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.sweep_stacked(x0, h)
        result["host_api_dense_transfer_ms_per_sweep"] = (time.perf_counter() - t0) / reps * 1e3
        result["host_api_note"] = ("og_fd_sweep, PCIe included: host_api_ms_per_sweep into the engine's registered persistent "
                                   "host matrix - page-locked and mapped since round 6: the launch stores its %.2f MB of non-zeros "
                                   "into it and reads x, h in place (OGPSX_HOST=staged: packed copy + host scatter, round 5's path); "
                                   "host_api_dense_transfer into a fresh n x m array (%.1f MB)"
                                   % (8e-6 * int(indptr[-1]), replica_bytes / 1e6))
    if world == 1 and rank == 0 and fused and not a.quick:
        # the same K steps as ONE hipGraph (the launch arguments are pointers only): what the loop costs without the
        # host's per-launch work
        try:
            side = torch.cuda.Stream()
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                cs = torch.cuda.current_stream().cuda_stream
                for i in range(a.steps):
                    sh = sweeps[i % nbuf]
                    eng.sweep_dev(d_x.data_ptr(), d_h.data_ptr(), lo, hi, sh.replica[lo:hi].data_ptr(), sh.F0.data_ptr(), cs)
            graph.replay()
            torch.cuda.synchronize()
            reps = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                graph.replay()
                torch.cuda.synchronize()
                reps.append(time.perf_counter() - t0)
            result["hip_graph_replay"] = {"ms_per_step_median": float(np.median(reps)) / a.steps * 1e3,
                                          "ms_per_step_min": float(np.min(reps)) / a.steps * 1e3, "steps_per_graph": a.steps,
                                          "evals_per_s": (3 * n + 2) * a.steps / float(np.median(reps))}
            del graph
        except Exception as exc:
            result["hip_graph_replay"] = {"error": repr(exc)}
    if world == 1 and rank == 0 and not a.no_cpu_baseline and not a.quick:
        base = cpu_baseline(a.workload, "serial", a.cpu_seconds, a.nodes)
        base["compiled_cpp_dense_loop_evals_per_s"] = compiled_loop_context(a.workload, a.nodes)
        result["cpu_baseline"] = base
        result["cpu_baseline_all_cores"] = cpu_baseline(a.workload, "all_cores", a.cpu_seconds, a.nodes)
        result["cpu_baseline_batch_last"] = cpu_baseline(a.workload, "batch_last", a.cpu_seconds, a.nodes)
        for key in ("cpu_baseline", "cpu_baseline_all_cores", "cpu_baseline_batch_last"):
            if result[key].get("value"):
                result["speedup_vs_" + key] = result["value"] / result[key]["value"]
    if world == 1 and rank == 0 and not a.quick:
        # exact-Jacobian mode (og_jacobian_exact_dev: evaluation + ogk_exact_struct), same resident x0, registered buffer
        d_jt = sweeps[0].replica
        for _ in range(3):
            eng.exact_dev(d_x.data_ptr(), 0, n, d_jt.data_ptr(), d_F0.data_ptr(), stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        e0.record()
        for _ in range(reps):
            eng.exact_dev(d_x.data_ptr(), 0, n, d_jt.data_ptr(), d_F0.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        result["exact_jacobian"] = {"ms_per_jacobian": e0.elapsed_time(e1) / reps, "kernel": "ogk_eval + ogk_exact_struct",
                                    "note": "forward-mode derivatives (opt-in mode, jacobian='exact')"}
    if world == 1 and rank == 0 and not a.quick and not a.no_cold_start:
        result["cold_start_s"] = cold_start(a.workload, a.nodes)
        # (import -> traced -> compiled -> handle -> F and the whole Jacobian of the first point on the host)
        result["first_solve_s"] = result["cold_start_s"].get("total_s")
    if world == 1 and rank == 0 and a.sqp_iterations > 0 and n + 1 <= 16384 and not a.quick:
        # (round 4: C5 too - its subproblems take 0.07-0.15 s since the wide LQ sweep; the CPU checker of the first
        # subproblem needs minutes there and runs in tests/test_slsqp_core.py instead)
        result["sqp"] = sqp_leg(eng, prob, a.sqp_iterations,
                                a.sqp_reference_iterations if n <= 1600 else 0, check_first_qp=n <= 3000)
    if world == 1 and rank == 0 and not a.quick and not a.no_solve and not a.nodes:
        # wall-clock to SLSQP convergence (second half of the metric) with the oracle's KKT check of the optimum: the
        # headline workload, and C4 (BASELINE.json's next configuration) beside it when the headline is C3
        try:
            result["solve"] = solve_leg(a.workload)
            # ... from --solve-starts neighbouring starts: median and range (one start is one sample of a chaotic path)
            if a.solve_starts > 1:
                result["solve"]["starts"] = solve_starts(a.workload, a.solve_starts, first=result["solve"])
            if a.workload == "polar_tsto":
                # C4 with the reference's defaults, and with the tolerance at which SLSQP's exit test means a KKT point
                c4 = solve_leg("low_thrust")
                if a.solve_starts > 1:
                    c4["starts"] = solve_starts("low_thrust", a.solve_starts, first=c4)
                result["solve"]["also"] = [c4, solve_leg("low_thrust", {"ftol": 1e-8, "maxiter": 400})]
                if not a.no_c5:
                    result["solve"]["also"].append(bounded_c5_leg())
        except Exception as exc:                               # a failed leg must not lose the line
            result["solve"] = {"error": repr(exc)}
    if baseline_config is not None:
        result["baseline_config"] = baseline_config
    if collective:
        # every rank's replicas hold the whole matrix: compare rank 0's with every other rank's (checksums)
        sums = torch.stack([sh.replica.sum(dtype=torch.float64) for sh in sweeps]).to(pg_dev)
        gathered = [torch.empty_like(sums) for _ in range(world)]
        dist.all_gather(gathered, sums)
        if rank == 0:
            assert all(torch.equal(g, gathered[0]) for g in gathered), "replicas differ between ranks"
            assert all(torch.equal(sh.replica, sweeps[0].replica) for sh in sweeps)
            result["self_check"] = {"replicas_equal_across_ranks": True}
    return finish(result)


if __name__ == "__main__":
    sys.exit(main() or 0)

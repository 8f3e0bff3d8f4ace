#!/usr/bin/env python
"""What the assembled exact Hessian of w . F costs (og_hessian_matrix*, include/ogpsx.h) against the two routes a user
has without it, both through og_hessian_vector_dev, in one process on one GPU:

    python tools/bench_hessian_matrix.py [--sizes C2,C3,C5] [--seeds FILE] [--out profiles/hessian_matrix.json]

Measured per size, the forms alternating ``--rounds`` times, HIP-event intervals around back-to-back units, p10 / median
/ p90 in microseconds per call:

  evaluation            og_eval_dev: what every form below contains
  exact_jacobian        og_jacobian_exact_dev over all n columns into a registered buffer: the figure the expectation is
                        stated against
  matrix_1, matrix_8    og_hessian_matrix_dev with 1 and 8 weight vectors (two launches)
  matrix_batch_B        og_hessian_matrix_batch_dev, B lanes, one vector each (three launches)
  hvp_units             route (a): og_hessian_vector_dev with all n unit directions, in chunks of 32 pairs
  hvp_coloured          route (b): the compressed route - the variables with the most partners removed, a greedy
                        distance-2 colouring of the pattern's other columns as seed directions (columns of one colour
                        share no row), one unit direction per removed variable; chunks of 32 pairs.  ``directions``
                        records how many that is.

The expectation, written down before the first measurement: a stored entry evaluates only the owner's terms that read
the partner, each term once per chunk of 8 vectors on second-order duals, so one call should cost about the
exact-Jacobian kernel's time multiplied by the mean number of partners per term (``partners_per_term``: listed terms over
the terms of all columns) - ``expected_us`` next to ``matrix_1``; ``held`` says whether the median is within a factor
of two of it.

The seed directions are computed from ``codegen.HessianPlan`` and written to ``--seeds``; on a tree without the plan (the
parent commit's) the tool reads them from there and times the two routes only: that is the parent commit's leg by the
same tool.  ``--merge`` / ``--merge-parent`` put result files into one, the parent's under ``parent_commit``.  Nothing is
gated on these times."""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"C2": "goddard", "C3": "polar_tsto", "C5": "launch4"}
CHUNK = 32


def commit_of_tree():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                              text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def stats(samples_us):
    s = np.sort(np.asarray(samples_us, dtype=float))
    q = lambda f: float(s[min(s.size - 1, int(f * s.size))])      # noqa: E731
    return {"median_us": float(np.median(s)), "p10_us": q(0.10), "p90_us": q(0.90), "min_us": float(s[0]),
            "max_us": float(s[-1]), "intervals": int(s.size)}


def coloured_seeds(indptr, cols, n):
    """``(heavy, colour[n])``: the variables removed (more partners than eight times the median, at least 64) and a
    greedy distance-2 colour of every other variable that has a partner (-1: none) - two variables of one colour share
    no row among the variables that stay."""
    adj = [set() for _ in range(n)]
    for j in range(n):
        for l in cols[indptr[j]:indptr[j + 1]]:
            adj[j].add(int(l))
            adj[int(l)].add(j)
    deg = np.array([len(a) for a in adj])
    limit = max(64, 8 * int(np.median(deg[deg > 0])) if (deg > 0).any() else 64)
    heavy = [j for j in range(n) if deg[j] > limit]
    gone = set(heavy)
    colour = -np.ones(n, dtype=int)
    for j in range(n):
        if j in gone or not adj[j]:
            continue
        taken = set()
        for i in adj[j] | {j}:
            if i in gone:
                continue
            taken.update(int(colour[l]) for l in adj[i] | {i} if l not in gone and colour[l] >= 0)
        c = 0
        while c in taken:
            c += 1
        colour[j] = c
    return heavy, colour


def seed_matrix(heavy, colour, n):
    ncol = int(colour.max()) + 1
    V = np.zeros((ncol + len(heavy), n))
    for j in np.flatnonzero(colour >= 0):
        V[colour[j], j] = 1.0
    for i, j in enumerate(heavy):
        V[ncol + i, j] = 1.0
    return V


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="C2,C3,C5")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20, help="event intervals per round")
    ap.add_argument("--inner", type=int, default=10, help="repetitions of the unit inside one interval")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the forms")
    ap.add_argument("--budget", type=float, default=12.0, help="seconds a form may take per size; the intervals shrink to fit")
    ap.add_argument("--seeds", default=None, help="npz of the seed directions: written with the plan, read without it")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", metavar="JSON", default=None)
    ap.add_argument("--merge-parent", nargs="+", metavar="JSON", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", "hessian_matrix.json")
    if a.merge:
        def merged(paths):
            res = None
            for path in paths:
                with open(path) as fh:
                    part = json.load(fh)
                if res is None:
                    res = part
                else:
                    res["sizes"].update(part["sizes"])
            return res
        result = merged(a.merge)
        if a.commit:
            result["commit"] = a.commit
        if a.merge_parent:
            result["parent_commit"] = merged(a.merge_parent)
            result["parent_commit"]["note"] = ("the same tool on the parent commit's tree in the same lease: the two "
                                               "Hessian-vector routes only, there is no assembled Hessian there")
        with open(out, "w") as fh:
            fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
        return

    import torch
    from opengoddard_amd import _native, problems
    from opengoddard_amd.engine import HipEngine
    if not torch.cuda.is_available() or _native.device_count() < 1:
        raise SystemExit("bench_hessian_matrix.py: no GPU; there is nothing to measure without one")
    has_matrix = hasattr(HipEngine, "hessian_matrix_dev")
    seeds_path = a.seeds or os.path.join(tempfile.gettempdir(), "hessian_matrix_seeds.npz")
    seeds = {}
    if not has_matrix:
        with np.load(seeds_path) as fh:
            seeds = {k: fh[k] for k in fh.files}
    dev = torch.device("cuda", 0)
    stream_obj = torch.cuda.Stream(device=dev)
    stream = stream_obj.cuda_stream

    def timed(unit, reps, inner):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        with torch.cuda.stream(stream_obj):
            for _ in range(inner):
                unit()
            stream_obj.synchronize()
            for e0, e1 in pairs:
                e0.record()
                for _ in range(inner):
                    unit()
                e1.record()
            stream_obj.synchronize()
        return [e0.elapsed_time(e1) * 1e3 / inner for e0, e1 in pairs]

    def fitted(unit, reps, inner):
        """One synchronised call on the wall clock, then as many intervals as ``--budget`` seconds per form allow ->
        ``(reps, inner, seconds of that call)``; reps 0: the one call is all the budget allows"""
        import time
        with torch.cuda.stream(stream_obj):
            stream_obj.synchronize()
            t0 = time.perf_counter()
            unit()
            stream_obj.synchronize()
            one = time.perf_counter() - t0
        if one * 2 * a.rounds > a.budget:
            return 0, 1, one
        cost = lambda r, i: one * i * (r + 1) * a.rounds          # noqa: E731
        while inner > 1 and cost(reps, inner) > a.budget:
            inner = max(1, inner // 2)
        while reps > 2 and cost(reps, inner) > a.budget:
            reps = max(2, reps // 2)
        return reps, inner, one

    def alternate(units):
        """{label: (unit, reps, inner)} -> {label: stats}, the forms taking turns round by round"""
        samples = {label: [] for label in units}
        fit = {label: fitted(*spec) for label, spec in units.items()}
        for _ in range(a.rounds):
            for label, (unit, _, _) in units.items():
                reps, inner, one = fit[label]
                samples[label] += timed(unit, reps, inner) if reps else []
        out = {}
        for label, v in samples.items():
            out[label] = stats(v) if v else dict(stats([fit[label][2] * 1e6]), note="one synchronised call on the wall clock")
        return out

    result = {"tool": "tools/bench_hessian_matrix.py", "host": socket.gethostname(), "commit": a.commit or commit_of_tree(),
              "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "rounds": a.rounds,
              "has_matrix": has_matrix, "chunk": CHUNK, "sizes": {}}
    B = a.batch
    for tag in a.sizes.split(","):
        name = SIZES[tag]
        prob, obj = problems.build(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            eng = HipEngine(prob, obj)
        n, m = eng.n, eng.m
        entry = {"problem": name, "n": n, "m": m, "module": os.path.basename(eng.module_path)}
        lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
        ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
        rng = np.random.default_rng(20250 + n)
        x0 = np.clip(prob.p, lb, ub)
        X = np.stack([np.clip(x0 * (1.0 + 1e-3 * rng.standard_normal(n)), lb, ub) for _ in range(B)])
        W = rng.standard_normal((B, m))
        W /= np.abs(W).max(axis=1)[:, None]
        nnz = 0
        if has_matrix:
            plan = eng._hessian_plan()                  # (codegen.HessianPlan, shared with the load)
            nnz = plan.nnz
            heavy, colour = coloured_seeds(plan.indptr, plan.cols, n)
            V = seed_matrix(heavy, colour, n)
            seeds[tag] = V
            entry.update({"nnz": nnz, "listed_terms": len(plan.tlist), "jacobian_terms": int(sum(plan.terms)),
                          "partners_per_term": len(plan.tlist) / max(1, sum(plan.terms)),
                          "removed_variables": len(heavy), "colours": int(colour.max()) + 1})
        else:
            V = seeds[tag]
        ndir = V.shape[0]
        entry["directions"] = ndir
        batch = eng.batch(B) if has_matrix else None
        with torch.cuda.stream(stream_obj):
            d_X, d_W = torch.from_numpy(X).to(dev), torch.from_numpy(W).to(dev)
            d_W1 = d_W[:1].expand(CHUNK, m).contiguous()          # one weight vector, as every pair of a chunk
            d_V = torch.from_numpy(V).to(dev)
            d_E = torch.eye(n, dtype=torch.float64, device=dev)
            d_F = torch.empty((B, m), dtype=torch.float64, device=dev)
            d_Q = torch.empty((CHUNK, n), dtype=torch.float64, device=dev)
            d_H = torch.empty((B, max(nnz, 1)), dtype=torch.float64, device=dev)
            d_JT = torch.empty((n, m), dtype=torch.float64, device=dev)
            eng.register_jt_dev(d_JT.data_ptr(), 0, n, stream)

        def products(d_dirs, count):
            for c0 in range(0, count, CHUNK):
                k = min(CHUNK, count - c0)
                eng.hessian_vector_dev(d_X.data_ptr(), k, d_W1.data_ptr(), d_dirs[c0].data_ptr(), d_Q.data_ptr(),
                                       d_F.data_ptr(), stream)

        long_inner = 1 if n > 1000 else 2
        m_reps, m_inner = (a.reps, a.inner) if n <= 1000 else (max(5, a.reps // 2), max(2, a.inner // 3))
        units = {"evaluation": (lambda: eng.eval_dev(d_X.data_ptr(), d_F.data_ptr(), stream), a.reps, a.inner),
                 "exact_jacobian": (lambda: eng.exact_dev(d_X.data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(), stream),
                                    a.reps, a.inner),
                 "hvp_units": (lambda: products(d_E, n), 3, long_inner),
                 "hvp_coloured": (lambda: products(d_V, ndir), 5, long_inner)}
        if has_matrix:
            for K in (1, 8):
                units["matrix_%d" % K] = ((lambda K=K: eng.hessian_matrix_dev(d_X.data_ptr(), K, d_W.data_ptr(), d_H.data_ptr(),
                                                                              d_F.data_ptr(), stream)), m_reps, m_inner)
            units["matrix_batch_%d" % B] = (lambda: batch.hessian_matrix_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_H.data_ptr(),
                                                                             d_F.data_ptr(), stream), m_reps, m_inner)
        with torch.cuda.stream(stream_obj):
            for label, (unit, _, _) in units.items():   # (every on-demand part is built and loaded before the clock runs)
                if label not in ("hvp_units", "hvp_coloured"):
                    unit()
            products(d_E, CHUNK)
            stream_obj.synchronize()
        entry.update(alternate(units))
        if has_matrix:
            expected = entry["exact_jacobian"]["median_us"] * entry["partners_per_term"]
            got = entry["matrix_1"]["median_us"]
            entry["expected_us"] = expected
            entry["held"] = bool(0.5 * expected <= got <= 2.0 * expected)
        result["sizes"][tag] = entry
        print("%s: " % tag + ", ".join("%s %.2f" % (k, v["median_us"]) for k, v in entry.items()
                                       if isinstance(v, dict) and "median_us" in v) + " us; directions %d" % ndir, flush=True)
        eng.unregister_jt_dev(d_JT.data_ptr())
        eng.close()
    if has_matrix:
        os.makedirs(os.path.dirname(os.path.abspath(seeds_path)), exist_ok=True)
        np.savez_compressed(seeds_path, **seeds)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(json.dumps({"bench_hessian_matrix": "done", "host": result["host"], "out": out}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What an exact adjoint product F'(x)^T w costs (og_adjoint*, include/ogpsx.h) against what a user has to do without it -
the whole exact Jacobian and its product with w - in one process on one GPU:

    python tools/bench_adjoint.py [--sizes C2,C3,C5] [--vectors 1,8,32] [--batch 32] [--out profiles/adjoint.json]

Measured per size, the forms alternating ``--rounds`` times, ``--reps`` HIP-event intervals per round around ``--inner``
back-to-back units, p10 / median / p90 in microseconds per call:

  evaluation                    og_eval_dev: what every form below contains
  adjoint_K                     og_adjoint_dev with K weight vectors of one point (two launches)
  exact_jacobian                og_jacobian_exact_dev into a registered buffer, all n columns
  exact_jacobian_product_K      the same followed by the product W[K, m] x J_T[n, m]^T on the device (torch.matmul)
  adjoint_batch_B               og_adjoint_batch_dev, B lanes, one weight vector each (three launches)
  exact_jacobian_batch_B        og_jacobian_exact_batch_dev, B lanes, packed values - WITHOUT the B sparse products a user
                                would still owe: a lower bound of today's way for a batch

On a tree without the adjoint calls only the Jacobian legs are timed: that is the parent commit's leg by the same tool;
``--merge`` / ``--merge-parent`` put result files into one, the parent's under ``parent_commit``.  Nothing is gated on
these times."""
import argparse
import json
import os
import socket
import subprocess
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"C2": "goddard", "C3": "polar_tsto", "C5": "launch4"}


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="C2,C3,C5")
    ap.add_argument("--vectors", default="1,8,32")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30, help="event intervals per round")
    ap.add_argument("--inner", type=int, default=10, help="repetitions of the unit inside one interval")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the forms")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", metavar="JSON", default=None)
    ap.add_argument("--merge-parent", nargs="+", metavar="JSON", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", "adjoint.json")
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
            result["parent_commit"]["note"] = ("the same tool on the parent commit's tree in the same lease: the exact "
                                               "Jacobian legs only, there is no adjoint product there")
        with open(out, "w") as fh:
            fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
        return

    import torch
    from opengoddard_amd import _native, problems
    from opengoddard_amd.engine import HipEngine
    if not torch.cuda.is_available() or _native.device_count() < 1:
        raise SystemExit("bench_adjoint.py: no GPU; there is nothing to measure without one")
    has_adjoint = hasattr(HipEngine, "adjoint_dev")
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

    def alternate(units):
        """{label: unit} -> {label: stats}, the forms taking turns round by round"""
        samples = {label: [] for label in units}
        for _ in range(a.rounds):
            for label, unit in units.items():
                samples[label] += timed(unit, a.reps, a.inner)
        return {label: stats(v) for label, v in samples.items()}

    result = {"tool": "tools/bench_adjoint.py", "host": socket.gethostname(), "commit": a.commit or commit_of_tree(),
              "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "rounds": a.rounds,
              "has_adjoint": has_adjoint, "sizes": {}}
    Ks = [int(v) for v in a.vectors.split(",")]
    B = a.batch
    for tag in a.sizes.split(","):
        name = SIZES[tag]
        prob, obj = problems.build(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            eng = HipEngine(prob, obj)
        n, m = eng.n, eng.m
        lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
        ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
        rng = np.random.default_rng(20250 + n)
        x0 = np.clip(prob.p, lb, ub)
        rows = max(Ks + [B])
        X = np.stack([np.clip(x0 * (1.0 + 1e-3 * rng.standard_normal(n)), lb, ub) for _ in range(B)])
        W = rng.standard_normal((rows, m))
        W /= np.abs(W).max(axis=1)[:, None]
        batch = eng.batch(B)
        with torch.cuda.stream(stream_obj):
            d_X, d_W = torch.from_numpy(X).to(dev), torch.from_numpy(W).to(dev)
            d_F = torch.empty((B, m), dtype=torch.float64, device=dev)
            d_G = torch.empty((rows, n), dtype=torch.float64, device=dev)
            d_JT = torch.zeros((n, m), dtype=torch.float64, device=dev)
            d_vals = torch.empty((B, batch.nnz), dtype=torch.float64, device=dev)
            eng.register_jt_dev(d_JT.data_ptr(), 0, n, stream)
        jac = lambda: eng.exact_dev(d_X.data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(), stream)      # noqa: E731
        units = {"evaluation": lambda: eng.eval_dev(d_X.data_ptr(), d_F.data_ptr(), stream), "exact_jacobian": jac}
        for K in Ks:
            units["exact_jacobian_product_%d" % K] = (lambda K=K: (jac(), torch.matmul(d_W[:K], d_JT.T, out=d_G[:K])))
        units["exact_jacobian_batch_%d" % B] = lambda: batch.exact_dev(B, d_X.data_ptr(), d_F.data_ptr(), d_vals.data_ptr(),
                                                                       stream)
        if has_adjoint:
            for K in Ks:
                units["adjoint_%d" % K] = (lambda K=K: eng.adjoint_dev(d_X.data_ptr(), K, d_W.data_ptr(), d_G.data_ptr(),
                                                                       d_F.data_ptr(), stream))
            units["adjoint_batch_%d" % B] = lambda: batch.adjoint_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_G.data_ptr(),
                                                                      d_F.data_ptr(), stream)
        entry = {"problem": name, "n": n, "m": m, "nnz": int(batch.nnz), "module": os.path.basename(eng.module_path)}
        with torch.cuda.stream(stream_obj):
            for unit in units.values():                 # (every on-demand part is built and loaded before the clock runs)
                unit()
            stream_obj.synchronize()
            if has_adjoint:
                # the two ways agree (the product in another order of summation: to rounding, in units of the column's scale)
                K = Ks[-1]
                eng.adjoint_dev(d_X.data_ptr(), K, d_W.data_ptr(), d_G.data_ptr(), d_F.data_ptr(), stream)
                jac()
                stream_obj.synchronize()
                scale = torch.clamp(torch.matmul(d_W[:K].abs(), d_JT.abs().T), min=1.0)
                entry["max_difference_from_the_product"] = float(((d_G[:K] - torch.matmul(d_W[:K], d_JT.T)).abs() / scale).max())
        entry.update(alternate(units))
        result["sizes"][tag] = entry
        print("%s: " % tag + ", ".join("%s %.2f" % (k, v["median_us"]) for k, v in entry.items()
                                       if isinstance(v, dict) and "median_us" in v) + " us", flush=True)
        eng.unregister_jt_dev(d_JT.data_ptr())
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(json.dumps({"bench_adjoint": "done", "host": result["host"], "out": out}))


if __name__ == "__main__":
    main()

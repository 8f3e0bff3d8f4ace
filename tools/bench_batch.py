#!/usr/bin/env python
"""What a batch of points per launch buys (og_batch_fd_sweep_dev, include/ogpsx.h) against the same points swept one
by one (og_fd_sweep_dev), in one process on one GPU:

    python tools/bench_batch.py [--sizes C1,C3,C4,C5] [--batches 1,2,4,8,16,32] [--out profiles/batch_sweep.json]

For every size and every B the two forms alternate (``--rounds`` times); each round takes ``--reps`` HIP-event
intervals on the launch stream, each around ``--inner`` back-to-back repetitions of the unit (one batched launch of B
lanes / B consecutive single-point calls into B registered buffers), after one untimed repetition block.  Reported per
form: median, min, max and the 10th / 90th percentile of the intervals, per launch (or per B calls) and per point.  The
host-pointer forms (``BatchSweep.sweep`` - into the batch's persistent result arrays, and into fresh arrays - against
B x ``HipEngine.sweep_persistent``) are timed with the host clock around the blocking calls.  The batched device leg is
timed twice: with the same four arrays on every call, and with arrays that change from call to call (the library binds
the arrays to the lanes with a small launch ahead of every batched launch either way).  On a tree without batches the
batch legs are skipped and the single-point legs remain (the baseline of an older commit).  ``--merge`` /
``--merge-parent`` put the result files of several runs into one.  B is limited by the device's free memory (every lane owns a dense n x m matrix).

``--exact`` measures the exact Jacobians instead (device-pointer forms only; result file profiles/batch_exact.json): one
og_jacobian_exact_batch_dev call with packed values against B consecutive og_jacobian_exact_dev calls into B registered
buffers, each followed by the og_pack_dev launch the batched kernel makes unnecessary - and against the same calls
without the pack - with the batched FD sweep of the same points alternating in the same rounds (what exactness costs per
point).  On a tree without the batched exact form the single-point legs remain (the baseline of the parent commit)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"C1": "brachistochrone", "C2": "goddard", "C3": "polar_tsto", "C4": "low_thrust", "C5": "launch4"}


def commit_of_tree():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                              text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def stats(samples_us, per):
    s = np.sort(np.asarray(samples_us, dtype=float))
    q = lambda f: float(s[min(s.size - 1, int(f * s.size))])      # noqa: E731
    return {"us_per_launch": float(np.median(s)), "us_per_point": float(np.median(s)) / per,
            "min_us": float(s[0]), "p10_us": q(0.10), "p90_us": q(0.90), "max_us": float(s[-1]),
            "intervals": int(s.size)}


def exact_legs(a, eng, timed, stream_obj, stream, dev, B, X, d_X, d_H, d_F, d_JT, has_batch):
    """The ``--exact`` legs of one (size, B): the forms alternate ``--rounds`` times -> the result row."""
    import torch
    from opengoddard_amd import _native
    n, m = eng.n, eng.m
    nnz = int(eng.pattern()[0][-1])
    with torch.cuda.stream(stream_obj):
        d_P = torch.empty((B, nnz), dtype=torch.float64, device=dev)
    ptrs = [(d_X[k].data_ptr(), d_JT[k].data_ptr(), d_F[k].data_ptr(), d_P[k].data_ptr()) for k in range(B)]

    def singles():
        for px, pj, pf, _pp in ptrs:
            eng.exact_dev(px, 0, n, pj, pf, stream)

    def singles_packed():
        for px, pj, pf, pp in ptrs:
            eng.exact_dev(px, 0, n, pj, pf, stream)
            _native.check(eng._lib.og_pack_dev(eng._handle, pj, 0, n, pp, stream), "og_pack_dev")

    batch = eng.batch(B) if has_batch else None
    has_exact = batch is not None and hasattr(batch, "exact_dev")
    if batch is not None:
        with torch.cuda.stream(stream_obj):
            d_Fb = torch.empty((B, m), dtype=torch.float64, device=dev)
            d_V = torch.empty((B, nnz), dtype=torch.float64, device=dev)
            d_Ff = torch.empty((B, m), dtype=torch.float64, device=dev)
            d_Vf = torch.empty((B, nnz), dtype=torch.float64, device=dev)

        def fd_batched():
            batch.sweep_dev(B, d_X.data_ptr(), d_H.data_ptr(), d_Ff.data_ptr(), d_Vf.data_ptr(), stream)

        def batched():
            batch.exact_dev(B, d_X.data_ptr(), d_Fb.data_ptr(), d_V.data_ptr(), stream)

    single_us, packed_us, batch_us, fd_us = [], [], [], []
    for _ in range(a.rounds):
        packed_us += timed(singles_packed, a.reps, a.inner)
        if has_exact:
            batch_us += timed(batched, a.reps, a.inner)
        single_us += timed(singles, a.reps, a.inner)
        if batch is not None:
            fd_us += timed(fd_batched, a.reps, a.inner)
    row = {"exact_single_packed_dev": stats(packed_us, B), "exact_single_dev": stats(single_us, B)}
    if batch is not None:
        row["fd_batch_dev"] = stats(fd_us, B)
    if has_exact:
        row["exact_batch_dev"] = stats(batch_us, B)
        # same results, at the size that was timed (the lanes' matrices hold the FD sweep's values by now: run once more)
        with torch.cuda.stream(stream_obj):
            singles_packed()
            batched()
        stream_obj.synchronize()
        row["all_points_finite"] = bool(torch.isfinite(d_F).all())
        row["bitwise_equal_F"] = bool(torch.equal(d_F, d_Fb))
        row["bitwise_equal_packed_values"] = bool(torch.equal(d_P, d_V))
        row["bitwise_equal_JT_lane0"] = bool(np.array_equal(batch.dense(0), d_JT[0].cpu().numpy()))
    if batch is not None:
        batch.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="C1,C3,C4,C5")
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=30, help="event intervals per round")
    ap.add_argument("--inner", type=int, default=10, help="repetitions of the unit inside one interval")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two forms")
    ap.add_argument("--host-reps", type=int, default=30)
    ap.add_argument("--exact", action="store_true",
                    help="the exact-Jacobian legs (og_jacobian_exact_batch_dev against B x og_jacobian_exact_dev + pack)")
    ap.add_argument("--commit", default=None, help="recorded in the result (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", metavar="JSON", default=None,
                    help="no measurement: merge result files of this tool (one per size) into --out")
    ap.add_argument("--merge-parent", nargs="+", metavar="JSON", default=None,
                    help="with --merge: result files of the same tool run on the parent commit's tree in the same "
                         "lease (single-point legs only); they go under 'parent_commit'")
    a = ap.parse_args()
    if a.merge:
        def merged(paths):
            out = None
            for path in paths:
                with open(path) as fh:
                    part = json.load(fh)
                if out is None:
                    out = part
                else:
                    out["sizes"].update(part["sizes"])
            return out
        result = merged(a.merge)
        result["merged_from"] = "one run of this tool per size, merged with --merge"
        if a.commit:
            result["commit"] = a.commit
        if a.merge_parent:
            result["parent_commit"] = merged(a.merge_parent)
            result["parent_commit"]["note"] = ("the same tool on the parent commit's tree in the same lease: "
                                               + ("the single-point exact legs and the FD batch, there is no batched "
                                                  "exact form there" if result.get("exact") else
                                                  "single-point legs only, there are no batches there"))
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
        return

    import torch
    from opengoddard_amd import _native, problems
    from opengoddard_amd.engine import HipEngine
    if not torch.cuda.is_available() or _native.device_count() < 1:
        raise SystemExit("bench_batch.py: no GPU; there is nothing to measure without one")
    dev = torch.device("cuda", 0)
    stream_obj = torch.cuda.Stream(device=dev)
    stream = stream_obj.cuda_stream

    def timed(unit, reps, inner):
        """-> microseconds per unit, one value per event interval"""
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

    result = {"tool": "tools/bench_batch.py", "host": socket.gethostname(), "commit": a.commit or commit_of_tree(),
              "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "rounds": a.rounds,
              "baseline": "B consecutive og_fd_sweep_dev calls (one launch each) into B registered n x m buffers",
              "sizes": {}}
    if a.exact:
        result["exact"] = True
        result["baseline"] = ("B consecutive og_jacobian_exact_dev calls (two launches each) into B registered n x m "
                              "buffers, each followed by og_pack_dev (one launch); also without the pack")
    want_b = [int(v) for v in a.batches.split(",")]
    for tag in a.sizes.split(","):
        name = SIZES[tag]
        prob, obj = problems.build(name)
        eng = HipEngine(prob, obj)
        has_batch = hasattr(eng, "batch")
        n, m = eng.n, eng.m
        lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
        ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
        rng = np.random.default_rng(20240 + n)
        x0 = np.clip(prob.p, lb, ub)
        entry = {"problem": name, "n": n, "m": m, "sweep_mode": eng.sweep_mode, "by_batch": {}}
        result["sizes"][tag] = entry
        for B in want_b:
            free, _total = torch.cuda.mem_get_info(dev)
            lane_bytes = 8 * n * m
            if 2 * B * lane_bytes > 0.7 * free:          # B registered buffers here + B lanes in the batch
                entry["by_batch"][str(B)] = {"skipped": "B lanes of %.0f MB do not fit twice into %.1f GB free"
                                                        % (lane_bytes / 2 ** 20, free / 2 ** 30)}
                continue
            # B distinct, feasible points around the start and SciPy's steps at each
            X = np.stack([np.clip(x0 * (1.0 + 1e-3 * rng.standard_normal(n)), lb, ub) for _ in range(B)])
            H = np.stack([_native.fd_step(x, lb, ub) for x in X])
            with torch.cuda.stream(stream_obj):
                d_X, d_H = torch.from_numpy(X).to(dev), torch.from_numpy(H).to(dev)
                d_F = torch.empty((B, m), dtype=torch.float64, device=dev)
                d_JT = torch.empty((B, n, m), dtype=torch.float64, device=dev)
                for k in range(B):
                    eng.register_jt_dev(d_JT[k].data_ptr(), 0, n, stream)
            ptrs = [(d_X[k].data_ptr(), d_H[k].data_ptr(), d_JT[k].data_ptr(), d_F[k].data_ptr()) for k in range(B)]

            def singles():
                for px, ph, pj, pf in ptrs:
                    eng.sweep_dev(px, ph, 0, n, pj, pf, stream)

            if a.exact:
                entry["by_batch"][str(B)] = row = exact_legs(a, eng, timed, stream_obj, stream, dev, B, X, d_X, d_H, d_F,
                                                             d_JT, has_batch)
                for k in range(B):
                    eng.unregister_jt_dev(d_JT[k].data_ptr())
                del d_JT
                torch.cuda.empty_cache()
                line = "%s B=%-2d exact: single+pack %8.2f us/point (p10 %.2f p90 %.2f), single %8.2f" % (
                    tag, B, row["exact_single_packed_dev"]["us_per_point"], row["exact_single_packed_dev"]["p10_us"] / B,
                    row["exact_single_packed_dev"]["p90_us"] / B, row["exact_single_dev"]["us_per_point"])
                if "exact_batch_dev" in row:
                    line += " | batch %8.2f us/point (p10 %.2f p90 %.2f), %8.2f us/call | FD batch %8.2f us/point" % (
                        row["exact_batch_dev"]["us_per_point"], row["exact_batch_dev"]["p10_us"] / B,
                        row["exact_batch_dev"]["p90_us"] / B, row["exact_batch_dev"]["us_per_launch"],
                        row["fd_batch_dev"]["us_per_point"])
                print(line, flush=True)
                continue
            batch = d_V = None
            if has_batch:
                batch = eng.batch(B)
                with torch.cuda.stream(stream_obj):
                    d_Fb = torch.empty((B, m), dtype=torch.float64, device=dev)
                    d_V = torch.empty((B, batch.nnz), dtype=torch.float64, device=dev)
                pb = (d_X.data_ptr(), d_H.data_ptr(), d_Fb.data_ptr(), d_V.data_ptr())

                def batched():
                    batch.sweep_dev(B, pb[0], pb[1], pb[2], pb[3], stream)

                # ... and with other arrays on every call (two sets, alternating)
                with torch.cuda.stream(stream_obj):
                    d_X2, d_H2 = d_X.clone(), d_H.clone()
                    d_Fb2, d_V2 = torch.empty_like(d_Fb), torch.empty_like(d_V)
                pb2 = (d_X2.data_ptr(), d_H2.data_ptr(), d_Fb2.data_ptr(), d_V2.data_ptr())
                turn = [0]

                def batched_other_arrays():
                    turn[0] ^= 1
                    q = pb2 if turn[0] else pb
                    batch.sweep_dev(B, q[0], q[1], q[2], q[3], stream)

            base_us, batch_us, batch2_us = [], [], []
            for _ in range(a.rounds):
                base_us += timed(singles, a.reps, a.inner)
                if batch is not None:
                    batch_us += timed(batched, a.reps, a.inner)
                    batch2_us += timed(batched_other_arrays, a.reps, a.inner)
            row = {"single_dev": stats(base_us, B)}
            if batch is not None:
                row["batch_dev_changing_arrays"] = stats(batch2_us, B)
            stream_obj.synchronize()
            row["all_points_finite"] = bool(torch.isfinite(d_F).all())
            if batch is not None:
                row["batch_dev"] = stats(batch_us, B)
                # same results, at the size that was timed
                stream_obj.synchronize()
                row["bitwise_equal_F"] = bool(torch.equal(d_F, d_Fb))
                row["bitwise_equal_JT_lane0"] = bool(np.array_equal(batch.dense(0), d_JT[0].cpu().numpy()))
            # host-pointer forms, host clock around blocking calls
            eng.sweep_persistent(X[0], H[0])
            for _ in range(12):                          # (the first ten calls decide how the host matrix is reached)
                eng.sweep_persistent(X[0], H[0])
            t_single = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                for k in range(B):
                    eng.sweep_persistent(X[k], H[k])
                t_single.append((time.perf_counter() - t0) * 1e6)
            row["single_host"] = stats(t_single, B)
            if batch is not None:
                # (persistent result arrays on both sides: sweep_persistent hands out views of the engine's matrix)
                for label, keep in (("batch_host", True), ("batch_host_fresh_arrays", False)):
                    batch.sweep(X, H, persistent=keep)
                    t_batch = []
                    for _ in range(a.host_reps):
                        t0 = time.perf_counter()
                        batch.sweep(X, H, persistent=keep)
                        t_batch.append((time.perf_counter() - t0) * 1e6)
                    row[label] = stats(t_batch, B)
                batch.close()
            for k in range(B):
                eng.unregister_jt_dev(d_JT[k].data_ptr())
            del d_JT, d_V
            d_X2 = d_H2 = d_Fb2 = d_V2 = None
            torch.cuda.empty_cache()
            entry["by_batch"][str(B)] = row
            line = "%s B=%-2d single %8.2f us/point (p10 %.2f p90 %.2f)" % (
                tag, B, row["single_dev"]["us_per_point"], row["single_dev"]["p10_us"] / B, row["single_dev"]["p90_us"] / B)
            if batch is not None:
                line += " | batch %8.2f us/point, %8.2f us/launch | host: single %.1f batch %.1f us/point" % (
                    row["batch_dev"]["us_per_point"], row["batch_dev"]["us_per_launch"],
                    row["single_host"]["us_per_point"], row["batch_host"]["us_per_point"])
            print(line, flush=True)
        eng.close()
    text = json.dumps(result, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps({"bench_batch": "done", "host": result["host"], "out": a.out}))


if __name__ == "__main__":
    main()

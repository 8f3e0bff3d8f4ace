#!/usr/bin/env python
"""What the exact second derivatives of w . F in the run-time parameters cost (og_parameter_hessian*, include/ogpsx.h)
against what a user has to do without them - per parameter, og_set_parameters_dev at theta_l +- h, two
og_parameter_jacobian_dev calls, the subtraction and the product with w - in one process on one GPU, on the
three-parameter problems of tools/bench_params.py (``PARAMS``):

    python tools/bench_parameter_hessian.py [--sizes C2,C3,C5] [--vectors 1,8] [--batch 32] [--out profiles/parameter_hessian.json]

Measured per size, the forms alternating ``--rounds`` times, ``--reps`` HIP-event intervals per round around ``--inner``
back-to-back units, p10 / median / p90 in microseconds per call:

  evaluation                    og_eval_dev: what every form below contains
  parameter_jacobian            og_parameter_jacobian_dev: what the expectation is stated against
  hessian_K                     og_parameter_hessian_dev with K weight vectors, all pairs (two launches)
  difference_K                  today's way: per parameter og_set_parameters_dev at theta + h e_l and at theta - h e_l,
                                og_parameter_jacobian_dev at each, the subtraction scaled by 1 / (2 h) and the product
                                with the K vectors; the parameters are put back at the end - 7 parameter launches and
                                6 parameter-Jacobian calls
  hessian_batch_B               og_parameter_hessian_batch_dev, B lanes, one vector each (three launches)
  difference_batch_B            the same difference with og_parameters_batch_dev and og_parameter_jacobian_batch_dev

``--build-only`` compiles every module part the run needs and measures nothing (no GPU needed).  On a tree without the
parameter-Hessian calls only the other legs are timed: that is the parent commit's leg by the same tool; ``--merge`` /
``--merge-parent`` put result files into one, the parent's under ``parent_commit``.  Nothing is gated on these times."""
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
STEP = 2.0 ** -20


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


def make(name):
    """The problem with the three parameters of tools/bench_params.py declared."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bench_params
    finally:
        sys.path.pop(0)
    return bench_params.make(name, True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="C2,C3,C5")
    ap.add_argument("--vectors", default="1,8")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30, help="event intervals per round")
    ap.add_argument("--inner", type=int, default=10, help="repetitions of the unit inside one interval")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the forms")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", metavar="JSON", default=None)
    ap.add_argument("--merge-parent", nargs="+", metavar="JSON", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", "parameter_hessian.json")
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
            result["parent_commit"]["note"] = ("the same tool on the parent commit's tree in the same lease: the evaluation, "
                                               "parameter-Jacobian and difference legs only, there is no parameter Hessian "
                                               "there")
        with open(out, "w") as fh:
            fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
        return

    from opengoddard_amd import build, codegen
    if a.build_only:
        for tag in a.sizes.split(","):
            prob, obj = make(SIZES[tag])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                header = codegen.emit_header(codegen.trace_problem(prob, obj))
            parts = [build.build_module(header), build.build_batch_part(header), build.build_parameter_part(header)]
            if hasattr(build, "build_pp_part"):
                parts.append(build.build_pp_part(header))
            print("%s: %s" % (tag, ", ".join(os.path.basename(p) for p in parts)), flush=True)
        return

    import torch
    from opengoddard_amd import _native
    from opengoddard_amd.engine import HipEngine
    if not torch.cuda.is_available() or _native.device_count() < 1:
        raise SystemExit("bench_parameter_hessian.py: no GPU; there is nothing to measure without one")
    has_pp = hasattr(HipEngine, "parameter_hessian_dev")
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

    result = {"tool": "tools/bench_parameter_hessian.py", "host": socket.gethostname(), "commit": a.commit or commit_of_tree(),
              "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "rounds": a.rounds,
              "has_parameter_hessian": has_pp, "step": STEP, "sizes": {}}
    Ks = [int(v) for v in a.vectors.split(",")]
    B = a.batch
    for tag in a.sizes.split(","):
        name = SIZES[tag]
        prob, obj = make(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            eng = HipEngine(prob, obj)
        n, m, n_par = eng.n, eng.m, eng.n_par
        lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
        ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
        rng = np.random.default_rng(20250 + n)
        x0 = np.clip(prob.p, lb, ub)
        rows = max(Ks + [B])
        X = np.stack([np.clip(x0 * (1.0 + 1e-3 * rng.standard_normal(n)), lb, ub) for _ in range(B)])
        W = rng.standard_normal((rows, m))
        W /= np.abs(W).max(axis=1)[:, None]
        theta = np.array(list(prob.parameters.values()), dtype=float)
        steps = STEP * np.maximum(1.0, np.abs(theta))
        # theta + h e_l, theta - h e_l per parameter, and theta itself; the same per lane of the batch
        TH = np.stack([theta + s * steps[l] * np.eye(n_par)[l] for l in range(n_par) for s in (1.0, -1.0)] + [theta])
        THB = np.repeat(TH[:, None, :], B, axis=1)
        batch = eng.batch(B)
        with torch.cuda.stream(stream_obj):
            d_X, d_W = torch.from_numpy(X).to(dev), torch.from_numpy(W).to(dev)
            d_TH, d_THB = torch.from_numpy(TH).to(dev), torch.from_numpy(np.ascontiguousarray(THB)).to(dev)
            d_F = torch.empty((B, m), dtype=torch.float64, device=dev)
            d_S = torch.empty((rows, n_par, n_par), dtype=torch.float64, device=dev)
            d_D = torch.empty((rows, n_par, n_par), dtype=torch.float64, device=dev)
            d_pu = torch.empty((B, n_par, m), dtype=torch.float64, device=dev)
            d_pd = torch.empty((B, n_par, m), dtype=torch.float64, device=dev)

        def difference(K):
            for l in range(n_par):
                eng.set_parameters_dev(d_TH[2 * l].data_ptr(), stream)
                eng.parameter_jacobian_dev(d_X.data_ptr(), d_pu.data_ptr(), d_F.data_ptr(), stream)
                eng.set_parameters_dev(d_TH[2 * l + 1].data_ptr(), stream)
                eng.parameter_jacobian_dev(d_X.data_ptr(), d_pd.data_ptr(), d_F.data_ptr(), stream)
                d_pu[0].sub_(d_pd[0])
                d_pu[0].mul_(0.5 / steps[l])
                d_D[:K, :, l].copy_(d_W[:K] @ d_pu[0].T)                           # [K, n_par]: column l of every S[d]
            eng.set_parameters_dev(d_TH[2 * n_par].data_ptr(), stream)

        def difference_batch():
            for l in range(n_par):
                batch.set_parameters_dev(B, d_THB[2 * l].data_ptr(), stream)
                batch.parameter_jacobian_dev(B, d_X.data_ptr(), d_pu.data_ptr(), d_F.data_ptr(), stream)
                batch.set_parameters_dev(B, d_THB[2 * l + 1].data_ptr(), stream)
                batch.parameter_jacobian_dev(B, d_X.data_ptr(), d_pd.data_ptr(), d_F.data_ptr(), stream)
                d_pu.sub_(d_pd)
                d_pu.mul_(0.5 / steps[l])
                d_D[:B, :, l].copy_(torch.bmm(d_pu, d_W[:B, :, None])[:, :, 0])    # lane c: dF[c] [n_par, m] times W[c]
            batch.set_parameters_dev(B, d_THB[2 * n_par].data_ptr(), stream)

        units = {"evaluation": lambda: eng.eval_dev(d_X.data_ptr(), d_F.data_ptr(), stream),
                 "parameter_jacobian": lambda: eng.parameter_jacobian_dev(d_X.data_ptr(), d_pu.data_ptr(), d_F.data_ptr(), stream)}
        for K in Ks:
            units["difference_%d" % K] = (lambda K=K: difference(K))
        units["difference_batch_%d" % B] = difference_batch
        if has_pp:
            for K in Ks:
                units["hessian_%d" % K] = (lambda K=K: eng.parameter_hessian_dev(d_X.data_ptr(), K, d_W.data_ptr(), d_S.data_ptr(),
                                                                                 d_F.data_ptr(), stream))
            units["hessian_batch_%d" % B] = lambda: batch.parameter_hessian_dev(B, d_X.data_ptr(), d_W.data_ptr(), d_S.data_ptr(),
                                                                                d_F.data_ptr(), stream)
        entry = {"problem": name, "n": n, "m": m, "parameters": list(prob.parameters), "module": os.path.basename(eng.module_path)}
        with torch.cuda.stream(stream_obj):
            for unit in units.values():                 # (every on-demand part is built and loaded before the clock runs)
                unit()
            stream_obj.synchronize()
            if has_pp:
                # the two ways agree to the difference's own noise, in units of the largest entry of the result
                K = Ks[-1]
                eng.parameter_hessian_dev(d_X.data_ptr(), K, d_W.data_ptr(), d_S.data_ptr(), d_F.data_ptr(), stream)
                difference(K)
                stream_obj.synchronize()
                entry["max_difference_from_the_jacobian_difference"] = float(
                    (d_S[:K] - d_D[:K]).abs().max() / torch.clamp(d_S[:K].abs().max(), min=1e-300))
                entry["largest_entry"] = float(d_S[:K].abs().max())
        entry.update(alternate(units))
        result["sizes"][tag] = entry
        print("%s: " % tag + ", ".join("%s %.2f" % (k, v["median_us"]) for k, v in entry.items()
                                       if isinstance(v, dict) and "median_us" in v) + " us", flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(json.dumps({"bench_parameter_hessian": "done", "host": result["host"], "out": out}))


if __name__ == "__main__":
    main()

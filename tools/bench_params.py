#!/usr/bin/env python
"""What a run-time parameter costs (Problem.parameter, og_set_parameters*, og_parameters_batch*; include/ogpsx.h) against
the module that has the same numbers baked in as literals, in one process on one GPU:

    python tools/bench_params.py [--sizes C3,C2] [--batches 1,8,32] [--out profiles/params_sweep.json]

Per problem three constants become parameters - one inside the dynamics, one in a boundary row, one bound (``PARAMS``).
In a baked problem a product of two constants (``obj.MaxG * obj.g0``) is a product of two Python floats: Python evaluates
it before the tracer sees it and it reaches the header as ONE literal.  The parameterised module reads an 8-byte table
entry where an immediate was and computes such parameter-only subexpressions in every thread.
Measured, forms alternating ``--rounds`` times, ``--reps`` HIP-event intervals per round around ``--inner`` back-to-back
units, p10 / median / p90:

  (a) the single-point sweep into a registered buffer (og_fd_sweep_dev): parameterised against baked;
  (b) the batched sweep (og_batch_fd_sweep_dev) at every B: the parameterised module with the handle's values in every
      lane (NULL) and with per-lane values - the lanes own a copy of the constant table either way - against the baked
      module's batch, whose lanes share one table;
  (d) the parameter launches alone: og_set_parameters_dev, og_parameters_batch_dev of B lanes.

``--setup`` adds what set_parameter saves, host clock: the set-up of a second solve (trace + header + loading the cached
module: ``HipEngine`` construction) against a cold build of the baked module's kernels (``build_module(force=True)``).
On a tree without parameters the baked legs remain: that is leg (c), the parent commit's batch by the same tool;
``--merge`` / ``--merge-parent`` put result files into one, the parent's under ``parent_commit``.

``--exact`` (default output profiles/params_exact.json) measures exact dF/dtheta instead, same method, at the same three
parameters per problem: og_parameter_jacobian_dev (an evaluation and one small launch) and og_parameter_jacobian_batch_dev
at every B, the forms alternating with the device path of the forward-difference ``parameter_sensitivity`` - per-lane
parameters and one batched evaluation of ``n_par + 1`` lanes.  On a tree without the exact calls only that path is timed:
the parent commit's leg, merged under ``parent_commit`` as above.  Nothing is gated on these times: the feature is
exactness."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"C2": "goddard", "C3": "polar_tsto", "C5": "launch4"}
# name -> (where it is read, how to fetch it from / store it into obj)
PARAMS = {"goddard": (("Hc", "dynamics"), ("Mf", "boundary row and bound"), ("T_max", "bound")),
          "polar_tsto": (("g0", "dynamics and bound"), ("Vtarget", "boundary row"), ("MaxG", "bound")),
          "launch4": (("c_q", "dynamics"), ("Vtarget", "boundary row"), ("MaxG", "bound"))}


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


def make(name, parameterised):
    from opengoddard_amd import problems
    prob, obj = problems.build(name)
    if parameterised:
        for attr, _where in PARAMS[name]:
            setattr(obj, attr, prob.parameter(attr, float(getattr(obj, attr))))
    return prob, obj


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="C3,C2")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=30, help="event intervals per round")
    ap.add_argument("--inner", type=int, default=10, help="repetitions of the unit inside one interval")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the forms")
    ap.add_argument("--exact", action="store_true", help="measure exact dF/dtheta against the FD device path instead")
    ap.add_argument("--setup", action="store_true", help="also time a second solve's set-up against a cold module build")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", metavar="JSON", default=None)
    ap.add_argument("--merge-parent", nargs="+", metavar="JSON", default=None)
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
        if a.commit:
            result["commit"] = a.commit
        if a.merge_parent:
            result["parent_commit"] = merged(a.merge_parent)
            result["parent_commit"]["note"] = (
                "the same tool on the parent commit's tree in the same lease: the FD device path only, there is no exact "
                "parameter Jacobian there" if result.get("mode") == "exact" else
                "the same tool on the parent commit's tree in the same lease: the baked legs only, there are no parameters there")
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
        return

    import torch
    from opengoddard_amd import _native, build, codegen, optimize
    from opengoddard_amd.engine import HipEngine
    if not torch.cuda.is_available() or _native.device_count() < 1:
        raise SystemExit("bench_params.py: no GPU; there is nothing to measure without one")
    has_params = hasattr(optimize.Problem, "parameter")
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

    result = {"tool": "tools/bench_params.py", "host": socket.gethostname(), "commit": a.commit or commit_of_tree(),
              "device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner, "rounds": a.rounds,
              "has_parameters": has_params, "sizes": {}}
    if a.exact:
        # exact dF/dtheta against the device path of the forward-difference parameter_sensitivity
        has_exact = hasattr(HipEngine, "parameter_jacobian_dev")
        result.update({"mode": "exact", "has_exact": has_exact})
        for tag in a.sizes.split(","):
            name = SIZES[tag]
            prob, obj = make(name, True)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                eng = HipEngine(prob, obj)
            n, m, n_par = eng.n, eng.m, eng.n_par
            lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
            ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
            x0 = np.clip(prob.p, lb, ub)
            theta = eng.get_parameters()
            h = _native.fd_step(theta, np.full(n_par, -np.inf), np.full(n_par, np.inf))
            TH = np.tile(theta, (n_par + 1, 1))
            TH[np.arange(1, n_par + 1), np.arange(n_par)] += h
            Bs = [int(v) for v in a.batches.split(",")]
            Bmax = max(Bs + [n_par + 1])
            with torch.cuda.stream(stream_obj):
                d_X = torch.from_numpy(np.tile(x0, (Bmax, 1))).to(dev)
                d_TH = torch.from_numpy(TH).to(dev)
                d_F = torch.empty((Bmax, m), dtype=torch.float64, device=dev)
                d_dF = torch.empty((Bmax, n_par, m), dtype=torch.float64, device=dev)
            fd_batch = eng.batch(n_par + 1)
            units = {"fd_device_path": lambda: (fd_batch.set_parameters_dev(n_par + 1, d_TH.data_ptr(), stream),
                                                fd_batch.values_dev(n_par + 1, d_X.data_ptr(), d_F.data_ptr(), stream))}
            batches = []
            if has_exact:
                units["exact_single"] = lambda: eng.parameter_jacobian_dev(d_X.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), stream)
                for B in Bs:
                    batch = eng.batch(B)
                    batches.append(batch)
                    units["exact_batch_%d" % B] = (lambda batch=batch, B=B: batch.parameter_jacobian_dev(
                        B, d_X.data_ptr(), d_dF.data_ptr(), d_F.data_ptr(), stream))
            entry = {"problem": name, "n": n, "m": m, "n_par": n_par, "parameters": {k: w for k, w in PARAMS[name]},
                     "fd_lanes": n_par + 1, "module": os.path.basename(eng.module_path)}
            entry.update(alternate(units))
            result["sizes"][tag] = entry
            print("%s exact: " % tag + ", ".join("%s %.2f us (p10 %.2f p90 %.2f)" % (k, v["median_us"], v["p10_us"], v["p90_us"])
                                                 for k, v in entry.items() if isinstance(v, dict) and "median_us" in v), flush=True)
            eng.close()
        out = a.out or os.path.join(ROOT, "profiles", "params_exact.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
        print(json.dumps({"bench_params": "done", "mode": "exact", "host": result["host"], "out": out}))
        return
    for tag in a.sizes.split(","):
        name = SIZES[tag]
        forms = {"baked": make(name, False)}
        if has_params:
            forms["parameterised"] = make(name, True)
        engines = {}
        for label, (prob, obj) in forms.items():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                engines[label] = HipEngine(prob, obj)
        prob = forms["baked"][0]
        eng0 = engines["baked"]
        n, m = eng0.n, eng0.m
        lb = np.array([-np.inf if b[0] is None else b[0] for b in prob.bounds], dtype=float)
        ub = np.array([np.inf if b[1] is None else b[1] for b in prob.bounds], dtype=float)
        rng = np.random.default_rng(20240 + n)
        x0 = np.clip(prob.p, lb, ub)
        entry = {"problem": name, "n": n, "m": m, "sweep_mode": eng0.sweep_mode,
                 "parameters": {k: w for k, w in PARAMS[name]}, "modules": {k: os.path.basename(e.module_path)
                                                                            for k, e in engines.items()}}
        result["sizes"][tag] = entry
        Bmax = max(int(v) for v in a.batches.split(","))
        X = np.stack([np.clip(x0 * (1.0 + 1e-3 * rng.standard_normal(n)), lb, ub) for _ in range(Bmax)])
        H = np.stack([_native.fd_step(x, lb, ub) for x in X])
        with torch.cuda.stream(stream_obj):
            d_X, d_H = torch.from_numpy(X).to(dev), torch.from_numpy(H).to(dev)
        # (a) single point, a registered buffer per form
        single, keep = {}, []
        for label, eng in engines.items():
            with torch.cuda.stream(stream_obj):
                d_F = torch.empty(m, dtype=torch.float64, device=dev)
                d_JT = torch.empty((n, m), dtype=torch.float64, device=dev)
                eng.register_jt_dev(d_JT.data_ptr(), 0, n, stream)
            keep.append((d_F, d_JT))
            single[label] = (lambda eng=eng, d_F=d_F, d_JT=d_JT:
                             eng.sweep_dev(d_X[0].data_ptr(), d_H[0].data_ptr(), 0, n, d_JT.data_ptr(), d_F.data_ptr(), stream))
        entry["single_dev"] = alternate(single)
        stream_obj.synchronize()
        if has_params:
            entry["single_dev"]["bitwise_equal_JT"] = bool(torch.equal(keep[0][1], keep[1][1]))
            par = engines["parameterised"]
            theta = par.get_parameters()
            with torch.cuda.stream(stream_obj):
                d_theta = torch.from_numpy(theta).to(dev)
            entry["set_parameters_dev"] = alternate({"handle": lambda: par.set_parameters_dev(d_theta.data_ptr(), stream)})["handle"]
        line = "%s single: " % tag + ", ".join("%s %.2f us (p10 %.2f p90 %.2f)" % (k, v["median_us"], v["p10_us"], v["p90_us"])
                                               for k, v in entry["single_dev"].items() if isinstance(v, dict))
        print(line, flush=True)
        # (b) / (c) batches
        entry["by_batch"] = {}
        for B in [int(v) for v in a.batches.split(",")]:
            units, batches, outs = {}, {}, {}
            for label, eng in engines.items():
                batch = batches[label] = eng.batch(B)
                with torch.cuda.stream(stream_obj):
                    d_Fb = torch.empty((B, m), dtype=torch.float64, device=dev)
                    d_V = torch.empty((B, batch.nnz), dtype=torch.float64, device=dev)
                outs[label] = (d_Fb, d_V)
                units["batch_" + label] = (lambda batch=batch, d_Fb=d_Fb, d_V=d_V:
                                           batch.sweep_dev(B, d_X.data_ptr(), d_H.data_ptr(), d_Fb.data_ptr(), d_V.data_ptr(), stream))
            row = {}
            if has_params:
                pb = batches["parameterised"]
                TH = np.tile(theta, (B, 1)) * (1.0 + 1e-3 * rng.standard_normal((B, theta.size)))
                with torch.cuda.stream(stream_obj):
                    d_TH = torch.from_numpy(TH).to(dev)
                sweep_par = units.pop("batch_parameterised")
                # NULL parameters first (every lane at the handle's values), then per-lane values: the same launch, what
                # differs is whether the lanes' tables hold the same numbers
                pb.set_parameters(None)
                part = alternate({"batch_baked": units["batch_baked"], "batch_parameterised_null": sweep_par})
                stream_obj.synchronize()
                row["bitwise_equal_values_null"] = bool(torch.equal(outs["baked"][1], outs["parameterised"][1]))
                pb.set_parameters(TH)
                part2 = alternate({"batch_parameterised_per_lane": sweep_par,
                                   "batch_parameters_dev": lambda: pb.set_parameters_dev(B, d_TH.data_ptr(), stream),
                                   "parameters_and_sweep": lambda: (pb.set_parameters_dev(B, d_TH.data_ptr(), stream), sweep_par())})
                row.update(part)
                row.update(part2)
            else:
                row.update(alternate(units))
            for batch in batches.values():
                batch.close()
            entry["by_batch"][str(B)] = row
            print("%s B=%-2d " % (tag, B) + ", ".join("%s %.2f" % (k.replace("batch_", ""), v["median_us"])
                                                      for k, v in row.items() if isinstance(v, dict)) + " us/launch", flush=True)
        if a.setup:
            # what set_parameter saves: the set-up of a second solve against a cold build of the baked module
            prob_p, obj_p = forms.get("parameterised", forms["baked"])
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                again = HipEngine(prob_p, obj_p)
            warm = time.perf_counter() - t0
            again.close()
            header = codegen.emit_header(codegen.trace_problem(*forms["baked"]))
            t0 = time.perf_counter()
            build.build_module(header, force=True, out_suffix=".cold")
            cold = time.perf_counter() - t0
            entry["setup"] = {"second_solve_setup_s": warm, "cold_module_build_s": cold,
                              "note": "HipEngine construction on the cached module (trace, header, dlopen, handle) against "
                                      "build_module(force=True) of the baked module's kernels; a baked re-solve pays both"}
            print("%s set-up: %.3f s with the cached module, %.2f s cold build" % (tag, warm, cold), flush=True)
        for eng in engines.values():
            eng.close()
    text = json.dumps(result, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps({"bench_params": "done", "host": result["host"], "out": a.out}))


if __name__ == "__main__":
    main()

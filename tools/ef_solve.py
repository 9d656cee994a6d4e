#!/usr/bin/env python
"""The extensive form of config 3 (farmer, 65,536 scenarios, cm = 1) by the Schur-complement
interior point (mpisppy_amd.opt.sc), one GPU: iterations, seconds to the
tolerance and mean milliseconds per iteration, with the objective it ends at.

One solve warms up (allocations), one is timed (host clock around ``solve()``; every iteration ends
in a wait for the device's record).  ``--path6`` adds the time of one cold path-6 solve of the same
batch (every scenario on its own, nothing fixed): the floor that one factorisation per scenario and
interior-point iteration sets.

    python tools/ef_solve.py [--scenarios 65536] [--cm 1] [--tol 1e-8] [--max-iter 100] [--path6]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mpi-sppy-1_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def _opt(S, cm, tol, max_iter):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.sc import SchurComplement
    o = {"toc": False, "device": "cuda:0", "batch_creator": farmer.batch_creator, "tol": tol, "max_iter": max_iter}
    return SchurComplement(o, farmer.scenario_names_creator(S), farmer.scenario_creator,
                           scenario_creator_kwargs={"crops_multiplier": cm, "num_scens": S})


def run_ef(S, cm, tol, max_iter):
    import torch
    out = {}
    for phase in ("warmup", "timed"):
        opt = _opt(S, cm, tol, max_iter)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = opt._run()
        wall = time.perf_counter() - t0
        if phase == "timed":
            r = opt.last
            e = opt.engine
            out = {"scenarios": S, "cm": cm, "nn": opt.batch.nn, "tol": tol, "converged": bool(done),
                   "iterations": opt.iterations, "seconds_iterations": opt.seconds, "seconds_total": wall,
                   "ms_per_iteration": 1e3 * opt.seconds / max(1, opt.iterations),
                   "objective": opt.objective_value(), "residuals": [r["pres"], r["dres"], r["gap"]],
                   "z": opt.root_nonants().tolist(), "workspace_MiB": e.workspace_bytes() / 2 ** 20
                   if hasattr(e, "workspace_bytes") else None,
                   "launches_per_iteration": sum(opt.engine.calls[k] for k in ("ef_schur", "ef_direction", "ef_step"))
                   / max(1, opt.iterations)}
        opt.engine.close()
    return out


def run_path6(S, cm):
    import torch
    from mpisppy_amd import _lib
    opt = _opt(S, cm, 1e-8, 1)
    opt._create_solvers()
    e = opt.engine
    e.set_terms(0, 0)
    e.fix_nonants(None)
    o = _lib.default_options()
    secs = []
    for _ in range(3):               # (the first compiles the pattern's module)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.solve(o, warm=False)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    it = e.iters.cpu().numpy()
    out = {"cold_path6_seconds": secs, "iterations_mean": float(it.mean()), "iterations_max": int(it.max()),
           "wait_and_see": opt.Eobjective()}
    e.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenarios", type=int, default=65536)
    p.add_argument("--cm", type=int, default=1)
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--max-iter", type=int, default=100)
    p.add_argument("--path6", action="store_true")
    a = p.parse_args()
    print(json.dumps({"ef": run_ef(a.scenarios, a.cm, a.tol, a.max_iter)}), flush=True)
    if a.path6:
        print(json.dumps({"path6": run_path6(a.scenarios, a.cm)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""PH on farmer with and without bundles (bundles_per_rank), one GPU: PH iterations
to a convergence threshold, the trivial bound, seconds per PH iteration and the interior-point
iterations per solve.

A bundle is the extensive form of a few scenarios, solved by the segmented interior point from a
cold start, so a bundled PH iteration costs tens of launches per interior-point iteration where
the unbundled one is a single launch: the gain is in PH iterations and in the bounds.  The
unbundled run of the same build is the baseline (a ``--sizes`` entry of 0 means no bundles; 1 is
one scenario per bundle, the same subproblems solved by the segmented interior point).

    python tools/bundle_convergence.py [--scenarios 1024] [--cm 1] [--sizes 0,1,8,64] [--rho 1.0]
                                       [--convthresh 1e-4] [--max-iter 500] [--bundle-tol 1e-10]
                                       [--bundle-step-tol 1e-8]

One JSON line per run.
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


def run(S, cm, size, rho, convthresh, max_iter, bundle_tol, bundle_step_tol):
    """``size`` scenarios per bundle (0: no bundles)."""
    import torch
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ph import PH
    o = {"solver_name": "mi355x_pdhg", "PHIterLimit": max_iter, "defaultPHrho": rho, "convthresh": convthresh,
         "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0",
         "batch_creator": farmer.batch_creator}
    if size:
        if S % size:
            raise SystemExit(f"--sizes: {size} does not divide {S} scenarios")
        # (the iteration counts of every solve are recorded with bundles only: recording turns the
        # unbundled loop's speculative solve off, which would slow the baseline down)
        o.update(bundles_per_rank=S // size, bundle_tol=bundle_tol, bundle_step_tol=bundle_step_tol, record_pdhg_iters=True)
    ph = PH(o, farmer.scenario_names_creator(S), farmer.scenario_creator,
            scenario_creator_kwargs={"crops_multiplier": cm, "num_scens": S})
    ph.PH_Prep()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tb = ph.Iter0()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ph.iterk_loop()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    st, last = ph.engine.status.cpu().numpy(), ph.engine.iters.cpu().numpy()
    its = ph.pdhg_iters or [(int(last.max()), float(last.mean()))]      # (unbundled: the last solve's)
    out = {"scenarios": S, "cm": cm, "scenarios_per_bundle": size, "bundles": S // size if size else 0, "rho": rho,
           "bundle_tol": bundle_tol if size else None, "bundle_step_tol": bundle_step_tol if size else None,
           "not_optimal_solves": getattr(ph, "bundle_griped", 0) if size else None, "convthresh": convthresh, "converged": bool(ph.converged), "ph_iterations": int(ph._PHIter),
           "conv": None if ph.conv is None else float(ph.conv), "trivial_bound": float(tb), "Eobjective": float(ph.Eobjective()),
           "seconds_iter0": t1 - t0, "seconds_per_ph_iteration": (t2 - t1) / max(1, ph._PHIter),
           "solver_iterations_max": max(m for m, _ in its), "solver_iterations_mean": sum(a for _, a in its) / len(its),
           "not_optimal_last_solve": int((st != 0).sum())}
    ph.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--cm", type=int, default=1)
    ap.add_argument("--sizes", default="0,1,8,64", help="scenarios per bundle, comma separated; 0: no bundles")
    ap.add_argument("--rho", type=float, default=1.0)
    ap.add_argument("--convthresh", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--bundle-tol", type=float, default=1e-10)
    ap.add_argument("--bundle-step-tol", type=float, default=1e-8)
    a = ap.parse_args()
    for size in [int(s) for s in a.sizes.split(",")]:
        print(json.dumps(run(a.scenarios, a.cm, size, a.rho, a.convthresh, a.max_iter, a.bundle_tol, a.bundle_step_tol)), flush=True)


if __name__ == "__main__":
    main()

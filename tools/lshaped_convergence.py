#!/usr/bin/env python
"""The L-shaped method against PH with its Lagrangian and xhat spokes: iterations and seconds to a
relative gap, and what an L-shaped iteration spends on the solve, the cuts and the master.

Config 3 (farmer, 65,536 scenarios, cm = 1) and farmer at 1,024 scenarios with cm = 10, one GPU.

L-shaped: ``LShapedMethod`` alone.  Its own gap after iteration k is (best E[f(x̂)] so far - the
outer bound of the master that produced x̂_k) / |outer bound|; reported are the first iteration
at which that is at most ``--gap``, the seconds up to there (host clock; every iteration ends in a
wait for the device), and the iteration at which no cut was added.  One run warms up (module
compilation), one is timed, and one more with a device synchronise after every phase gives the
split solve / cuts (cut pass, all-reduce, append) / master in milliseconds per iteration.

PH: ``ph_hub`` with ``lagrangian_spoke`` and ``xhatxbar_spoke`` in one process (co-located), stopped
by the hub at the same relative gap or after ``--ph-iters`` iterations; reported are the iterations
done, the gap reached and the seconds of the wheel.

    python tools/lshaped_convergence.py [--configs 65536:1,1024:10] [--gap 1e-5] [--ph-iters 300]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mpi-sppy-1_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def _lshaped(S, cm, **more):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.lshaped import LShapedMethod
    o = {"root_solver": "mi355x_pdhg", "sp_solver": "mi355x_pdhg", "toc": False, "device": "cuda:0",
         "batch_creator": farmer.batch_creator, "max_iter": 40}
    o.update(more)
    return LShapedMethod(o, farmer.scenario_names_creator(S), farmer.scenario_creator,
                         scenario_creator_kwargs={"crops_multiplier": cm, "num_scens": S})


def run_lshaped(S, cm, gap):
    import torch
    out = {}
    for phase in ("warmup", "timed", "split"):
        opt = _lshaped(S, cm, time_phases=(phase == "split"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = opt.lshaped_algorithm()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        h = opt.history
        if phase == "timed":
            best, hit = float("inf"), None
            outer = float(opt.etalb.sum())
            for k, (bound, q, added, mit, secs) in enumerate(h):
                best = min(best, q)
                g = (best - outer) / abs(outer)
                if hit is None and g <= gap:
                    hit = {"iteration": k + 1, "seconds": secs, "gap": g}
                outer = bound
            out.update({"scenarios": S, "cm": cm, "nn": opt.batch.nn, "cut_groups": opt.cut_groups,
                        "iterations_to_no_cut": len(h), "ended_without_a_cut": int(res["added"]) == 0,
                        "seconds_total": wall, "seconds_setup": wall - h[-1][4], "to_gap": hit,
                        "outer_bound": opt._LShaped_bound, "expected_cost": opt.Eobj_at_xhat,
                        "cuts_held": int(res["held"]), "master_iterations": [x[3] for x in h]})
        if phase == "split":
            n = len(h)
            out["ms_per_iteration"] = {k: 1e3 * v / n for k, v in opt.timing.items()}
        opt.engine.close()
    return out


def run_ph(S, cm, gap, iters):
    import torch
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    names = farmer.scenario_names_creator(S)
    kw = {"crops_multiplier": cm, "num_scens": S}
    out = {}
    for phase, n in (("warmup", 3), ("timed", iters)):
        cfg = SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=n, rel_gap=gap,
                              intra_hub_conv_thresh=-1.0, device="cuda:0", toc=False, batch_creator=farmer.batch_creator,
                              iterk_solver_options=dict(farmer.PDHG_ITERK_OPTIONS))
        hub = vanilla.ph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
        spokes = [vanilla.lagrangian_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw),
                  vanilla.xhatxbar_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)]
        ws = WheelSpinner(hub, spokes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ws.spin(placement="colocated")
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        h = ws.spcomm
        if phase == "timed":
            _, rel = h.compute_gaps()
            out = {"iterations": int(h.opt._PHIter), "iteration_cap": n, "gap": rel, "seconds": wall,
                   "outer": ws.BestOuterBound, "inner": ws.BestInnerBound}
        for s in ws.spokes:
            s.opt.engine.close()
        h.opt.engine.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--configs", default="65536:1,1024:10", help="scenarios:crops_multiplier, comma separated")
    p.add_argument("--gap", type=float, default=1e-5)
    p.add_argument("--ph-iters", type=int, default=300)
    p.add_argument("--no-ph", action="store_true")
    a = p.parse_args()
    for c in a.configs.split(","):
        S, cm = (int(v) for v in c.split(":"))
        try:
            row = {"lshaped": run_lshaped(S, cm, a.gap)}
        except RuntimeError as ex:      # (a master that was not solved: reported, the next config still runs)
            row = {"lshaped": {"scenarios": S, "cm": cm, "failed": str(ex)}}
        print(json.dumps(row), flush=True)
        if not a.no_ph:
            row = {"scenarios": S, "cm": cm, "ph_wheel": run_ph(S, cm, a.gap, a.ph_iters)}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

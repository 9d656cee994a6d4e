#!/usr/bin/env python
"""The extensive form of config 3 (farmer, 65,536 scenarios, cm = 1) by the Schur-complement
interior point (mpisppy_amd.opt.sc), one GPU: iterations, seconds to the
tolerance and mean milliseconds per iteration, with the objective it ends at.

One solve warms up (allocations), one is timed (host clock around ``solve()``; every iteration ends
in a wait for the device's record).  ``--path6`` adds the time of one cold path-6 solve of the same
batch (every scenario on its own, nothing fixed): the floor that one factorisation per scenario and
interior-point iteration sets.

    python tools/ef_solve.py [--scenarios 65536] [--cm 1] [--tol 1e-8] [--max-iter 100] [--path6]

``--model aircond --bf a,b,c`` solves the MULTISTAGE extensive form of aircond on that tree instead
(mpisppy_amd.opt.ef; config 4's parameters: ``--bf 32,32,64`` is config 4's tree)
``--passes`` times over after the warm-up, and with ``--ph`` runs PH on the same tree to its
convergence (conv < 1e-2, as tests/test_gpu_config4.py does) and reports the relative difference
between the extensive form's objective and PH's expected objective there.

    python tools/ef_solve.py --model aircond --bf 4,3,2 [--passes 3] [--ph]
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


# config 4's parameters (bench.py AIRCOND_KW)
AIRCOND_KW = {"Capacity": 200, "QuadShortCoeff": 0.3, "BeginInventory": 50, "mu_dev": 0, "sigma_dev": 40, "start_seed": 0}


def _aircond(cls, bf, **options):
    import numpy as np
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import create_nodenames_from_branching_factors
    o = {"toc": False, "device": "cuda:0", "batch_creator": aircond.batch_creator}
    o.update(options)
    return cls(o, aircond.scenario_names_creator(int(np.prod(bf))), aircond.scenario_creator,
               scenario_creator_kwargs={"branching_factors": list(bf), **AIRCOND_KW},
               all_nodenames=create_nodenames_from_branching_factors(list(bf)))


def run_tree(bf, tol, max_iter, passes):
    """One warm-up solve, then ``passes`` timed ones (host clock around the iterations, which end in
    a device synchronisation): every pass's seconds, and the median's milliseconds per iteration."""
    import torch
    from mpisppy_amd.opt.ef import ExtensiveForm
    from mpisppy_amd.spopt import SOLVER_NAMES
    ef = _aircond(ExtensiveForm, bf, solver=SOLVER_NAMES[0], tol=tol, max_iter=max_iter)
    secs = []
    for p in range(passes + 1):
        torch.cuda.synchronize()
        res = ef.solve_extensive_form()
        if p:
            secs.append(ef.seconds)
    r, e, it = ef.last, ef.engine, max(1, ef.iterations)
    med = sorted(secs)[len(secs) // 2]
    out = {"bf": list(bf), "scenarios": ef.batch.S, "nodes": len(ef.batch.node_names), "nn": ef.batch.nn, "ztot": e.eft_ztot,
           "tol": tol, "converged": res.solver.termination_condition == "optimal", "iterations": ef.iterations,
           "seconds_passes": secs, "seconds_median": med, "ms_per_iteration": 1e3 * med / it,
           "objective": ef.get_objective_value(), "residuals": [r["pres"], r["dres"], r["gap"]],
           "root": ef.root_nonants().tolist(), "workspace_MiB": e.workspace_bytes() / 2 ** 20,
           "entry_calls_per_iteration": sum(e.calls[k] for k in ("eft_schur", "eft_direction", "eft_step")) / (it + 1),
           # not counted: what phgpu_eft_schur / _direction / _step launch by construction
           "launches_per_iteration_by_construction": 23 + 4 * (ef.batch.depth - 1)}
    e.close()
    return out


def run_ph(bf):
    """PH on the same tree to conv < 1e-2 with the model's interior-point constants: its expected
    objective there."""
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.opt.ph import PH
    ph = _aircond(PH, bf, solver_name="mi355x_pdhg", PHIterLimit=40, defaultPHrho=1.0, convthresh=0.01, verbose=False,
                  display_progress=False, ipm_tuning=aircond.IPM_TUNING)
    t0 = time.perf_counter()
    _, eobj, tbound = ph.ph_main()
    out = {"ph_iterations": ph._PHIter, "ph_converged": bool(ph.converged), "ph_seconds": time.perf_counter() - t0,
           "ph_expected_objective": eobj, "ph_trivial_bound": tbound}
    ph.engine.close()
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
    p.add_argument("--model", choices=["farmer", "aircond"], default="farmer")
    p.add_argument("--bf", type=lambda v: [int(t) for t in v.split(",")], default=[4, 3, 2],
                   help="aircond branching factors (scenarios = their product)")
    p.add_argument("--passes", type=int, default=3, help="timed solves after the warm-up (aircond)")
    p.add_argument("--ph", action="store_true", help="aircond: PH on the same tree, for its expected objective")
    a = p.parse_args()
    if a.model == "aircond":
        out = run_tree(a.bf, a.tol, a.max_iter, a.passes)
        if a.ph:
            out.update(run_ph(a.bf))
            out["rel_diff_to_ph"] = abs(out["objective"] - out["ph_expected_objective"]) / abs(out["ph_expected_objective"])
        print(json.dumps({"ef_tree": out}), flush=True)
        return
    print(json.dumps({"ef": run_ef(a.scenarios, a.cm, a.tol, a.max_iter)}), flush=True)
    if a.path6:
        print(json.dumps({"path6": run_path6(a.scenarios, a.cm)}), flush=True)


if __name__ == "__main__":
    main()

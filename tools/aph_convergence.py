#!/usr/bin/env python
"""PH against APH at dispatch_frac 1, 0.5 and 0.25: iterations, seconds, and what APH's own
passes and its list solve cost per iteration.

Config 3 (farmer, 65,536 scenarios, cm = 1, rho = 1) and a small config (farmer, 1,024 scenarios),
one GPU.  Every mode runs ``--iters`` iterations from a fresh object (convthresh 0: nothing stops
early), once to warm up (module compilation, first launches) and ``--repeats`` times timed, the
modes alternating.  Reported per mode: seconds for the loop after Iter0 (host clock around work
that ends in a device synchronise), the mode's own convergence metric at the end, and one metric
both algorithms share, sum_s p_s |x_s - x̄|_1 of the last solves; for APH also, by HIP events in a
run of their own (each event pair is a marker that idles the GPU a few microseconds), the
milliseconds per iteration of the projective passes (phgpu_aph_reduce, _norms, _update), of the
selection, of the solve of the dispatch (full or list) and of phgpu_aph_mark.

    python tools/aph_convergence.py [--scens 65536,1024] [--iters 50] [--repeats 3] [--fracs 1,0.5,0.25]

PHGPU_LIB selects the library (the PH row of DESIGN.md 7.6 was taken with the parent commit's).
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


def _options(a, iters, **more):
    from mpisppy_amd.examples import farmer
    o = {"solver_name": "mi355x_pdhg", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": 0.0, "verbose": False,
         "display_progress": False, "toc": False, "device": "cuda:0", "batch_creator": farmer.batch_creator,
         "iterk_solver_options": dict(farmer.PDHG_ITERK_OPTIONS)}
    o.update(more)
    return o


def _make(a, S, mode, iters):
    from mpisppy_amd.examples import farmer
    names = farmer.scenario_names_creator(S)
    kw = {"crops_multiplier": 1, "num_scens": S}
    if mode == "ph":
        from mpisppy_amd.opt.ph import PH
        return PH(_options(a, iters), names, farmer.scenario_creator, scenario_creator_kwargs=kw)
    from mpisppy_amd.opt.aph import APH
    return APH(_options(a, iters, dispatch_frac=float(mode), APHgamma=1.0, APHnu=1.0), names, farmer.scenario_creator,
               scenario_creator_kwargs=kw)


def _spread(opt):
    """sum_s p_s |x_s - x̄|_1 with x̄ the probability-weighted mean of the last solves' nonants
    (two-stage: one node)."""
    e = opt.engine
    xn = e.nonant_x_dev()[:e.nn]
    xb = (xn * e.prob).sum(1, keepdim=True) / e.prob.sum()
    return float(((xn - xb).abs().sum(0) * e.prob).sum().item())


def run_once(a, S, mode, iters, events=False):
    import torch
    opt = _make(a, S, mode, iters)
    spans = {}
    if mode == "ph":
        opt.PH_Prep()
        opt.Iter0()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.iterk_loop()
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
    else:
        opt.PH_Prep()
        opt.Iter0()
        e = opt.engine
        e.aph_init(use_lag=opt.use_lag)
        e.aph_bind(True)
        if events:
            def timed(name, fn):
                def wrapped(*args, **kw):
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[0].record()
                    r = fn(*args, **kw)
                    ev[1].record()
                    spans.setdefault(name, []).append(ev)
                    return r
                return wrapped
            for name, attr in (("passes", "aph_reduce"), ("passes", "aph_norms"), ("passes", "aph_update"),
                               ("select", "select_smallest"), ("solve_list", "solve_list"), ("solve_full", "solve"),
                               ("mark", "aph_mark")):
                setattr(e, attr, timed(name, getattr(e, attr)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.APH_iterk(None)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        e.aph_bind(False)
    res = {"mode": mode, "scenarios": S, "iterations": int(opt._PHIter), "seconds": secs, "conv": opt.conv,
           "spread": _spread(opt), "ms_per_iteration": 1e3 * secs / max(1, int(opt._PHIter))}
    if spans:
        n = max(1, int(opt._PHIter))
        res["device_ms_per_iteration"] = {k: sum(p[0].elapsed_time(p[1]) for p in v) / n for k, v in spans.items()}
        res["launches"] = {k: len(v) for k, v in spans.items()}
    opt.engine.close()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scens", default="65536,1024")
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--fracs", default="1,0.5,0.25")
    p.add_argument("--modes", default=None, help="comma list of ph and fractions (default: ph and every --fracs)")
    a = p.parse_args()
    modes = a.modes.split(",") if a.modes else ["ph"] + a.fracs.split(",")
    out = []
    for S in (int(s) for s in a.scens.split(",")):
        for m in modes:                                   # warm-up: compilation and first launches
            run_once(a, S, m, min(a.iters, 5))
        rows = {m: [] for m in modes}
        for _ in range(a.repeats):                        # the modes alternate
            for m in modes:
                rows[m].append(run_once(a, S, m, a.iters))
        for m in modes:
            secs = sorted(r["seconds"] for r in rows[m])
            r = dict(rows[m][0])
            r["seconds_all"] = secs
            r["seconds"] = secs[len(secs) // 2]
            r["ms_per_iteration"] = 1e3 * r["seconds"] / max(1, r["iterations"])
            if m != "ph":
                ev = run_once(a, S, m, a.iters, events=True)
                r["device_ms_per_iteration"] = ev["device_ms_per_iteration"]
                r["launches"] = ev["launches"]
            out.append(r)
            d = r.get("device_ms_per_iteration", {})
            print(f"# S {S:6d}  {('PH' if m == 'ph' else 'APH ' + m):9s} {r['iterations']:4d} iterations  "
                  f"{r['seconds']:.4f} s (median of {len(secs)}: {' '.join(f'{v:.4f}' for v in secs)})  "
                  f"{r['ms_per_iteration']:.4f} ms / iteration  conv {r['conv'] or float('nan'):.4e}  spread {r['spread']:.4e}" +
                  ("" if not d else "  device ms / iteration: " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(d.items()))),
                  flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What an FWPH outer iteration costs, and what its bound buys a wheel.

Config 3 (farmer, 65,536 scenarios, cm = 1, rho = 1), one GPU.

1. FWPH alone for ``--iters`` outer iterations: milliseconds per outer iteration by HIP events,
   split into the LP solve launches, the column passes (phgpu_fwph_column) and the x̄ / W step
   (phgpu_ph_reduce + phgpu_ph_update_ex on the QP points); and per inner iteration the column
   pass next to the LP solve launch it follows.
2. A wheel -- PH hub + fwph + lagrangian + xhatshuffle, co-located -- for ``--limit`` hub
   iterations: the outer bound of the FWPH spoke and of the Lagrangian spoke against wall time.

    python tools/fwph_bounds.py [--scens 65536] [--iters 10] [--limit 30] [--fw-iter-limit 3]
                                [--fw-weight 0.0] [--max-columns 32]
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


def _cfg(a, limit):
    from mpisppy_amd.examples import farmer
    return SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=limit, rel_gap=1e-9,
                           intra_hub_conv_thresh=-1.0, device="cuda:0", toc=False, verbose=False,
                           batch_creator=farmer.batch_creator, iterk_solver_options=dict(farmer.PDHG_ITERK_OPTIONS),
                           fwph_iter_limit=a.fw_iter_limit, fwph_weight=a.fw_weight, fwph_conv_thresh=1e-4,
                           fwph_stop_check_tol=1e-4, fwph_max_columns=a.max_columns)


def fwph_alone(a):
    import torch
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    S = a.scens
    names = farmer.scenario_names_creator(S)
    d = vanilla.fwph_spoke(_cfg(a, a.iters), farmer.scenario_creator, None, names,
                           scenario_creator_kwargs={"crops_multiplier": 1, "num_scens": S})
    opt = d["opt_class"](**d["opt_kwargs"])
    best = opt.fw_prep()
    e = opt.engine
    spans = {"solve": [], "column": [], "xbar_W": []}

    def timed(name, fn):
        def wrapped(*args, **kw):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            r = fn(*args, **kw)
            ev[1].record()
            spans[name].append(ev)
            return r
        return wrapped
    e.solve = timed("solve", e.solve)
    e.fwph_column = timed("column", e.fwph_column)
    e.fwph_xbar_step = timed("xbar_W", e.fwph_xbar_step)
    rows = []
    for itr in range(a.iters):
        n0 = {k: len(v) for k, v in spans.items()}
        torch.cuda.synchronize()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        t0 = time.perf_counter()
        ev[0].record()
        best, stop = opt.fw_step(itr, best)
        ev[1].record()
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        ms = {k: [p[0].elapsed_time(p[1]) for p in v[n0[k]:]] for k, v in spans.items()}
        st = e.fwph_export()
        rows.append({"iteration": itr + 1, "bound": opt._local_bound, "diff": opt.fw_last_diff,
                     "inner_iterations": opt.fw_inner_iters[-1], "wall_ms": wall, "gpu_ms": ev[0].elapsed_time(ev[1]),
                     "solve_ms": ms["solve"], "column_ms": ms["column"], "xbar_W_ms": sum(ms["xbar_W"]),
                     "columns_max": int(st["ncols"].max()), "columns_mean": float(st["ncols"].mean())})
        r = rows[-1]
        print(f"# FWPH {itr + 1:3d}  bound {r['bound']!s:>20}  diff {r['diff']:.4e}  {r['inner_iterations']} inner  "
              f"{wall:8.3f} ms wall  LP " + " ".join(f"{v:.3f}" for v in r["solve_ms"]) + "  column " +
              " ".join(f"{v:.3f}" for v in r["column_ms"]) + f"  x̄/W {r['xbar_W_ms']:.3f}  K <= {r['columns_max']}",
              flush=True)
        if stop:
            break
    ws = e.workspace_bytes()
    e.close()
    tot = lambda k: sum(sum(r[k]) if isinstance(r[k], list) else r[k] for r in rows) / len(rows)   # noqa: E731
    res = {"what": "fwph_alone", "scenarios": S, "outer_iterations": len(rows), "trivial_bound": opt.trivial_bound,
           "ms_per_outer_wall": sum(r["wall_ms"] for r in rows) / len(rows),
           "ms_per_outer_solves": tot("solve_ms"), "ms_per_outer_columns": tot("column_ms"),
           "ms_per_outer_xbar_W": tot("xbar_W_ms"), "workspace_bytes": ws, "rows": rows}
    return res


def wheel(a):
    import torch
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    S = a.scens
    names = farmer.scenario_names_creator(S)
    cfg = _cfg(a, a.limit)
    kw = {"crops_multiplier": 1, "num_scens": S}
    which = ["fwph", "lagrangian", "xhatshuffle"]
    hub = vanilla.ph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
    spokes = [getattr(vanilla, w + "_spoke")(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
              for w in which]
    trace = {w: [] for w in which[:2]}
    t0 = [None]
    ws = WheelSpinner(hub, spokes)
    for w, sd in zip(which[:2], spokes):
        cls = sd["spoke_class"]

        def make(w, cls):
            main0, work0 = cls.main, cls.do_work

            def main(self):
                if t0[0] is None:
                    torch.cuda.synchronize()
                    t0[0] = time.perf_counter()
                main0(self)
                torch.cuda.synchronize()
                trace[w].append((time.perf_counter() - t0[0], float(self.bound)))

            def do_work(self):
                n = self.local_write_id
                work0(self)
                if self.local_write_id != n:
                    torch.cuda.synchronize()
                    trace[w].append((time.perf_counter() - t0[0], float(self.bound)))
            cls.main, cls.do_work = main, do_work
            return main0, work0
        sd["_orig"] = make(w, cls)
    try:
        ws.spin(placement="colocated")
    finally:
        for sd in spokes[:2]:
            sd["spoke_class"].main, sd["spoke_class"].do_work = sd["_orig"]
    h = ws.spcomm
    res = {"what": "wheel", "spokes": which, "scenarios": S, "ph_iterations": int(h.opt._PHIter),
           "inner": ws.BestInnerBound, "outer": ws.BestOuterBound,
           "last_outer_from": None if not h.last_ob_idx else which[h.last_ob_idx - 1], "trace": trace}
    for w in which[:2]:
        best = -float("inf")
        for t, b in trace[w]:
            if b > best:
                best = b
                print(f"# {w:10s} {t:9.4f} s  best outer bound {best:.4f}", flush=True)
    for sp in ws.spokes:
        sp.opt.engine.close()
    h.opt.engine.close()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scens", type=int, default=65536)
    p.add_argument("--iters", type=int, default=10, help="outer iterations of FWPH alone")
    p.add_argument("--limit", type=int, default=30, help="PH iteration limit of the wheel's hub")
    p.add_argument("--fw-iter-limit", type=int, default=3)
    p.add_argument("--fw-weight", type=float, default=0.0)
    p.add_argument("--max-columns", type=int, default=32)
    p.add_argument("--no-wheel", action="store_true")
    a = p.parse_args()
    r = fwph_alone(a)
    print(f"# FWPH alone, {r['scenarios']} scenarios: {r['ms_per_outer_wall']:.3f} ms wall per outer iteration = LP solve "
          f"launches {r['ms_per_outer_solves']:.3f} + column passes {r['ms_per_outer_columns']:.3f} + x̄ / W step "
          f"{r['ms_per_outer_xbar_W']:.3f} ms (HIP events) + host; workspace {r['workspace_bytes'] / 2**20:.1f} MiB",
          flush=True)
    print(json.dumps(r), flush=True)
    if not a.no_wheel:
        print(json.dumps(wheel(a)), flush=True)


if __name__ == "__main__":
    main()

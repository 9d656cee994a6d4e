#!/usr/bin/env python
"""What the x̄ inner-bound spoke buys a wheel, and what it costs per sync.

The config-3 wheel (farmer, 65,536 scenarios, cm = 1, rho = 1; PH hub + Lagrangian +
xhatshuffle, co-located on one GPU) runs to ``rel_gap`` twice: as it is, and with
XhatXbarInnerBound added (``--spokes`` can add the slam heuristics too).  Per run: PH
iterations and wall seconds of the hub's main loop to the gap, the final bounds, which spoke
gave the last inner bound, and the mean wall milliseconds of one hub sync (delivery, every
spoke's pass, bounds back).  The extra milliseconds per sync of the added spokes is the
difference of the two means; the tool also times the added spoke's pass on its own at the
end of its run (HIP events around ``do_work``, the last nonants delivered again).

    python tools/xhat_bounds.py [--scens 65536] [--rel-gap 1e-3] [--limit 300]
                                [--spokes xhatxbar[,slammin,slammax]] [--tries-per-sync 1]
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

BASE = ["lagrangian", "xhatshuffle"]


def run_wheel(a, which):
    import torch
    from mpisppy_amd.cylinders import hub as hubmod
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    S = a.scens
    names = farmer.scenario_names_creator(S)
    cfg = SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=a.limit, rel_gap=a.rel_gap,
                          intra_hub_conv_thresh=-1.0, device="cuda:0", toc=False, batch_creator=farmer.batch_creator,
                          iterk_solver_options=dict(farmer.PDHG_ITERK_OPTIONS), xhat_tries_per_sync=a.tries_per_sync)
    kw = {"crops_multiplier": 1, "num_scens": S}
    hub = vanilla.ph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
    spokes = [getattr(vanilla, w + "_spoke")(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
              for w in which]
    t = {"main": 0.0, "sync": 0.0, "syncs": 0}
    main0, sync0 = hubmod.PHHub.main, hubmod.PHHub.sync

    def main(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        main0(self)
        torch.cuda.synchronize()
        t["main"] = time.perf_counter() - t0

    def sync(self):
        # the spokes' passes read their bounds back, so a sync ends synchronised already;
        # its start is not (the hub's solve may still run): that wait is the hub's, not the sync's
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sync0(self)
        t["sync"] += time.perf_counter() - t0
        t["syncs"] += 1

    hubmod.PHHub.main, hubmod.PHHub.sync = main, sync
    try:
        ws = WheelSpinner(hub, spokes)
        ws.spin()
    finally:
        hubmod.PHHub.main, hubmod.PHHub.sync = main0, sync0
    h = ws.spcomm
    gap = (ws.BestInnerBound - ws.BestOuterBound) / abs(ws.BestOuterBound)
    res = {"spokes": which, "scenarios": S, "rel_gap_target": a.rel_gap, "ph_iterations": int(h.opt._PHIter),
           "reached_gap": bool(gap <= a.rel_gap), "main_seconds": t["main"], "syncs": t["syncs"],
           "ms_per_sync": 1e3 * t["sync"] / max(1, t["syncs"]), "inner": ws.BestInnerBound,
           "outer": ws.BestOuterBound, "rel_gap": gap,
           "last_inner_from": None if not h.last_ib_idx else which[h.last_ib_idx - 1],
           "spoke_bounds": {w: float(sp.bound) for w, sp in zip(which, ws.spokes)}}
    extra = {}
    for w, sp in zip(which, ws.spokes):
        if w in BASE:
            continue
        sp._killed = False
        reps = 20
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        t0 = None
        for r in range(reps + 2):
            if r == 2:
                torch.cuda.synchronize()
                ev[0].record()
                t0 = time.perf_counter()
            sp._deliver(sp.remote_write_id + 1, h._nonant_snapshot)
            sp.got_kill_signal()
            sp.do_work()
        ev[1].record()
        ev[1].synchronize()
        extra[w] = {"wall_ms_per_pass": 1e3 * (time.perf_counter() - t0) / reps,
                    "gpu_ms_per_pass": ev[0].elapsed_time(ev[1]) / reps}
    res["added_spoke_pass"] = extra
    for sp in ws.spokes:
        sp.opt.engine.close()
    h.opt.engine.close()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scens", type=int, default=65536)
    p.add_argument("--rel-gap", type=float, default=1e-3)
    p.add_argument("--limit", type=int, default=300, help="PH iteration limit of the hub")
    p.add_argument("--spokes", default="xhatxbar", help="spokes added in the second run (xhatxbar, slammin, slammax)")
    p.add_argument("--tries-per-sync", type=int, default=1, help="xhatshuffle candidates per sync")
    a = p.parse_args()
    added = [s.strip() for s in a.spokes.split(",") if s.strip()]
    out = []
    for which in (BASE, BASE + added):
        r = run_wheel(a, which)
        out.append(r)
        print(f"# {'+'.join(which):40s} {r['ph_iterations']:4d} PH iterations  {r['main_seconds']:7.3f} s  "
              f"{r['ms_per_sync']:.3f} ms / sync  inner {r['inner']:.4f}  outer {r['outer']:.4f}  "
              f"gap {r['rel_gap']:.3e}  reached {r['reached_gap']}  last inner bound from {r['last_inner_from']}",
              flush=True)
        print(json.dumps(r), flush=True)
    print(f"# extra ms per sync with {'+'.join(added)}: {out[1]['ms_per_sync'] - out[0]['ms_per_sync']:.3f}", flush=True)


if __name__ == "__main__":
    main()

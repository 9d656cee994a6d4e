#!/usr/bin/env python
"""The Mak-Morton-Wood confidence interval of a PH candidate on farmer, one GPU: what the
one-launch form costs, phase by phase, next to the same interval computed batch by batch.

1. x̂: x̄ of a short PH run (``--ph-iters``) on the first ``--xhat-scens`` scenarios.
2. ``MMWConfidenceIntervals`` over ``--batches`` batches of ``--batch-size`` new scenarios (32 x
   2,048 by default, the scenario count of config 3): seconds in the x* runs (one L-shaped run per
   batch), in the two batched solves and in the moments pass, each ended by a device synchronise.
3. The same interval from ``gap_estimators`` called once per batch (the reference's loop,
   mmw_ci.py:144-166): the check, and the baseline.
4. The moments pass (phgpu_gap_moments) next to phgpu_expectations on the merged engine, by HIP
   events over ``--reps`` calls after a warm-up.

    python tools/mmw_ci.py [--batches 32] [--batch-size 2048] [--xhat-scens 30] [--ph-iters 50]
                           [--reps 200] [--no-loop] [--out FILE]

``--model aircond --bf a,b,c`` runs the MULTISTAGE interval instead (EF_mstage) on
sample trees with those branching factors: per batch G and s, the interior-point iterations of the
free extensive form and of each stage's conditioned one, and the seconds spent in the free extensive
form, the conditioned ones and the two evaluations.  Then, unless ``--no-loop``, the reference's walk
on the first batch's sample tree -- one SampleSubtree per node -- for its time and the largest
iteration count among the subtrees of each stage: what sharing one mu and one pair of step lengths
over a stage's subtrees costs, and what solving a stage at once buys.

    python tools/mmw_ci.py --model aircond --bf 4,3,2 [--batches 3] [--no-loop] [--out FILE]
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

SOLVER = "mi355x_pdhg"


def candidate(a):
    """x̄ of a short PH run: a first-stage feasible candidate (the acreage row is convex)."""
    import numpy as np
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.ph import PH
    names = farmer.scenario_names_creator(a.xhat_scens)
    opts = {"solver_name": SOLVER, "PHIterLimit": a.ph_iters, "defaultPHrho": 1.0, "convthresh": 1e-8,
            "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0",
            "batch_creator": farmer.batch_creator, "iterk_solver_options": dict(farmer.PDHG_ITERK_OPTIONS)}
    ph = PH(opts, names, farmer.scenario_creator, scenario_creator_kwargs={"num_scens": a.xhat_scens})
    conv, _, tb = ph.ph_main()
    x = np.array(ph.xbar_by_node()["ROOT"][:3], dtype=np.float64)
    ph.engine.close()
    return x, float(conv), float(tb)


def moments_next_to_expectations(a, xhat, start):
    """ms per call of gap_moments (device part) and of phgpu_expectations on one engine."""
    import numpy as np
    import torch
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    S = a.batches * a.batch_size
    ev = Xhat_Eval({"solver_name": SOLVER, "toc": False, "device": "cuda:0", "batch_creator": farmer.batch_creator},
                   farmer.scenario_names_creator(S, start=start), farmer.scenario_creator,
                   scenario_creator_kwargs={"num_scens": a.batch_size})
    ev._lazy_create_solvers()
    e = ev.engine
    ev._fix_nonants({"ROOT": xhat})
    ev.solve_loop()
    f_hat, st_hat = e.obj.clone(), e.status.clone()
    seg = torch.arange(a.batches + 1, dtype=torch.int64, device=e.device) * a.batch_size
    out = torch.zeros((a.batches, 8), dtype=torch.float64, device=e.device)
    from mpisppy_amd import _lib
    from mpisppy_amd.engine import _ptr

    def moments():
        _lib.check(e.lib.phgpu_gap_moments(e.h, _ptr(f_hat), _ptr(st_hat), _ptr(e.obj), _ptr(e.status), _ptr(seg),
                                           a.batches, 0, _ptr(out), e._stream()), "phgpu_gap_moments")

    def expectations():
        _lib.check(e.lib.phgpu_expectations(e.h, _ptr(e.obj), _ptr(e.bound), _ptr(e.status), _ptr(e.exp_buf),
                                            e._stream()), "phgpu_expectations")
    res = {}
    for rnd in range(2):            # the two alternate; the second round is reported
        for name, fn in (("gap_moments", moments), ("expectations", expectations)):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            t = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            t[0].record()
            for _ in range(a.reps):
                fn()
            t[1].record()
            torch.cuda.synchronize()
            res.setdefault(name + "_ms_per_call", []).append(t[0].elapsed_time(t[1]) / a.reps)
    res["left_out"] = float(np.asarray(out.cpu())[:, 6].sum())
    e.close()
    return res


def aircond_interval(a):
    """The multistage interval on aircond (module docstring)."""
    import numpy as np
    import torch
    from mpisppy_amd.confidence_intervals import ciutils, sample_tree
    from mpisppy_amd.examples import aircond
    from mpisppy_amd.sputils import number_of_nodes
    bfs = [int(v) for v in a.bf.split(",")]
    S = int(np.prod(bfs))
    cfg = {"branching_factors": bfs, "EF_mstage": True, "EF_solver_name": SOLVER, "device": "cuda:0"}
    t0 = time.perf_counter()
    xhat = ciutils.ef_xstar_solver(aircond, solver_name=SOLVER, device="cuda:0")(
        aircond.scenario_names_creator(S), {"branching_factors": bfs, "start_seed": 0})
    print(f"xhat_one {xhat} from the extensive form of a {bfs} tree at seed 0 ({time.perf_counter() - t0:.3f} s)", flush=True)
    res = {"model": "aircond", "bf": bfs, "xhat_one": xhat.tolist(), "batches": []}
    seed = S
    for rnd, nb in (("warm-up", 1), ("timed", a.batches)):          # the first round loads the code objects
        s0 = seed
        for b in range(nb):
            info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                est = ciutils.gap_estimators({"ROOT": xhat}, aircond, solving_type="EF_mstage",
                                             sample_options={"branching_factors": bfs, "seed": s0}, cfg=cfg, solver_name=SOLVER,
                                             info=info)
            except RuntimeError as err:                # (an extensive form short of its tolerance: say where it stopped)
                print(f"[{rnd}] batch {b} (seed {s0}): no estimate: {err}", flush=True)
                res.setdefault("failed", []).append({"seed": s0, "error": str(err)})
                break
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            sec, it = info["seconds"], info["iterations"]
            print(f"[{rnd}] batch {b} (seed {s0}): G {est['G']:.6f} s {est['s']:.6f}; iterations free {it['free']} conditioned "
                  f"{it['conditioned']}; seconds {wall:.3f}: free {sec['free']:.4f} conditioned {sec['conditioned']:.4f} "
                  f"(solves {['%.4f' % v for v in info['walk']['seconds']]}) evaluations {sec['evaluations']:.4f}", flush=True)
            if rnd == "timed":
                res["batches"].append({"seed": s0, "G": est["G"], "s": est["s"], "iterations": it, "seconds": sec,
                                       "walk_seconds": info["walk"]["seconds"], "wall": wall})
            s0 = est["seed"]
    if not a.no_loop:
        tree = sample_tree.SampleSubtree(aircond, [], None, 1, bfs, seed, cfg, SOLVER)
        tree.run()
        scens = dict(tree.ef.scenarios())
        tree.close()
        walk = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stopped = None
        try:
            sample_tree.walking_tree_xhats(aircond, scens, xhat, bfs, seed + number_of_nodes(bfs), cfg, solver_name=SOLVER,
                                           info=walk, batched=False)
        except RuntimeError as err:                    # (a subtree short of its tolerance ends the walk there)
            stopped = str(err)
        torch.cuda.synchronize()
        loop = time.perf_counter() - t0
        # the walk meets the nodes scenario by scenario: group its iteration counts by the node's stage
        order = list(sample_tree.walk_seeds(scens, bfs, 0)[0])[:len(walk["iterations"])]
        by_stage = {}
        for nd, it in zip(order, walk["iterations"]):
            by_stage.setdefault(nd.count("_") + 1, []).append(it)
        worst = {t: max(v) for t, v in sorted(by_stage.items())}
        res["one_at_a_time"] = {"seconds": loop, "subtrees": len(order), "max_iterations_by_stage": worst,
                                "solve_seconds": float(np.sum(walk["seconds"])), "stopped": stopped}
        if stopped:
            print(f"one subtree at a time: the walk ended after {len(order)} subtrees: {stopped}", flush=True)
        print(f"one subtree at a time: {len(order)} extensive forms in {loop:.3f} s; largest iteration count per stage {worst} "
              f"(the stage's one conditioned solve: {res['batches'][0]['iterations']['conditioned'] if res['batches'] else 'none'})", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("farmer", "aircond"), default="farmer")
    ap.add_argument("--bf", default="4,3,2", help="aircond: the sample trees' branching factors")
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--xhat-scens", type=int, default=30)
    ap.add_argument("--ph-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-loop", action="store_true", help="skip the batch-by-batch baseline")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.model == "aircond":
        import torch
        assert torch.cuda.is_available(), "tools/mmw_ci.py needs the GPU"
        if a.batches == 32:
            a.batches = 3
        return aircond_interval(a)
    import numpy as np
    import torch
    from mpisppy_amd.confidence_intervals import ciutils
    from mpisppy_amd.confidence_intervals.mmw_ci import MMWConfidenceIntervals
    from mpisppy_amd.examples import farmer
    assert torch.cuda.is_available(), "tools/mmw_ci.py needs the GPU"
    res = {"batches": a.batches, "batch_size": a.batch_size}
    t0 = time.perf_counter()
    xhat, conv, tb = candidate(a)
    res["xhat"] = {"x": xhat.tolist(), "ph_conv": conv, "trivial_bound": tb, "seconds": time.perf_counter() - t0}
    print(f"xhat {xhat} from {a.ph_iters} PH iterations on {a.xhat_scens} scenarios (conv {conv:.2e})", flush=True)
    cfg = SimpleNamespace(EF_2stage=True, EF_solver_name=SOLVER, crops_multiplier=1, device="cuda:0")
    start = a.xhat_scens
    for rnd, nb in (("warm-up", min(2, a.batches)), ("timed", a.batches)):   # the first round loads the code objects
        info = {"time_phases": True}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mmw = MMWConfidenceIntervals(farmer, cfg, {"ROOT": xhat}, nb, batch_size=a.batch_size, start=start,
                                     verbose=False)
        r = mmw.run(info=info)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        print(f"[{rnd}] one launch: {wall:.3f} s; x* runs {info['seconds']['xstar']:.3f}, two solves "
              f"{info['seconds']['solves']:.4f}, moments pass and read {info['seconds']['moments']:.5f}; "
              f"{info['solves']} batched solves over {nb} batches; {len(info['xstar_certified_gaps'])} x* run(s) ended "
              f"on the certified gap {['%.1e' % g for g in info['xstar_certified_gaps']]}", flush=True)
    res["one_launch"] = {"seconds": wall, "phases": info["seconds"], "solves": info["solves"], "Gbar": r["Gbar"],
                         "xstar_certified_gaps": info["xstar_certified_gaps"],
                         "std": r["std"], "gap_inner_bound": r["gap_inner_bound"], "Glist": r["Glist"].tolist()}
    print(f"MMW: Gbar {r['Gbar']:.4f}, std {r['std']:.4f}, gap_inner_bound {r['gap_inner_bound']:.4f}", flush=True)
    if not a.no_loop:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        G, phases = [], {}
        for b in range(a.batches):
            info = {"time_phases": True}
            est = ciutils.gap_estimators({"ROOT": xhat}, farmer, scenario_names=farmer.scenario_names_creator(
                a.batch_size, start=start + b * a.batch_size), cfg=cfg, solver_name=SOLVER, info=info)
            G.append(est["G"])
            for k, v in info["seconds"].items():
                phases[k] = phases.get(k, 0.0) + v
        torch.cuda.synchronize()
        loop = time.perf_counter() - t0
        G = np.array(G)
        t = ciutils.t_ppf(0.95, a.batches - 1)
        inner = float(np.mean(G) + t * np.std(G) / np.sqrt(a.batches))
        res["per_batch_loop"] = {"seconds": loop, "phases": phases, "Gbar": float(np.mean(G)), "std": float(np.std(G)),
                                 "gap_inner_bound": inner, "max_abs_G_difference": float(np.abs(G - r["Glist"]).max())}
        print(f"batch by batch: {loop:.3f} s (x* runs {phases['xstar']:.3f}, solves {phases['solves']:.4f}, moments "
              f"{phases['moments']:.5f}); gap_inner_bound {inner:.4f}; max |G - G one launch| "
              f"{np.abs(G - r['Glist']).max():.3e}; one launch / loop = {wall / loop:.3f}", flush=True)
        rest = lambda ph: ph["solves"] + ph["moments"]  # noqa: E731
        print(f"without the x* runs: one launch {rest(res['one_launch']['phases']):.4f} s, loop {rest(phases):.4f} s",
              flush=True)
    res["device_passes"] = moments_next_to_expectations(a, xhat, start)
    d = res["device_passes"]
    print(f"per call on {a.batches * a.batch_size} scenarios: gap_moments {d['gap_moments_ms_per_call'][-1] * 1e3:.2f} us "
          f"({a.batches} segments, two launches), expectations {d['expectations_ms_per_call'][-1] * 1e3:.2f} us", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

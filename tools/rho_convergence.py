#!/usr/bin/env python
"""PH iterations and time to convergence with fixed rho and with the rho extensions.

Config 3 (farmer, 65,536 scenarios, cm = 1, rho = 1) from Iter0 to conv < convthresh:

  fixed        no extension (the speculative loop with the PH step folded into the solve);
               tests/golden/farmer_conv.json holds its break iterations (1,078 at 1e-3)
  updater      NormRhoUpdater with the reference's default options (the speculative loop
               with the rho update between Update_W and the solve)
  noop         an extension whose miditer does nothing on the host: the non-speculative
               loop, i.e. what any miditer extension cost before miditer_on_device
  updater-host NormRhoUpdater with the speculative solve turned off
  gradient     Gradient_extension: the cost-proportional rho (order_stat 0.5, scenario-
               dependent denominators), rewritten on the device when W_diff stalls; the
               speculative loop
  mult         MultRhoUpdater with the reference's default options: a host miditer, so the
               non-speculative loop

  fixer        Fixer with the same tuple on every nonant (--fixer-th, --fixer-nb; iter0 tuples
               without a lag): the counters, decisions and bound rewrite in one device pass
               between Update_W and the solve; the speculative loop.  Fixing trades optimality
               for speed: compare its E[obj] with the fixed mode's
  fixer-idle   the same with a threshold of 0, which never counts or fixes: what the pass costs
  noop-device  an extension whose miditer does nothing and is marked miditer_on_device: the
               speculative loop without the PH step folded into the solve, as under the Fixer

and, with --kernels, the HIP-event time of phgpu_ph_residuals and phgpu_norm_rho_update
next to phgpu_ph_update_ex on the same engine.  Prints one line per mode: PH iterations,
wall seconds of iterk_loop, mean ms per PH iteration, the final conv and rho range.

    python tools/rho_convergence.py [--scens 65536] [--convthresh 1e-3] [--limit 3000]
                                    [--modes fixed,updater,noop,updater-host,gradient,mult,fixer,fixer-idle,
                                             noop-device] [--kernels] [--fixer-th 10] [--fixer-nb 3]
                                    [--order-stat 0.5] [--indep-denom]
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


def make_ph(mode, S, thresh, limit, norm_rho_options, grad_options=None, fixer=(10.0, 3)):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.extensions.extension import Extension
    from mpisppy_amd.extensions.fixer import Fixer
    from mpisppy_amd.extensions.gradient_extension import Gradient_extension
    from mpisppy_amd.extensions.mult_rho_updater import MultRhoUpdater
    from mpisppy_amd.extensions.norm_rho_updater import NormRhoUpdater
    from mpisppy_amd.opt.ph import PH

    class NoopMiditer(Extension):
        def miditer(self):
            pass

    class NoopDevice(NoopMiditer):
        miditer_on_device = True

    ext = {"fixed": None, "updater": NormRhoUpdater, "noop": NoopMiditer, "updater-host": NormRhoUpdater,
           "gradient": Gradient_extension, "mult": MultRhoUpdater, "fixer": Fixer, "fixer-idle": Fixer,
           "noop-device": NoopDevice}[mode]
    th = [0.0 if mode == "fixer-idle" else float(fixer[0])] * 3
    fix_arrays = {"iter0": {"th": th}, "iterk": {"th": th, "nb": [int(fixer[1])] * 3}}
    opts = {"solver_name": "mi355x_pdhg", "PHIterLimit": limit, "defaultPHrho": 1.0, "convthresh": thresh,
            "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0",
            "batch_creator": farmer.batch_creator, "iterk_solver_options": dict(farmer.PDHG_ITERK_OPTIONS),
            "speculative_solve": mode != "updater-host", "norm_rho_options": dict(norm_rho_options),
            "gradient_extension_options": dict(grad_options or {"order_stat": 0.5}),
            "fixeroptions": {"verbose": False, "boundtol": 1e-2, "fix_arrays": fix_arrays}}
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator, extensions=ext,
              scenario_creator_kwargs={"crops_multiplier": 1, "num_scens": S})


def run_mode(mode, a, norm_rho_options):
    import torch
    ph = make_ph(mode, a.scens, a.convthresh, a.limit, norm_rho_options,
                 {"order_stat": a.order_stat, "indep_denom": a.indep_denom}, (a.fixer_th, a.fixer_nb))
    ph.PH_Prep()
    ph.Iter0()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ph.iterk_loop()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    e = ph.engine
    rho = e.rho[:e.nn]
    res = {"mode": mode, "scenarios": a.scens, "convthresh": a.convthresh, "converged": bool(ph.converged),
           "ph_iterations": int(ph._PHIter), "loop_seconds": dt, "ms_per_iteration": 1e3 * dt / max(1, ph._PHIter),
           "conv": float(ph.conv), "rho_min": float(rho.min()), "rho_max": float(rho.max()),
           "speculative": bool(ph._speculate(ph.extensions is not None)),
           "calls": {k: v for k, v in e.calls.items() if v}}
    if mode.startswith("fixer"):
        res["fixer_totals"] = list(e.fixer_totals_host())
        res["nonants_fixed"] = res["fixer_totals"][0] / a.scens
        if a.kernels:
            res["kernel_us"] = fixer_kernel_times(e, ph)
    if mode.startswith("updater") and e.calls["norm_rho_update"]:
        res["last_counts"] = e.norm_rho_counts().tolist()
    if mode == "gradient":
        res["rho_update_iterations"] = ph.extobject.rho_update_iterations()
    if mode == "mult":
        res["rho_update_iterations"] = list(ph.extobject.acted)
    if a.kernels and mode == "updater":
        res["kernel_us"] = kernel_times(e, ph)
    if a.kernels and mode == "gradient":
        res["kernel_us"] = grad_kernel_times(e, ph)
    res["Eobj"] = xbar_objective(ph)
    e.close()
    return res


def xbar_objective(ph):
    """E[f] with every nonant fixed at the final x̄ (W and prox off): what the run's answer is
    worth, comparable between the modes."""
    e = ph.engine
    e._flush_xbar()
    ph.disable_W_and_prox()
    e.fix_nonants(e.xbar.clone())
    e.solve(ph._to_phgpu_options(ph.current_solver_options), warm=True)
    obj = float(ph.Eobjective())
    e.fix_nonants(None)
    ph.reenable_W_and_prox()
    return obj


def kernel_times(e, ph, reps=200):
    """Mean HIP-event microseconds per call of the two new entries and of phgpu_ph_update_ex
    (x̄ scatter, W update, conv) on this engine's current state; rho and W are restored."""
    import torch
    from mpisppy_amd import _lib
    prm = ph.extobject._params(ph._PHIter)
    rho0, W0 = e.rho.clone(), e.W.clone()
    e.compute_xbar()
    e.residuals()
    e.xbar_snapshot()
    conv = torch.zeros(1, dtype=torch.float64, device=e.device)

    def upd():
        _lib.check(e.lib.phgpu_ph_update_ex(e.h, e.x.data_ptr(), e.node_buf.data_ptr(), e.xbar.data_ptr(),
                                            e.W.data_ptr(), e.rho.data_ptr(), 1, conv.data_ptr(), None, e._stream()),
                   "phgpu_ph_update_ex")

    out = {}
    for name, fn in (("phgpu_ph_residuals", e.residuals), ("phgpu_norm_rho_update", lambda: e.norm_rho_update(prm)),
                     ("phgpu_ph_update_ex", upd)):
        for _ in range(10):
            fn()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        ev[1].synchronize()
        out[name] = 1e3 * ev[0].elapsed_time(ev[1]) / reps
    e.rho.copy_(rho0)
    e.W.copy_(W0)
    return out


def fixer_kernel_times(e, ph, reps=200):
    """Mean HIP-event microseconds per engine.fixer_step (the nfix clear, the pass and the totals
    launch) with a threshold of 0, which changes nothing, next to phgpu_ph_update_ex."""
    import torch
    from mpisppy_amd import _lib
    none = e.fixer_arg([None] * e.nn, torch.int32)
    th = e.fixer_arg([0.0] * e.nn, torch.float64)
    prm = _lib.FixerParams(boundtol=1e-2, iter0=0)
    W0 = e.W.clone()
    conv = torch.zeros(1, dtype=torch.float64, device=e.device)
    e.compute_xbar()

    def upd():
        _lib.check(e.lib.phgpu_ph_update_ex(e.h, e.x.data_ptr(), e.node_buf.data_ptr(), e.xbar.data_ptr(),
                                            e.W.data_ptr(), e.rho.data_ptr(), 1, conv.data_ptr(), None, e._stream()),
                   "phgpu_ph_update_ex")

    out = {}
    for name, fn in (("fixer_step", lambda: e.fixer_step(prm, th, none, none, none)), ("phgpu_ph_update_ex", upd)):
        for _ in range(10):
            fn()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        ev[1].synchronize()
        out[name] = 1e3 * ev[0].elapsed_time(ev[1]) / reps
    e.W.copy_(W0)
    return out


def grad_kernel_times(e, ph, reps=200):
    """Mean HIP-event microseconds per call of engine.w_diff and engine.find_rho (the ratio pass,
    its final sum and the rule, gate closed so rho stays) on this engine's current state."""
    import torch
    cost = ph.extobject.grad_object.cost
    shut = torch.tensor([0.0, 1.0], dtype=torch.float64, device=e.device)
    out = {}
    for name, fn in (("w_diff", e.w_diff), ("find_rho", lambda: e.find_rho(cost, 0.5, gate=shut)),
                     ("grad_cost", lambda: e.grad_cost(e.xbar))):
        for _ in range(10):
            fn()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        ev[1].synchronize()
        out[name] = 1e3 * ev[0].elapsed_time(ev[1]) / reps
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scens", type=int, default=65536)
    p.add_argument("--convthresh", type=float, default=1e-3)
    p.add_argument("--limit", type=int, default=3000, help="PHIterLimit")
    p.add_argument("--modes", default="fixed,updater,noop,updater-host")
    p.add_argument("--kernels", action="store_true", help="time the new launches next to the update kernel")
    p.add_argument("--norm-rho-option", action="append", default=[], metavar="KEY=VALUE")
    p.add_argument("--order-stat", type=float, default=0.5, help="gradient mode: 0 the min, 0.5 the mean, 1 the max")
    p.add_argument("--indep-denom", action="store_true", help="gradient mode: the scenario-independent denominator")
    p.add_argument("--fixer-th", type=float, default=10.0, help="fixer mode: the threshold of every nonant")
    p.add_argument("--fixer-nb", type=int, default=3, help="fixer mode: the nb lag of every nonant")
    a = p.parse_args()
    nro = {}
    for kv in a.norm_rho_option:
        k, v = kv.split("=", 1)
        nro[k] = json.loads(v)
    gold = os.path.join(ROOT, "tests", "golden", "farmer_conv.json")
    if a.scens == 65536 and os.path.exists(gold):
        g = json.load(open(gold))
        known = g["breaks"].get(f"{a.convthresh:g}")
        if known:
            print(f"# fixed rho = {g['rho']:g}: the oracle breaks at PH iteration {known['iteration']} "
                  f"(tests/golden/farmer_conv.json)", flush=True)
    for mode in a.modes.split(","):
        r = run_mode(mode.strip(), a, nro)
        print(f"# {r['mode']:13s} {r['ph_iterations']:5d} PH iterations  {r['loop_seconds']:8.4f} s  "
              f"{r['ms_per_iteration']:.4f} ms / iteration  conv {r['conv']:.3e}  "
              f"rho [{r['rho_min']:g}, {r['rho_max']:g}]  converged {r['converged']}  E[obj] {r['Eobj']:.6f}", flush=True)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()

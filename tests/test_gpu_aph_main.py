"""APH end to end on the device (mpisppy_amd/opt/aph.py) against the trajectories of the numpy
restatement tests/aph_ref.py that tests/test_aph.py admits (tests/golden/aph_*.json):

* APH_main against every admitted fixture: W, z and x̄ at 1e-5 absolute; theta, conv, tau and phi
  at 1e-5 relative, phi and theta relative to the fixture's sum of |phi_s|; the dispatch lists
  exactly; the trivial bound and E[obj] at 1e-5 relative.  The solves run at the default options;
* the pins of the reference's own tests (mpisppy/tests/test_aph.py:230-280);
* two gloo ranks on one GPU against the one-rank result;
* a wheel with aph_hub, a Lagrangian spoke and an x̄ spoke that terminates on its gap;
* a maximisation model.
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

import aph_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REL = 1e-5
ABS = 1e-5
FARMER_EF_OBJ = -108390.0
AIR_KW = R.AIR_KW


def _recorder():
    from mpisppy_amd.extensions.extension import Extension

    class Recorder(Extension):
        """The state after every projective step (miditer) and every dispatch (enditer)."""

        def __init__(self, opt):
            super().__init__(opt)
            self.iters = []

        def miditer(self):
            o, e = self.opt, self.opt.engine
            h = o.aph_history[-1]
            self.iters.append({"tau": h["tau"], "phi": h["phi"], "theta": h["theta"], "conv": h["conv"],
                               "phisum": h["phisum"], "W": e.host("W")[:, :e.nn].copy(),
                               "z": e.host("aph_z")[:, :e.nn].copy(), "xbar": e.host("xbar")[:, :e.nn].copy()})

        def enditer(self):
            m = self.opt.engine.aph_mask.cpu().numpy()
            self.iters[-1]["dispatch"] = np.nonzero(m)[0].tolist()
            self.iters[-1]["scnt"] = self.opt.dispatch_counts[-1]
            lst = self.opt.engine.aph_list.cpu().numpy()
            if self.iters[-1]["scnt"] < self.opt.engine.S:
                assert lst[:self.iters[-1]["scnt"]].tolist() == self.iters[-1]["dispatch"]

    return Recorder


def _aph(cfg, mpicomm=None, sense=1, iters=None, start=0, **more):
    from mpisppy_amd.examples import aircond, farmer
    from mpisppy_amd.opt.aph import APH
    options = {"solver_name": "mi355x_pdhg", "PHIterLimit": cfg["iters"] if iters is None else iters,
               "defaultPHrho": cfg["rho"], "convthresh": 0.0, "verbose": False, "display_progress": False,
               "toc": False, "device": "cuda:0", "APHgamma": cfg.get("gamma", 1.0), "APHnu": cfg.get("nu", 1.0),
               "APHuse_lag": cfg.get("use_lag", False), "dispatch_frac": cfg.get("dispatch_frac", 1.0),
               "shelf_life": cfg.get("shelf_life", 99), "round_robin_dispatch": cfg.get("round_robin", False),
               "async_frac_needed": 1.0, "async_sleep_secs": 0.01}
    options.update(more)
    if cfg["model"] == "farmer":
        S = cfg["S"]
        return APH(options, farmer.scenario_names_creator(S, start=start), farmer.scenario_creator,
                   scenario_creator_kwargs={"num_scens": S, "sense": sense}, mpicomm=mpicomm,
                   extensions=_recorder())
    from oracle.models import create_nodenames_from_branching_factors
    bfs = list(cfg["bfs"])
    return APH(options, aircond.scenario_names_creator(int(np.prod(bfs))), aircond.scenario_creator,
               scenario_creator_kwargs={"branching_factors": bfs, **AIR_KW},
               all_nodenames=create_nodenames_from_branching_factors(bfs), mpicomm=mpicomm, extensions=_recorder())


def _compare(iters, fx, lo=0, hi=None, offset=0, with_conv=True, with_phisum=True):
    sl = slice(lo, hi)
    for it, (o, g) in enumerate(zip(iters, fx["iters"])):
        dW, dz, dx = (float(np.abs(o[k] - np.array(g[k])[sl]).max()) for k in ("W", "z", "xbar"))
        print(f"iteration {it + 1}: theta {o['theta']:.9f} ({g['theta']:.9f}) conv {o['conv']} ({g['conv']}) "
              f"tau {o['tau']:.6e} phi {o['phi']:.6e} ({g['phi']:.6e}) max|W - ref| {dW:.2e} max|z - ref| {dz:.2e} "
              f"max|xbar - ref| {dx:.2e}")
        assert dW <= ABS and dz <= ABS and dx <= ABS, it
        # phi before the step and theta = phi nu / tau relative to the fixture's sum of |phi_s| (at
        # the first pass W = y = 0: every phi_s and theta are exactly 0); the post-step sum likewise
        nu = fx["config"].get("nu", 1.0)
        assert abs(o["tau"] - g["tau"]) <= REL * abs(g["tau"]), it
        assert abs(o["phi"] - g["phi"]) <= REL * g["abs_phi_pre"], it
        assert abs(o["theta"] - g["theta"]) <= REL * nu * g["abs_phi_pre"] / g["tau"], it
        if with_phisum:
            assert abs(o["phisum"] - g["phisum"]) <= REL * g["abs_phi"], it
        if not with_conv:
            pass
        elif g["conv"] is None:
            assert o["conv"] is None
        else:
            assert abs(o["conv"] - g["conv"]) <= REL * abs(g["conv"]), it
        want = [s - offset for s in g["dispatch"] if lo <= s < (hi if hi is not None else 10 ** 9)]
        if "dispatch" in o and offset == 0 and hi is None:
            assert o["dispatch"] == want, (it, o["dispatch"], want)


@pytest.mark.parametrize("name", sorted(R.TRAJECTORIES))
def test_aph_matches_the_recorded_trajectory(gpu, name):
    fx = json.load(open(os.path.join(HERE, "golden", f"aph_{name}.json")))
    cfg = R.TRAJECTORIES[name]
    opt = _aph(cfg)
    try:
        conv, eobj, tb = opt.APH_main()
        rec = opt.extobject
        assert len(rec.iters) == cfg["iters"]
        assert abs(tb - fx["trivial"]) <= REL * abs(fx["trivial"])
        _compare(rec.iters, fx)
        assert abs(conv - fx["conv"]) <= REL * abs(fx["conv"])
        print(f"E[obj] {eobj:.6f} ({fx['eobj']:.6f})")
        assert abs(eobj - fx["eobj"]) <= REL * abs(fx["eobj"])
        c = opt.engine.calls
        S, frac = opt.engine.S, cfg.get("dispatch_frac", 1.0)
        partial = cfg["iters"] - 1 if R.scnt_of(S, frac) < S else 0
        assert rec.iters[0]["scnt"] == S                       # the first pass dispatches everything
        assert c["solve_list"] == c["select_smallest"] == partial
        # one read per iteration, nothing per scenario
        assert c["aph_scalars_read"] == c["aph_update"] == c["aph_reduce"] == c["aph_norms"] == cfg["iters"]
    finally:
        opt.engine.close()


def test_the_reference_tests_pins(gpu):
    """Farmer scenarios 1 .. 30, PHIterLimit 2, rho 1 (mpisppy/tests/test_aph.py:230-280): trivial bound 137846;
    E[obj] 134796 at full dispatch and 134680 at dispatch_frac 0.25, to three significant digits."""
    def sig3(v):
        return float(f"{v:.3g}")
    for frac, target in ((1.0, 134796.0), (0.25, 134680.0)):
        opt = _aph(dict(model="farmer", S=30, rho=1.0, iters=2, dispatch_frac=frac), start=1)
        try:
            conv, eobj, tb = opt.APH_main()
            print(f"dispatch_frac {frac}: trivial bound {-tb:.2f}, E[obj] {-eobj:.2f}")
            assert sig3(-tb) == sig3(137846.0)
            assert sig3(-eobj) == sig3(target)
        finally:
            opt.engine.close()


def test_a_maximisation_model(gpu):
    fx = json.load(open(os.path.join(HERE, "golden", "aph_farmer30_quarter.json")))
    cfg = R.TRAJECTORIES["farmer30_quarter"]
    opt = _aph(cfg, sense=-1)
    try:
        conv, eobj, tb = opt.APH_main()
        assert not opt.is_minimizing
        assert abs(tb + fx["trivial"]) <= REL * abs(fx["trivial"])
        assert abs(eobj + fx["eobj"]) <= REL * abs(fx["eobj"])
        _compare(opt.extobject.iters, fx)                       # the device problem is the minimisation
    finally:
        opt.engine.close()


# ------------------------------------------------------------------ two gloo ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(HERE)
    for p in (HERE, os.path.join(root, "mpi-sppy-1_amd"), root):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mpisppy_amd.comm import Comm
        opt = _aph(R.TRAJECTORIES["farmer30_full"], mpicomm=Comm())
        conv, eobj, tb = opt.APH_main()
        got = {"conv": conv, "eobj": eobj, "trivial": tb, "names": list(opt.local_scenario_names), "iters": []}
        for o in opt.extobject.iters:
            got["iters"].append({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in o.items()})
        opt.engine.close()
        with open(os.path.join(out_dir, f"aph_r{rank}.json"), "w") as f:
            json.dump(got, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_give_the_one_rank_trajectory(gpu, tmp_path):
    """Full dispatch (the dispatch count is per rank, so a partial dispatch of two ranks is
    another algorithm than one rank's): both reductions over the ranks.  W, z, x̄, tau, phi, theta,
    the trivial bound and E[obj] are the one-rank trajectory's."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    fx = json.load(open(os.path.join(HERE, "golden", "aph_farmer30_full.json")))
    lo = 0
    local_phisums = []
    for k in range(2):
        r = json.load(open(tmp_path / f"aph_r{k}.json"))
        n = len(r["names"])
        assert n == 15
        for o in r["iters"]:
            for key in ("W", "z", "xbar"):
                o[key] = np.array(o[key])
        # (conv is left out: with several ranks the other ranks' W and z norms reach a rank one
        # iteration late, through the next second reduction, as in the reference, aph.py:491-496)
        _compare(r["iters"], fx, lo, lo + n, offset=lo, with_conv=False, with_phisum=False)
        local_phisums.append([o["phisum"] for o in r["iters"]])
        assert abs(r["eobj"] - fx["eobj"]) <= REL * abs(fx["eobj"])
        assert abs(r["trivial"] - fx["trivial"]) <= REL * abs(fx["trivial"])
        lo += n
    for a, b, g in zip(*local_phisums, fx["iters"]):             # the post-step phi sum is per rank
        assert abs(a + b - g["phisum"]) <= REL * g["abs_phi"]


# ------------------------------------------------------------------ a wheel
def test_wheel_with_the_aph_hub(gpu):
    """aph_hub + lagrangian_spoke + xhatxbar_spoke on farmer 3 scenarios: the wheel stops on its
    gap, and outer <= EF optimum <= inner at termination."""
    from types import SimpleNamespace
    from mpisppy_amd.cylinders.hub import APHHub
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.opt.aph import APH
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    names = farmer.scenario_names_creator(3)
    cfg = SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=200, rel_gap=1e-3,
                          intra_hub_conv_thresh=-1.0, device="cuda:0", toc=False, aph_gamma=1.0, aph_nu=1.0,
                          aph_frac_needed=1.0, aph_dispatch_frac=0.67, aph_sleep_seconds=0.01)
    kw = {"num_scens": 3}
    hub = vanilla.aph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
    spokes = [vanilla.lagrangian_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw),
              vanilla.xhatxbar_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)]
    ws = WheelSpinner(hub, spokes)
    ws.spin(placement="colocated")
    h = ws.spcomm
    try:
        assert isinstance(h, APHHub) and isinstance(h.opt, APH)
        assert h.opt._PHIter < 200                                   # stopped on the gap, not on the limit
        assert h.opt.dispatch_counts[0] == 3 and set(h.opt.dispatch_counts[1:]) == {2}
        gap = (ws.BestInnerBound - ws.BestOuterBound) / abs(ws.BestOuterBound)
        print(f"stopped at iteration {h.opt._PHIter}: outer {ws.BestOuterBound:.4f} inner {ws.BestInnerBound:.4f} "
              f"gap {gap:.2e}")
        assert gap <= 1e-3
        assert ws.BestOuterBound <= FARMER_EF_OBJ + REL * abs(FARMER_EF_OBJ)
        assert ws.BestInnerBound >= FARMER_EF_OBJ - REL * abs(FARMER_EF_OBJ)
    finally:
        for s in ws.spokes:
            s.opt.engine.close()
        h.opt.engine.close()

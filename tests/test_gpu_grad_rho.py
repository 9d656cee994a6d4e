"""The gradient-rho entries on the device (phgpu_grad_cost, phgpu_w_diff, phgpu_rho_ratio_stats,
phgpu_rho_from_stats; include/phgpu.h) and the classes on top of them against the numpy
restatement in tests/grad_rho_ref.py, fed the device's own inputs.

Tolerances: sums 1e-12 relative (at most 1,000 positive fp64 terms: S eps ~ 2e-13); the
minimum / maximum planes, ``applied`` and a rho the closed gate left alone bitwise; the
gradient cost bitwise (two roundings, as numpy's c + q * x).  PH against the stepped oracle:
W and x̄ at the project's 1e-5 up to the first rewrite; rho at a rewrite (i) 1e-12 against the
restatement fed the GPU's own x, x̄ and cost and (ii) against the oracle's rho within
grad_rho_ref.perturbation_tolerance (twice the effect of moving the oracle's x by 1e-5).
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

import grad_rho_ref as G
import norm_rho_ref as N

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "rho_test_data")
ABS = 1e-5
SUM_REL = 1e-12
ALPHAS = (0.0, 0.4, 0.5, 0.9, 1.0)
QP_S, QP_N, QP_NONANTS = 130, 12, [7, 2, 9, 4, 11]


# ------------------------------------------------------------------ the shapes
def qp_batch_creator(names, **kw):
    """A random two-stage QP batch: n = 12 columns in [-10, 10], 4 loose rows, q > 0 on every
    column, c different in every scenario; 5 nonants whose columns are neither first nor
    contiguous.  A scenario's data depend on its name only (ranks build their own slices)."""
    from mpisppy_amd.batch import ScenarioBatch
    idx = np.array([int(nm[4:]) for nm in names])
    rng = np.random.default_rng(17)
    n, m, S = QP_N, 4, QP_S
    cols = [np.sort(rng.choice(n, 5, replace=False)) for _ in range(m)]
    row_ptr = np.arange(0, 5 * m + 1, 5, dtype=np.int32)
    col_idx = np.concatenate(cols).astype(np.int32)
    A = rng.normal(0.0, 1.0, (S, 5 * m))
    c = rng.normal(0.0, 20.0, (S, n))
    q = rng.uniform(0.5, 4.0, (S, n))
    ru = np.full((S, m), 50.0)
    nn = len(QP_NONANTS)
    return ScenarioBatch([f"scen{i}" for i in idx], row_ptr, col_idx, A[idx], c[idx], np.full((len(idx), n), -10.0),
                         np.full((len(idx), n), 10.0), np.full((len(idx), m), -np.inf), ru[idx], q[idx],
                         np.zeros(len(idx)), np.array(QP_NONANTS, np.int32), np.zeros(nn, np.int32),
                         np.arange(nn, dtype=np.int32), np.zeros((len(idx), 1), np.int32), ["ROOT"],
                         np.full(len(idx), 1.0 / S), np.full((len(idx), 1), 1.0 / S),
                         nonant_names=[f"x[{j}]" for j in QP_NONANTS])


def _engine(shape):
    from mpisppy_amd.engine import PHEngine
    if shape.startswith("farmer"):
        from mpisppy_amd.examples import farmer
        S = int(shape[6:])
        b = farmer.batch_creator(farmer.scenario_names_creator(S), crops_multiplier=1, num_scens=S)
    elif shape == "qp":
        b = qp_batch_creator([f"scen{i}" for i in range(QP_S)])
    elif shape == "uc":                        # the smallest shared-matrix batch of tests/test_gpu_uc.py
        from mpisppy_amd.examples import uc
        gold = json.load(open(os.path.join(HERE, "golden", "uc.json")))
        b = uc.batch_creator(gold["names"], num_scens=gold["num_scens"])
    elif shape == "aircond432":
        from mpisppy_amd.examples import aircond
        b = aircond.batch_creator(aircond.scenario_names_creator(24), branching_factors=N.AIR_BF, **N.AIR_KW)
    e = PHEngine(b, device="cuda:0")
    assert e.shared == (shape == "uc")
    return e


def _dev(e, a):
    """host [S, nn] -> device [nn, S]."""
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T), device=e.device)


def _random_state(e, seed):
    rng = np.random.default_rng(seed)
    e.x.copy_(torch.as_tensor(rng.normal(0.0, 50.0, (e.n, e.S)), device=e.device))
    e.set_xbar(rng.normal(0.0, 50.0, (e.S, e.nn)))
    e.set_rho(rng.uniform(0.1, 10.0, (e.S, e.nn)))
    return rng


def _host_state(e):
    b = e.batch
    x = e.x.cpu().numpy()[np.asarray(b.nonant_col)].T
    xbar = e.xbar.cpu().numpy()[:e.nn].T
    pcoef = np.tile(e.prob_coeff.cpu().numpy().reshape(-1, e.S)[0][:, None], (1, e.nn))
    return x, xbar, pcoef


def _assert_planes(got, ref, what):
    print(what, "sum plane max abs err / max", np.abs(got[0] - ref[0]).max() / max(np.abs(ref[0]).max(), 1e-300))
    np.testing.assert_allclose(got[0], ref[0], rtol=SUM_REL, atol=0, err_msg=what)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), what


SHAPES = ["farmer3", "farmer65", "farmer193", "farmer1000", "qp", "uc"]


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_against_the_restatement(gpu, shape):
    e = _engine(shape)
    b, nn, S = e.batch, e.nn, e.S
    nc = np.asarray(b.nonant_col)
    ws0 = e.workspace_bytes()
    rng = _random_state(e, 23)
    # -- phgpu_grad_cost against c + q x in numpy
    xn = rng.normal(0.0, 30.0, (S, nn))
    cost_dev = e.grad_cost(_dev(e, xn))
    cost = cost_dev.cpu().numpy()[:nn].T.copy()
    assert np.array_equal(cost, G.grad_cost(b.c[:, nc], b.q[:, nc], xn))
    if shape == "qp":
        assert (b.q[:, nc] > 0).all() and np.ptp(b.c[:, nc], axis=0).min() > 1.0
    # -- phgpu_w_diff: 0 at the first call, then the mean |W - W_prev|; W_prev follows W
    W0, W1 = rng.normal(0.0, 40.0, (S, nn)), rng.normal(0.0, 40.0, (S, nn))
    e.set_W(W0)
    e.w_diff()
    assert e.w_diff_value() == 0.0 and torch.equal(e._W_prev, e.W)
    e.set_W(W1)
    gate = e.w_diff()
    want = G.w_diff(W1, W0)
    got = e.w_diff_value()
    print("w_diff", got, want, abs(got / want - 1))
    assert abs(got - want) <= SUM_REL * want and torch.equal(e._W_prev, e.W)
    assert gate.cpu().tolist() == [0.0, got]
    e._W_prev.copy_(_dev(e, W0))
    e.w_diff()
    assert e.w_diff_value() == got                                # the same bits on every run
    assert e.w_diff_history().tolist() == [0.0, got, got]
    # -- phgpu_rho_ratio_stats / phgpu_rho_from_stats, both denominators
    x, xbar, pcoef = _host_state(e)
    for indep in (False, True):
        p = e.rho_ratio_stats(cost_dev, indep, 1e3).reshape(3, -1).cpu().numpy()[:, :nn]
        gden = None
        if indep:
            gden = e.gden.cpu().numpy()[:nn]
            np.testing.assert_allclose(gden, G.grad_denom(x, xbar, pcoef), rtol=SUM_REL, atol=0)
        ref = G.planes(G.ratios(cost, x, xbar, gden))
        _assert_planes(p, ref, f"{shape} indep={indep}")
        again = e.rho_ratio_stats(cost_dev, indep, 1e3).reshape(3, -1).cpu().numpy()[:, :nn]
        assert np.array_equal(p, again)
        for alpha in ALPHAS:
            e.rho.fill_(-7.0)
            e.find_rho(cost_dev, alpha, indep, 1e3)
            rho = e.rho.cpu().numpy()[:nn]
            assert (rho == rho[:, :1]).all() and int(e.rho_applied.item()) == 1
            np.testing.assert_allclose(rho[:, 0], G.compute_rho(cost, x, xbar, alpha, gden), rtol=1e-12, atol=0)
    # workspace of their own, allocated at the first calls: the block sums and the counter of
    # w_diff, the per-wave partials of the ratios and of the residuals (the independent mode)
    waves = (S + 63) // 64
    assert e.workspace_bytes() == ws0 + 256 * 8 + 4 + waves * nn * (3 * 8 + 4) + waves * nn * (4 * 8 + 4)
    e.close()


def test_a_scenario_at_xbar_gives_an_infinite_maximum(gpu):
    e = _engine("farmer65")
    _random_state(e, 5)
    s0 = 17
    nc = torch.as_tensor(np.asarray(e.batch.nonant_col), dtype=torch.long, device=e.device)
    e.x[nc, s0] = e.xbar[:e.nn, s0]                     # this scenario's denominator is exactly 0
    cost_dev = e.grad_cost(e.xbar)
    cost = cost_dev.cpu().numpy()[:e.nn].T
    assert (cost != 0).all()                            # farmer's cost is the planting cost: no 0 / 0
    x, xbar, _ = _host_state(e)
    p = e.rho_ratio_stats(cost_dev).reshape(3, -1).cpu().numpy()
    ref = G.planes(G.ratios(cost, x, xbar))
    assert np.isposinf(ref[0]).all() and np.isposinf(ref[2]).all() and np.isfinite(ref[1]).all()
    assert np.array_equal(p, ref)
    e.close()


def test_gate_on_the_device(gpu):
    """prev = 0 (inf), NaN, and ratios 0.049 / 0.051 on either side of thr = 0.05."""
    e = _engine("farmer193")
    rng = _random_state(e, 9)
    cost_dev = e.grad_cost(e.xbar)
    x, xbar, _ = _host_state(e)
    want = G.compute_rho(cost_dev.cpu().numpy()[:e.nn].T, x, xbar, 0.5)
    rho0 = rng.uniform(0.1, 10.0, (e.S, e.nn))
    nan = float("nan")
    for prev, cur in ((0.0, 1.0), (0.0, 0.0), (nan, 1.0), (1.0, nan), (1.0, 0.951), (1.0, 0.949), (1.0, 1.049),
                      (1.0, 1.051), (float("inf"), 1.0)):
        opened = G.gate_open(prev, cur, 0.05)
        assert opened == (abs(cur - 1.0) < 0.05 and prev == 1.0)
        e.set_rho(rho0)
        before = e.rho.clone()
        g = torch.tensor([prev, cur], dtype=torch.float64, device=e.device)
        flag = torch.full((1,), 5, dtype=torch.int32, device=e.device)
        e.find_rho(cost_dev, 0.5, gate=g, thr=0.05, applied=flag)
        assert int(flag.item()) == int(opened), (prev, cur)
        if opened:
            np.testing.assert_allclose(e.rho.cpu().numpy()[:e.nn, 0], want, rtol=1e-12, atol=0)
        else:
            assert torch.equal(e.rho, before), (prev, cur)
    e.close()


def test_multistage_handle_is_refused(gpu):
    from mpisppy_amd import _lib
    e = _engine("aircond432")
    _random_state(e, 3)
    before = e.rho.clone()
    half = e.num_nodes * e.nlen_max
    planes = torch.full((3 * half,), 7.0, dtype=torch.float64, device=e.device)
    cost = torch.ones_like(e.W)
    rc = e.lib.phgpu_rho_ratio_stats(e.h, cost.data_ptr(), e.x.data_ptr(), e.xbar.data_ptr(), None,
                                     planes.data_ptr(), None)
    assert rc == -3 and "two-stage" in _lib.last_error()
    rc = e.lib.phgpu_rho_from_stats(e.h, planes.data_ptr(), e.S, 0.5, None, 0.05, e.rho.data_ptr(), None, None)
    assert rc == -3 and "two-stage" in _lib.last_error()
    with pytest.raises(_lib.PhgpuError):
        e.find_rho(cost, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(e.rho, before) and (planes == 7.0).all()           # nothing launched
    # the cost and the dual metric do not depend on the tree
    e.grad_cost(e.xbar)
    e.w_diff()
    assert e.w_diff_value() == 0.0
    e.close()


# ------------------------------------------------------------------ the classes
def _ph(case, iters, thresh=-1.0, ext="gradient", spec=True, mpicomm=None, alpha=None, **extra):
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.extensions.gradient_extension import Gradient_extension
    from mpisppy_amd.extensions.mult_rho_updater import MultRhoUpdater
    from mpisppy_amd.opt.ph import PH
    S = int(case[6:])
    opts = {"solver_name": "mi355x_pdhg", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": thresh,
            "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0",
            "speculative_solve": spec, "fused_ph_loop": False, "batch_creator": farmer.batch_creator,
            "gradient_extension_options": {"order_stat": G.CASES[case]["alpha"] if alpha is None else alpha}}
    opts.update(extra)
    ext = {"gradient": Gradient_extension, "mult": MultRhoUpdater, None: None}.get(ext, ext)
    return PH(opts, farmer.scenario_names_creator(S), farmer.scenario_creator, extensions=ext, mpicomm=mpicomm,
              scenario_creator_kwargs={"crops_multiplier": 1, "num_scens": S})


def test_find_rho_on_farmer3_gives_the_reference_fixture(gpu, tmp_path):
    """The engine on farmer 3 after Iter0 and Compute_Xbar with the reference's cost file:
    rho.csv and the pinned 0.0523..., and the restatement fed the GPU's own x."""
    from mpisppy_amd.utils import find_rho, gradient
    ph = _ph("farmer3", 0, ext=None)
    ph.ph_main(finalize=False)
    e = ph.engine
    cfg = {"whatpath": os.path.join(DATA, "grad_cost.csv"), "order_stat": 0.4, "rho_file": str(tmp_path / "rho.csv")}
    fr = find_rho.Find_Rho(ph, cfg)
    x0 = e.nonant_x()
    assert fr._w_denom(0)[0] == pytest.approx(25.0, rel=1e-9)              # x̄ = 0 still
    assert fr._prox_denom(0)[0] == pytest.approx(1250.0, rel=1e-9)
    assert fr._grad_denom()[0] == pytest.approx(21.48148148148148, rel=1e-9)
    indep = fr.compute_rho(indep_denom=True)
    dep = fr.compute_rho()
    want = G.read_rho_csv(os.path.join(DATA, "rho.csv"))
    print("indep", indep, "dep", dep)
    for v, r in want.items():
        assert indep[v] == pytest.approx(r, rel=1e-9)
    assert dep["DevotedAcreage[CORN0]"] == pytest.approx(0.05230103406621424, rel=1e-9)
    x, xbar, pcoef = _host_state(e)
    assert np.array_equal(x, x0)
    cost = np.tile([-150.0, -230.0, -260.0], (3, 1))
    np.testing.assert_allclose(list(indep.values()), G.compute_rho(cost, x, xbar, 0.4, G.grad_denom(x, xbar, pcoef)),
                               rtol=1e-12)
    np.testing.assert_allclose(list(dep.values()), G.compute_rho(cost, x, xbar, 0.4), rtol=1e-12)
    fr.write_rho()
    assert find_rho.read_rho_file(cfg["rho_file"]) == dep
    # Find_Grad: the true planting costs, at the fixture's xhat (the farmer's cost is constant)
    fg = gradient.Find_Grad(ph, {"xhatpath": os.path.join(DATA, "farmer_cyl_nonants.npy"), "order_stat": 0.4,
                                 "grad_cost_file": str(tmp_path / "cost.csv"),
                                 "grad_rho_file": str(tmp_path / "grho.csv")})
    fg.write_grad_cost()
    assert fg.c[("scen0", "DevotedAcreage[CORN0]")] == -230.0
    assert [fg.c[("scen2", v)] for v in want] == G.FARMER_COST.tolist()
    assert find_rho.read_cost_file(str(tmp_path / "cost.csv")) == fg.c
    fg.write_grad_rho()
    np.testing.assert_allclose(list(find_rho.read_rho_file(str(tmp_path / "grho.csv")).values()),
                               G.compute_rho(np.tile(G.FARMER_COST, (3, 1)), x, xbar, 0.4), rtol=1e-12)
    e.close()


def test_grad_cost_needs_no_solve_on_the_qp_batch(gpu):
    """The cost at xhat equals the cost taken at the x of an Xhat_Eval solve with the nonants
    fixed at xhat: the reference's fix / solve / unfix only moves the evaluation point."""
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    names = [f"scen{i}" for i in range(QP_S)]
    opts = {"solver_name": "mi355x_pdhg", "verbose": False, "toc": False, "device": "cuda:0",
            "batch_creator": qp_batch_creator}
    xe = Xhat_Eval(opts, names, None)
    xhat = np.random.default_rng(2).uniform(-8.0, 8.0, len(QP_NONANTS))
    assert xe.evaluate({"ROOT": xhat}) is not None
    e = xe.engine
    b = e.batch
    nc = np.asarray(b.nonant_col)
    x = e.nonant_x()
    assert np.abs(x - xhat).max() <= 1e-9                      # the solve kept the nonants at xhat
    got = e.grad_cost(torch.as_tensor(xhat, device=e.device)[:, None].expand(e.nn, e.S)).cpu().numpy().T
    at_solved_x = G.grad_cost(b.c[:, nc], b.q[:, nc], x)
    print("max |cost(xhat) - cost(x of the fixed solve)|", np.abs(got - at_solved_x).max())
    np.testing.assert_allclose(got, at_solved_x, rtol=0, atol=4.0 * 1e-9 * 2)      # q <= 4, |x - xhat| <= 1e-9
    e.close()


def _recording(base):
    """The extension with a host miditer that records what its rule read and wrote."""
    class Recording(base):
        def __init__(self, ph):
            super().__init__(ph)
            self.miditer_on_device = False
            self.rec = []

        def miditer(self):
            e = self.opt.engine
            e._flush_xbar()
            r = {"iter": self.opt._PHIter, "conv": self.opt.conv, "x": e.nonant_x(),
                 "xbar": e.host("xbar")[:, :e.nn].copy(), "W": e.host("W")[:, :e.nn].copy()}
            super().miditer()
            r["rho"] = e.host("rho")[:, :e.nn].copy()
            if hasattr(self, "_applied"):
                r["applied"] = bool(self._applied[r["iter"]].item())
                r["cost"] = self.grad_object.cost.cpu().numpy()[:e.nn].T.copy()
            self.rec.append(r)
    return Recording


@pytest.mark.parametrize("case", ["farmer3", "farmer1000"])
def test_ph_with_gradient_extension_matches_the_stepped_restatement(gpu, case):
    from mpisppy_amd.extensions.gradient_extension import Gradient_extension
    c = G.CASES[case]
    g = G.trajectory(case)
    ph = _ph(case, c["iters"], c["thresh"], ext=_recording(Gradient_extension))
    conv, _, tb = ph.ph_main(finalize=False)
    ext = ph.extobject
    oracle = {r["iter"]: r for r in g.log}
    wd = ph.engine.w_diff_history()
    ratios = [float(G.gate_ratio(a, b)) for a, b in zip(wd[:-1], wd[1:])]
    print(case, "rewrites", ext.rho_update_iterations(), "last iteration", ph._PHIter, "conv", conv)
    print("gate ratios", ["%.4f" % r for r in ratios])
    assert set(ext.rho_update_iterations()) == c["applied"] == {r["iter"] for r in ext.rec if r["applied"]}
    assert abs(tb - g.trivial_bound) <= 1e-5 * abs(g.trivial_bound)
    first = min(c["applied"])
    for r in ext.rec:
        o = oracle[r["iter"]]
        if r["iter"] <= first:
            assert np.abs(r["xbar"] - o["xbar"]).max() <= ABS and np.abs(r["W"] - o["W"]).max() <= ABS, r["iter"]
            assert abs(r["conv"] - o["conv"]) <= ABS
        if r["iter"] < first:                 # W_diff == conv while rho = 1
            assert wd[r["iter"]] == pytest.approx(r["conv"], rel=1e-9)
        if not r["applied"]:
            continue
        assert np.array_equal(r["cost"], np.tile(G.FARMER_COST, (r["cost"].shape[0], 1)))
        assert (r["rho"] == r["rho"][:1]).all()
        own = G.compute_rho(r["cost"], r["x"], r["xbar"], c["alpha"])
        np.testing.assert_allclose(r["rho"][0], own, rtol=1e-12, atol=0)                          # (i)
        tol = G.perturbation_tolerance(o, G.FARMER_COST, c["alpha"])
        err = np.abs(r["rho"][0] / o["rho"][0] - 1).max()
        print(case, "rewrite at", r["iter"], "rho", r["rho"][0], "oracle", o["rho"][0], "rel err", err, "tol", tol)
        assert err <= tol                                                                          # (ii)
    if case == "farmer1000":
        assert ph.converged and conv < 1e-3 and abs(ph._PHIter - 22) <= 1, (ph._PHIter, conv)
    ph.engine.close()


def _state(ph):
    e = ph.engine
    return {"rho": e.host("rho")[:, :e.nn].copy(), "W": ph.W_array().copy(), "xbar": e.host("xbar")[:, :e.nn].copy(),
            "conv": ph.conv, "iter": ph._PHIter, "calls": dict(e.calls), "wd": e.w_diff_history().copy(),
            "applied": ph.extobject.rho_update_iterations()}


def test_speculative_solve_stays_on_and_invisible_with_the_extension(gpu):
    case, iters = "farmer3", G.CASES["farmer3"]["iters"]
    out = {}
    for spec in (True, False):
        ph = _ph(case, iters, spec=spec)
        ph.ph_main(finalize=False)
        assert ph._speculate(True) == spec and ph._miditer_early(True) and ph.extobject.miditer_on_device
        out[spec] = _state(ph)
        ph.engine.close()
    a, b = out[True], out[False]
    assert a["iter"] == b["iter"] == iters and a["conv"] == b["conv"], (a["conv"], b["conv"])
    for k in ("rho", "W", "xbar", "wd"):
        assert np.array_equal(a[k], b[k]), (k, np.abs(a[k] - b[k]).max())
    assert set(a["applied"]) == set(b["applied"]) == G.CASES[case]["applied"]
    # speculative solves ran, no step was deferred into a solve launch, and every miditer
    # enqueued the metric and the rule
    assert a["calls"]["solve_deferred"] == iters and b["calls"]["solve_deferred"] == 0
    assert a["calls"]["ph_step_defer"] == 0 and b["calls"]["ph_step_defer"] == 0
    for c in (a["calls"], b["calls"]):
        assert c["w_diff"] == iters + 1 and c["rho_from_stats"] == iters and c["grad_cost"] == 1, c


def test_verbose_takes_the_plain_loop(gpu, capsys):
    iters = G.CASES["farmer3"]["iters"]
    ph = _ph("farmer3", iters, gradient_extension_options={"order_stat": 0.4, "verbose": True})
    ph.ph_main(finalize=False)
    assert not ph._speculate(True) and ph.engine.calls["solve_deferred"] == 0
    assert set(ph.extobject.rho_update_iterations()) == G.CASES["farmer3"]["applied"]
    out = capsys.readouterr().out
    assert out.count("scen0 rho values: ") == 1 + len(G.CASES["farmer3"]["applied"])    # post_iter0 and the rewrites
    ph.engine.close()


def test_a_plain_ph_loop_launches_nothing_new(gpu):
    ph = _ph("farmer3", 3, ext=None)
    ph.ph_main(finalize=False)
    c = ph.engine.calls
    assert c["grad_cost"] == c["w_diff"] == c["rho_ratio_stats"] == c["rho_from_stats"] == 0 and c["ph_step_defer"] == 3
    ph.engine.close()


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tracing(base):
    """The extension keeping, per miditer, device copies of what its rule reads (x, x̄) and of W:
    no read back, so miditer stays on the device and the loop speculative."""
    class Tracing(base):
        def __init__(self, ph):
            super().__init__(ph)
            self.trace = {}

        def miditer(self):
            e = self.opt.engine
            e._flush_xbar()
            self.trace[self.opt._PHIter] = (e.nonant_x_dev().clone(), e.xbar[:e.nn].clone(), e.W[:e.nn].clone())
            super().miditer()

        def host_trace(self):
            return {it: [v.T.cpu().numpy() for v in tr] for it, tr in self.trace.items()}
    return Tracing


def _traced_run(case, mpicomm=None):
    from mpisppy_amd.extensions.gradient_extension import Gradient_extension
    ph = _ph(case, G.CASES[case]["iters"], ext=_tracing(Gradient_extension), mpicomm=mpicomm)
    ph.ph_main(finalize=False)
    s = _state(ph)
    s["trace"] = ph.extobject.host_trace()
    s["names"], s["spec"] = list(ph.local_scenario_names), bool(ph._speculate(True))
    ph.engine.close()
    return s


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
        res = {}
        for case in ("farmer3", "farmer193"):
            s = _traced_run(case, mpicomm=Comm())
            res[case] = {"rho": s["rho"].tolist(), "wd": s["wd"].tolist(), "applied": s["applied"],
                         "names": s["names"], "spec": s["spec"], "calls": s["calls"],
                         "trace": {str(it): [v.tolist() for v in tr] for it, tr in s["trace"].items()}}
        with open(os.path.join(out_dir, f"gr_r{rank}.json"), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


def _scenario_denom(x, xbar):
    """Every scenario's denominator of find_rho.py:189, [S]."""
    return np.maximum(G.w_denom(x, xbar), G.prox_denom(x, xbar)).max(axis=1)


@pytest.mark.timeout(300)
def test_two_ranks_match_the_single_process_run(gpu, tmp_path):
    """An uneven split (the package's rank slices give farmer 3 as 1 + 2 and farmer 193 as
    96 + 97).  ``applied`` equals the one-process run exactly and the two ranks' W_diff agree
    to the bit.  rho and W_diff are functions of x, x̄ and W, which differ between the runs in
    their last bits (the ranks' x̄ sum is taken in another order, and every later solve starts
    from that), so they are held to bounds computed from the runs' own recorded x, x̄ and W:

    * rho is a convex combination (order statistic in [0, 1]) of the mean, minimum and maximum
      of |cost| / d_s with the same cost, so its relative change is at most the largest relative
      change of a scenario's denominator d_s between the two runs at the rewrite, plus the
      2e-12 of two sums against the restatement;
    * W_diff at an iteration changes by at most the mean |W - W'| at that iteration plus that
      of the one before, plus 1e-12 of its value for the order of the sum."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / f"gr_r{k}.json")) for k in range(2)]
    for case in ("farmer3", "farmer193"):
        c = G.CASES[case]
        S = int(case[6:])
        one = _traced_run(case)
        assert set(one["applied"]) == c["applied"] and one["spec"]
        assert r[0][case]["names"] + r[1][case]["names"] == [f"scen{i}" for i in range(S)]
        assert sorted(len(r[k][case]["names"]) for k in range(2)) == [S // 2, (S + 1) // 2]
        # the ranks' recorded x, x̄, W of all scenarios, per iteration
        both = {int(it): [np.concatenate([np.array(r[k][case]["trace"][it][j]) for k in range(2)]) for j in range(3)]
                for it in r[0][case]["trace"]}
        last = max(c["applied"])
        d1, d2 = _scenario_denom(*one["trace"][last][:2]), _scenario_denom(*both[last][:2])
        rho_tol = float((np.abs(d1 - d2) / np.minimum(d1, d2)).max()) + 2e-12
        wd_tol = np.zeros(c["iters"] + 1)                    # entry 0: post_iter0, W = 0 in both runs
        dW = {0: 0.0, **{it: float(np.abs(both[it][2] - one["trace"][it][2]).mean()) for it in both}}
        for it in range(1, c["iters"] + 1):
            wd_tol[it] = dW[it] + dW[it - 1] + 1e-12 * one["wd"][it]
        lo = 0
        for k in range(2):
            q = r[k][case]
            n = len(q["names"])
            assert q["applied"] == one["applied"] and q["spec"], (case, k, q["applied"])
            err = np.abs(np.array(q["rho"]) / one["rho"][lo:lo + n] - 1).max()
            werr = np.abs(np.array(q["wd"]) - one["wd"])
            print(case, "rank", k, "rho rel err", err, "bound", rho_tol, "W_diff abs err", werr.max(), "bound",
                  wd_tol.max())
            assert err <= rho_tol and (werr <= wd_tol).all(), (werr, wd_tol)
            assert q["calls"]["allreduce_wdiff"] == c["iters"] + 1, q["calls"]
            assert q["calls"]["allreduce_ratio_sum"] == q["calls"]["allreduce_ratio_max"] == c["iters"], q["calls"]
            lo += n
        assert r[0][case]["wd"] == r[1][case]["wd"]                    # the ranks agree to the bit


# ------------------------------------------------------------------ MultRhoUpdater, cfg_vanilla
def test_mult_rho_updater_against_the_restatement(gpu):
    from mpisppy_amd.extensions.mult_rho_updater import MultRhoUpdater
    iters = 6
    ph = _ph("farmer3", iters, ext=_recording(MultRhoUpdater))
    ph.ph_main(finalize=False)
    assert not ph._speculate(True)                     # a host miditer: the plain loop
    g = G.GradStepped(N.make("farmer3"), G.FARMER_COST, 0.5)
    g.iter0()
    ref = G.MultRho(g.o.rho)
    log = g.run(iters, mult=ref)
    print("acted", ph.extobject.acted, "restatement", ref.acted)
    print("conv", [r["conv"] for r in ph.extobject.rec], "restatement", [r["conv"] for r in log])
    assert ph.extobject.acted == ref.acted and len(ref.acted) >= 1
    upto = ref.acted[0]                                # the second new best conv (the first attaches)
    for r, o in zip(ph.extobject.rec, log):
        if r["iter"] <= upto:
            print("iter", r["iter"], "rho rel err", np.abs(r["rho"] / o["rho"] - 1).max())
            np.testing.assert_allclose(r["rho"], o["rho"], rtol=1e-9, atol=0)
    ph.engine.close()


def test_cfg_vanilla_helpers_build_hubs_that_run(gpu):
    from types import SimpleNamespace
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.extensions.gradient_extension import Gradient_extension
    from mpisppy_amd.extensions.mult_rho_updater import MultRhoUpdater
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    names = farmer.scenario_names_creator(3)
    for flag, adder, cls in (({"grad_rho_setter": True, "order_stat": 0.4}, vanilla.add_gradient_rho, Gradient_extension),
                             ({"mult_rho": True, "mult_rho_update_start_iteration": 2}, vanilla.add_mult_rho_updater,
                              MultRhoUpdater)):
        cfg = SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=12, device="cuda:0",
                              toc=False, intra_hub_conv_thresh=-1.0, **flag)
        hub = vanilla.ph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs={"num_scens": 3})
        plain = {k: v for k, v in hub["opt_kwargs"].items()}
        assert adder(vanilla.ph_hub(cfg, farmer.scenario_creator, None, names), SimpleNamespace())["opt_kwargs"][
            "extensions"] is None                                   # no flag: nothing changes
        hub = adder(hub, cfg)
        assert hub["opt_kwargs"]["extensions"] is cls and plain["extensions"] is None
        ws = WheelSpinner(hub, [])
        ws.spin()
        ph = ws.spcomm.opt
        assert ph._PHIter == 12 and isinstance(ph.extobject, cls)
        if cls is Gradient_extension:
            assert ph.options["gradient_extension_options"]["order_stat"] == 0.4
            assert set(ph.extobject.rho_update_iterations()) == {4, 11}
        else:
            assert ph.options["mult_rho_options"] == {"rho_update_start_iteration": 2} and ph.extobject.acted
        ph.engine.close()

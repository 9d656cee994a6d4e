"""FWPH on the device (phgpu_fwph_*, include/phgpu.h; mpisppy_amd/fwph/fwph.py) against the
numpy restatement of mpisppy/fwph/fwph.py in tests/fwph_ref.py.

* the passes alone on constructed stores (farmer S = 130: three waves, the last ragged;
  aircond [4, 3, 2]: waves span nodes; the same batch on a shared-matrix handle): K = 1,
  K = nn + 2, a repeated column, a full store, rho differing per nonant, optima that are one
  column and optima inside a face, inactive scenarios, a status that is not OPTIMAL.  xq and phi
  against the restatement's QP at 1e-5 absolute + 1e-5 relative (the project's standing
  tolerances); a >= 0, |sum a - 1| <= 1e-12; Gamma, dual_bound and the counts against numpy;
  the QP's own gap at most 10 times the restatement's (floor 1e-12 max(1, |objective|));
* FWPH end to end against the recorded trajectories tests/test_fwph.py admits: bound and diff
  at 1e-5 relative, x̄ and W at 1e-5 absolute, column and inner iteration counts exactly;
* properties on farmer S = 130 with FW_max_columns 4 and on aircond [4, 3, 2]: weak duality
  against Xhat_Eval at FWPH's own x̄, the cap, the same bits twice;
* two gloo ranks on one GPU, a wheel with the spoke, a maximisation model.
"""
import json
import os
import socket

import numpy as np
import pytest
import torch

import fwph_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REL = 1e-5
ABS = 1e-5
TAU, SCT = 1e-4, 1e-4
FARMER_EF_OBJ = -108390.0
AIR_KW = {"start_seed": 1134}


# ------------------------------------------------------------------ the passes alone
def _engine(model):
    from mpisppy_amd.engine import PHEngine
    from mpisppy_amd.examples import aircond, farmer
    if model == "farmer":
        b = farmer.batch_creator(farmer.scenario_names_creator(130), crops_multiplier=1, num_scens=130)
    else:
        b = aircond.batch_creator(aircond.scenario_names_creator(24), branching_factors=[4, 3, 2], **AIR_KW)
    return PHEngine(b, device="cuda:0", shared=True if model == "aircond_shared" else None)


def _put(t, a):
    t[:a.shape[0]].copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=t.dtype, device=t.device))


def _state(e, K, kind, rng):
    """K columns per scenario [K, nn, S] with costs, and W, rho (differing per nonant), x̄."""
    nn, S = e.nn, e.S
    X = rng.integers(0, 6, size=(K, nn, S)).astype(float) * 50.0 + rng.integers(0, 3, size=(K, 1, S)) * 7.0
    f = -rng.random((K, S)) * 1e5
    if kind == "repeat":                      # column 2 repeats column 0, cost and all
        X[2], f[2] = X[0], f[0]
    W = rng.normal(size=(nn, S)) * 20.0
    rho = (0.5 + 0.25 * np.arange(nn))[:, None] * np.ones((1, S))
    xbar = rng.random((nn, S)) * 200.0
    return X, f, W, rho, xbar


def _expected(X, f, a_prev, newest, xnew, fnew, W, rho, xbar, max_cols):
    """The restatement's column step of one scenario: (columns, costs, a, xq, phi, slot)."""
    X, f = [c for c in X], list(f)
    if len(X) < max_cols:
        X.append(xnew)
        f.append(fnew)
        slot = len(X) - 1
    else:
        a = a_prev.copy()
        a[newest] = np.inf
        slot = int(np.argmin(a))
        X[slot], f[slot] = xnew, fnew
    X, f = np.array(X), np.array(f)
    a, xq, phi = R.solve_column_qp(X, f, W, rho, xbar)
    return X, f, a, xq, phi, slot


CASES = [("k1", 1, 4), ("knn2", None, None), ("repeat", 3, 8), ("full", 4, 4)]
GAPS = {}


@pytest.mark.parametrize("model", ["farmer", "aircond", "aircond_shared"])
def test_passes_against_the_restatement(gpu, model):
    from mpisppy_amd import _lib
    e = _engine(model)
    nn, S = e.nn, e.S
    cols = np.asarray(e.batch.nonant_col)
    prm = _lib.FwphParams(TAU, SCT)
    worst = (0.0, 0.0)
    try:
        for ci, (kind, K, mc) in enumerate(CASES):
            rng = np.random.default_rng(100 + ci)
            if kind == "knn2":
                K, mc = nn + 1, nn + 3
            assert mc <= 64
            X, f, W, rho, xbar = _state(e, K, kind, rng)
            a0 = None
            if kind == "full":
                # even scenarios: a tie for the least weight, the lowest index goes; odd ones: the
                # newest column (the last loaded) has the least weight and stays
                a0 = np.where(np.arange(S)[None, :] % 2 == 0, np.array([0.3, 0.0, 0.0, 0.7])[:, None],
                              np.array([0.5, 0.3, 0.2, 0.0])[:, None])
            e.fwph_init(mc)
            assert e.workspace_bytes() >= 8 * S * (mc * (nn + 5) + mc * (mc + 1))
            _put(e.W, W), _put(e.rho, rho), _put(e.xbar, xbar)
            e.fwph_load(torch.as_tensor(X), torch.as_tensor(f), None if a0 is None else torch.as_tensor(a0))
            a_prev = a0 if a0 is not None else np.vstack([np.ones((1, S)), np.zeros((K - 1, S))])
            st0 = e.fwph_export()
            xq0, phi0 = np.einsum("ks,kns->ns", a_prev, X), (a_prev * f).sum(0)
            assert np.abs(st0["xq"] - xq0).max() <= 1e-9 and np.abs(st0["phi"] - phi0).max() <= 1e-9 * 1e5
            assert (st0["ncols"] == K).all() and (st0["active"] == 1).all() and (st0["nit"] == 0).all()
            # -- pass 1 (t0): What by the direction pass, a crafted "last solve"
            alpha = 0.25
            e.fwph_direction(True, alpha)
            What = W + rho * ((1 - alpha) * xbar + alpha * xq0 - xbar)
            assert np.abs(e.fw_What.cpu().numpy()[:nn] - What).max() <= 1e-10
            xnew = rng.integers(0, 6, size=(nn, S)).astype(float) * 50.0 + 3.0
            if kind == "repeat":
                xnew[:, ::3] = X[1][:, ::3]                     # the LP returns a point it returned before
            fnew = -rng.random(S) * 1e5
            fnew[::4] -= 1e7                                    # an optimum that is this one column
            val1 = phi0 + (What * xq0).sum(0)
            val0 = fnew + (What * xnew).sum(0)
            s5 = np.arange(S) % 5
            val0 = np.where(s5 == 0, val1 - 1e-6 * np.abs(val1), val0)      # Gamma ~ 1e-6 < tau: done
            val0 = np.where(s5 == 1, val1 + 1e-3 * np.abs(val1), val0)      # Gamma ~ -1e-3 < -stop_check_tol
            fnew = val0 - (What * xnew).sum(0)
            status = np.where(np.arange(S) % 7 == 3, 1, 0).astype(np.int32)
            bound = val0 - rng.random(S)
            gam = np.where(np.abs(val0) > 1e-9, (val1 - val0) / np.abs(val0), val1 - val0)
            assert np.abs(gam - TAU).min() > 1e-7 and np.abs(gam + SCT).min() > 1e-7    # no count rounding decides
            e.x.zero_()
            e.x[torch.as_tensor(cols, device=e.device)] = torch.as_tensor(xnew, device=e.device)
            _put(e.obj, val0), _put(e.bound, bound), _put(e.status, status)
            sent = -777.0
            e.fw_gamma.fill_(sent), e.fw_dual_bound.fill_(sent), e.fw_ncols.fill_(-7)
            e.fw_xq.fill_(sent), e.fw_xqx.fill_(sent)
            e.fwph_column(prm, True)
            opt = status == 0
            cnt = e.fwph_counts()
            assert cnt == (int((opt & ~(gam < TAU)).sum()), int((opt & (gam < -SCT)).sum()), int((~opt).sum())), cnt
            st1 = e.fwph_export()
            g1, db1 = e.fw_gamma.cpu().numpy(), e.fw_dual_bound.cpu().numpy()
            xq1, xqx1, nc1 = e.fw_xq.cpu().numpy()[:nn], e.fw_xqx.cpu().numpy(), e.fw_ncols.cpu().numpy()
            assert np.array_equal(db1, bound)                   # every scenario was active at t0
            assert np.abs(g1[opt] - gam[opt]).max() <= 1e-12 + 1e-9 * np.abs(gam[opt]).max()
            # a status that is not OPTIMAL: nothing added, the QP point kept, inactive from here
            assert (g1[~opt] == sent).all() and (nc1[~opt] == -7).all() and (xq1[:, ~opt] == sent).all()
            for k in ("X", "f", "a", "ncols", "xq", "phi", "nit"):
                assert np.array_equal(st1[k][..., ~opt], st0[k][..., ~opt]), k
            assert (st1["active"][~opt] == 0).all()
            assert np.array_equal(st1["active"][opt], (~(gam < TAU)).astype(np.int32)[opt])
            assert (st1["nit"][opt] == 1).all() and (nc1[opt] == min(K + 1, mc)).all()
            single = inside = 0
            for s in np.nonzero(opt)[0]:
                Xe, fe, ae, xqe, phie, slot = _expected(X[:, :, s], f[:, s], a_prev[:, s], K - 1, xnew[:, s], fnew[s],
                                                        W[:, s], rho[:, s], xbar[:, s], mc)
                Kn = len(fe)
                assert np.array_equal(st1["X"][:Kn, :, s], Xe), (kind, s, slot)      # the slot, the replacement rule
                assert np.abs(st1["f"][:Kn, s] - fe).max() <= 1e-9 * np.abs(fe).max()
                a = st1["a"][:Kn, s]
                assert a.min() >= 0.0 and abs(a.sum() - 1.0) <= 1e-12, (kind, s, a)
                assert (st1["a"][Kn:, s] == 0).all()
                assert np.abs(xq1[:, s] - xqe).max() <= ABS + REL * np.abs(xqe).max(), (kind, s, xq1[:, s], xqe)
                assert abs(st1["phi"][s] - phie) <= ABS + REL * abs(phie), (kind, s)
                assert np.array_equal(xq1[:, s], st1["xq"][:, s]) and np.array_equal(xqx1[cols, s], xq1[:, s])
                gd = R.qp_gap(Xe, st1["f"][:Kn, s], W[:, s], rho[:, s], xbar[:, s], a)
                gr = R.qp_gap(Xe, st1["f"][:Kn, s], W[:, s], rho[:, s], xbar[:, s], ae)
                floor = 1e-12 * max(1.0, abs(R.qp_objective(Xe, st1["f"][:Kn, s], W[:, s], rho[:, s], xbar[:, s], a)))
                assert gd <= max(10.0 * gr, floor), (kind, s, gd, gr, floor)
                worst = max(worst, (gd, gr))
                single += int((a > 0).sum() == 1)
                inside += int((a > 0).sum() >= 2)
            assert single > 0 and inside > 0, (kind, single, inside)
            if kind == "full":
                ev, od = np.nonzero(opt & (np.arange(S) % 2 == 0))[0], np.nonzero(opt & (np.arange(S) % 2 == 1))[0]
                assert np.array_equal(st1["X"][1][:, ev], xnew[:, ev]) and np.array_equal(st1["X"][2][:, od], xnew[:, od])
            # -- pass 2 (not t0): the inactive scenarios are untouched, dual_bound is not rewritten
            e.fwph_direction(False, alpha)
            assert np.abs(e.fw_What.cpu().numpy()[:nn] - (W + rho * (st1["xq"] - xbar))).max() <= 1e-9
            act = st1["active"] == 1
            _put(e.bound, bound + 5.0), _put(e.status, np.zeros(S, dtype=np.int32))
            e.fwph_column(prm, False)
            cnt2 = e.fwph_counts()
            st2 = e.fwph_export()
            assert cnt2[2] == 0 and cnt2[0] <= int(act.sum())
            assert np.array_equal(e.fw_dual_bound.cpu().numpy(), bound)
            for k in ("X", "f", "a", "ncols", "xq", "phi", "nit", "active"):
                assert np.array_equal(st2[k][..., ~act], st1[k][..., ~act]), k
            assert np.array_equal(e.fw_gamma.cpu().numpy()[~act], g1[~act])
            assert (st2["nit"][act] == 2).all()
            # -- the diff reduction: the same bits twice, the value against numpy
            d1 = float(e.fwph_diff().item())
            d2 = float(e.fwph_diff().item())
            ref = float((e.batch.prob.reshape(-1) * ((st2["xq"] - xbar) ** 2).sum(0)).sum())
            assert d1 == d2 and abs(d1 - ref) <= 1e-12 * abs(ref)
        GAPS[model] = worst
        print(f"{model}: largest QP gap on the device {worst[0]:.2e} (the restatement's there {worst[1]:.2e})")
    finally:
        e.close()


def test_store_lifetime(gpu):
    """The store is the handle's: counted from phgpu_fwph_init on, resized by another init."""
    from mpisppy_amd import _lib
    e = _engine("farmer")
    try:
        with pytest.raises(_lib.PhgpuError, match="phgpu_fwph_init has not run"):
            _lib.check(e.lib.phgpu_fwph_diff(e.h, None, None, None), "phgpu_fwph_diff")
        b0 = e.workspace_bytes()
        for bad in (1, 65):
            with pytest.raises(_lib.PhgpuError, match=r"not in \[2, 64\]"):
                e.fwph_init(bad)
        e.fwph_init(8)
        b8 = e.workspace_bytes()
        per = lambda mc: 8 * (mc * (e.nn + 5) + mc * (mc + 1) + e.nn + 1) + 16     # noqa: E731
        assert b8 - b0 == e.S * per(8) + 16
        e.fwph_init(8)
        assert e.workspace_bytes() == b8
        e.fwph_init(64)
        assert e.workspace_bytes() - b0 == e.S * per(64) + 16
    finally:
        e.close()


# ------------------------------------------------------------------ FWPH end to end
def _fwph(S=3, mpicomm=None, sense=1, iters=50, model="farmer", **fw):
    from mpisppy_amd.examples import aircond, farmer
    from mpisppy_amd.fwph.fwph import FWPH
    ph_options = {"solver_name": "mi355x_pdhg", "PHIterLimit": iters, "defaultPHrho": 1.0, "convthresh": 0.0,
                  "verbose": False, "display_progress": False, "toc": False, "device": "cuda:0"}
    fw_options = {"FW_iter_limit": 3, "FW_weight": 0.0, "FW_conv_thresh": TAU, "solver_name": "mi355x_pdhg",
                  "FW_verbose": False}
    fw_options.update(fw)
    if model == "farmer":
        return FWPH(ph_options, fw_options, farmer.scenario_names_creator(S), farmer.scenario_creator,
                    scenario_creator_kwargs={"num_scens": S, "sense": sense}, mpicomm=mpicomm)
    from oracle.models import create_nodenames_from_branching_factors
    bfs = [4, 3, 2]
    return FWPH(ph_options, fw_options, aircond.scenario_names_creator(24), aircond.scenario_creator,
                scenario_creator_kwargs={"branching_factors": bfs, **AIR_KW},
                all_nodenames=create_nodenames_from_branching_factors(bfs), mpicomm=mpicomm)


def _run(opt, iters):
    """fw_prep and ``iters`` outer iterations: what the parity tests compare, per iteration."""
    best = opt.fw_prep()
    out = {"trivial": best, "iters": []}
    e = opt.engine
    for itr in range(iters):
        best, stop = opt.fw_step(itr, best)
        st = e.fwph_export()
        out["iters"].append({"bound": opt._local_bound, "diff": opt.fw_last_diff,
                             "xbar": e.host("xbar")[:, :e.nn].copy(), "W": e.host("W")[:, :e.nn].copy(),
                             "ncols": st["ncols"].tolist(), "nit": st["nit"].tolist(),
                             "node_xbar": {k: v.tolist() for k, v in opt.xbar_by_node().items()}})
        assert not stop
    return out


def _compare(got, fx, lo=0, hi=None):
    assert abs(got["trivial"] - fx["trivial"]) <= REL * abs(fx["trivial"])
    for it, (o, g) in enumerate(zip(got["iters"], fx["iters"])):
        sl = slice(lo, hi)
        print(f"iteration {it + 1}: bound {o['bound']:.6f} ({g['bound']:.6f}) diff {o['diff']:.6e} ({g['diff']:.6e}) "
              f"max|xbar - ref| {np.abs(o['xbar'] - np.array(g['xbar'])[sl]).max():.2e} "
              f"max|W - ref| {np.abs(o['W'] - np.array(g['W'])[sl]).max():.2e}")
        assert abs(o["bound"] - g["bound"]) <= REL * abs(g["bound"]), it
        assert abs(o["diff"] - g["diff"]) <= REL * abs(g["diff"]), it
        assert np.abs(o["xbar"] - np.array(g["xbar"])[sl]).max() <= ABS, it
        assert np.abs(o["W"] - np.array(g["W"])[sl]).max() <= ABS, it
        assert o["ncols"] == g["ncols"][sl] and o["nit"] == g["nit"][sl], (it, o["ncols"], g["ncols"], o["nit"], g["nit"])


@pytest.mark.parametrize("name", sorted(R.TRAJECTORIES))
def test_fwph_matches_the_recorded_trajectory(gpu, name):
    fx = json.load(open(os.path.join(HERE, "golden", f"fwph_{name}.json")))
    cfg = R.TRAJECTORIES[name]
    opt = _fwph(S=cfg["S"], FW_weight=cfg["alpha"], FW_iter_limit=cfg["iter_limit"])
    try:
        got = _run(opt, cfg["iters"])
        _compare(got, fx)
        # nothing is read back per scenario: one column pass per LP solve launch, no status copies
        assert opt.engine.calls["fwph_column"] == sum(opt.fw_inner_iters) == opt.engine.calls["fwph_direction"]
        assert opt.fw_gamma_warnings == 0
    finally:
        opt.engine.close()


@pytest.mark.parametrize("model", ["farmer", "aircond"])
def test_bounds_are_outer_bounds_and_runs_repeat(gpu, model):
    """Weak duality: every reported bound is at most the expected objective of FWPH's own x̄
    (Xhat_Eval), up to the solve tolerance; the store never exceeds its cap; a second run gives
    the same bits."""
    from mpisppy_amd.utils.xhat_eval import Xhat_Eval
    cap = 4 if model == "farmer" else 32
    runs = []
    for _ in range(2):
        opt = _fwph(S=130, model=model, FW_max_columns=cap, FW_weight=0.5)
        try:
            runs.append(_run(opt, 6))
            kw = dict(all_scenario_names=opt.all_scenario_names, scenario_creator=opt.scenario_creator,
                      scenario_creator_kwargs=opt.scenario_creator_kwargs, all_nodenames=opt.all_nodenames)
        finally:
            opt.engine.close()
    a, b = runs
    for o, p in zip(a["iters"], b["iters"]):
        assert o["bound"] == p["bound"] and o["diff"] == p["diff"] and o["ncols"] == p["ncols"]
        assert np.array_equal(o["W"], p["W"]) and np.array_equal(o["xbar"], p["xbar"])
        assert max(o["ncols"]) <= cap
    if model == "farmer":
        assert max(a["iters"][-1]["ncols"]) == cap              # the replacement rule was at work
    ev = Xhat_Eval({"solver_name": "mi355x_pdhg", "device": "cuda:0", "toc": False, "verbose": False}, **kw)
    try:
        for it in (0, 2, 5):
            cache = {nd: np.array(v) for nd, v in a["iters"][it]["node_xbar"].items()}
            inner = ev.evaluate(cache)
            assert inner is not None
            # (an outer iteration with an LP that was not OPTIMAL reports no bound)
            bounds = [o["bound"] for o in a["iters"] if o["bound"] is not None]
            assert len(bounds) >= 4, [o["bound"] for o in a["iters"]]
            print(f"{model}: inner bound at the x̄ of iteration {it + 1}: {inner:.4f}; best of {len(bounds)} outer "
                  f"bounds {max(bounds):.4f}")
            for bd in bounds:
                assert bd <= inner + REL * abs(inner), (it, bd, inner)
            assert a["trivial"] <= inner + REL * abs(inner)
    finally:
        ev.engine.close()


def test_a_maximisation_model_reports_sense_times_the_bound(gpu):
    fx = json.load(open(os.path.join(HERE, "golden", "fwph_farmer3.json")))
    opt = _fwph(S=3, sense=-1, FW_weight=1.0)
    try:
        got = _run(opt, 3)
        assert not opt.is_minimizing
        assert abs(got["trivial"] + fx["trivial"]) <= REL * abs(fx["trivial"])
        for o, g in zip(got["iters"], fx["iters"]):
            assert abs(o["bound"] + g["bound"]) <= REL * abs(g["bound"])
            assert o["bound"] >= -FARMER_EF_OBJ * (1 - REL)      # an upper bound of the maximum
    finally:
        opt.engine.close()


def test_an_lp_that_is_not_optimal_reports_no_bound(gpu):
    """Solves that end at the iteration limit: no scenario adds a column, the outer iteration
    reports no bound (the spoke keeps its previous one)."""
    opt = _fwph(S=3, FW_weight=1.0)
    try:
        best = opt.fw_prep()
        solve = opt.solve_loop

        def at_the_limit(*a, **k):
            solve(*a, **k)
            opt.engine.status.fill_(1)          # PHGPU_ITER_LIMIT
        opt.solve_loop = at_the_limit
        st0 = opt.engine.fwph_export()
        best2, stop = opt.fw_step(0, best)
        st1 = opt.engine.fwph_export()
        assert opt._local_bound is None and best2 == best and not stop and opt.fw_not_optimal == (3, 3)
        assert opt.fw_inner_iters == [1]                         # the active count reached 0 at once
        assert np.array_equal(st1["ncols"], st0["ncols"]) and np.array_equal(st1["xq"], st0["xq"])
    finally:
        opt.engine.close()


def test_a_later_lp_that_is_not_optimal_costs_a_column_not_the_bound(gpu):
    """The bound is made of the t = 0 LPs: scenario 0 ends its second LP at the iteration limit,
    keeps the column of its first and its QP point, and the iteration reports the trajectory's
    bound."""
    fx = json.load(open(os.path.join(HERE, "golden", "fwph_farmer3.json")))
    opt = _fwph(S=3, FW_weight=1.0)
    try:
        best = opt.fw_prep()
        solve = opt.solve_loop
        calls = []

        def second_at_the_limit(*a, **k):
            solve(*a, **k)
            calls.append(1)
            if len(calls) == 2:
                opt.engine.status[0] = 1
        opt.solve_loop = second_at_the_limit
        opt.fw_step(0, best)
        st = opt.engine.fwph_export()
        assert abs(opt._local_bound - fx["iters"][0]["bound"]) <= REL * abs(fx["iters"][0]["bound"])
        assert opt.fw_not_optimal == (1, 0)
        assert st["ncols"].tolist() == [2] + fx["iters"][0]["ncols"][1:] and st["nit"][0] == 1
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
        cfg = R.TRAJECTORIES["farmer12"]
        opt = _fwph(S=12, mpicomm=Comm(), FW_weight=cfg["alpha"])
        got = _run(opt, cfg["iters"])
        for o in got["iters"]:
            o["xbar"], o["W"] = o["xbar"].tolist(), o["W"].tolist()
        got["names"] = list(opt.local_scenario_names)
        opt.engine.close()
        with open(os.path.join(out_dir, f"fw_r{rank}.json"), "w") as f:
            json.dump(got, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_give_the_one_rank_trajectory(gpu, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    fx = json.load(open(os.path.join(HERE, "golden", "fwph_farmer12.json")))
    lo = 0
    for k in range(2):
        r = json.load(open(tmp_path / f"fw_r{k}.json"))
        n = len(r["names"])
        assert n == 6
        for o in r["iters"]:
            o["xbar"], o["W"] = np.array(o["xbar"]), np.array(o["W"])
        _compare(r, fx, lo, lo + n)
        lo += n


# ------------------------------------------------------------------ a wheel
def test_wheel_with_the_fwph_spoke(gpu):
    """PH hub + fwph_spoke + xhatshuffle_spoke on farmer 3 scenarios: the hub's outer bound comes
    from 'F', and outer <= EF optimum <= inner at termination."""
    from types import SimpleNamespace
    from mpisppy_amd.cylinders.fwph_spoke import FrankWolfeOuterBound
    from mpisppy_amd.examples import farmer
    from mpisppy_amd.spin_the_wheel import WheelSpinner
    from mpisppy_amd.utils import cfg_vanilla as vanilla
    names = farmer.scenario_names_creator(3)
    cfg = SimpleNamespace(solver_name="mi355x_pdhg", default_rho=1.0, max_iterations=14, rel_gap=1e-6,
                          intra_hub_conv_thresh=-1.0, device="cuda:0", toc=False, fwph_iter_limit=3, fwph_weight=1.0,
                          fwph_conv_thresh=TAU, fwph_stop_check_tol=SCT)
    kw = {"num_scens": 3}
    hub = vanilla.ph_hub(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)
    spokes = [vanilla.fwph_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw),
              vanilla.xhatshuffle_spoke(cfg, farmer.scenario_creator, None, names, scenario_creator_kwargs=kw)]
    ws = WheelSpinner(hub, spokes)
    ws.spin(placement="colocated")
    h = ws.spcomm
    try:
        fw = ws.spokes[0]
        assert isinstance(fw, FrankWolfeOuterBound) and h.outerbound_spoke_chars == {1: "F"}
        assert h.bounds_only_indices == {1} and fw._itr >= 6
        assert h.last_ob_idx == 1                                    # the best outer bound is the spoke's
        assert ws.BestOuterBound > h.opt.trivial_bound + 1000.0      # (trivial: -115405.56)
        assert ws.BestOuterBound == pytest.approx(max(fw._best, h.opt.trivial_bound), rel=1e-12)
        assert ws.BestOuterBound <= FARMER_EF_OBJ + REL * abs(FARMER_EF_OBJ)
        assert ws.BestInnerBound >= FARMER_EF_OBJ - REL * abs(FARMER_EF_OBJ)
        assert fw.final_bound == fw.bound == fw.opt._local_bound
    finally:
        for s in ws.spokes:
            s.opt.engine.close()
        h.opt.engine.close()
